"""Plain numpy restatement of the LSS chain (cora/signal/lssutil.py: diff2, calculate_width, exponential_FoG_kernel,
lognormal_transform; cora/signal/lss.py: the bias, linear-dynamics, Fingers-of-God and map steps) in the reference's
operation order, for the tests of csrc/lsschain.hip.  tests/test_lsschain_host.py pins it to the goldens."""
import numpy as np


def diff2(f, x, axis=-1):
    """Second derivative on a non-uniform grid along ``axis``; rows 2 .. N-2 three-point (sum built term by term as
    alpha f[i-2], + beta f[i-1], - (alpha + beta + gamma) f[i], + gamma f[i+1]), rows 0, 1, N-1 one-sided 4-point."""
    f = np.moveaxis(np.asarray(f, dtype=np.float64), axis, 0)
    x = np.asarray(x, dtype=np.float64)
    N = f.shape[0]
    d2 = np.zeros_like(f)
    for i in range(2, N - 1):
        dm2, dm1, dp1 = x[i] - x[i - 2], x[i] - x[i - 1], x[i + 1] - x[i]
        al = 2 * (dp1 - dm1) / (dm2 * (dm2 + dp1) * (dm2 - dm1))
        be = 2 * (dm2 - dp1) / (dm1 * (dm2 - dm1) * (dm1 + dp1))
        ga = 2 * (dm2 + dm1) / (dp1 * (dm1 + dp1) * (dm2 + dp1))
        row = al * f[i - 2]
        row = row + be * f[i - 1]
        row = row - (al + be + ga) * f[i]
        d2[i] = row + ga * f[i + 1]

    def four(w, rows):
        return ((w[0] * f[rows[0]] + w[1] * f[rows[1]]) + w[2] * f[rows[2]]) + w[3] * f[rows[3]]

    p1, p2, p3 = x[1] - x[0], x[2] - x[0], x[3] - x[0]
    d2[0] = four((2 * (p1 + p2 + p3) / (p1 * p2 * p3), -2 * (p2 + p3) / (p1 * (p1 - p2) * (p1 - p3)),
                  2 * (p1 + p3) / ((p1 - p2) * p2 * (p2 - p3)), 2 * (p1 + p2) / ((p1 - p3) * p3 * (-p2 + p3))),
                 (0, 1, 2, 3))
    m1, p1, p2 = x[1] - x[0], x[2] - x[1], x[3] - x[1]
    d2[1] = four((2 * (p1 + p2) / (m1 * (m1 + p1) * (m1 + p2)), 2 * (m1 - p1 - p2) / (m1 * p1 * p2),
                  2 * (m1 - p2) / (p1 * (m1 + p1) * (p1 - p2)), -2 * (m1 - p1) / ((p1 - p2) * p2 * (m1 + p2))),
                 (0, 1, 2, 3))
    m1, m2, m3 = x[-1] - x[-2], x[-1] - x[-3], x[-1] - x[-4]
    d2[N - 1] = four((2 * (m1 + m2) / ((m1 - m3) * m3 * (-m2 + m3)), 2 * (m1 + m3) / ((m1 - m2) * m2 * (m2 - m3)),
                      -2 * (m2 + m3) / (m1 * (m1 - m2) * (m1 - m3)), 2 * (m1 + m2 + m3) / (m1 * m2 * m3)),
                     (N - 4, N - 3, N - 2, N - 1))
    return np.ascontiguousarray(np.moveaxis(d2, 0, axis))


def calculate_width(centres):
    c = np.asarray(centres, dtype=np.float64)
    w = np.zeros(len(c))
    w[1:-1] = (c[2:] - c[:-2]) / 2.0
    w[0] = 2 * (c[1] - (w[1] / 2.0) - c[0])
    w[-1] = 2 * (c[-1] - (w[-2] / 2.0) - c[-2])
    return np.abs(w)


def exponential_FoG_kernel(chi, sigmaP, D):
    chi = np.asarray(chi, dtype=np.float64)
    sigmaP = sigmaP if isinstance(sigmaP, np.ndarray) else np.ones_like(chi) * sigmaP
    D = D if isinstance(D, np.ndarray) else np.ones_like(chi) * D
    ar = (2**0.5 / sigmaP)[:, None]
    dchi = calculate_width(chi)[None, :]
    sep = np.abs(chi[:, None] - chi[None, :])
    K = np.exp(-ar * sep) * (np.sinh(ar * dchi / 2.0) / (ar * dchi / 2.0))
    np.fill_diagonal(K, np.diagonal(np.exp(-ar * dchi / 4) * (np.sinh(ar * dchi / 4) / (ar * dchi / 4))))
    K /= np.sum(K, axis=1)[:, None]
    K /= D[None, :]
    K *= D[:, None]
    return K


def lognormal_transform(field, axis=None):
    out = np.array(field, dtype=np.float64)
    out -= field.var(axis=axis, keepdims=True) / 2.0
    np.exp(out, out=out)
    out -= 1
    return out


def biased_field(delta, D, b1=None, b2=None, lognormal=False, lightcone=True):
    out = np.zeros_like(delta)
    if b1 is not None:
        out += (D * b1)[:, None] * delta
    if b2 is not None:
        d2m = (delta**2).mean(axis=1)[:, None]
        out += (D**2 * b2)[:, None] * (delta**2 - d2m)
    if lognormal:
        out = lognormal_transform(out, axis=1 if lightcone else None)
    return out


def linear_dynamics(phi, delta, delta_bias, chi, D, f=None):
    out = np.array(delta_bias, dtype=np.float64)
    out += D[:, None] * delta
    if f is not None:
        v = diff2(phi, chi, axis=0)
        v *= -(D * f)[:, None]
        out += v
    return out


def fingers_of_god(field, chi, sigmaP, D=None, alpha_FoG=1.0):
    if alpha_FoG == 0.0:
        return field
    n = field.shape[0]
    K = exponential_FoG_kernel(chi, alpha_FoG * sigmaP, np.full(n, 1.0) if D is None else D)
    return np.matmul(K, field.reshape(n, -1)).reshape(field.shape)


def biased_lss_to_map(delta, lognormal=False, map_prefactor=1.0, T_b=None, polarisation=True):
    n, npix = delta.shape
    m = np.zeros((n, 4 if polarisation else 1, npix))
    m[:, 0] = lognormal_transform(delta, axis=1) if lognormal else delta
    if map_prefactor != 1:
        m *= map_prefactor
    if T_b is not None:
        m[:, 0] *= T_b[:, None]
    return m


def diff2_kernel_order(coef, first, f):
    """The stencil as csrc/lsschain.hip applies it: ((c0 w0 + c1 w1) + c2 w2) + c3 w3 over rows first[i] .. first[i] + 3."""
    out = np.zeros_like(f)
    for i in range(f.shape[0]):
        s = first[i]
        out[i] = ((coef[i, 0] * f[s] + coef[i, 1] * f[s + 1]) + coef[i, 2] * f[s + 2]) + coef[i, 3] * f[s + 3]
    return out
