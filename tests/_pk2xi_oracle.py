"""Host oracle of the P(k) -> xi(r) kernels (cora_amd/csrc/pk2xi.hip) and of ``corrfunc.ps_to_corr``: numpy
restatements that return the value AND a first-order bound on what the device may differ by.  CPU only.

eps = 2^-52; one rounding costs eps / 2.  No constant below was fitted to device output; the GPU tests print the observed
err / bound next to them.  Values are in ``numpy.longdouble`` where that is cheap (the Romberg sums, the phase); numpy has
no longdouble FFT, so the convolution is numpy.fft in double and its bound carries the oracle's own error as well.

Romberg (``sinc_romb``).  Sample i has class t = number of trailing zero bits of i; S_t is the class sum, e = (f_0 + f_K) / 2,
T_t = 2^t (e + sum_{s >= t} S_s) the trapezoid estimate at stride 2^t, and the 4^j table over T_k .. T_0 ends in
sum_t c_t T_t with the coefficients c_t of ``romb_coefficients`` (alternating in sign).  The effective weight of a sample of
class t is W = sum_{t' <= t} c_t' 2^t' >= 0; the bound uses Wabs = sum_{t' <= t} |c_t'| 2^t' >= W, which is what the
roundings of the separate estimates see.  Per sample, relative to |g_i|:
    argument  fl(ka r): eps / 2 relative in x, |x sinc'(x)| = |cos x - sinc x| <= 2                 1 eps
    sine      2 ulp (the documented bound of the device's double sin), / x (eps / 2), * g (eps / 2)    3 eps
A class sum is a thread's samples in sequence (at most K / 256 terms), one add in the lane, six shuffle adds, then up to k
adds of the running sum c: a path of D = max(K / 256, 1) + 7 + k additions, D eps / 2 relative to the absolute sum.  The
table: every entry is below 1.97 Tmax in magnitude (the product of (4^j + 1) / (4^j - 1)), each of the k steps on the path
to the result commits at most 2 eps of that; the last product with dlk eps / 2.
    bound = dlk eps [ (4.5 + D / 2) sum_i Wabs_i |g_i| + 4 k Tmax ],  Tmax = max_t 2^t (|e|abs + sum_{s >= t} sum_class |g|)

Phase (``fftlog_phase``).  theta = eta ln 2 + 2 [ (xw - 1/2) arg w + y (ln|w| - 1) + Im series - sum_j atan2(y, x + j) ],
w = x + n + i y, x = (mu + 1) / 2, y = eta / 2.  The device shifts by n = 16 and stops the series at w^-13: the first term
left out is B_16 / (240 w^15) < 2.6e-20 (TRUNC = 1e-19 for both sides of the factor 2).  The oracle shifts by 40 and adds
that term, in longdouble.  With M = |eta| ln 2 + 2 (|xw - 1/2| |arg| + |y| (|ln|w|| + 1) + |series| + sum |atan2|):
    eta = fl(fl(2 pi m) / L) with the double 2 pi: 1.5 eps relative, and |eta dtheta/deta| <= M        1.5 eps M
    every term: the function (atan2, log: 2 ulp) and its product                                      2.5 eps M
    the sums: four of full size (2 eps M), the 16 arctangents in sequence (8 eps of their absolute sum)
    bound_theta = eps (8 M + 8 sum |atan2|) + TRUNC;   |U_dev - U| <= bound_theta + 3 eps (sincos, 2 ulp a component)

Convolution (``logconv``).  In the 2-norm a radix-2-equivalent butterfly stage with rounded twiddles costs at most 4 eps
(complex product sqrt(5) eps / 2 + sum eps / 2 + twiddle 2 eps).  A power-of-two pass of length n has log2 n stages, a
Bluestein pass two transforms of length P < 4 n and three pointwise products: <= 2 log2 n + 7.  Two passes each way
(log2 N1 + log2 N2 = log2 N), the four-step twiddle each way, the product with U:
    stages <= 2 (2 log2 N + 14 + 1) + 1 = 4 log2 N + 31
and an element differs by no more than the 2-norm of the error: bound = 4 eps (4 log2 N + 31) ||f||_2 per element, i.e.
C eps log2(N) ||f||_2 with C = 16 + 124 / log2 N.  The oracle's own double transform (pocketfft, two transforms) is inside
the same count.

End to end.  The direct part as above.  A level of the FFTLog part: the convolution bound plus what the error of U does,
(2 / N) sum_m |F_m| bound_U_m, both times (2 pi)^-1.5 r^-1.5, plus 4 eps |xi| for f = P k^1.5, the flip and that factor;
the Richardson table is linear, result = sum_ii w_ii estimate_ii (``richardson_weights``: ||w||_1 = 5.0, 7.76, 8.19 for
3, 6, 9 levels at t = 2), so the level bounds add with |w_ii|, plus 3 eps per table step on sum |w_ii| |estimate_ii|.
"""
import os

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the oracle needs an extended-precision long double"
EPS = 2.0**-52
TRUNC = 1e-19
PI_LD = 4 * np.arctan(LD(1))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pk2xi_vectors.npz")

# B_2k / (2k (2k - 1)), k = 1 .. 8
STIRLING = [(1, 12), (-1, 360), (1, 1260), (-1, 1680), (1, 1188), (-691, 360360), (1, 156), (-3617, 122400)]


def load_golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------------
# Richardson / Romberg
# ---------------------------------------------------------------------------------------------------------------------
def richardson(estimates, t, base_pow=1, return_table=False):
    """The reference's table (corrfunc.py:19-69), restated."""
    k = len(estimates)
    table = []
    for row in range(k):
        new = [estimates[row]]
        for col in range(1, row + 1):
            n = col * base_pow
            new.append((t**n * new[col - 1] - table[row - 1][col - 1]) / (t**n - 1.0))
        table.append(new)
    return table if return_table else table[k - 1][k - 1]


def richardson_weights(n, t=2.0, base_pow=1):
    """w with richardson(estimates) = sum_i w_i estimates_i (longdouble)."""
    eye = np.eye(n, dtype=LD)
    return np.asarray(richardson([eye[i] for i in range(n)], LD(t), base_pow), dtype=LD)


def romb_coefficients(k, defect=None):
    """c[t], t = 0 .. k, with romb = sum_t c[t] T_t (T_t the trapezoid estimate at stride 2^t), longdouble."""
    four = LD(4) if defect != "pow4" else LD(2)
    eye = np.eye(k + 1, dtype=LD)
    prev = None
    for i in range(k + 1):                      # estimate i is T_{k - i}: coarsest first
        row = [eye[k - i]]
        for j in range(1, i + 1):
            row.append(row[j - 1] + (row[j - 1] - prev[j - 1]) / (four**j - 1))
        prev = row
    return prev[k]


def sample_classes(k):
    """Class (trailing zero bits) of the samples 0 .. 2^k; -1 for the two ends."""
    i = np.arange((1 << k) + 1)
    cls = np.full(i.size, -1)
    inner = i[1:-1]
    cls[1:-1] = np.log2(inner & -inner).astype(int)
    return cls


def romb_weights(k, defect=None):
    """(W, Wabs) per sample of the 2^k + 1: the effective Romberg weights and their absolute counterparts.
    defect: "class" (every class taken one too high), "half" (the end samples at full weight), "pow4" (2^j for 4^j)."""
    c = romb_coefficients(k, defect)
    p2 = LD(2) ** np.arange(k + 1)
    cum = np.cumsum(c * p2)                      # weight of class t: sum_{t' <= t} c_t' 2^t'
    cumabs = np.cumsum(np.abs(c) * p2)
    cls = sample_classes(k)
    use = np.minimum(cls + 1, k - 1) if defect == "class" else cls
    W = np.where(cls >= 0, cum[np.maximum(use, 0)], cum[k] * (LD(1) if defect == "half" else LD(0.5)))
    Wabs = np.where(cls >= 0, cumabs[np.maximum(cls, 0)], cumabs[k] * LD(0.5))
    return W, Wabs


def sinc(x, defect=None):
    x = np.asarray(x, dtype=LD)
    safe = np.where(x == 0, LD(1), x)
    return np.where(x == 0, LD(0) if defect == "r0" else LD(1), np.sin(safe) / safe)


def sinc_romb(g, ka, dlk, r, defect=None, chunk=64):
    """corahip_sinc_romb -> (value [nr] longdouble, bound [nr] float64)."""
    g = np.asarray(g, dtype=np.float64)
    ka = np.asarray(ka, dtype=np.float64)
    r = np.atleast_1d(np.asarray(r, dtype=np.float64))
    K = g.size - 1
    k = K.bit_length() - 1
    assert K == 1 << k and k >= 1 and ka.size == g.size
    W, Wabs = romb_weights(k, defect)
    val = np.empty(r.size, dtype=LD)
    for a in range(0, r.size, chunk):
        x = (ka[None, :] * r[a : a + chunk, None]).astype(LD)          # the double product, as the device forms it
        val[a : a + chunk] = (sinc(x, defect) * (W * g.astype(LD))[None, :]).sum(axis=1) * LD(dlk)
    ag = np.abs(g)
    cls = sample_classes(k)
    absS = np.array([ag[cls == t].sum() for t in range(k)] + [0.0])
    tail = np.cumsum(absS[::-1])[::-1]                                   # sum_{s >= t} |S_s|
    Tmax = max(2.0**t * (0.5 * (ag[0] + ag[K]) + tail[t]) for t in range(k + 1))
    D = max(K // 256, 1) + 7 + k
    bound = abs(dlk) * EPS * ((4.5 + D / 2.0) * float((Wabs * ag).sum()) + 4.0 * k * Tmax)
    return val, np.full(r.size, bound)


def corr_direct(psfunc, log_k0, log_k1, r, k=16):
    """The reference's _corr_direct (corrfunc.py:72-84) through the oracle -> (value, bound)."""
    ka = np.logspace(log_k0, log_k1, (1 << k) + 1)
    dlk = np.log(ka[1] / ka[0])
    g = np.reshape(psfunc(ka[np.newaxis, :]), -1) * ka**3 / (2 * np.pi**2)
    return sinc_romb(g, ka, dlk, r)


# ---------------------------------------------------------------------------------------------------------------------
# the FFTLog kernel
# ---------------------------------------------------------------------------------------------------------------------
def _im_lngamma_terms(x, y, shift, nterms):
    """Im lnGamma(x + i y) by a shift and the Stirling series -> (value, sum of the absolute terms), longdouble."""
    sa = np.zeros_like(y)
    for j in range(shift):
        sa = sa + np.arctan2(y, x + j)
    xw = x + shift
    r2 = xw * xw + y * y
    lnabs = LD(0.5) * np.log(r2)
    arg = np.arctan2(y, xw)
    iw = (xw - 1j * y) / r2
    ser = np.zeros_like(iw)
    for num, den in reversed(STIRLING[:nterms]):
        ser = ser * iw * iw + LD(num) / LD(den)
    ser = (ser * iw).imag
    val = (xw - LD(0.5)) * arg + y * (lnabs - 1) + ser - sa
    mag = np.abs(xw - LD(0.5)) * np.abs(arg) + np.abs(y) * (np.abs(lnabs) + 1) + np.abs(ser) + sa
    return val, mag, sa


def fftlog_theta(mu, L, N):
    """theta_m, m = 0 .. N // 2 -> (theta longdouble, bound float64)."""
    m = np.arange(N // 2 + 1, dtype=LD)
    eta = 2 * PI_LD * m / LD(L)
    x = LD(0.5) * (LD(mu) + 1)
    y = LD(0.5) * eta
    val, _, _ = _im_lngamma_terms(x, y, 40, 8)
    theta = eta * np.log(LD(2)) + 2 * val
    _, mag, sa = _im_lngamma_terms(x, y, 16, 7)
    M = np.abs(eta) * np.log(LD(2)) + 2 * mag
    return theta, (EPS * (8.0 * M + 8.0 * sa) + TRUNC).astype(np.float64)


def fftlog_phase(mu, L, N):
    """corahip_fftlog_phase -> (U [N // 2 + 1] complex longdouble, bound on |U_dev - U|)."""
    theta, bt = fftlog_theta(mu, L, N)
    return np.cos(theta) + 1j * np.sin(theta), bt + 3 * EPS


# ---------------------------------------------------------------------------------------------------------------------
# the convolution
# ---------------------------------------------------------------------------------------------------------------------
def logconv_bound(f):
    f = np.asarray(f, dtype=np.float64)
    return 4.0 * EPS * (4.0 * np.log2(max(f.size, 2)) + 31.0) * float(np.sqrt((f.astype(LD) ** 2).sum()))


def logconv(f, U):
    """corahip_logconv -> (irfft(rfft(f) U) [N] float64, bound (scalar, per element))."""
    f = np.asarray(f, dtype=np.float64)
    U = np.asarray(U).astype(np.complex128)
    assert U.size == f.size // 2 + 1
    return np.fft.irfft(np.fft.rfft(f) * U, f.size), logconv_bound(f)


def logconv_four_step(f, U, N1, N2, defect=None):
    """The device's scheme, step by step in numpy.  defect: "unconj" (U_{N-m} above N / 2, not its conjugate), "nyquist"
    (the Nyquist product kept complex), "twiddle" (the forward twiddle left out)."""
    f = np.asarray(f, dtype=np.float64)
    U = np.asarray(U).astype(np.complex128)
    N = N1 * N2
    assert f.size == N and U.size == N // 2 + 1
    m = np.arange(N)
    full = np.where(2 * m <= N, U[np.minimum(m, N // 2)], (U if defect == "unconj" else np.conj(U))[np.minimum(N - m, N // 2)])
    if N1 == 1 or N2 == 1:
        spec = np.fft.fft(f.astype(np.complex128)) * full
        spec[0] = spec[0].real
        if N % 2 == 0 and defect != "nyquist":
            spec[N // 2] = spec[N // 2].real
        return np.fft.ifft(spec)
    k1 = np.arange(N1)[:, None]
    n2 = np.arange(N2)[None, :]
    tw = np.exp(-2j * np.pi * ((k1 * n2) % N) / N)
    a = np.fft.fft(f.astype(np.complex128).reshape(N1, N2), axis=0)
    if defect != "twiddle":
        a = a * tw
    a = np.fft.fft(a, axis=1)
    mode = k1 + N1 * np.arange(N2)[None, :]
    a = a * full[mode]
    a[0, 0] = a[0, 0].real
    if N % 2 == 0 and defect != "nyquist":
        a[mode == N // 2] = a[mode == N // 2].real
    a = np.fft.ifft(a, axis=1) * np.conj(tw)
    return np.fft.ifft(a, axis=0).reshape(N)


# ---------------------------------------------------------------------------------------------------------------------
# hankl.P2xi and ps_to_corr
# ---------------------------------------------------------------------------------------------------------------------
def fftlog_g(k, P):
    """(r, g) of the FFTLog transform with f = P k^1.5, mu = 1/2, q = 0: r_j = 1 / k_{N-1-j}, g_j = irfft(rfft(f) U)[N-1-j],
    L = N ln(k_1 / k_0)."""
    k = np.asarray(k, dtype=np.float64)
    N = k.size
    U, _ = fftlog_phase(0.5, N * np.log(k[1] / k[0]), N)
    g, _ = logconv(np.asarray(P, dtype=np.float64) * k**1.5, U)
    return 1.0 / k[::-1], g[::-1]


def P2xi(k, P, l=0, lowring=False):
    """Stand-in for ``hankl.P2xi(k, P, 0, lowring=False)`` -> (r, xi): xi = g (2 pi)^-1.5 r^-1.5 of ``fftlog_g``."""
    assert l == 0 and not lowring
    r, g = fftlog_g(k, P)
    return r, g * (2 * np.pi) ** -1.5 * r**-1.5


def _level_bound(f, k):
    """Bound of g = irfft(rfft(f) U) per element: the convolution plus the error of U."""
    N = f.size
    _, bU = fftlog_phase(0.5, N * np.log(k[1] / k[0]), N)
    F = np.abs(np.fft.rfft(f))
    return logconv_bound(f) + 2.0 / N * float((F * bU).sum())


def ps_to_corr(psfunc, minlogr=-1, maxlogr=5, switchlogr=2, samples_per_decade=100, minlogk=-5, maxlogk=3,
               richardson_n=6, pad_low=2, pad_high=1):
    """corrfunc.ps_to_corr (corrfunc.py:189-264 with :150-186 inlined) -> (r, value float64, bound float64)."""
    rlow = np.logspace(minlogr, switchlogr, int((switchlogr - minlogr) * samples_per_decade), endpoint=False)
    lo = switchlogr - pad_low
    hi = maxlogr + pad_high
    n = int(samples_per_decade * (hi - lo))
    umax = 2 ** (richardson_n - 1)
    kfine = np.logspace(-hi, -lo, n * umax, endpoint=False)
    Pfine = np.reshape(psfunc(kfine), -1)                       # one evaluation: level ii is a strided subset
    r0 = 1.0 / np.logspace(-hi, -lo, n, endpoint=False)[::-1]   # the r of level 0, which every level lands on
    fac = (2 * np.pi) ** -1.5 * r0**-1.5
    rs, est, bnd = [], [], []
    for ii in range(richardson_n):
        u = 2**ii
        k, P = kfine[:: umax >> ii], Pfine[:: umax >> ii]
        r, g = fftlog_g(k, P)
        rs.append(r[(u - 1) :: u])
        est.append(g[(u - 1) :: u] * fac)
        bnd.append(_level_bound(P * k**1.5, k) * fac + 4 * EPS * np.abs(est[-1]))
    for r in rs:
        assert np.allclose(r, r0)
    mask = (np.log10(r0) >= switchlogr) & (np.log10(r0) <= maxlogr)
    rhigh = r0[mask]
    est = [e[mask] for e in est]
    bnd = [b[mask] for b in bnd]
    w = np.abs(richardson_weights(richardson_n)).astype(np.float64)
    fhigh = richardson(est, 2.0)
    bhigh = sum(w[i] * bnd[i] for i in range(richardson_n))
    bhigh = bhigh + 3 * EPS * richardson_n * sum(w[i] * np.abs(est[i]) for i in range(richardson_n))
    rlow = np.insert(rlow, 0, 0.0)
    flow, blow = corr_direct(psfunc, minlogk, maxlogk, rlow)
    return np.concatenate([rlow, rhigh]), np.concatenate([flow.astype(np.float64), fhigh]), np.concatenate([blow + EPS * np.abs(flow.astype(np.float64)), bhigh])


# ---------------------------------------------------------------------------------------------------------------------
# the analytic pair P = k e^(-a k)
# ---------------------------------------------------------------------------------------------------------------------
A_PAIR = 8.0


def pk_pair(k, a=A_PAIR):
    return k * np.exp(-a * k)


def xi_pair(r, a=A_PAIR):
    """xi(r) = 2 sin(3 atan(r / a)) / (2 pi^2 r (a^2 + r^2)^1.5), xi(0) = 6 / (2 pi^2 a^4)."""
    r = np.asarray(r, dtype=LD)
    safe = np.where(r == 0, LD(1), r)
    v = 2 * np.sin(3 * np.arctan(safe / a)) / (2 * PI_LD ** 2 * safe * (a * a + safe * safe) ** LD(1.5))
    return np.where(r == 0, 6 / (2 * PI_LD ** 2 * LD(a) ** 4), v)


def xi_envelope(r, a=A_PAIR):
    """2 / (2 pi^2 r (a^2 + r^2)^1.5), and xi(0) at r = 0: the scale the errors of the pair are judged against."""
    r = np.asarray(r, dtype=np.float64)
    safe = np.where(r == 0, 1.0, r)
    return np.where(r == 0, 6 / (2 * np.pi**2 * a**4), 2 / (2 * np.pi**2 * safe * (a * a + safe * safe) ** 1.5))


def cutoff(x, cut, sign, width, index):
    """lssutil.cutoff (lssutil.py:264-290) in longdouble."""
    x = np.asarray(x, dtype=LD)
    return (LD(0.5) * (1 + np.tanh(np.sign(sign) * (np.log10(x) - LD(cut)) / LD(width)))) ** LD(index)
