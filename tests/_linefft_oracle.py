"""Host oracle of the flat-sky line FFTs (cora_amd/csrc/flatsky.hip, flatsky_ct.hip, fft_ct.h, tile_walk.h): a longdouble
DFT at chosen output indices, closed forms, numpy restatements of the three schemes, and per-line bounds on what the device
may differ by.  CPU only.

u = 2^-53 is one rounding, EPS = 2 u.  No constant below was fitted to device output; the GPU tests print the observed
err / bound next to them.  Everything is first order in u.  Costs of the pieces, relative and for complex values:
    ADD    an addition                                                                           u
    MUL    a product, (a.x b.x - a.y b.y, a.x b.y + a.y b.x) with or without fma                 sqrt(5) u
    TAB    a constant or table entry rounded from a longdouble value, a component                sqrt(2) u
    SCP    a twiddle from the device's sincospi: 2 ulp a component (as _pk2xi_oracle takes it)   2 sqrt(2) u
    LEVEL  one radix-2-equivalent level inside a register butterfly: an addition and at most one product with a rounded
           constant = ADD + MUL + TAB.  levels(R) = log2 R for R = 2, 4, 8, 16 (DftR<16> = dft4, nine constants, dft4: 7.7 u
           on the longest path against 4 LEVEL = 18.6 u) and 5 for R = 10, 12, 14 (dft2 + dft5 / dft7 with four or six
           fma and as many constants: <= 9 u; dft4 + constants + dft3: <= 9.7 u; against 23.3 u).
    CHAIN(R)  the pass twiddles w^r, r < R, that tw_apply makes from w by squarings and products: w^r carries r SCP +
           (r - 1) MUL, and its own product MUL: (R - 1) (SCP + MUL).

Which bound covers which route, and why.

Cooley-Tukey routes - ``bound_c2c`` / ``bound_r2c`` / ``bound_c2r`` with a "sched", "h2" or "r4" route - pointwise in the line's 1-norm.  Every output is sum_j x_j times a product of at most
three rounded twiddles, formed by additions; a relative perturbation d of one factor or one partial sum changes the
output by at most d ||x||_1.  So |err_k| <= c ||x||_1 for EVERY k, with c the sum of the costs on the longest path.  The
bound stays sharp for an impulse (||x||_1 = 1, every |X_k| = 1) and for a tone (||x||_1 = n = the one non-zero output).
    scheduled R0 x 16 x R2 (linec2c_ct, the transforms inside linec2r_ct / liner2c_ct):
        c_sched(N) = [levels(R0) + 4 + levels(R2)] LEVEL + CHAIN(R0) + CHAIN(16) + ADD (the scale)
    linec2c_h2_ct (1024 as two 512s): c_sched(512) + ADD (the last radix-2) + the twiddle w^k = wK wK2^it, it <= 7:
        8 SCP + 7 MUL, and its product MUL
    generic radix-4 stages (linefft_kernel, power-of-two n): a stage multiplies by w1 = w2^2 (2 TAB + MUL) and by w2 (TAB),
        two products, two additions: STAGE4 = 3 TAB + 3 MUL + 2 ADD; c_r4(P) = floor(log4 P) STAGE4 + (log2 P odd) ADD + ADD
    real split on top, r2c: X_k = 1/2 [(Za + conj Zb) - i w (Za - conj Zb)], |Za|, |Zb| <= ||z||_1 <= ||x||_1:
        |err| <= [2 c_fft + 3 ADD + e_w + MUL] ||x||_1;  e_w = SCP + MO (SCP + MUL) where the twiddle is rotated MO =
        NCH N / T times (liner2c_ct), TAB where it is the plan's table (generic mode 4)
    real split below, c2r: Z_k = (X_k + conj X_{N-k}) + i w (X_k - conj X_{N-k}), |Z_k| <= 2 (|X_k| + |X_{N-k}|), so
        ||Z||_1 <= 2 ||X||_h with ||X||_h = |Re X_0| + |Re X_N| + 2 sum_{0<k<N} |X_k| (the 1-norm of the Hermitian line):
        |err| <= scale [2 c_fft + 3 ADD + e_w + MUL] ||X||_h;  e_w = SCP + TAB + MUL (linec2r_ct: wH times a constant), TAB

Bluestein routes - the same three functions with a "blu" route - per element, in the line's 2-norm.  X_k = c_k sum_j (x_j c_j) b_{k-j} as FFT_P, product
with the filter F = FFT_P(b) / P, inverse FFT_P.  In the 2-norm a transform's relative error is the sum of its stage costs
(c_P: c_sched(P) or c_r4(P), the same counts, now relative to the 2-norm because every stage is sqrt(R) times a unitary
map).  With S = max_k |FFT_P(b)_k| (computed here; about 2 sqrt(n)) everything behind the forward transform
is relative to at most sqrt(P) ||A F||_2 <= S ||x||_2:
    input chirp TAB + MUL, forward c_P, filter product MUL, inverse c_P, output chirp TAB + MUL, scale ADD: all times S
    the filter's own error: made on the host in longdouble (generic kernel): TAB |F_k|, i.e. TAB S;
        made on the device by the same transform (flat_blu_filter_kernel): only ||dF||_inf <= ||dF||_2 <= c_P ||F||_2 =
        c_P sqrt((2 n - 1) / P) is certain, which costs c_P sqrt(P (2 n - 1)) - the one term that is not a multiple of S
    |err_k| <= ||err||_2 <= scale ||x||_2 { S [2 TAB + 3 MUL + ADD + 2 c_P] + filter term }
``blu_const`` returns the brace divided by sqrt(n): the bound reads C sqrt(n) ||x||_2, sqrt(n) ||x||_2 being ||X||_2.
    even real lengths 2 h through a complex line of length h (lineblu_r2c_ct / _c2r_ct, generic modes 3 / 4):
        r2c: ||z||_2 = ||x||_2 and |Z_k| <= sqrt(h) ||x||_2: |err| <= 2 B(h, ||x||_2) + [3 ADD + TAB + MUL] sqrt(h) ||x||_2
        c2r: the packed line has ||Z||_2 <= 2 (||X_{0..h-1}||_2 + ||X_{1..h}||_2) =: Zn, packing costs 3 ADD + TAB + MUL of
             it and reaches the output through sqrt(h): |err| <= scale { B(h, Zn) + [3 ADD + TAB + MUL] sqrt(h) Zn }
    odd real lengths (generic modes 1 / 2): a full complex line: r2c B(n, ||x||_2), c2r scale B(n, ||Hermitian line||_2)
(Im of the DC bin, and of the Nyquist bin of an even length, is left out of every norm of a half-complex line: numpy
ignores it, and so must the device.)

numpy's own error - ``numpy_allowance`` - widens the bound where numpy.fft is the reference.  pocketfft makes its twiddles
correctly rounded (TAB) and runs radix 2, 3, 4, 5, 7, 11 passes: at most ceil(log2 n) levels of LEVEL.  A prime factor
p > 11 goes through a direct p-term pass (p additions) or through Bluestein of length p; the allowance takes the larger of
p^1.5 u and this module's own Bluestein count for (p, next power of two) relative to the 2-norm.  All of that is relative
to ||X||_2 = sqrt(n) ||x||_2 in the 2-norm; for 11-smooth n it also holds pointwise in ||x||_1, and the smaller of the
two is used.  Closed forms need no allowance except that a tone is rounded when it is stored: u ||x||_1.

The oracle's own sums are pairwise in longdouble: (log2 n + 3) 2^-64 ||x||_1, below 1e-3 of any bound here, not carried.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "the oracle needs an extended-precision long double"
EPS = 2.0**-52
U = EPS / 2
PI_LD = 4 * np.arctan(LD(1))

ADD = U
MUL = np.sqrt(5.0) * U
TAB = np.sqrt(2.0) * U
SCP = 2 * np.sqrt(2.0) * U
LEVEL = ADD + MUL + TAB
STAGE4 = 3 * TAB + 3 * MUL + 2 * ADD

# DIF radices of the three-pass schedules, largest stride first (fft_ct.h, Sch<N>)
SCH = {256: (16, 16, 1), 512: (16, 16, 2), 1024: (16, 16, 4), 2048: (16, 16, 8), 4096: (16, 16, 16),
       192: (12, 16, 1), 384: (12, 16, 2), 768: (12, 16, 4), 1536: (12, 16, 8), 3072: (12, 16, 16),
       320: (10, 16, 2), 640: (10, 16, 4), 1280: (10, 16, 8), 2560: (10, 16, 16), 3584: (14, 16, 16)}
# the compile-time convolution lengths and their lines per item (flat_blu_length, flat_blu_c2c_ct / flat_blu_real_ct)
BLU_P = (256, 320, 384, 512, 640, 768, 1024, 1280, 1536, 2048, 2560, 3072, 3584, 4096)
BLU_NCH = {256: 16, 320: 16, 384: 16, 512: 16, 640: 8, 768: 8, 1024: 8, 1280: 4, 1536: 4, 2048: 4, 2560: 2, 3072: 2,
           3584: 2, 4096: 2}


def blu_length(n):
    """flat_blu_length: the smallest scheduled P >= 2 n - 1 (0: none; flat_blu_plan also declines n < 17)."""
    if n < 17:
        return 0
    for P in BLU_P:
        if P >= 2 * n - 1:
            return P
    return 0


def pow2_length(n, blu):
    P = 1
    while P < (2 * n - 1 if blu else n):
        P <<= 1
    return P


# ---------------------------------------------------------------------------------------------------------------------
# reference: longdouble DFT at chosen outputs, closed forms
# ---------------------------------------------------------------------------------------------------------------------
def phase(idx, n, sign):
    """e^{sign 2 pi i idx / n} for integer idx, reduced mod n in integers before the one rounding; complex longdouble."""
    a = (2 * PI_LD) * (np.asarray(idx, dtype=np.int64) % n).astype(LD) / LD(n)
    out = np.empty(a.shape, dtype=CLD)
    out.real = np.cos(a)
    out.imag = sign * np.sin(a)
    return out


def dft(x, ks, sign=-1):
    """X_k = sum_j x_j e^{sign 2 pi i (j k mod n) / n} for k in ks; x [..., n] -> [..., len(ks)] complex longdouble."""
    x = np.asarray(x)
    n = x.shape[-1]
    ks = np.asarray(ks, dtype=np.int64)
    W = phase(np.arange(n, dtype=np.int64)[None, :] * ks[:, None], n, sign)
    return (x.astype(CLD)[..., None, :] * W).sum(axis=-1)


def hermitian_clean(X, n):
    """A half-complex line as numpy reads it: Im of the DC bin (and of the Nyquist bin of an even n) dropped."""
    X = np.array(X, dtype=np.complex128)
    X[..., 0] = X[..., 0].real
    if n % 2 == 0:
        X[..., n // 2] = X[..., n // 2].real
    return X


def hermitian_weights(n):
    w = np.full(n // 2 + 1, 2.0)
    w[0] = 1.0
    if n % 2 == 0:
        w[n // 2] = 1.0
    return w


def irdft(X, n, js):
    """numpy.fft.irfft(X, n)[js] in longdouble: X [..., n // 2 + 1] -> [..., len(js)]."""
    Xc = hermitian_clean(X, n).astype(CLD) * hermitian_weights(n).astype(LD)
    js = np.asarray(js, dtype=np.int64)
    W = phase(np.arange(n // 2 + 1, dtype=np.int64)[None, :] * js[:, None], n, +1)
    return (Xc[..., None, :] * W).real.sum(axis=-1) / LD(n)


def impulse_spectrum(n, j, ks, sign=-1):
    """DFT of the unit impulse at j: e^{sign 2 pi i j k / n}; every |X_k| = 1."""
    return phase(int(j) * np.asarray(ks, dtype=np.int64), n, sign)


def tone(n, m, sign=+1):
    """x_j = e^{sign 2 pi i m j / n} rounded to double: its DFT of the opposite sign is n at k = m and leakage elsewhere."""
    return phase(int(m) * np.arange(n, dtype=np.int64), n, sign).astype(np.complex128)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def levels(R):
    return {1: 0, 2: 1, 4: 2, 8: 3, 16: 4, 10: 5, 12: 5, 14: 5}[R]


def chain(R):
    return (R - 1) * (SCP + MUL) if R > 1 else 0.0


def c_sched(N):
    R0, R1, R2 = SCH[N]
    return (levels(R0) + levels(R1) + levels(R2)) * LEVEL + chain(R0) + chain(R1) + ADD


def c_h2(N=1024):
    return c_sched(N // 2) + ADD + 8 * SCP + 7 * MUL + MUL


def c_r4(P):
    logP = int(P).bit_length() - 1
    assert 1 << logP == P
    return (logP // 2) * STAGE4 + (logP & 1) * ADD + ADD


class Route:
    """How a line transform is computed.  kind: "sched" (Sch<N> passes), "h2" (linec2c_h2_ct), "r4" (generic radix-4
    stages), "blu" (Bluestein at P; ct: on the compile-time passes with the device-made filter).  n: complex length."""

    def __init__(self, kind, n, P=0, ct=True, nch=1, mo=0):
        self.kind, self.n, self.P, self.ct, self.nch, self.mo = kind, int(n), int(P), bool(ct), int(nch), int(mo)

    @property
    def compile_time(self):
        return self.kind in ("sched", "h2") or (self.kind == "blu" and self.ct)

    def __repr__(self):
        return "%s(n=%d%s%s)" % (self.kind, self.n, ", P=%d" % self.P if self.P else "", "" if self.compile_time else ", generic")


def c_fft(route):
    """The Cooley-Tukey constant of a route's complex transform (pointwise in the 1-norm; relative in the 2-norm)."""
    if route.kind == "sched":
        return c_sched(route.n)
    if route.kind == "h2":
        return c_h2(route.n)
    assert route.kind == "r4"
    return c_r4(route.n)


_S_CACHE = {}


def chirp_table(n):
    """c_j = e^{-i pi j^2 / n}, j < n (j^2 mod 2 n keeps the angle exact), complex128 as the plan stores it."""
    j = np.arange(n, dtype=np.int64)
    return phase(j * j, 2 * n, -1).astype(np.complex128)


def wrapped_filter(n, P, defect=None):
    """b[m] = conj c_m at m < n and at P - m, zero between; defect "wrap": the entry b[P - (n - 1)] left out."""
    b = np.zeros(P, dtype=np.complex128)
    c = np.conj(chirp_table(n))
    b[:n] = c
    b[P - np.arange(1, n)] = c[1:]
    if defect == "wrap" and n > 1:
        b[P - (n - 1)] = 0.0
    return b


def filter_peak(n, P):
    """S = max_k |FFT_P(b)_k| (double transform of 2 n - 1 unit entries: good to 1e-13, taken 1e-12 high)."""
    if (n, P) not in _S_CACHE:
        _S_CACHE[(n, P)] = float(np.abs(np.fft.fft(wrapped_filter(n, P))).max()) * (1 + 1e-12)
    return _S_CACHE[(n, P)]


def blu_brace(n, P, ct):
    """The brace of the module docstring: |err_k| <= scale ||x||_2 blu_brace."""
    cP = c_sched(P) if ct else c_r4(P)
    S = filter_peak(n, P)
    filt = cP * np.sqrt(P * (2.0 * n - 1.0)) if ct else TAB * S
    return S * (2 * TAB + 3 * MUL + ADD + 2 * cP) + filt


def blu_const(route):
    """C with |err_k| <= C sqrt(n) ||x||_2 for a Bluestein route."""
    return blu_brace(route.n, route.P, route.ct) / np.sqrt(route.n)


def norms(x):
    """(||x||_1, ||x||_2) per line of x [..., n], in longdouble sums returned as float64."""
    a = np.abs(np.asarray(x)).astype(LD)
    return a.sum(axis=-1).astype(np.float64), np.sqrt((a * a).sum(axis=-1)).astype(np.float64)


def herm_norms(X, n):
    """(||X||_h, 2-norm of the Hermitian line) per half-complex line X [..., n // 2 + 1] of real length n."""
    a = np.abs(hermitian_clean(X, n)).astype(LD)
    w = hermitian_weights(n).astype(LD)
    return (a * w).sum(axis=-1).astype(np.float64), np.sqrt((a * a * w).sum(axis=-1)).astype(np.float64)


SPLIT = 3 * ADD + MUL          # the additions and the product of the real split, without its twiddle


def _split_twiddle(route, c2r):
    if route.kind == "sched":
        return SCP + TAB + MUL if c2r else SCP + route.mo * (SCP + MUL)
    return TAB


def bound_c2c(route, x, scale=1.0):
    """Per line of x [lines, n]: the bound on every output of the complex transform times ``scale``."""
    n1, n2 = norms(x)
    if route.kind == "blu":
        return abs(scale) * blu_brace(route.n, route.P, route.ct) * n2
    return abs(scale) * c_fft(route) * n1


def bound_r2c(route, x):
    """Per line of the real x [lines, n]: even n through route (complex length n / 2), odd n as a full Bluestein line."""
    n = x.shape[-1]
    n1, n2 = norms(x)
    if n % 2:
        assert route.kind == "blu" and route.n == n
        return blu_brace(n, route.P, route.ct) * n2
    h = n // 2
    assert route.n == h
    tw = _split_twiddle(route, False)
    if route.kind == "blu":
        return 2 * blu_brace(h, route.P, route.ct) * n2 + (SPLIT + tw) * np.sqrt(h) * n2
    return (2 * c_fft(route) + SPLIT + tw) * n1


def bound_c2r(route, X, n):
    """Per half-complex line X [lines, n // 2 + 1]: the bound on every real output of irfft(X, n) (scale 1 / n)."""
    h1, h2 = herm_norms(X, n)
    if n % 2:
        assert route.kind == "blu" and route.n == n
        return blu_brace(n, route.P, route.ct) * h2 / n
    h = n // 2
    assert route.n == h
    tw = _split_twiddle(route, True)
    if route.kind == "blu":
        Xc = hermitian_clean(X, n)
        Zn = 2 * (norms(Xc[..., :h])[1] + norms(Xc[..., 1:])[1])
        return (blu_brace(h, route.P, route.ct) + (SPLIT + tw) * np.sqrt(h)) * Zn / n
    return (2 * c_fft(route) + SPLIT + tw) * h1 / n


def _largest_prime(n):
    p, f = 1, 2
    while f * f <= n:
        while n % f == 0:
            p, n = max(p, f), n // f
        f += 1
    return max(p, n) if n > 1 else p


_NP_CACHE = {}


def numpy_consts(n):
    """(c1 or None, c2): numpy's transform of length n errs by at most c1 ||x||_1 (11-smooth n) and c2 sqrt(n) ||x||_2."""
    if n not in _NP_CACHE:
        lv = int(np.ceil(np.log2(max(n, 2)))) * LEVEL
        p = _largest_prime(n)
        if p <= 11:
            _NP_CACHE[n] = (lv, lv)
        else:
            P = pow2_length(p, True)
            cP = int(np.log2(P)) * LEVEL
            blu = (filter_peak(p, P) * (2 * TAB + 3 * MUL + ADD + 2 * cP) + cP * np.sqrt(P * (2.0 * p - 1.0))) / np.sqrt(p)
            _NP_CACHE[n] = (None, lv + max(p**1.5 * U, blu))
    return _NP_CACHE[n]


def numpy_allowance(n, n1, n2, scale=1.0):
    """What numpy.fft's own result may be off by, per line with norms (n1, n2) of its input (Hermitian norms for irfft)."""
    c1, c2 = numpy_consts(n)
    a = c2 * np.sqrt(n) * np.asarray(n2)
    if c1 is not None:
        a = np.minimum(a, c1 * np.asarray(n1))
    return abs(scale) * a


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of the three schemes (double precision, as the device computes; lines [L, n])
# ---------------------------------------------------------------------------------------------------------------------
def _small_dft(R, sign):
    k = np.arange(R, dtype=np.int64)
    return phase(k[:, None] * k[None, :], R, sign).astype(np.complex128)


def three_pass_dif(x, sign=-1, defect=None):
    """The R0 x 16 x R2 decimation-in-frequency passes of Sch<N> on natural-order lines x [L, N]: pass A (sub-length N,
    stride Q0 = N / R0, twiddle e^{sign 2 pi i j0 k0 / N}), pass B (sub-length Q0, twiddle e^{sign 2 pi i j1 k1 / Q0}), the
    radix-R2 pass on contiguous elements; output k = k0 + R0 k1 + 16 R0 k2.
    defect "twiddle": the pass-A twiddle w^r of (j0 = Q0 - 1, r = 3) off by 1e-13 relative."""
    x = np.asarray(x, dtype=np.complex128)
    L, N = x.shape
    R0, R1, R2 = SCH[N]
    Q0, Q1 = N // R0, R2
    a = np.einsum("kr,lrj->lkj", _small_dft(R0, sign), x.reshape(L, R0, Q0))
    twA = phase(np.arange(R0, dtype=np.int64)[:, None] * np.arange(Q0, dtype=np.int64)[None, :], N, sign).astype(np.complex128)
    if defect == "twiddle":
        twA[3, Q0 - 1] *= 1.0 + 1e-13
    a = a * twA[None]
    b = np.einsum("kr,lmrj->lmkj", _small_dft(R1, sign), a.reshape(L, R0, R1, Q1))
    twB = phase(np.arange(R1, dtype=np.int64)[:, None] * np.arange(Q1, dtype=np.int64)[None, :], Q0, sign).astype(np.complex128)
    b = b * twB[None, None]
    c = np.einsum("kr,lmjr->lmjk", _small_dft(R2, sign), b)          # [L, k0, k1, k2]
    return np.ascontiguousarray(c.transpose(0, 3, 2, 1)).reshape(L, N)


def _fft_scheme(x, sign):
    """Unnormalised transform of the lines of x by the three-pass scheme where the length has one, numpy otherwise."""
    if x.shape[-1] in SCH:
        return three_pass_dif(x, sign)
    return np.fft.fft(x, axis=-1) if sign < 0 else np.fft.ifft(x, axis=-1) * x.shape[-1]


def bluestein(x, P, sign=-1, defect=None, scale=1.0):
    """X_k = c_k sum_j (x_j c_j) b_{k-j} at the convolution length P >= 2 n - 1 with the wrapped filter b[m], b[P - m]; the
    inverse transform by conjugation at the commit and the store, as the kernels do.  Lines share one buffer, as the
    lines of successive items share LDS.  defect: "chirp" (the output chirp of k = n - 1 taken at n - 2), "wrap" (filter
    entry b[P - (n - 1)] left out), "pad" (the pad [n, P / 2) of a line not cleared: it holds what the previous line left)."""
    x = np.asarray(x, dtype=np.complex128)
    L, n = x.shape
    assert P >= 2 * n - 1
    c = chirp_table(n)
    F = _fft_scheme(wrapped_filter(n, P, defect)[None, :], -1)[0] / P
    cout = c.copy()
    if defect == "chirp" and n > 1:
        cout[n - 1] = c[n - 2]
    out = np.empty_like(x)
    buf = np.zeros(P, dtype=np.complex128)
    for l in range(L):
        v = np.conj(x[l]) if sign > 0 else x[l]
        buf[:n] = v * c
        if defect != "pad":
            buf[n : P // 2] = 0.0
        buf[P // 2 :] = 0.0
        A = _fft_scheme(buf[None, :], -1)[0]
        buf[:] = _fft_scheme((A * F)[None, :], +1)[0]
        y = buf[:n] * cout
        out[l] = (np.conj(y) if sign > 0 else y) * scale
    return out


def real_unpack(x, fft, defect=None):
    """rfft of even-length real lines x [L, 2 h] through z_j = x_2j + i x_2j+1, Z = fft(z) (forward, length h) and the split
    X_k = 1/2 [(Z_k + conj Z_{h-k}) - i e^{-i pi k / h} (Z_k - conj Z_{h-k})], k = 0 .. h, Z_h := Z_0.
    defect "noconj": the partner Z_{h-k} taken without its conjugate."""
    x = np.asarray(x, dtype=np.float64)
    L, n = x.shape
    h = n // 2
    Z = fft(x[:, 0::2] + 1j * x[:, 1::2])
    k = np.arange(h + 1)
    Za = Z[:, k % h]
    Zb = Z[:, (h - k) % h]
    if defect != "noconj":
        Zb = np.conj(Zb)
    w = phase(k, 2 * h, -1).astype(np.complex128)
    return 0.5 * ((Za + Zb) - 1j * w[None, :] * (Za - Zb))


def real_pack(X, n, ifft, defect=None):
    """irfft(X, n) of even n = 2 h: Z_k = (X_k + conj X_{h-k}) + i e^{i pi k / h} (X_k - conj X_{h-k}), k < h, z = ifft(Z)
    (sign +, unnormalised, length h), x_2j = Re z_j / n, x_2j+1 = Im z_j / n.
    defect "imdc": Im of the DC and Nyquist bins kept."""
    X = np.asarray(X, dtype=np.complex128)
    h = n // 2
    Xc = X.copy() if defect == "imdc" else hermitian_clean(X, n)
    k = np.arange(h)
    Xa, Xb = Xc[:, k], np.conj(Xc[:, h - k])
    w = phase(k, 2 * h, +1).astype(np.complex128)
    z = ifft((Xa + Xb) + 1j * w[None, :] * (Xa - Xb)) / n
    out = np.empty((X.shape[0], n))
    out[:, 0::2] = z.real
    out[:, 1::2] = z.imag
    return out


def leak(out, defect=None):
    """defect "leak": line c's result added into line c + 1 at 1e-14 of line c's norm (per element: 1e-14 of its values)."""
    if defect != "leak":
        return out
    out = np.array(out)
    out[1:] += 1e-14 * out[:-1]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# input families: every line different
# ---------------------------------------------------------------------------------------------------------------------
SCALE_EXP = (300, -300, 150, -150, 0, 299, -299, 75, -75, 1, -1, 225, -225)
FAMILIES = ("impulse", "scaled", "tone", "noise")     # the order in which neighbouring lines take them


def line_plan(nlines, n, q0, offset=0, rot=0):
    """[(family, parameter)] per line: ("impulse", j), ("tone", m), ("noise", 0), ("scaled", exponent).  Neighbouring
    lines cycle through the four families, so that any four lines in a row hold all of them and every scaled line sits
    next to lines of another scale, whatever the lines per item; group g = (line + offset) / 4 + rot takes the g-th
    impulse position, tone and exponent.  Impulses at j = 0, 1, n / 2, n - 1, q0 - 1, q0 (q0: first-pass stride of
    the route, 0: none); tones m = 1, n / 2, n - 1."""
    imp = [0, 1, n // 2, n - 1, (q0 - 1) if q0 else n // 3, q0 if q0 else (2 * n) // 3]
    imp = [min(max(j, 0), n - 1) for j in imp]
    ton = [min(1, n - 1), n // 2, n - 1]
    plan = []
    for l in range(nlines):
        fam = FAMILIES[(l + offset) % 4]
        g = (l + offset) // 4 + rot
        par = {"impulse": imp[g % 6], "tone": ton[g % 3], "noise": 0, "scaled": SCALE_EXP[g % len(SCALE_EXP)]}[fam]
        plan.append((fam, par))
    return plan


def make_lines(kind, n, nlines, seed, q0=0, offset=0, rot=0):
    """Input lines of a transform and what is known about them in closed form.
    kind: "fwd" / "inv" (complex, length n), "r2c" (real, length n), "c2r" (half-complex, n // 2 + 1 bins of real length n).
    Returns (x [nlines, n_in], plan, exact) with exact[l] = None or (k, value): the output of line l is ``value`` at k and
    zero elsewhere (tones), or exact[l] = ("all", spectrum) for impulses."""
    rng = np.random.default_rng(seed)
    nb = n // 2 + 1
    plan = line_plan(nlines, n if kind != "c2r" else nb, q0, offset, rot)
    if kind in ("fwd", "inv"):
        x = rng.standard_normal((nlines, n)) + 1j * rng.standard_normal((nlines, n))
    elif kind == "r2c":
        x = rng.standard_normal((nlines, n))
    else:
        x = rng.standard_normal((nlines, nb)) + 1j * rng.standard_normal((nlines, nb))     # Im of DC / Nyquist is not zero
    sgn = -1 if kind in ("fwd", "r2c") else +1
    inv_scale = 1.0 / n if kind in ("inv", "c2r") else 1.0
    exact = [None] * nlines
    kout = np.arange(nb if kind == "r2c" else n)
    memo = {}                                    # (family, parameter) -> (input line, closed form): few distinct ones

    def known(fam, par):
        if fam == "impulse":
            line = np.zeros(x.shape[1], dtype=x.dtype)
            if kind == "c2r":
                # spectrum impulse at bin par, amplitude 1 + 0.75 i: Im is ignored at the DC / Nyquist bins
                line[par] = 1.0 + 0.75j
                edge = par == 0 or (n % 2 == 0 and par == n // 2)
                ph = phase(par * np.arange(n, dtype=np.int64), n, +1)
                val = ph.real / LD(n) if edge else 2 * (ph * CLD(1.0 + 0.75j)).real / LD(n)
                return line, ("all", val.astype(np.float64))
            line[par] = 1.0
            return line, ("all", (impulse_spectrum(n, par, kout, sgn) * LD(inv_scale)).astype(np.complex128))
        if kind in ("fwd", "inv"):
            return tone(n, par, -sgn), (par, n * inv_scale)
        if kind == "r2c":
            m = min(par, n - par)
            return tone(n, par, +1).real, (m, float(n) if (m == 0 or 2 * m == n) else n / 2.0)
        # the spectrum of the unit impulse at j0 = par (a real-space position < nb): x = delta_{j0}
        return impulse_spectrum(n, par, np.arange(nb), -1).astype(np.complex128), (par, 1.0)

    for l, (fam, par) in enumerate(plan):
        if fam == "scaled":
            x[l] *= 2.0**par
        elif fam in ("impulse", "tone"):
            if (fam, par) not in memo:
                memo[(fam, par)] = known(fam, par)
            x[l], exact[l] = memo[(fam, par)]
    return x, plan, exact


def exact_rows(exact, nout):
    """exact -> (rows, ref [len(rows), nout], rounded to double) for the lines known in closed form."""
    rows = [l for l, e in enumerate(exact) if e is not None]
    cplx = any(np.iscomplexobj(exact[l][1]) for l in rows)
    ref = np.zeros((len(rows), nout), dtype=np.complex128 if cplx else np.float64)
    for i, l in enumerate(rows):
        k, v = exact[l]
        if isinstance(k, str):
            ref[i] = v
        else:
            ref[i, k] = v
    return np.asarray(rows, dtype=np.int64), ref


# ---------------------------------------------------------------------------------------------------------------------
# the check shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def sample_outputs(nout, half, rng, count=64):
    """At least ``count`` output indices (all of them where there are fewer) including 0, 1, n / 2 and the last one."""
    if nout <= count:
        return np.arange(nout, dtype=np.int64)
    must = np.array([0, 1, half, nout - 1], dtype=np.int64)
    rest = rng.choice(nout, size=count, replace=False)
    return np.unique(np.concatenate([must, rest]))


def check_lines(kind, route, n, x, exact, got, ld_lines, seed=0):
    """Hold the transform ``got`` [lines, n_out] of the input lines ``x`` (make_lines) to the route's bound, per line and
    per element: every output against numpy.fft (bound + numpy_allowance) or, where the line has one, its closed form
    (bound + u |ref|, and u ||x||_1 for the rounding of a stored tone); the outputs ``sample_outputs`` of the lines
    ``ld_lines`` against the longdouble DFT under the bare bound.
    Returns (worst err / bound against numpy and closed forms, worst against the longdouble DFT, messages of failures)."""
    x = np.asarray(x)
    got = np.asarray(got)
    msgs = []
    if not np.isfinite(got.view(np.float64)).all():
        msgs.append("output not finite")
        return np.inf, np.inf, msgs
    if kind in ("fwd", "inv"):
        scale = 1.0 if kind == "fwd" else 1.0 / n
        B = bound_c2c(route, x, scale)
        ref = np.fft.fft(x, axis=-1) if kind == "fwd" else np.fft.ifft(x, axis=-1)
        n1, n2 = norms(x)
    elif kind == "r2c":
        scale = 1.0
        B = bound_r2c(route, x)
        ref = np.fft.rfft(x, axis=-1)
        n1, n2 = norms(x)
    else:
        scale = 1.0 / n
        B = bound_c2r(route, x, n)
        ref = np.fft.irfft(x, n, axis=-1)
        n1, n2 = herm_norms(x, n)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    allowed = np.repeat((B + numpy_allowance(n, n1, n2, scale))[:, None], ref.shape[1], axis=1)
    rows, eref = exact_rows(exact, ref.shape[1])
    if rows.size:
        eref = eref.astype(ref.dtype)
        ref[rows] = eref
        tone_rows = np.array([not isinstance(exact[l][0], str) for l in rows])
        allowed[rows] = B[rows, None] + U * np.abs(eref) + (tone_rows * U * scale * n1[rows])[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        ratio = np.abs(got - ref) / allowed
    worst_np = float(ratio.max())
    if not worst_np < 1.0:
        l, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        msgs.append("line %d output %d: err / bound = %.3g against %s" % (l, k, worst_np, "the closed form" if l in set(rows.tolist()) else "numpy"))
    ld_lines = np.asarray(sorted(ld_lines), dtype=np.int64)
    ks = sample_outputs(ref.shape[1], n // 2 if kind != "r2c" else ref.shape[1] - 1, np.random.default_rng(seed))
    if kind == "c2r":
        want = irdft(x[ld_lines], n, ks)
    else:
        want = dft(x[ld_lines], ks, -1 if kind in ("fwd", "r2c") else +1) * LD(scale)
    r = (np.abs(got[ld_lines][:, ks].astype(want.dtype) - want) / B[ld_lines, None].astype(LD)).max(axis=1)
    for l, v in zip(ld_lines, r):
        if not v < 1.0:
            msgs.append("line %d: err / bound = %.3g against the longdouble DFT" % (l, float(v)))
    return worst_np, float(r.max()), msgs
