"""The bounds of tests/_linefft_oracle.py discriminate: the numpy restatements of the three line-FFT schemes (three-pass
DIF with the Sch radices, Bluestein with the wrapped filter, the half-length real pack / unpack) stay under them for
every input family of tests/test_gpu_linefft.py, and each of seven planted defects is rejected by at least one family.
CPU only; no observed GPU figure is asserted here."""
import numpy as np
import pytest

import _linefft_oracle as lo

NL = 32        # eight groups of the line plan: every family, impulse position, tone, and scales 2^+-300 next to 1


def _run(kind, route, n, transform, q0=0, seed=1):
    """worst err / bound of ``transform`` (lines -> lines) over the families of make_lines, per family."""
    x, plan, exact = lo.make_lines(kind, n, NL, seed, q0=q0)
    got = transform(x)
    fam = np.array([p[0] for p in plan])
    out = {}
    for f in ("noise", "impulse", "tone", "scaled"):
        rows = np.nonzero(fam == f)[0]
        sub_exact = [exact[l] for l in rows]
        a, b, _ = lo.check_lines(kind, route, n, x[rows], sub_exact, got[rows], [0, len(rows) - 1], seed)
        out[f] = max(a, b)
    return out


def _c2c(N, sign, defect=None):
    return lambda x: lo.leak(lo.three_pass_dif(x, sign, defect) * (1.0 if sign < 0 else 1.0 / N), defect)


def _blu(n, P, sign, defect=None):
    return lambda x: lo.leak(lo.bluestein(x, P, sign, defect, 1.0 if sign < 0 else 1.0 / n), defect)


def _fft_of(route, sign, defect=None):
    """The unnormalised complex transform of a route, as the real pack / unpack uses it."""
    if route.kind == "blu":
        return lambda z: lo.bluestein(z, route.P, sign, defect)
    return lambda z: lo.three_pass_dif(z, sign, defect)


def _r2c(route, defect=None):
    return lambda x: lo.leak(lo.real_unpack(x, _fft_of(route, -1, defect), defect), defect)


def _c2r(route, n, defect=None):
    return lambda X: lo.leak(lo.real_pack(X, n, _fft_of(route, +1, defect), defect), defect)


SCHED = sorted(lo.SCH)
# both ends of the range of four convolution lengths, and the largest
BLU = [(17, 256), (127, 256), (128, 256), (129, 320), (160, 320), (257, 640), (320, 640), (641, 1536), (1793, 4096), (2047, 4096)]


@pytest.mark.parametrize("N", SCHED)
def test_three_pass_dif_is_under_the_pointwise_bound(N):
    route = lo.Route("sched", N)
    q0 = N // lo.SCH[N][0]
    for kind, sign in (("fwd", -1), ("inv", +1)):
        worst = _run(kind, route, N, _c2c(N, sign), q0)
        print("three-pass DIF N = %d %s: worst err / bound per family %s" % (N, kind, worst))
        assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize("n,P", BLU)
def test_bluestein_is_under_the_two_norm_bound(n, P):
    route = lo.Route("blu", n, P)
    for kind, sign in (("fwd", -1), ("inv", +1)):
        worst = _run(kind, route, n, _blu(n, P, sign), P // lo.SCH[P][0])
        print("Bluestein n = %d P = %d %s: worst err / bound per family %s, S / sqrt(n) = %.3f, C = %.1f EPS"
              % (n, P, kind, worst, lo.filter_peak(n, P) / np.sqrt(n), lo.blu_const(route) / lo.EPS))
        assert max(worst.values()) < 1.0, worst


REAL = [lo.Route("sched", 192, mo=6), lo.Route("sched", 1024, mo=16), lo.Route("sched", 2048, mo=16),
        lo.Route("blu", 17, 256), lo.Route("blu", 128, 256), lo.Route("blu", 161, 384), lo.Route("blu", 1280, 2560)]


@pytest.mark.parametrize("route", REAL, ids=repr)
def test_real_pack_and_unpack_are_under_the_bounds(route):
    h = route.n
    q0 = (route.P or h) // lo.SCH[route.P or h][0]
    a = _run("r2c", route, 2 * h, _r2c(route), q0)
    b = _run("c2r", route, 2 * h, _c2r(route, 2 * h), q0)
    print("real length %d through %r: r2c %s, c2r %s" % (2 * h, route, a, b))
    assert max(a.values()) < 1.0 and max(b.values()) < 1.0, (a, b)
    # the restatements are the transforms they claim to be
    x = np.random.default_rng(0).standard_normal((3, 2 * h))
    assert np.abs(_r2c(route)(x) - np.fft.rfft(x)).max() < 1e-9 * h
    assert np.abs(_c2r(route, 2 * h)(np.fft.rfft(x)) - x).max() < 1e-9


def test_the_bound_of_the_packed_line_holds():
    """||Z||_2 of the packed half-complex line, which bound_c2r takes as 2 (||X_{0..h-1}||_2 + ||X_{1..h}||_2), is
    sqrt(2 H) exactly (H: the squared 2-norm of the Hermitian line) and so below it."""
    rng = np.random.default_rng(3)
    for h in (17, 128, 192):
        X = rng.standard_normal((4, h + 1)) + 1j * rng.standard_normal((4, h + 1))
        Xc = lo.hermitian_clean(X, 2 * h)
        k = np.arange(h)
        w = np.exp(1j * np.pi * k / h)
        Z = (Xc[:, k] + np.conj(Xc[:, h - k])) + 1j * w * (Xc[:, k] - np.conj(Xc[:, h - k]))
        zn = np.sqrt((np.abs(Z) ** 2).sum(axis=1))
        assert np.allclose(zn, np.sqrt(2.0) * lo.herm_norms(X, 2 * h)[1], rtol=1e-12)
        assert (zn <= 2 * (lo.norms(Xc[:, :h])[1] + lo.norms(Xc[:, 1:])[1])).all()


# (defect, kind, route, transform factory, q0): every defect on a scheme that has the step it breaks
def _defect_cases():
    s1024, s384 = lo.Route("sched", 1024), lo.Route("sched", 384)
    b17, b129, b641 = lo.Route("blu", 17, 256), lo.Route("blu", 129, 320), lo.Route("blu", 641, 1536)
    rs, rb = lo.Route("sched", 256, mo=8), lo.Route("blu", 161, 384)
    cases = []
    for r in (b17, b129, b641):
        q0 = r.P // lo.SCH[r.P][0]
        for d in ("chirp", "wrap", "pad", "leak"):
            cases.append((d, "fwd", r, lambda d=d, r=r: _blu(r.n, r.P, -1, d), q0))
            cases.append((d, "inv", r, lambda d=d, r=r: _blu(r.n, r.P, +1, d), q0))
    for r in (s1024, s384):
        q0 = r.n // lo.SCH[r.n][0]
        for d in ("twiddle", "leak"):
            cases.append((d, "fwd", r, lambda d=d, r=r: _c2c(r.n, -1, d), q0))
            cases.append((d, "inv", r, lambda d=d, r=r: _c2c(r.n, +1, d), q0))
    for r in (rs, rb):
        q0 = (r.P or r.n) // lo.SCH[r.P or r.n][0]
        cases.append(("imdc", "c2r", r, lambda r=r: _c2r(r, 2 * r.n, "imdc"), q0))
        cases.append(("noconj", "r2c", r, lambda r=r: _r2c(r, "noconj"), q0))
        cases.append(("leak", "r2c", r, lambda r=r: _r2c(r, "leak"), q0))
        cases.append(("leak", "c2r", r, lambda r=r: _c2r(r, 2 * r.n, "leak"), q0))
    return cases


DEFECTS = _defect_cases()


@pytest.mark.parametrize("case", DEFECTS, ids=lambda c: "%s-%s-%r" % (c[0], c[1], c[2]))
def test_every_planted_defect_is_rejected(case):
    defect, kind, route, make, q0 = case
    n = route.n if kind in ("fwd", "inv") else 2 * route.n
    worst = _run(kind, route, n, make(), q0)
    print("%s on %r (%s): err / bound per family %s" % (defect, route, kind, worst))
    assert max(worst.values()) > 1.0, worst
    if defect == "leak":
        assert worst["scaled"] > 1e50        # a line at 2^-300 next to one at 1: no single scale passes, no leak hides
    if defect == "twiddle" and kind in ("fwd", "inv"):
        assert worst["impulse"] > 1.0        # the 1-norm bound is what keeps the impulse sharp enough for 1e-13


def test_all_seven_defects_are_planted():
    assert {c[0] for c in DEFECTS} == {"chirp", "wrap", "pad", "imdc", "noconj", "twiddle", "leak"}


def test_reference_and_closed_forms():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 255, 256):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        ks = np.arange(n)
        assert np.abs(lo.dft(x, ks) - np.fft.fft(x)).max() < 1e-12 * n
        assert np.abs(lo.dft(x, ks, +1) / n - np.fft.ifft(x)).max() < 1e-12
        r = rng.standard_normal(n)
        X = np.fft.rfft(r) + 0.5j * rng.standard_normal(n // 2 + 1)       # not Hermitian-consistent: numpy ignores it
        assert np.abs(lo.irdft(X, n, ks) - np.fft.irfft(X, n)).max() < 1e-13
        for j in {0, n // 2, n - 1}:
            e = np.zeros(n)
            e[j] = 1.0
            assert np.abs(lo.impulse_spectrum(n, j, ks) - lo.dft(e, ks)).max() < 1e-18
            assert np.abs(np.abs(lo.impulse_spectrum(n, j, ks)) - 1).max() < 1e-18
            t = lo.dft(lo.tone(n, j), ks)
            want = np.zeros(n)
            want[j] = n
            assert np.abs(t - want).max() <= lo.U * n * 1.01
    # the dispatch tables restated in the oracle
    assert [lo.blu_length(n) for n in (16, 17, 128, 129, 160, 161, 2047, 2048, 2049)] == [0, 256, 256, 320, 320, 384, 4096, 4096, 0]


def test_every_gpu_case_sees_every_family_on_neighbouring_lines():
    """The table of tests/test_gpu_linefft.py, without a GPU: over the shapes of every case all four input families, all
    six impulse positions and all three tones occur; wherever an item holds more than one line, some item holds a
    scaled line next to a line of another family; and the largest shape holds all four families on consecutive lines."""
    import test_gpu_linefft as gl

    entries = [(c, gl.shapes_of(c)) for c in gl.CASES]
    entries += [(e[1], [(gl.persistent_shape(e[1], t), 0, 0) for t in gl.persistent_tiles(e[2](256))]) for e in gl.PERSISTENT]
    for case, shapes in entries:
        n = case[1]
        fams, imps, tones, mixed = set(), set(), set(), False
        for shape, offset, rot in shapes:
            nlines = shape[0] * shape[1] if len(shape) == 2 else shape[0]
            plan = lo.line_plan(nlines, n, 0, offset, rot)
            items = gl.items_of(case, shape)
            assert len(items) == nlines
            fams |= {p[0] for p in plan}
            imps |= {p[1] for p in plan if p[0] == "impulse"}
            tones |= {p[1] for p in plan if p[0] == "tone"}
            for l in range(nlines - 1):
                if items[l] == items[l + 1] and "scaled" in (plan[l][0], plan[l + 1][0]) and plan[l][0] != plan[l + 1][0]:
                    mixed = True
        assert fams == set(lo.FAMILIES), (case, fams)
        assert imps == {p[1] for p in lo.line_plan(24, n, 0) if p[0] == "impulse"}, (case, imps)
        assert tones == {min(1, n - 1), n // 2, n - 1}, (case, tones)
        assert mixed or gl.table_route(case).nch == 1, case
        big = max(shapes, key=lambda s: s[0][0] * (s[0][1] if len(s[0]) == 2 else 1))
        assert (big[0][0] * (big[0][1] if len(big[0]) == 2 else 1)) >= gl.MIN_LINES, (case, big)
