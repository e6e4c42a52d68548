"""Who ends the numpy-stream draw session and who releases the generator's lock (cora_amd/core/skysim.py:
prepare_numpy_stream, _PreparedStream, draw_numpy_stream, mkfullsky_device's shape check) - on a stub context, no GPU."""
import gc

import numpy as np
import pytest

from cora_amd import _lib
from cora_amd.core import skysim

MAXL, NUMZ = 7, 3


class FakeSession:
    """The states of ``_lib.DrawSession`` (prepared -> ran -> ended) with the library's calls counted: ``ends`` is the
    number of ``corahip_draw_alm_numpy_end`` calls the real session would have made."""

    def __init__(self, ctx, spec):
        self.ctx, self.spec, self.state = ctx, spec, "prepared"
        self.runs = self.finishes = self.aborts = self.ends = 0

    def run(self, T, info, lmax, F, **kw):
        self.runs += 1
        assert self.state == "prepared" and (lmax, F) == (MAXL, NUMZ)
        if self.ctx.fail_run is not None:
            self.state, self.ends = "ended", self.ends + 1         # (a run that raises ends the session itself)
            raise self.ctx.fail_run
        self.state, self.kw = "ran", kw
        return "alm"

    def finish(self):
        self.finishes += 1
        assert self.state == "ran"
        self.state, self.ends = "ended", self.ends + 1
        return self.ctx.after

    def abort(self):
        self.aborts += 1
        if self.state != "ended":
            self.state, self.ends = "ended", self.ends + 1


class StubContext:
    """``draw_alm_numpy_prepare`` of ``_lib.Context``: hands out FakeSessions, or raises ``fail_prepare``."""

    def __init__(self):
        self.sessions, self.fail_prepare, self.fail_run, self.after = [], None, None, None

    def draw_alm_numpy_prepare(self, rng, lmax, F, ring_bytes=0):
        if self.fail_prepare is not None:
            raise self.fail_prepare
        self.sessions.append(FakeSession(self, rng))
        return self.sessions[-1]


def _status(code):
    e = _lib.CoraHipError("libcorahip status %d" % code)
    e.status = code
    return e


@pytest.fixture(params=["pcg64", "randomstate", "global"])
def gen(request):
    """(rng as the caller passes it, its twin, the lock numpy's draws hold, draw(n) of rng, state `moved`)."""
    saved = np.random.get_state()
    if request.param == "pcg64":
        rng, twin, moved = np.random.default_rng(11), np.random.default_rng(11), np.random.default_rng(11)
        moved.standard_normal(9)
        lock, draw, after = rng.bit_generator.lock, rng.standard_normal, moved.bit_generator.state["state"]["state"]
    else:
        twin, moved = np.random.RandomState(12), np.random.RandomState(12)
        moved.standard_normal(9)
        after = moved.get_state(legacy=False)
        if request.param == "randomstate":
            rng = np.random.RandomState(12)
            draw = rng.standard_normal
        else:
            np.random.seed(12)
            rng, draw = None, np.random.standard_normal
        lock = skysim._legacy_state_of(rng)[2]
    yield rng, twin, lock, draw, (moved, after)
    np.random.set_state(saved)


def _lock_is_free(lock):
    got = lock.acquire(False)
    if got:
        lock.release()
    return got


@pytest.mark.parametrize("ahead", [False, True])
@pytest.mark.parametrize("defer", [False, True])
def test_success_finishes_once_frees_the_lock_and_writes_the_state_back(gen, ahead, defer):
    rng, _twin, lock, draw, (moved, after) = gen
    ctx = StubContext()
    ctx.after = after
    prep = skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ) if ahead else None
    if ahead:
        assert prep is not None and not _lock_is_free(lock)
    got = skysim.draw_numpy_stream(ctx, "T", "info", rng, MAXL, NUMZ, nu0=1, nnu=2, defer=defer, prepared=prep)
    (s,) = ctx.sessions
    assert s.spec[0] == ("pcg64" if isinstance(rng, np.random.Generator) else "legacy")
    assert s.kw == dict(nu0=1, nnu=2, out=None, rows=False, chunks=None)
    if defer:
        alm, finish = got
        assert (s.runs, s.finishes, s.ends) == (1, 0, 0) and not _lock_is_free(lock)
        finish()
    else:
        alm = got
    assert alm == "alm"
    assert (s.runs, s.finishes, s.ends) == (1, 1, 1)
    assert _lock_is_free(lock)
    assert np.array_equal(draw(5), moved.standard_normal(5))         # the generator is where the session left it


@pytest.mark.parametrize("ahead", [False, True])
@pytest.mark.parametrize("error", [AssertionError((8, 3, 3)), _status(-1), MemoryError("a_lm")])
def test_a_failed_run_ends_the_session_once_and_leaves_lock_and_generator(gen, ahead, error):
    rng, twin, lock, draw, _ = gen
    ctx = StubContext()
    ctx.fail_run = error
    prep = skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ) if ahead else None
    with pytest.raises(type(error)):
        skysim.draw_numpy_stream(ctx, "T", "info", rng, MAXL, NUMZ, defer=True, prepared=prep)
    (s,) = ctx.sessions
    assert (s.runs, s.finishes, s.ends) == (1, 0, 1)
    assert _lock_is_free(lock)
    assert np.array_equal(draw(5), twin.standard_normal(5))
    if prep is not None:
        prep.abort()                                                  # (what a caller's own error path may still do)
        assert s.ends == 1 and _lock_is_free(lock)


def test_abort_twice_is_harmless(gen):
    rng, twin, lock, draw, _ = gen
    ctx = StubContext()
    prep = skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ)
    assert not _lock_is_free(lock)
    prep.abort()
    prep.abort()
    (s,) = ctx.sessions
    assert (s.runs, s.finishes, s.ends) == (0, 0, 1)
    assert _lock_is_free(lock)
    assert np.array_equal(draw(5), twin.standard_normal(5))


def test_a_state_error_at_prepare_gives_none_with_the_lock_free(gen):
    rng, twin, lock, draw, _ = gen
    ctx = StubContext()
    ctx.fail_prepare = _status(_lib.CORAHIP_ESTATE)
    assert _lib.CORAHIP_ESTATE == -3
    assert skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ) is None
    assert _lock_is_free(lock)
    # every other status is raised as it is - with the lock free as well
    ctx.fail_prepare = _status(-2)
    with pytest.raises(_lib.CoraHipError) as e:
        skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ)
    assert e.value.status == -2
    assert _lock_is_free(lock) and ctx.sessions == []
    assert np.array_equal(draw(5), twin.standard_normal(5))


def test_a_dropped_prepared_stream_ends_its_session(gen):
    rng, twin, lock, draw, _ = gen
    ctx = StubContext()
    prep = skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ)
    assert not _lock_is_free(lock)
    del prep
    gc.collect()
    (s,) = ctx.sessions
    assert (s.runs, s.finishes, s.ends) == (0, 0, 1)
    assert _lock_is_free(lock)
    assert np.array_equal(draw(5), twin.standard_normal(5))


def test_mkfullsky_device_gives_a_prepared_session_up_on_its_shape_error(gen, monkeypatch):
    rng, twin, lock, draw, _ = gen
    ctx = StubContext()
    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: ctx)
    prep = skysim.prepare_numpy_stream(ctx, rng, MAXL, NUMZ)
    with pytest.raises(Exception, match="Correlation matrix is incorrect shape"):
        skysim.mkfullsky_device(np.zeros((MAXL + 1, NUMZ, NUMZ + 1)), 4, rng=rng, prepared=prep)
    (s,) = ctx.sessions
    assert (s.runs, s.finishes, s.ends) == (0, 0, 1)
    assert _lock_is_free(lock)
    assert np.array_equal(draw(5), twin.standard_normal(5))


# ------------------------------------------------------------------ _lib.DrawSession on a recording library
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


class RecordingLib:
    """The three entry points a DrawSession calls; ``run_rc``: the status ``corahip_draw_alm_numpy_run`` returns."""

    def __init__(self, run_rc=0):
        self.calls, self.run_rc = [], run_rc

    def corahip_draw_alm_numpy_prepare(self, h, r, lmax, F, ring_bytes, pend):
        self.calls.append("prepare")
        return 0

    def corahip_draw_alm_numpy_run(self, *a):
        self.calls.append("run")
        return self.run_rc

    def corahip_draw_alm_numpy_end(self, h, pend, r):
        self.calls.append("end")
        return 0


class LibContext:
    h = None

    def __init__(self, lib, oom=False):
        self.lib, self.oom = lib, oom

    def _alm_out(self, lmax, nnu, out=None):
        if self.oom:
            raise MemoryError("a_lm")
        return "alm"

    def _f64(self, t):
        return None

    _p0 = _f64


_SPEC = ("pcg64", 5 << 70 | 3, 9)


def test_draw_session_ends_once_after_finish_abort_and_drop():
    lib = RecordingLib()
    s = _lib.DrawSession(LibContext(lib), _SPEC, 4, 2)
    assert s.run(_Shape(5, 2, 2), None, 4, 2) == "alm" and s.state == "ran"
    assert s.finish() == _SPEC[1]                                     # (the recording _end leaves the struct as it was)
    s.abort()
    del s
    gc.collect()
    assert lib.calls == ["prepare", "run", "end"]
    s = _lib.DrawSession(LibContext(lib), _SPEC, 4, 2)
    s.abort()
    s.abort()
    assert lib.calls[3:] == ["prepare", "end"]
    s = _lib.DrawSession(LibContext(lib), _SPEC, 4, 2)
    del s
    gc.collect()
    assert lib.calls[5:] == ["prepare", "end"]


@pytest.mark.parametrize("case", ["other shape", "T shape", "allocation", "status"])
def test_draw_session_run_that_raises_ends_the_session(case, monkeypatch):
    lib = RecordingLib(run_rc=-1 if case == "status" else 0)
    monkeypatch.setattr(_lib, "load", lambda: type("L", (), {"corahip_last_error": staticmethod(lambda: b"refused")}))
    s = _lib.DrawSession(LibContext(lib, oom=case == "allocation"), _SPEC, 4, 2)
    T = _Shape(5, 3, 2) if case == "T shape" else _Shape(5, 2, 2)
    error = {"allocation": MemoryError, "status": _lib.CoraHipError}.get(case, AssertionError)
    with pytest.raises(error):
        s.run(T, None, 5 if case == "other shape" else 4, 2)
    assert lib.calls == ["prepare"] + (["run"] if case == "status" else []) + ["end"]
    s.abort()
    del s
    gc.collect()
    assert lib.calls[-1] == "end" and lib.calls.count("end") == 1
