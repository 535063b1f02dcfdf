"""GPU: every device pass against its reference on a poisoned pool.

KS_DEBUG_POOL_FILL=<byte> makes the context's pool fill every block it hands out, so a pass that reads a word it never wrote (a flag,
a counter, a head bitmap, a first-offender slot, one element past what an earlier kernel wrote) reads the same poison on a fresh
block as on a recycled one.  255 makes a stale flag true, a stale count huge and a stale first-offender word "none"; 0 makes a slot
that was meant to start at all ones (a running minimum, an unset id) read as set.

1. the knob does what it says: the slack of a recycled and of a fresh block holds the fill, and what the block held before without it;
2. the table of tests/pool_fill_cases.py: the suite's own reference-compared tests, called with poisoned contexts;
3. nothing left out: the entry points called while the table ran, against the header."""
import ctypes as C
import inspect
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_fill_cases as PF  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib  # noqa: E402

ENV = PF.ENV
N, RUNS = 1000, 250  # 8000 bytes of hashes: a size class of its own next to the 4000 bytes of abundances and the offsets
OLD = np.uint64(0xA5A5A5A500000000) + np.arange(1, N + 1, dtype=np.uint64)
SHARED = np.arange(1, RUNS + 1, dtype=np.uint64) << np.uint64(20)


# ---- 1. the knob ---------------------------------------------------------------------------------------------------------------------
def download(ctx, d_ptr, n, dtype):
    got = np.zeros(n, dtype)
    ctx._check(ctx._L.ks_dev_download(ctx._h, got.ctypes.data_as(C.c_void_p), C.c_void_p(int(d_ptr)), got.nbytes))
    return got


def union_slack(ctx):
    """A union by group whose output hash array is sized by its N input hashes and written for RUNS of them, twice: on blocks the
    pool has to make, then on the block a column fully written by sketches_from_host (OLD) held until it was freed.  Returns for
    each the N words of the output array and the pool's hipMalloc calls during the pass; for the second also whether the block is
    the freed one."""
    four = ctx.sketches_from_host(np.arange(0, N + 1, RUNS), np.tile(SHARED, N // RUNS), np.ones(N, np.uint32), 10, 1, "protein")
    out = {}
    m0 = ctx.pool_stats()["mallocs"]
    U = four.union_groups([0, N // RUNS])
    assert U.n_hashes == RUNS
    out["fresh"] = (download(ctx, U.device_ptrs()[1], N, np.uint64), ctx.pool_stats()["mallocs"] - m0)
    U.free()  # (the pool now holds every block the pass takes)
    full = ctx.sketches_from_host([0, N], OLD, np.ones(N, np.uint32), 10, 1, "protein")
    held = full.device_ptrs()[1]
    assert np.array_equal(download(ctx, held, N, np.uint64), OLD)
    full.free()
    m0 = ctx.pool_stats()["mallocs"]
    U = four.union_groups([0, N // RUNS])
    assert U.n_hashes == RUNS
    out["reused"] = (download(ctx, U.device_ptrs()[1], N, np.uint64), ctx.pool_stats()["mallocs"] - m0, U.device_ptrs()[1] == held)
    U.free(); four.free()
    return out


@pytest.mark.parametrize("fill", PF.FILLS)
def test_slack_of_a_recycled_and_of_a_fresh_block_holds_the_fill(monkeypatch, fill):
    monkeypatch.setenv(ENV, str(fill))
    with ks.Context(0) as ctx:
        monkeypatch.delenv(ENV)  # (read when the context was made)
        got = union_slack(ctx)
    poison = np.full(N - RUNS, fill * 0x0101010101010101, np.uint64)
    words, mallocs = got["fresh"]
    assert mallocs > 0 and np.array_equal(words[:RUNS], SHARED)
    assert np.array_equal(words[RUNS:], poison), "a block straight from hipMalloc was handed out unfilled"
    words, mallocs, same = got["reused"]
    assert mallocs == 0 and same, "the output did not take the freed block: the reuse path is not the one tested"
    assert np.array_equal(words[:RUNS], SHARED)
    assert np.array_equal(words[RUNS:], poison), "a recycled block was handed out unfilled"


@pytest.mark.parametrize("value", [None, "256", "-1", "x", "", "12x", "0x10"])
def test_without_the_knob_the_slack_holds_what_the_block_held_before(monkeypatch, value):
    """... or the test above proves nothing; and a value that is no integer in 0..255 counts as unset."""
    if value is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, value)
    with ks.Context(0) as ctx:
        got = union_slack(ctx)
    words, mallocs, same = got["reused"]
    assert mallocs == 0 and same
    assert np.array_equal(words[:RUNS], SHARED) and np.array_equal(words[RUNS:], OLD[RUNS:])


def test_follow_debug_env_switches_the_fill_per_call(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    with ks.Context(0, follow_debug_env=True) as ctx:
        assert np.array_equal(union_slack(ctx)["reused"][0][RUNS:], OLD[RUNS:])
        monkeypatch.setenv(ENV, "255")
        assert np.array_equal(union_slack(ctx)["reused"][0][RUNS:], np.full(N - RUNS, 2 ** 64 - 1, np.uint64))
        monkeypatch.setenv(ENV, "0")
        assert not union_slack(ctx)["reused"][0][RUNS:].any()


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------------
class Recorder:
    """The library handle with the name of every ks_* function called through it written down."""

    def __init__(self, L, names):
        self._L, self._names = L, names

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("ks_"):
            return f
        names = self._names

        def call(*a):
            names.add(name)
            return f(*a)
        return call


class Poisoned:
    """One fill value: the module-scoped fixtures of the suite made under it (each module's `ctx` among them), what ran and what
    was called."""

    def __init__(self, fill):
        self.fill, self.called, self.ran, self.cache, self.finalizers = fill, set(), set(), {}, []
        self.lib = Recorder(_lib.load(), self.called)

    def close(self):
        for fin in reversed(self.finalizers):
            fin()


def _finish(gen):
    def fin():
        for _ in gen:
            raise RuntimeError("a fixture yielded twice")
    return fin


class Call:
    """The arguments of one test function, from the same places pytest takes them: the parameter set, pytest's own fixtures,
    tests/conftest.py, and the fixtures of the test's module — its `ctx` too — made here from their plain functions while the
    variable is set, kept for the fill value where they are module-scoped, and finished the way the module finishes them (a
    module that caches device objects of its context drops them there)."""

    def __init__(self, pool, module, request, monkeypatch, tmp_path, fparams):
        self.pool, self.module, self.request, self.fparams = pool, module, request, fparams
        self.own = {"monkeypatch": monkeypatch, "tmp_path": tmp_path}
        self.after = []

    def value(self, name):
        if name in self.own:
            return self.own[name]
        fx = getattr(self.module, name, None)
        if not PF.is_fixture(fx):
            return self.request.getfixturevalue(name)
        marker, key = PF.fixture_marker(fx), (self.module.__name__, name)
        shared = marker.scope in ("module", "session", "package") and marker.params is None
        if shared and key in self.pool.cache:
            return self.pool.cache[key]
        f = PF.fixture_function(fx)
        kw = {a: types.SimpleNamespace(param=self.fparams.get(name)) if a == "request" else self.value(a) for a in inspect.signature(f).parameters}
        v = f(**kw)
        if inspect.isgenerator(v):
            gen, v = v, next(v)
            (self.pool.finalizers if shared else self.after).append(_finish(gen))
        if shared:
            self.pool.cache[key] = v
        return v

    def run(self, fn, kw):
        try:
            args = {a: kw[a] if a in kw else self.value(a) for a in inspect.signature(fn).parameters}
            fn(**args)
        finally:
            for fin in reversed(self.after):
                fin()


@pytest.fixture(scope="module", params=PF.FILLS, ids=lambda f: f"fill{f}")
def pool(request):
    p = Poisoned(request.param)
    yield p
    p.close()


TABLE = PF.expand()


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_on_a_poisoned_pool(pool, case, request, monkeypatch, tmp_path):
    cid, module, function, pset = case
    mod = PF.load(module)
    fn = getattr(mod, function)
    kw, fparams = PF.resolve(mod, fn, pset)
    pool.ran.add(cid)
    monkeypatch.setenv(ENV, str(pool.fill))          # every context made from here on is poisoned; one that follows the variables stays so
    monkeypatch.setattr(_lib, "_lib", pool.lib)      # ... and the calls of every context made from here on are written down
    Call(pool, mod, request, monkeypatch, tmp_path, fparams).run(fn, kw)


# ---- 3. nothing left out ---------------------------------------------------------------------------------------------------------------
def test_every_entry_point_that_can_allocate_ran_on_a_poisoned_pool(pool):
    if pool.ran != {c[0] for c in TABLE}:
        pytest.skip("the table did not run as a whole (a selection): what it reaches is checked on a full run of the file")
    exempt = PF.exempt()
    missing = sorted(set(PF.declared()) - set(exempt) - pool.called)
    assert not missing, f"no case of tests/pool_fill_cases.py calls {missing} (fill {pool.fill}): add one, or exempt it with a reason"
