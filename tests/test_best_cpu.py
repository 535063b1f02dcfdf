"""CPU-side checks of ks_hits_best: the numpy restatement (tests/best_ref.py) on hand-written rows, the new symbols with the
prototypes _lib.py declares, the refusals that need no device (no context), the option words Context.best_hits builds, and the
wire entry points' old path with top_k = 0.  No GPU compute here."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_ref  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ks_hits_best", "ks_hits_device_rank", "ks_hits_device_src_row", "ks_hits_copy_best_to_host"]
NAN, INF = math.nan, math.inf


@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_ties_at_the_cut_go_to_the_smaller_tid():
    qid = [0] * 6 + [2] * 3
    tid = [1, 3, 4, 7, 8, 9, 0, 5, 6]
    score = [2.0, 5.0, 2.0, 5.0, 2.0, 1.0, 1.0, 1.0, 1.0]
    kept, rank = best_ref.best(qid, tid, score, 3)
    assert rank.tolist() == [2, 0, 3, 1, 4, 5, 0, 1, 2]
    assert kept.tolist() == [True, True, False, True, False, False, True, True, True]
    kept, rank = best_ref.best(qid, tid, score, 1)
    assert kept.tolist() == [False, True, False, False, False, False, True, False, False]
    kept, rank2 = best_ref.best(qid, tid, score, 6)  # k >= every length: all rows, the same ranks
    assert kept.all() and np.array_equal(rank, rank2)
    kept, _ = best_ref.best(qid, tid, score, 2 ** 32 - 1)
    assert kept.all()


def test_reference_orders_nan_infinities_and_zeros():
    tid = list(range(9))
    score = [NAN, -INF, -1.5, -0.0, 0.0, 1e-300, 2.0, INF, float.fromhex("-0x1.8p+0") * NAN]
    kept, rank = best_ref.best([5] * 9, tid, score, 4)
    #             NaN -inf -1.5 -0.0 +0.0 1e-300 2.0 inf NaN
    assert rank.tolist() == [7, 6, 5, 3, 4, 2, 1, 0, 8]  # -0.0 ties +0.0 (tid decides), NaNs tie each other below -inf
    assert kept.tolist() == [False, False, False, True, False, True, True, True, False]
    kept, rank = best_ref.best([0, 0, 0], [4, 2, 9], [NAN, NAN, NAN], 2)  # all NaN: the smallest tids
    assert rank.tolist() == [1, 0, 2] and kept.tolist() == [True, True, False]
    assert best_ref.best([], [], [], 3)[0].shape == (0,)


def test_reference_scores():
    Q = (np.array([0, 4, 4, 10], np.uint64), np.arange(10, dtype=np.uint64), np.ones(10, np.uint32))
    T = (np.array([0, 3, 12], np.uint64), np.arange(12, dtype=np.uint64), np.ones(12, np.uint32))
    qid, tid, isect = [0, 0, 2], [0, 1, 1], [3, 2, 5]
    assert best_ref.scores("intersect", qid, tid, isect).tolist() == [3.0, 2.0, 5.0]
    assert best_ref.scores("target_containment", qid, tid, isect, T=T).tolist() == [3 / 3, 2 / 9, 5 / 9]
    assert best_ref.scores("max_containment", qid, tid, isect, Q, T).tolist() == [3 / 3, 2 / 4, 5 / 6]
    assert best_ref.scores("jaccard", qid, tid, isect, Q, T).tolist() == [3 / 4, 2 / 11, 5 / 10]
    src, rank = best_ref.best_rows("jaccard", qid, tid, isect, 1, Q, T)
    assert src.tolist() == [0, 2] and rank.tolist() == [0, 0]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return m.group(1).split()[-1], len([p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"])


def test_new_symbols_exported_with_declared_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        ret, n_params = _prototype(name)
        assert len(args) == n_params, (name, len(args), n_params)
        assert (res is C.c_int) == (ret == "int"), (name, ret)
    assert C.sizeof(_lib.ks_best_opts) == 16
    assert [f[0] for f in _lib.ks_best_opts._fields_] == ["rank_by", "k", "flags", "reserved"]
    assert (_lib.KS_BEST_INTERSECT, _lib.KS_BEST_TARGET_CONTAINMENT, _lib.KS_BEST_MAX_CONTAINMENT, _lib.KS_BEST_JACCARD,
            _lib.KS_BEST_SCORE) == (0, 1, 2, 3, 4)
    header = open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read()
    for name, v in (("INTERSECT", 0), ("TARGET_CONTAINMENT", 1), ("MAX_CONTAINMENT", 2), ("JACCARD", 3), ("SCORE", 4)):
        assert re.search(r"#define KS_BEST_" + name + r"\s+" + str(v) + r"u\b", header), name


SOME = C.c_void_p(64)  # a non-NULL pointer the option checks never follow

# (rank_by, k, flags, reserved), queries, targets, d_score
REFUSED = [
    ((0, 0, 0, 0), None, None, None),        # k == 0
    ((5, 3, 0, 0), None, None, None),        # unknown rank_by
    ((0xffffffff, 3, 0, 0), None, None, None),
    ((0, 3, 1, 0), None, None, None),        # flags
    ((0, 3, 0, 9), None, None, None),        # reserved
    ((4, 3, 0, 0), None, None, None),        # KS_BEST_SCORE without a column
    ((0, 3, 0, 0), None, None, SOME),        # a column without KS_BEST_SCORE
    ((3, 3, 0, 0), SOME, SOME, SOME),
    ((1, 3, 0, 0), SOME, None, None),        # a needed set NULL
    ((2, 3, 0, 0), None, SOME, None),
    ((2, 3, 0, 0), SOME, None, None),
    ((3, 3, 0, 0), None, SOME, None),
    ((3, 3, 0, 0), None, None, None),
    None,                                    # opts == NULL
    ((0, 3, 0, 0), None, None, None),        # fine options, but no context
]


@pytest.mark.parametrize("case", REFUSED)
def test_refusals_without_a_context_leave_out_null(lib, case):
    out = C.c_void_p(12345)
    if case is None:
        st = lib.ks_hits_best(None, None, None, None, None, None, C.byref(out))
    else:
        words, q, t, score = case
        st = lib.ks_hits_best(None, None, q, t, score, C.byref(_lib.ks_best_opts(*words)), C.byref(out))
    assert st == _lib.KS_ERR_INVALID_ARG
    assert not out.value
    if case is not None:
        assert lib.ks_hits_best(None, None, case[1], case[2], case[3], C.byref(_lib.ks_best_opts(*case[0])), None) == _lib.KS_ERR_INVALID_ARG


def test_accessors_accept_null(lib):
    assert not lib.ks_hits_device_rank(None) and not lib.ks_hits_device_src_row(None)
    assert lib.ks_hits_copy_best_to_host(None, None, None, None) == _lib.KS_ERR_INVALID_ARG


# ---- engine -------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the loaded library: records which entry point a Context method called, and with what arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            opts = None
            for a in args:
                obj = getattr(a, "_obj", None)
                if isinstance(obj, _lib.ks_best_opts):
                    opts = (obj.rank_by, obj.k, obj.flags, obj.reserved)
            ptrs = [None if a is None else getattr(a, "value", None) for a in args[1:5]] if name == "ks_hits_best" else None
            self.calls.append((name, opts, ptrs))
            return _lib.KS_OK
        return call


def _fake_context():
    ctx = engine.Context.__new__(engine.Context)
    ctx._L = _Recorder()
    ctx._h = C.c_void_p(1)
    ctx._pinned, ctx._close_pending = 0, True  # (never destroys anything)
    return ctx


class _Tensor:
    def data_ptr(self):
        return 4096


def test_best_hits_maps_its_keywords_to_the_option_words(monkeypatch):
    monkeypatch.setattr(engine.Hits, "__del__", lambda self: None, raising=False)
    monkeypatch.setattr(engine.Sketches, "__del__", lambda self: None, raising=False)
    ctx = _fake_context()
    hits = engine.Hits.__new__(engine.Hits)
    q, t = engine.Sketches.__new__(engine.Sketches), engine.Sketches.__new__(engine.Sketches)
    hits._h, q._h, t._h = C.c_void_p(2), C.c_void_p(3), C.c_void_p(5)

    ctx.best_hits(hits, 10)
    ctx.best_hits(hits, 1, "target_containment", targets=t)
    ctx.best_hits(hits, 2 ** 32 - 1, "max_containment", q, t)
    ctx.best_hits(hits, 7, rank_by="jaccard", queries=q, targets=t)
    ctx.best_hits(hits, 5, score=8192)                 # rank_by left at its default: score
    ctx.best_hits(hits, 5, "score", score=_Tensor())   # anything with data_ptr()
    assert ctx._L.calls == [
        ("ks_hits_best", (0, 10, 0, 0), [2, None, None, None]),
        ("ks_hits_best", (1, 1, 0, 0), [2, None, 5, None]),
        ("ks_hits_best", (2, 2 ** 32 - 1, 0, 0), [2, 3, 5, None]),
        ("ks_hits_best", (3, 7, 0, 0), [2, 3, 5, None]),
        ("ks_hits_best", (4, 5, 0, 0), [2, None, None, 8192]),
        ("ks_hits_best", (4, 5, 0, 0), [2, None, None, 4096]),
    ]
    with pytest.raises(ValueError):
        ctx.best_hits(hits, 3, "containment")
    with pytest.raises(ValueError):
        ctx.best_hits(hits, 2 ** 32)
    assert sorted(engine.BEST_RANK_BY) == sorted(best_ref.RANK_BY)
    assert callable(engine.Hits.best_to_host)
    assert isinstance(engine.Significance.tf_idf_ptr, property) and isinstance(engine.Significance.prob_overlap_ptr, property)


# ---- wire ---------------------------------------------------------------------------------------------------------------------
class _WireContext:
    """A context whose search finds nothing; best_hits must not be reached with top_k = 0."""

    def __init__(self):
        self.calls = []

    def sketches_from_host(self, *a):
        self.calls.append("sketches_from_host")
        return self

    def index_build(self, t):
        self.calls.append("index_build")
        return self

    def search(self, ix, q):
        self.calls.append("search")
        return self

    def best_hits(self, *a, **kw):
        self.calls.append("best_hits")
        return self

    def to_host(self):
        return (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint64))


def test_do_manysearch_with_top_k_0_takes_the_old_path(monkeypatch, tmp_path):
    sig = (["a"], np.array([0, 1], np.uint64), np.array([7], np.uint64), np.array([1], np.uint32), 16, 5, "hp")
    monkeypatch.setattr(wire, "read_sig_zip", lambda path: sig)
    ctx = _WireContext()
    out = tmp_path / "o.csv"
    assert wire.do_manysearch("q", "t", str(out), 16, 5, "hp", ctx=ctx) == 0
    assert wire.do_manysearch("q", "t", str(out), 16, 5, "hp", ctx=ctx, top_k=0, rank_by="jaccard") == 0
    assert "best_hits" not in ctx.calls and ctx.calls.count("search") == 2
    assert open(out).read().strip() == ",".join(wire.MANYSEARCH_COLUMNS)
    assert wire.do_manysearch("q", "t", str(out), 16, 5, "hp", ctx=ctx, top_k=3) == 0
    assert ctx.calls[-1] == "best_hits"
    import inspect
    for f in (wire.do_manysearch, wire.do_multisearch):
        p = inspect.signature(f).parameters
        assert p["top_k"].default == 0 and p["rank_by"].default == "intersect"
