"""No GPU: the host restatement of ks_hits_gather (tests/gather_ref.py) against an independent version on Python sets and
against the invariants of the contract, over seeded random small instances; the text of wire.gather_rows on a hand-made result;
the layout of ks_gather_opts; the option checks of ks_hits_gather that need no device."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import gather_ref  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ks_hits_gather", "ks_hits_device_unique_intersect", "ks_hits_device_remaining", "ks_hits_device_unique_weighted",
               "ks_hits_copy_gather_to_host"]


def _instance(seed):
    """a small random (Q, T, rows): queries and targets draw from a pool of 40 hashes, so targets overlap heavily"""
    rng = np.random.default_rng([2024, seed])
    n_q, n_t = int(rng.integers(1, 6)), int(rng.integers(1, 12))
    pool = np.arange(1, 41, dtype=np.uint64) * np.uint64(1000003)

    def draw(n, lo, hi):
        seq, h = [], []
        for s in range(n):
            m = int(rng.integers(lo, hi))
            seq += [s] * m; h += rng.choice(pool, m, replace=False).tolist()
        return seq, h

    qs, qh = draw(n_q, 0, 30)
    ts, th = draw(n_t, 0, 20)
    Q = cs._csr(qs, qh, rng.integers(1, 9, len(qh)), n_q)
    T = cs._csr(ts, th, np.ones(len(th)), n_t)
    return Q, T, cs.ref_join(T, Q)


SEEDS = list(range(60))


@pytest.mark.parametrize("opts", [(1, 0), (0, 0), (2, 0), (5, 0), (1, 1), (1, 2), (3, 3)])
def test_reference_agrees_with_the_version_on_sets(opts):
    some = 0
    for seed in SEEDS:
        Q, T, rows = _instance(seed)
        a = gather_ref.gather(Q, T, rows[0], rows[1], rows[2], *opts)
        b = gather_ref.gather_sets(Q, T, rows[0], rows[1], rows[2], *opts)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), (seed, opts)
        some += len(a[0])
    assert some > 100


def test_reference_invariants():
    dropped = 0
    for seed in SEEDS:
        Q, T, rows = _instance(seed)
        qid, tid, isect = rows[0], rows[1], rows[2]
        src, rank, uniq, rem, uw = gather_ref.gather(Q, T, qid, tid, isect)
        assert np.all(src[1:] > src[:-1])  # row order: (qid, tid) order
        dropped += len(qid) - len(src)
        for q in np.unique(qid).tolist():
            seg = np.nonzero(qid == q)[0]
            mine = np.nonzero(qid[src] == q)[0]
            o = mine[np.argsort(rank[mine])]
            assert rank[o].tolist() == list(range(len(o))) and len(o) >= 1  # 0, 1, 2 ... without gaps
            assert np.all(uniq[o][1:] <= uniq[o][:-1])  # non-increasing in rank
            first = src[o[0]]
            assert uniq[o[0]] == isect[first] == isect[seg].max()
            assert first == seg[np.argmax(isect[seg])]  # of equal intersects the smaller tid
            nq = int(Q[0][q + 1] - Q[0][q])
            assert int(uniq[o].sum()) + int(rem[o[-1]]) == nq
            assert np.array_equal(rem[o], nq - np.cumsum(uniq[o]))
            assert np.all(uw[o] >= uniq[o])  # abundances are >= 1 here
    assert dropped > 50  # (the instances do hold redundant targets)


def test_reference_on_the_order_case_of_the_contract():
    """A holds 10 hashes, B 9 of which 8 are A's, C 5 of its own: ranks A, C, B with 10, 5, 1 new hashes."""
    h = np.arange(1, 17, dtype=np.uint64)
    A, B, Cc = h[:10], np.concatenate([h[2:10], h[10:11]]), h[11:16]
    Q = cs._csr([0] * 16, h, np.arange(1, 17), 1)
    T = cs._csr([0] * 10 + [1] * 9 + [2] * 5, np.concatenate([A, B, Cc]), np.ones(24), 3)
    rows = cs.ref_join(T, Q)
    assert rows[2].tolist() == [10, 9, 5]
    src, rank, uniq, rem, uw = gather_ref.gather(Q, T, rows[0], rows[1], rows[2])
    assert (src.tolist(), rank.tolist(), uniq.tolist(), rem.tolist()) == ([0, 1, 2], [0, 2, 1], [10, 1, 5], [6, 0, 1])
    assert uw.tolist() == [sum(range(1, 11)), 11, sum(range(12, 17))]
    src, rank, uniq, rem, uw = gather_ref.gather(Q, T, rows[0], rows[1], rows[2], 2, 0)  # B's single new hash is too few
    assert (src.tolist(), rank.tolist()) == ([0, 2], [0, 1])
    src, rank, _, _, _ = gather_ref.gather(Q, T, rows[0], rows[1], rows[2], 1, 1)
    assert (src.tolist(), rank.tolist()) == ([0], [0])
    with pytest.raises(AssertionError):
        gather_ref.gather(Q, T, rows[0], rows[1], np.array([10, 8, 5], np.uint32))  # an intersect that is not the sketches'


# ---- wire ----------------------------------------------------------------------------------------------------------------------
def test_gather_rows_text():
    q_names, t_names = ["q zero", "q1"], ["t0", "t1", "t2"]
    q_off = np.array([0, 4, 7], np.uint64)
    q_mins = np.array([10, 20, 30, 40, 10, 50, 60], np.uint64)
    q_ab = np.array([1, 2, 3, 4, 5, 5, 5], np.uint32)
    t_off = np.array([0, 3, 5, 6], np.uint64)
    t_mins = np.array([10, 20, 99, 30, 40, 50], np.uint64)
    # rows in (qid, tid) order; query 0 kept t1 first (rank 0), then t0
    hits = (np.array([0, 0, 1], np.uint32), np.array([0, 1, 2], np.uint32), np.array([2, 2, 1], np.uint32), np.zeros(3, np.uint64))
    rank = np.array([1, 0, 0], np.uint32)
    gathered = (np.array([2, 2, 1], np.uint32), np.array([0, 2, 2], np.uint32), np.array([3, 7, 5], np.uint64))
    rows = wire.gather_rows(q_names, q_off, q_mins, q_ab, t_names, t_off, t_mins, hits, rank, gathered, 16, 5, "hp")
    assert [list(r) for r in rows] == [wire.GATHER_COLUMNS] * 3
    assert wire.GATHER_COLUMNS == ["query_name", "query_md5", "match_name", "match_md5", "gather_result_rank", "intersect_bp",
                                   "unique_intersect_bp", "remaining_bp", "f_orig_query", "f_unique_to_query", "f_match", "f_match_orig",
                                   "f_unique_weighted", "average_abund", "ksize", "scaled", "moltype"]
    assert [(r["query_name"], r["match_name"], r["gather_result_rank"]) for r in rows] == [("q zero", "t1", 0), ("q zero", "t0", 1), ("q1", "t2", 0)]
    a, b, c = rows
    assert (a["intersect_bp"], a["unique_intersect_bp"], a["remaining_bp"]) == (10, 10, 10)
    assert (b["intersect_bp"], b["unique_intersect_bp"], b["remaining_bp"]) == (10, 10, 0)
    assert (c["intersect_bp"], c["unique_intersect_bp"], c["remaining_bp"]) == (5, 5, 10)
    assert (a["f_orig_query"], a["f_unique_to_query"], a["f_match"], a["f_match_orig"]) == ("0.5", "0.5", "1.0", "1.0")
    assert (a["f_unique_weighted"], a["average_abund"]) == ("0.7", "3.5")
    assert (b["f_match"], b["f_match_orig"], b["f_unique_weighted"], b["average_abund"]) == ("0.6666666666666666", "0.6666666666666666", "0.3", "1.5")
    assert (c["f_orig_query"], c["f_unique_weighted"], c["average_abund"]) == ("0.3333333333333333", "0.3333333333333333", "5.0")
    assert (a["ksize"], a["scaled"], a["moltype"]) == (48, 5, "hp")
    assert a["query_md5"] == b["query_md5"] == wire.sourmash_md5(q_mins[:4], 16) and a["match_md5"] == wire.sourmash_md5(t_mins[3:5], 16)
    assert wire.gather_rows(q_names, q_off, q_mins, q_ab, t_names, t_off, t_mins, tuple(x[:0] for x in hits), rank[:0],
                            tuple(x[:0] for x in gathered), 16, 5, "hp") == []
    assert "no parity" in wire.do_gather.__doc__
    p = inspect.signature(wire.do_gather).parameters
    assert (p["min_unique"].default, p["max_results"].default, p["min_containment"].default) == (1, 0, 0.0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def test_gather_opts_layout_matches_header():
    o = _lib.ks_gather_opts
    assert C.sizeof(o) == 16
    assert [(getattr(o, f).offset, getattr(o, f).size) for f, _ in o._fields_] == [(0, 4), (4, 4), (8, 4), (12, 4)]
    text = open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read()
    body = re.search(r"typedef struct ks_gather_opts \{(.*?)\} ks_gather_opts;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [f for f, _ in o._fields_] == ["min_unique", "max_results", "flags", "reserved"]


def test_new_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert callable(engine.Context.gather) and callable(engine.Hits.gather_to_host)
    p = inspect.signature(engine.Context.gather).parameters
    assert (p["min_unique"].default, p["max_results"].default) == (1, 0)


def test_bad_options_are_refused_without_a_context(lib):
    some = C.c_void_p(64)  # a non-NULL pointer the option checks never follow
    for words in ((1, 0, 1, 0), (1, 0, 0, 1), (0, 0, 0xffffffff, 0), (0, 3, 0, 7)):
        out = C.c_void_p(12345)
        st = lib.ks_hits_gather(None, some, some, some, C.byref(_lib.ks_gather_opts(*words)), C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG, words
        assert not out.value
        assert lib.ks_hits_gather(None, None, None, None, C.byref(_lib.ks_gather_opts(*words)), None) == _lib.KS_ERR_INVALID_ARG
    out = C.c_void_p(1)
    # good options, or none, and no context: still an error, and nothing is made
    assert lib.ks_hits_gather(None, None, None, None, C.byref(_lib.ks_gather_opts(1, 0, 0, 0)), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert not out.value
    assert lib.ks_hits_gather(None, None, None, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    # the accessors of no object
    assert not lib.ks_hits_device_unique_intersect(None) and not lib.ks_hits_device_remaining(None)
    assert not lib.ks_hits_device_unique_weighted(None)
    assert lib.ks_hits_copy_gather_to_host(None, None, None, None, None) == _lib.KS_ERR_INVALID_ARG


def test_engine_refuses_option_words_that_do_not_fit():
    ctx = engine.Context.__new__(engine.Context)
    ctx._h, ctx._pinned, ctx._close_pending = None, 0, False
    for kw in ({"min_unique": -1}, {"min_unique": 2 ** 32}, {"max_results": 2 ** 32}):
        with pytest.raises(ValueError):
            ctx.gather(None, None, None, **kw)
