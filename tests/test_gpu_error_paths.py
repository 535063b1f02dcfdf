"""GPU: the error paths of every entry point that creates a result object.

Each entry point is run once uncapped and compared with the reference its own parity test uses, then again on a ladder of
KS_DEBUG_POOL_CAP values between the pool's bytes_in_use before the call and its bytes_held after it, a fresh context per rung:
the library's pool refuses an allocation at a different place of the driver each time (a status, before anything is launched).
A refused rung must come back as KS_ERR_OOM ("pool cap"), leave bytes_in_use where it was, and the same context must give the
right result once the cap is gone; a rung that is not refused must give the right result.  One more run throws
(KS_DEBUG_THROW=bad_alloc) inside the entry point's guard and checks the same triple.

Inputs: 200 synthetic proteins at k = 10, scaled = 1 and scaled = 5, queries = targets; a 3-sequence batch with an empty one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_ref  # noqa: E402
import crafted_sketches as crafted  # noqa: E402
import matchpos_join  # noqa: E402
import regions_ref  # noqa: E402
import signif_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import synth  # noqa: E402
from oracle import oracle  # noqa: E402

K, MOL = 10, "protein"
RUNGS = 6
OOM = ks._lib.KS_ERR_OOM


class Data:
    """The inputs of one parameter set and the CPU references, computed once."""

    def __init__(self, res, offs, scaled):
        self.res, self.offs, self.scaled = res, offs, scaled
        self.hits, self.mp, self.sk, _ = matchpos_join.reference(res, offs, res, offs, K, scaled, MOL)
        self.table = matchpos_join.position_table(res, offs, K, scaled, MOL, self.sk)
        self.pairs = crafted.ref_pairs(self.sk, self.sk)


@pytest.fixture(scope="module")
def data():
    res, offs = synth.proteome(200, stream=4107)
    d = {"s1": Data(res, offs, 1), "s5": Data(res, offs, 5)}
    e_res, e_offs = ks.pack([b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY", b"", b"MKVLAAGIVGLCARSTWYHHPQNDEFMKVLAAGIV"])
    d["empty"] = Data(e_res, e_offs, 1)
    return d


def _eq(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if w.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, i)
        else:
            assert np.array_equal(g, w.astype(g.dtype)), (what, i)


def _done(objs, got, want, what):
    for o in objs:
        if o is not None:
            o.free()
    _eq(got, want, what)


# ---- inputs on the device (built with no cap; from host arrays, so that they leave no idle scratch block behind) ------------
def _sketches(ctx, D):
    return ctx.sketches_from_host(*D.sk, K, D.scaled, MOL)


def _nothing(ctx, D):
    return {}


def _device_batch(ctx, D):
    return {"res": ctx.to_device(np.concatenate([D.res, np.zeros(16, np.uint8)])), "offs": ctx.to_device(D.offs)}


def _args(D, I):
    return I["res"].ptr, I["offs"].ptr, len(D.offs) - 1, int(D.offs[-1])


def _with_index(ctx, D):
    I = _device_batch(ctx, D)
    I["S"] = _sketches(ctx, D)
    I["ix"] = ctx.index_build(I["S"])
    return I


def _with_hits(ctx, D):
    I = {"S": _sketches(ctx, D)}
    I["ix"] = ctx.index_build(I["S"])
    I["H"] = ctx.search(I["ix"], I["S"])
    return I


def _with_tables(ctx, D):
    I = _with_hits(ctx, D)
    I["P"] = ctx.kmer_positions_table(D.res, D.offs, K, D.scaled, MOL)
    return I


def _with_matchpos(ctx, D):
    I = _with_tables(ctx, D)
    I["M"] = ctx.match_positions(I["P"], I["P"], I["H"], max_pairs=1 << 30)
    return I


def _with_corpus(ctx, D):
    I = _with_hits(ctx, D)
    I["C"] = I["S"].corpus()
    return I


def _merge_inputs(ctx, D):
    """two rank blocks: the hit rows of the even and of the odd targets, each ordered by (qid, tid)"""
    h = D.hits
    blocks = [np.nonzero(h[1] % 2 == r)[0] for r in (0, 1)]
    rows = np.concatenate(blocks)
    order = np.argsort(h[0][rows], kind="stable")  # the merged order: by qid, rank blocks in rank order inside a query
    I = {"rows": [len(b) for b in blocks], "n": len(rows), "want": [c[rows][order] for c in h]}
    I["in"] = [ctx.to_device(np.ascontiguousarray(c[rows])) for c in h]
    I["out"] = [ctx.to_device(np.zeros_like(c)) for c in h]
    return I


# ---- the calls: (I, D) -> nothing; each compares with the reference and frees what it made ---------------------------------
def c_sketch_batch(ctx, D, I):
    S = ctx.sketch_batch(D.res, D.offs, K, D.scaled, MOL)
    _done([S], S.to_host(), D.sk, "sketch_batch")


def c_sketch_batch_device(ctx, D, I):
    S = ctx.sketch_batch_device(*_args(D, I), K, D.scaled, MOL)
    _done([S], S.to_host(), D.sk, "sketch_batch_device")


def c_sketch_queries_device(ctx, D, I):
    S = ctx.sketch_queries_device(I["ix"], *_args(D, I))
    _done([S], S.to_host(), D.sk, "sketch_queries_device")


def c_sketch_search_device(ctx, D, I):
    S, H = ctx.sketch_search_device(I["ix"], *_args(D, I))
    _done([S, H], S.to_host() + H.to_host(), tuple(D.sk) + tuple(D.hits), "sketch_search_device")


def c_sketches_from_host(ctx, D, I):
    S = _sketches(ctx, D)
    _done([S], S.to_host(), D.sk, "sketches_from_host")


def c_union(ctx, D, I):
    U = I["S"].union()
    _done([U], U.to_host(), crafted.ref_union(D.sk), "union")


def c_corpus(ctx, D, I):
    C = I["S"].corpus()
    want = signif_ref.corpus(D.sk)
    total = C.total_abund
    _done([C], C.to_host(), want[:3], "corpus")
    assert total == want[3]


def c_index_build(ctx, D, I):
    ix = ctx.index_build(I["S"])
    n = (ix.n_targets, ix.n_postings)
    try:
        H = ctx.search(ix, I["S"])  # (an index shows what it holds through a search)
    except ks.KmerseekError:
        ix.free()  # (the search was refused, not the build: the index is this call's to give back)
        raise
    _done([H, ix], H.to_host(), D.hits, "index_build")
    assert n == (len(D.sk[0]) - 1, len(D.sk[1]))


def c_search(ctx, D, I):
    H = ctx.search(I["ix"], I["S"])
    _done([H], H.to_host(), D.hits, "search")


def c_search_sliced(ctx, D, I):
    H = ctx.search(I["ix"], I["S"], abund_stats=True)
    path = H.partition_path
    _done([H], H.to_host() + H.abund_stats_to_host(), tuple(D.hits) + crafted.ref_stats(D.hits, D.sk, D.sk), "search_sliced")
    assert path == 3  # the slices' lists were concatenated


def c_kmer_positions(ctx, D, I):
    P = ctx.kmer_positions_table(D.res, D.offs, K, D.scaled, MOL)
    _done([P], P.to_host(), D.table, "kmer_positions")


def c_match_positions(ctx, D, I):
    M = ctx.match_positions(I["P"], I["P"], I["H"], max_pairs=1 << 30)
    _done([M], M.to_host(), D.mp, "match_positions")


def c_match_regions(ctx, D, I):
    R = ctx.match_regions(I["M"])
    want = regions_ref.chain(D.mp[0], D.mp[1], D.mp[2], K)
    _done([R], R.to_host(), want, "match_regions")


def c_significance(ctx, D, I):
    G = ctx.significance(I["S"], I["S"], I["H"], I["C"], I["C"])
    _done([G], G.to_host(), signif_ref.significance(D.sk, D.sk, D.hits[0], D.hits[1])[:2], "significance")


def c_best_hits(ctx, D, I):
    B = ctx.best_hits(I["H"], 1, "jaccard", I["S"], I["S"])
    src, rank = best_ref.best_rows("jaccard", D.hits[0], D.hits[1], D.hits[2], 1, D.sk, D.sk)
    want = tuple(c[src] for c in D.hits) + (rank, src)
    _done([B], B.to_host() + B.best_to_host(), want, "best_hits")


def c_merge(ctx, D, I):
    ctx.merge_hits_by_qid_device(*[b.ptr for b in I["in"]], I["rows"], len(D.offs) - 1, *[b.ptr for b in I["out"]])
    ctx.synchronize()
    got = [b.to_host(c.dtype, I["n"]) for b, c in zip(I["out"], D.hits)]
    _eq(got, I["want"], "merge")


# name -> (inputs, call, extra KS_DEBUG_* of the call)
ENTRIES = {
    "sketch_batch": (_nothing, c_sketch_batch, {}),
    "sketch_batch_device": (_device_batch, c_sketch_batch_device, {}),
    "sketch_queries_device": (_with_index, c_sketch_queries_device, {}),
    "sketch_search_device": (_with_index, c_sketch_search_device, {}),
    "sketches_from_host": (_nothing, c_sketches_from_host, {}),
    "union": (lambda ctx, D: {"S": _sketches(ctx, D)}, c_union, {}),
    "corpus": (lambda ctx, D: {"S": _sketches(ctx, D)}, c_corpus, {}),
    "index_build": (lambda ctx, D: {"S": _sketches(ctx, D)}, c_index_build, {}),
    "search": (_with_hits, c_search, {}),
    "search_sliced": (_with_hits, c_search_sliced, {"KS_DEBUG_PAIR_LIMIT": "PAIRS/3"}),
    "kmer_positions": (_nothing, c_kmer_positions, {}),
    "match_positions": (_with_tables, c_match_positions, {}),
    "match_regions": (_with_matchpos, c_match_regions, {}),
    "significance": (_with_corpus, c_significance, {}),
    "best_hits": (_with_hits, c_best_hits, {}),
    "merge": (_merge_inputs, c_merge, {}),
}
CASES = [(e, p) for e in ENTRIES for p in ("s1", "s5")] + [(e, "empty") for e in ("sketch_batch", "sketch_batch_device", "kmer_positions")]


class _Run:
    """One context with the inputs of one entry point on it."""

    def __init__(self, monkeypatch, entry, D):
        self.mp, self.D = monkeypatch, D
        setup, self.call, env = ENTRIES[entry]
        self.env = {k: (str(D.pairs // 3) if v == "PAIRS/3" else v) for k, v in env.items()}
        self.ctx = ks.Context(0, follow_debug_env=True)
        self.I = setup(self.ctx, D)
        self.before = self.ctx.pool_stats()["bytes_in_use"]

    def go(self, **knobs):
        """the call under the entry's own knobs and `knobs`; -> the KmerseekError it raised, or None"""
        env = dict(self.env, **knobs)
        for k, v in env.items():
            self.mp.setenv(k, v)
        try:
            self.call(self.ctx, self.D, self.I)
            return None
        except ks.KmerseekError as e:
            return e
        finally:
            for k in env:
                self.mp.delenv(k)

    def refused_cleanly(self, err, what):
        """the triple: the status, nothing leaked, the context still works"""
        assert err.status == OOM, (what, err.status, str(err))
        assert self.ctx.pool_stats()["bytes_in_use"] == self.before, what
        again = self.go()
        assert again is None, (what, str(again))

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("entry,params", CASES)
def test_pool_refusals_leave_nothing_behind(monkeypatch, data, entry, params):
    D = data[params]
    first = _Run(monkeypatch, entry, D)
    try:
        err = first.go()
        assert err is None, str(err)
        assert first.ctx.pool_stats()["bytes_in_use"] == first.before
        lo, hi = max(first.before, 1), first.ctx.pool_stats()["bytes_held"]
    finally:
        first.close()
    assert hi > lo, (lo, hi)
    caps = [lo + (hi - lo) * i // (RUNGS - 1) for i in range(RUNGS)]
    refused = []
    for cap in caps:
        run = _Run(monkeypatch, entry, D)
        try:
            err = run.go(KS_DEBUG_POOL_CAP=str(cap))
            refused.append(err is not None)
            if err is not None:
                assert "pool cap" in str(err), (cap, str(err))
                run.refused_cleanly(err, (entry, params, cap))
        finally:
            run.close()
    print(f"{entry}/{params}: bytes_in_use {lo}, bytes_held {hi}, refused rungs {refused}")
    assert any(refused), (entry, params, caps)   # the ladder reaches into the driver's allocations ...
    assert not refused[-1], (entry, params, caps)  # ... and ends where the call fits


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_exception_inside_the_guard_leaves_nothing_behind(monkeypatch, data, entry):
    run = _Run(monkeypatch, entry, data["s5"])
    try:
        err = run.go(KS_DEBUG_THROW="bad_alloc")
        assert err is not None, entry
        run.refused_cleanly(err, entry)
    finally:
        run.close()
