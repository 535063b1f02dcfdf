"""GPU: ks_regions_cull_device — per hit row the regions no better region of the row covers — and the three takes.

Every result array is compared exactly with the plain-loop restatement of tests/rcull_ref.py; the fixed cases also with the
hand-written expectations of tests/rcull_cases.py (tests/test_region_cull_cpu.py holds the reference against those).  The
synthetic inputs run under KS_DEBUG_CULL_PATH unset, 1, 2 and 3 — by length, a wave per row, a workgroup per row, a workgroup
with the small LDS capacity — on a context created after the variable is set, and give the same arrays.  Cases: the fixed
inputs, a fuzz with frequent coverage and ties, rows of 8 / 9 / 64 / 65 regions and around the small LDS capacity, a row of
700 and one of 3,000 regions, 2,000 short rows, both object entry points on a pipeline's own columns, the deletion pair
through take and traceback, row_best_score as the rank key of best_hits, the golden pair through the wire, and the errors."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rcull_cases as RC  # noqa: E402
import rcull_ref  # noqa: E402
import rtrace_cases  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
MODES = (None, "1", "2", "3")  # KS_DEBUG_CULL_PATH
OPTS = ({}, {"P": 50}, {"P": 1, "min_score": 3}, {"P": 80, "N": 2}, {"N": 1, "min_score": 10})


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


@pytest.fixture(params=MODES, ids=lambda m: f"path_{m}")
def mode_ctx(request, monkeypatch):
    """A context created after KS_DEBUG_CULL_PATH is set (the knobs are read when a context is made)."""
    if request.param is None:
        monkeypatch.delenv("KS_DEBUG_CULL_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_CULL_PATH", request.param)
    with ks.Context(0) as c:
        yield c


def _lds_rows():
    small = C.c_uint32(0)
    big = int(_lib.load().ks_debug_rcull_lds_rows(C.byref(small)))
    return big, int(small.value)


def device_cull(ctx, cols, P=100, N=0, min_score=None, t_length=True):
    """The columns uploaded with Context.to_device, culled by cull_regions_device -> the arrays of RegionCull.to_host()."""
    bufs = [ctx.to_device(c if len(c) else np.zeros(1, c.dtype)) for c in cols]
    try:
        cu = ctx.cull_regions_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr if t_length else None, bufs[5].ptr,
                                     len(cols[0]) - 1, len(cols[1]), overlap_pct=P, min_score=min_score, max_per_row=N)
        assert (cu.n_rows, cu.n_regions) == (len(cols[0]) - 1, len(cols[1]))
        got = cu.to_host()
        assert cu.n_kept == len(got[1]) == int(got[0][-1]) and all(p != 0 for p in cu.device_ptrs())
        assert cu.row_best_score_ptr == cu.device_ptrs()[5]
        assert [a.dtype for a in got] == [np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.float64]
        cu.free()
        return got
    finally:
        for b in bufs:
            b.free()


# ---- the synthetic inputs and their reference results, computed once -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_input():
    return rcull_ref.fuzz_rows(7, 300, 24)


@functools.lru_cache(maxsize=None)
def ladder_input():
    """Rows on both sides of every threshold between two paths, a row of 700 (several sweeps of the staged workgroup path) and one
    of 3,000 regions (beyond the LDS capacity), with empty rows between them."""
    big, small = _lds_rows()
    assert small + 1 < 64 < big < 3000
    return rcull_ref.fuzz_rows(21, 0, 0, lengths=[8, 9, 0, 64, 65, small - 1, small, small + 1, 0, 1, 2, 700, 3000, 0, 3], n_centres=12)


@functools.lru_cache(maxsize=None)
def many_rows_input():
    return rcull_ref.fuzz_rows(33, 2000, 20, tie_scores=False)


@functools.lru_cache(maxsize=None)
def reference(which, opts):
    cols = {"fuzz": fuzz_input, "ladder": ladder_input, "many": many_rows_input}[which]()
    return rcull_ref.cull(*cols, **dict(opts))


def check_invariants(cols, got):
    offs, src, rank, nm, keeper, best = got
    n = len(cols[1])
    assert int(nm.sum()) + int((keeper == rcull_ref.NONE).sum()) == n
    kept = keeper == np.arange(n, dtype=np.uint32)
    assert np.array_equal(np.flatnonzero(kept), src) and np.array_equal(np.bincount(keeper[keeper != rcull_ref.NONE], minlength=n)[src], nm)


# ---- 1. the fixed cases -----------------------------------------------------------------------------------------------------------
def test_fixed_cases(mode_ctx):
    for c in RC.CASES:
        o = c["opts"]
        got = device_cull(mode_ctx, RC.columns(c), P=o["P"], N=o["N"], min_score=o["min_score"])
        RC.assert_same(got, RC.expected(c), c["name"])
    c = next(c for c in RC.CASES if c["name"] == "boundary_p100")
    RC.assert_same(device_cull(mode_ctx, RC.columns(c), P=0), RC.expected(c), "overlap_pct 0 means 100")


# ---- 2. the fuzz, the ladder of row lengths, many short rows ---------------------------------------------------------------------
@pytest.mark.parametrize("which,opts", [("fuzz", o) for o in OPTS] + [("ladder", OPTS[0]), ("ladder", OPTS[1]), ("ladder", OPTS[3]),
                                                                      ("many", OPTS[0]), ("many", {"P": 60, "min_score": -2 ** 39})],
                         ids=lambda v: v if isinstance(v, str) else "_".join(f"{k}{x}" for k, x in v.items()) or "defaults")
def test_synthetic_rows(mode_ctx, which, opts):
    cols = {"fuzz": fuzz_input, "ladder": ladder_input, "many": many_rows_input}[which]()
    want = reference(which, tuple(sorted(opts.items())))
    got = device_cull(mode_ctx, cols, **opts)
    RC.assert_same(got, want, f"{which} {opts}")
    check_invariants(cols, got)


def test_culling_the_kept_again_keeps_everything(ctx):
    cols = fuzz_input()
    for P in (100, 50):
        offs, src = device_cull(ctx, cols, P=P)[:2]
        again = device_cull(ctx, (offs, *[c[src] for c in cols[1:]]), P=P)
        assert np.array_equal(again[0], offs) and np.array_equal(again[1], np.arange(len(src))) and (again[3] == 1).all()
        assert np.array_equal(again[4], np.arange(len(src)))


def test_empty_inputs(ctx):
    empty = [np.zeros(0, d) for d in (np.uint32, np.uint32, np.uint32, np.uint32, np.int64)]
    got = device_cull(ctx, (np.zeros(1, np.uint64), *empty))
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])
    got = device_cull(ctx, (np.zeros(6, np.uint64), *empty))
    assert got[0].tolist() == [0] * 6 and len(got[1]) == 0 and np.isnan(got[5]).all() and len(got[5]) == 5


# ---- 3. the object entry points, take and traceback on a pipeline -------------------------------------------------------------------
class _Pipe:
    """queries x targets up to the regions, their scores and their alignments, on the device."""

    def __init__(self, ctx, queries, targets, k, scaled=1, mol="protein"):
        self.ctx, self.q, self.t = ctx, ks.pack(queries), ks.pack(targets)
        q, t = self.q, self.t
        T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
        Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
        self.hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
        tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
        mp = ctx.match_positions(qp, tp, self.hits)
        self.rg = ctx.match_regions(mp)
        self.sc = ctx.score_regions(self.rg, self.hits, q[0], q[1], t[0], t[1], extend=True, x_drop=10)
        self.al = ctx.align_regions(self.rg, self.hits, q[0], q[1], t[0], t[1])
        for o in (mp, qp, tp, Q, T):
            o.free()

    def trace(self, rg, al, **kw):
        return self.ctx.trace_regions(rg, self.hits, self.q[0], self.q[1], self.t[0], self.t[1], al, **kw)

    def close(self):
        for o in (self.al, self.sc, self.rg, self.hits):
            o.free()


@pytest.fixture(scope="module")
def indel_pipe(ctx):
    qs, ts, _ = rtrace_cases.indel_batch(16, 86)
    q, t, _ = RC.deletion_pair()
    p = _Pipe(ctx, qs + [q], ts + [t], rtrace_cases.INDEL_K)
    yield p
    p.close()


def test_object_entry_points_against_the_reference(ctx, indel_pipe):
    p = indel_pipe
    al, sc = p.al.to_host(), p.sc.to_host()
    assert p.rg.n_regions > p.rg.n_rows > 10  # indels split matches: rows of several regions
    for opts in ({}, {"P": 50}, {"P": 90, "N": 1}, {"min_score": 40}):
        kw = {"overlap_pct": opts.get("P", 100), "max_per_row": opts.get("N", 0), "min_score": opts.get("min_score")}
        cu = ctx.cull_regions(p.al, **kw)
        RC.assert_same(cu.to_host(), rcull_ref.cull(*al[:6], **opts), f"raligns {opts}")
        cu.free()
        cu = ctx.cull_regions(p.sc, **kw)  # one length for both sides: d_t_length == NULL semantics
        want = rcull_ref.cull(sc[0], sc[1], sc[3], sc[2], None, sc[4], **opts)
        RC.assert_same(cu.to_host(), want, f"rscores {opts}")
        cu.free()
        got = device_cull(ctx, (sc[0], sc[1], sc[3], sc[2], sc[3], sc[4]), t_length=False, **opts)
        RC.assert_same(got, want, f"device entry with d_t_length NULL {opts}")
    assert len(rcull_ref.cull(*al[:6])[1]) < p.rg.n_regions  # the cull removes something here
    with pytest.raises(TypeError):
        ctx.cull_regions(p.rg)


def test_take_gathers_every_column(ctx, indel_pipe):
    p = indel_pipe
    cu = ctx.cull_regions(p.al, overlap_pct=80)
    offs, src = cu.to_host()[:2]
    for obj in (p.rg, p.sc, p.al):
        taken = cu.take(obj)
        assert type(taken) is type(obj) and taken.n_rows == obj.n_rows and taken.n_regions == cu.n_kept
        got, full = taken.to_host(), obj.to_host()
        assert np.array_equal(got[0], offs)
        for g, f in zip(got[1:], full[1:]):
            assert g.dtype == f.dtype and np.array_equal(g, f[src])
        taken.free()
    with pytest.raises(TypeError):
        cu.take(p.hits)
    cu.free()


def test_deletion_pair_keeps_one_alignment_and_traces_it(ctx, indel_pipe):
    """tests/test_region_cull_cpu.py: the pair's two fragment alignments coincide.  The cull keeps one of them for both; tracing
    the taken regions and alignments gives exactly the CIGARs of tracing everything, indexed by src_region."""
    p = indel_pipe
    qid, tid = p.hits.to_host()[:2]
    q_last, t_last = len(p.q[1]) - 2, len(p.t[1]) - 2
    row = int(np.flatnonzero((qid == q_last) & (tid == t_last))[0])
    rg = p.rg.to_host()
    b, e = int(rg[0][row]), int(rg[0][row + 1])
    assert [(int(rg[1][g]), int(rg[2][g]), int(rg[3][g])) for g in range(b, e)] == RC.deletion_pair()[2]
    cu = ctx.cull_regions(p.al)
    offs, src, rank, nm, keeper, best = cu.to_host()
    assert offs[row + 1] - offs[row] == 1 and src[offs[row]] == b and nm[offs[row]] == 2 and rank[offs[row]] == 0
    assert keeper[b:e].tolist() == [b, b] and best[row] == float(p.al.to_host()[5][b])
    for eqx in (False, True):
        all_cg = p.trace(p.rg, p.al, eqx=eqx)
        t_rg, t_al = cu.take(p.rg), cu.take(p.al)
        kept_cg = p.trace(t_rg, t_al, eqx=eqx)
        assert kept_cg.n_regions == cu.n_kept < all_cg.n_regions
        every = all_cg.strings()
        assert kept_cg.strings() == [every[g] for g in src.tolist()]
        assert "3I" in every[b] and "3I" in every[b + 1]
        for o in (all_cg, kept_cg, t_rg, t_al):
            o.free()
    cu.free()


def test_row_best_score_ranks_the_hits(ctx, indel_pipe):
    p = indel_pipe
    al = p.al.to_host()
    floor = int(np.median(al[5]))
    cu = ctx.cull_regions(p.al, min_score=floor)  # some rows keep nothing: NaN, ranked last
    best = cu.to_host()[5]
    assert np.isnan(best).any() and not np.isnan(best).all()
    qid, tid = p.hits.to_host()[:2]
    for k in (1, 3, 5):
        top = ctx.best_hits(p.hits, k, score=cu.row_best_score_ptr)
        rank, src_row = top.best_to_host()
        want = []
        for q in np.unique(qid):
            rows = np.flatnonzero(qid == q).tolist()
            rows.sort(key=lambda r: (np.isnan(best[r]), -best[r] if not np.isnan(best[r]) else 0.0, tid[r]))
            want += [(r, i) for i, r in enumerate(rows[:k])]
        assert sorted(zip(src_row.tolist(), rank.tolist())) == sorted(want)
        top.free()
    cu.free()


# ---- 4. the golden pair through the wire ----------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    plain = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, cigar=True)
    culled = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, cigar=True, cull=True)
    # the reference's selection, on the device's own regions and alignments
    p = _Pipe(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], 16, 5, "hp")
    want = rcull_ref.cull(*p.al.to_host()[:6])
    cg = p.trace(p.rg, p.al)
    qid, tid = p.hits.to_host()[:2]
    rows = wire.region_rows(ced9_records, bcl2_records, qid, tid, p.rg.to_host(), "hp", alignments=p.al.to_host(), cigars=cg.to_host(), cull=want)
    cg.free()
    p.close()
    assert culled == rows and len(culled) == len(want[1]) <= len(plain) == 7
    strip = lambda r: {k: v for k, v in r.items() if k not in ("aln_rank", "aln_n_merged")}
    kept = [strip(r) for r in culled]
    assert all(r in plain for r in kept) and [r for r in plain if r in kept] == kept
    # scores only: the other pair of columns; a limit of one row per hit; and a cull of nothing is refused
    s_rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, score=True, extend=True, x_drop=10, cull=True, max_alns=1)
    assert s_rows and all(r["region_rank"] == 0 and r["region_n_merged"] >= 1 for r in s_rows)
    assert len({(r["query_name"], r["match_name"]) for r in s_rows}) == len(s_rows)
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, cull=True)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, indel_pipe):
    L = ctx._L
    c = next(c for c in RC.CASES if c["name"] == "empty_rows_between")
    cols = RC.columns(c)
    bufs = [ctx.to_device(a) for a in cols]
    ptrs = [C.c_void_p(b.ptr) for b in bufs]
    n_rows, n = len(cols[0]) - 1, len(cols[1])
    before = ctx.pool_stats()["bytes_in_use"]
    # the options: before any device work, with ctx == NULL too
    for opts in (_lib.ks_rcull_opts(100, 0, 0, 2, 0), _lib.ks_rcull_opts(100, 0, 0, 0, 1), _lib.ks_rcull_opts(101, 0, 0, 0, 0),
                 _lib.ks_rcull_opts(100, 0, 0, _lib.KS_RCULL_MIN_SCORE | 4, 0)):
        for h in (ctx._h, None):
            out = C.c_void_p()
            assert L.ks_regions_cull_device(h, None, None, None, None, None, None, 0, 0, C.byref(opts), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
            assert L.ks_raligns_cull(h, indel_pipe.al._h, C.byref(opts), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
            assert L.ks_rscores_cull(h, indel_pipe.sc._h, C.byref(opts), C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
    with pytest.raises(ValueError):
        ctx.cull_regions(indel_pipe.al, overlap_pct=101)
    # NULL arguments
    out = C.c_void_p()
    assert L.ks_regions_cull_device(ctx._h, None, *ptrs[1:], n_rows, n, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_regions_cull_device(ctx._h, ptrs[0], None, *ptrs[2:], n_rows, n, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_regions_cull_device(ctx._h, *ptrs, n_rows, n, None, None) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_raligns_cull(ctx._h, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_rscores_cull(ctx._h, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    # row_offsets that is no CSR from 0 to n: the first bad row is named
    for bad, row in (([1, 1, 2, 2, 3, 3], 0), ([0, 0, 2, 1, 3, 3], 2), ([0, 0, 2, 2, 3, 2], 4), ([0, 0, 2, 2, 4, 4], 3), ([0, 0, 2, 2, 2, 2], 4)):
        ob = ctx.to_device(np.array(bad, np.uint64))
        with pytest.raises(ks.KmerseekError) as e:
            ctx.cull_regions_device(ob.ptr, *[b.ptr for b in bufs[1:]], n_rows, n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"hit row {row} " in str(e.value), (bad, str(e.value))
        ob.free()
    with pytest.raises(ks.KmerseekError) as e:  # regions without a row
        ctx.cull_regions_device(bufs[0].ptr, *[b.ptr for b in bufs[1:]], 0, n)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG
    # a region with a length of 0: the first one is named
    for col in (2, 4):
        z = cols[col].copy()
        z[1:] = 0
        zb = ctx.to_device(z)
        with pytest.raises(ks.KmerseekError) as e:
            ctx.cull_regions_device(*[zb.ptr if i == col else b.ptr for i, b in enumerate(bufs)], n_rows, n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "region 1 " in str(e.value)
        zb.free()
    # more rows or regions than 32 bits index: refused before any device work
    for nr, ng in ((2 ** 32 - 2, n), (n_rows, 2 ** 32)):
        with pytest.raises(ks.KmerseekError) as e:
            ctx.cull_regions_device(*[b.ptr for b in bufs], nr, ng)
        assert e.value.status == _lib.KS_ERR_CAPACITY
    # objects of another context; a cull of other regions
    cu = ctx.cull_regions(indel_pipe.al)
    small = ctx.cull_regions_device(*[b.ptr for b in bufs], n_rows, n)
    with ks.Context(0) as other:
        out = C.c_void_p()
        assert other._L.ks_raligns_cull(other._h, indel_pipe.al._h, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
        assert other._L.ks_rscores_cull(other._h, indel_pipe.sc._h, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
        assert other._L.ks_raligns_take(other._h, indel_pipe.al._h, cu._h, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
    for obj in (indel_pipe.rg, indel_pipe.sc, indel_pipe.al):
        with pytest.raises(ks.KmerseekError) as e:
            small.take(obj)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "a cull of other regions" in str(e.value)
    assert L.ks_regions_take(ctx._h, None, cu._h, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_regions_take(ctx._h, indel_pipe.rg._h, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    cu.free(); small.free()
    assert ctx.pool_stats()["bytes_in_use"] == before
    # the context stays usable
    RC.assert_same(device_cull(ctx, cols), RC.expected(c))
    for b in bufs:
        b.free()
