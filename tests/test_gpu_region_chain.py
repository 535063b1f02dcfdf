"""GPU: ks_regions_chain_device — per hit row the best colinear chain of its regions — and ks_rchain_coverage.

Every result array is compared exactly with the plain-loop restatement of tests/rchain_ref.py; the fixed cases also with the
hand-written expectations of tests/rchain_cases.py (tests/test_region_chain_cpu.py holds the reference against those and against
exhaustive enumeration).  The synthetic inputs run under KS_DEBUG_CHAIN_PATH unset, 1, 2 and 3 — by length, a wave per row, a
workgroup per row, a workgroup with the small LDS capacity — on a context created after the variable is set, and give the same
arrays.  Cases: the fixed inputs, a fuzz of tracks and scattered regions with ties, rows of 8 / 9 / 64 / 65 regions and around
the small LDS capacity, a row of 700 and one of 3,000 regions whose chains have hundreds of members, 2,000 short rows, both
object entry points on a pipeline's own columns, the insertion pair, row_chain_score as the rank key of best_hits, the coverage
column bit for bit and as the edge score of cluster_greedy, the golden pair through the wire, and the errors."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import greedy_ref  # noqa: E402
import rchain_cases as RH  # noqa: E402
import rchain_ref  # noqa: E402
import rcull_ref  # noqa: E402
import rtrace_cases  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
MODES = (None, "1", "2", "3")  # KS_DEBUG_CHAIN_PATH
OPTS = ({}, {"max_overlap": 4}, {"max_gap": 30, "max_overlap": 4, "link_cost": 2, "skew_cost": 1, "overlap_cost": 1},
        {"max_overlap": 2 ** 32 - 1, "overlap_cost": 3, "link_cost": 11}, {"max_gap": 8, "skew_cost": 2 ** 16})
VARIANTS = ("full", "no_t_length", "no_sums")  # every column; d_t_length NULL; d_identities and d_aln_length NULL


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


@pytest.fixture(params=MODES, ids=lambda m: f"path_{m}")
def mode_ctx(request, monkeypatch):
    """A context created after KS_DEBUG_CHAIN_PATH is set (the knobs are read when a context is made)."""
    if request.param is None:
        monkeypatch.delenv("KS_DEBUG_CHAIN_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_CHAIN_PATH", request.param)
    with ks.Context(0) as c:
        yield c


def _lds_rows():
    small = C.c_uint32(0)
    big = int(_lib.load().ks_debug_rchain_lds_rows(C.byref(small)))
    return big, int(small.value)


def device_chain(ctx, cols, variant="full", null_opts=False, **opts):
    """The columns (row_offsets, q_start, q_length, t_start, t_length, score[, identities, aln_length]) uploaded with
    Context.to_device and chained by chain_regions_device -> the arrays of RegionChain.to_host()."""
    bufs = [ctx.to_device(c if len(c) else np.zeros(1, c.dtype)) for c in cols]
    p = [b.ptr for b in bufs] + [None] * (8 - len(bufs))
    if variant == "no_t_length":
        p[4] = None
    if variant == "no_sums":
        p[6] = p[7] = None
    n_rows, n = len(cols[0]) - 1, len(cols[1])
    try:
        if null_opts:  # opts == NULL through the C entry point itself
            out = C.c_void_p()
            ctx._check(ctx._L.ks_regions_chain_device(ctx._h, *[C.c_void_p(x) if x else None for x in p], n_rows, n, None, C.byref(out)))
            ch = ks.RegionChain(ctx, out)
        else:
            ch = ctx.chain_regions_device(*p[:6], n_rows, n, d_identities=p[6], d_aln_length=p[7], **opts)
        assert (ch.n_rows, ch.n_regions) == (n_rows, n)
        got = ch.to_host()
        assert ch.n_chained == len(got[1]) == int(got[0][-1]) and all(x != 0 for x in ch.device_ptrs())
        assert ch.row_chain_score_ptr == ch.device_ptrs()[13] and ch.row_coverage_ptr == 0
        ch.free()
        return got
    finally:
        for b in bufs:
            b.free()


def ref_chain(cols, variant="full", **opts):
    tl = None if variant == "no_t_length" else cols[4]
    sums = {} if variant == "no_sums" or len(cols) < 8 else {"identities": cols[6], "aln_length": cols[7]}
    return rchain_ref.chain(cols[0], cols[1], cols[2], cols[3], tl, cols[5], **sums, **opts)


# ---- the synthetic inputs and their reference results, computed once -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_input():
    return rchain_ref.chain_rows(7, 300, 24)


@functools.lru_cache(maxsize=None)
def ladder_input():
    """Rows on both sides of every threshold between two paths, a row of 700 (several sweeps of the staged workgroup path) and one
    of 3,000 regions (beyond the LDS capacity), with empty rows between them."""
    big, small = _lds_rows()
    assert small + 1 < 64 < 700 <= big < 3000
    return rchain_ref.chain_rows(21, 0, 0, lengths=[8, 9, 0, 64, 65, small - 1, small, small + 1, 0, 1, 2, 700, 3000, 0, 3])


@functools.lru_cache(maxsize=None)
def many_rows_input():
    return rchain_ref.chain_rows(33, 2000, 12, n_tracks=2)


INPUTS = {"fuzz": fuzz_input, "ladder": ladder_input, "many": many_rows_input}


@functools.lru_cache(maxsize=None)
def reference(which, opts, variant):
    return ref_chain(INPUTS[which](), variant, **dict(opts))


def check_invariants(cols, got, opts):
    """Every member but the first has its predecessor as pred; chain_score is the members' scores minus the link costs."""
    offs, src, best, pred, score = [a.tolist() for a in got[:5]]
    ext = lambda g: tuple(int(cols[c][g]) for c in (1, 2, 3, 4))
    price = {k: opts.get(k, 0) for k in ("link_cost", "skew_cost", "overlap_cost")}
    for r in range(len(offs) - 1):
        mem = src[offs[r]:offs[r + 1]]
        assert (len(mem) == 0) == (cols[0][r] == cols[0][r + 1])
        if mem:
            assert pred[mem[0]] == rchain_ref.NONE and all(pred[b] == a for a, b in zip(mem, mem[1:]))
            links = sum(rchain_ref.cost(ext(a), ext(b), **price) for a, b in zip(mem, mem[1:]))
            assert score[r] == best[mem[-1]] == sum(int(cols[5][g]) for g in mem) - links


# ---- 1. the fixed cases -----------------------------------------------------------------------------------------------------------
def test_fixed_cases(mode_ctx):
    for c in RH.CASES:
        RH.assert_same(device_chain(mode_ctx, RH.columns(c), **c["opts"]), RH.expected(c), c["name"])
    for c in RH.CASES:
        if not c["opts"]:
            RH.assert_same(device_chain(mode_ctx, RH.columns(c), null_opts=True), RH.expected(c), c["name"] + " with opts == NULL")


# ---- 2. the fuzz, the ladder of row lengths, many short rows ---------------------------------------------------------------------
@pytest.mark.parametrize("which,opts", [("fuzz", o) for o in OPTS] + [("ladder", OPTS[0]), ("ladder", OPTS[2]), ("ladder", OPTS[3]),
                                                                      ("many", OPTS[0]), ("many", OPTS[2])],
                         ids=lambda v: v if isinstance(v, str) else "_".join(f"{k}{x}" for k, x in v.items()) or "defaults")
def test_synthetic_rows(mode_ctx, which, opts):
    cols = INPUTS[which]()
    for variant in VARIANTS:
        want = reference(which, tuple(sorted(opts.items())), variant)
        got = device_chain(mode_ctx, cols, variant, **opts)
        RH.assert_same(got, want, f"{which} {opts} {variant}")
    check_invariants(cols, got, opts)
    if which == "ladder" and not opts:
        n_mem = np.diff(want[0].astype(np.int64))
        assert n_mem[11] >= 50 and n_mem[12] >= 200  # long dependent chains, and a long walk back


# ---- 3. empty inputs ----------------------------------------------------------------------------------------------------------------
def test_empty_inputs(ctx):
    empty = [np.zeros(0, d) for d in (np.uint32, np.uint32, np.uint32, np.uint32, np.int64)]
    got = device_chain(ctx, (np.zeros(1, np.uint64), *empty))
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])
    got = device_chain(ctx, (np.zeros(6, np.uint64), *empty))
    RH.assert_same(got, rchain_ref.chain(np.zeros(6, np.uint64), *empty), "rows without regions")
    assert got[0].tolist() == [0] * 6 and len(got[1]) == 0 and np.isnan(got[13]).all() and len(got[13]) == 5
    assert all(not a.any() for a in got[4:13])


# ---- 4. the object entry points on a pipeline ---------------------------------------------------------------------------------------
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

    def close(self):
        for o in (self.al, self.sc, self.rg, self.hits):
            o.free()


@pytest.fixture(scope="module")
def indel_pipe(ctx):
    qs, ts, _ = rtrace_cases.indel_batch(16, 86)
    q, t, _ = RH.insertion_pair()
    p = _Pipe(ctx, qs + [q], ts + [t], rtrace_cases.INDEL_K)
    yield p
    p.close()


def _al_ref(al, **opts):
    return rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **opts)


def _sc_ref(sc, **opts):
    return rchain_ref.chain(sc[0], sc[1], sc[3], sc[2], None, sc[4], identities=sc[5], aln_length=sc[3], **opts)


def test_object_entry_points_against_the_reference(ctx, indel_pipe):
    p = indel_pipe
    al, sc = p.al.to_host(), p.sc.to_host()
    assert p.rg.n_regions > p.rg.n_rows > 10  # indels split matches: rows of several regions
    for opts in ({}, {"max_overlap": 10}, {"max_overlap": 200, "overlap_cost": 1, "skew_cost": 1}, {"max_gap": 5, "link_cost": 20}):
        ch = ctx.chain_regions(p.al, **opts)
        RH.assert_same(ch.to_host(), _al_ref(al, **opts), f"raligns {opts}")
        ch.free()
        ch = ctx.chain_regions(p.sc, **opts)  # one length for both sides and as aln_length
        RH.assert_same(ch.to_host(), _sc_ref(sc, **opts), f"rscores {opts}")
        ch.free()
    with pytest.raises(TypeError):
        ctx.chain_regions(p.rg)
    with pytest.raises(ValueError):
        ctx.chain_regions(p.al, link_cost=2 ** 30 + 1)
    # what the cull kept: the chain of the taken objects equals the reference on the taken columns
    cu = ctx.cull_regions(p.al)
    taken = cu.take(p.al)
    assert taken.n_regions < p.al.n_regions
    for opts in ({}, {"max_overlap": 10, "skew_cost": 1}):
        ch = ctx.chain_regions(taken, **opts)
        RH.assert_same(ch.to_host(), _al_ref(taken.to_host(), **opts), f"taken {opts}")
        ch.free()
    taken.free(); cu.free()


def test_insertion_pair_chains_its_two_alignments(ctx, indel_pipe):
    """tests/test_region_chain_cpu.py: the pair's two alignments end and begin at the insertion, 40 positions apart on the query
    alone.  Neither covers the other: the cull keeps both.  The chain joins them for |dq - dt| = 40 times the skew cost."""
    p = indel_pipe
    q, t, seeds = RH.insertion_pair()
    qid, tid = p.hits.to_host()[:2]
    row = int(np.flatnonzero((qid == len(p.q[1]) - 2) & (tid == len(p.t[1]) - 2))[0])
    rg = p.rg.to_host()
    b, e = int(rg[0][row]), int(rg[0][row + 1])
    assert [(int(rg[1][g]), int(rg[2][g]), int(rg[3][g])) for g in range(b, e)] == seeds
    cu = ctx.cull_regions(p.al)
    taken = cu.take(p.al)
    t_al = taken.to_host()
    kb, ke = int(t_al[0][row]), int(t_al[0][row + 1])
    assert ke - kb == 2  # two alignments after the cull
    s0, s1 = int(t_al[5][kb]), int(t_al[5][kb + 1])
    ch = ctx.chain_regions(taken, skew_cost=1)
    h = ch.to_host()
    assert h[1][h[0][row]:h[0][row + 1]].tolist() == [kb, kb + 1]  # it chains both
    assert h[4][row] == s0 + s1 - RH.INSERTION and h[13][row] == float(s0 + s1 - RH.INSERTION)
    assert h[3][kb] == rchain_ref.NONE and h[3][kb + 1] == kb
    assert (h[5][row], h[5][row] + h[6][row], h[7][row], h[7][row] + h[8][row]) == (0, len(q), 0, len(t))
    assert h[9][row] <= len(q) - RH.INSERTION and h[10][row] <= len(t) and h[9][row] == t_al[2][kb] + t_al[2][kb + 1]
    assert h[11][row] == int(t_al[6][kb]) + int(t_al[6][kb + 1]) and h[12][row] == int(t_al[10][kb]) + int(t_al[10][kb + 1])
    ch.free()
    ch = ctx.chain_regions(taken, skew_cost=2 ** 16)  # the link costs more than an alignment is worth: a chain of one
    h = ch.to_host()
    assert h[0][row + 1] - h[0][row] == 1 and h[4][row] == max(s0, s1)
    ch.free()
    taken.free(); cu.free()


# ---- 5. row_chain_score as a rank key -----------------------------------------------------------------------------------------------
def test_row_chain_score_ranks_the_hits(ctx, indel_pipe):
    p = indel_pipe
    al = p.al.to_host()
    floor = int(np.median(al[5]))
    cu = ctx.cull_regions(p.al, min_score=floor)  # some rows keep nothing: their chain is empty, NaN, ranked last
    taken = cu.take(p.al)
    ch = ctx.chain_regions(taken, max_overlap=5)
    best = ch.to_host()[13]
    assert np.isnan(best).any() and not np.isnan(best).all()
    qid, tid = p.hits.to_host()[:2]
    for k in (1, 3, 5):
        top = ctx.best_hits(p.hits, k, score=ch.row_chain_score_ptr)
        rank, src_row = top.best_to_host()
        want = []
        for q in np.unique(qid):
            rows = np.flatnonzero(qid == q).tolist()
            rows.sort(key=lambda r: (np.isnan(best[r]), -best[r] if not np.isnan(best[r]) else 0.0, tid[r]))
            want += [(r, i) for i, r in enumerate(rows[:k])]
        assert sorted(zip(src_row.tolist(), rank.tolist())) == sorted(want)
        top.free()
    ch.free(); taken.free(); cu.free()


# ---- 6. coverage --------------------------------------------------------------------------------------------------------------------
def test_coverage_bit_for_bit(ctx, indel_pipe):
    p = indel_pipe
    cu = ctx.cull_regions(p.al, min_score=int(np.median(p.al.to_host()[5])))
    taken = cu.take(p.al)
    ch = ctx.chain_regions(taken, max_overlap=5)
    host = ch.to_host()
    qid, tid = p.hits.to_host()[:2]
    assert ch.row_coverage_ptr == 0
    with pytest.raises(ks.KmerseekError):
        ch.coverage_to_host()
    for mode, name in enumerate(("query", "target", "min", "max")):
        ptr = ch.coverage_from_host(p.hits, p.q[1], p.t[1], mode=name)
        assert ptr != 0 and ptr == ch.row_coverage_ptr
        got = ch.coverage_to_host()
        want = rchain_ref.coverage(host, qid, tid, p.q[1], p.t[1], mode)
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(want)].view(np.uint64), want[~np.isnan(want)].view(np.uint64))
        assert np.isnan(want).any() and (want[~np.isnan(want)] > 0).all() and (want[~np.isnan(want)] <= 1).all()
        bufs = [ctx.to_device(np.ascontiguousarray(a, np.uint64)) for a in (p.q[1], p.t[1])]  # from device pointers, the mode by number
        assert ch.coverage(p.hits, bufs[0].ptr, len(p.q[1]) - 1, bufs[1].ptr, len(p.t[1]) - 1, mode=mode) == ptr
        assert np.array_equal(ch.coverage_to_host(), got, equal_nan=True)
        for b in bufs:
            b.free()
    with pytest.raises(ValueError):
        ch.coverage_from_host(p.hits, p.q[1], p.t[1], mode="both")
    ch.free(); taken.free(); cu.free()


def _family_set():
    """Five families of proteins: a parent of 150 residues, a copy, the parent with 40 residues inserted, its first 100 residues,
    and its first 130: copies and the long prefix cover 80 percent of the shorter-or-longer sequence, the others do not."""
    rng = np.random.default_rng(99)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    seq = lambda n: bytes(aa[rng.integers(0, 20, n)])
    out = []
    for _ in range(5):
        p = seq(150)
        out += [p, p, p[:75] + seq(40) + p[75:], p[:100], p[:130]]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def test_coverage_as_the_edge_score_of_cluster_greedy(ctx):
    seqs = _family_set()
    p = _Pipe(ctx, seqs, seqs, 7)
    try:
        cu = ctx.cull_regions(p.al)
        taken = cu.take(p.al)
        ch = ctx.chain_regions(taken, max_overlap=5)
        ptr = ch.coverage_from_host(p.hits, p.q[1], p.t[1], mode="min")
        cov = ch.coverage_to_host()
        rows = p.hits.to_host()[:3]
        assert ((cov >= 0.8) & (rows[0] != rows[1])).any() and ((cov < 0.8) & (rows[0] != rows[1])).any()
        for assign in greedy_ref.ASSIGN:
            cl = ctx.cluster_greedy(p.hits, threshold=0.8, score=ptr, n_nodes=len(seqs), assign=assign)
            want = greedy_ref.cluster_hits("score", len(seqs), *rows, 0.8, score=cov, assign=assign)
            got = dict(zip(("label", "cluster_id", "offsets", "members", "representative"), cl.to_host()))
            for name, g in got.items():
                assert np.array_equal(g, want[name]), name
            assert 1 < cl.n_clusters == want["n_clusters"] < len(seqs)
            cl.free()
        ch.free(); taken.free(); cu.free()
    finally:
        p.close()


# ---- 7. the golden pair through the wire ----------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    chain_opts = {"chain_max_overlap": 5, "chain_skew_cost": 1}
    ref_opts = {"max_overlap": 5, "skew_cost": 1}
    plain = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True)
    chained = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, chain=True, **chain_opts)
    culled = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, cull=True, chain=True, **chain_opts)
    hit_rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, cull=True, chain=True, hit_rows=True, **chain_opts)
    p = _Pipe(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], 16, 5, "hp")
    al = p.al.to_host()
    qid, tid = p.hits.to_host()[:2]
    want = _al_ref(al, **ref_opts)
    assert chained == wire.region_rows(ced9_records, bcl2_records, qid, tid, p.rg.to_host(), "hp", alignments=al, chain=want)
    assert [{k: v for k, v in r.items() if k != "chain_pos"} for r in chained] == plain and len(plain) == 7
    assert sum(1 for r in chained if r["chain_pos"] >= 0) == len(want[1]) and all(r["chain_pos"] >= -1 for r in chained)
    cull = rcull_ref.cull(*al[:6])
    kept = (cull[0], *[np.asarray(c)[cull[1]] for c in al[1:]])
    want_kept = _al_ref(kept, **ref_opts)
    assert culled == wire.region_rows(ced9_records, bcl2_records, qid, tid, p.rg.to_host(), "hp", alignments=al, cull=cull, chain=want_kept)
    assert hit_rows == wire.hit_chain_rows(ced9_records, bcl2_records, qid, tid, want_kept)
    assert len(hit_rows) == int((np.diff(want_kept[0].astype(np.int64)) > 0).sum()) == p.hits.count > 0  # one row per hit
    by_name = {r["match_name"]: r for r in hit_rows}
    for r in range(len(qid)):
        row = by_name[bcl2_records[tid[r]][0]]
        assert row["chain_score"] == int(want_kept[4][r]) and row["n_alns"] == int(want_kept[0][r + 1] - want_kept[0][r])
        assert row["q_aligned"] == int(want_kept[9][r]) and row["t_aligned"] == int(want_kept[10][r])
    p.close()
    # scores only; a chain of nothing is refused, and so are hit rows without a chain
    s_rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, score=True, extend=True, x_drop=10, chain=True)
    assert s_rows and all("chain_pos" in r and "aln_score" not in r for r in s_rows)
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, chain=True)
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, hit_rows=True)


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, indel_pipe):
    L = ctx._L
    c = next(c for c in RH.CASES if c["name"] == "empty_rows_between")
    cols = RH.columns(c)
    bufs = [ctx.to_device(a) for a in cols]
    ptrs = [C.c_void_p(b.ptr) for b in bufs]
    n_rows, n = len(cols[0]) - 1, len(cols[1])
    before = ctx.pool_stats()["bytes_in_use"]
    two = C.c_uint32 * 2
    # the options: before any device work, with ctx == NULL too
    for o in (_lib.ks_rchain_opts(0, 0, 2 ** 30 + 1, 0, 0, 0, two(0, 0)), _lib.ks_rchain_opts(0, 0, 0, 2 ** 16 + 1, 0, 0, two(0, 0)),
              _lib.ks_rchain_opts(0, 0, 0, 0, 2 ** 16 + 1, 0, two(0, 0)), _lib.ks_rchain_opts(0, 0, 0, 0, 0, 1, two(0, 0)),
              _lib.ks_rchain_opts(0, 0, 0, 0, 0, 0, two(1, 0)), _lib.ks_rchain_opts(0, 0, 0, 0, 0, 0, two(0, 1))):
        for h in (ctx._h, None):
            out = C.c_void_p()
            assert L.ks_regions_chain_device(h, None, None, None, None, None, None, None, None, 0, 0, C.byref(o), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
            assert L.ks_raligns_chain(h, indel_pipe.al._h, C.byref(o), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
            assert L.ks_rscores_chain(h, indel_pipe.sc._h, C.byref(o), C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
    ok = _lib.ks_rchain_opts(2 ** 32 - 1, 2 ** 32 - 1, 2 ** 30, 2 ** 16, 2 ** 16, 0, two(0, 0))  # the bounds themselves pass
    out = C.c_void_p()
    assert L.ks_regions_chain_device(ctx._h, *ptrs, None, None, n_rows, n, C.byref(ok), C.byref(out)) == _lib.KS_OK
    L.ks_rchain_free(out)
    for kw in ({"link_cost": 2 ** 30 + 1}, {"skew_cost": 2 ** 16 + 1}, {"overlap_cost": 2 ** 16 + 1}, {"max_gap": -1}, {"max_overlap": 2 ** 32}):
        with pytest.raises(ValueError):
            ctx.chain_regions(indel_pipe.al, **kw)
    # NULL arguments
    out = C.c_void_p()
    assert L.ks_regions_chain_device(ctx._h, None, *ptrs[1:], None, None, n_rows, n, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_regions_chain_device(ctx._h, ptrs[0], None, *ptrs[2:], None, None, n_rows, n, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_regions_chain_device(ctx._h, *ptrs, None, None, n_rows, n, None, None) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_raligns_chain(ctx._h, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_rscores_chain(ctx._h, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    # row_offsets that is no CSR from 0 to n: the first bad row is named
    for bad, row in (([1, 1, 2, 2, 3, 3], 0), ([0, 0, 2, 1, 3, 3], 2), ([0, 0, 2, 2, 3, 2], 4), ([0, 0, 2, 2, 4, 4], 3), ([0, 0, 2, 2, 2, 2], 4)):
        ob = ctx.to_device(np.array(bad, np.uint64))
        with pytest.raises(ks.KmerseekError) as e:
            ctx.chain_regions_device(ob.ptr, *[b.ptr for b in bufs[1:]], n_rows, n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"hit row {row} " in str(e.value), (bad, str(e.value))
        ob.free()
    with pytest.raises(ks.KmerseekError) as e:  # regions without a row
        ctx.chain_regions_device(bufs[0].ptr, *[b.ptr for b in bufs[1:]], 0, n)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG
    # a length of 0, an end beyond 0xffffffff, a score of 2^30 + 1: the first such region is named
    # (lengths 10, 10, 5: a start of 2^32 - 10 puts region 1's end at 2^32, one of 2^32 - 5 region 2's)
    for col, value, region in ((2, 0, 1), (4, 0, 2), (1, 2 ** 32 - 10, 1), (3, 2 ** 32 - 5, 2), (5, 2 ** 30 + 1, 1), (5, -2 ** 30 - 1, 2)):
        z = cols[col].copy()
        z[region:] = value
        zb = ctx.to_device(z)
        with pytest.raises(ks.KmerseekError) as e:
            ctx.chain_regions_device(*[zb.ptr if i == col else b.ptr for i, b in enumerate(bufs)], n_rows, n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"region {region} " in str(e.value), (col, str(e.value))
        zb.free()
    for col, value in ((5, 2 ** 30), (5, -2 ** 30), (1, 2 ** 32 - 11), (3, 2 ** 32 - 11)):  # the bounds themselves pass
        z = cols[col].copy()
        z[1:] = value
        zb = ctx.to_device(z)
        ctx.chain_regions_device(*[zb.ptr if i == col else b.ptr for i, b in enumerate(bufs)], n_rows, n).free()
        zb.free()
    # more rows or regions than 32 bits index: refused before any device work
    for nr, ng in ((2 ** 32 - 2, n), (n_rows, 2 ** 32)):
        with pytest.raises(ks.KmerseekError) as e:
            ctx.chain_regions_device(*[b.ptr for b in bufs], nr, ng)
        assert e.value.status == _lib.KS_ERR_CAPACITY
    # objects of another context; coverage with hits of another row count, with ids beyond the batches, with other sequences
    ch = ctx.chain_regions(indel_pipe.al)
    small = ctx.chain_regions_device(*[b.ptr for b in bufs], n_rows, n)
    q_off, t_off = indel_pipe.q[1], indel_pipe.t[1]
    with ks.Context(0) as other:
        out = C.c_void_p()
        assert other._L.ks_raligns_chain(other._h, indel_pipe.al._h, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
        assert other._L.ks_rscores_chain(other._h, indel_pipe.sc._h, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
        assert other._L.ks_rchain_coverage(other._h, ch._h, indel_pipe.hits._h, ptrs[0], 1, ptrs[0], 1, 0) == _lib.KS_ERR_INVALID_ARG
    with pytest.raises(ks.KmerseekError) as e:
        small.coverage_from_host(indel_pipe.hits, q_off, t_off)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hits of other regions" in str(e.value)
    with pytest.raises(ks.KmerseekError) as e:  # fewer targets than the hits name
        ch.coverage_from_host(indel_pipe.hits, q_off, t_off[:2])
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit row " in str(e.value)
    with pytest.raises(ks.KmerseekError) as e:  # sequences a tenth as long: the chains do not fit
        ch.coverage_from_host(indel_pipe.hits, q_off // 10, t_off // 10)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit row 0 " in str(e.value) and ch.row_coverage_ptr == 0
    assert L.ks_rchain_coverage(ctx._h, None, indel_pipe.hits._h, ptrs[0], 1, ptrs[0], 1, 0) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_rchain_coverage(ctx._h, ch._h, None, ptrs[0], 1, ptrs[0], 1, 0) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_rchain_coverage(ctx._h, ch._h, indel_pipe.hits._h, None, 1, ptrs[0], 1, 0) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_rchain_coverage(ctx._h, ch._h, indel_pipe.hits._h, ptrs[0], 1, ptrs[0], 1, 4) == _lib.KS_ERR_INVALID_ARG
    ch.free(); small.free()
    assert ctx.pool_stats()["bytes_in_use"] == before
    # the context stays usable
    RH.assert_same(device_chain(ctx, cols), RH.expected(c))
    for b in bufs:
        b.free()


RUNGS = 8


def test_pool_refusals_leave_nothing_behind(monkeypatch):
    """The method of tests/test_gpu_error_paths.py: a ladder of KS_DEBUG_POOL_CAP values through the driver's allocations, a fresh
    context per rung.  A refused rung is KS_ERR_OOM "pool cap", leaves bytes_in_use where it was and the context usable; the
    last rung fits and gives the right result."""
    cols = fuzz_input()
    want = reference("fuzz", (), "full")

    def run(cap=None):
        with ks.Context(0, follow_debug_env=True) as c:
            bufs = [c.to_device(a) for a in cols]
            before = c.pool_stats()["bytes_in_use"]
            call = lambda: c.chain_regions_device(*[b.ptr for b in bufs[:6]], len(cols[0]) - 1, len(cols[1]), d_identities=bufs[6].ptr,
                                                  d_aln_length=bufs[7].ptr)
            if cap is not None:
                monkeypatch.setenv("KS_DEBUG_POOL_CAP", str(cap))
            try:
                ch, err = call(), None
            except ks.KmerseekError as e:
                ch, err = None, e
            finally:
                monkeypatch.delenv("KS_DEBUG_POOL_CAP", raising=False)
            if err is not None:
                assert err.status == _lib.KS_ERR_OOM and "pool cap" in str(err), (cap, str(err))
                assert c.pool_stats()["bytes_in_use"] == before, cap
                ch = call()  # the same context, the cap gone
            RH.assert_same(ch.to_host(), want, f"cap {cap}")
            ch.free()
            assert c.pool_stats()["bytes_in_use"] == before
            return err is not None, before, c.pool_stats()["bytes_held"]

    _, lo, hi = run()
    assert hi > lo
    refused = [run(lo + (hi - lo) * i // (RUNGS - 1))[0] for i in range(RUNGS)]
    print(f"region chain: bytes_in_use {lo}, bytes_held {hi}, refused rungs {refused}")
    assert any(refused) and not refused[-1]
