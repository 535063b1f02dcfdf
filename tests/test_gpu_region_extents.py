"""GPU: the region pipeline after match_regions — align, trace, cull, take, chain, stitch — at the extents its contracts allow and
on real proteins (tests/rextent_cases.py has the inputs, tests/test_region_extents_cpu.py shows from the references alone that
they are what they claim to be).  Every comparison is exact.

1. fills of ks_regions_stitch with a long side around two stages, around the default max_fill and around its limit, a short side of
   1, 2, 63 and 64, both orientations: the class of every link, every array against tests/rstitch_ref.py, the fill's score against
   an independent global optimum (test_region_extents_cpu.gotoh_global), and the same under a scratch budget of one link;
2. one pair of relatives with every class of link, stage by stage against the references and against a CIGAR written by hand;
3. alignments of 2^20 columns whose extents, scores and CIGARs are stated on paper (no reference walks 2^20 rows);
4. seventeen human proteins all against all, stage by stage against the references, and through the wire."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rchain_cases as RH  # noqa: E402
import rchain_ref  # noqa: E402
import rcull_cases as RC  # noqa: E402
import rcull_ref  # noqa: E402
import rextent_cases as EC  # noqa: E402
import rstitch_ref as SR  # noqa: E402
import rtrace_ref  # noqa: E402
import test_gpu_region_stitch as TS  # noqa: E402  (its _Pipe and check_invariants)
from test_region_extents_cpu import gotoh_global  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

M, I, D, EQ, X = SR.M, SR.I, SR.D, SR.EQ, SR.X


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


def _stage():
    s = int(_lib.load().ks_debug_rstitch_stage())
    assert s == EC.STAGE
    return s


# ---- 1. long fills ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(EC.long_sides()))
def test_mismatch_fills(ctx, group):
    """W's against Y's: the class of every link at max_fill 0, 1024 and 4096, an open link literally, a filled one by the closed
    form (min(X, Y) mismatched pairs and one run of the difference) and by the independent optimum."""
    shapes, qs, ts = EC.mismatch_batch(EC.long_sides(_stage())[group], seed=11)
    p = TS._Pipe(ctx, qs, ts, EC.EXACT)
    m = ralign_ref.default_matrix()
    try:
        assert p.qid.tolist() == p.tid.tolist() == list(range(len(shapes)))  # hit row r is shape r
        got = {}
        with EC.FILLS:
            for max_fill in (0, 1024, 4096):
                got[max_fill] = g = p.check(f"{group} max_fill={max_fill}", eqx=(True, False), max_fill=max_fill)
                text = SR.strings(g[0], g[1])
                rows = 0
                for r, (x, y) in enumerate(shapes):
                    cigar, score, n_filled, n_open, opens, length = EC.mismatch_row(x, y, max_fill)
                    assert (g[12][r], g[13][r], g[14][r], g[15][r]) == (2, n_filled, n_open, 0), (x, y, max_fill)
                    assert (g[6][r], g[9][r], g[11][r], g[16][r]) == (score, opens, length, float(score)), (x, y, max_fill, text[r])
                    assert cigar is None or text[r] == cigar, (x, y, max_fill, text[r])
                    if n_filled:
                        qm, tm = EC.middles(qs[r], ts[r])
                        assert int(g[6][r]) - 60 == gotoh_global(qm, tm, m, 11, 1), (x, y, max_fill)
                        rows += (max(x, y) + 1) // 2 * 2
                assert p.last == (1, 64 * rows)  # one slice; 64 bytes per row of the longer side of every filled link
        SR.assert_same(got[0], got[1024], "max_fill 0 is 1024")
        assert got[4096][13].sum() >= got[0][13].sum() and (max(max(s) for s in shapes) < 4095 or got[0][13].sum() == 0)
    finally:
        p.close()


def test_limit_fills_one_per_slice_and_the_refusal(ctx):
    """A budget of exactly one 4096-row link: every filled link runs in a slice of its own and nothing changes; one row less and
    the first filled link is refused by name, the pool as it was, the context usable."""
    shapes, qs, ts = EC.mismatch_batch(EC.SLICED[0], seed=13, shorts=EC.SLICED[1])
    p = TS._Pipe(ctx, qs, ts, EC.EXACT)
    try:
        with EC.FILLS:
            whole = p.check("whole", eqx=(False,), max_fill=4096)
            n_filled = int(whole[13].sum())
            link_rows = [r for x, y in shapes for r in (0, (max(x, y) + 1) // 2 * 2 if EC.link_class(x, y, 4096) == "filled" else 0)]
            assert p.last[0] == 1 and n_filled == 8 and link_rows == [0, 4096] * 8
            sliced = p.check("one link per slice", eqx=(False,), max_fill=4096, max_scratch_bytes=64 * 4096)
            assert p.last == (n_filled, 64 * 4096) and EC.slices_of(link_rows, 4096) == n_filled
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, sliced))
            before = ctx.pool_stats()["bytes_in_use"]
            first = int(np.flatnonzero(whole[13])[0])
            member = int(p.ch_host[0][first]) + 1  # the second member of the first row with a filled link
            assert EC.slices_of(link_rows, 4095) == -1 - member
            with pytest.raises(ks.KmerseekError) as e:
                p.stitch(max_fill=4096, max_scratch_bytes=64 * 4095)
            assert e.value.status == _lib.KS_ERR_CAPACITY and f"chain member {member} " in str(e.value) and "max_scratch_bytes" in str(e.value)
            assert ctx.pool_stats()["bytes_in_use"] == before
            SR.assert_same(p.check("after the refusal", eqx=(False,), max_fill=4096), whole, "after the refusal")
    finally:
        p.close()


@pytest.mark.parametrize("gaps", EC.PATH_GAPS, ids=lambda g: f"gap{g[0]}_{g[1]}")
@pytest.mark.parametrize("seeded", (False, True), ids=("plus_minus_1", "seeded_matrix"))
def test_path_fills(ctx, seeded, gaps):
    """Middles with a real path — gap runs of thousands of rows with pairs on either side — under +1 / -1 and under a seeded
    asymmetric matrix, with gap costs that make ties: the reference, the independent optimum, and one link per slice."""
    o, e = gaps
    matrix = EC.path_matrix(17) if seeded else None
    m = ralign_ref.default_matrix() if matrix is None else [[int(v) for v in row] for row in matrix.tolist()]
    shapes, qs, ts = EC.path_batch(seed=23, stage=_stage())
    p = TS._Pipe(ctx, qs, ts, dict(EC.EXACT, gap_open=o, gap_extend=e, matrix=matrix))
    try:
        assert p.qid.tolist() == p.tid.tolist() == list(range(len(shapes))) and p.al.n_regions == 2 * len(shapes)
        with EC.FILLS:
            got = p.check(f"paths {seeded} {gaps}", eqx=(True, False), max_fill=4096)
            assert (got[12] == 2).all() and (got[13] == 1).all() and (got[14] == 0).all() and (got[15] == 0).all()
            for r, (x, y) in enumerate(shapes):
                qm, tm = EC.middles(qs[r], ts[r])
                flanks = int(p.al_host[5][2 * r]) + int(p.al_host[5][2 * r + 1])  # EXACT leaves nothing to trim
                assert (len(qm), len(tm)) == (x, y) and int(got[6][r]) - flanks == gotoh_global(qm, tm, m, o, e), (x, y)
            assert p.last[0] == 1
            sliced = p.check("sliced", eqx=(False,), max_fill=4096, max_scratch_bytes=64 * 4096)
            assert p.last[0] >= 4 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, sliced))
    finally:
        p.close()


# ---- every stage against its reference ------------------------------------------------------------------------------------------
class _Seeds:
    """queries x targets up to the regions, on the device."""

    def __init__(self, ctx, queries, targets, k=EC.K):
        self.ctx, self.q, self.t = ctx, ks.pack(queries), ks.pack(targets)
        q, t = self.q, self.t
        T = ctx.sketch_batch(t[0], t[1], k, 1, "protein")
        Q = ctx.sketch_batch(q[0], q[1], k, 1, "protein")
        self.hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table(q[0], q[1], k, 1, "protein")
        tp = ctx.kmer_positions_table(t[0], t[1], k, 1, "protein")
        mp = ctx.match_positions(qp, tp, self.hits)
        self.rg = ctx.match_regions(mp)
        for o in (mp, qp, tp, Q, T):
            o.free()
        self.qid, self.tid = self.hits.to_host()[:2]
        self.rg_host = self.rg.to_host()

    def close(self):
        self.rg.free()
        self.hits.free()


class _Stages:
    """The regions of a _Seeds through align, cull, take and chain on the device, every result copied to the host; trace and
    stitch on demand.  (al_host, ch_host, qid, tid, q, t: what test_gpu_region_stitch.check_invariants reads.)"""

    def __init__(self, seeds, align, chain=None):
        s = self.seeds = seeds
        self.ctx, self.q, self.t, self.qid, self.tid, self.align, self.chain_opts = s.ctx, s.q, s.t, s.qid, s.tid, align, chain or {}
        self.times = {}
        self.al_all = self._timed("align", s.ctx.align_regions, s.rg, s.hits, *self.batches(), **align)
        self.cu = s.ctx.cull_regions(self.al_all)
        self.rg, self.al = self.cu.take(s.rg), self.cu.take(self.al_all)
        self.ch = s.ctx.chain_regions(self.al, **self.chain_opts)
        self.all_host, self.cu_host, self.kept_host = self.al_all.to_host(), self.cu.to_host(), self.rg.to_host()
        self.al_host, self.ch_host = self.al.to_host(), self.ch.to_host()

    def batches(self):
        return self.q[0], self.q[1], self.t[0], self.t[1]

    def _timed(self, what, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        self.times[what] = time.perf_counter() - t0
        return out

    def trace(self, eqx=False, **kw):
        return self._timed("trace", self.ctx.trace_regions, self.rg, self.seeds.hits, *self.batches(), self.al, eqx=eqx, **kw)

    def stitch(self, cg, eqx=False, **kw):
        return self._timed("stitch", self.ctx.stitch_chains, self.ch, self.al, cg, self.seeds.hits, *self.batches(), eqx=eqx, **kw)

    def matrix(self):
        m = self.align.get("matrix")
        return ralign_ref.default_matrix() if m is None else [[int(v) for v in row] for row in np.asarray(m).tolist()]

    def check_front(self, what):
        """align, cull, take and chain against their references, each on the device's input to that stage."""
        s, kw = self.seeds, {**EC.PROBE, **self.align}
        want = ralign_ref.align(s.rg_host, self.qid, self.tid, *self.batches(), **kw)
        assert len(self.all_host) == len(want) == len(ralign_ref.COLUMNS)
        for g, w, name in zip(self.all_host, want, ralign_ref.COLUMNS):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:8].tolist())
        RC.assert_same(self.cu_host, rcull_ref.cull(*self.all_host[:6]), what)
        src = self.cu_host[1].astype(np.int64)
        for got, whole in ((self.al_host, self.all_host), (self.kept_host, s.rg_host)):
            assert np.array_equal(got[0], self.cu_host[0]) and len(got) == len(whole)
            assert all(g.dtype == w.dtype and np.array_equal(g, np.asarray(w)[src]) for g, w in zip(got[1:], whole[1:])), what
        al = self.al_host
        RH.assert_same(self.ch_host, rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **self.chain_opts), what)

    def check_trace(self, what, eqx, cg):
        """-> the device's (op_offsets, ops): equal to rtrace_ref.trace, and re-scored they give the device's columns."""
        kw = {k: v for k, v in {**EC.PROBE, **self.align}.items() if k != "x_drop"}
        offs, ops = cg.to_host()
        w_offs, w_ops = EC.encode([c for c, _ in rtrace_ref.trace(self.kept_host, self.al_host, self.qid, self.tid, *self.batches(), eqx=eqx, **kw)])
        assert offs.dtype == w_offs.dtype and ops.dtype == w_ops.dtype and np.array_equal(offs, w_offs) and np.array_equal(ops, w_ops), what
        m, al = self.matrix(), [c.tolist() for c in self.al_host]
        q_bytes, t_bytes = bytes(self.q[0]), bytes(self.t[0])
        for r in range(len(self.qid)):
            qseq = q_bytes[int(self.q[1][self.qid[r]]):int(self.q[1][self.qid[r] + 1])]
            tseq = t_bytes[int(self.t[1][self.tid[r]]):int(self.t[1][self.tid[r] + 1])]
            for g in range(al[0][r], al[0][r + 1]):
                cigar = [(int(v) >> 4, int(v) & 15) for v in ops[int(offs[g]):int(offs[g + 1])]]
                score, ident, pos, opens, gaps, length, ql, tl = rtrace_ref.rescore(cigar, qseq, tseq, al[1][g], al[3][g], m, kw["gap_open"], kw["gap_extend"])
                assert (ql, tl, score, ident, pos, opens, gaps, length) == tuple(al[i][g] for i in (2, 4, 5, 6, 7, 8, 9, 10)), (what, g)
        return offs, ops

    def host(self):
        return dict(chain=self.ch_host, alignments=self.al_host, hits=(self.qid, self.tid), q=self.q, t=self.t)

    def check_stitch(self, what, eqx, cg, max_fill=0, **kw):
        """-> the device's arrays: equal to rstitch_ref.stitch on the device's chain, alignments and ops, invariants and all."""
        st = self.stitch(cg, eqx=eqx, max_fill=max_fill, **kw)
        got = st.to_host()
        assert st.n_rows == len(self.qid) and st.strings() == SR.strings(got[0], got[1])
        self.last = st.n_slices, st.scratch_bytes
        st.free()
        kw = {**EC.PROBE, **self.align}
        want = EC.ref_stitch(self.host(), matrix=kw.get("matrix"), gap_open=kw["gap_open"], gap_extend=kw["gap_extend"], max_fill=max_fill,
                             eqx=eqx, cigars=cg.to_host())[0]
        SR.assert_same(got, want, what)
        TS.check_invariants(self, got, eqx)
        return got

    def close(self):
        for o in (self.ch, self.al, self.rg, self.cu, self.al_all):
            o.free()


# ---- 2. the pair of relatives ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", range(len(EC.RELATIVE_CONFIGS)), ids=("band16_xdrop30", "band31_no_xdrop"))
def test_relative_pair_through_every_stage(ctx, config):
    q, t, cols = EC.relative_pair()
    seeds = _Seeds(ctx, [q], [t])
    p = _Stages(seeds, EC.RELATIVE_CONFIGS[config], chain=EC.CHAIN)
    try:
        assert seeds.rg.n_regions == sum(len(i) for _, i in EC.STRETCHES)
        p.check_front("relatives")                                                  # columns, cull, take, chain
        assert p.cu_host[3].tolist() == list(EC.RELATIVE_MERGED)                    # the islands of one stretch: one alignment
        assert p.ch_host[1].tolist() == list(range(EC.RELATIVE_MEMBERS))           # six members, hand-counted
        for eqx in (False, True):
            cg = p.trace(eqx)
            offs, ops = p.check_trace("relatives", eqx, cg)
            for max_fill in (0, 4096):
                got = p.check_stitch(f"relatives eqx={eqx} max_fill={max_fill}", eqx, cg, max_fill=max_fill)
                assert SR.strings(got[0], got[1]) == [EC.relative_cigar(cols, max_fill, eqx)], (eqx, max_fill)
                assert (got[12][0], got[13][0], got[14][0], got[15][0]) == (EC.RELATIVE_MEMBERS, *EC.relative_counts(max_fill), 0)
            # the same through a traceback in slices: a budget of the longest region's rows (and one stage to spare)
            budget = 64 * (int(p.al_host[2].max()) + 64)
            cut = p.trace(eqx, max_scratch_bytes=budget)
            c_offs, c_ops = cut.to_host()
            assert cg.n_slices == 1 and cut.n_slices >= 3 and cut.scratch_bytes <= budget
            assert np.array_equal(c_offs, offs) and np.array_equal(c_ops, ops)
            again = p.check_stitch("relatives, sliced traceback", eqx, cut, max_fill=4096)
            assert SR.strings(again[0], again[1]) == [EC.relative_cigar(cols, 4096, eqx)]
            cut.free(); cg.free()
    finally:
        p.close(); seeds.close()


# ---- 3. the capacity limit, on paper ----------------------------------------------------------------------------------------------------
N3 = EC.CAPACITY  # the length of this section's sequences: 2^20, the contract's limit


def _single(p, eqx=False):
    """Trace and stitch a pipeline whose rows have one member each -> (cigar strings, stitched arrays)."""
    cg = p.trace(eqx)
    st = p.stitch(cg, eqx=eqx)
    got = st.to_host()
    text = cg.strings()
    assert st.strings() == text and (got[12] == 1).all() and not got[13].any() and not got[14].any() and not got[15].any()
    for i, j in zip((2, 3, 4, 5, 6, 7, 8, 9, 10, 11), (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)):  # a row of one member: its alignment's columns
        assert np.array_equal(got[i], p.al_host[j])
    assert got[16].dtype == np.float64 and got[16].tolist() == [float(int(v)) for v in p.al_host[5]]
    scratch = cg.scratch_bytes
    st.free(); cg.free()
    return text, got, scratch


def test_capacity_unrelated_pair_under_extreme_matrices(ctx):
    """Two unrelated sequences of 2^20 residues that share CORE at offsets 1000 and 1037.  All +127: every pair scores, so the
    alignment is the whole diagonal through the anchor, clipped by the two ends — 2^20 - 37 pairs, a score of 127 times that.
    -128 but for W over W and Y over Y: no pair outside CORE scores above -128, one row beyond it drops by more than x_drop
    whichever way it is reached (a gap costs 12 and then 1 a row: 20 rows later the best of the row has dropped by 31) — CORE
    alone, twelve pairs of +127."""
    q, t = EC.unrelated_pair(N3)
    t0 = time.perf_counter()
    seeds = _Seeds(ctx, [q], [t], k=EC.K_LONG)
    print(f"\n[extents] n = {N3}: sketch, search and regions of the unrelated pair {time.perf_counter() - t0:.2f} s")
    try:
        assert seeds.hits.count == 1 and seeds.rg.n_regions == 1 and seeds.rg_host[3].tolist() == [len(EC.CORE)]
        d = EC.T_CORE_AT - EC.Q_CORE_AT
        n = N3 - d
        p = _Stages(seeds, dict(matrix=EC.all_127(), band=16, gap_open=11, gap_extend=1, x_drop=30))
        try:
            diag = int((np.frombuffer(q, np.uint8)[:n] == np.frombuffer(t, np.uint8)[d:]).sum())
            assert [int(c[0]) for c in p.al_host[1:]] == [0, n, d, n, 127 * n, diag, n, 0, 0, n]
            text, got, scratch = _single(p)
            assert text == [f"{n}M"] and got[16][0] == float(127 * n) and scratch == EC.trace_scratch(p.kept_host, p.al_host)
            print(f"[extents] all +127: align {p.times['align']:.3f} s, trace {p.times['trace']:.3f} s, stitch {p.times['stitch']:.3f} s")
        finally:
            p.close()
        p = _Stages(seeds, dict(matrix=EC.core_only_matrix(), band=16, gap_open=11, gap_extend=1, x_drop=30))
        try:
            c = len(EC.CORE)
            assert [int(col[0]) for col in p.al_host[1:]] == [EC.Q_CORE_AT, c, EC.T_CORE_AT, c, 127 * c, c, c, 0, 0, c]
            p.check_front("core alone")  # (the references stop with the X-drop as well: a few dozen rows)
            text, got, _ = _single(p, eqx=True)
            assert text == [f"{c}="] and got[16][0] == float(127 * c)
        finally:
            p.close()
    finally:
        seeds.close()


def test_capacity_identical_and_deleted_pair(ctx):
    """A sequence of 2^20 residues against itself and against a copy without 20 residues at the midpoint, band 31, +1 / -1, gaps
    (11, 1), x_drop 30: 1048576M, and <a>M20I<b>M from either of the two seeds — one kept alignment, a chain of one."""
    full, cut = EC.deleted_pair(N3)
    t0 = time.perf_counter()
    seeds = _Seeds(ctx, [full], [full, cut], k=EC.K_LONG)
    print(f"\n[extents] n = {N3}: sketch, search and regions of the deleted pair {time.perf_counter() - t0:.2f} s")
    p = _Stages(seeds, dict(band=31, gap_open=11, gap_extend=1, x_drop=30))
    try:
        n, gap = N3, EC.DELETED
        a, b = n // 2, n - n // 2 - gap
        assert seeds.tid.tolist() == [0, 1] and seeds.rg_host[0].tolist() == [0, 1, 3]
        assert p.cu_host[3].tolist() == [1, 2] and p.al_host[0].tolist() == [0, 1, 2] and p.ch_host[1].tolist() == [0, 1]
        assert [c.tolist() for c in p.al_host[1:]] == [[0, 0], [n, n], [0, 0], [n, n - gap], [n, n - gap - (11 + gap)], [n, n - gap],
                                                       [n, n - gap], [0, 1], [0, gap], [n, n]]
        for eqx, pair in ((False, "M"), (True, "=")):
            text, got, scratch = _single(p, eqx)
            assert text == [f"{n}{pair}", f"{a}{pair}{gap}I{b}{pair}"]
            assert scratch == EC.trace_scratch(p.kept_host, p.al_host) >= 64 * 2 * (n - 2)
        print(f"[extents] deleted pair: align {p.times['align']:.3f} s, trace {p.times['trace']:.3f} s, stitch {p.times['stitch']:.3f} s")
    finally:
        p.close(); seeds.close()


# ---- 4. real proteins -------------------------------------------------------------------------------------------------------------------
def _real(ctx, what, eqx, matrix=None, wire_rows=False):
    recs = EC.real_records()
    seqs = [s for _, s in recs]
    seeds = _Seeds(ctx, seqs, seqs)
    p = _Stages(seeds, dict(EC.PROBE, matrix=matrix), chain=EC.CHAIN)
    try:
        p.check_front(what)
        cg = p.trace(eqx)
        p.check_trace(what, eqx, cg)
        got = p.check_stitch(what, eqx, cg)
        if wire_rows:  # the rows a caller sees, built from the device's output and from the references'
            al = p.al_host
            ch = rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **EC.CHAIN)
            want = EC.ref_stitch(dict(p.host(), chain=ch), eqx=eqx, cigars=cg.to_host())[0]
            rows = wire.hit_chain_rows(recs, recs, p.qid, p.tid, p.ch_host, stitched=got)
            assert rows == wire.hit_chain_rows(recs, recs, p.qid, p.tid, ch, stitched=want) and len(rows) == len(p.qid)
        cg.free()
        return p.al_host, got
    finally:
        p.close(); seeds.close()


def test_real_proteins_through_every_stage(ctx):
    al, got = _real(ctx, "real proteins", eqx=False, wire_rows=True)
    assert got[13].sum() >= 3 and got[14].sum() >= 3 and got[12].max() >= 3 and al[10].max() >= 2000


def test_real_proteins_with_eqx(ctx):
    _, got = _real(ctx, "real proteins, eqx", eqx=True)
    assert got[13].sum() >= 3 and got[14].sum() >= 3


def test_real_proteins_under_a_seeded_matrix(ctx):
    _real(ctx, "real proteins, seeded matrix", eqx=False, matrix=EC.random_matrix(29))
