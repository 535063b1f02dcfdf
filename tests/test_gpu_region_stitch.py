"""GPU: ks_regions_stitch — the chain of every hit row as one gapped alignment with one CIGAR.

Every result array is compared exactly with the plain-loop restatement of tests/rstitch_ref.py, run on the host copies of what
the device stages before it produced (chain, alignments, CIGARs: each has its own tests); the fixed pairs also with the
hand-written CIGARs of tests/rstitch_cases.py.  Cases: the fixed pairs; rows of 0, 1, 2 and 9 members; rectangles with a short
side of 0, 1, 62, 63, 64 and a long side around the stage and around max_fill = 70, both orientations and squares; M / I / D and
= / X; the two fuzz batches whole and in at least three slices, and a chain of doctored columns whose second member is trimmed to nothing
(tests/test_region_stitch_cpu.py shows on the CPU that together they go through every class of link, trim and tie); the invariants of the header on the device's own output; row_score as the rank
key of best_hits; the golden pair through the wire; every refusal, with the context usable afterwards."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rstitch_cases as SC  # noqa: E402
import rstitch_ref as SR  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
M, I, D, EQ, X = SR.M, SR.I, SR.D, SR.EQ, SR.X
EXACT = dict(band=0, gap_open=11, gap_extend=1, x_drop=0)  # an alignment is the exact matches around its seed


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


class _Pipe:
    """queries x targets up to what the stitch takes, on the device: hits, the alignments the cull kept, their paths (traced
    with and without eqx, on demand) and their chain."""

    def __init__(self, ctx, queries, targets, align, chain=None, k=SC.K, scaled=1, mol="protein", min_kmers=1, cull_opts=None, cull=True):
        self.ctx, self.q, self.t, self.align = ctx, ks.pack(queries), ks.pack(targets), align
        q, t = self.q, self.t
        T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
        Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
        self.hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
        tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
        mp = ctx.match_positions(qp, tp, self.hits)
        rg = ctx.match_regions(mp, min_kmers=min_kmers)
        al = ctx.align_regions(rg, self.hits, q[0], q[1], t[0], t[1], **align)
        if cull:
            cu = ctx.cull_regions(al, **(cull_opts or {}))
            self.rg, self.al = cu.take(rg), cu.take(al)
            for o in (cu, al, rg):
                o.free()
        else:
            self.rg, self.al = rg, al
        self.ch = ctx.chain_regions(self.al, **(chain or {}))
        self.cg = {}
        for o in (mp, qp, tp, Q, T):
            o.free()
        self.qid, self.tid = self.hits.to_host()[:2]
        self.al_host, self.ch_host = self.al.to_host(), self.ch.to_host()

    def cigars(self, eqx):
        if eqx not in self.cg:
            self.cg[eqx] = self.ctx.trace_regions(self.rg, self.hits, self.q[0], self.q[1], self.t[0], self.t[1], self.al, eqx=eqx)
        return self.cg[eqx]

    def stitch(self, eqx=False, **kw):
        return self.ctx.stitch_chains(self.ch, self.al, self.cigars(eqx), self.hits, self.q[0], self.q[1], self.t[0], self.t[1], eqx=eqx, **kw)

    def ref(self, eqx=False, max_fill=0):
        return SR.stitch(self.ch_host, self.al_host, self.cigars(eqx).to_host(), self.qid, self.tid, self.q[0], self.q[1], self.t[0], self.t[1],
                         matrix=self.align.get("matrix"), gap_open=self.align["gap_open"], gap_extend=self.align["gap_extend"], max_fill=max_fill,
                         eqx=eqx)[0]

    def check(self, what, eqx=(False, True), max_fill=0, own_chain=True, **kw):
        """Stitched on the device and by the reference, for each eqx -> the device's arrays of the last one."""
        got = None
        for x in eqx:
            st = self.stitch(eqx=x, max_fill=max_fill, **kw)
            got = st.to_host()
            assert st.n_rows == len(self.qid) and st.n_ops == len(got[1]) == int(got[0][-1]) and all(p != 0 for p in st.device_ptrs())
            assert st.row_score_ptr == st.device_ptrs()[16] and st.strings() == SR.strings(got[0], got[1])
            assert all(np.array_equal(a, b) for a, b in zip(st.ops_to_host(), got[:2]))
            SR.assert_same(got, self.ref(x, max_fill), f"{what} eqx={x}")
            check_invariants(self, got, x, own_chain)
            self.last = st.n_slices, st.scratch_bytes
            st.free()
        return got

    def close(self):
        for o in (*self.cg.values(), self.ch, self.al, self.rg, self.hits):
            o.free()


def check_invariants(p, got, eqx, own_chain=True):
    """What the header promises of every row, on the device's own output.  own_chain: the chain was made of these alignments
    (its span columns are theirs)."""
    offs, ops = got[0].tolist(), got[1].tolist()
    c_offs, src = p.ch_host[0].tolist(), p.ch_host[1].tolist()
    for r in range(len(offs) - 1):
        mine = [(v >> 4, v & 15) for v in ops[offs[r]:offs[r + 1]]]
        assert all(a[1] != b[1] for a, b in zip(mine, mine[1:])) and all(k >= 1 for k, _ in mine)  # merged runs
        assert {c for _, c in mine} <= ({EQ, X, I, D} if eqx else {M, I, D})
        pairs = sum(k for k, c in mine if c in (M, EQ, X))
        assert sum(k for k, _ in mine) == got[11][r]                                  # the ops sum to aln_length
        assert pairs + sum(k for k, c in mine if c == I) == got[3][r]                # pairs + I = q_length
        assert pairs + sum(k for k, c in mine if c == D) == got[5][r]                # pairs + D = t_length
        assert sum(1 for _, c in mine if c in (I, D)) == got[9][r] and sum(k for k, c in mine if c in (I, D)) == got[10][r]
        if eqx:
            assert sum(k for k, c in mine if c == EQ) == got[7][r]
        assert got[12][r] == c_offs[r + 1] - c_offs[r]
        assert np.isnan(got[16][r]) == (got[12][r] == 0) and (got[12][r] == 0 or got[16][r] == float(got[6][r]))
        if got[12][r] == 1:  # a single-member row reproduces its alignment's columns
            g = src[c_offs[r]]
            assert [int(got[i][r]) for i in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11)] == [int(p.al_host[i][g]) for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)]
            assert (got[13][r], got[14][r], got[15][r]) == (0, 0, 0)
    for i, j in ((2, 5), (3, 6), (4, 7), (5, 8)):  # the span equals the chain's
        assert not own_chain or np.array_equal(got[i], p.ch_host[j])


def _row(p, qi, ti):
    return int(np.flatnonzero((p.qid == qi) & (p.tid == ti))[0])


# ---- 1. the fixed pairs ----------------------------------------------------------------------------------------------------------------
def test_fixed_pairs(ctx):
    for name, q, t, opts, want, want_eqx in SC.pipe_cases():
        p = _Pipe(ctx, [q], [t], opts)
        try:
            for eqx, w in ((False, want), (True, want_eqx)):
                st = p.stitch(eqx=eqx)
                assert st.strings() == [w], name
                st.free()
            got = p.check(name)
            assert (got[2][0], got[3][0], got[4][0], got[5][0], got[12][0]) == (0, len(q), 0, len(t), 2)
            if name == "insertion_pair":  # one alignment with a single long I where the chain had two alignments and a hole
                s0, s1 = (int(v) for v in p.al_host[5])
                assert got[6][0] == s0 + s1 - (11 + SC.INSERTION) and (got[9][0], got[10][0], got[7][0]) == (1, SC.INSERTION, 120)
        finally:
            p.close()


# ---- 2. rows of 0, 1, 2 and 9 members -------------------------------------------------------------------------------------------------
def test_rows_of_0_1_2_and_9_members(ctx):
    rng = np.random.default_rng(77)
    blocks = [SC._seq(rng, 20, SC.FLANK) for _ in range(9)]
    nine_q = b"".join(b + b"W" * 10 for b in blocks[:-1]) + blocks[-1]   # eight insertions of 10: band 4 bridges none
    nine_t = b"".join(blocks)
    one = SC._seq(rng, 50, SC.FLANK)
    two_q, two_t = SC._flanked(rng, b"W" * 12, b"Y" * 3)
    lone = SC._seq(rng, 7, SC.FLANK)  # one shared k-mer: a hit row whose one-k-mer region min_kmers = 2 drops
    none_q, none_t = SC._seq(rng, 20, SC.FLANK) + lone + SC._seq(rng, 20, SC.FLANK), SC._seq(rng, 20, SC.FLANK) + lone + SC._seq(rng, 20, SC.FLANK)
    p = _Pipe(ctx, [nine_q, one, two_q, none_q], [nine_t, one, two_t, none_t], dict(band=4, gap_open=2, gap_extend=1, x_drop=6), min_kmers=2)
    try:
        got = p.check("member counts", eqx=(True, False))
        members = {(int(p.qid[r]), int(p.tid[r])): int(got[12][r]) for r in range(len(p.qid))}
        assert [members[(i, i)] for i in range(4)] == [9, 1, 2, 0]
        r9, r0 = _row(p, 0, 0), _row(p, 3, 3)
        assert SR.strings(got[0], got[1])[r9] == "20M" + "10I20M" * 8 and got[9][r9] == 8
        assert got[0][r0 + 1] == got[0][r0] and np.isnan(got[16][r0]) and not any(int(got[i][r0]) for i in range(2, 16))
    finally:
        p.close()


# ---- 3. rectangles around the lanes, the stage and max_fill ------------------------------------------------------------------------------
MAX_FILL = 70


def _shapes():
    stage = int(_lib.load().ks_debug_rstitch_stage())
    assert stage + 1 < MAX_FILL
    longs = (stage - 1, stage, stage + 1, MAX_FILL, MAX_FILL + 1)
    shapes = {(a, b) for a in longs for b in (0, 1, 62, 63, 64)}
    shapes |= {(b, a) for a, b in shapes} | {(n, n) for n in (1, 2, 62, 63, 64)}
    return sorted(shapes - {(0, 0)})


def test_rectangles_around_the_stage_and_max_fill(ctx):
    """All-mismatch middles (the shape of a link is exactly the two middles) and middles that match but for every fifth residue
    (no shared k-mer, a fill with a real path)."""
    rng = np.random.default_rng(123)
    shapes = _shapes()
    qs, ts = [], []
    for x, y in shapes:
        q, t = SC._flanked(rng, b"W" * x, b"Y" * y)
        qs.append(q); ts.append(t)
    for x, y in ((64, 62), (65, 63), (70, 63), (63, 70), (62, 65), (63, 63), (70, 1), (1, 70)):
        n = max(x, y)
        base = bytearray(SC._seq(rng, n, np.frombuffer(b"WY", np.uint8)))
        other = bytearray(c if i % 5 and i != n - 1 else ord("W") + ord("Y") - c for i, c in enumerate(base))
        qm, tm = bytes(base[:x]), bytes(other[:y])
        if x and y and qm[-1] == tm[-1]:  # the last residues must differ as well: the flank behind extends over no match
            tm = tm[:-1] + bytes([ord("W") + ord("Y") - tm[-1]])
        q, t = SC._flanked(rng, qm, tm)
        qs.append(q); ts.append(t)
    p = _Pipe(ctx, qs, ts, EXACT)
    try:
        got = p.check("rectangles", eqx=(True, False), max_fill=MAX_FILL)
        text = SR.strings(got[0], got[1])
        for i, (x, y) in enumerate(shapes):  # the all-mismatch half: what each shape must have become
            r = _row(p, i, i)
            lo, hi = min(x, y), max(x, y)
            filled = lo >= 1 and lo <= 63 and hi <= MAX_FILL
            assert (got[12][r], got[13][r], got[14][r], got[15][r]) == (2, int(filled), int(lo >= 1 and not filled), 0), (x, y)
            if not filled:
                assert text[r] == "30M" + (f"{x}I" if x else "") + (f"{y}D" if y else "") + "30M", (x, y, text[r])
            else:  # min(x, y) mismatched pairs and one run of the difference
                assert got[11][r] == 60 + hi and got[9][r] == (1 if x != y else 0) and got[6][r] == 60 - lo - ((11 + hi - lo) if x != y else 0), (x, y, text[r])
        assert p.last[0] == 1 and p.last[1] >= 64 * MAX_FILL
        # the stage knob does not show: the same arrays in slices of one link
        whole = p.check("rectangles", eqx=(False,), max_fill=MAX_FILL)
        sliced = p.check("rectangles sliced", eqx=(False,), max_fill=MAX_FILL, max_scratch_bytes=64 * (MAX_FILL + (MAX_FILL & 1)))
        assert p.last[0] >= 3 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, sliced))
        # the default max_fill fills what 70 left open by its long side alone
        wide = p.check("rectangles max_fill 0", eqx=(False,))
        assert wide[13].sum() > got[13].sum() and wide[14].sum() < got[14].sum()
    finally:
        p.close()


# ---- 4. the fuzz ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fuzz_batch(i):
    return SC.FUZZ[i]["batch"]()


@pytest.mark.parametrize("i", range(len(SC.FUZZ)), ids=[F["name"] for F in SC.FUZZ])
def test_fuzz_whole_and_in_slices(ctx, i):
    F = SC.FUZZ[i]
    qs, ts = _fuzz_batch(i)
    p = _Pipe(ctx, qs, ts, F["align"], chain=F["chain"])
    try:
        whole = p.check(F["name"], max_fill=F["max_fill"])
        assert whole[13].sum() > 10 and p.last[0] == 1
        budget = max(64 * (F["max_fill"] + 1), p.last[1] // 4)
        sliced = p.check(F["name"] + " sliced", eqx=(True,), max_fill=F["max_fill"], max_scratch_bytes=budget)
        assert p.last[0] >= 3 and p.last[1] <= budget
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, sliced))
    finally:
        p.close()


def test_member_trimmed_to_nothing(ctx):
    """A chain of the alignments themselves never links equal ends, so the case comes from a chain of doctored columns
    (rstitch_cases.duplicate_pair): the second member loses every column, its end still stands."""
    q, t, opts = SC.duplicate_pair()
    p = _Pipe(ctx, [q], [t], opts, cull=False)
    try:
        assert [c.tolist() for c in p.al_host[1:5]] == [[0, 0], [61, 61], [0, 0], [61, 61]] and p.ch.n_chained == 1
        cols = [ctx.to_device(np.ascontiguousarray(c)) for c in SC.doctored_columns(p.al_host)]
        ch = ctx.chain_regions_device(*[b.ptr for b in cols], 1, 2, **SC.DOCTORED_CHAIN)
        assert ch.to_host()[1].tolist() == [0, 1]
        p.ch.free()
        p.ch, p.ch_host = ch, ch.to_host()
        got = p.check("trimmed to nothing", eqx=(True, False), own_chain=False)
        assert SR.strings(got[0], got[1]) == ["61M"] and (got[12][0], got[13][0], got[14][0], got[15][0]) == (2, 0, 0, 61)
        assert [int(got[i][0]) for i in (6, 7, 9, 11)] == [int(p.al_host[i][0]) for i in (5, 6, 8, 10)]  # the one alignment, once
        for b in cols:
            b.free()
    finally:
        p.close()


# ---- 5. row_score as a rank key --------------------------------------------------------------------------------------------------------
def test_row_score_ranks_the_hits(ctx):
    qs, ts = _fuzz_batch(0)
    F = SC.FUZZ[0]
    p = _Pipe(ctx, qs[:80], ts[:80], F["align"], chain=F["chain"], cull_opts=dict(min_score=20))  # some rows keep nothing: NaN, ranked last
    try:
        st = p.stitch(max_fill=F["max_fill"])
        best = st.to_host()[16]
        assert np.isnan(best).any() and not np.isnan(best).all()
        for k in (1, 2):
            top = ctx.best_hits(p.hits, k, score=st.row_score_ptr)
            rank, src_row = top.best_to_host()
            want = []
            for q in np.unique(p.qid):
                rows = np.flatnonzero(p.qid == q).tolist()
                rows.sort(key=lambda r: (np.isnan(best[r]), -best[r] if not np.isnan(best[r]) else 0.0, p.tid[r]))
                want += [(r, i) for i, r in enumerate(rows[:k])]
            assert sorted(zip(src_row.tolist(), rank.tolist())) == sorted(want)
            top.free()
        st.free()
    finally:
        p.close()


# ---- 6. the golden pair through the wire ---------------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    chain_opts = {"chain_max_overlap": 5, "chain_skew_cost": 1}
    on = dict(regions=True, gapped=True, cigar=True, cull=True, chain=True, hit_rows=True)
    base = wire.search_extract_kmers_device(*args, ctx=ctx, **on, **chain_opts)
    p = _Pipe(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], dict(band=16, gap_open=11, gap_extend=1, x_drop=30),
              chain={"max_overlap": 5, "skew_cost": 1}, k=16, scaled=5, mol="hp")
    try:
        for eqx in (False, True):
            rows = wire.search_extract_kmers_device(*args, ctx=ctx, stitch=True, eqx=eqx, **on, **chain_opts)
            want = p.ref(eqx)
            assert rows == wire.hit_chain_rows(ced9_records, bcl2_records, p.qid, p.tid, p.ch_host, stitched=want)
            assert [{k: v for k, v in r.items() if not k.startswith("aln_") and k not in ("n_filled", "n_open")} for r in rows] == base
            assert len(rows) == p.hits.count > 0 and all(r["aln_cigar"] and r["aln_length"] >= r["query_end"] - r["query_start"] for r in rows)
        p.check("golden")
    finally:
        p.close()
    for missing in ("gapped", "cigar", "chain", "hit_rows"):
        with pytest.raises(ValueError):
            wire.search_extract_kmers_device(*args, ctx=ctx, stitch=True, **dict(on, **{missing: False}))


# ---- 7. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    L = ctx._L
    rng = np.random.default_rng(5)
    pairs = [SC._flanked(rng, b"W" * x, b"Y" * y) for x, y in ((3, 2), (40, 5), (2, 9))]
    qs, ts = [q for q, _ in pairs], [t for _, t in pairs]
    p = _Pipe(ctx, qs, ts, EXACT)
    wider = [SC._flanked(rng, b"W" * x, b"Y" * y, 31) for x, y in ((3, 2), (40, 5), (2, 9))]  # as many regions, other extents
    other = _Pipe(ctx, [q for q, _ in wider], [t for _, t in wider], EXACT)
    fewer = _Pipe(ctx, qs[:2], ts[:2], EXACT)
    bufs = [ctx.to_device(a) for a in (p.q[0], p.q[1], p.t[0], p.t[1])]
    batch = (C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr), len(p.q[1]) - 1, len(p.q[0]), C.c_void_p(bufs[2].ptr), C.c_void_p(bufs[3].ptr),
             len(p.t[1]) - 1, len(p.t[0]))
    cg = p.cigars(False)
    two = C.c_uint32 * 2
    try:
        want = p.check("before")
        fewer.cigars(False); other.cigars(False)  # (made before the pool is measured)
        before = ctx.pool_stats()["bytes_in_use"]

        def call(h, ch, al, cigars, hits, opts=None, out=True, args=batch):
            o = C.c_void_p()
            st = L.ks_regions_stitch(h, ch, al, cigars, hits, *args, C.byref(opts) if opts is not None else None, C.byref(o) if out else None)
            assert not o.value
            return st
        # the options: before any device work, with ctx == NULL too
        for o in (_lib.ks_rstitch_opts(4097, 0, 0, two(0, 0)), _lib.ks_rstitch_opts(0, 2, 0, two(0, 0)), _lib.ks_rstitch_opts(0, 0, 0, two(1, 0)),
                  _lib.ks_rstitch_opts(0, 0, 0, two(0, 1))):
            for h in (ctx._h, None):
                assert call(h, p.ch._h, p.al._h, cg._h, p.hits._h, o) == _lib.KS_ERR_INVALID_ARG
        for kw in ({"max_fill": 4097}, {"max_fill": -1}, {"max_scratch_bytes": 2 ** 64}, {"max_fill": 1.5}):
            with pytest.raises(ValueError):
                p.stitch(**kw)
        # NULL arguments
        for a in ((None, p.al._h, cg._h, p.hits._h), (p.ch._h, None, cg._h, p.hits._h), (p.ch._h, p.al._h, None, p.hits._h), (p.ch._h, p.al._h, cg._h, None)):
            assert call(ctx._h, *a) == _lib.KS_ERR_INVALID_ARG
        assert call(ctx._h, p.ch._h, p.al._h, cg._h, p.hits._h, out=False) == _lib.KS_ERR_INVALID_ARG
        assert call(ctx._h, p.ch._h, p.al._h, cg._h, p.hits._h, args=(batch[0], None, *batch[2:])) == _lib.KS_ERR_INVALID_ARG
        # objects of another context
        with ks.Context(0) as ctx2:
            assert call(ctx2._h, p.ch._h, p.al._h, cg._h, p.hits._h) == _lib.KS_ERR_INVALID_ARG
        # counts that disagree
        for a in ((fewer.ch, p.al, cg, p.hits), (p.ch, fewer.al, cg, p.hits), (p.ch, p.al, fewer.cigars(False), p.hits), (p.ch, p.al, cg, fewer.hits)):
            with pytest.raises(ks.KmerseekError) as e:
                ctx.stitch_chains(*a, p.q[0], p.q[1], p.t[0], p.t[1])
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and "objects of other regions" in str(e.value)
        # M where = / X are expected, and the other way round: the first such region is named
        for cigars, eqx in ((cg, True), (p.cigars(True), False)):
            with pytest.raises(ks.KmerseekError) as e:
                ctx.stitch_chains(p.ch, p.al, cigars, p.hits, p.q[0], p.q[1], p.t[0], p.t[1], eqx=eqx)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and "region 0 " in str(e.value) and "KS_RSTITCH_EQX" in str(e.value)
        # paths of other alignments: their ops consume other extents
        assert other.al.n_regions == p.al.n_regions == 6 and other.al.n_rows == p.al.n_rows == 3
        with pytest.raises(ks.KmerseekError) as e:
            ctx.stitch_chains(p.ch, p.al, other.cigars(False), p.hits, p.q[0], p.q[1], p.t[0], p.t[1])
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "region 0 do not consume" in str(e.value)
        # chains that were not made from these alignments, through chain_regions_device on doctored columns: the two regions of
        # every row in swapped places (the second member ends before the first), and all regions in one row (a member outside
        # its row's alignments)
        al = p.al_host
        swap = np.arange(6) ^ 1
        for offs, order, words in ((al[0], swap, "chain member 1 ends before"), (np.array([0, 0, 6, 6], np.uint64), np.arange(6), "chain member 0 names a region outside")):
            cb = [ctx.to_device(np.ascontiguousarray(c)) for c in (offs, *[al[i][order] for i in (1, 2, 3, 4, 5)])]
            bad = ctx.chain_regions_device(*[b.ptr for b in cb], 3, 6)
            assert bad.n_chained >= 2
            with pytest.raises(ks.KmerseekError) as e:
                ctx.stitch_chains(bad, p.al, cg, p.hits, p.q[0], p.q[1], p.t[0], p.t[1])
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and words in str(e.value), str(e.value)
            bad.free()
            for b in cb:
                b.free()
        # other sequences: half as long (an extent outside its sequence), fewer of them (an id beyond the batch)
        with pytest.raises(ks.KmerseekError) as e:
            ctx.stitch_chains(p.ch, p.al, cg, p.hits, p.q[0], p.q[1] // 2, p.t[0], p.t[1])
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "does not lie inside" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            ctx.stitch_chains(p.ch, p.al, cg, p.hits, p.q[0], p.q[1], p.t[0], p.t[1][:2])
        assert e.value.status == _lib.KS_ERR_INVALID_ARG
        # a single filled link whose directions do not fit the budget: 40 rows of 64 bytes
        with pytest.raises(ks.KmerseekError) as e:
            p.stitch(max_scratch_bytes=64 * 39)
        assert e.value.status == _lib.KS_ERR_CAPACITY and "max_scratch_bytes" in str(e.value)
        p.stitch(max_scratch_bytes=64 * 40).free()  # the bound itself passes
        assert ctx.pool_stats()["bytes_in_use"] == before
        # the context stays usable
        SR.assert_same(p.check("after"), want, "after the refusals")
    finally:
        for b in bufs:
            b.free()
        for o in (p, other, fewer):
            o.close()
