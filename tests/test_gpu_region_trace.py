"""GPU: ks_regions_traceback — the path of every region alignment as a CIGAR.

Every op of every region is compared exactly with the plain-loop restatement of tests/rtrace_ref.py, run on the regions the
device chained and the alignments the device made (both have tests of their own); nothing is compared with the library itself
and no region is left out.  The invariants the header lists are checked on the device's ops against the alignment's columns as
well.  tests/test_region_trace_cpu.py establishes which branches of the walk the fixed inputs (tests/rtrace_cases.py) take.
Cases: identical sequences, indels of 1 / W / W + 1 on either side, end cells around the staging chunk on either side, bands
0 / 1 / 16 / 31, anchors at the first and last position, sequences and seeds of length 1, the tie-heavy two-letter fuzz, an
asymmetric matrix, lower-case and odd bytes, = / X ops, rows without regions, one row with thousands of regions, empty input,
the golden pair through the wire, slices under a small scratch budget, and the errors."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rtrace_cases as RC  # noqa: E402
import rtrace_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
HUGE = RC.HUGE
DEFAULTS = {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30}
AL = {n: i for i, n in enumerate(ralign_ref.COLUMNS)}


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


def random_matrix(seed):
    """A seeded int8 matrix, not symmetric, that holds both limits."""
    m = np.random.default_rng(seed).integers(-128, 128, (28, 28)).astype(np.int8)
    m[3, 7], m[7, 3] = -128, 127
    assert not np.array_equal(m, m.T)
    return m


def encode(cigars):
    """per region [(len, code)] -> (op_offsets, ops) as the device lays them out"""
    offs = np.zeros(len(cigars) + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in cigars], dtype=np.uint64)
    return offs, np.array([n << 4 | c for cg in cigars for n, c in cg], np.uint32)


def check_invariants(al, offs, ops, eqx):
    """The device's ops against the device's alignment columns, region by region."""
    length, code = (ops >> 4).astype(np.int64), ops & 15
    assert set(code.tolist()) <= ({1, 2, 7, 8} if eqx else {0, 1, 2}) and (length >= 1).all()
    seg = np.repeat(np.arange(len(offs) - 1), np.diff(offs.astype(np.int64)))
    total = lambda mask: np.bincount(seg[mask], weights=length[mask], minlength=len(offs) - 1).astype(np.int64)
    count = lambda mask: np.bincount(seg[mask], minlength=len(offs) - 1)
    pair, gap = np.isin(code, (0, 7, 8)), np.isin(code, (1, 2))
    assert np.array_equal(total(pair | gap), al[AL["aln_length"]])
    assert np.array_equal(total(pair) + total(code == 1), al[AL["q_length"]])
    assert np.array_equal(total(pair) + total(code == 2), al[AL["t_length"]])
    assert np.array_equal(count(gap), al[AL["gap_opens"]]) and np.array_equal(total(gap), al[AL["gaps"]])
    if eqx:
        assert np.array_equal(total(code == 7), al[AL["identities"]])
    same = code[1:] == code[:-1]
    assert not (same & (seg[1:] == seg[:-1])).any()  # adjacent equal ops are merged


class _Case:
    """The device objects of one (queries, targets, parameters) up to the regions; check() aligns and traces them on the
    device and compares every op with the yardstick run on the same regions and alignments."""

    def __init__(self, ctx, queries, targets, k, scaled=1, mol="protein", max_gap=0, min_kmers=1):
        self.ctx, self.q, self.t = ctx, ks.pack(queries), ks.pack(targets)
        q, t = self.q, self.t
        T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
        Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
        tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
        mp = ctx.match_positions(qp, tp, hits)
        self.rg = ctx.match_regions(mp, max_gap=max_gap, min_kmers=min_kmers)
        self.hits, self.hits_host, self.regions = hits, hits.to_host(), self.rg.to_host()
        for o in (mp, qp, tp, Q, T):
            o.free()

    def align(self, **kw):
        return self.ctx.align_regions(self.rg, self.hits, self.q[0], self.q[1], self.t[0], self.t[1], **kw)

    def trace(self, al, q=None, t=None, **kw):
        q, t = q or self.q, t or self.t
        return self.ctx.trace_regions(self.rg, self.hits, q[0], q[1], t[0], t[1], al, **kw)

    def ref(self, al_host, eqx=False, **kw):
        kw = {**DEFAULTS, **kw}
        kw.pop("x_drop")
        return rtrace_ref.trace(self.regions, al_host, self.hits_host[0], self.hits_host[1], self.q[0], self.q[1], self.t[0], self.t[1],
                                eqx=eqx, **kw)

    def check(self, what="", eqx=(False,), max_scratch_bytes=0, **kw):
        """-> (the alignment columns, per region the reference's (cigar, events))"""
        al = self.align(**kw)
        al_host = al.to_host()
        want = None
        for x in eqx:
            cg = self.trace(al, eqx=x, max_scratch_bytes=max_scratch_bytes)
            assert cg.n_rows == self.rg.n_rows and cg.n_regions == self.rg.n_regions and cg.n_slices >= 1
            assert all(p != 0 for p in cg.device_ptrs()) or cg.n_ops == 0
            offs, ops = cg.to_host()
            assert offs.dtype == np.uint64 and ops.dtype == np.uint32 and len(ops) == cg.n_ops == int(offs[-1])
            want = self.ref(al_host, eqx=x, **kw)
            w_offs, w_ops = encode([c for c, _ in want])
            assert np.array_equal(offs, w_offs), (what, kw, x, offs.tolist()[:20], w_offs.tolist()[:20])
            bad = np.flatnonzero(ops != w_ops)
            assert len(bad) == 0, (what, kw, x, bad[:5].tolist(), ops[bad[:5]].tolist(), w_ops[bad[:5]].tolist())
            check_invariants(al_host, offs, ops, x)
            assert cg.strings() == [rtrace_ref.cigar_string(c) for c, _ in want]
            cg.free()
        al.free()
        return al_host, want

    def close(self):
        self.rg.free()
        self.hits.free()


def _chunk():
    c, s = int(_lib.load().ks_debug_ralign_chunk()), int(_lib.load().ks_debug_rtrace_stage())
    assert c == s == 64  # the forward rows and the walk stage alike: one set of end cells crosses both
    return c


# ---- 1. identical sequences, an asymmetric matrix -----------------------------------------------------------------------------
def test_identical_sequences_are_one_op(ctx):
    rng = np.random.default_rng(21)
    seqs = [bytes(RC.PROTEIN[rng.integers(0, 20, n)]) for n in (1, 7, 64, 65, 129, 400)]
    case = _Case(ctx, seqs, seqs, 7)
    al, want = case.check("identical", eqx=(False, True))
    offs = case.regions[0].tolist()
    rows = {(q, t): r for r, (q, t) in enumerate(zip(case.hits_host[0].tolist(), case.hits_host[1].tolist()))}
    for i, s in enumerate(seqs[1:], 1):
        g = offs[rows[(i, i)]]
        assert want[g][0] == [(len(s), rtrace_ref.EQ)]
    for seed in (1, 2):
        case.check("asymmetric", matrix=random_matrix(seed), band=31, gap_open=20, gap_extend=3, x_drop=200, eqx=(False, True))
        case.check("asymmetric", matrix=random_matrix(seed), band=2, gap_open=0, gap_extend=0, x_drop=HUGE)
    case.close()


# ---- 2. indels of 1, W and W + 1 residues, as I and as D, left and right ------------------------------------------------------
@pytest.mark.parametrize("W", RC.INDEL_BANDS)
def test_indels_at_the_band_edge(ctx, W):
    qs, ts, cases = RC.indel_batch(W, 70 + W)
    case = _Case(ctx, qs, ts, RC.INDEL_K)
    assert case.hits_host[1].tolist() == list(range(len(cases)))
    al, want = case.check("indel", band=W, eqx=(False, True), **RC.INDEL_OPTS)
    al, want = case.check("indel", band=W, **RC.INDEL_OPTS)
    offs = case.regions[0].tolist()
    for i, (side, kind, L) in enumerate(cases):
        for g in range(offs[i], offs[i + 1]):
            gaps = [(n, c) for n, c in want[g][0] if c != rtrace_ref.M]
            # the target has L residues more ("ins": D ops, the query is the read) or fewer ("del": I ops)
            assert gaps == ([(L, rtrace_ref.D if kind == "ins" else rtrace_ref.I)] if L <= W else []), (side, kind, L, want[g][0])
    case.check("indel, defaults")
    case.close()


# ---- 3. end cells around the staging chunk on either side -----------------------------------------------------------------------
def flank_matrix():
    m = np.array(ralign_ref.default_matrix(), np.int8)
    m[ord("W") - 65, ord("M") - 65] = 1
    return m


@pytest.mark.parametrize("side", [1, -1])
def test_end_cells_around_the_chunk(ctx, side):
    """The query is W x 150 + CORE + W x 150, a target CORE and a flank of M (W over M scores +1) that ends at extension row T:
    with the largest x_drop the end cell lies in row T (band 0) or near it, T = c - 1, c, c + 1, 2c + 1."""
    c = _chunk()
    core_rows = 5 if side > 0 else 6  # the rest of CORE beyond the anchor CORE[6]
    Ts = (c - 1, c, c + 1, 2 * c + 1)
    targets = [(b"NNN" + RC.CORE + b"M" * (T - core_rows)) if side > 0 else (b"M" * (T - core_rows) + RC.CORE + b"NNN") for T in Ts]
    # and flanks with an indel in them, so that gapped paths cross the chunk too
    targets += [(b"NNN" + RC.CORE + b"M" * 30 + b"N" * 2 + b"M" * (T - core_rows)) if side > 0 else
                (b"M" * (T - core_rows) + b"N" * 2 + b"M" * 30 + RC.CORE + b"NNN") for T in Ts]
    case = _Case(ctx, [b"W" * 150 + RC.CORE + b"W" * 150], targets, 7)
    assert case.regions[0].tolist() == list(range(len(targets) + 1))  # one region per row
    m = flank_matrix()
    al, _ = case.check("band 0", matrix=m, band=0, gap_open=0, gap_extend=0, x_drop=HUGE, eqx=(False, True))
    anchor = case.regions[1] + case.regions[3] // 2
    x_end = (al[AL["q_start"]] + al[AL["q_length"]] - 1 - anchor) if side > 0 else (anchor - al[AL["q_start"]])
    assert x_end.tolist()[:4] == list(Ts)
    for kw in ({"band": 1, "gap_open": 1, "gap_extend": 1, "x_drop": HUGE}, {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30},
               {"band": 31, "gap_open": 2, "gap_extend": 1, "x_drop": HUGE}, {"band": 31, "gap_open": 0, "gap_extend": 0, "x_drop": 3}):
        case.check("gapped", matrix=m, **kw)
    case.check("defaults")
    case.close()


# ---- 4. ties: a two-letter alphabet, gap costs 0 and 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("gap_open,gap_extend", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_tie_heavy_fuzz(ctx, gap_open, gap_extend):
    qs, ts = RC.fuzz_batch(gap_open, gap_extend)
    case = _Case(ctx, qs, ts, RC.FUZZ_K)
    assert 50 < case.rg.n_regions < 3000
    for kw in RC.FUZZ_OPTS:
        case.check("fuzz", gap_open=gap_open, gap_extend=gap_extend, eqx=(False, True), **kw)
    case.check("fuzz", gap_open=gap_open, gap_extend=gap_extend, band=0, x_drop=2)
    case.check("fuzz", gap_open=gap_open, gap_extend=gap_extend, band=16, x_drop=4)
    case.close()


def test_thousands_of_regions_in_one_row_next_to_rows_with_none(ctx):
    """k = 1: seeds and sequences of length 1, anchors at the first and at the last position, thousands of regions in one row;
    min_kmers = 2 leaves rows without a region."""
    qs, ts = RC.k1_batch()
    case = _Case(ctx, qs, ts, 1)
    per_row = np.diff(case.regions[0].astype(np.int64))
    assert per_row.max() > 2000 and 1 in case.regions[3].tolist()
    first = slice(int(case.regions[0][0]), int(case.regions[0][1]))
    assert (case.hits_host[0][0], case.hits_host[1][0]) == (0, 0)
    q_anchor = (case.regions[1][first] + case.regions[3][first] // 2).tolist()
    t_anchor = (case.regions[2][first] + case.regions[3][first] // 2).tolist()
    assert 0 in q_anchor and 89 in q_anchor and 0 in t_anchor and 4 in t_anchor
    for kw in RC.K1_OPTS:
        case.check("k = 1", eqx=(False, True), **kw)
    case.close()
    case = _Case(ctx, qs, ts, 1, min_kmers=2)
    per_row = np.diff(case.regions[0].astype(np.int64))
    assert (per_row == 0).any() and per_row.max() > 100
    case.check("rows without regions", band=3, gap_open=1, gap_extend=0, x_drop=5)
    case.close()


def test_empty_input(ctx):
    """Hit rows without a single region, and no hit rows at all: a valid empty result."""
    qs, ts = RC.k1_batch()
    case = _Case(ctx, qs, ts, 1, min_kmers=10 ** 6)
    assert case.rg.n_regions == 0 and case.rg.n_rows > 0
    al = case.align()
    cg = case.trace(al)
    assert (cg.n_regions, cg.n_ops, cg.n_rows) == (0, 0, case.rg.n_rows)
    offs, ops = cg.to_host()
    assert offs.tolist() == [0] and len(ops) == 0 and cg.strings() == []
    for o in (cg, al):
        o.free()
    case.close()
    case = _Case(ctx, [b"AAAAAAAAAA"], [b"CCCCCCCCCC"], 7)
    assert case.rg.n_rows == 0 and case.rg.n_regions == 0
    al = case.align()
    cg = case.trace(al, eqx=True)
    assert (cg.n_rows, cg.n_regions, cg.n_ops) == (0, 0, 0) and cg.to_host()[0].tolist() == [0]
    for o in (cg, al):
        o.free()
    case.close()


# ---- 5. lower-case and odd bytes ---------------------------------------------------------------------------------------------
def test_odd_bytes(ctx):
    """Lower case, '*', X, B / Z / J / U / O and bytes >= 0x80 where the walk reads them: = is equality of the upper-cased bytes."""
    q_left, t_left = b"ju\x85*zBx", b"QJU\x85*ZbO"
    q_right, t_right = b"Xa*bzjuo\x80\xffAcde*x", b"aA*BZJOU\x80\xfeacDE*X\x90"
    case = _Case(ctx, [q_left + RC.CORE + q_right], [b"ACDEFGH", t_left + RC.CORE + t_right], 7)
    assert case.rg.n_regions == 2
    for matrix in (None, random_matrix(3), random_matrix(4)):
        for kw in ({"band": 0, "x_drop": HUGE}, {"band": 3, "gap_open": 1, "gap_extend": 1, "x_drop": HUGE}, {"band": 31, "x_drop": 3}):
            al, want = case.check("bytes", matrix=matrix, eqx=(False, True), **kw)
            if matrix is None and kw["band"] == 0:
                # left: 7 pairs, x / O differs.  CORE.  right: 16 pairs; X / a, u / O, o / U and 0xff / 0xfe differ
                assert rtrace_ref.cigar_string(want[1][0]) == "6=1X12=1X5=2X1=1X6="
    case.close()


# ---- 6. the golden pair through the wire ------------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    pinned = json.load(open(os.path.join(GOLDEN, "rtrace_expected.json")))
    gapped = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True)
    for name, kw in (("default", {}), ("eqx", {"eqx": True}), ("band31_eqx", {"band": 31, "gap_open": 3, "gap_extend": 1, "gapped_x_drop": 50, "eqx": True})):
        rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, cigar=True, **kw)
        assert len(rows) == 7 and [r["aln_cigar"] for r in rows] == pinned[name]
        if name != "band31_eqx":
            assert [{k: v for k, v in r.items() if k != "aln_cigar"} for r in rows] == gapped  # every other column is untouched
    # ... and the pinned strings are the reference's, on the device's regions and alignments
    case = _Case(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], 16, 5, "hp")
    al, want = case.check("golden", eqx=(False, True))
    assert sorted(rtrace_ref.cigar_string(c) for c, _ in want) == sorted(pinned["eqx"])
    case.close()
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, cigar=True)


# ---- 7. the scratch budget ---------------------------------------------------------------------------------------------------
def test_slices_under_a_small_budget(ctx):
    qs, ts, cases = RC.indel_batch(16, 86)
    case = _Case(ctx, qs, ts, RC.INDEL_K)
    al = case.align(band=16, **RC.INDEL_OPTS)
    al_host = al.to_host()
    whole = case.trace(al)
    assert whole.n_slices == 1 and whole.scratch_bytes >= 64 * int((al_host[AL["q_length"]].astype(np.int64) - 1).sum())
    want = whole.to_host()
    per_region = 64 * (int(al_host[AL["q_length"]].max()) + 1)  # an upper bound of one region's directions
    for budget in (per_region, 3 * per_region, whole.scratch_bytes // 3 + per_region):
        cut = case.trace(al, max_scratch_bytes=budget)
        assert cut.n_slices >= 3 and cut.scratch_bytes <= budget, (budget, cut.n_slices, cut.scratch_bytes)
        got = cut.to_host()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        cut.free()
    # a budget below one region: refused, the first region that does not fit named
    first = int(np.flatnonzero(al_host[AL["q_length"]] > 1)[0])
    before = ctx.pool_stats()["bytes_in_use"]
    for budget in (1, 64):
        with pytest.raises(ks.KmerseekError) as e:
            case.trace(al, max_scratch_bytes=budget)
        assert e.value.status == _lib.KS_ERR_CAPACITY and f"region {first} " in str(e.value)
    assert ctx.pool_stats()["bytes_in_use"] == before
    whole.free()
    al.free()
    case.check("the context stays usable", band=16, **RC.INDEL_OPTS)
    case.close()


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_alignments_of_other_regions_or_other_sequences(ctx):
    qs, ts, _ = RC.indel_batch(16, 86)
    case = _Case(ctx, qs, ts, RC.INDEL_K)
    other = _Case(ctx, qs, ts[:5], RC.INDEL_K)
    assert other.rg.n_regions != case.rg.n_regions
    al, al_other = case.align(), other.align()
    before = ctx.pool_stats()["bytes_in_use"]
    with pytest.raises(ks.KmerseekError) as e:  # alignments of another region list: checked on the host
        case.trace(al_other)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "alignments of other regions" in str(e.value)
    # batches of the same shape that hold other sequences: every extent fits, the paths do not give the alignments back
    rng = np.random.default_rng(3)
    t_other = (RC.PROTEIN[rng.integers(0, 20, len(case.t[0]))], case.t[1])
    with pytest.raises(ks.KmerseekError) as e:
        case.trace(al, t=t_other)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "region 0 " in str(e.value)
    # shorter target sequences: extents outside them, refused before anything is indexed
    t_short = ks.pack([s[:30] for s in ts])
    with pytest.raises(ks.KmerseekError) as e:
        case.trace(al, t=t_short)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and ("region " in str(e.value) or "hit row " in str(e.value))
    for opts in (_lib.ks_rtrace_opts(2, 0, 0), _lib.ks_rtrace_opts(0, 1, 0), _lib.ks_rtrace_opts(_lib.KS_RTRACE_EQX | 4, 0, 0)):
        for h in (ctx._h, None):  # the options are checked before anything else, with ctx == NULL too
            out = C.c_void_p()
            st = ctx._L.ks_regions_traceback(h, case.rg._h, case.hits._h, None, None, 0, 0, None, None, 0, 0, al._h, C.byref(opts), C.byref(out))
            assert st == _lib.KS_ERR_INVALID_ARG and not out.value
    assert ctx.pool_stats()["bytes_in_use"] == before
    for o in (al, al_other):
        o.free()
    case.check("the context stays usable")
    other.close()
    case.close()
