"""GPU: ks_regions_align — every region of a hit list extended with gaps from the middle of its seed (banded affine X-drop).

Every column of every region is compared exactly (integers) with the plain-loop restatement of tests/ralign_ref.py, run on the
regions the device chained (their chaining has tests of its own); nothing is compared with the library itself and no region is
left out.  Cases: identical sequences, terminations and sequence ends around the staging chunk on either side, a dip of
exactly x_drop and one more, an equal maximum in a later row, anchors at the first and the last position, sequences and seeds
of length 1, bands 0 / 1 / 16 / 31, indels at the band's edge, tie-heavy two-letter fuzz, an asymmetric matrix, odd bytes, rows
without regions, one row with thousands of regions, the golden pair through the wire, a mismatched hit list and the capacity
bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402
import ralign_ref  # noqa: E402
import regions_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
COLUMNS = ralign_ref.COLUMNS
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
HUGE = 2 ** 20  # the largest x_drop: the walk never stops early
DEFAULTS = {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30}


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


class _Case:
    """The device objects of one (queries, targets, parameters) up to the regions; align() aligns them, ref() is the yardstick
    on the same regions."""

    def __init__(self, ctx, q, t, k, scaled, mol, max_gap=0, min_kmers=1):
        self.ctx, self.q, self.t = ctx, q, t
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
        al = self.ctx.align_regions(self.rg, self.hits, self.q[0], self.q[1], self.t[0], self.t[1], **kw)
        assert al.n_rows == self.rg.n_rows == len(self.hits_host[0]) and al.n_regions == self.rg.n_regions
        assert all(p != 0 for p in al.device_ptrs())
        out = al.to_host()
        al.free()
        return out

    def ref(self, **kw):
        return ralign_ref.align(self.regions, self.hits_host[0], self.hits_host[1], self.q[0], self.q[1], self.t[0], self.t[1],
                                **{**DEFAULTS, **kw})

    def check(self, what="", **kw):
        got, want = self.align(**kw), self.ref(**kw)
        assert len(got) == len(want) == len(COLUMNS)
        for g, w, name in zip(got, want, COLUMNS):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, kw, name, g.tolist()[:20], w.tolist()[:20])
        return want

    def rows_of(self, want):
        """per hit row (qid, tid) -> the list of its regions' values as dicts"""
        offs = want[0].tolist()
        cols = [c.tolist() for c in want[1:]]
        out = {}
        for r, (q, t) in enumerate(zip(self.hits_host[0].tolist(), self.hits_host[1].tolist())):
            out[(q, t)] = [dict(zip(COLUMNS[1:], [c[g] for c in cols])) for g in range(offs[r], offs[r + 1])]
        return out

    def close(self):
        self.rg.free()
        self.hits.free()


def _chunk():
    c = int(_lib.load().ks_debug_ralign_chunk())
    assert c == 64
    return c


# ---- 1. terminations and sequence ends around the staging chunk ---------------------------------------------------------------
# protein k=7 scaled=1.  Query 0 is W x 150 + CORE + W x 150, a target is <flank> + CORE + <flank>: the twelve residues of CORE
# give one region per row, its anchor is CORE[6]: extension rows 1 .. 5 (right) or 1 .. 6 (left) are the rest of CORE, the
# flank follows.  Under FLANK_MATRIX W over M scores +1 and W over N -1: a flank is written as a string of + and -.
CORE, CORE2 = b"ACDEFGHIKLPQ", b"YVTSRQPLKIHG"
QFLANK = 150


def flank_matrix():
    m = np.array(ralign_ref.default_matrix(), np.int8)
    m[ord("W") - 65, ord("M") - 65] = 1
    return m


def _flank(pattern):
    return bytes(ord("M") if c == "+" else ord("N") for c in pattern)


def crafted_patterns(c, core_rows):
    """name -> the flank; `core_rows`: the extension rows the rest of CORE takes before the flank begins"""
    P = {}
    for T in (c - 1, c, c + 1, 2 * c + 1):
        P[f"stop_at_row_{T}"] = "+" * (T - 3 - core_rows) + "---" + "+" * 10  # B - R = 3 first at row T when nothing is gapped
        P[f"target_ends_at_row_{T}"] = "+" * (T - core_rows)
        P[f"dip_before_row_{T}"] = "+" * (T - 6 - core_rows) + "--" + "+" * 12  # a dip of exactly 2, over before row T
    P["equal_maximum_later"] = "+" * 10 + "----" + "+-" * 30 + "++++" + "------"
    P["nothing_to_extend"] = ""
    P["never_stops"] = "+++" + "-" * 50 + "+" * 80
    return P


def crafted_batch(side):
    c = _chunk()
    core_rows = 5 if side > 0 else 6
    P = crafted_patterns(c, core_rows)
    names = list(P)
    targets = [(b"NNN" + CORE + _flank(P[n])) if side > 0 else (_flank(P[n])[::-1] + CORE + b"NNN") for n in names]
    long_flank = b"M" * 140
    queries = [b"W" * QFLANK + CORE + b"W" * QFLANK]
    for T in (c - 1, c, c + 1, 2 * c + 1):  # queries that end at extension row T, against a target that goes on
        own = b"W" * (T - core_rows)
        queries.append((CORE2 + own) if side > 0 else (own + CORE2))
    targets.append((CORE2 + long_flank) if side > 0 else (long_flank + CORE2))
    # CORE2 alone touches its start and its end: anchors next to both ends of a sequence
    queries.append(CORE2)
    return ks.pack(queries), ks.pack(targets), names


@pytest.mark.parametrize("side", [1, -1])
def test_terminations_and_ends_around_the_chunk(ctx, side):
    c = _chunk()
    q, t, names = crafted_batch(side)
    case = _Case(ctx, q, t, 7, 1, "protein")
    n_rows = len(names) + 5
    assert len(case.hits_host[0]) == n_rows and case.regions[0].tolist() == list(range(n_rows + 1))  # one region per row
    assert set(case.regions[3].tolist()) == {len(CORE)}
    m = flank_matrix()
    core_rows = 5 if side > 0 else 6
    # ungapped (band 0): the extents are what the patterns were written for
    for x_drop, ext_of in ((2, {f"stop_at_row_{T}": T - 3 for T in (c - 1, c, c + 1, 2 * c + 1)}),
                           (3, {f"stop_at_row_{T}": T + 10 for T in (c - 1, c, c + 1, 2 * c + 1)}),
                           (1, {f"dip_before_row_{T}": T - 6 for T in (c - 1, c, c + 1, 2 * c + 1)}),
                           (2, {f"dip_before_row_{T}": T + 8 for T in (c - 1, c, c + 1, 2 * c + 1)}),
                           (HUGE, {"equal_maximum_later": 10 + core_rows, "nothing_to_extend": core_rows,
                                   **{f"target_ends_at_row_{T}": T for T in (c - 1, c, c + 1, 2 * c + 1)}})):
        want = case.check("band 0", matrix=m, band=0, gap_open=0, gap_extend=0, x_drop=x_drop)
        rows = case.rows_of(want)
        for name, ext in ext_of.items():
            v = rows[(0, names.index(name))][0]
            other = 6 if side > 0 else 5  # the rest of CORE on the other side, and its three N over W beyond
            assert (v["q_length"], v["t_length"], v["gaps"]) == (ext + 1 + other, ext + 1 + other, 0), (name, x_drop, v)
            assert v["aln_length"] == v["q_length"]
        if x_drop == HUGE:
            for i, T in enumerate((c - 1, c, c + 1, 2 * c + 1)):  # the queries that end at row T
                v = rows[(1 + i, len(names))][0]
                assert (v["q_length"], v["score"]) == (len(CORE2) + T - core_rows, len(CORE2) + T - core_rows)
            v = rows[(5, len(names))][0]  # CORE2 alone: anchors 6 from its start, 5 from its end
            assert (v["q_start"], v["q_length"], v["identities"]) == (0, len(CORE2), len(CORE2))
    # gapped, every band
    for kw in ({"band": 1, "gap_open": 1, "gap_extend": 1, "x_drop": 2}, {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30},
               {"band": 31, "gap_open": 2, "gap_extend": 1, "x_drop": HUGE}, {"band": 31, "gap_open": 0, "gap_extend": 0, "x_drop": 3},
               {"band": 16, "gap_open": 255, "gap_extend": 255, "x_drop": 0}):
        case.check("gapped", matrix=m, **kw)
    case.check("defaults")
    case.close()


# ---- 2. indels at the band's edge ---------------------------------------------------------------------------------------------
def indel_batch(W, seed):
    """One query; per (side, kind, L) a target that equals it but for L residues inserted into / deleted from the flank 20
    residues away from CORE.  Flanks of 90 random residues: bridging a gap pays (it costs at most 5 + 32, 70 identities follow)."""
    rng = np.random.default_rng(seed)
    seq = lambda n: bytes(PROTEIN[rng.integers(0, 20, n)])
    left, right = seq(90), seq(90)
    cases, targets = [], []
    for side in (1, -1):
        for kind in ("ins", "del"):
            for L in sorted({1, W, W + 1}):
                if side > 0:
                    fl = right[:20] + (seq(L) + right[20:] if kind == "ins" else right[20 + L:])
                    targets.append(left + CORE + fl)
                else:
                    fl = (left[:70] + seq(L) if kind == "ins" else left[:70 - L]) + left[70:]
                    targets.append(fl + CORE + right)
                cases.append((side, kind, L))
    return ks.pack([left + CORE + right]), ks.pack(targets), cases


@pytest.mark.parametrize("W", [1, 16, 31])
def test_indels_at_the_band_edge(ctx, W):
    q, t, cases = indel_batch(W, 70 + W)
    case = _Case(ctx, q, t, 7, 1, "protein")
    assert case.hits_host[1].tolist() == list(range(len(cases)))
    want = case.check("indel", band=W, gap_open=5, gap_extend=1, x_drop=HUGE)
    rows = case.rows_of(want)
    for i, (side, kind, L) in enumerate(cases):
        assert len(rows[(0, i)]) == 2, (side, kind, L)  # the identical runs on either side of the indel: two diagonals
        for v in rows[(0, i)]:
            if L <= W:  # bridged from either seed: one gap of L residues, both sequences aligned from end to end
                assert (v["gap_opens"], v["gaps"], v["q_start"], v["q_length"], v["t_start"]) == (1, L, 0, 192, 0), (side, kind, L, v)
                assert v["t_length"] == 192 + (L if kind == "ins" else -L) and v["aln_length"] == 192 + (L if kind == "ins" else 0)
            else:       # one residue beyond the band: nothing to bridge with
                assert v["gaps"] == 0 and v["q_length"] < 192, (side, kind, L, v)
    case.check("indel, defaults")
    case.close()


# ---- 3. ties: a two-letter alphabet, gap costs 0 and 1; one row with thousands of regions, rows with none -------------------
def two_letter_batch(seed, n_q, n_t, lo, hi):
    rng = np.random.default_rng(seed)
    seq = lambda: bytes(np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, int(rng.integers(lo, hi + 1)))])
    return ks.pack([seq() for _ in range(n_q)]), ks.pack([seq() for _ in range(n_t)])


@pytest.mark.parametrize("gap_open,gap_extend", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_tie_heavy_fuzz(ctx, gap_open, gap_extend):
    """+1 / -1 over {A, C}: nearly every maximum is attained more than once, so the counts pin every tie rule."""
    q, t = two_letter_batch(11 + 2 * gap_open + gap_extend, 3, 4, 20, 70)
    case = _Case(ctx, q, t, 6, 1, "protein")
    assert 50 < case.rg.n_regions < 3000
    for band, x_drop in ((1, 1), (2, 3), (5, HUGE), (16, 4), (31, 2), (0, 2)):
        case.check("fuzz", band=band, gap_open=gap_open, gap_extend=gap_extend, x_drop=x_drop)
    case.close()


def test_thousands_of_regions_in_one_row_next_to_rows_with_none(ctx):
    """k = 1 over {A, C}: every maximal run of equal residue pairs on a diagonal is a seed, a quarter of them of length 1, and
    90 x 110 residues give thousands of them in one row.  A hit row cannot be without pairs, but min_kmers = 2 leaves the rows
    of the sequences of one residue without a region."""
    rng = np.random.default_rng(5)
    two = lambda n: bytes(np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, n)])
    q = ks.pack([two(90), b"AC" * 3 + b"A", two(1)])
    t = ks.pack([b"CACCA", two(110), b"A", b"C"])
    case = _Case(ctx, q, t, 1, 1, "protein")
    per_row = np.diff(case.regions[0].astype(np.int64))
    assert per_row.max() > 2000 and 1 in case.regions[3].tolist()  # thousands in one row; seeds of length 1
    assert 1 in np.diff(case.q[1].astype(np.int64)).tolist() and 1 in np.diff(case.t[1].astype(np.int64)).tolist()  # sequences of length 1
    first = slice(int(case.regions[0][0]), int(case.regions[0][1]))  # hit row 0: query 0 (90 residues) against target 0 (5)
    assert (case.hits_host[0][0], case.hits_host[1][0]) == (0, 0)
    q_anchor = (case.regions[1][first] + case.regions[3][first] // 2).tolist()
    t_anchor = (case.regions[2][first] + case.regions[3][first] // 2).tolist()
    assert 0 in q_anchor and 89 in q_anchor and 0 in t_anchor and 4 in t_anchor  # anchors at the first and at the last position
    case.check("k = 1", band=2, gap_open=1, gap_extend=1, x_drop=2)
    case.check("k = 1", band=5, gap_open=0, gap_extend=1, x_drop=0)
    case.close()
    case = _Case(ctx, q, t, 1, 1, "protein", min_kmers=2)
    per_row = np.diff(case.regions[0].astype(np.int64))
    assert (per_row == 0).any() and per_row.max() > 100
    case.check("rows without regions", band=3, gap_open=1, gap_extend=0, x_drop=5)
    case.close()


# ---- 4. identical sequences, an asymmetric matrix, odd bytes ---------------------------------------------------------------------
def test_identical_sequences_and_an_asymmetric_matrix(ctx):
    rng = np.random.default_rng(21)
    seqs = [bytes(PROTEIN[rng.integers(0, 20, n)]) for n in (1, 7, 64, 65, 129, 400)]
    q = ks.pack(seqs)
    case = _Case(ctx, q, q, 7, 1, "protein")
    want = case.check("identical", band=16, gap_open=11, gap_extend=1, x_drop=30)
    rows = case.rows_of(want)
    for i, s in enumerate(seqs[1:], 1):  # the whole sequence, no gap
        v = rows[(i, i)][0]
        assert (v["q_start"], v["q_length"], v["t_length"], v["score"], v["identities"], v["gaps"], v["aln_length"]) == \
            (0, len(s), len(s), len(s), len(s), 0, len(s))
    for seed in (1, 2):
        case.check("asymmetric", matrix=random_matrix(seed), band=31, gap_open=20, gap_extend=3, x_drop=200)
        case.check("asymmetric", matrix=random_matrix(seed), band=2, gap_open=0, gap_extend=0, x_drop=HUGE)
    case.close()


def test_odd_bytes(ctx):
    """Lower case, '*', X, B / Z / J / U / O and bytes >= 0x80 where the extension reads them."""
    q_left, t_left = b"ju\x85*zBx", b"QJU\x85*ZbO"
    q_right, t_right = b"Xa*bzjuo\x80\xffAcde*x", b"aA*BZJOU\x80\xfeacDE*X\x90"
    q = ks.pack([q_left + CORE + q_right])
    t = ks.pack([b"ACDEFGH", t_left + CORE + t_right])
    case = _Case(ctx, q, t, 7, 1, "protein")
    assert case.rg.n_regions == 2
    for matrix in (None, random_matrix(3), random_matrix(4)):
        for kw in ({"band": 0, "x_drop": HUGE}, {"band": 3, "gap_open": 1, "gap_extend": 1, "x_drop": HUGE}, {"band": 31, "x_drop": 3}):
            want = case.check("bytes", matrix=matrix, **kw)
            if matrix is None and kw["band"] == 0:
                # +1 / -1, both walks reach the query's ends.  left: 7 pairs, one differs (x / O).  right: 16 pairs; X / a, u / O and
                # o / U differ; 0xff over 0xfe is no identity but both are of the class "other": +1, a positive
                v = case.rows_of(want)[(0, 1)][0]
                assert (v["q_start"], v["q_length"], v["score"], v["identities"], v["positives"]) == \
                    (0, 7 + 12 + 16, (6 - 1) + 12 + (13 - 3), 6 + 12 + 12, 6 + 12 + 13)
    case.close()


# ---- 5. the golden pair through the wire ------------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    q = oracle.pack([s for _, s in ced9_records])
    t = oracle.pack([s for _, s in bcl2_records])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 16, 5, "hp")
    rg = regions_ref.chain(join[0], join[1], join[2], 16)
    plain = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True)
    assert plain == wire.region_rows(ced9_records, bcl2_records, hits[0], hits[1], rg, "hp") and "aln_score" not in plain[0]
    for kw in ({}, {"band": 31, "gap_open": 3, "gap_extend": 1, "gapped_x_drop": 50}):
        rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, **kw)
        ref_kw = {**DEFAULTS, **{("x_drop" if k == "gapped_x_drop" else k): v for k, v in kw.items()}}
        al = ralign_ref.align(rg, hits[0], hits[1], q[0], q[1], t[0], t[1], **ref_kw)
        assert rows == wire.region_rows(ced9_records, bcl2_records, hits[0], hits[1], rg, "hp", alignments=al)
        assert len(rows) == 7 and all(r["aln_length"] >= 1 and r["aln_q_start"] <= r["query_start"] + r["length"] // 2 < r["aln_q_end"] for r in rows)
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, gapped=True)


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
def test_mismatched_hit_list_and_the_context_keeps_working(ctx, ced9_records, bcl2_records):
    q = ks.pack([s for _, s in ced9_records])
    t = ks.pack([s for _, s in bcl2_records])
    case = _Case(ctx, q, t, 16, 5, "hp")
    other = _Case(ctx, q, t, 15, 5, "hp")
    assert len(case.hits_host[0]) != len(other.hits_host[0])
    before = ctx.pool_stats()["bytes_in_use"]
    with pytest.raises(ks.KmerseekError) as e:  # regions and hits of different row counts
        ctx.align_regions(case.rg, other.hits, q[0], q[1], t[0], t[1])
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit rows" in str(e.value)
    with pytest.raises(ks.KmerseekError) as e:  # the batches swapped: 25 targets, but one sequence in the batch passed as theirs
        ctx.align_regions(case.rg, case.hits, t[0], t[1], q[0], q[1])
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit row 0 " in str(e.value)
    for opts in (_lib.ks_ralign_opts(None, 32, 11, 1, 30, 0), _lib.ks_ralign_opts(None, 16, 256, 1, 30, 0),
                 _lib.ks_ralign_opts(None, 16, 11, 256, 30, 0), _lib.ks_ralign_opts(None, 16, 11, 1, 2 ** 20 + 1, 0),
                 _lib.ks_ralign_opts(None, 16, 11, 1, 30, 1)):
        for h in (ctx._h, None):  # the options are checked before anything else, with ctx == NULL too
            out = C.c_void_p()
            st = ctx._L.ks_regions_align(h, case.rg._h, case.hits._h, None, None, 0, 0, None, None, 0, 0, C.byref(opts), C.byref(out))
            assert st == _lib.KS_ERR_INVALID_ARG and not out.value
    assert ctx.pool_stats()["bytes_in_use"] == before
    case.check("the context stays usable")
    other.close()
    case.close()


def test_capacity(ctx):
    """A sequence of 2^20 residues is aligned, one of 2^20 + 1 is refused and its row named."""
    rng = np.random.default_rng(9)
    big = lambda n: bytes(PROTEIN[rng.integers(0, 20, n)])
    ok, too_long = b"WWW" + CORE + big(2 ** 20 - 15), b"MM" + CORE + big(2 ** 20 + 1 - 14)
    assert (len(ok), len(too_long)) == (2 ** 20, 2 ** 20 + 1)
    q = ks.pack([b"WWWW" + CORE + b"WWWW"])
    case = _Case(ctx, q, ks.pack([ok]), 7, 1, "protein")
    assert case.rg.n_regions >= 1
    case.check("2^20")
    case.close()
    case = _Case(ctx, q, ks.pack([ok, too_long]), 7, 1, "protein")
    assert case.hits_host[1].tolist() == [0, 1]
    with pytest.raises(ks.KmerseekError) as e:
        case.align()
    assert e.value.status == _lib.KS_ERR_CAPACITY and "hit row 1 " in str(e.value)
    case.close()
