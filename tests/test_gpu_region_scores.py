"""GPU: ks_regions_score — every region of a hit list scored under a substitution matrix and extended without gaps (X-drop).

Everything is compared exactly (integers) with the plain-loop restatement of tests/rscore_ref.py, run on the regions of
tests/regions_ref.py over the pairs of tests/matchpos_join.py, or on regions written down in closed form; nothing is compared
with the library itself.  Cases: the golden pair (ced9 vs BCL2-25), extensions crafted around the wave's step, odd bytes in the
flanks, one long region, a row with hundreds of regions next to rows with none, thresholded / best / empty hit lists, the
refused calls, and the wire rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402
import regions_ref  # noqa: E402
import rscore_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
COLUMNS = rscore_ref.COLUMNS
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
HUGE = 2 ** 32 - 1


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
    """The device objects of one (queries, targets, parameters) up to the regions; score() scores them."""

    def __init__(self, ctx, q, t, k, scaled, mol, max_gap=0, min_kmers=1, min_containment=0.0, best_k=None):
        self.ctx, self.q, self.t = ctx, q, t
        T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
        Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q, min_containment=min_containment)
        if best_k is not None:
            all_hits, hits = hits, ctx.best_hits(hits, best_k)
            all_hits.free()
        qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
        tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
        mp = ctx.match_positions(qp, tp, hits)
        self.rg = ctx.match_regions(mp, max_gap=max_gap, min_kmers=min_kmers)
        self.hits, self.hits_host, self.regions = hits, hits.to_host(), self.rg.to_host()
        for o in (mp, qp, tp, Q, T):
            o.free()

    def score(self, **kw):
        sc = self.ctx.score_regions(self.rg, self.hits, self.q[0], self.q[1], self.t[0], self.t[1], **kw)
        assert sc.n_rows == self.rg.n_rows == len(self.hits_host[0]) and sc.n_regions == self.rg.n_regions
        assert all(p != 0 for p in sc.device_ptrs())
        out = sc.to_host()
        sc.free()
        return out

    def ref(self, regions, **kw):
        return rscore_ref.score(regions, self.hits_host[0], self.hits_host[1], self.q[0], self.q[1], self.t[0], self.t[1], **kw)

    def close(self):
        self.rg.free()
        self.hits.free()


def _same(got, want, what=""):
    assert len(got) == len(want) == len(COLUMNS)
    for g, w, name in zip(got, want, COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def _same_regions(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _exts(regions, scores):
    """(left_ext, right_ext) of every region"""
    left = regions[1].astype(np.int64) - scores[1].astype(np.int64)
    return left.tolist(), (scores[3].astype(np.int64) - regions[3].astype(np.int64) - left).tolist()


def _records(name, n=None):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    return ks.pack([s.upper() for _, s in (recs if n is None else recs[:n])])


# ---- 1. golden ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scaled,mol,n_regions", [(15, 5, "hp", 17), (16, 5, "hp", 7), (24, 5, "hp", 0), (5, 1, "protein", 3)])
def test_golden(ctx, ced9_records, bcl2_records, k, scaled, mol, n_regions):
    q = ks.pack([s for _, s in ced9_records])
    t = ks.pack([s for _, s in bcl2_records])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], k, scaled, mol)
    for max_gap in (0, 16):
        want_rg = regions_ref.chain(join[0], join[1], join[2], k, max_gap)
        case = _Case(ctx, q, t, k, scaled, mol, max_gap=max_gap)
        assert np.array_equal(case.hits_host[0], hits[0]) and np.array_equal(case.hits_host[1], hits[1])
        _same_regions(case.regions, want_rg)
        if max_gap == 0:
            assert len(want_rg[1]) == n_regions
        for matrix in (None, random_matrix(k)):
            for kw in ({}, {"extend": True, "x_drop": 0}, {"extend": True, "x_drop": 7}, {"extend": True, "x_drop": 300}):
                got = case.score(matrix=matrix, **kw)
                _same(got, case.ref(want_rg, matrix=matrix, **kw), (max_gap, matrix is None, kw))
                if not kw:  # without the flag the placement is the seed's
                    _same_regions(got[:4], want_rg[:4])
                if mol == "protein" and max_gap == 0:  # the seeds are identical residues: every core position is an identity
                    assert len(got[7]) > 0 and np.array_equal(got[7], want_rg[3])
        case.close()


# ---- 2. crafted extension lengths -----------------------------------------------------------------------------------------
# protein k=7 scaled=1.  Query 0 is W x 200 + CORE + W x 200, a target is <flank> + CORE + <flank>: the twelve residues of CORE
# give six shared windows on one diagonal — one region per row — and the flanks share no window (the target's are spelled in M
# and N).  Under FLANK_MATRIX W over M scores +1 and W over N -1: a flank is written as a string of + and -, pair 1 first.
CORE, CORE2 = b"ACDEFGHIKLPQ", b"YVTSRQPLKIHG"
QFLANK = 200


def flank_matrix():
    m = np.array(rscore_ref.default_matrix(), np.int8)
    m[ord("W") - 65, ord("M") - 65] = 1
    return m


def _flank(pattern):
    return bytes(ord("M") if c == "+" else ord("N") for c in pattern)


def crafted_patterns(step):
    """name -> (pattern, {x_drop: the extension it must give})"""
    P = {}
    for T in (step - 1, step, step + 1, 2 * step + 1):  # B - S = 3 first at pair T
        P[f"stop_at_{T}"] = ("+" * (T - 3) + "---" + "+" * 10, {2: T - 3, 3: T + 10, 0: T - 3})  # (x_drop 3: the walk goes on to the end and the whole flank is the best prefix)
    P["query_end_first"] = ("+" * (QFLANK + 60), {0: QFLANK, HUGE: QFLANK})
    P["target_end_first"] = ("+" * (step + 6), {0: step + 6, HUGE: step + 6})
    P["nothing_to_extend"] = ("", {0: 0, HUGE: 0})
    # the best sum 10 at pair 10 (step 1) and again, equal, at pair 78 (step 2); then the walk is stopped
    P["equal_maximum_in_the_next_step"] = ("+" * 10 + "----" + "+-" * 30 + "++++" + "------", {5: 10, 4: 10, HUGE: 10})
    P["dip"] = ("+++++" + "--" + "+++++", {2: 12, 1: 5, 0: 5})
    P["dip_across_steps"] = ("+" * (step - 2) + "-----" + "+" * 9, {3: step - 2, 5: step + 12, 4: step - 2})
    P["never_stops"] = ("+++" + "-" * 50 + "+" * 100, {HUGE: 153, 49: 3, 50: 153})
    return P


def crafted_batch(step, side):
    """-> (q, t, names, regions in closed form): the patterns on the right (side = 1) or, mirrored, on the left of the core."""
    P = crafted_patterns(step)
    names = list(P)
    targets = [(b"NNN" + CORE + _flank(P[n][0])) if side > 0 else (_flank(P[n][0])[::-1] + CORE + b"NNN") for n in names]
    # query 1 is CORE2 alone — it touches its start and its end — against a target with flanks and a target that is CORE2 too
    targets += [b"MMM" + CORE2 + b"MMM", CORE2]
    q = ks.pack([b"W" * QFLANK + CORE + b"W" * QFLANK, CORE2])
    t = ks.pack(targets)
    b_start = [3 if side > 0 else len(P[n][0]) for n in names]
    n_rows = len(names) + 2
    regions = (np.arange(n_rows + 1, dtype=np.uint64), np.array([QFLANK] * len(names) + [0, 0], np.uint32),
               np.array(b_start + [3, 0], np.uint32), np.full(n_rows, len(CORE), np.uint32))
    return q, t, names, regions


@pytest.mark.parametrize("side", [1, -1])
def test_crafted_extension_lengths(ctx, side):
    step = int(_lib.load().ks_debug_rscore_step())
    assert step == 64
    q, t, names, regions = crafted_batch(step, side)
    P = crafted_patterns(step)
    case = _Case(ctx, q, t, 7, 1, "protein")
    assert case.hits_host[0].tolist() == [0] * len(names) + [1, 1] and case.hits_host[1].tolist() == list(range(len(names) + 2))
    _same_regions(case.regions[:4], regions)
    m = flank_matrix()
    for x_drop in sorted({x for _, want in P.values() for x in want}):
        want = case.ref(regions, matrix=m, extend=True, x_drop=x_drop)
        left, right = _exts(regions, want)
        for i, n in enumerate(names):  # the yardstick gives what the pattern was written for ...
            if x_drop in P[n][1]:
                assert (right if side > 0 else left)[i] == P[n][1][x_drop], (n, x_drop)
        assert (left[-2:], right[-2:]) == ([0, 0], [0, 0])  # (query 1 touches both of its ends)
        _same(case.score(matrix=m, extend=True, x_drop=x_drop), want, (side, x_drop))  # ... and the device gives the same
    _same(case.score(matrix=m), case.ref(regions, matrix=m), "no extension")
    case.close()


# ---- 3. bytes ---------------------------------------------------------------------------------------------------------------
def test_odd_bytes_in_the_flanks(ctx):
    """Lower case, '*', X, B / Z / J / U / O and bytes >= 0x80 where the extension reads them; the pair next to the core differs
    on either side and no seven pairs in a row are equal, so the core stays the one region."""
    q_left, t_left = b"ju\x85*zBx", b"QJU\x85*ZbO"
    q_right, t_right = b"Xa*bzjuo\x80\xffAcde*x", b"aA*BZJOU\x80\xfeacDE*X\x90"
    q = ks.pack([q_left + CORE + q_right])
    t = ks.pack([b"ACDEFGH", t_left + CORE + t_right])
    case = _Case(ctx, q, t, 7, 1, "protein")
    regions = (np.array([0, 1, 2], np.uint64), np.array([len(q_left)] * 2, np.uint32), np.array([0, len(t_left)], np.uint32),
               np.array([7, len(CORE)], np.uint32))
    assert case.hits_host[1].tolist() == [0, 1]
    _same_regions(case.regions[:4], regions)
    for matrix in (None, random_matrix(3), random_matrix(4)):
        for x_drop in (0, 3, HUGE):
            want = case.ref(regions, matrix=matrix, extend=True, x_drop=x_drop)
            _same(case.score(matrix=matrix, extend=True, x_drop=x_drop), want, (matrix is None, x_drop))
            if matrix is None and x_drop == HUGE:
                # +1 / -1, both walks reach the query's end.  left: 7 pairs, one differs (x / O).  right: 16 pairs; X / a, u / O and
                # o / U differ; 0xff over 0xfe is no identity but both are of the class "other": +1, a positive
                assert [c.tolist()[1] for c in want[1:]] == [0, 1, 7 + 12 + 16, (6 - 1) + 12 + (13 - 3), 6 + 12 + 12, 6 + 12 + 13, 12]
    case.close()


# ---- 4. one long region -----------------------------------------------------------------------------------------------------
def test_long_region(ctx):
    rng = np.random.default_rng(41)
    seq = lambda n: bytes(PROTEIN[rng.integers(0, 20, n)])
    shared = seq(5003)
    q, t = ks.pack([seq(37) + shared + seq(91)]), ks.pack([seq(50) + shared + seq(64)])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 7, 1, "protein")
    want_rg = regions_ref.chain(join[0], join[1], join[2], 7)
    assert (37, 50, 5003) in list(zip(*[c.tolist() for c in want_rg[1:4]]))
    case = _Case(ctx, q, t, 7, 1, "protein")
    _same_regions(case.regions, want_rg)
    for matrix in (None, random_matrix(5)):
        _same(case.score(matrix=matrix), case.ref(want_rg, matrix=matrix), "core")
        _same(case.score(matrix=matrix, extend=True, x_drop=20), case.ref(want_rg, matrix=matrix, extend=True, x_drop=20), "extended")
    case.close()


# ---- 5. many regions in one row, rows with none -------------------------------------------------------------------------------
def many_regions_batch():
    t_res, t_off = synth.proteome(12, stream=931)
    q_res, q_off = synth.queries(8, t_res, t_off, stream=932, frac_related=0.8)
    qs, ts = matchpos_join.seqs_of(q_res, q_off), matchpos_join.seqs_of(t_res, t_off)
    return ks.pack(qs[:4] + [b"A" * 400] + qs[4:]), ks.pack(ts[:5] + [b"G" * 500] + ts[5:])


def test_many_regions_in_one_row_next_to_rows_with_none(ctx):
    """hp k=24 scaled=1: A x 400 meets G x 500 — every diagonal of the 377 x 477 rectangle of pairs is a region — between ordinary
    related sequences whose regions min_kmers = 200 drops."""
    q, t = many_regions_batch()
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 24, 1, "hp")
    want_rg = regions_ref.chain(join[0], join[1], join[2], 24, 0, 200)
    per_row = (want_rg[0][1:] - want_rg[0][:-1]).astype(np.int64)
    assert len(per_row) > 4 and per_row.max() == 377 + 477 - 1 - 2 * 199 and sorted(per_row.tolist())[-2] == 0
    case = _Case(ctx, q, t, 24, 1, "hp", min_kmers=200)
    _same_regions(case.regions, want_rg)
    m = np.array(rscore_ref.default_matrix(), np.int8)
    m[0, 6] = 2  # A over G: the extensions run along the whole diagonal
    for matrix, kw in ((None, {}), (None, {"extend": True, "x_drop": 3}), (m, {"extend": True, "x_drop": 3})):
        _same(case.score(matrix=matrix, **kw), case.ref(want_rg, matrix=matrix, **kw), kw)
    case.close()


# ---- 6. other hit lists -----------------------------------------------------------------------------------------------------
def test_thresholded_best_and_empty_hit_lists(ctx):
    k, scaled, mol = 10, 1, "protein"
    q = _records(BCL2_300, 40)
    all_hits, _, q_sk, t_sk = matchpos_join.reference(q[0], q[1], q[0], q[1], k, scaled, mol)
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], q[0], q[1], k, scaled, mol, 0.2)
    assert 0 < len(hits[0]) < len(all_hits[0])
    want_rg = regions_ref.chain(join[0], join[1], join[2], k)
    case = _Case(ctx, q, q, k, scaled, mol, min_containment=0.2)
    assert np.array_equal(case.hits_host[0], hits[0]) and np.array_equal(case.hits_host[1], hits[1])
    _same_regions(case.regions, want_rg)
    got = case.score(extend=True, x_drop=10)
    _same(got, case.ref(want_rg, extend=True, x_drop=10), "thresholded")
    assert len(got[7]) > 40 and np.array_equal(got[7], want_rg[3])  # protein, max_gap = 0: the seeds are identities throughout
    assert np.all(got[5] >= got[7]) and np.all(got[3] >= want_rg[3])
    case.close()
    case = _Case(ctx, q, q, k, scaled, mol, max_gap=16, best_k=1)  # the best row of every query
    assert 0 < len(case.hits_host[0]) < len(all_hits[0])
    tab = matchpos_join.position_table(q[0], q[1], k, scaled, mol, q_sk)
    join = matchpos_join.join(tab, tab, case.hits_host[0], case.hits_host[1], k)
    want_rg = regions_ref.chain(join[0], join[1], join[2], k, 16)
    _same_regions(case.regions, want_rg)
    m = random_matrix(6)
    _same(case.score(matrix=m, extend=True, x_drop=40), case.ref(want_rg, matrix=m, extend=True, x_drop=40), "best hits")
    case.close()
    case = _Case(ctx, synth.proteome(20, stream=926), synth.proteome(50, stream=925), k, scaled, mol)  # no hits
    got = case.score(extend=True, x_drop=5)
    assert len(case.hits_host[0]) == 0 and got[0].tolist() == [0] and all(len(c) == 0 for c in got[1:])
    assert [c.dtype for c in got] == [c.dtype for c in rscore_ref.score(case.regions, [], [], *case.q, *case.t)]
    case.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------
def test_refused_calls(ctx, ced9_records, bcl2_records):
    q = ks.pack([s for _, s in ced9_records])
    t = ks.pack([s for _, s in bcl2_records])
    case = _Case(ctx, q, t, 16, 5, "hp")
    other = _Case(ctx, q, t, 15, 5, "hp")
    assert len(case.hits_host[0]) != len(other.hits_host[0])
    L = ctx._L
    bufs = [ctx.to_device(a) for a in (q[0], q[1], t[0], t[1])]
    batches = (C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr), len(q[1]) - 1, len(q[0]),
               C.c_void_p(bufs[2].ptr), C.c_void_p(bufs[3].ptr), len(t[1]) - 1, len(t[0]))
    before = ctx.pool_stats()["bytes_in_use"]
    for opts in (_lib.ks_rscore_opts(2, 0, None, 0), _lib.ks_rscore_opts(0x80000001, 0, None, 0), _lib.ks_rscore_opts(1, 0, None, 1)):
        for h in (ctx._h, None):  # the options are checked before anything else, with ctx == NULL too
            out = C.c_void_p()
            st = L.ks_regions_score(h, case.rg._h, case.hits._h, *batches, C.byref(opts), C.byref(out))
            assert st == _lib.KS_ERR_INVALID_ARG and not out.value
    assert "options" in L.ks_last_error(ctx._h).decode()
    with pytest.raises(ks.KmerseekError) as e:  # regions and hits of different row counts
        ctx.score_regions(case.rg, other.hits, q[0], q[1], t[0], t[1])
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit rows" in str(e.value)
    with pytest.raises(ks.KmerseekError) as e:  # the batches swapped: 25 targets, but one sequence in the batch passed as theirs
        ctx.score_regions(case.rg, case.hits, t[0], t[1], q[0], q[1], extend=True)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "hit row 0 " in str(e.value)
    with pytest.raises(ValueError):
        ctx.score_regions(case.rg, case.hits, q[0], q[1], t[0], t[1], matrix=np.zeros((20, 20), np.int8))
    assert ctx.pool_stats()["bytes_in_use"] == before
    _same(case.score(extend=True, x_drop=4), case.ref(case.regions, extend=True, x_drop=4), "the context stays usable")
    for b in bufs:
        b.free()
    other.close()
    case.close()


# ---- 8. wire ----------------------------------------------------------------------------------------------------------------
def test_search_extract_kmers_device_with_scores(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    q = oracle.pack([s for _, s in ced9_records])
    t = oracle.pack([s for _, s in bcl2_records])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 16, 5, "hp")
    rg = regions_ref.chain(join[0], join[1], join[2], 16)
    m = random_matrix(8)
    for kw in ({"extend": True, "x_drop": 6}, {"extend": True, "x_drop": 6, "matrix": m}, {}):
        rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, score=True, **kw)
        ref_kw = {"extend": kw.get("extend", False), "x_drop": kw.get("x_drop", 0), "matrix": kw.get("matrix")}
        sc = rscore_ref.score(rg, hits[0], hits[1], q[0], q[1], t[0], t[1], **ref_kw)
        assert rows == wire.region_rows(ced9_records, bcl2_records, hits[0], hits[1], rg, "hp", scores=sc)
        assert len(rows) == 7 and all(r["seed_length"] in (16, 17) and r["length"] >= r["seed_length"] for r in rows)
    with pytest.raises(ValueError):
        wire.search_extract_kmers_device(*args, ctx=ctx, score=True)
    plain = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True)
    assert "score" not in plain[0] and len(plain) == 7
