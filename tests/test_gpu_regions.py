"""GPU: ks_match_regions — every hit row's (query start, target start) pairs chained into maximal colinear regions.

Everything is compared exactly (integers): with the numpy restatement of tests/regions_ref.py on the pairs of
tests/matchpos_join.py, or with regions written down in closed form.  Cases: the golden rows (ced9 vs BCL2-25: seven regions),
real proteins over max_gap x min_kmers, one-residue repeats (every diagonal of an m x n rectangle is a region; long enough for the
MSD sort), the gap boundary around substitutions and an insertion, forced row slices and sort variants, and the edges."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402
import regions_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
COLUMNS = regions_ref.COLUMNS
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
OPTIONS = [(0, 1), (16, 1), (0, 3), (16, 3)]  # (max_gap, min_kmers)


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


class _Case:
    """The device objects of one (queries, targets, parameters) up to the match positions; regions() chains them."""

    def __init__(self, ctx, q, t, k, scaled, mol, min_containment=0.0, best_k=None):
        self.ctx, self.k = ctx, k
        T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
        Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q, min_containment=min_containment)
        if best_k is not None:
            all_hits, hits = hits, ctx.best_hits(hits, best_k)
            all_hits.free()
        qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
        tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
        self.mp = ctx.match_positions(qp, tp, hits)
        self.hits = hits.to_host()
        self.pairs = self.mp.to_host()[:3]
        self.mp_slices = self.mp.n_slices
        for o in (qp, tp, hits, Q, T):
            o.free()

    def regions(self, max_gap=0, min_kmers=1):
        """-> (Regions.to_host(), n_slices)"""
        rg = self.ctx.match_regions(self.mp, max_gap=max_gap, min_kmers=min_kmers)
        assert rg.n_rows == self.mp.n_rows == len(self.hits[0])
        out = rg.to_host()
        assert rg.n_regions == len(out[1]) == int(out[0][-1])
        assert all(p != 0 for p in rg.device_ptrs())
        n = rg.n_slices
        rg.free()
        return out, n

    def close(self):
        self.mp.free()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def _records(name, n=None):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    return ks.pack([s.upper() for _, s in (recs if n is None else recs[:n])])


_REAL = {}


def _real_reference(k, scaled, mol):
    """BCL2, the first 60 sequences against themselves: (inputs, hits, join) of the CPU restatement, computed once per config."""
    key = (k, scaled, mol)
    if key not in _REAL:
        q = _records(BCL2_300, 60)
        hits, join, _, _ = matchpos_join.reference(q[0], q[1], q[0], q[1], k, scaled, mol)
        _REAL[key] = (q, hits, join)
    return _REAL[key]


# ---- golden ---------------------------------------------------------------------------------------------------------------
GOLDEN_REGIONS = [(59, 57, 17, 2, 17), (76, 23, 16, 1, 16), (170, 46, 17, 2, 17), (197, 255, 16, 1, 16), (241, 1084, 16, 1, 16),
                  (245, 42, 16, 1, 16), (264, 555, 16, 1, 16)]


def test_golden_seven_regions_from_the_device(ctx, ced9_records, bcl2_records):
    q = ks.pack([s for _, s in ced9_records])
    t = ks.pack([s for _, s in bcl2_records])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 16, 5, "hp")
    case = _Case(ctx, q, t, 16, 5, "hp")
    got, n_slices = case.regions()
    assert n_slices == 1 and sorted(zip(*[c.tolist() for c in got[1:]])) == GOLDEN_REGIONS
    _same(got, regions_ref.chain(join[0], join[1], join[2], 16))
    got2, _ = case.regions(min_kmers=2)
    assert sorted(zip(*[c.tolist() for c in got2[1:]])) == [(59, 57, 17, 2, 17), (170, 46, 17, 2, 17)]
    assert sorted((got2[0][1:] - got2[0][:-1]).tolist()) == [0, 0, 0, 1, 1]
    case.close()


def test_search_extract_kmers_device_with_regions(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True)
    assert len(rows) == 7
    assert [(r["query_start"], r["match_start"], r["length"], r["n_kmers"], r["covered"]) for r in rows] == GOLDEN_REGIONS
    q = oracle.pack([s for _, s in ced9_records])
    t = oracle.pack([s for _, s in bcl2_records])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 16, 5, "hp")
    assert rows == wire.region_rows(ced9_records, bcl2_records, hits[0], hits[1], regions_ref.chain(join[0], join[1], join[2], 16), "hp")
    assert len(wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, min_kmers=2)) == 2
    plain = wire.search_extract_kmers_device(*args, ctx=ctx)
    assert plain == wire.search_extract_kmers_device(*args, ctx=ctx, regions=False) == wire.search_extract_kmers(*args, ctx=ctx)
    assert len(plain) == 5


# ---- real proteins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scaled,mol,rows,pairs,regions0", [(10, 1, "protein", 78, 24996, 144), (16, 5, "dayhoff", None, None, None),
                                                               (24, 5, "hp", 84, 5046, 148)])
def test_real_proteins(ctx, k, scaled, mol, rows, pairs, regions0):
    q, hits, join = _real_reference(k, scaled, mol)
    case = _Case(ctx, q, q, k, scaled, mol)
    assert np.array_equal(case.hits[0], hits[0]) and np.array_equal(case.hits[1], hits[1])
    for g, w in zip(case.pairs, join[:3]):
        assert np.array_equal(g, w)
    for max_gap, min_kmers in OPTIONS:
        want = regions_ref.chain(join[0], join[1], join[2], k, max_gap, min_kmers)
        got, n_slices = case.regions(max_gap, min_kmers)
        assert n_slices == 1
        _same(got, want, (max_gap, min_kmers))
        if (max_gap, min_kmers) == (0, 1):
            per_row = (want[0][1:] - want[0][:-1]).astype(np.int64)
            assert per_row.max() > 1 and np.array_equal(want[3], want[5])
            if rows is not None:
                assert (len(hits[0]), int(join[0][-1]), int(want[0][-1])) == (rows, pairs, regions0)
    case.close()


# ---- one-residue repeats: every diagonal of an m x n rectangle of pairs is one region -------------------------------------
def _rectangle(m, n, k):
    """The regions of a row whose pairs are all (a, b) in [0, m) x [0, n), in the result's order (q_start, t_start)."""
    out = []
    for d in list(range(0, n)) + list(range(-1, -m, -1)):
        lo, hi = max(0, -d), min(m, n - d)
        out.append((lo, lo + d, hi - lo + k - 1, hi - lo, hi - lo + k - 1))
    return out


def test_repeats_every_diagonal_is_a_region(ctx):
    q, t = ks.pack([b"A" * 1200]), ks.pack([b"G" * 1500])
    case = _Case(ctx, q, t, 24, 1, "hp")
    assert len(case.hits[0]) == 1 and len(case.pairs[1]) == 1177 * 1477  # (long enough for the MSD sort; regions span workgroups)
    got, _ = case.regions()
    want = _rectangle(1177, 1477, 24)
    assert len(want) == 1177 + 1477 - 1 == 2653 and got[0].tolist() == [0, 2653]
    assert list(zip(*[c.tolist() for c in got[1:]])) == want
    got3, _ = case.regions(max_gap=7, min_kmers=1000)
    assert list(zip(*[c.tolist() for c in got3[1:]])) == [w for w in want if w[3] >= 1000]
    case.close()


def test_repeat_rows_next_to_ordinary_rows(ctx):
    """hp k=24 scaled=1: L x 200 meets G x 260 and S x 150 meets K x 300 (L and K themselves share no hp k-mer), between
    ordinary related sequences."""
    t_res, t_off = synth.proteome(24, stream=921)
    q_res, q_off = synth.queries(16, t_res, t_off, stream=922, frac_related=0.6)
    q = ks.pack([b"L" * 200] + matchpos_join.seqs_of(q_res, q_off) + [b"S" * 150])
    ts = matchpos_join.seqs_of(t_res, t_off)
    t = ks.pack(ts[:10] + [b"K" * 300, b"G" * 260] + ts[10:])
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 24, 1, "hp")
    case = _Case(ctx, q, t, 24, 1, "hp")
    assert np.array_equal(case.hits[0], hits[0]) and np.array_equal(case.hits[1], hits[1]) and len(hits[0]) > 4
    rows = {(a, b): r for r, (a, b) in enumerate(zip(hits[0].tolist(), hits[1].tolist()))}
    for max_gap, min_kmers in ((0, 1), (16, 3)):
        got, _ = case.regions(max_gap, min_kmers)
        _same(got, regions_ref.chain(join[0], join[1], join[2], 24, max_gap, min_kmers), (max_gap, min_kmers))
        assert regions_ref.as_tuples(got, rows[(0, 11)]) == [w for w in _rectangle(177, 237, 24) if w[3] >= min_kmers]
        assert regions_ref.as_tuples(got, rows[(len(q[1]) - 2, 10)]) == [w for w in _rectangle(127, 277, 24) if w[3] >= min_kmers]
    case.close()


# ---- the gap boundary ---------------------------------------------------------------------------------------------------------
def test_gap_boundary_substitutions_and_an_insertion(ctx):
    """protein k=10 scaled=1, a random 400-residue query (391 windows, all distinct) against three edited copies:
      one substitution at 100        windows 91..100 are lost: starts 0..90 and 101..390, a step of k + 1 = 11
      substitutions at 200 and 205   windows 191..205 are lost: starts 0..190 and 206..390, a step of k + 1 + 5 = 16
      one residue inserted at 150    starts 0..140 on diagonal 0, 150..390 on diagonal +1 (141..149 straddle the insertion)"""
    k = 10
    rng = np.random.default_rng(31)
    idx = rng.integers(0, 20, 400)
    other = PROTEIN[(idx + 1) % 20]
    query = PROTEIN[idx].copy()
    sub1 = query.copy(); sub1[100] = other[100]
    sub2 = query.copy(); sub2[[200, 205]] = other[[200, 205]]
    x = next(c for c in PROTEIN if c != query[149] and c != query[150])
    ins = np.concatenate([query[:150], [x], query[150:]]).astype(np.uint8)
    q, t = ks.pack([bytes(query)]), ks.pack([bytes(sub1), bytes(sub2), bytes(ins)])
    case = _Case(ctx, q, t, k, 1, "protein")
    assert case.hits[1].tolist() == [0, 1, 2]
    assert (case.pairs[0][1:] - case.pairs[0][:-1]).tolist() == [91 + 290, 191 + 185, 141 + 241]

    def run(n_ones):  # a run of n windows that step by one: (length, n_kmers, covered)
        return (n_ones + k - 1, n_ones, n_ones + k - 1)
    sub1_split = [(0, 0) + run(91), (101, 101) + run(290)]
    sub1_joined = [(0, 0, 400, 381, 399)]  # one residue, the substituted one, lies under no shared window
    sub2_split = [(0, 0) + run(191), (206, 206) + run(185)]
    sub2_joined = [(0, 0, 400, 376, 190 + 10 + 184 + 10)]  # steps of one, the step of 16 counts k, + k: 394 — six residues uncovered
    ins_regions = [(0, 0) + run(141), (150, 151) + run(241)]
    for max_gap, want1, want2 in ((0, sub1_split, sub2_split), (1, sub1_joined, sub2_split), (5, sub1_joined, sub2_split),
                                  (6, sub1_joined, sub2_joined), (2 ** 32 - 1, sub1_joined, sub2_joined)):
        got, _ = case.regions(max_gap)
        assert regions_ref.as_tuples(got, 0) == want1, max_gap
        assert regions_ref.as_tuples(got, 1) == want2, max_gap
        assert regions_ref.as_tuples(got, 2) == ins_regions, max_gap
    case.close()


# ---- forced slices, sort variants ---------------------------------------------------------------------------------------------
def test_forced_slices_and_sort_variants_give_the_same_result(monkeypatch):
    k, scaled, mol = 10, 1, "protein"
    q, hits, join = _real_reference(k, scaled, mol)
    want = {o: regions_ref.chain(join[0], join[1], join[2], k, *o) for o in OPTIONS}
    n_rows = len(hits[0])
    with ks.Context(0, follow_debug_env=True) as c:
        plain = _Case(c, q, q, k, scaled, mol)
        for bits in ("3", "1"):
            monkeypatch.setenv("KS_DEBUG_REGIONS_ROW_BITS", bits)
            per = (1 << int(bits)) - 1
            for o in OPTIONS if bits == "3" else OPTIONS[:1]:
                got, n = plain.regions(*o)
                assert n == (n_rows + per - 1) // per > 1
                _same(got, want[o], (bits, o))
        monkeypatch.setenv("KS_DEBUG_REGIONS_ROW_BITS", "3")  # ... with the match positions made in slices too
        monkeypatch.setenv("KS_DEBUG_MATCHPOS_ROW_BITS", "2")
        both = _Case(c, q, q, k, scaled, mol)
        assert both.mp_slices > 1
        got, n = both.regions(16, 3)
        assert n > 1
        _same(got, want[(16, 3)], "both sliced")
        both.close()
        monkeypatch.delenv("KS_DEBUG_REGIONS_ROW_BITS")
        monkeypatch.delenv("KS_DEBUG_MATCHPOS_ROW_BITS")
        for knobs in ({"KS_DEBUG_PAIRS_LSD": "1"}, {"KS_DEBUG_PAIRS_LSD": "1", "KS_DEBUG_SCAN_3PASS": "1", "KS_DEBUG_REGIONS_ROW_BITS": "4"}):
            for name, v in knobs.items():
                monkeypatch.setenv(name, v)
            got, _ = plain.regions(0, 1)
            _same(got, want[(0, 1)], knobs)
        plain.close()


def test_forced_slices_on_the_long_repeat_row(monkeypatch):
    """The MSD sort inside every slice, and regions that outnumber a workgroup in one of them."""
    t_res, t_off = synth.proteome(12, stream=923)
    q_res, q_off = synth.queries(8, t_res, t_off, stream=924, frac_related=0.8)
    q = ks.pack(matchpos_join.seqs_of(q_res, q_off)[:4] + [b"A" * 1200] + matchpos_join.seqs_of(q_res, q_off)[4:])
    t = ks.pack(matchpos_join.seqs_of(t_res, t_off) + [b"G" * 1500])
    with ks.Context(0, follow_debug_env=True) as c:
        case = _Case(c, q, t, 24, 1, "hp")
        plain, n1 = case.regions(3, 2)
        assert n1 == 1 and len(case.hits[0]) > 2
        big = [r for r, (a, b) in enumerate(zip(case.hits[0].tolist(), case.hits[1].tolist())) if (a, b) == (4, 12)]
        assert regions_ref.as_tuples(plain, big[0]) == [w for w in _rectangle(1177, 1477, 24) if w[3] >= 2]
        monkeypatch.setenv("KS_DEBUG_REGIONS_ROW_BITS", "2")
        sliced, n = case.regions(3, 2)
        assert n > 1
        _same(sliced, plain)
        case.close()


# ---- edges ------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    t = synth.proteome(50, stream=925)
    unrelated = synth.proteome(20, stream=926)
    case = _Case(ctx, unrelated, t, 10, 1, "protein")  # no hits
    got, n = case.regions()
    assert len(case.hits[0]) == 0 and got[0].tolist() == [0] and all(len(c) == 0 for c in got[1:]) and n == 0
    case.close()
    longest = max(matchpos_join.seqs_of(*t), key=len)
    case = _Case(ctx, ks.pack([longest[40:50]]), ks.pack([longest]), 10, 1, "protein")  # one row with one pair
    got, n = case.regions()
    assert n == 1 and [c.tolist() for c in got] == [[0, 1], [0], [40], [10], [1], [10]]
    got, _ = case.regions(min_kmers=2)  # ... which min_kmers = 2 drops: a row without a region
    assert got[0].tolist() == [0, 0] and all(len(c) == 0 for c in got[1:])
    case.close()


def _related_targets():
    """80 independent proteins and 40 lightly mutated copies of some of them: a query related to a copied protein hits both, so
    best_hits(k=1) has rows to drop."""
    base = synth.proteome(80, stream=927)
    copies = synth.queries(40, base[0], base[1], stream=929, frac_related=1.0, p_sub=0.03)
    return np.concatenate([base[0], copies[0]]), np.concatenate([base[1], copies[1][1:] + base[1][-1]])


def test_thresholded_and_best_hits(ctx):
    t = _related_targets()
    q = synth.queries(80, t[0], t[1], stream=928, frac_related=0.6)
    k, scaled, mol = 7, 1, "protein"
    all_hits, all_join, q_sk, t_sk = matchpos_join.reference(q[0], q[1], t[0], t[1], k, scaled, mol)
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], k, scaled, mol, 0.5)
    assert 0 < len(hits[0]) < len(all_hits[0])
    case = _Case(ctx, q, t, k, scaled, mol, min_containment=0.5)
    assert np.array_equal(case.hits[0], hits[0]) and np.array_equal(case.hits[1], hits[1])
    for o in ((0, 1), (16, 3), (2 ** 32 - 1, 1)):
        _same(case.regions(*o)[0], regions_ref.chain(join[0], join[1], join[2], k, *o), o)
    got, _ = case.regions(0, 10 ** 6)  # a min_kmers that empties every row
    assert got[0].tolist() == [0] * (len(hits[0]) + 1) and all(len(c) == 0 for c in got[1:])
    case.close()
    case = _Case(ctx, q, t, k, scaled, mol, best_k=1)  # the hits thinned to the best row of every query
    n_best = len(case.hits[0])
    assert 0 < n_best == len(set(case.hits[0].tolist())) < len(all_hits[0])
    q_tab = matchpos_join.position_table(q[0], q[1], k, scaled, mol, q_sk)
    t_tab = matchpos_join.position_table(t[0], t[1], k, scaled, mol, t_sk)
    join = matchpos_join.join(q_tab, t_tab, case.hits[0], case.hits[1], k)
    for g, w in zip(case.pairs, join[:3]):
        assert np.array_equal(g, w)
    _same(case.regions(2, 2)[0], regions_ref.chain(join[0], join[1], join[2], k, 2, 2))
    case.close()


def test_unknown_flags_are_refused_and_the_context_stays_usable(ctx):
    q, hits, join = _real_reference(24, 5, "hp")
    case = _Case(ctx, q, q, 24, 5, "hp")
    before = ctx.pool_stats()["bytes_in_use"]
    for opts in ((1, 1, 0, 0), (0, 1, 0, 9)):
        out = C.c_void_p()
        st = ctx._L.ks_match_regions(ctx._h, case.mp._h, C.byref(_lib.ks_regions_opts(*opts)), C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG and not out.value
    assert ctx.pool_stats()["bytes_in_use"] == before
    _same(case.regions(2 ** 32 - 1, 1)[0], regions_ref.chain(join[0], join[1], join[2], 24, 2 ** 32 - 1, 1))
    case.close()
    assert ctx.pool_stats()["bytes_in_use"] < before
