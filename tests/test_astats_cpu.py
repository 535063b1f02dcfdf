"""CPU: the alignment statistics without a GPU.  The reference (tests/astats_ref.py) is held against first principles — the
root of every regular row of the cases is bracketed by an exact rational sign change, the Karlin-Altschul series reproduces the
closed forms of +1 / -1 scoring and does not see a scaling of the matrix — then the library's host function against the
reference, its error cases, the option checks that need no context, and the wire's column functions on hand-made statistics."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import astats_cases as AC  # noqa: E402
import astats_ref as R  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, build as ks_build, wire  # noqa: E402

BRACKET = Fraction(1, 10 ** 12)


@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def freq_on(n_letters: int) -> np.ndarray:
    """Uniform weights on the first n standard letters: a match probability of 1 / n under +1 / -1."""
    f = np.zeros(R.A)
    f[R.STD[:n_letters]] = 1.0
    return f


def exact_f(c, x: Fraction) -> Fraction:
    return sum(Fraction(v) * x ** k for k, v in enumerate(c))


def assert_bracketed(c, x: float):
    xf = Fraction(x)
    below, above = exact_f(c, xf * (1 - BRACKET)), exact_f(c, xf * (1 + BRACKET))
    assert below > 0 > above, (x, float(below), float(above))


# ---- the root -----------------------------------------------------------------------------------------------------------------------
def test_class_table_and_composition():
    assert [R.residue_class(b) for b in b"AaZz*@[ "] == [0, 0, 25, 25, 26, 27, 27, 27]
    assert sorted(R.STD) == R.STD and len(set(R.STD)) == 20 and max(R.STD) == 24
    res, offs = AC.pack([np.frombuffer(b"ACca*x", np.uint8), np.zeros(0, np.uint8)])
    counts, totals, length = R.composition(res, offs)
    assert counts[0, 0] == 2 and counts[0, 2] == 2 and counts[0, 26] == 1 and counts[0, 23] == 1 and counts[1].sum() == 0
    assert totals.sum() == 6 and length.tolist() == [6, 0]


@pytest.mark.parametrize("name", sorted(AC.MATRICES))
def test_every_regular_root_is_bracketed_exactly(name):
    """f changes sign between x (1 - 1e-12) and x (1 + 1e-12) in exact rational arithmetic, for every random row: none of them
    is a fallback row (a uniform-letter 30-mer under these matrices has an expected score far below 0)."""
    q_res, q_off, t_res, t_off, qid, tid = AC.random_batches()
    cq, ct = R.composition(q_res, q_off)[0], R.composition(t_res, t_off)[0]
    status, x = AC.rows_reference(name)
    assert len(x) == 200 and not status.any()
    smin, smax = R.score_range(AC.MATRICES[name])
    for r in range(len(x)):
        assert 0.0 < x[r] < 1.0
        assert_bracketed(R.coefficients(R.pair_histogram(AC.MATRICES[name], cq[qid[r]], ct[tid[r]]), smin, smax), float(x[r]))


def test_wide_row_degree_255():
    cq, ct = AC.wide_counts()
    m = AC.matrix_wide()
    smin, smax = R.score_range(m)
    assert (smin, smax) == (-128, 127)
    h = R.pair_histogram(m, cq, ct)
    assert sum(h.values()) == 2 ** 40 and R.is_regular(h)
    c = R.coefficients(h, smin, smax)
    assert len(c) == 256 and all(abs(v) <= 2 ** 40 for v in c)
    assert_bracketed(c, R.bisect_root(c))


def test_fallback_rows_of_the_cases():
    q_res, q_off, t_res, t_off, qid, tid = AC.fallback_batches()
    cq, ct = R.composition(q_res, q_off)[0], R.composition(t_res, t_off)[0]
    for name, m in AC.MATRICES.items():
        smin, smax = R.score_range(m)
        for q, t in zip(qid, tid):
            assert R.row_root(m, cq[q], ct[t], smin, smax) == (R.ROW_FALLBACK, 0.0), (name, q)
    h = R.pair_histogram(None, cq[3], ct[3])
    assert sum(s * v for s, v in h.items()) == 0 and sum(h.values()) == 2400


# ---- lambda, K, H -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_letters, terms", [(20, 43), (10, 69), (5, 153)])
def test_series_reproduces_the_closed_forms(n_letters, terms):
    p = 1.0 / n_letters
    q = 1.0 - p
    f = freq_on(n_letters)
    lam, K, H, n_terms = R.karlin_ungapped(None, f, f)
    assert abs(lam / math.log(q / p) - 1.0) <= 1e-14
    assert abs(K / ((q - p) ** 2 / q) - 1.0) <= 1e-12
    assert n_terms == terms < 400
    assert abs(H / (lam * (q - p)) - 1.0) <= 1e-13  # sum s P(s) e^(lambda s) = q - p at the root


@pytest.mark.parametrize("base", ["p5m4", "strong"])
def test_scaling_the_matrix_leaves_K(base):
    """K does not see a common factor of the scores (the gcd is divided out), lambda is divided by it."""
    m = AC.MATRICES["p5m4"] if base == "p5m4" else AC.matrix_random(seed=3, lo=-9, hi=-2)
    f = np.random.default_rng(2).random(R.A) + 0.2
    lam, K, H, _ = R.karlin_ungapped(m, f, f)
    for c in (2, 3):
        lc, Kc, Hc, _ = R.karlin_ungapped((m.astype(np.int64) * c).astype(np.int8), f, f)
        assert abs(Kc / K - 1.0) <= 1e-9 and abs(lc * c / lam - 1.0) <= 1e-12 and abs(Hc / H - 1.0) <= 1e-12


def test_library_agrees_with_the_reference(lib):
    rng = np.random.default_rng(4)
    cases = [(None, freq_on(20), freq_on(20)), (None, freq_on(5), freq_on(10)), (AC.MATRICES["p5m4"], rng.random(R.A), rng.random(R.A)),
             (AC.matrix_random(seed=3, lo=-9, hi=-2), rng.random(R.A) + 0.1, rng.random(R.A) + 0.1),
             ((AC.matrix_random(seed=3, lo=-9, hi=-2).astype(np.int64) * 3).astype(np.int8), rng.random(R.A), rng.random(R.A))]
    for m, fq, ft in cases:
        lam, K, H = ks.karlin_ungapped(m, fq, ft)
        rl, rK, rH, _ = R.karlin_ungapped(m, fq, ft)
        assert abs(lam / rl - 1.0) <= 1e-12 and abs(H / rH - 1.0) <= 1e-12 and abs(K / rK - 1.0) <= 1e-9
    # weights outside the standard classes do not count
    f = freq_on(20)
    g = f.copy(); g[[1, 9, 26, 27]] = 50.0
    assert ks.karlin_ungapped(None, f, f) == ks.karlin_ungapped(None, g, g)


def test_library_refuses(lib):
    f = freq_on(20)

    def refused(m, fq, ft, word):
        with pytest.raises(ks.KmerseekError) as e:
            ks.karlin_ungapped(m, fq, ft)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and word in str(e.value), str(e.value)
    refused(AC.matrix_pm(-1, -2), f, f, "no positive score")
    refused(AC.matrix_pm(1, -1), freq_on(1), freq_on(1), "not negative")            # every pair matches
    refused(AC.matrix_pm(5, 1), f, f, "not negative")
    refused(AC.MATRICES["random"], f, f, "expected score too close to zero")       # -0.6 a pair: the 400 terms do not suffice
    with pytest.raises(ValueError):
        R.karlin_ungapped(AC.MATRICES["random"], f, f)
    bad = f.copy(); bad[0] = -1.0
    refused(None, bad, f, "weights")
    refused(None, np.zeros(R.A), f, "weights")
    nan = f.copy(); nan[27] = math.nan
    refused(None, f, nan, "weights")
    dp = C.POINTER(C.c_double)
    assert lib.ks_karlin_ungapped(None, None, f.ctypes.data_as(dp), None, None, None) == _lib.KS_ERR_INVALID_ARG
    # lambda alone needs no series: the matrix the series gives up on still has one
    lam = C.c_double(0)
    assert lib.ks_karlin_ungapped(AC.MATRICES["random"].ctypes.data_as(C.POINTER(C.c_int8)), f.ctypes.data_as(dp), f.ctypes.data_as(dp),
                                  C.byref(lam), None, None) == _lib.KS_OK
    assert abs(sum(v * math.exp(lam.value * s) for s, v in R.score_probs(AC.MATRICES["random"], f, f).items()) - 1.0) < 1e-13


# ---- the option checks that need no context ------------------------------------------------------------------------------------------
def test_options_refused_without_a_context(lib):
    assert C.sizeof(_lib.ks_astats_opts) == 80

    def opts(**kw):
        o = _lib.ks_astats_opts(0, 0, None, 0.0, 0.0, None, 0.0, 0.0, 0, 0, 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    out = C.c_void_p()

    def call(o):
        return lib.ks_scores_stats_device(None, None, None, 0, 0, None, None, None, C.byref(o), C.byref(out))
    bad = [opts(flags=8), opts(reserved=1), opts(lambda_=0.3), opts(K=0.1), opts(lambda_=-0.3, K=0.1), opts(lambda_=math.nan, K=0.1),
           opts(lambda_=0.3, K=math.nan), opts(ratio_min=-0.5, ratio_max=1.0), opts(ratio_min=math.nan, ratio_max=1.0),
           opts(ratio_min=0.9, ratio_max=0.5)]
    for o in bad:
        assert call(o) == _lib.KS_ERR_INVALID_ARG
    for fn, n_obj in ((lib.ks_rscores_stats, 1), (lib.ks_raligns_stats, 1), (lib.ks_hitalns_stats, 2)):
        for o in bad + [opts()]:
            assert fn(None, *([None] * n_obj), None, None, None, C.byref(o), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert call(opts(lambda_=0.267, K=0.041, ratio_min=0.5, ratio_max=1.0)) == _lib.KS_ERR_INVALID_ARG  # (valid options: no context)
    assert lib.ks_residue_composition_device(None, None, None, 0, 0, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    for name in ("ks_astats_n_rows", "ks_astats_n_entries", "ks_astats_n_fallback", "ks_astats_params_source", "ks_rcomp_n_seqs"):
        assert getattr(lib, name)(None) == 0
    assert lib.ks_astats_device_x(None) is None and lib.ks_rcomp_device_counts(None) is None
    wave_max, group_max = C.c_uint32(0), C.c_uint32(0)
    lib.ks_debug_rcomp_limits(C.byref(wave_max), C.byref(group_max))
    assert 64 < wave_max.value < group_max.value <= 2 ** 20


def test_engine_refuses_before_the_library():
    with pytest.raises(ValueError):
        ks.Context._astats_opts(np.zeros((20, 20), np.int8), None, None, True, False, False, (0.5, 1.0), 0, 0, 0)
    with pytest.raises(ValueError):
        ks.Context._astats_opts(None, None, np.zeros(20), True, False, False, (0.5, 1.0), 0, 0, 0)
    with pytest.raises(ValueError):
        ks.Context._astats_opts(None, None, None, True, False, False, (0.5, 1.0), -1, 0, 0)
    o, _ = ks.Context._astats_opts(None, (0.267, 0.041), None, False, True, True, (0.25, 2.0), 7, 3, 11)
    assert (o.flags, o.length_adjust, o.lambda_, o.K, o.ratio_min, o.ratio_max, o.db_residues, o.db_seqs) == (7, 11, 0.267, 0.041, 0.25, 2.0, 7, 3)


# ---- the wire's columns ---------------------------------------------------------------------------------------------------------------
Q_RECS = [("q0", b"ACDEFGHIKLMNPQRSTVWY"), ("q1", b"MKVLAAGIVGLCAK")]
T_RECS = [("t0", b"ACDEFGHIKLMNPQRSTVWYAC"), ("t1", b"MKVLAAGIVGLCAKHH")]


def _hand_made():
    qid, tid = np.array([0, 1], np.uint32), np.array([0, 1], np.uint32)
    offs = np.array([0, 2, 3], np.uint64)
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    regions = (offs, u32(0, 10, 0), u32(0, 10, 0), u32(8, 10, 14), u32(1, 3, 7), u32(8, 10, 14))
    scores = (offs, u32(0, 10, 0), u32(0, 10, 0), u32(8, 10, 14), np.array([8, 10, 14], np.int64), u32(8, 10, 14), u32(8, 10, 14), u32(8, 10, 14))
    stats = (np.zeros(2, np.uint8), np.array([0.3, 0.4]), np.array([0.75, 1.0]), np.array([10.5, 12.25, 20.0]), np.array([1e-3, 2.5, 1e-9]),
             np.array([12.25, 20.0]), np.array([1e-3, 1e-9]))
    return qid, tid, regions, scores, stats


def test_region_rows_with_statistics():
    qid, tid, regions, scores, stats = _hand_made()
    plain = wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", scores=scores)
    rows = wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", scores=scores, stats=stats)
    assert [{k: v for k, v in r.items() if k not in ("region_bit_score", "region_evalue", "lambda_ratio")} for r in rows] == plain
    assert [(r["region_bit_score"], r["region_evalue"], r["lambda_ratio"]) for r in rows] == [(10.5, 1e-3, 0.75), (12.25, 2.5, 0.75), (20.0, 1e-9, 1.0)]
    al = (scores[0], scores[1], scores[3], scores[2], scores[3], scores[4], scores[5], scores[6], u32z(3), u32z(3), scores[3])
    rows = wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", alignments=al, stats=stats)
    assert [(r["aln_bit_score"], r["aln_evalue"]) for r in rows] == [(10.5, 1e-3), (12.25, 2.5), (20.0, 1e-9)] and "region_evalue" not in rows[0]
    # with a cull: the statistics of all regions, or of the kept ones alone
    cull = (np.array([0, 1, 2], np.uint64), np.array([1, 2], np.uint32), np.zeros(2, np.uint32), np.array([2, 1], np.uint32),
            np.array([1, 1, 2], np.uint32), np.array([10.0, 14.0]))
    kept = tuple(c if i < 3 else c[[1, 2]] for i, c in enumerate(stats[:5])) + stats[5:]
    for st in (stats, kept):
        rows = wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", scores=scores, cull=cull, stats=st)
        assert [(r["query_start"], r["region_evalue"]) for r in rows] == [(10, 2.5), (0, 1e-9)]
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", stats=stats)
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, qid, tid, regions, "protein", scores=scores, stats=tuple(c[:1] for c in stats))


def u32z(n):
    return np.zeros(n, np.uint32)


def test_hit_chain_rows_with_statistics():
    qid, tid = np.array([0, 1], np.uint32), np.array([0, 1], np.uint32)
    offs = np.array([0, 1, 2], np.uint64)
    chain = (offs, np.array([0, 1], np.uint32), np.zeros(2, np.int64), u32z(2), np.array([8, 14], np.int64), u32z(2), np.array([8, 14], np.uint32),
             u32z(2), np.array([8, 14], np.uint32), np.array([8, 14], np.uint32), np.array([8, 14], np.uint32), np.array([8, 14], np.uint64),
             np.array([8, 14], np.uint64), np.array([8.0, 14.0]))
    ops = np.array([8 << 4, 14 << 4], np.uint32)
    stitched = (offs, ops, u32z(2), np.array([8, 14], np.uint32), u32z(2), np.array([8, 14], np.uint32), np.array([8, 14], np.int64),
                np.array([8, 14], np.uint32), np.array([8, 14], np.uint32), u32z(2), u32z(2), np.array([8, 14], np.uint32),
                np.ones(2, np.uint32), u32z(2), u32z(2), u32z(2), np.array([8.0, 14.0]))
    stats = (np.zeros(2, np.uint8), np.zeros(2), np.ones(2), np.array([9.5, 21.0]), np.array([0.5, 1e-7]), np.array([9.5, 21.0]), np.array([0.5, 1e-7]))
    plain = wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stitched=stitched)
    rows = wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stitched=stitched, stats=stats)
    assert [{k: v for k, v in r.items() if k not in ("aln_bit_score", "aln_evalue")} for r in rows] == plain
    assert [(r["query_name"], r["aln_bit_score"], r["aln_evalue"]) for r in rows] == [("q0", 9.5, 0.5), ("q1", 21.0, 1e-7)]
    with pytest.raises(ValueError):
        wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stats=stats)


def test_search_extract_refuses_statistics_without_scores():
    for kw in (dict(evalue=True), dict(stat_params=(0.3, 0.1)), dict(max_evalue=1.0), dict(regions=True, gapped=True, evalue=True),
               dict(regions=True, score=True, chain=True, hit_rows=True, evalue=True)):
        with pytest.raises(ValueError):
            wire.search_extract_kmers_device("q.fa", "t.fa", 7, 1, "protein", **kw)
