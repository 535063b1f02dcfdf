"""No GPU: the traceback's yardstick against the alignment's, and what the fixed inputs of the GPU test exercise.

1. tests/rtrace_ref.py (tables + walk) against tests/ralign_ref.py (counts carried forward) on seeded cases: every invariant the
   header lists for a region's ops holds, and re-scoring the ops gives the alignment's score and positives.
2. The inputs test_gpu_region_trace.py runs (tests/rtrace_cases.py), on the reference alone: an I run beside a D run, an E
   jump longer than 1, a gap of exactly W at the band's edge, a leading row-0 gap next to the anchor, and a path through each
   of the four tie branches all occur.
3. RegionCigars.strings' formatting and the aln_cigar column of wire.region_rows, on hand-made arrays."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402
import ralign_ref  # noqa: E402
import regions_ref  # noqa: E402
import rtrace_cases as RC  # noqa: E402
import rtrace_ref  # noqa: E402

from kmerseek_amd import engine, wire  # noqa: E402
from oracle import oracle  # noqa: E402

M, I, D, EQ, X = rtrace_ref.M, rtrace_ref.I, rtrace_ref.D, rtrace_ref.EQ, rtrace_ref.X


def check_region(qseq, tseq, a, b, n, matrix, band, o, e, x_drop):
    """One region through both references; -> the events on its path"""
    qs, ql, ts, tl, score, ident, pos, opens, gaps, alen = ralign_ref.align_region(qseq, tseq, a, b, n, matrix, band, o, e, x_drop)
    what = (qseq, tseq, a, b, n, band, o, e, x_drop)
    events = None
    for eqx in (False, True):
        cigar, cols, tr_score, events = rtrace_ref.trace_region(qseq, tseq, a, b, n, (qs, ql, ts, tl), matrix, band, o, e, eqx=eqx)
        assert tr_score == score, what  # H of the two end cells
        assert all(x[1] != y[1] for x, y in zip(cigar, cigar[1:])) and all(k >= 1 for k, _ in cigar), what  # merged runs
        assert len(cols) == alen == sum(k for k, _ in cigar), what
        pairs = sum(k for k, c in cigar if c in (M, EQ, X))
        assert pairs + sum(k for k, c in cigar if c == I) == ql and pairs + sum(k for k, c in cigar if c == D) == tl, what
        assert sum(1 for _, c in cigar if c in (I, D)) == opens and sum(k for k, c in cigar if c in (I, D)) == gaps, what
        assert {c for _, c in cigar} <= ({EQ, X, I, D} if eqx else {M, I, D}), what
        if eqx:
            assert sum(k for k, c in cigar if c == EQ) == ident, what
        # the columns name consecutive residues of both extents
        assert [qi for _, qi, _ in cols if qi is not None] == list(range(qs, qs + ql)), what
        assert [ti for _, _, ti in cols if ti is not None] == list(range(ts, ts + tl)), what
        assert rtrace_ref.rescore(cigar, qseq, tseq, qs, ts, matrix, o, e) == (score, ident, pos, opens, gaps, alen, ql, tl), what
    return events


def seeded_matrix(rng):
    m = rng.integers(-6, 7, (28, 28))
    m[np.arange(28), np.arange(28)] = rng.integers(1, 8, 28)
    return [[int(v) for v in row] for row in m.tolist()]


def test_traceback_reference_against_the_alignment_reference():
    rng = np.random.default_rng(20240607)
    two, twenty = np.frombuffer(b"AC", np.uint8), RC.PROTEIN
    n_cases, seen = 0, set()
    for band in (0, 1, 3, 16, 31):
        for o in (0, 1, 11):
            for e in (0, 1, 11):
                for rep in range(45):
                    alpha = two if rep % 2 == 0 else twenty
                    lq, lt = (int(v) for v in rng.integers(1, [121, 41, 13][rep % 3], 2))
                    qseq = bytes(alpha[rng.integers(0, len(alpha), lq)])
                    if rep % 5 == 0:  # a relative of the query: a few substitutions and indels
                        t = bytearray(qseq)
                        for _ in range(int(rng.integers(0, 4))):
                            p = int(rng.integers(0, len(t) + 1))
                            if rng.integers(0, 2) and len(t) > 1:
                                del t[min(p, len(t) - 1):min(p, len(t) - 1) + int(rng.integers(1, 4))]
                            else:
                                t[p:p] = bytes(alpha[rng.integers(0, len(alpha), int(rng.integers(1, 4)))])
                        tseq = bytes(t) or b"A"
                    else:
                        tseq = bytes(alpha[rng.integers(0, len(alpha), lt)])
                    n = int(rng.integers(1, min(len(qseq), len(tseq), 9) + 1))
                    a, b = int(rng.integers(0, len(qseq) - n + 1)), int(rng.integers(0, len(tseq) - n + 1))
                    matrix = ralign_ref.default_matrix() if rep % 3 else seeded_matrix(rng)
                    x_drop = int([2, 30, RC.HUGE][int(rng.integers(0, 3))])
                    seen |= check_region(qseq, tseq, a, b, n, matrix, band, o, e, x_drop)
                    n_cases += 1
    assert n_cases == 5 * 3 * 3 * 45  # about 2,000
    assert seen >= {"tie_F", "tie_Ht", "tie_E", "tie_H", "E_jump_gt1", "I_beside_D", "row0_gap", "band_edge"}


def test_lower_case_and_odd_bytes_in_the_reference():
    q = b"ju\x85*zBx" + RC.CORE + b"Xa*bzjuo\x80\xffAcde*x"
    t = b"QJU\x85*ZbO" + RC.CORE + b"aA*BZJOU\x80\xfeacDE*X\x90"
    for band, o, e in ((0, 0, 0), (3, 1, 1), (31, 11, 1)):
        check_region(q, t, 7, 8, len(RC.CORE), ralign_ref.default_matrix(), band, o, e, RC.HUGE)


def reference_events(qs, ts, k, **kw):
    """The fixed input through the CPU yardsticks alone: oracle sketches and join, chained regions, alignments, paths.
    -> per region (cigar, events, band)"""
    q, t = oracle.pack(qs), oracle.pack(ts)
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], k, 1, "protein")
    rg = regions_ref.chain(join[0], join[1], join[2], k)
    al = ralign_ref.align(rg, hits[0], hits[1], q[0], q[1], t[0], t[1], **kw)
    tr = rtrace_ref.trace(rg, al, hits[0], hits[1], q[0], q[1], t[0], t[1], **{a: v for a, v in kw.items() if a != "x_drop"})
    assert len(tr) == len(rg[1]) > 0
    return [(cg, ev, kw["band"]) for cg, ev in tr]


def test_the_gpu_tests_inputs_exercise_every_branch():
    out = []
    for o in (0, 1):
        for e in (0, 1):
            qs, ts = RC.fuzz_batch(o, e)
            for kw in RC.FUZZ_OPTS:
                out += reference_events(qs, ts, RC.FUZZ_K, gap_open=o, gap_extend=e, **kw)
    for W in RC.INDEL_BANDS:
        qs, ts, cases = RC.indel_batch(W, 70 + W)
        got = reference_events(qs, ts, RC.INDEL_K, band=W, **RC.INDEL_OPTS)
        # an indel of 1 and of W is bridged from either seed as I and as D, on the left and on the right; W + 1 is not
        strings = {rtrace_ref.cigar_string(cg) for cg, _, _ in got}
        for L in {1, W}:
            assert any(f"{L}D" in s for s in strings) and any(f"{L}I" in s for s in strings), (W, L, strings)
        assert not any(f"{W + 1}D" in s or f"{W + 1}I" in s for s in strings)
        out += got
    qs, ts = RC.k1_batch()
    for kw in RC.K1_OPTS:
        out += reference_events(qs, ts, 1, **kw)
    events = set().union(*[ev for _, ev, _ in out])
    assert "I_beside_D" in events                                   # an I run directly beside a D run
    assert "E_jump_gt1" in events                                   # an E jump longer than 1
    assert any("band_edge" in ev and W >= 1 and any(k == W and c in (I, D) for k, c in cg) for cg, ev, W in out)  # a gap of exactly W at the edge
    assert "row0_gap" in events                                     # a leading row-0 gap next to the anchor
    assert {"tie_F", "tie_Ht", "tie_E", "tie_H"} <= events          # a path through each of the four tie branches


def test_cigar_strings_and_the_aln_cigar_column():
    offs = np.array([0, 5, 6, 6, 9], np.uint64)
    ops = np.array([35 << 4 | M, 2 << 4 | D, 17 << 4 | M, 1 << 4 | I, 40 << 4 | M, (2 ** 21 + 31) << 4 | M,
                    3 << 4 | EQ, 1 << 4 | X, 2 << 4 | EQ], np.uint32)
    assert engine.cigar_strings(offs, ops) == ["35M2D17M1I40M", f"{2 ** 21 + 31}M", "", "3=1X2="]
    assert engine.cigar_strings(np.zeros(1, np.uint64), np.zeros(0, np.uint32)) == []
    with pytest.raises(ValueError):
        engine.cigar_strings(np.array([0, 1], np.uint64), np.array([1 << 4 | 9], np.uint32))
    # two hit rows, three regions
    q_recs, t_recs = [("q0", b"ACDEFGHIKL"), ("q1", b"MNPQRSTVWY")], [("t0", b"ACDEFGGHIKL")]
    regions = (np.array([0, 2, 3], np.uint64), np.array([0, 6, 0], np.uint32), np.array([0, 7, 0], np.uint32),
               np.array([6, 4, 1], np.uint32), np.array([1, 1, 1], np.uint32), np.array([6, 4, 1], np.uint32))
    al = (regions[0], np.array([0, 0, 0], np.uint32), np.array([10, 10, 1], np.uint32), np.array([0, 0, 0], np.uint32),
          np.array([11, 11, 1], np.uint32), np.array([9, 9, -1], np.int64), np.array([10, 10, 0], np.uint32),
          np.array([10, 10, 0], np.uint32), np.array([1, 1, 0], np.uint32), np.array([1, 1, 0], np.uint32), np.array([11, 11, 1], np.uint32))
    cg = (np.array([0, 3, 6, 7], np.uint64),
          np.array([6 << 4 | M, 1 << 4 | D, 4 << 4 | M, 6 << 4 | M, 1 << 4 | D, 4 << 4 | M, 1 << 4 | M], np.uint32))
    qid, tid = np.array([0, 1], np.uint32), np.array([0, 0], np.uint32)
    plain = wire.region_rows(q_recs, t_recs, qid, tid, regions, "protein", alignments=al)
    rows = wire.region_rows(q_recs, t_recs, qid, tid, regions, "protein", alignments=al, cigars=cg)
    assert [r["aln_cigar"] for r in rows] == ["6M1D4M", "6M1D4M", "1M"]
    assert [{k: v for k, v in r.items() if k != "aln_cigar"} for r in rows] == plain and "aln_cigar" not in plain[0]
    assert list(rows[0])[-1] == "aln_cigar"  # one column, added last
    with pytest.raises(ValueError):
        wire.region_rows(q_recs, t_recs, qid, tid, regions, "protein", cigars=cg)  # paths without alignments
    with pytest.raises(ValueError):
        wire.region_rows(q_recs, t_recs, qid, tid, regions, "protein", alignments=al, cigars=(cg[0][:3], cg[1][:6]))
