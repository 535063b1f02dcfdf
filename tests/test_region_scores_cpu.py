"""CPU: the yardstick of the region-score tests (tests/rscore_ref.py) against cases worked out by hand, the NCBI matrix reader
and the scored rows of wire.region_rows.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rscore_ref  # noqa: E402

from kmerseek_amd import wire  # noqa: E402

PM = rscore_ref.default_matrix()


def _pairs(q, t):
    return list(zip(q, t))


# ---- the class table -----------------------------------------------------------------------------------------------------
def test_class_table_over_all_bytes():
    for x in range(256):
        c = rscore_ref.residue_class(x)
        ch = chr(x)
        if "A" <= ch <= "Z":
            assert c == x - 65
        elif "a" <= ch <= "z":
            assert c == x - 97
        elif ch == "*":
            assert c == 26
        else:
            assert c == 27
        assert rscore_ref.upper(x) == (x - 32 if "a" <= ch <= "z" else x)
    assert sorted({rscore_ref.residue_class(x) for x in range(256)}) == list(range(28))
    assert rscore_ref.ALPHABET == 28 and len(PM) == 28 and all(PM[i][j] == (1 if i == j else -1) for i in range(28) for j in range(28))


# ---- one side's extension, by hand (+1 / -1: S_j is matches minus mismatches) -----------------------------------------------
def test_tie_the_shortest_extension_wins():
    # s = +1 -1 +1: S = 1 0 1, the best 1 is reached at j = 1 and again at j = 3
    assert rscore_ref.extend(_pairs(b"AAA", b"ACA"), PM, 5) == (1, 1, 1, 1)
    # s = -1 +1: S = -1 0, the best is S_0 = 0 — the empty extension wins against j = 2
    assert rscore_ref.extend(_pairs(b"CA", b"AA"), PM, 5) == (0, 0, 0, 0)


def test_x_drop_zero_stops_at_the_first_step_below_the_best():
    # s = +1 +1 -1 +1 +1 +1: at j = 3 S = 1 < B = 2
    assert rscore_ref.extend(_pairs(b"AAAAAA", b"AACAAA"), PM, 0) == (2, 2, 2, 2)
    assert rscore_ref.extend(_pairs(b"C", b"A"), PM, 0) == (0, 0, 0, 0)
    assert rscore_ref.extend([], PM, 0) == (0, 0, 0, 0)


def test_termination_exactly_at_x_drop_and_one_beyond():
    # s = +1 -1 -1 +1 +1 +1 +1: S = 1 0 -1 0 1 2 3: the dip lies 2 below the best
    p = _pairs(b"AAAAAAA", b"ACCAAAA")
    assert rscore_ref.extend(p, PM, 2) == (7, 3, 5, 5)  # B - S = 2 is not > 2: goes on, recovers
    assert rscore_ref.extend(p, PM, 1) == (1, 1, 1, 1)  # 2 > 1: stops at j = 3, the best prefix is j = 1
    assert rscore_ref.extend(p, PM, 2 ** 32 - 1) == (7, 3, 5, 5)


def test_positives_follow_the_matrix_and_identities_the_bytes():
    m = [row[:] for row in PM]
    m[0][2] = 3    # query A over target C scores +3: a positive, not an identity
    m[2][0] = -7   # ... and the matrix is not symmetric
    m[3][3] = -2   # D over D: an identity, not a positive
    assert rscore_ref.extend(_pairs(b"Ad", b"CD"), m, 10) == (1, 3, 0, 1)
    assert rscore_ref.extend(_pairs(b"CA", b"AA"), m, 10) == (0, 0, 0, 0)
    assert rscore_ref.extend(_pairs(b"aD", b"Ad"), m, 10) == (1, 1, 1, 1)


# ---- whole regions ---------------------------------------------------------------------------------------------------------
def test_region_core_and_both_extensions():
    #          0123456789
    q = b"GGACDEFKLW"
    t = b"TTGACDEFKLWW"
    # core: q[3:6] = CDE over t[4:7] = CDE.  right: F K L W match, then the query ends: +4.  left: A, G match, then G / T: S = 1 2 1
    assert rscore_ref.score_region(q, t, 3, 4, 3, PM, False, 0) == (3, 4, 3, 3, 3, 3, 3)
    assert rscore_ref.score_region(q, t, 3, 4, 3, PM, True, 0) == (1, 2, 9, 9, 9, 9, 3)
    assert rscore_ref.score_region(q, t, 3, 4, 3, PM, True, 9) == (1, 2, 9, 9, 9, 9, 3)
    # the target ends first on the right, the target starts first on the left
    assert rscore_ref.score_region(b"AACDEFF", b"ACDEF", 2, 1, 3, PM, True, 3) == (1, 0, 5, 5, 5, 5, 3)
    # a region that touches both starts and both ends: nothing to extend
    assert rscore_ref.score_region(b"CDE", b"CDE", 0, 0, 3, PM, True, 3) == (0, 0, 3, 3, 3, 3, 3)
    # a core with a mismatch: core_identities counts the core alone, lower case is folded
    assert rscore_ref.score_region(b"acXde", b"ACYDE", 1, 1, 3, PM, True, 1) == (0, 0, 5, 3, 4, 4, 2)


def test_score_over_rows():
    q_res, q_off = np.frombuffer(b"GGACDEFKLW" + b"CDE", np.uint8), np.array([0, 10, 13], np.uint64)
    t_res, t_off = np.frombuffer(b"CDE" + b"TTGACDEFKLWW", np.uint8), np.array([0, 3, 15], np.uint64)
    regions = (np.array([0, 1, 1, 2], np.uint64), np.array([3, 0], np.uint32), np.array([4, 0], np.uint32), np.array([3, 3], np.uint32))
    got = rscore_ref.score(regions, [0, 0, 1], [1, 0, 0], q_res, q_off, t_res, t_off, extend=True, x_drop=2)
    assert [c.tolist() for c in got] == [[0, 1, 1, 2], [1, 0], [2, 0], [9, 3], [9, 3], [9, 3], [9, 3], [3, 3]]
    assert [c.dtype for c in got] == [np.uint64, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32]
    empty = rscore_ref.score((np.zeros(1, np.uint64),) + (np.zeros(0, np.uint32),) * 3, [], [], q_res, q_off, t_res, t_off)
    assert empty[0].tolist() == [0] and all(len(c) == 0 for c in empty[1:])


# ---- the matrix reader ---------------------------------------------------------------------------------------------------
MATRIX_TEXT = """# a small matrix
#  second comment line
   A  R  *  B  1
A  4 -1 -4 -2  0   # trailing comment
R -2  5 -4 -1  0
*  -4 -4  1 -4  0
b  9  9  9  9  9
"""


def test_read_score_matrix(tmp_path):
    p = tmp_path / "small.mat"
    p.write_text(MATRIX_TEXT)
    m = wire.read_score_matrix(str(p))
    assert m.shape == (28, 28) and m.dtype == np.int8
    A, R, B, STAR = 0, 17, 1, 26
    want = np.full((28, 28), -4, np.int8)  # pairs the file does not give: its smallest value
    want[A, A], want[A, R], want[A, STAR], want[A, B] = 4, -1, -4, -2
    want[R, A], want[R, R], want[R, STAR], want[R, B] = -2, 5, -4, -1  # (not symmetric: the row is the first symbol)
    want[STAR, A], want[STAR, R], want[STAR, STAR], want[STAR, B] = -4, -4, 1, -4
    assert np.array_equal(m, want)  # ('1' and 'b' are no residue classes: ignored)
    assert m[27, 27] == -4 and m[B, A] == -4


@pytest.mark.parametrize("text,why", [
    ("", "no matrix"), ("# only a comment\n", "no matrix"), ("  A R\n", "no matrix"),
    ("  A R\nA 1\n", "values"), ("  A R\nA 1 2 3\n", "values"), ("  A R\nA 1 x\n", "not an integer"), ("  A R\nA 1 2.5\n", "not an integer"),
    ("  A R\nA 1 128\n", "int8"), ("  A R\nA -129 1\n", "int8"), ("  A R\nA 1 2\nA 1 2\n", "twice"), ("  A A\nA 1 2\n", "twice"),
])
def test_read_score_matrix_errors(tmp_path, text, why):
    p = tmp_path / "bad.mat"
    p.write_text(text)
    with pytest.raises(ValueError) as e:
        wire.read_score_matrix(str(p))
    assert why in str(e.value)


def test_read_score_matrix_int8_limits(tmp_path):
    p = tmp_path / "lim.mat"
    p.write_text("  A C\nA 127 -128\nC 0 1\n")
    m = wire.read_score_matrix(str(p))
    assert (m[0, 0], m[0, 2], m[2, 0], m[2, 2], m[5, 5]) == (127, -128, 0, 1, -128)


# ---- scored region rows ----------------------------------------------------------------------------------------------------
def test_region_rows_with_scores():
    q_recs = [("q0", b"ggacdefklw")]
    t_recs = [("t0", b"CDE"), ("t1", b"TTGACDEFKLWW")]
    qid, tid = [0, 0], [0, 1]
    regions = (np.array([0, 1, 2], np.uint64), np.array([3, 3], np.uint32), np.array([0, 4], np.uint32), np.array([3, 3], np.uint32),
               np.array([1, 1], np.uint32), np.array([3, 3], np.uint32))
    plain = wire.region_rows(q_recs, t_recs, qid, tid, regions, "hp")
    assert plain == wire.region_rows(q_recs, t_recs, qid, tid, regions, "hp", scores=None)
    assert [sorted(r) for r in plain] == [sorted(["match_name", "query_name", "query_start", "query_end", "query", "match_start", "match_end",
                                                  "match", "encoded", "length", "n_kmers", "covered"])] * 2
    scores = (regions[0], np.array([3, 1], np.uint32), np.array([0, 2], np.uint32), np.array([3, 9], np.uint32), np.array([3, -7], np.int64),
              np.array([3, 8], np.uint32), np.array([3, 9], np.uint32), np.array([3, 3], np.uint32))
    rows = wire.region_rows(q_recs, t_recs, qid, tid, regions, "hp", scores=scores)
    assert rows[0] == {"match_name": "t1", "query_name": "q0", "query_start": 1, "query_end": 10, "query": "GACDEFKLW", "match_start": 2,
                       "match_end": 11, "match": "GACDEFKLW", "encoded": wire.encode_kmer("GACDEFKLW", "hp"), "length": 9, "n_kmers": 1,
                       "covered": 3, "score": -7, "identities": 8, "positives": 9, "pident": wire.format_f64(100.0 * 8 / 9),
                       "seed_start": 3, "seed_length": 3}
    assert rows[1] == {**plain[0], "score": 3, "identities": 3, "positives": 3, "pident": "100.0", "seed_start": 3, "seed_length": 3}
    assert rows[0]["pident"] == "88.88888888888889"
    with pytest.raises(ValueError):
        wire.region_rows(q_recs, t_recs, qid, tid, regions, "hp", scores=(np.array([0, 2, 2], np.uint64),) + scores[1:])
