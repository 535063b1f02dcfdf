"""CPU: the yardstick of the region-alignment tests (tests/ralign_ref.py) against an independent three-matrix Gotoh over the
band, against the ungapped rule of tests/rscore_ref.py at band 0 and against indels worked out by hand; the option checks of
Context._ralign_opts and the alignment columns of wire.region_rows.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rscore_ref  # noqa: E402

from kmerseek_amd import Context, wire  # noqa: E402

PM = ralign_ref.default_matrix()
HUGE = 2 ** 20
NEG = -10 ** 9


def gotoh_band_best(Q, T, matrix, W, o, e):
    """The largest H of the textbook three-matrix affine-gap recurrence (H, E, F full matrices, E and F both read H) over the
    cells |y - x| <= W, H(0, 0) = 0: what an extension without X-drop scores.  Written apart from ralign_ref on purpose."""
    X, Y = len(Q), len(T)
    H = np.full((X + 1, Y + 1), NEG, np.int64)
    E = np.full((X + 1, Y + 1), NEG, np.int64)
    F = np.full((X + 1, Y + 1), NEG, np.int64)
    H[0, 0] = 0
    for x in range(X + 1):
        for y in range(Y + 1):
            if abs(y - x) > W or (x == 0 and y == 0):
                continue
            if y >= 1 and abs(y - 1 - x) <= W:
                E[x, y] = max(H[x, y - 1] - o - e, E[x, y - 1] - e)
            if x >= 1 and abs(y - (x - 1)) <= W:
                F[x, y] = max(H[x - 1, y] - o - e, F[x - 1, y] - e)
            d = NEG
            if x >= 1 and y >= 1:
                d = H[x - 1, y - 1] + int(matrix[ralign_ref.residue_class(Q[x - 1])][ralign_ref.residue_class(T[y - 1])])
            H[x, y] = max(d, E[x, y], F[x, y])
    return int(H.max())


@pytest.mark.parametrize("letters", [b"AC", b"ACGT"])
def test_scores_equal_three_matrix_gotoh(letters):
    rng = np.random.default_rng(len(letters))
    alpha = np.frombuffer(letters, np.uint8)
    n = 0
    for W in (0, 1, 2, 5, 31):
        for o in (0, 1, 2, 5, 11):
            for e in (0, 1, 2):
                for _ in range(20):
                    Q = bytes(alpha[rng.integers(0, len(alpha), int(rng.integers(0, 13)))])
                    T = bytes(alpha[rng.integers(0, len(alpha), int(rng.integers(0, 13)))])
                    got = ralign_ref.extend(Q, T, PM, W, o, e, HUGE)
                    assert got[2] == gotoh_band_best(Q, T, PM, W, o, e), (Q, T, W, o, e, got)
                    x, y, _, ident, pos, opens, gaps = got
                    assert 0 <= x <= len(Q) and 0 <= y <= len(T) and abs(y - x) <= W and opens <= gaps and (x + y - gaps) % 2 == 0
                    assert ident == pos <= (x + y - gaps) // 2  # +1 / -1: the positives are the identities
                    n += 1
    assert n == 1500


def test_band_zero_is_the_ungapped_rule_from_the_anchor():
    rng = np.random.default_rng(7)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    m = np.random.default_rng(8).integers(-4, 5, (28, 28)).tolist()
    for i in range(600):
        Q = bytes(alpha[rng.integers(0, 4, int(rng.integers(0, 40)))])
        T = bytes(alpha[rng.integers(0, 4, int(rng.integers(0, 40)))])
        matrix = PM if i % 2 else m
        for x_drop in (0, 1, 3, HUGE):
            ext, score, ident, pos = rscore_ref.extend(list(zip(Q, T)), matrix, x_drop)
            assert ralign_ref.extend(Q, T, matrix, 0, 11, 1, x_drop) == (ext, ext, score, ident, pos, 0, 0), (Q, T, x_drop)


# ---- by hand ------------------------------------------------------------------------------------------------------------------
def test_small_cases_by_hand():
    # nothing to extend
    assert ralign_ref.extend(b"", b"", PM, 5, 1, 1, 0) == (0, 0, 0, 0, 0, 0, 0)
    assert ralign_ref.extend(b"AAA", b"", PM, 5, 1, 1, HUGE) == (0, 0, 0, 0, 0, 0, 0)
    # free gaps: every cell of row 0 is 0; the smallest y wins
    assert ralign_ref.extend(b"", b"AAA", PM, 5, 0, 0, HUGE) == (0, 0, 0, 0, 0, 0, 0)
    # Q = AC, T = AGC, o = 0, e = 1: A-A, a gap under G (-1), C-C: 1; equal to A-A alone: the smallest x wins
    assert ralign_ref.extend(b"AC", b"AGC", PM, 2, 0, 1, HUGE) == (1, 1, 1, 1, 1, 0, 0)
    # ... and with a second C-C... Q = ACC, T = AGCC: 1 - 1 + 2 = 2 at (3, 4), one gap of one residue in the query
    assert ralign_ref.extend(b"ACC", b"AGCC", PM, 2, 0, 1, HUGE) == (3, 4, 2, 3, 3, 1, 1)
    # the same gap on the other side (F)
    assert ralign_ref.extend(b"AGCC", b"ACC", PM, 2, 0, 1, HUGE) == (4, 3, 2, 3, 3, 1, 1)
    # D against F on a tie: D.  Q = CA, T = A, o = e = 0: (1, 1) is a mismatch -1; (2, 1): D = H(1, 0) + 1 = 0 + 1
    assert ralign_ref.extend(b"CA", b"A", PM, 1, 0, 0, HUGE) == (2, 1, 1, 1, 1, 1, 1)
    # a dip of exactly x_drop goes on, one more stops: + - - + + + with the row maximum on the diagonal (band 0)
    assert ralign_ref.extend(b"AAAAAAA", b"ACCAAAA", PM, 0, 1, 1, 2) == (7, 7, 3, 5, 5, 0, 0)
    assert ralign_ref.extend(b"AAAAAAA", b"ACCAAAA", PM, 0, 1, 1, 1) == (1, 1, 1, 1, 1, 0, 0)
    # an equal maximum in a later row does not win: + - +
    assert ralign_ref.extend(b"AAA", b"ACA", PM, 0, 1, 1, HUGE) == (1, 1, 1, 1, 1, 0, 0)


def _indel_case(W, L, side, kind, seed):
    """q = left(110) + X + right(110) over 20 letters, the anchor X in the middle; the target equals it but for L residues
    inserted into (`ins`) or deleted from (`del`) the flank on `side`, 10 residues away from the anchor: 100 identities wait
    behind a gap that costs 5 + L <= 36."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    seq = lambda n: bytes(alpha[rng.integers(0, 20, n)])
    left, right = seq(110), seq(110)
    q = left + b"W" + right
    if side > 0:
        t = left + b"W" + right[:10] + (seq(L) + right[10:] if kind == "ins" else right[10 + L:])
        b = 110
    else:
        t = (left[:100] + seq(L) if kind == "ins" else left[:100 - L]) + left[100:] + b"W" + right
        b = len(t) - 111
    return q, t, b


@pytest.mark.parametrize("W", [4, 31])
@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("kind", ["ins", "del"])
def test_one_indel_on_either_side_of_the_anchor(W, side, kind):
    for L in (1, W, W + 1):
        q, t, b = _indel_case(W, L, side, kind, 100 * W + L)
        got = ralign_ref.align_region(q, t, 110, b, 1, PM, W, 5, 1, HUGE)
        q_start, q_len, t_start, t_len, score, ident, pos, opens, gaps, aln_len = got
        if L <= W:  # bridged: both sequences from end to end, one gap of L residues
            pairs = min(len(q), len(t))
            assert got == (0, 221, 0, len(t), pairs - (5 + L), pairs, pairs, 1, L, pairs + L), (L, got)
        else:       # one residue beyond the band: no path to the other diagonal; what an odd chance match is worth is no gap's price
            assert (opens, gaps) == (0, 0) and q_len == t_len == aln_len and q_len < 221, (L, got)
            if side > 0:
                assert (q_start, t_start) == (0, 0) and 121 <= q_len <= 125
            else:
                assert q_start + q_len == 221 and t_start + t_len == len(t) and 121 <= q_len <= 125


def test_anchor_is_the_middle_of_the_seed():
    q, t = b"CCCCAAAACCCC", b"GGAAAAGG"
    for n, (a, b) in ((4, (4, 2)), (3, (4, 2)), (1, (7, 5)), (2, (5, 3))):
        got = ralign_ref.align_region(q, t, a, b, n, PM, 3, 2, 1, HUGE)
        assert got == (4, 4, 2, 4, 4, 4, 4, 0, 0, 4), (n, got)
    # lower case is an identity with its upper case; '*' and other bytes have classes of their own
    assert ralign_ref.align_region(b"a*\x80", b"A*\x81", 1, 1, 1, PM, 0, 1, 1, HUGE) == (0, 3, 0, 3, 3, 2, 3, 0, 0, 3)


# ---- the option checks ---------------------------------------------------------------------------------------------------------
def test_ralign_opts_refusals():
    o, keep = Context._ralign_opts(None, 16, 11, 1, 30)
    assert (o.band, o.gap_open, o.gap_extend, o.x_drop, o.flags, keep) == (16, 11, 1, 30, 0, None) and not o.matrix
    o, keep = Context._ralign_opts(np.zeros((28, 28), np.int8), 31, 255, 255, 2 ** 20)
    assert (o.band, o.gap_open, o.gap_extend, o.x_drop) == (31, 255, 255, 2 ** 20) and keep is not None and bool(o.matrix)
    Context._ralign_opts(None, 0, 0, 0, 0)
    for bad in ((None, 32, 11, 1, 30), (None, -1, 11, 1, 30), (None, 16, 256, 1, 30), (None, 16, -1, 1, 30), (None, 16, 11, 256, 30),
                (None, 16, 11, -1, 30), (None, 16, 11, 1, 2 ** 20 + 1), (None, 16, 11, 1, -1), (None, 1.5, 11, 1, 30),
                (None, True, 11, 1, 30), (np.zeros((20, 20), np.int8), 16, 11, 1, 30), (np.zeros((28, 28), np.int32), 16, 11, 1, 30)):
        with pytest.raises(ValueError):
            Context._ralign_opts(*bad)


# ---- the wire ---------------------------------------------------------------------------------------------------------------------
def test_region_rows_alignment_columns():
    q_records = [("q0", b"ACDEFGHIKLMNPQ")]
    t_records = [("t0", b"ACDEFGHIKLMNPQ"), ("t1", b"WWACDEFGHIKL")]
    qid, tid = [0, 0], [0, 1]
    regions = (np.array([0, 1, 3], np.uint64), np.array([0, 0, 5], np.uint32), np.array([0, 2, 7], np.uint32), np.array([14, 5, 5], np.uint32),
               np.array([8, 1, 1], np.uint32), np.array([14, 5, 5], np.uint32))
    al = (np.array([0, 1, 3], np.uint64), np.array([0, 0, 0], np.uint32), np.array([14, 10, 12], np.uint32), np.array([0, 2, 2], np.uint32),
          np.array([14, 10, 9], np.uint32), np.array([14, 10, -3], np.int64), np.array([14, 10, 7], np.uint32), np.array([14, 10, 8], np.uint32),
          np.array([0, 0, 1], np.uint32), np.array([0, 0, 3], np.uint32), np.array([14, 10, 12], np.uint32))
    plain = wire.region_rows(q_records, t_records, qid, tid, regions, "protein")
    rows = wire.region_rows(q_records, t_records, qid, tid, regions, "protein", alignments=al)
    added = ("aln_score", "aln_q_start", "aln_q_end", "aln_t_start", "aln_t_end", "aln_length", "aln_identities", "aln_positives",
             "aln_mismatches", "aln_gap_opens", "aln_gaps", "aln_pident")
    assert [{k: v for k, v in r.items() if k not in added} for r in rows] == plain  # nothing else changes, the order included
    assert all(list(r)[-len(added):] == list(added) for r in rows) and not any(k in plain[0] for k in added)
    last = [r for r in rows if r["match_name"] == "t1" and r["query_start"] == 5][0]
    assert [last[k] for k in added] == [-3, 0, 12, 2, 11, 12, 7, 8, 2, 1, 3, wire.format_f64(100.0 * 7 / 12)]
    first = [r for r in rows if r["match_name"] == "t0"][0]
    assert [first[k] for k in added] == [14, 0, 14, 0, 14, 14, 14, 14, 0, 0, 0, wire.format_f64(100.0)]
    with pytest.raises(ValueError):
        wire.region_rows(q_records, t_records, qid, tid, regions, "protein", alignments=(np.array([0, 2, 3], np.uint64),) + al[1:])
