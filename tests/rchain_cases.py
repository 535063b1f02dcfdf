"""Fixed inputs of the region chain with hand-written expected outputs: each is the smallest case that can go wrong.

A case: name, row_offsets, regions [(q_start, q_length, t_start, t_length, score)], opts (the five options of ks_rchain_opts)
and expect: row_offsets and src_region of the chains, best and pred per input region (X: none), and per hit row chain_score,
q_aligned and t_aligned (a row without regions: 0, and NaN as its row_chain_score).  The span columns follow from the first and
the last member; identities and aln_length are not passed, so their sums are 0.
"""
import math

import numpy as np

X = 0xFFFFFFFF  # KS_RCHAIN_NONE
TOP = 0xFFFFFFFF  # the largest end a region may have


def case(name, row_offsets, regions, expect, **opts):
    return {"name": name, "row_offsets": row_offsets, "regions": regions, "opts": opts,
            "expect": dict(zip(("row_offsets", "src_region", "best", "pred", "chain_score", "q_aligned", "t_aligned"), expect))}


def pair_rows(name, rows, **opts):
    """Rows of two regions [a, b] of score 5 with the hand-decided verdict `b follows a` (the link is free): linked -> the chain
    is [a, b] and worth 10, aligned = the hand-written union lengths; not linked -> the chain is a alone (equal best: the smaller
    index), worth 5, and covers a's lengths."""
    regions, offs, o_offs, src, best, pred, score, qa, ta = [], [0], [0], [], [], [], [], [], []
    for a, b, linked, union in rows:
        at = len(regions)
        regions += [a + (5,), b + (5,)]
        offs.append(len(regions))
        src += [at, at + 1] if linked else [at]
        o_offs.append(len(src))
        best += [5, 10 if linked else 5]; pred += [X, at if linked else X]; score.append(10 if linked else 5)
        qa.append(union[0] if linked else a[1]); ta.append(union[1] if linked else a[3])
    return case(name, offs, regions, (o_offs, src, best, pred, score, qa, ta), **opts)


A10 = (0, 10, 0, 10)
CASES = [
    case("no_rows", [0], [], ([0], [], [], [], [], [], [])),
    case("two_regions_chain", [0, 2], [(0, 10, 0, 10, 5), (20, 10, 25, 10, 7)], ([0, 2], [0, 1], [5, 12], [X, 0], [12], [20], [20])),
    case("single_negative_region", [0, 1], [(3, 4, 5, 6, -7)], ([0, 1], [0], [-7], [X], [-7], [4], [6])),
    # follows needs strictly ascending starts and ends: equal q_start, equal q_end
    case("equal_q_start", [0, 2], [(0, 10, 0, 10, 5), (0, 12, 5, 12, 7)], ([0, 1], [1], [5, 7], [X, X], [7], [12], [12])),
    case("equal_q_end", [0, 2], [(0, 10, 0, 10, 5), (5, 5, 20, 5, 7)], ([0, 1], [1], [5, 7], [X, X], [7], [5], [5])),
    # two domains in swapped order: ascending on the query, descending on the target: a chain of one — the better, or with
    # equal scores the smaller index
    case("swapped_domains", [0, 2, 4], [(0, 50, 100, 50, 30), (100, 50, 0, 50, 40), (0, 50, 100, 50, 30), (100, 50, 0, 50, 30)],
         ([0, 1, 2], [1, 2], [30, 40, 30, 30], [X, X, X, X], [40, 30], [50, 50], [50, 50])),
    # ov == max_overlap links, one more does not: on the query, then on the target
    pair_rows("overlap_boundary", [(A10, (7, 10, 10, 10), True, (17, 20)), (A10, (6, 10, 10, 10), False, None),
                                   (A10, (10, 10, 7, 10), True, (20, 17)), (A10, (10, 10, 6, 10), False, None)], max_overlap=3),
    # max(dq, dt) == max_gap links, one more does not
    pair_rows("gap_boundary", [(A10, (20, 10, 12, 10), True, (20, 20)), (A10, (21, 10, 12, 10), False, None),
                               (A10, (12, 10, 20, 10), True, (20, 20)), (A10, (12, 10, 21, 10), False, None)], max_gap=10),
    # best[j] - cost exactly 0: not taken (the chain is b alone); exactly 1: taken
    case("link_worth_0_and_1", [0, 2, 4], [(0, 10, 0, 10, 5), (20, 10, 20, 10, 10), (0, 10, 0, 10, 6), (20, 10, 20, 10, 10)],
         ([0, 1, 3], [1, 2, 3], [5, 10, 6, 11], [X, X, X, 2], [10, 11], [10, 20], [10, 20]), link_cost=5),
    # dq = 5, dt = 2: the link costs 2 * 3
    case("skew_cost", [0, 2], [(0, 10, 0, 10, 20), (15, 10, 12, 10, 20)], ([0, 2], [0, 1], [20, 34], [X, 0], [34], [20], [20]), skew_cost=2),
    # an overlap of 3 on the query costs 4 * 3
    case("overlap_cost", [0, 2], [(0, 10, 0, 10, 20), (7, 10, 10, 10, 20)], ([0, 2], [0, 1], [20, 28], [X, 0], [28], [17], [20]),
         max_overlap=3, overlap_cost=4),
    # two predecessors of equal value: the smaller index wins, though the other one is evaluated first (it starts earlier)
    case("equal_predecessors", [0, 3], [(1, 10, 1, 10, 5), (0, 10, 0, 10, 5), (30, 10, 30, 10, 5)],
         ([0, 2], [0, 2], [5, 5, 10], [X, X, 0], [10], [20], [20])),
    # two end regions of equal best: the smaller index wins, though it starts later
    case("equal_ends", [0, 2], [(5, 10, 0, 10, 5), (0, 10, 50, 10, 5)], ([0, 1], [0], [5, 5], [X, X], [5], [10], [10])),
    # a region of negative score between two good ones is skipped (it still links back: 10 - 4 > 0)
    case("negative_region_skipped", [0, 3], [(0, 10, 0, 10, 10), (15, 5, 15, 5, -4), (30, 10, 30, 10, 10)],
         ([0, 2], [0, 2], [10, 6, 20], [X, 0, 0], [20], [20], [20])),
    case("empty_rows_between", [0, 0, 2, 2, 3, 3], [(0, 10, 0, 10, 5), (20, 10, 20, 10, 7), (0, 5, 0, 5, 3)],
         ([0, 0, 2, 2, 3, 3], [0, 1, 2], [5, 12, 3], [X, 0, X], [None, 12, None, 3, None], [0, 20, 0, 5, 0], [0, 20, 0, 5, 0])),
    # the union with a short middle member: [0,100) + [95,103) + [98,200) is 200 positions, not 100 + 8 + 102 - overlaps of the ends
    case("union_short_middle", [0, 3], [(0, 100, 0, 100, 10), (95, 8, 95, 8, 10), (98, 102, 98, 102, 10)],
         ([0, 3], [0, 1, 2], [10, 20, 30], [X, 0, 1], [30], [200], [200]), max_overlap=5),
    # q_end == 0xffffffff (and the same on the target): ends are not computed in 32 bits
    case("end_at_top", [0, 2, 4], [(TOP - 200, 100, 0, 100, 5), (TOP - 100, 100, 100, 100, 5), (0, 100, TOP - 200, 100, 5), (100, 100, TOP - 100, 100, 5)],
         ([0, 2, 4], [0, 1, 2, 3], [5, 10, 5, 10], [X, 0, X, 2], [10, 10], [200, 200], [200, 200])),
]


INSERTION_K = 7
INSERTION = 40


def insertion_pair():
    """A target of 120 random residues and the query it becomes when 40 random residues are inserted after residue 60: the
    shared 7-mers lie on two diagonals 40 apart, so the chaining reports two seed regions — (q_start, t_start, length) =
    (0, 0, 60) and (100, 60, 60) — that neither the band (<= 31) nor the X-drop can bridge.  -> (query, target, the two seeds)."""
    rng = np.random.default_rng(2027)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    t = bytes(aa[rng.integers(0, 20, 120)])
    ins = bytes(aa[rng.integers(0, 20, INSERTION)])
    return t[:60] + ins + t[60:], t, [(0, 0, 60), (100, 60, 60)]


def columns(c):
    """(row_offsets u64, q_start, q_length, t_start, t_length u32, score i64) of a case."""
    r = c["regions"]
    return (np.array(c["row_offsets"], np.uint64), *[np.array([g[i] for g in r], np.uint32) for i in range(4)],
            np.array([g[4] for g in r], np.int64))


def expected(c):
    """The expectation as the arrays of RegionChain.to_host()."""
    e, r = c["expect"], c["regions"]
    offs, src = e["row_offsets"], e["src_region"]
    span = [[], [], [], []]
    for i in range(len(offs) - 1):
        f, l = (r[src[offs[i]]], r[src[offs[i + 1] - 1]]) if offs[i + 1] > offs[i] else ((0, 0, 0, 0), (0, 0, 0, 0))
        for col, v in zip(span, (f[0], l[0] + l[1] - f[0], f[2], l[2] + l[3] - f[2])):
            col.append(v)
    n_rows = len(offs) - 1
    return (np.array(offs, np.uint64), np.array(src, np.uint32), np.array(e["best"], np.int64), np.array(e["pred"], np.uint32),
            np.array([0 if v is None else v for v in e["chain_score"]], np.int64), *[np.array(col, np.uint32) for col in span],
            np.array(e["q_aligned"], np.uint32), np.array(e["t_aligned"], np.uint32), np.zeros(n_rows, np.uint64), np.zeros(n_rows, np.uint64),
            np.array([math.nan if v is None else float(v) for v in e["chain_score"]], np.float64))


NAMES = ("row_offsets", "src_region", "best", "pred", "chain_score", "q_start", "q_length", "t_start", "t_length", "q_aligned",
         "t_aligned", "identities", "aln_length", "row_chain_score")


def assert_same(got, want, what=""):
    assert len(got) == len(want) == len(NAMES)
    for n, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype, f"{what}: {n} is {g.dtype}, expected {w.dtype}"
        assert g.shape == w.shape, f"{what}: {n} has {g.shape}, expected {w.shape}"
        if not np.array_equal(g, w, equal_nan=(n == "row_chain_score")):
            at = np.flatnonzero(~((g == w) | ((g != g) & (w != w))))[:8]
            raise AssertionError(f"{what}: {n} differs at {at.tolist()}: got {g[at].tolist()}, expected {w[at].tolist()}")
