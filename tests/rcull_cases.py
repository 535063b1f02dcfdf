"""Fixed inputs of the region cull with hand-written expected outputs: each is the smallest case that can go wrong.

A case: name, row_offsets, regions [(q_start, q_length, t_start, t_length, score)], opts (P, N, min_score) and expect:
row_offsets, src_region, rank, n_merged of the kept regions, keeper per input region (X: dropped), row_best_score (None: NaN).
"""
import math

import numpy as np

X = 0xFFFFFFFF  # KS_RCULL_NONE
T32 = 2 ** 32
BIG = 2 ** 40


def case(name, row_offsets, regions, expect, P=100, N=0, min_score=None):
    return {"name": name, "row_offsets": row_offsets, "regions": regions, "opts": {"P": P, "N": N, "min_score": min_score},
            "expect": dict(zip(("row_offsets", "src_region", "rank", "n_merged", "keeper", "row_best_score"), expect))}


def pair_rows(name, P, rows):
    """Rows of two regions [k (score 9), g (score 1)] with the hand-decided verdict `k covers g`: covered -> g names k and k stands
    for two; not covered -> both are kept, k first."""
    regions, offs, src, rank, nm, keeper = [], [0], [], [], [], []
    for k, g, covered in rows:
        b = len(regions)
        regions += [k + (9,), g + (1,)]
        offs.append(len(regions))
        if covered:
            src += [b]; rank += [0]; nm += [2]; keeper += [b, b]
        else:
            src += [b, b + 1]; rank += [0, 1]; nm += [1, 1]; keeper += [b, b + 1]
    o_offs = [0]
    for k, g, covered in rows:
        o_offs.append(o_offs[-1] + (1 if covered else 2))
    return case(name, offs, regions, (o_offs, src, rank, nm, keeper, [9] * len(rows)), P=P)


CASES = [
    case("no_rows", [0], [], ([0], [], [], [], [], [])),
    # rows without regions between rows that have some; two disjoint regions: both kept, the better one has rank 0
    case("empty_rows_between", [0, 0, 2, 2, 3, 3], [(0, 10, 0, 10, 5), (100, 10, 100, 10, 7), (0, 5, 0, 5, 3)],
         ([0, 0, 2, 2, 3, 3], [0, 1, 2], [1, 0, 0], [1, 1, 1], [0, 1, 2], [None, 7, None, 3, None])),
    case("single_passes_min_score", [0, 1], [(3, 4, 5, 6, 10)], ([0, 1], [0], [0], [1], [0], [10]), min_score=10),
    case("single_fails_min_score", [0, 1], [(3, 4, 5, 6, 9)], ([0, 0], [], [], [], [X], [None]), min_score=10),
    # two identical regions: one kept, it stands for two, the smaller index wins
    case("two_identical", [0, 2], [(5, 20, 7, 20, 50), (5, 20, 7, 20, 50)], ([0, 1], [0], [0], [2], [0, 0], [50])),
    # equal scores: the smaller index goes first and is inside the other, which it therefore cannot remove (the other way
    # round the long one would remove the short one)
    case("equal_scores_different_extents", [0, 2], [(0, 10, 0, 10, 5), (0, 20, 0, 20, 5)], ([0, 2], [0, 1], [0, 1], [1, 1], [0, 1], [5])),
    # the boundary of covers: ov * 100 == P * len against one residue less, on the query and on the target
    pair_rows("boundary_p100", 100, [
        ((10, 10, 0, 30), (10, 10, 10, 10), True),    # ovq = 10 = len
        ((11, 10, 0, 30), (10, 10, 10, 10), False),   # ovq = 9
        ((0, 30, 10, 10), (10, 10, 10, 10), True),    # ovt = 10
        ((0, 30, 11, 10), (10, 10, 10, 10), False),   # ovt = 9
    ]),
    pair_rows("boundary_p50", 50, [
        ((15, 20, 0, 40), (10, 10, 10, 10), True),    # ovq = 5: 500 >= 500
        ((16, 20, 0, 40), (10, 10, 10, 10), False),   # ovq = 4
        ((0, 40, 15, 20), (10, 10, 10, 10), True),
        ((0, 40, 16, 20), (10, 10, 10, 10), False),
    ]),
    pair_rows("boundary_p1", 1, [
        ((0, 101, 0, 1000), (100, 100, 100, 100), True),   # ovq = 1: 100 >= 100
        ((0, 100, 0, 1000), (100, 100, 100, 100), False),  # ovq = 0
        ((0, 1000, 0, 101), (100, 100, 100, 100), True),
        ((0, 1000, 0, 100), (100, 100, 100, 100), False),
        ((0, 101, 0, 1000), (100, 101, 100, 101), False),  # ovq = 1: 100 < 101, nothing is rounded
    ]),
    # covered on the query, disjoint on the target: a repeat, both kept
    case("query_covered_target_disjoint", [0, 2], [(0, 100, 0, 100, 9), (10, 10, 500, 10, 1)], ([0, 2], [0, 1], [0, 1], [1, 1], [0, 1], [9])),
    # greedy, not transitive (P = 50): A removes B; only B would have covered C; C is kept
    case("non_transitive_chain", [0, 3], [(0, 100, 0, 100, 30), (50, 100, 50, 100, 20), (110, 40, 110, 40, 10)],
         ([0, 2], [0, 2], [0, 1], [2, 1], [0, 0, 2], [30]), P=50),
    # a short high-scoring region inside a long low-scoring one: covers is relative to the region being removed, both kept
    case("short_high_inside_long_low", [0, 2], [(0, 100, 0, 100, 50), (40, 10, 40, 10, 100)], ([0, 2], [0, 1], [1, 0], [1, 1], [0, 1], [100])),
    # scores of +-2^40: a compare of the low 32 bits orders both rows the other way round
    case("scores_beyond_32_bits", [0, 2, 4], [(0, 20, 0, 20, BIG), (5, 10, 5, 10, 5), (100, 20, 100, 20, -BIG), (105, 10, 105, 10, -5)],
         ([0, 1, 3], [0, 2, 3], [0, 1, 0], [2, 1, 1], [0, 0, 2, 3], [float(BIG), -5])),
    case("negative_min_score", [0, 3], [(0, 10, 0, 10, -3), (50, 10, 50, 10, -BIG), (100, 10, 100, 10, -10)],
         ([0, 2], [0, 2], [0, 1], [1, 1], [0, X, 2], [-3]), min_score=-10),
    # q_start + q_length == 2^32 (and the same on the target): an end computed in 32 bits is 0
    case("end_at_2_32", [0, 2, 4], [(T32 - 100, 100, 0, 100, 9), (T32 - 50, 50, 50, 50, 1), (0, 100, T32 - 100, 100, 9), (50, 50, T32 - 50, 50, 1)],
         ([0, 1, 2], [0, 2], [0, 0], [2, 2], [0, 0, 2, 2], [9, 9])),
    # max_per_row: a later region that is covered still gets its keeper (rule 2 before rule 3), one that is not gets none
    case("max_per_row_1", [0, 3], [(0, 100, 0, 100, 30), (10, 10, 10, 10, 20), (500, 10, 500, 10, 10)],
         ([0, 1], [0], [0], [2], [0, 0, X], [30]), N=1),
    case("max_per_row_2", [0, 5], [(0, 100, 0, 100, 30), (10, 10, 10, 10, 20), (500, 10, 500, 10, 10), (700, 10, 700, 10, 5), (505, 2, 505, 2, 1)],
         ([0, 2], [0, 2], [0, 1], [2, 2], [0, 0, 2, X, 2], [30]), N=2),
]


DELETION_K = 7


def deletion_pair():
    """A query of 120 random residues and the target it becomes when residues [60, 63) are deleted: the shared 7-mers lie on
    two diagonals, so the chaining reports two seed fragments — (q_start, t_start, length) = (0, 0, 60) and (63, 60, 57).
    -> (query, target, the two seeds)."""
    rng = np.random.default_rng(2024)
    q = bytes(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)[rng.integers(0, 20, 120)])
    return q, q[:60] + q[63:], [(0, 0, 60), (63, 60, 57)]


def columns(c):
    """(row_offsets u64, q_start, q_length, t_start, t_length u32, score i64) of a case."""
    r = c["regions"]
    return (np.array(c["row_offsets"], np.uint64), *[np.array([g[i] for g in r], np.uint32) for i in range(4)],
            np.array([g[4] for g in r], np.int64))


def expected(c):
    """The expectation as the arrays of RegionCull.to_host()."""
    e = c["expect"]
    return (np.array(e["row_offsets"], np.uint64), np.array(e["src_region"], np.uint32), np.array(e["rank"], np.uint32),
            np.array(e["n_merged"], np.uint32), np.array(e["keeper"], np.uint32),
            np.array([math.nan if v is None else float(v) for v in e["row_best_score"]], np.float64))


def assert_same(got, want, what=""):
    names = ("row_offsets", "src_region", "rank", "n_merged", "keeper", "row_best_score")
    for n, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {n} has {g.shape}, expected {w.shape}"
        assert np.array_equal(g, w, equal_nan=(n == "row_best_score")), f"{what}: {n} = {g.tolist()}, expected {w.tolist()}"
