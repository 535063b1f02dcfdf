"""The region cull in plain Python loops, straight from the contract in include/kmerseek_amd.h: a sort by (-score, index), then
the four rules.  Python integers: nothing here can overflow.  The yardstick of ks_regions_cull_device."""
import math

import numpy as np

NONE = 0xFFFFFFFF


def covers(P, k, g):
    """k, g: (q_start, q_length, t_start, t_length).  k covers g: at least P percent of g on both sequences."""
    ovq = max(0, min(k[0] + k[1], g[0] + g[1]) - max(k[0], g[0]))
    ovt = max(0, min(k[2] + k[3], g[2] + g[3]) - max(k[2], g[2]))
    return ovq * 100 >= P * g[1] and ovt * 100 >= P * g[3]


def cull_row(ext, score, P=100, N=0, min_score=None):
    """One row: ext[i] = (q_start, q_length, t_start, t_length), score[i].  -> (keeper by local index, None: dropped; the kept
    local indices in priority order)."""
    P = P or 100
    n = len(ext)
    keeper = [None] * n
    kept = []
    for g in sorted(range(n), key=lambda i: (-score[i], i)):
        if min_score is not None and score[g] < min_score:
            continue                                   # rule 1
        k = next((k for k in kept if covers(P, ext[k], ext[g])), None)
        if k is not None:
            keeper[g] = k                              # rule 2
        elif N and len(kept) >= N:
            continue                                   # rule 3
        else:
            keeper[g] = g                              # rule 4
            kept.append(g)
    return keeper, kept


def cull(row_offsets, q_start, q_length, t_start, t_length, score, P=100, N=0, min_score=None):
    """-> (row_offsets u64, src_region u32, rank u32, n_merged u32, keeper u32, row_best_score f64), as RegionCull.to_host().
    t_length None: the query lengths."""
    offs = [int(v) for v in row_offsets]
    qs, ql, ts = [[int(v) for v in c] for c in (q_start, q_length, t_start)]
    tl = ql if t_length is None else [int(v) for v in t_length]
    sc = [int(v) for v in score]
    n_rows, n = len(offs) - 1, len(qs)
    keeper = [NONE] * n
    o_offs, src, rank, nm, best = [0], [], [], [], []
    for r in range(n_rows):
        b, e = offs[r], offs[r + 1]
        ext = [(qs[g], ql[g], ts[g], tl[g]) for g in range(b, e)]
        kp, kept = cull_row(ext, sc[b:e], P, N, min_score)
        for i, k in enumerate(kp):
            if k is not None:
                keeper[b + i] = b + k
        rk = {g: i for i, g in enumerate(kept)}
        for g in sorted(kept):
            src.append(b + g); rank.append(rk[g]); nm.append(sum(1 for k in kp if k == g))
        o_offs.append(len(src))
        best.append(float(sc[b + kept[0]]) if kept else math.nan)
    return (np.array(o_offs, np.uint64), np.array(src, np.uint32), np.array(rank, np.uint32), np.array(nm, np.uint32),
            np.array(keeper, np.uint32), np.array(best, np.float64))


def fuzz_rows(seed, n_rows, max_len, span=60, tie_scores=True, lengths=None, n_centres=None):
    """Rows of 0 .. max_len regions whose intervals are drawn around a few shared centres per row, so that coverage is frequent;
    scores from a small range, so that ties are.  lengths: the rows' lengths instead of random ones; n_centres: centres per row
    instead of a quarter of its length.  -> (row_offsets, q_start, q_length, t_start, t_length, score) as numpy columns."""
    rng = np.random.default_rng(seed)
    offs, cols = [0], [[], [], [], [], []]
    for r in range(len(lengths) if lengths is not None else n_rows):
        m = int(rng.integers(0, max_len + 1)) if lengths is None else int(lengths[r])
        centres = rng.integers(span, 20 * span, size=(n_centres or max(1, m // 4 + 1), 2))
        for _ in range(m):
            cq, ct = centres[int(rng.integers(0, len(centres)))]
            ql, tl = int(rng.integers(1, span)), int(rng.integers(1, span))
            if rng.random() < 0.3:
                tl = ql
            cols[0].append(int(cq) - ql // 2 + int(rng.integers(-3, 4))); cols[1].append(ql)
            cols[2].append(int(ct) - tl // 2 + int(rng.integers(-3, 4))); cols[3].append(tl)
            cols[4].append(int(rng.integers(-5, 40)) if tie_scores else int(rng.integers(-2 ** 40, 2 ** 40)))
        offs.append(len(cols[0]))
    return (np.array(offs, np.uint64), np.array(cols[0], np.uint32), np.array(cols[1], np.uint32), np.array(cols[2], np.uint32),
            np.array(cols[3], np.uint32), np.array(cols[4], np.int64))
