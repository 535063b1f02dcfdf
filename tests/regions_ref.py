"""CPU restatement of ks_match_regions for the tests: the pairs of `matchpos_join.join` (itself built on the oracle) chained per
hit row into maximal colinear regions, in integers.  Not a test module."""
import numpy as np

COLUMNS = ("row_offsets", "q_start", "t_start", "length", "n_kmers", "covered")


def chain(row_offsets, q_start, t_start, ksize, max_gap=0, min_kmers=1):
    """-> (row_offsets u64[n_rows + 1], q_start, t_start, length, n_kmers, covered u32[n_regions]); inside a row the regions are
    ordered by (q_start, t_start).  A region: pairs of one row on one diagonal d = t_start - q_start whose query starts, ascending,
    step by at most ksize + max_gap."""
    offs = np.asarray(row_offsets).astype(np.int64)
    n_rows = len(offs) - 1
    step = min(int(ksize) + int(max_gap), 2 ** 32 - 1)
    out_offs = np.zeros(n_rows + 1, np.uint64)
    cols = [[] for _ in range(5)]
    for r in range(n_rows):
        a = np.asarray(q_start[offs[r]:offs[r + 1]]).astype(np.int64)
        b = np.asarray(t_start[offs[r]:offs[r + 1]]).astype(np.int64)
        d = b - a
        o = np.lexsort((a, d))
        a, d = a[o], d[o]
        assert np.all((d[1:] != d[:-1]) | (a[1:] > a[:-1]))  # the pairs of a row are distinct
        da = a[1:] - a[:-1]
        head = np.concatenate([[True], (d[1:] != d[:-1]) | (da > step)]) if len(a) else np.zeros(0, bool)
        term = np.concatenate([[0], np.where(head[1:], 0, np.minimum(ksize, da))]) if len(a) else np.zeros(0, np.int64)
        h = np.flatnonzero(head)
        e = np.concatenate([h[1:], [len(a)]]) if len(h) else h
        csum = np.concatenate([[0], np.cumsum(term)])
        qs, ts, nk = a[h], a[h] + d[h], e - h
        length = a[e - 1] + ksize - qs
        covered = csum[e] - csum[h] + ksize
        keep = nk >= min_kmers
        row = [c[keep] for c in (qs, ts, length, nk, covered)]
        o = np.lexsort((row[1], row[0]))
        for c, v in zip(cols, row):
            c.append(v[o])
        out_offs[r + 1] = out_offs[r] + np.uint64(len(o))
    cat = lambda parts: np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return (out_offs, *[cat(c) for c in cols])


def as_tuples(regions, row):
    """The regions of one hit row as (q_start, t_start, length, n_kmers, covered) tuples."""
    s, e = int(regions[0][row]), int(regions[0][row + 1])
    return [tuple(int(c[g]) for c in regions[1:]) for g in range(s, e)]
