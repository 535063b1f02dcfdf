"""CPU restatement of ks_hits_best (include/kmerseek_amd.h): the score of a hit row per rank key, and which rows of every query
are kept with which rank.  Plain numpy, nothing from the library.

Order inside one query: row a beats row b iff score(a) > score(b), or the scores are equal and tid(a) < tid(b); -0.0 equals
+0.0, NaN compares below every number (-inf included) and NaNs are equal to each other.  rank = the rows of the same query
that beat the row; kept iff rank < k."""
import numpy as np

RANK_BY = ("intersect", "target_containment", "max_containment", "jaccard", "score")


def sizes(S):
    """distinct hashes per sketch of a host set (offsets, hashes, abunds)"""
    return np.diff(np.asarray(S[0], np.uint64)).astype(np.uint64)


def scores(rank_by, qid, tid, isect, Q=None, T=None, score=None):
    """f64 score per row, one rounding per operation (numpy's f64 division is correctly rounded, like the device's)"""
    qid = np.asarray(qid, np.int64); tid = np.asarray(tid, np.int64)
    i = np.asarray(isect, np.uint64)
    if rank_by == "intersect":
        return i.astype(np.float64)
    if rank_by == "score":
        s = np.asarray(score, np.float64)
        assert s.shape == qid.shape
        return s
    nt = sizes(T)[tid]
    if rank_by == "target_containment":
        assert np.all(nt > 0)
        return i.astype(np.float64) / nt.astype(np.float64)
    nq = sizes(Q)[qid]
    assert np.all(nt > 0) and np.all(nq > 0)
    if rank_by == "max_containment":
        return i.astype(np.float64) / np.minimum(nq, nt).astype(np.float64)
    if rank_by == "jaccard":
        return i.astype(np.float64) / (nq + nt - i).astype(np.float64)  # (the denominator in u64)
    raise ValueError(rank_by)


def best(qid, tid, score, k):
    """-> (kept bool mask, rank u32) per row; rows ordered by (qid, tid) or not, tids distinct inside a query"""
    qid = np.asarray(qid, np.int64); tid = np.asarray(tid, np.int64)
    s = np.asarray(score, np.float64)
    n = len(qid)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -(s + 0.0))  # (s + 0.0: -0.0 -> +0.0); ascending -score = descending score
    neg = neg + 0.0
    order = np.lexsort((tid, neg, nan, qid))  # per query: numbers before NaNs, score descending, tid ascending
    rank = np.zeros(n, np.int64)
    if n:
        q_sorted = qid[order]
        start = np.zeros(n, np.int64)
        heads = np.nonzero(np.concatenate(([True], q_sorted[1:] != q_sorted[:-1])))[0]
        start[heads] = heads
        start = np.maximum.accumulate(start)
        rank[order] = np.arange(n) - start
    return rank < int(k), rank.astype(np.uint32)


def best_rows(rank_by, qid, tid, isect, k, Q=None, T=None, score=None):
    """-> (src_row of the kept rows, ascending; their ranks)"""
    kept, rank = best(qid, tid, scores(rank_by, qid, tid, isect, Q, T, score), k)
    src = np.nonzero(kept)[0].astype(np.uint32)
    return src, rank[src]
