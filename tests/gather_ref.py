"""CPU restatement of ks_hits_gather (include/kmerseek_amd.h): per query the greedy non-redundant targets of a hit list.

Plain numpy / Python on host CSRs and host hit rows; nothing from the library.  For every query q with rows, R_0 = the hashes
of q; round i: every row r of q not yet picked counts c_i(r) = |R_i and hashes(tid(r))|; the row with the largest count wins,
ties to the smaller tid (the earlier row); the query stops when that count is below max(min_unique, 1), when i == max_results
!= 0, or when no row is left; otherwise the winner is kept with rank i, unique_intersect c_i, unique_weighted = the sum of q's
abundances over the newly covered hashes, R_(i+1) = R_i without them, remaining = |R_(i+1)|.

gather() works on boolean masks over q's positions (searchsorted); gather_sets() is a second, independent version on Python
sets, for the tests to hold the first against."""
import numpy as np


def _seq(S, i):
    return S[1][int(S[0][i]):int(S[0][i + 1])]


def _segments(qid):
    """[(first row, one past the last row)] of every run of equal qid"""
    qid = np.asarray(qid)
    if len(qid) == 0:
        return []
    cuts = np.concatenate([[0], np.nonzero(qid[1:] != qid[:-1])[0] + 1, [len(qid)]])
    return list(zip(cuts[:-1].tolist(), cuts[1:].tolist()))


def _result(src, rank, uniq, rem, uw):
    o = np.argsort(np.asarray(src, np.int64), kind="stable")
    return (np.asarray(src, np.uint32)[o], np.asarray(rank, np.uint32)[o], np.asarray(uniq, np.uint32)[o],
            np.asarray(rem, np.uint32)[o], np.array([int(x) for x in uw], np.uint64)[o])


def gather(Q, T, qid, tid, isect, min_unique=1, max_results=0):
    """-> (src_row u32, rank u32, unique_intersect u32, remaining u32, unique_weighted u64) of the kept rows, in row order —
    (qid, tid) order.  Q, T: (offsets u64, hashes u64, abundances u32).  A row whose round-0 count is not its `intersect` is
    an assertion: hits and sketches do not belong together."""
    need = max(int(min_unique), 1)
    src, rank, uniq, rem, uw = [], [], [], [], []
    for b, e in _segments(qid):
        q = int(qid[b])
        qh = _seq(Q, q)
        qa = Q[2][int(Q[0][q]):int(Q[0][q + 1])].astype(np.uint64)
        lists = []
        for r in range(b, e):
            th = _seq(T, int(tid[r]))
            at = np.searchsorted(qh, th)
            ok = at < len(qh)
            ok[ok] = qh[at[ok]] == th[ok]
            pos = at[ok]
            assert len(pos) == int(isect[r]), (r, len(pos), int(isect[r]))
            lists.append(pos)
        live = np.ones(len(qh), bool)
        picked = [False] * (e - b)
        i = 0
        while True:
            if max_results and i == max_results:
                break
            best, best_c = -1, 0
            for j, pos in enumerate(lists):
                if picked[j]:
                    continue
                c = int(np.count_nonzero(live[pos]))
                if c > best_c:  # (strictly: the earlier row keeps a tie)
                    best, best_c = j, c
            if best < 0 or best_c < need:
                break
            new = lists[best][live[lists[best]]]
            live[new] = False
            picked[best] = True
            src.append(b + best); rank.append(i); uniq.append(best_c); rem.append(int(np.count_nonzero(live)))
            uw.append(sum(int(x) for x in qa[new]))  # (Python integers: no wrap)
            i += 1
    return _result(src, rank, uniq, rem, uw)


def gather_sets(Q, T, qid, tid, isect, min_unique=1, max_results=0):
    """the same through Python sets and dicts, every row recounted in every round"""
    need = max(int(min_unique), 1)
    src, rank, uniq, rem, uw = [], [], [], [], []
    rows_of = {}
    for r, q in enumerate(np.asarray(qid).tolist()):
        rows_of.setdefault(q, []).append(r)
    for q in sorted(rows_of):
        ab = dict(zip(_seq(Q, q).tolist(), Q[2][int(Q[0][q]):int(Q[0][q + 1])].tolist()))
        R = set(ab)
        left = {r: set(_seq(T, int(tid[r])).tolist()) for r in rows_of[q]}
        i = 0
        while left and not (max_results and i == max_results):
            counts = {r: len(R & t) for r, t in left.items()}
            top = max(counts.values())
            if top < need:
                break
            r = min(r for r, c in counts.items() if c == top)  # rows of a query ascend with tid
            new = R & left.pop(r)
            R -= new
            src.append(r); rank.append(i); uniq.append(top); rem.append(len(R)); uw.append(sum(ab[h] for h in new))
            i += 1
    return _result(src, rank, uniq, rem, uw)
