"""Plain Python / numpy restatement of the significance columns (include/kmerseek_amd.h: ks_corpus_build,
ks_hits_significance) — what the device is held to, bit for bit.

A sketch set is (offsets u64[n + 1], mins u64, abunds u32), a plain CSR.  Everything that is rounded is a Python float (an IEEE
double; one rounding per operation, nothing contracted), added sequentially in ascending hash order; integers become floats
BEFORE they are divided (`float(a) / float(b)`: Python's int / int rounds the exact quotient, which is another number once an
operand passes 2^53); the logarithm is math.log — libm's, where numpy's vectorised log need not agree in the last bit."""
import math

import numpy as np


def corpus(S):
    """-> (hashes u64 ascending, abund_sum u64, doc_freq u32, total int): the corpus table of the set"""
    _, mins, abunds = S
    hashes, inv = np.unique(np.asarray(mins, np.uint64), return_inverse=True)
    sums = np.zeros(len(hashes), np.uint64)
    np.add.at(sums, inv, np.asarray(abunds).astype(np.uint64))
    df = np.bincount(inv, minlength=len(hashes)).astype(np.uint32)
    return hashes, sums, df, sum(int(a) for a in np.asarray(abunds).tolist())


def idf_table(n_targets, max_doc_freq):
    return [math.log((1.0 + float(n_targets)) / (1.0 + float(d))) + 1.0 for d in range(max_doc_freq + 1)]


def join(Q, T, min_containment=0.0):
    """Hit rows (qid u32, tid u32, intersect u32) in (qid, tid) order, for sets small enough for a dict of postings; rows with
    (double)intersect / (double)|q| below min_containment are dropped."""
    qo, qm, _ = Q
    to, tm, _ = T
    holders = {}
    for t in range(len(to) - 1):
        for h in tm[int(to[t]):int(to[t + 1])].tolist():
            holders.setdefault(h, []).append(t)
    qid, tid, isect = [], [], []
    for q in range(len(qo) - 1):
        count = {}
        hs = qm[int(qo[q]):int(qo[q + 1])].tolist()
        for h in hs:
            for t in holders.get(h, ()):
                count[t] = count.get(t, 0) + 1
        for t in sorted(count):
            if float(count[t]) / float(len(hs)) >= min_containment:
                qid.append(q); tid.append(t); isect.append(count[t])
    return np.array(qid, np.uint32), np.array(tid, np.uint32), np.array(isect, np.uint32)


def significance(Q, T, qid, tid, q_corpus=None, t_corpus=None):
    """-> (prob_overlap f64, tf_idf f64, shared counts) per hit row (qid[r], tid[r])"""
    qo, qm, qa = Q
    to, tm, _ = T
    cq = q_corpus or corpus(Q)
    ct = t_corpus or corpus(T)
    sum_q = dict(zip(cq[0].tolist(), cq[1].tolist()))
    sum_t = dict(zip(ct[0].tolist(), ct[1].tolist()))
    df_t = dict(zip(ct[0].tolist(), ct[2].tolist()))
    tot_q, tot_t = float(cq[3]), float(ct[3])
    idf = idf_table(len(to) - 1, int(ct[2].max()) if len(ct[2]) else 0)
    po, tf, shared = [], [], []
    cache, t_sets = {}, {}
    for q, t in zip(np.asarray(qid).tolist(), np.asarray(tid).tolist()):
        if q not in cache:
            cache.clear()  # (rows are ordered by query)
            hs = qm[int(qo[q]):int(qo[q + 1])].tolist()
            ab = qa[int(qo[q]):int(qo[q + 1])].tolist()
            cache[q] = (hs, ab, float(sum(ab)))
        hs, ab, q_sum = cache[q]
        if t not in t_sets:
            t_sets[t] = frozenset(tm[int(to[t]):int(to[t + 1])].tolist())
        th = t_sets[t]
        p, f, n = 0.0, 0.0, 0
        for h, a in zip(hs, ab):  # ascending: a sketch is sorted
            if h in th:
                p += (float(sum_q[h]) / tot_q) * (float(sum_t[h]) / tot_t)
                f += (float(a) / q_sum) * idf[df_t[h]]
                n += 1
        po.append(p); tf.append(f); shared.append(n)
    return np.array(po, np.float64), np.array(tf, np.float64), np.array(shared, np.uint32)


def derived(prob_overlap, intersect, q_size, n_queries, n_targets):
    """(prob_overlap_adjusted, containment_adjusted, containment_adjusted_log10) of one row"""
    adj = prob_overlap * float(n_queries * n_targets)
    c_adj = (float(intersect) / float(q_size)) / adj
    return adj, c_adj, math.log10(c_adj)
