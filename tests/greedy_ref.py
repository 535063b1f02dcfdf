"""CPU restatement of ks_hits_cluster_greedy (include/kmerseek_amd.h): greedy representative clustering of a hit list read as a
graph.  Plain numpy / Python, nothing from the library: the sequential definition, a loop over the nodes in priority order with
an adjacency list.  The scores are those of tests/best_ref.py (ks_hits_best's, bit for bit).

Row r = (q, t) is an undirected edge iff q != t and score(r) >= threshold (a NaN score never is).  Priority: with node sizes
more distinct hashes first, ties to the smaller id; without them the smaller id first.  In that order a node becomes a
representative iff none of its neighbours of higher priority is one.  Every other node joins a neighbouring representative:
assign "first" the one of highest priority, "best" the one at the other end of the passing row with the largest score (rows
(v, u) and (u, v) are each a candidate; ties to the higher priority).  label = the representative's id, clusters numbered by
ascending representative, the CSR with ascending members; n_edges counts the rows that passed, self rows and both directions
included."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from best_ref import scores  # noqa: E402,F401  (re-exported: the tests compute the score column with it)

ASSIGN = ("first", "best")


def priority(n, node_sizes=None):
    """-> (order, rank): order[k] = the node of rank k, rank[v] = its place; rank 0 is the highest priority"""
    ids = np.arange(n, dtype=np.int64)
    if node_sizes is None:
        return ids, ids.copy()
    w = np.minimum(np.asarray(node_sizes, np.uint64), np.uint64(0xffffffff)).astype(np.int64)
    assert len(w) == n
    order = np.lexsort((ids, -w))
    rank = np.zeros(n, np.int64)
    rank[order] = ids
    return order, rank


def _passing(qid, tid, score, threshold):
    qid = np.asarray(qid, np.int64); tid = np.asarray(tid, np.int64)
    s = np.asarray(score, np.float64)
    assert qid.shape == tid.shape == s.shape
    assert not np.isnan(threshold)
    with np.errstate(invalid="ignore"):
        passed = s >= float(threshold)  # (NaN >= x is False; -0.0 >= 0.0 is True; -inf >= -inf is True)
    return qid, tid, s, passed


def cluster(n, qid, tid, score, threshold, node_sizes=None, assign="first"):
    """-> dict(label, cluster_id u32[n], offsets u64[n_clusters + 1], members u32[n], representative u32[n_clusters],
    n_nodes, n_clusters, n_edges, largest)"""
    assert assign in ASSIGN
    qid, tid, s, passed = _passing(qid, tid, score, threshold)
    assert len(qid) == 0 or (qid.min() >= 0 and tid.min() >= 0 and qid.max() < n and tid.max() < n)
    order, rank = priority(n, node_sizes)
    rank_l = rank.tolist()
    adj = [[] for _ in range(n)]  # per node (neighbour, score of the row): one entry per passing non-self row it is an end of
    for a, b, x in zip(qid[passed].tolist(), tid[passed].tolist(), s[passed].tolist()):
        if a != b:
            adj[a].append((b, x))
            adj[b].append((a, x))
    is_rep = [False] * n
    for v in order.tolist():
        is_rep[v] = not any(is_rep[u] for u, _ in adj[v] if rank_l[u] < rank_l[v])
    label = np.arange(n, dtype=np.uint32)
    for v in range(n):
        if is_rep[v]:
            continue
        cand = [(u, x) for u, x in adj[v] if is_rep[u]]
        assert cand, "a node that is no representative has one among its neighbours"
        if assign == "first":
            label[v] = min(cand, key=lambda c: rank_l[c[0]])[0]
        else:
            top = max(x for _, x in cand)  # (-0.0 == 0.0: both are the maximum then)
            label[v] = min((c for c in cand if c[1] == top), key=lambda c: rank_l[c[0]])[0]
    roots = np.nonzero(label == np.arange(n, dtype=np.uint32))[0]
    index_of = np.zeros(n, np.int64)
    index_of[roots] = np.arange(len(roots))
    cluster_id = index_of[label.astype(np.int64)].astype(np.uint32)
    members = np.lexsort((np.arange(n), cluster_id)).astype(np.uint32)
    sizes = np.bincount(cluster_id, minlength=len(roots)).astype(np.uint64)
    offsets = np.zeros(len(roots) + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes)
    return dict(label=label, cluster_id=cluster_id, offsets=offsets, members=members, representative=roots.astype(np.uint32), n_nodes=n,
                n_clusters=len(roots), n_edges=int(np.count_nonzero(passed)), largest=int(sizes.max()) if n else 0)


def cluster_hits(similarity, n, qid, tid, isect, threshold, S=None, score=None, assign="first"):
    """the same from host hit rows and a host sketch set S = (offsets, hashes, abunds) (None: no node set)"""
    sc = scores(similarity, qid, tid, isect, S, S, score)
    return cluster(n, qid, tid, sc, threshold, None if S is None else np.diff(np.asarray(S[0], np.uint64)), assign)


def check_invariants(label, n, qid, tid, score, threshold, node_sizes=None, assign="first"):
    """What a user relies on, checked on labels from anywhere: every member has a passing row with its representative, no
    passing row joins two representatives, and — under assign "first" — a representative has the highest priority of its
    cluster.  ("best" may send a node to a representative of lower priority than its own: the row with the better score.  The
    node is no representative because another neighbour, of higher priority, is one.)"""
    qid, tid, s, passed = _passing(qid, tid, score, threshold)
    label = np.asarray(label).astype(np.int64)
    assert label.shape == (n,)
    is_rep = label == np.arange(n)
    assert np.all(is_rep[label]), "a label that is no representative"
    q, t = qid[passed], tid[passed]
    off = q != t
    q, t = q[off], t[off]
    assert not np.any(is_rep[q] & is_rep[t]), "a passing row joins two representatives"
    linked = set((q * n + t).tolist()) | set((t * n + q).tolist())
    m = np.nonzero(~is_rep)[0]
    assert all(k in linked for k in (m * n + label[m]).tolist()), "a member without a passing row to its representative"
    if assign == "first":
        _, rank = priority(n, node_sizes)
        assert np.all(rank[label] <= rank), "a member of higher priority than its representative"
