"""CPU restatement of ks_hits_cluster (include/kmerseek_amd.h): the connected components of a hit list read as a graph.
Plain numpy / Python, nothing from the library.  The scores are those of tests/best_ref.py (ks_hits_best's, bit for bit).

Row r = (q, t) is an undirected edge iff q != t and score(r) >= threshold (a NaN score never is).  Per node its label (the
smallest id of its cluster) and cluster_id (clusters numbered by ascending smallest member); the clusters as a CSR (offsets,
members ascending); per cluster a representative: with node sizes the member with the most distinct hashes, ties to the
smaller id, without them the smallest member.  n_edges counts the rows that passed, self rows and both directions included."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from best_ref import scores  # noqa: E402,F401  (re-exported: the tests compute the score column with it)


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:  # full compression: the host has no reason to be clever
        parent[x], x = root, parent[x]
    return root


def cluster(n, qid, tid, score, threshold, node_sizes=None):
    """-> dict(label, cluster_id u32[n], offsets u64[n_clusters + 1], members u32[n], representative u32[n_clusters],
    n_nodes, n_clusters, n_edges, largest)"""
    qid = np.asarray(qid, np.int64); tid = np.asarray(tid, np.int64)
    s = np.asarray(score, np.float64)
    assert qid.shape == tid.shape == s.shape
    assert not np.isnan(threshold)
    assert len(qid) == 0 or (qid.min() >= 0 and tid.min() >= 0 and qid.max() < n and tid.max() < n)
    with np.errstate(invalid="ignore"):
        passed = s >= float(threshold)  # (NaN >= x is False; -0.0 >= 0.0 is True; -inf >= -inf is True)
    parent = list(range(n))
    for a, b in zip(qid[passed].tolist(), tid[passed].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)  # the root of a tree is its smallest id
    label = np.array([_find(parent, i) for i in range(n)], np.uint32) if n else np.zeros(0, np.uint32)
    roots = np.nonzero(label == np.arange(n, dtype=np.uint32))[0]
    index_of = np.zeros(n, np.int64)
    index_of[roots] = np.arange(len(roots))
    cluster_id = index_of[label.astype(np.int64)].astype(np.uint32)
    order = np.lexsort((np.arange(n), cluster_id))
    members = order.astype(np.uint32)
    sizes = np.bincount(cluster_id, minlength=len(roots)).astype(np.uint64)
    offsets = np.zeros(len(roots) + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes)
    rep = np.zeros(len(roots), np.uint32)
    for c in range(len(roots)):
        ids = members[int(offsets[c]):int(offsets[c + 1])]
        if node_sizes is None:
            rep[c] = ids[0]
        else:
            w = np.asarray(node_sizes, np.uint64)[ids.astype(np.int64)]
            rep[c] = ids[int(np.argmax(w))]  # (argmax: the first of the largest = the smaller id)
    return dict(label=label, cluster_id=cluster_id, offsets=offsets, members=members, representative=rep, n_nodes=n,
                n_clusters=len(roots), n_edges=int(np.count_nonzero(passed)), largest=int(sizes.max()) if n else 0)


def cluster_hits(similarity, n, qid, tid, isect, threshold, S=None, score=None):
    """the same from host hit rows and a host sketch set S = (offsets, hashes, abunds) (None: no node set)"""
    sc = scores(similarity, qid, tid, isect, S, S, score)
    return cluster(n, qid, tid, sc, threshold, None if S is None else np.diff(np.asarray(S[0], np.uint64)))
