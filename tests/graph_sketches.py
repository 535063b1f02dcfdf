"""Sketch sets that realise a given weighted graph, for the tests of ks_hits_cluster.

build(n, edges) makes a valid input of ks_sketches_from_host (crafted_sketches._csr / check_valid) in which
  * node i holds 1 + i % 3 private hashes (+ extra[i] more on request; none at all for the nodes listed in `empty`),
  * edge (a, b, w) is w hashes that only a and b hold.
The search of the set against itself then has exactly the rows (a, b, w) and (b, a, w) for every edge and (a, a, |a|) for every
non-empty node, in (qid, tid) order: rows() returns them, and every GPU test compares the searched rows with them first, so
that what it then tests is the cluster pass.  No GPU is needed here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402

U64_MAX = (1 << 64) - 1


def _edges(edges):
    e = np.asarray(edges, np.int64).reshape(-1, 3)
    return e[:, 0], e[:, 1], e[:, 2]


def build(n, edges, empty=(), extra=None):
    """-> (S = (offsets u64, hashes u64, abunds u32), rows = (qid u32, tid u32, intersect u32))"""
    a, b, w = _edges(edges)
    assert n >= 1 and np.all(a != b) and np.all(w >= 1)
    assert len(a) == 0 or (min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < n)
    pair = np.minimum(a, b) * n + np.maximum(a, b)
    assert len(np.unique(pair)) == len(pair), "an edge is listed twice"
    empty = np.asarray(sorted(empty), np.int64)
    assert not np.isin(a, empty).any() and not np.isin(b, empty).any(), "an empty node has no edge"
    priv = 1 + np.arange(n, dtype=np.int64) % 3
    if extra:
        for i, x in extra.items():
            priv[i] += x
    priv[empty] = 0
    # the hashes are evenly spaced over (0, 2^64): the private ones first, node by node, then w per edge, each held by both
    # ends (consecutive integers would all fall into one join bucket of the search)
    p_seq = np.repeat(np.arange(n, dtype=np.int64), priv)
    e_of = np.repeat(np.arange(len(a), dtype=np.int64), w)
    total = len(p_seq) + len(e_of)
    spaced = (1 + np.arange(total, dtype=np.uint64)) * np.uint64(U64_MAX // (total + 1))
    p_hash, e_hash = spaced[:len(p_seq)], spaced[len(p_seq):]
    seq = np.concatenate([p_seq, a[e_of], b[e_of]])
    h = np.concatenate([p_hash, e_hash, e_hash])
    S = cs._csr(seq, h, np.ones(len(h), np.uint32), n)
    cs.check_valid(S, 1)
    size = priv.copy()
    np.add.at(size, a, w)
    np.add.at(size, b, w)
    assert np.array_equal(np.diff(S[0]).astype(np.int64), size)
    live = np.nonzero(size > 0)[0]
    q = np.concatenate([a, b, live]); t = np.concatenate([b, a, live]); i = np.concatenate([w, w, size[live]])
    o = np.lexsort((t, q))
    return S, (q[o].astype(np.uint32), t[o].astype(np.uint32), i[o].astype(np.uint32))


def chain(n, perm=None):
    """edges i - i + 1 of weight 1 + i % 2; perm: a permutation of the ids (node i becomes perm[i])"""
    i = np.arange(n - 1, dtype=np.int64)
    a, b = i, i + 1
    if perm is not None:
        perm = np.asarray(perm, np.int64)
        a, b = perm[a], perm[b]
    return np.stack([a, b, 1 + i % 2], axis=1)


def star(n_leaves, hub):
    """hub - every other node of 0 .. n_leaves, weight 1"""
    leaves = np.array([i for i in range(n_leaves + 1) if i != hub], np.int64)
    return np.stack([np.full(n_leaves, hub, np.int64), leaves, np.ones(n_leaves, np.int64)], axis=1)


def cliques_with_bridge(m, w_in=3, w_bridge=1):
    """two m-node cliques (nodes 0 .. m-1 and m .. 2m-1) of weight w_in, joined by the edge (m - 1, m) of weight w_bridge"""
    e = [(i, j, w_in) for base in (0, m) for i in range(base, base + m) for j in range(i + 1, base + m)]
    return np.array(e + [(m - 1, m, w_bridge)], np.int64)


def random_graph(n, n_edges, seed, w_max=3):
    """n_edges distinct random pairs, weights 1 .. w_max"""
    rng = np.random.default_rng(seed)
    pairs = np.zeros(0, np.int64)
    while len(pairs) < n_edges:
        a = rng.integers(0, n, 2 * n_edges); b = rng.integers(0, n, 2 * n_edges)
        ok = a != b
        key = np.minimum(a, b)[ok] * n + np.maximum(a, b)[ok]
        seen = np.concatenate([pairs, key])
        _, first = np.unique(seen, return_index=True)
        pairs = seen[np.sort(first)][:n_edges]
    return np.stack([pairs // n, pairs % n, rng.integers(1, w_max + 1, n_edges)], axis=1)
