"""No GPU: the host restatement of ks_hits_cluster (tests/cluster_ref.py) on hand-written graphs, the graph sketch builder, the
text of wire.cluster_rows and the sizes histogram, and the option checks of ks_hits_cluster that need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref  # noqa: E402
import crafted_sketches as cs  # noqa: E402
import graph_sketches as gs  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(edges):
    """(qid, tid) with both directions of every edge, in (qid, tid) order"""
    e = sorted([(a, b) for a, b in edges] + [(b, a) for a, b in edges])
    return np.array([x for x, _ in e], np.int64), np.array([y for _, y in e], np.int64)


# ---- the reference union-find ------------------------------------------------------------------------------------------------
def test_triangle_plus_isolate():
    q, t = _both([(1, 2), (2, 4), (1, 4)])
    r = cluster_ref.cluster(5, q, t, np.ones(len(q)), 1.0)
    assert r["label"].tolist() == [0, 1, 1, 3, 1]
    assert r["cluster_id"].tolist() == [0, 1, 1, 2, 1]
    assert r["offsets"].tolist() == [0, 1, 4, 5] and r["members"].tolist() == [0, 1, 2, 4, 3]
    assert r["representative"].tolist() == [0, 1, 3]
    assert (r["n_nodes"], r["n_clusters"], r["n_edges"], r["largest"]) == (5, 3, 6, 3)
    # with node sizes: the member with the most hashes, ties to the smaller id
    r = cluster_ref.cluster(5, q, t, np.ones(len(q)), 1.0, node_sizes=[9, 2, 7, 0, 7])
    assert r["representative"].tolist() == [0, 2, 3]


def test_threshold_cuts_a_bridge():
    edges = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5)]
    q, t = _both(edges)
    score = np.where(((q == 2) & (t == 3)) | ((q == 3) & (t == 2)), 1.0, 3.0)
    one = cluster_ref.cluster(6, q, t, score, 1.0)
    assert one["n_clusters"] == 1 and one["label"].tolist() == [0] * 6 and one["largest"] == 6 and one["n_edges"] == 14
    two = cluster_ref.cluster(6, q, t, score, 2.0)
    assert two["label"].tolist() == [0, 0, 0, 3, 3, 3] and two["offsets"].tolist() == [0, 3, 6] and two["n_edges"] == 12
    none = cluster_ref.cluster(6, q, t, score, 3.5)
    assert none["n_clusters"] == 6 and none["n_edges"] == 0 and none["largest"] == 1
    assert none["members"].tolist() == list(range(6)) and none["representative"].tolist() == list(range(6))


def test_one_directional_row_still_joins():
    # (3, 1) alone, no (1, 3); a self row counts as an edge row but joins nothing; NaN never passes, -0.0 equals 0.0
    q, t = np.array([0, 2, 3, 4]), np.array([0, 4, 1, 2])
    score = np.array([5.0, np.nan, -0.0, -np.inf])
    r = cluster_ref.cluster(5, q, t, score, 0.0)
    assert r["label"].tolist() == [0, 1, 2, 1, 4] and r["n_edges"] == 2
    r = cluster_ref.cluster(5, q, t, score, -np.inf)
    assert r["label"].tolist() == [0, 1, 2, 1, 2] and r["n_edges"] == 3
    with pytest.raises(AssertionError):
        cluster_ref.cluster(5, q, t, score, np.nan)
    assert cluster_ref.cluster(3, [], [], [], 0.0)["label"].tolist() == [0, 1, 2]


def test_reference_uses_the_best_hits_scores():
    S, rows = gs.build(4, [(0, 1, 2), (1, 2, 1)])
    # sizes: |0| = 1 + 2, |1| = 2 + 3, |2| = 3 + 1, |3| = 1
    assert np.diff(S[0]).tolist() == [3, 5, 4, 1]
    assert list(zip(*[r.tolist() for r in rows])) == [(0, 0, 3), (0, 1, 2), (1, 0, 2), (1, 1, 5), (1, 2, 1), (2, 1, 1), (2, 2, 4), (3, 3, 1)]
    j = cluster_ref.scores("jaccard", *rows, S, S)
    assert j.tolist() == [1.0, 2 / 6, 2 / 6, 1.0, 1 / 8, 1 / 8, 1.0, 1.0]
    r = cluster_ref.cluster_hits("jaccard", 4, *rows, 0.2, S)
    assert r["label"].tolist() == [0, 0, 2, 3] and r["representative"].tolist() == [1, 2, 3] and r["n_edges"] == 6
    # target containment is one-directional: (2, 1) = 1 / 5 fails, (1, 2) = 1 / 4 passes, and the pair is joined
    r = cluster_ref.cluster_hits("target_containment", 4, *rows, 0.25, S)
    assert r["label"].tolist() == [0, 0, 0, 3]


# ---- the graph sketch builder ------------------------------------------------------------------------------------------------
def test_graph_sketches_realise_their_rows():
    n = 300
    edges = gs.random_graph(n - 1, 200, seed=5)
    lonely = sorted(set(range(n - 1)) - set(edges[:, :2].ravel().tolist()))
    S, rows = gs.build(n, edges, empty=[lonely[3], n - 1], extra={7: 40})
    assert np.diff(S[0])[[lonely[3], n - 1]].tolist() == [0, 0] and len(rows[0]) == 2 * 200 + n - 2
    got = cs.ref_join(S, S)
    for g, w in zip(got[:3], rows):
        assert np.array_equal(g, w)
    for e, kind in ((gs.chain(50, np.random.default_rng(1).permutation(50)), "chain"), (gs.star(20, 20), "star"), (gs.cliques_with_bridge(5), "bridge")):
        m = int(e[:, :2].max()) + 1
        S, rows = gs.build(m + 2, e, empty=[m])
        got = cs.ref_join(S, S)
        for g, w in zip(got[:3], rows):
            assert np.array_equal(g, w), kind
        assert not np.any(rows[0] == m) and np.any(rows[0] == m + 1)


# ---- wire ----------------------------------------------------------------------------------------------------------------------
def test_cluster_rows_and_sizes_histogram():
    names = ["a b", "c", "d", "e", "f"]
    q, t = _both([(1, 2), (2, 4)])
    r = cluster_ref.cluster(5, q, t, np.ones(len(q)), 1.0, node_sizes=[1, 1, 3, 1, 2])
    rows = wire.cluster_rows(names, r["offsets"], r["members"], r["representative"])
    assert rows == [("Component_0", "a b", 1, "a b"), ("Component_1", "d", 3, "c;d;f"), ("Component_2", "e", 1, "e")]
    assert wire.cluster_size_histogram(r["offsets"]) == [(1, 2), (3, 1)]
    assert wire.CLUSTER_COLUMNS == ["cluster", "representative", "size", "nodes"]
    assert "no parity" in wire.do_cluster.__doc__


# ---- the option checks need no device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def test_cluster_opts_layout_matches_header():
    assert C.sizeof(_lib.ks_cluster_opts) == 24
    o = _lib.ks_cluster_opts
    assert [(getattr(o, f).offset, getattr(o, f).size) for f, _ in o._fields_] == [(0, 4), (4, 4), (8, 8), (16, 4), (20, 4)]
    text = open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read()
    body = re.search(r"typedef struct ks_cluster_opts \{(.*?)\} ks_cluster_opts;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|double)\s+(\w+);", body)
    ctype = {"uint32_t": C.c_uint32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(o._fields_)


def test_bad_options_are_refused_without_a_context(lib):
    J, S, I = _lib.KS_BEST_JACCARD, _lib.KS_BEST_SCORE, _lib.KS_BEST_INTERSECT
    column = C.c_void_p(8)  # never read: the options are refused first
    bad = [
        ((5, 3, 0.0, 0, 0), None),          # unknown similarity
        ((I, 3, 0.0, 1, 0), None),          # flags
        ((I, 3, 0.0, 0, 1), None),          # reserved
        ((I, 3, float("nan"), 0, 0), None),  # NaN threshold
        ((S, 3, 0.0, 0, 0), None),          # KS_BEST_SCORE without a column
        ((I, 3, 0.0, 0, 0), column),        # a column without KS_BEST_SCORE
        ((J, 3, 0.0, 0, 0), None),          # a key that needs sizes, no node set
        ((_lib.KS_BEST_TARGET_CONTAINMENT, 3, 0.0, 0, 0), None),
        ((_lib.KS_BEST_MAX_CONTAINMENT, 3, 0.0, 0, 0), None),
    ]
    for words, col in bad:
        out = C.c_void_p(1)
        st = lib.ks_hits_cluster(None, None, None, col, C.byref(_lib.ks_cluster_opts(*words)), C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG, words
        assert not out.value
    out = C.c_void_p(1)
    assert lib.ks_hits_cluster(None, None, None, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
    # good options and no context: still an error, and nothing is made
    assert lib.ks_hits_cluster(None, None, None, None, C.byref(_lib.ks_cluster_opts(I, 3, 0.0, 0, 0)), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    # the accessors of no object
    assert lib.ks_clusters_n_nodes(None) == 0 and lib.ks_clusters_n_edges(None) == 0 and not lib.ks_clusters_device_label(None)
    lib.ks_clusters_free(None)
