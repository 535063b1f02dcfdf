"""No GPU: the host restatement of ks_hits_cluster_greedy (tests/greedy_ref.py) on hand-written graphs whose answers are written
out here, its three invariants on random graphs, every greedy cluster inside one connected component (tests/cluster_ref.py),
the text of wire.cluster_rows for a greedy result, and the struct layout and the option checks of ks_hits_cluster_greedy that
need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref  # noqa: E402
import graph_sketches as gs  # noqa: E402
import greedy_ref  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(edges):
    """(qid, tid) with both directions of every edge, in (qid, tid) order"""
    e = sorted([(a, b) for a, b in edges] + [(b, a) for a, b in edges])
    return np.array([x for x, _ in e], np.int64), np.array([y for _, y in e], np.int64)


# ---- the sequential definition on graphs small enough to do by hand ----------------------------------------------------------
def test_path_in_id_order():
    q, t = _both([(0, 1), (1, 2), (2, 3), (3, 4)])
    r = greedy_ref.cluster(5, q, t, np.ones(len(q)), 1.0)
    # 0 is a representative, 1 joins it, so 2 is free to be one, 3 joins it, 4 is one
    assert r["label"].tolist() == [0, 0, 2, 2, 4]
    assert r["cluster_id"].tolist() == [0, 0, 1, 1, 2]
    assert r["offsets"].tolist() == [0, 2, 4, 5] and r["members"].tolist() == [0, 1, 2, 3, 4]
    assert r["representative"].tolist() == [0, 2, 4]
    assert (r["n_nodes"], r["n_clusters"], r["n_edges"], r["largest"]) == (5, 3, 8, 2)
    # the connected components make one cluster of it
    assert cluster_ref.cluster(5, q, t, np.ones(len(q)), 1.0)["n_clusters"] == 1


def test_first_and_best_differ_on_the_better_row():
    q, t = _both([(0, 1), (1, 2), (2, 3), (3, 4)])
    score = np.where((q == 1) & (t == 2), 5.0, 1.0)  # the row (1, 2) alone; (2, 1) scores 1 like the rest
    first = greedy_ref.cluster(5, q, t, score, 1.0, assign="first")
    assert first["label"].tolist() == [0, 0, 2, 2, 4]
    best = greedy_ref.cluster(5, q, t, score, 1.0, assign="best")
    # 1 has rows of score 1 with 0 and a row of score 5 with 2; 3 ties between 2 and 4: the higher priority
    assert best["label"].tolist() == [0, 2, 2, 2, 4]
    assert best["offsets"].tolist() == [0, 1, 4, 5] and best["members"].tolist() == [0, 1, 2, 3, 4]
    assert best["representative"].tolist() == [0, 2, 4] and best["largest"] == 3
    # the representatives never depend on the assignment
    assert np.array_equal(first["representative"], best["representative"])


def test_sizes_set_the_priority_and_ties_go_to_the_smaller_id():
    q, t = _both([(0, 1), (1, 2), (2, 3), (3, 4)])
    one = np.ones(len(q))
    # 3 is the largest: a representative; 2 and 4 join it; 0 and 1 tie in size, 0 first: a representative, 1 joins it
    r = greedy_ref.cluster(5, q, t, one, 1.0, node_sizes=[2, 2, 5, 9, 1])
    assert r["label"].tolist() == [0, 0, 3, 3, 3] and r["representative"].tolist() == [0, 3]
    # 1 larger than 0: now 1 is the representative, and 2 could join 1 or 3: the higher priority (first), here 3
    r = greedy_ref.cluster(5, q, t, one, 1.0, node_sizes=[2, 3, 5, 9, 1])
    assert r["label"].tolist() == [1, 1, 3, 3, 3] and r["representative"].tolist() == [1, 3]
    assert r["cluster_id"].tolist() == [0, 0, 1, 1, 1] and r["offsets"].tolist() == [0, 2, 5]
    order, rank = greedy_ref.priority(5, [2, 2, 5, 9, 1])
    assert order.tolist() == [3, 2, 0, 1, 4] and rank.tolist() == [2, 3, 1, 0, 4]


def test_star_by_id_and_by_size():
    n = 7
    e = [(6, i) for i in range(6)]  # the hub is the last id
    q, t = _both(e)
    by_id = greedy_ref.cluster(n, q, t, np.ones(len(q)), 1.0)
    # 0 is a representative and takes the hub; the other leaves have no neighbour left: singletons
    assert by_id["label"].tolist() == [0, 1, 2, 3, 4, 5, 0] and by_id["n_clusters"] == 6 and by_id["largest"] == 2
    by_size = greedy_ref.cluster(n, q, t, np.ones(len(q)), 1.0, node_sizes=[1, 1, 1, 1, 1, 1, 6])
    assert by_size["label"].tolist() == [6] * 7 and by_size["n_clusters"] == 1 and by_size["representative"].tolist() == [6]
    assert by_size["members"].tolist() == list(range(7))


def test_one_direction_nan_and_signed_zero():
    # (3, 1) alone, no (1, 3); a self row counts as a passing row but is no edge; NaN never passes, -0.0 equals 0.0
    q, t = np.array([0, 2, 3, 4]), np.array([0, 4, 1, 2])
    score = np.array([5.0, np.nan, -0.0, -np.inf])
    r = greedy_ref.cluster(5, q, t, score, 0.0)
    assert r["label"].tolist() == [0, 1, 2, 1, 4] and r["n_edges"] == 2
    r = greedy_ref.cluster(5, q, t, score, -np.inf)
    assert r["label"].tolist() == [0, 1, 2, 1, 2] and r["n_edges"] == 3
    with pytest.raises(AssertionError):
        greedy_ref.cluster(5, q, t, score, np.nan)
    assert greedy_ref.cluster(3, [], [], [], 0.0)["label"].tolist() == [0, 1, 2]
    # best: the two rows of one pair are candidates of their own, +0.0 and -0.0 tie
    q, t = np.array([0, 2, 2, 1]), np.array([2, 0, 1, 2])
    r = greedy_ref.cluster(3, q, t, np.array([0.0, 7.0, -0.0, 0.0]), 0.0, node_sizes=[5, 5, 1], assign="best")
    assert r["label"].tolist() == [0, 1, 0]  # (2, 0) = 7 beats everything
    r = greedy_ref.cluster(3, q, t, np.array([0.0, -0.0, -0.0, 0.0]), 0.0, node_sizes=[5, 5, 1], assign="best")
    assert r["label"].tolist() == [0, 1, 0]  # all zeros tie: the higher priority
    r = greedy_ref.cluster(3, q, t, np.array([0.0, -0.0, 1e-300, 0.0]), 0.0, node_sizes=[5, 5, 1], assign="best")
    assert r["label"].tolist() == [0, 1, 1]


def test_bridge_gives_two_clusters_where_the_components_give_one():
    e = gs.cliques_with_bridge(40)
    S, rows = gs.build(80, e)
    sizes = np.diff(S[0]).astype(np.int64)
    assert sizes.max() == 120 and np.nonzero(sizes == 120)[0][:2].tolist() == [2, 5] and sizes[39] == 119 and sizes[40] == 120
    r = greedy_ref.cluster_hits("intersect", 80, *rows, 1.0, S)
    assert r["n_clusters"] == 2 and r["representative"].tolist() == [2, 40]
    assert r["label"].tolist() == [2] * 40 + [40] * 40 and r["offsets"].tolist() == [0, 40, 80]
    assert cluster_ref.cluster_hits("intersect", 80, *rows, 1.0, S)["n_clusters"] == 1


# ---- invariants on random graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edges", (150, 900))
@pytest.mark.parametrize("key", ("intersect", "target_containment", "max_containment", "jaccard"))
def test_invariants_and_containment_in_components(key, n_edges):
    n = 300
    S, rows = gs.build(n, gs.random_graph(n, n_edges, seed=n_edges))
    sc = greedy_ref.scores(key, *rows, S, S)
    off = sc[rows[0] != rows[1]]
    sizes = np.diff(S[0])
    for thr in (float(np.quantile(off, 0.3, method="lower")), float(np.quantile(off, 0.8, method="lower"))):
        comp = cluster_ref.cluster(n, rows[0], rows[1], sc, thr)
        for node_sizes in (None, sizes):
            reps = None
            for assign in greedy_ref.ASSIGN:
                r = greedy_ref.cluster(n, rows[0], rows[1], sc, thr, node_sizes, assign)
                greedy_ref.check_invariants(r["label"], n, rows[0], rows[1], sc, thr, node_sizes, assign)
                # a greedy cluster lies inside one component
                assert np.array_equal(comp["label"][r["label"].astype(np.int64)], comp["label"])
                assert r["n_clusters"] >= comp["n_clusters"] and r["n_edges"] == comp["n_edges"]
                assert reps is None or np.array_equal(reps, r["representative"])
                reps = r["representative"]
                assert np.array_equal(r["representative"], np.unique(r["label"]))
                assert int(r["offsets"][-1]) == n and np.array_equal(np.sort(r["members"]), np.arange(n))


def test_check_invariants_catches_a_wrong_label():
    q, t = _both([(0, 1), (1, 2), (2, 3)])
    one = np.ones(len(q))
    greedy_ref.check_invariants([0, 0, 2, 2], 4, q, t, one, 1.0)
    with pytest.raises(AssertionError):
        greedy_ref.check_invariants([0, 0, 0, 3], 4, q, t, one, 1.0)  # 2 has no row with 0
    with pytest.raises(AssertionError):
        greedy_ref.check_invariants([0, 1, 2, 2], 4, q, t, one, 1.0)  # 0 and 1 are neighbours
    with pytest.raises(AssertionError):
        greedy_ref.check_invariants([1, 1, 3, 3], 4, q, t, one, 1.0)  # 0 has the higher priority
    greedy_ref.check_invariants([1, 1, 3, 3], 4, q, t, one, 1.0, assign="best")  # (best may join a representative of lower priority)


# ---- wire ----------------------------------------------------------------------------------------------------------------------
def test_cluster_rows_name_greedy_clusters():
    names = ["a b", "c", "d", "e", "f"]
    q, t = _both([(1, 2), (2, 4)])
    r = greedy_ref.cluster(5, q, t, np.ones(len(q)), 1.0, node_sizes=[1, 1, 3, 1, 2])
    rows = wire.cluster_rows(names, r["offsets"], r["members"], r["representative"], "Cluster")
    assert rows == [("Cluster_0", "a b", 1, "a b"), ("Cluster_1", "d", 3, "c;d;f"), ("Cluster_2", "e", 1, "e")]
    assert wire.cluster_rows(names, r["offsets"], r["members"], r["representative"])[1][0] == "Component_1"
    assert "greedy" in wire.do_cluster.__doc__ and "no parity" in wire.do_cluster.__doc__
    with pytest.raises(ValueError):
        wire.do_cluster("none.sig.zip", "none.csv", 7, 1, "protein", method="linkage")


# ---- the option checks need no device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def test_greedy_opts_layout_matches_header():
    assert C.sizeof(_lib.ks_greedy_opts) == 24
    o = _lib.ks_greedy_opts
    assert [(getattr(o, f).offset, getattr(o, f).size) for f, _ in o._fields_] == [(0, 4), (4, 4), (8, 8), (16, 4), (20, 4)]
    text = open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read()
    body = re.search(r"typedef struct ks_greedy_opts \{(.*?)\} ks_greedy_opts;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|double)\s+(\w+);", body)
    ctype = {"uint32_t": C.c_uint32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(o._fields_)
    assert [n for _, n in fields] == ["similarity", "n_nodes", "threshold", "assign", "flags"]
    assert (_lib.KS_GREEDY_ASSIGN_FIRST, _lib.KS_GREEDY_ASSIGN_BEST) == (0, 1)
    assert re.search(r"#define KS_GREEDY_ASSIGN_FIRST 0u", text) and re.search(r"#define KS_GREEDY_ASSIGN_BEST\s+1u", text)


def test_bad_greedy_options_are_refused_without_a_context(lib):
    J, S, I = _lib.KS_BEST_JACCARD, _lib.KS_BEST_SCORE, _lib.KS_BEST_INTERSECT
    column = C.c_void_p(8)  # never read: the options are refused first
    bad = [
        ((5, 3, 0.0, 0, 0), None),          # unknown similarity
        ((I, 3, 0.0, 0, 1), None),          # flags
        ((I, 3, 0.0, 2, 0), None),          # unknown assign mode
        ((I, 3, float("nan"), 0, 0), None),  # NaN threshold
        ((I, 3, float("nan"), 1, 0), None),
        ((S, 3, 0.0, 0, 0), None),          # KS_BEST_SCORE without a column
        ((I, 3, 0.0, 1, 0), column),        # a column without KS_BEST_SCORE
        ((J, 3, 0.0, 0, 0), None),          # a key that needs sizes, no node set
        ((_lib.KS_BEST_TARGET_CONTAINMENT, 3, 0.0, 1, 0), None),
        ((_lib.KS_BEST_MAX_CONTAINMENT, 3, 0.0, 0, 0), None),
    ]
    for words, col in bad:
        out = C.c_void_p(1)
        st = lib.ks_hits_cluster_greedy(None, None, None, col, C.byref(_lib.ks_greedy_opts(*words)), C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG, words
        assert not out.value
    out = C.c_void_p(1)
    assert lib.ks_hits_cluster_greedy(None, None, None, None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
    # good options and no context: still an error, and nothing is made
    for assign in (0, 1):
        good = _lib.ks_greedy_opts(I, 3, 0.0, assign, 0)
        assert lib.ks_hits_cluster_greedy(None, None, None, None, C.byref(good), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    # the accessor of no object, and the constant the GPU tests size their edge lists with
    assert lib.ks_clusters_n_rounds(None) == 0
    assert 1024 <= lib.ks_debug_greedy_tail_edges() <= 1 << 20
