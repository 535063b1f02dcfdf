"""GPU: ks_hits_cluster_greedy — greedy representative clustering of an all-vs-all hit list.

Everything is exact, integers only: every output array and scalar except n_rounds is compared with the sequential host
definition of tests/greedy_ref.py.  The graphs come from tests/graph_sketches.py through a real self-search, and every case
first checks that the searched rows are the rows the graph was built to give, so that what is tested is the greedy pass.  Every
case runs once per value of KS_DEBUG_GREEDY_PATH (unset: grid rounds until few edges are live, then one workgroup; 1: grid rounds
only; 2: the one workgroup straight after the first round) and under both assign modes.  The shapes are the smallest that can
still go wrong: chains around the wave size (the worst case for the number of rounds), stars, two cliques and a bridge, random
graphs below and above the percolation point under all four computed keys, rows of one direction only, an uploaded score
column with NaN / infinities / signed zeros, empty nodes, one node, no rows, priority ties, an edge list on either side of the
threshold between the two round kernels, the refusals, the input left unchanged, and real proteins through wire."""
import csv
import functools
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref  # noqa: E402
import graph_sketches as gs  # noqa: E402
import greedy_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
KNOB = "KS_DEBUG_GREEDY_PATH"
PATHS = (None, "1", "2")
KEYS = ("intersect", "target_containment", "max_containment", "jaccard")
ASSIGN = greedy_ref.ASSIGN
ARRAYS = ("label", "cluster_id", "offsets", "members", "representative")
SCALARS = ("n_nodes", "n_clusters", "n_edges", "largest")


def _set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, path)


def _upload(ctx, S):
    return ctx.sketches_from_host(S[0], S[1], S[2], 10, 1, "protein")


def _search(ctx, S, rows):
    """the set against itself; the rows must be the ones the graph was built to give"""
    dS = _upload(ctx, S)
    hits = ctx.search(ctx.index_build(dS), dS)
    h = hits.to_host()
    assert hits.count == len(rows[0])
    for g, w in zip(h, rows):
        assert np.array_equal(g, w)
    return dS, hits, h


def _check(cl, want):
    """every array and scalar; n_rounds is a diagnostic: at least one round on a set that has nodes, nothing more is asked"""
    got = dict(zip(ARRAYS, cl.to_host()))
    for name in SCALARS:
        assert getattr(cl, name) == want[name], (name, getattr(cl, name), want[name])
    for name in ARRAYS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert all(p != 0 for p in cl.device_ptrs())
    assert cl.n_rounds >= 1 if want["n_nodes"] else cl.n_rounds == 0
    return got


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """-> (n, S, rows): built once, shared by the paths"""
    if kind.startswith("chain_permuted_"):
        n = int(kind.rsplit("_", 1)[1])
        e = gs.chain(n, np.random.default_rng(11).permutation(n))
    elif kind.startswith("chain_"):
        n = int(kind.rsplit("_", 1)[1])
        e = gs.chain(n)
    elif kind == "star_low":
        n, e = 301, gs.star(300, 0)
    elif kind == "star_high":
        n, e = 301, gs.star(300, 300)
    elif kind == "bridge":
        n, e = 80, gs.cliques_with_bridge(40)
    elif kind == "sparse":
        n, e = 3000, gs.random_graph(3000, 1500, seed=21)
    elif kind == "dense":
        n, e = 3000, gs.random_graph(3000, 9000, seed=22)
    else:
        raise ValueError(kind)
    S, rows = gs.build(n, e)
    return n, S, rows


@functools.lru_cache(maxsize=None)
def _want(kind, key, threshold, with_sizes=True, assign="first"):
    n, S, rows = _graph(kind)
    return greedy_ref.cluster_hits(key, n, *rows, threshold, S if with_sizes else None, assign=assign)


# ---- chains: the worst case for the number of rounds ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("chain", "chain_permuted"))
def test_chains(monkeypatch, kind, path):
    with ks.Context(0, follow_debug_env=True) as c:
        for n in (63, 64, 65, 257, 2000):
            _, S, rows = _graph(f"{kind}_{n}")
            dS, hits, _ = _search(c, S, rows)
            _set_path(monkeypatch, path)
            for assign in ASSIGN:
                want = _want(f"{kind}_{n}", "intersect", 1.0, False, assign)  # priority = id
                if kind == "chain":
                    assert want["representative"].tolist() == list(range(0, n, 2))  # every second node
                cl = c.cluster_greedy(hits, "intersect", 1.0, n_nodes=n, assign=assign)
                _check(cl, want)
                assert cl.n_rounds >= 1
                cl.free()
            # the links of weight 2 pull their member over under "best": the modes differ on a chain
            assert not np.array_equal(_want(f"{kind}_{n}", "intersect", 1.0, False, "first")["label"],
                                      _want(f"{kind}_{n}", "intersect", 1.0, False, "best")["label"])
            # with the node set the sizes order the nodes
            _check(c.cluster_greedy(hits, "intersect", 1.0, nodes=dS), _want(f"{kind}_{n}", "intersect", 1.0, True))
            monkeypatch.delenv(KNOB, raising=False)
            for o in (hits, dS):
                o.free()


# ---- stars -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("star_low", "star_high"))
def test_stars(monkeypatch, kind, path):
    n, S, rows = _graph(kind)
    hub = 0 if kind == "star_low" else n - 1
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            # by size the hub is the one representative
            want = _want(kind, "intersect", 1.0, True, assign)
            assert want["n_clusters"] == 1 and want["representative"].tolist() == [hub] and want["largest"] == 301
            got = _check(c.cluster_greedy(hits, "intersect", 1.0, nodes=dS, assign=assign), want)
            assert got["label"].tolist() == [hub] * 301
            _check(c.cluster_greedy(hits, "jaccard", 0.0, nodes=dS, assign=assign), _want(kind, "jaccard", 0.0, True, assign))
            # by id: a hub that comes first takes everything; a hub that comes last joins node 0 and every other leaf stays alone
            bare = _want(kind, "intersect", 1.0, False, assign)
            assert bare["n_clusters"] == (1 if hub == 0 else 300) and bare["largest"] == (301 if hub == 0 else 2)
            got = _check(c.cluster_greedy(hits, "intersect", 1.0, n_nodes=n, assign=assign), bare)
            assert got["label"][hub] == 0 and got["label"][1] == (0 if hub == 0 else 1)


# ---- two cliques and a bridge: where single linkage chains -----------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_bridge_is_two_clusters(monkeypatch, path):
    n, S, rows = _graph("bridge")
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            want = _want("bridge", "intersect", 1.0, True, assign)
            assert want["n_clusters"] == 2 and want["representative"].tolist() == [2, 40]
            got = _check(c.cluster_greedy(hits, "intersect", 1.0, nodes=dS, assign=assign), want)
            assert got["label"].tolist() == [2] * 40 + [40] * 40 and got["offsets"].tolist() == [0, 40, 80]
        components = c.cluster(hits, "intersect", 1.0, nodes=dS)
        assert components.n_clusters == 1 and components.n_rounds == 0  # the contrast: one component


# ---- random graphs: all four keys, both modes ------------------------------------------------------------------------------------
def _thresholds(kind, key):
    """two thresholds that are scores of off-diagonal rows (the >= is tested on equality): a low and a high quantile"""
    n, S, rows = _graph(kind)
    s = greedy_ref.scores(key, *rows, S, S)[rows[0] != rows[1]]
    return tuple(float(np.quantile(s, q, method="lower")) for q in (0.3, 0.8))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("sparse", "dense"))
def test_random_graphs(monkeypatch, kind, path):
    n, S, rows = _graph(kind)
    sizes = np.diff(S[0])
    differ = 0
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            _check(c.cluster_greedy(hits, "intersect", 1.0, n_nodes=n, assign=assign), _want(kind, "intersect", 1.0, False, assign))
        for key in KEYS:
            sc = greedy_ref.scores(key, *rows, S, S)
            for thr in _thresholds(kind, key):
                labels = []
                for assign in ASSIGN:
                    want = _want(kind, key, thr, True, assign)
                    assert 1 < want["n_clusters"] < n
                    cl = c.cluster_greedy(hits, key, thr, nodes=dS, assign=assign)
                    got = _check(cl, want)
                    cl.free()
                    greedy_ref.check_invariants(got["label"], n, rows[0], rows[1], sc, thr, sizes, assign)  # on the device's output
                    labels.append(got["label"])
                if key == "target_containment":
                    differ += int(not np.array_equal(*labels))
    assert differ  # target containment scores the two rows of a pair differently: there the two modes part


# ---- rows of one direction only --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_one_direction_is_enough(monkeypatch, path):
    import torch
    n, S, rows = _graph("sparse")
    # self rows rank last: the one kept row of a query is its best neighbour, and most pairs survive in one direction only
    score = np.where(rows[0] == rows[1], -1.0, rows[2].astype(np.float64))
    d_score = torch.from_numpy(score).to("cuda:0")
    torch.cuda.synchronize()
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        best = c.best_hits(hits, 1, "score", score=d_score)
        b = best.to_host()
        key = set(zip(b[0].tolist(), b[1].tolist()))
        one_way = sum((t, q) not in key for q, t in key if q != t)
        assert best.count == n and one_way > 100
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            for k in ("jaccard", "target_containment"):
                _check(c.cluster_greedy(best, k, 0.0, nodes=dS, assign=assign), greedy_ref.cluster_hits(k, n, *b[:3], 0.0, S, assign=assign))
            _check(c.cluster_greedy(best, "intersect", 2.0, n_nodes=n, assign=assign), greedy_ref.cluster_hits("intersect", n, *b[:3], 2.0, assign=assign))


# ---- an uploaded score column ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_score_column(monkeypatch, path):
    import torch
    n, S, rows = _graph("sparse")
    vals = np.array([np.nan, -np.inf, -1.5, -0.0, 0.0, 1e-300, 2.0, np.inf])
    score = vals[np.random.default_rng(32).integers(0, 8, len(rows[0]))]
    assert np.signbit(score[score == 0.0]).any() and not np.signbit(score[score == 0.0]).all()
    d_score = torch.from_numpy(score).to("cuda:0")
    torch.cuda.synchronize()
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            for thr in (-np.inf, -1.5, 0.0, 1e-300, np.inf):
                want = greedy_ref.cluster_hits("score", n, *rows, thr, score=score, assign=assign)
                cl = c.cluster_greedy(hits, threshold=thr, score=d_score, n_nodes=n, assign=assign)
                _check(cl, want)
                if thr == -np.inf:
                    assert cl.n_edges == np.count_nonzero(~np.isnan(score))  # everything but NaN
                if thr == 0.0:
                    assert cl.n_edges == np.count_nonzero(score == 0.0) + np.count_nonzero(score > 0.0)  # -0.0 is in
                cl.free()
            # with the node set the sizes order the nodes
            _check(c.cluster_greedy(hits, "score", 0.0, nodes=dS, score=int(d_score.data_ptr()), assign=assign),
                   greedy_ref.cluster_hits("score", n, *rows, 0.0, S, score=score, assign=assign))
        # "best" on a column where -0.0 and +0.0 are the best a member has: a tie, the higher priority
        assert not np.array_equal(greedy_ref.cluster_hits("score", n, *rows, -1.5, score=score, assign="first")["label"],
                                  greedy_ref.cluster_hits("score", n, *rows, -1.5, score=score, assign="best")["label"])


# ---- empty nodes, one node, no rows, priority ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_empty_nodes_one_node_no_rows_and_ties(monkeypatch, path):
    e = np.array([(0, 1, 2), (1, 5, 1), (6, 8, 1), (8, 9, 3)], np.int64)
    S, rows = gs.build(12, e, empty=[3, 4, 11])
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            for key in KEYS:
                want = greedy_ref.cluster_hits(key, 12, *rows, 0.0, S, assign=assign)
                # sizes: |1| = 2 + 3, |8| = 3 + 4: the two representatives that have members; empty nodes represent themselves
                assert want["label"].tolist() == [1, 1, 2, 3, 4, 1, 8, 7, 8, 8, 10, 11]
                _check(c.cluster_greedy(hits, key, 0.0, nodes=dS, n_nodes=12 if key == "jaccard" else 0, assign=assign), want)
            # one node
            S1, rows1 = gs.build(1, [])
            d1, hits1, _ = _search(c, S1, rows1)
            want = greedy_ref.cluster_hits("jaccard", 1, *rows1, 0.0, S1, assign=assign)
            assert (want["n_clusters"], want["n_edges"], want["largest"]) == (1, 1, 1)
            _check(c.cluster_greedy(hits1, "jaccard", 0.0, nodes=d1, assign=assign), want)
            _check(c.cluster_greedy(hits1, "intersect", 5.0, n_nodes=1, assign=assign), dict(want, n_edges=0))
            # sketches that share nothing: self rows only, n singletons
            S0, rows0 = gs.build(200, [])
            d0, hits0, _ = _search(c, S0, rows0)
            want = greedy_ref.cluster_hits("jaccard", 200, *rows0, 0.0, S0, assign=assign)
            assert want["n_clusters"] == 200 and want["n_edges"] == 200
            _check(c.cluster_greedy(hits0, "jaccard", 0.0, nodes=d0, assign=assign), want)
            # no rows at all: the set searched against an index of a set it shares nothing with; and no nodes at all
            other = c.sketches_from_host(S0[0], S0[1] + np.uint64(12345), S0[2], 10, 1, "protein")
            none = c.search(c.index_build(other), d0)
            assert none.count == 0
            empty = tuple(np.zeros(0, np.uint32) for _ in range(3))
            _check(c.cluster_greedy(none, "jaccard", 0.0, nodes=d0, assign=assign), greedy_ref.cluster_hits("jaccard", 200, *empty, 0.0, S0))
            _check(c.cluster_greedy(none, "intersect", 0.0, n_nodes=7, assign=assign), greedy_ref.cluster_hits("intersect", 7, *empty, 0.0))
            nothing = c.cluster_greedy(none, "intersect", 0.0, n_nodes=0, assign=assign)
            assert (nothing.n_nodes, nothing.n_clusters, nothing.n_rounds) == (0, 0, 0) and nothing.to_host()[2].tolist() == [0]
            # ties: |0| = 2, |1| = |2| = 4 — 1 is taken before 2 and takes both neighbours; were 2 first, 0 would stand alone
            St, rows_t = gs.build(3, [(0, 1, 1), (1, 2, 1)])
            assert np.diff(St[0]).tolist() == [2, 4, 4]
            dt, hits_t, _ = _search(c, St, rows_t)
            got = _check(c.cluster_greedy(hits_t, "intersect", 1.0, nodes=dt, assign=assign), greedy_ref.cluster_hits("intersect", 3, *rows_t, 1.0, St, assign=assign))
            assert got["label"].tolist() == [1, 1, 1]
            for o in (hits_t, dt, nothing, none, other, hits0, d0, hits1, d1):
                o.free()


# ---- an edge list on either side of the threshold between grid rounds and the one workgroup ----------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_edge_list_around_the_tail_threshold(monkeypatch, path):
    import torch
    tail = _lib.load().ks_debug_greedy_tail_edges()
    n = max(3000, tail // 8)
    S, rows = gs.build(n, gs.random_graph(n, tail // 2 + 600, seed=51))
    off = np.nonzero(rows[0] != rows[1])[0]
    assert len(off) > tail + 1
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for n_live in (tail - 1, tail, tail + 1):  # unset: tail and fewer go to the one workgroup at once, tail + 1 takes grid rounds first
            score = np.zeros(len(rows[0]))
            score[off[:n_live]] = 1.0
            d_score = torch.from_numpy(score).to("cuda:0")
            torch.cuda.synchronize()
            for assign in ASSIGN:
                want = greedy_ref.cluster_hits("score", n, *rows, 0.5, S, score=score, assign=assign)
                assert want["n_edges"] == n_live and 1 < want["n_clusters"] < n
                cl = c.cluster_greedy(hits, "score", 0.5, nodes=dS, score=d_score, assign=assign)
                _check(cl, want)
                cl.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_refusals_leave_the_context_usable(monkeypatch, path):
    n = 500
    S, rows = gs.build(n, gs.random_graph(n, 600, seed=41))
    small = 60
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, h = _search(c, S, rows)
        _set_path(monkeypatch, path)
        # the first `small` sketches as the node set: the list was searched on a larger one, tids run beyond it
        k = int(S[0][small])
        d_small = c.sketches_from_host(S[0][:small + 1].copy(), S[1][:k].copy(), S[2][:k].copy(), 10, 1, "protein")
        first_bad = int(np.nonzero((h[0] >= small) | (h[1] >= small))[0][0])
        assert first_bad > 0
        # a node set of the right length in which the first node that has an edge is empty
        hollow_id = int(h[0][np.nonzero(h[0] != h[1])[0][0]])
        lo, hi = int(S[0][hollow_id]), int(S[0][hollow_id + 1])
        keep = np.ones(len(S[1]), bool); keep[lo:hi] = False
        offs = S[0].copy(); offs[hollow_id + 1:] -= np.uint64(hi - lo)
        hollow = c.sketches_from_host(offs, S[1][keep], S[2][keep], 10, 1, "protein")
        first_hollow = int(np.nonzero((h[0] == hollow_id) | (h[1] == hollow_id))[0][0])
        c.cluster_greedy(hits, "jaccard", 0.1, nodes=dS, assign="best").free()  # (the pool has grown to what the pass needs)
        before = c.pool_stats()["bytes_in_use"]
        for assign in ASSIGN:
            for key in KEYS:
                with pytest.raises(ks.KmerseekError) as e:
                    c.cluster_greedy(hits, key, 0.0, nodes=d_small, assign=assign)
                assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_bad} names a node beyond the {small} nodes" in str(e.value), str(e.value)
            with pytest.raises(ks.KmerseekError) as e:
                c.cluster_greedy(hits, "intersect", 0.0, n_nodes=small, assign=assign)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_bad} " in str(e.value), str(e.value)
            for key in ("max_containment", "jaccard"):
                with pytest.raises(ks.KmerseekError) as e:
                    c.cluster_greedy(hits, key, 0.0, nodes=hollow, assign=assign)
                assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_hollow} names an empty sketch" in str(e.value), str(e.value)
            c.cluster_greedy(hits, "intersect", 0.0, nodes=hollow, assign=assign).free()  # (the key reads no size)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster_greedy(hits, "jaccard", 0.0, nodes=dS, n_nodes=n + 1)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "n_nodes" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster_greedy(hits, "jaccard", float("nan"), nodes=dS)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "options" in str(e.value) and "NaN" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster_greedy(hits, "score", 0.0, n_nodes=n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "score" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster_greedy(hits, "jaccard", 0.0, nodes=dS, score=8)  # an explicit key with a column it does not read (never dereferenced)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "score column" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster_greedy(hits, "jaccard", 0.0)  # a key that needs sizes, no node set
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "node sketches" in str(e.value)
        with pytest.raises(ValueError):
            c.cluster_greedy(hits, "cosine")
        with pytest.raises(ValueError):
            c.cluster_greedy(hits, "jaccard", nodes=dS, assign="nearest")
        assert c.pool_stats()["bytes_in_use"] == before
        # the context stays usable
        _check(c.cluster_greedy(hits, "jaccard", 0.1, nodes=dS), greedy_ref.cluster_hits("jaccard", n, *rows, 0.1, S))
        cl = c.cluster(hits, "jaccard", 0.1, nodes=dS)
        assert cl.n_clusters == cluster_ref.cluster_hits("jaccard", n, *rows, 0.1, S)["n_clusters"]


# ---- the input is left alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_input_unchanged_and_scratch_returned(monkeypatch, path):
    n, S, rows = _graph("dense")
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, h = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for assign in ASSIGN:
            c.cluster_greedy(hits, "jaccard", 0.1, nodes=dS, assign=assign).free()  # (the pool has grown to what the pass needs)
            before = c.pool_stats()["bytes_in_use"]
            cl = c.cluster_greedy(hits, "jaccard", 0.1, nodes=dS, assign=assign)
            assert c.pool_stats()["bytes_in_use"] > before
            _check(cl, _want("dense", "jaccard", 0.1, True, assign))
            cl.free()
            assert c.pool_stats()["bytes_in_use"] == before
        for g, w in zip(hits.to_host(), h):
            assert np.array_equal(g, w)
        assert hits.count == len(rows[0])
        for g, w in zip(dS.to_host(), S):
            assert np.array_equal(g, w)


# ---- real proteins through wire ------------------------------------------------------------------------------------------------------
def _lines(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _csv_bytes(rows):
    f = io.StringIO(newline="")
    w = csv.writer(f, lineterminator="\n")
    w.writerow(wire.CLUSTER_COLUMNS)
    w.writerows(rows)
    return f.getvalue().encode()


@pytest.mark.parametrize("path", PATHS)
def test_do_cluster_greedy_on_bcl2(monkeypatch, tmp_path, path):
    moltype, ksize, scaled = "hp", 16, 5
    fasta = tmp_path / BCL2_300
    fasta.write_bytes(open(os.path.join(GOLDEN, BCL2_300), "rb").read())
    with ks.Context(0, follow_debug_env=True) as c:
        sig = wire.sketch(str(fasta), moltype, ksize, scaled, ctx=c)
        names, so, sm, sa, *_ = wire.read_sig_zip(sig)
        assert len(names) == 300
        S = c.sketches_from_host(so, sm, sa, ksize, scaled, moltype)
        h = c.search(c.index_build(S), S).to_host()
        sc = greedy_ref.scores("jaccard", *h[:3], (so, sm, sa), (so, sm, sa))
        _set_path(monkeypatch, path)
        seen = set()
        for thr in (0.05, 0.3):
            for assign in ASSIGN:
                out, sizes = str(tmp_path / f"greedy_{thr}_{assign}.csv"), str(tmp_path / f"sizes_{thr}_{assign}.csv")
                want = greedy_ref.cluster_hits("jaccard", 300, *h[:3], thr, (so, sm, sa), assign=assign)
                greedy_ref.check_invariants(want["label"], 300, h[0], h[1], sc, thr, np.diff(so), assign)
                n_rows = wire.do_cluster(sig, out, ksize, scaled, moltype, "jaccard", thr, sizes_output=sizes, ctx=c, method="greedy", assign=assign)
                rows = wire.cluster_rows(names, want["offsets"], want["members"], want["representative"], "Cluster")
                assert n_rows == want["n_clusters"] == len(rows) and rows[0][0] == "Cluster_0"
                assert _lines(out) == [wire.CLUSTER_COLUMNS] + [[str(x) for x in r] for r in rows]
                hist = np.unique(np.diff(want["offsets"].astype(np.int64)), return_counts=True)
                assert _lines(sizes) == [["cluster_size", "count"]] + [[str(s), str(k)] for s, k in zip(*[x.tolist() for x in hist])]
                seen.add(want["n_clusters"])
            # the default method writes what it always wrote, byte for byte: the connected components, named Component_<i>
            plain = str(tmp_path / f"components_{thr}.csv")
            comp = cluster_ref.cluster_hits("jaccard", 300, *h[:3], thr, (so, sm, sa))
            assert wire.do_cluster(sig, plain, ksize, scaled, moltype, "jaccard", thr, ctx=c) == comp["n_clusters"]
            assert open(plain, "rb").read() == _csv_bytes(wire.cluster_rows(names, comp["offsets"], comp["members"], comp["representative"]))
            assert comp["n_clusters"] <= want["n_clusters"]
        assert 1 < min(seen) and max(seen) < 300
