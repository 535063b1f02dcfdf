"""GPU: ks_hits_cluster — the connected components of an all-vs-all hit list.

Everything is exact, integers only: every output array and scalar is compared with the host union-find of tests/cluster_ref.py.
The graphs come from tests/graph_sketches.py, and every case first checks that the searched rows are the rows the graph was
built to give, so that what is tested is the cluster pass.  Every case runs once per value of KS_DEBUG_CLUSTER_PATH (unset: the
default; 1: the plain lane-per-row path; 2: the wave-uniform query path).  Cases: long chains in and against id order, stars around a low and
a high hub, two cliques and a bridge under three thresholds, random graphs below and above the percolation point under all
four computed keys, empty nodes, one node, an empty hit list, rows of one direction only, an uploaded score column with NaN /
infinities / signed zeros, the representative's ties, the refusals, the input left unchanged, and real proteins through wire."""
import csv
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref  # noqa: E402
import crafted_sketches as cs  # noqa: E402
import graph_sketches as gs  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
PATHS = (None, "1", "2")  # KS_DEBUG_CLUSTER_PATH: the default, the plain lane-per-row path, the wave-uniform query path
KEYS = ("intersect", "target_containment", "max_containment", "jaccard")
ARRAYS = ("label", "cluster_id", "offsets", "members", "representative")
SCALARS = ("n_nodes", "n_clusters", "n_edges", "largest")


def _set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv("KS_DEBUG_CLUSTER_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_CLUSTER_PATH", path)


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
    got = dict(zip(ARRAYS, cl.to_host()))
    for name in SCALARS:
        assert getattr(cl, name) == want[name], (name, getattr(cl, name), want[name])
    for name in ARRAYS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert all(p != 0 for p in cl.device_ptrs())


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """-> (n, S, rows): built once, shared by both paths"""
    if kind == "chain":
        n, e = 70001, gs.chain(70001)
    elif kind == "chain_permuted":
        n, e = 70001, gs.chain(70001, np.random.default_rng(11).permutation(70001))
    elif kind == "star_low":
        n, e = 5001, gs.star(5000, 0)
    elif kind == "star_high":
        n, e = 5001, gs.star(5000, 5000)
    elif kind == "bridge":
        n, e = 80, gs.cliques_with_bridge(40)
    elif kind == "sparse":
        n, e = 20000, gs.random_graph(20000, 10000, seed=21)
    elif kind == "dense":
        n, e = 20000, gs.random_graph(20000, 40000, seed=22)
    else:
        raise ValueError(kind)
    S, rows = gs.build(n, e)
    return n, S, rows


@functools.lru_cache(maxsize=None)
def _want(kind, key, threshold, with_sizes=True):
    n, S, rows = _graph(kind)
    return cluster_ref.cluster_hits(key, n, *rows, threshold, S if with_sizes else None)


# ---- chains and stars ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("chain", "chain_permuted"))
def test_chains(monkeypatch, kind, path):
    n, S, rows = _graph(kind)
    want = _want(kind, "intersect", 1.0)
    assert want["n_clusters"] == 1 and want["largest"] == n and want["n_edges"] == len(rows[0])
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        _check(c.cluster(hits, "intersect", 1.0, nodes=dS), want)
        # only the heavier links (weight 2, every second one): pairs
        want2 = _want(kind, "intersect", 2.0)
        assert want2["largest"] == 2 and want2["n_clusters"] == n - (n - 1) // 2
        bare = _want(kind, "intersect", 2.0, False)  # without the node set the smallest member represents
        assert np.array_equal(bare["representative"], np.unique(bare["label"])) and not np.array_equal(bare["representative"], want2["representative"])
        _check(c.cluster(hits, "intersect", 2.0, nodes=dS), want2)
        _check(c.cluster(hits, "intersect", 2.0, n_nodes=n), bare)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("star_low", "star_high"))
def test_stars(monkeypatch, kind, path):
    n, S, rows = _graph(kind)
    hub = 0 if kind == "star_low" else n - 1
    want = _want(kind, "jaccard", 0.0)
    assert want["n_clusters"] == 1 and want["representative"].tolist() == [hub] and want["label"].max() == 0
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        _check(c.cluster(hits, "jaccard", 0.0, nodes=dS), want)
        _check(c.cluster(hits, "target_containment", 0.25, nodes=dS), _want(kind, "target_containment", 0.25))


# ---- two cliques and a bridge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_threshold_cuts_the_bridge(monkeypatch, path):
    n, S, rows = _graph("bridge")
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for thr, n_clusters in ((2.0, 2), (1.0, 1), (1000.0, 80)):
            want = _want("bridge", "intersect", thr)
            assert want["n_clusters"] == n_clusters
            cl = c.cluster(hits, "intersect", thr, nodes=dS)
            _check(cl, want)
        assert cl.n_edges == 0 and cl.largest == 1
        two = c.cluster(hits, "intersect", 2.0, nodes=dS).to_host()
        assert two[0].tolist() == [0] * 40 + [40] * 40 and two[2].tolist() == [0, 40, 80]


# ---- random graphs: components of every size, all four keys ------------------------------------------------------------------------
def _thresholds(kind, key):
    """two thresholds that are scores of off-diagonal rows (the >= is tested on equality): a low and a high quantile"""
    n, S, rows = _graph(kind)
    s = cluster_ref.scores(key, *rows, S, S)[rows[0] != rows[1]]
    return tuple(float(np.quantile(s, q, method="lower")) for q in (0.3, 0.8))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ("sparse", "dense"))
def test_random_graphs(monkeypatch, kind, path):
    n, S, rows = _graph(kind)
    everything = _want(kind, "intersect", 1.0)
    sizes = np.diff(everything["offsets"].astype(np.int64))
    if kind == "sparse":
        assert len(set(sizes.tolist())) >= 8 and sizes.max() < n // 4  # components of many sizes, no giant one yet
    else:
        assert sizes.max() > n // 2  # one giant component
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        _check(c.cluster(hits, "intersect", 1.0, nodes=dS), everything)
        for key in KEYS:
            for thr in _thresholds(kind, key):
                want = _want(kind, key, thr)
                assert 1 < want["n_clusters"] < n
                cl = c.cluster(hits, key, thr, nodes=dS)
                _check(cl, want)
                cl.free()


# ---- empty nodes, one node, no rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_empty_nodes_one_node_and_no_rows(monkeypatch, path):
    e = np.array([(0, 1, 2), (1, 5, 1), (6, 8, 1), (8, 9, 3)], np.int64)
    S, rows = gs.build(12, e, empty=[3, 4, 11])
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for key in KEYS:
            want = cluster_ref.cluster_hits(key, 12, *rows, 0.0, S)
            assert want["label"].tolist() == [0, 0, 2, 3, 4, 0, 6, 7, 6, 6, 10, 11]
            _check(c.cluster(hits, key, 0.0, nodes=dS, n_nodes=12 if key == "jaccard" else 0), want)
        assert want["representative"].tolist() == [1, 2, 3, 4, 8, 7, 10, 11]  # empty nodes represent themselves
        # one node
        S1, rows1 = gs.build(1, [])
        d1, hits1, _ = _search(c, S1, rows1)
        want = cluster_ref.cluster_hits("jaccard", 1, *rows1, 0.0, S1)
        assert (want["n_clusters"], want["n_edges"], want["largest"]) == (1, 1, 1)
        _check(c.cluster(hits1, "jaccard", 0.0, nodes=d1), want)
        _check(c.cluster(hits1, "intersect", 5.0, n_nodes=1), dict(want, n_edges=0))
        # sketches that share nothing: self rows only, n singletons
        S0, rows0 = gs.build(200, [])
        d0, hits0, _ = _search(c, S0, rows0)
        want = cluster_ref.cluster_hits("jaccard", 200, *rows0, 0.0, S0)
        assert want["n_clusters"] == 200 and want["n_edges"] == 200
        _check(c.cluster(hits0, "jaccard", 0.0, nodes=d0), want)
        # no rows at all: the set searched against an index of a set it shares nothing with
        other = c.sketches_from_host(S0[0], S0[1] + np.uint64(12345), S0[2], 10, 1, "protein")
        none = c.search(c.index_build(other), d0)
        assert none.count == 0
        empty = tuple(np.zeros(0, np.uint32) for _ in range(3))
        _check(c.cluster(none, "jaccard", 0.0, nodes=d0), cluster_ref.cluster_hits("jaccard", 200, *empty, 0.0, S0))
        _check(c.cluster(none, "intersect", 0.0, n_nodes=7), cluster_ref.cluster_hits("intersect", 7, *empty, 0.0))


# ---- rows of one direction only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_one_direction_is_enough(monkeypatch, path):
    # |2| = 3 + 2, |5| = 3 + 2 + 95: (2, 5) scores 2 / 100, (5, 2) scores 2 / 5
    e = np.array([(2, 5, 2)], np.int64)
    S, rows = gs.build(7, e, extra={5: 95})
    tc = cluster_ref.scores("target_containment", *rows, S, S)
    pair = {(int(q), int(t)): float(s) for q, t, s in zip(rows[0], rows[1], tc)}
    assert pair[(2, 5)] == 0.02 and pair[(5, 2)] == 0.4
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, h = _search(c, S, rows)
        _set_path(monkeypatch, path)
        want = cluster_ref.cluster_hits("target_containment", 7, *rows, 0.3, S)
        assert want["label"].tolist() == [0, 1, 2, 3, 4, 2, 6] and want["n_edges"] == 7 + 1  # the self rows and (5, 2)
        _check(c.cluster(hits, "target_containment", 0.3, nodes=dS), want)
        # a best-hits list and a thresholded search keep one direction of some pairs: valid inputs, judged on their own rows
        n, Sr, rows_r = _graph("sparse")
        dR, hits_r, _ = _search(c, Sr, rows_r)
        best = c.best_hits(hits_r, 1, "intersect", dR, dR)  # (the self row wins every query: no edge survives)
        b = best.to_host()
        assert best.count == n and np.array_equal(b[0], b[1])
        _check(c.cluster(best, "jaccard", 0.0, nodes=dR), cluster_ref.cluster_hits("jaccard", n, *b[:3], 0.0, Sr))
        best2 = c.best_hits(hits_r, 2, "intersect", dR, dR)
        b = best2.to_host()
        key = set(zip(b[0].tolist(), b[1].tolist()))
        assert any((t, q) not in key for q, t in key)  # some pair kept in one direction only
        _check(c.cluster(best2, "jaccard", 0.0, nodes=dR), cluster_ref.cluster_hits("jaccard", n, *b[:3], 0.0, Sr))
        thin = c.search(c.index_build(dR), dR, min_containment=0.3)
        t = thin.to_host()
        key = set(zip(t[0].tolist(), t[1].tolist()))
        assert 0 < thin.count < hits_r.count and any((tt, q) not in key for q, tt in key)
        _check(c.cluster(thin, "max_containment", 0.0, nodes=dR), cluster_ref.cluster_hits("max_containment", n, *t[:3], 0.0, Sr))


# ---- an uploaded score column ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_score_column(monkeypatch, path):
    import torch
    n = 3000
    S, rows = gs.build(n, gs.random_graph(n, 2500, seed=31))
    vals = np.array([np.nan, -np.inf, -1.5, -0.0, 0.0, 1e-300, 2.0, np.inf])
    score = vals[np.random.default_rng(32).integers(0, 8, len(rows[0]))]
    assert np.signbit(score[score == 0.0]).any() and not np.signbit(score[score == 0.0]).all()
    d_score = torch.from_numpy(score).to("cuda:0")
    torch.cuda.synchronize()
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        for thr in (-np.inf, -1.5, 0.0, 1e-300, np.inf):
            want = cluster_ref.cluster_hits("score", n, *rows, thr, score=score)
            cl = c.cluster(hits, threshold=thr, score=d_score, n_nodes=n)  # (no node set: the smallest member represents)
            _check(cl, want)
            assert np.array_equal(want["representative"], want["label"][want["representative"].astype(np.int64)])
            if thr == -np.inf:
                assert cl.n_edges == np.count_nonzero(~np.isnan(score))  # everything but NaN
            if thr == 0.0:
                n_neg_zero = np.count_nonzero((score == 0.0) & np.signbit(score))
                assert n_neg_zero > 0 and cl.n_edges == n_neg_zero + np.count_nonzero((score == 0.0) & ~np.signbit(score)) + np.count_nonzero(score > 0.0)  # -0.0 is in
            cl.free()
        # with the node set the representative is the largest member again
        _check(c.cluster(hits, "score", 0.0, nodes=dS, score=int(d_score.data_ptr())), cluster_ref.cluster_hits("score", n, *rows, 0.0, S, score=score))


# ---- the representative ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_representative(monkeypatch, path):
    # |3| = 3, |6| = 5, |9| = 3: the middle one; |0| = |12| = 2: a tie, the smaller id; |1| = 3, |2| = 4: the larger id
    e = np.array([(3, 6, 2), (6, 9, 2), (0, 12, 1), (1, 2, 1)], np.int64)
    S, rows = gs.build(13, e)
    assert np.diff(S[0])[[3, 6, 9, 0, 12, 1, 2]].tolist() == [3, 5, 3, 2, 2, 3, 4]
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, _ = _search(c, S, rows)
        _set_path(monkeypatch, path)
        want = cluster_ref.cluster_hits("intersect", 13, *rows, 1.0, S)
        assert want["label"][want["representative"].astype(np.int64)].tolist() == [0, 1, 3, 4, 5, 7, 8, 10, 11]
        assert want["representative"].tolist() == [0, 2, 6, 4, 5, 7, 8, 10, 11]
        _check(c.cluster(hits, "intersect", 1.0, nodes=dS), want)
        bare = cluster_ref.cluster_hits("intersect", 13, *rows, 1.0)
        assert bare["representative"].tolist() == [0, 1, 3, 4, 5, 7, 8, 10, 11]
        _check(c.cluster(hits, "intersect", 1.0, n_nodes=13), bare)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
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
        before = c.pool_stats()["bytes_in_use"]
        for key in KEYS:
            with pytest.raises(ks.KmerseekError) as e:
                c.cluster(hits, key, 0.0, nodes=d_small)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_bad} " in str(e.value), str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster(hits, "intersect", 0.0, n_nodes=small)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_bad} " in str(e.value), str(e.value)
        for key in ("max_containment", "jaccard"):
            with pytest.raises(ks.KmerseekError) as e:
                c.cluster(hits, key, 0.0, nodes=hollow)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_hollow} " in str(e.value), str(e.value)
        c.cluster(hits, "intersect", 0.0, nodes=hollow).free()  # (the key reads no size)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster(hits, "jaccard", 0.0, nodes=dS, n_nodes=n + 1)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "n_nodes" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster(hits, "jaccard", float("nan"), nodes=dS)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "options" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster(hits, "score", 0.0, n_nodes=n)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "score" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.cluster(hits, "jaccard", 0.0, nodes=dS, score=8)  # an explicit key with a column it does not read (never dereferenced)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "score column" in str(e.value)
        with pytest.raises(ValueError):
            c.cluster(hits, "cosine")
        assert c.pool_stats()["bytes_in_use"] == before
        # the context stays usable
        _check(c.cluster(hits, "jaccard", 0.1, nodes=dS), cluster_ref.cluster_hits("jaccard", n, *rows, 0.1, S))


# ---- the input is left alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_input_unchanged_and_scratch_returned(monkeypatch, path):
    n, S, rows = _graph("bridge")
    with ks.Context(0, follow_debug_env=True) as c:
        dS, hits, h = _search(c, S, rows)
        _set_path(monkeypatch, path)
        c.cluster(hits, "jaccard", 0.1, nodes=dS).free()  # (the pool has grown to what the pass needs)
        before = c.pool_stats()["bytes_in_use"]
        cl = c.cluster(hits, "jaccard", 0.1, nodes=dS)
        assert c.pool_stats()["bytes_in_use"] > before
        _check(cl, _want("bridge", "jaccard", 0.1))
        cl.free()
        assert c.pool_stats()["bytes_in_use"] == before
        for g, w in zip(hits.to_host(), h):
            assert np.array_equal(g, w)
        assert hits.count == len(rows[0])
        Sh = dS.to_host()
        for g, w in zip(Sh, S):
            assert np.array_equal(g, w)


# ---- real proteins through wire ------------------------------------------------------------------------------------------------------------
def _lines(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("moltype,ksize,scaled", (("hp", 16, 5), ("protein", 7, 1)))
def test_do_cluster_on_bcl2(monkeypatch, tmp_path, moltype, ksize, scaled, path):
    fasta = tmp_path / BCL2_300
    fasta.write_bytes(open(os.path.join(GOLDEN, BCL2_300), "rb").read())
    with ks.Context(0, follow_debug_env=True) as c:
        sig = wire.sketch(str(fasta), moltype, ksize, scaled, ctx=c)
        names, so, sm, sa, *_ = wire.read_sig_zip(sig)
        assert len(names) == 300
        S = c.sketches_from_host(so, sm, sa, ksize, scaled, moltype)
        h = c.search(c.index_build(S), S).to_host()
        _set_path(monkeypatch, path)
        seen = set()
        for thr in (0.05, 0.3):
            out, sizes = str(tmp_path / f"clusters_{thr}.csv"), str(tmp_path / f"sizes_{thr}.csv")
            want = cluster_ref.cluster_hits("jaccard", 300, *h[:3], thr, (so, sm, sa))
            n_rows = wire.do_cluster(sig, out, ksize, scaled, moltype, "jaccard", thr, sizes_output=sizes, ctx=c)
            rows = wire.cluster_rows(names, want["offsets"], want["members"], want["representative"])
            assert n_rows == want["n_clusters"] == len(rows)
            assert _lines(out) == [wire.CLUSTER_COLUMNS] + [[str(x) for x in r] for r in rows]
            hist = np.unique(np.diff(want["offsets"].astype(np.int64)), return_counts=True)
            assert _lines(sizes) == [["cluster_size", "count"]] + [[str(s), str(k)] for s, k in zip(*[x.tolist() for x in hist])]
            big = str(tmp_path / f"big_{thr}.csv")
            assert wire.do_cluster(sig, big, ksize, scaled, moltype, "jaccard", thr, min_size=2, ctx=c) == sum(r[2] >= 2 for r in rows)
            assert _lines(big) == [wire.CLUSTER_COLUMNS] + [[str(x) for x in r] for r in rows if r[2] >= 2]
            seen.add(want["n_clusters"])
        assert len(seen) == 2 and 1 < min(seen) and max(seen) < 300  # the thresholds cut differently, neither trivially
