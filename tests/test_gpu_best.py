"""GPU: ks_hits_best — the k best rows of every query of a hit list, by a rank key.

Everything is exact, no tolerance: kept rows, rank and src_row are compared as integers with the numpy restatement of
tests/best_ref.py, and every column of the output with input[src_row].  Cases: a ladder of segment lengths around k, the wave's
64 rows and the workgroup path's LDS chunk, on every path (KS_DEBUG_BEST_PATH); one segment of ties only; an uploaded score
column with NaN / infinities / signed zeros; the pass combined with significance, match positions, a thresholded search with
abundance statistics; the edges and refusals; the two wire entry points."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_ref  # noqa: E402
import crafted_sketches as cs  # noqa: E402
from conftest import load_golden  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
BH_CHUNK = 1024  # ks_best.hip: keys of the workgroup path's LDS chunk; a longer segment is streamed from memory
KS = (1, 2, 10, 64, 65, 2 ** 32 - 1)
KEYS = ("intersect", "target_containment", "max_containment", "jaccard")
MODES = (None, "1", "2", "3")  # KS_DEBUG_BEST_PATH: by length, wave only, workgroup only, workgroup with a 64-row chunk
# one query per length: around every k, the wave's 64 rows and the chunk
LADDER = sorted(({k + d for k in KS[:-1] for d in (-1, 0, 1)} | {1, 2, 63, 64, 65, BH_CHUNK - 1, BH_CHUNK, BH_CHUNK + 1, 2 * BH_CHUNK + 3})
                - {0})


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("KS_DEBUG_BEST_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_BEST_PATH", mode)


def _upload(ctx, S, k=10, scaled=1, mol="protein"):
    return ctx.sketches_from_host(S[0], S[1], S[2], k, scaled, mol)


def _ladder():
    """Query 0 and the last query have no row; query j = 1 .. owns 8 private hashes and target t < LADDER[j - 1] holds the first
    1 + (7 t + 3 j) % 8 of them: 8 score values per segment, ties everywhere.  Target t also holds t % 5 hashes of its own, so
    |t| differs and the four computed keys order differently.  -> (Q, T, rows (qid, tid, intersect))"""
    n_q, n_t = len(LADDER) + 2, max(LADDER)
    qs, qh, ts, th = [], [], [], []
    rows = []
    for j in range(n_q):
        own = [1_000_000 + 8 * j + i for i in range(8)]
        qs += [j] * 8; qh += own
        if j == 0 or j == n_q - 1:
            continue
        for t in range(LADDER[j - 1]):
            c = 1 + (7 * t + 3 * j) % 8
            ts += [t] * c; th += own[:c]
            rows.append((j, t, c))
    for t in range(n_t):
        ts += [t] * (t % 5); th += [10 ** 12 + 8 * t + e for e in range(t % 5)]
    Q = cs._csr(qs, qh, [1] * len(qh), n_q)
    T = cs._csr(ts, th, [1] * len(th), n_t)
    cs.check_valid(Q, 1); cs.check_valid(T, 1)
    r = np.array(rows, np.int64)
    return Q, T, (r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint32), r[:, 2].astype(np.uint32))


@pytest.fixture(scope="module")
def ladder():
    return _ladder()


def _check(best, hits_host, want_src, want_rank, extra=()):
    """best: a Hits of best_hits; hits_host: the input's columns (and `extra` further per-row columns with the output's)"""
    got = best.to_host()
    rank, src = best.best_to_host()
    assert best.count == len(want_src), (best.count, len(want_src))
    assert np.array_equal(src, want_src)
    assert np.array_equal(rank, want_rank)
    for g, w in zip(got, hits_host):
        assert g.dtype == w.dtype and np.array_equal(g, w[src])
    order = (got[0].astype(np.uint64) << np.uint64(32)) | got[1].astype(np.uint64)
    assert np.all(order[1:] > order[:-1])
    for g, w in extra:
        assert np.array_equal(g.view(np.uint64), w[src].view(np.uint64))
    assert all(p != 0 for p in best.device_ptrs())


# ---- the ladder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_segment_length_ladder(monkeypatch, ladder, mode):
    Q, T, rows = ladder
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        for g, w in zip(h, rows):
            assert np.array_equal(g, w)
        assert hits.best_to_host() is None
        _set_mode(monkeypatch, mode)
        for key in KEYS:
            score = best_ref.scores(key, h[0], h[1], h[2], Q, T)
            for k in KS:
                kept, rank = best_ref.best(h[0], h[1], score, k)
                src = np.nonzero(kept)[0].astype(np.uint32)
                best = c.best_hits(hits, k, key, dQ, dT)
                _check(best, h, src, rank[src])
                if k >= max(LADDER):  # the input plus the two columns
                    assert best.count == hits.count
                assert (best.n_pair_instances, best.partition_path, best.bucket_posting_bytes, best.has_abund_stats) == \
                       (hits.n_pair_instances, hits.partition_path, hits.bucket_posting_bytes, False)
                best.free()
        assert hits.count == len(rows[0]) and np.array_equal(hits.to_host()[0], rows[0])  # the input is unchanged


# ---- ties only ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_all_ties_keep_the_smallest_tids(monkeypatch, mode):
    n_t = 3 * BH_CHUNK + 1
    Q = cs._csr([0], [77], [1], 1)
    T = cs._csr(list(range(n_t)), [77] * n_t, [1] * n_t, n_t)
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        assert hits.count == n_t and np.array_equal(h[1], np.arange(n_t))
        _set_mode(monkeypatch, mode)
        for key in ("intersect", "jaccard"):
            for k in KS:
                m = min(k, n_t)
                best = c.best_hits(hits, k, key, dQ, dT)
                _check(best, h, np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32))
                best.free()


# ---- an uploaded score column ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_external_score_column(monkeypatch, ladder, mode):
    import torch
    Q, T, rows = ladder
    vals = np.array([np.nan, -np.inf, -1.5, -0.0, 0.0, 1e-300, 2.0, np.inf])
    score = vals[np.random.default_rng(7).integers(0, 8, len(rows[0]))]
    for length in (10, 65, BH_CHUNK + 1):  # segments of NaN only: the k smallest tids
        score[rows[0] == 1 + LADDER.index(length)] = np.nan
    assert np.signbit(score[score == 0.0]).any() and not np.signbit(score[score == 0.0]).all()
    d_score = torch.from_numpy(score).to("cuda:0")
    torch.cuda.synchronize()
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        _set_mode(monkeypatch, mode)
        for k in KS:
            kept, rank = best_ref.best(h[0], h[1], score, k)
            src = np.nonzero(kept)[0].astype(np.uint32)
            best = c.best_hits(hits, k, score=d_score)  # (no sets: the ids are not bounded, the sizes not read)
            _check(best, h, src, rank[src])
            seg = np.nonzero(h[0][src] == 1 + LADDER.index(65))[0]
            assert np.array_equal(h[1][src][seg], np.arange(min(k, 65))) and np.array_equal(rank[src][seg], np.arange(min(k, 65)))
            best.free()
        best = c.best_hits(hits, 3, "score", score=int(d_score.data_ptr()))
        assert best.count == 3 * len(LADDER) - 3  # (lengths 1 and 2 keep all they have)
        best.free()


# ---- with the other passes -------------------------------------------------------------------------------------------------------
def _records(name):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    return ks.pack([s.upper() for _, s in recs])


@pytest.fixture(scope="module")
def bcl2_all_vs_all():
    """BCL2-300 against itself at hp k=16 scaled=5: (context, records, sketches, host copy, index, hits, host copy)"""
    with ks.Context(0) as c:
        res, off = _records(BCL2_300)
        S = c.sketch_batch(res, off, 16, 5, "hp")
        ix = c.index_build(S)
        hits = c.search(ix, S)
        assert hits.count > 300
        yield c, (res, off), S, S.to_host(), ix, hits, hits.to_host()


def test_best_by_jaccard_then_significance(bcl2_all_vs_all):
    c, _, S, Sh, _, hits, h = bcl2_all_vs_all
    src, rank = best_ref.best_rows("jaccard", h[0], h[1], h[2], 10, Sh, Sh)
    assert 0 < len(src) < hits.count
    best = c.best_hits(hits, 10, "jaccard", S, S)
    _check(best, h, src, rank)
    sig_all = c.significance(S, S, hits)
    sig_best = c.significance(S, S, best)
    for g, w in zip(sig_best.to_host(), sig_all.to_host()):
        assert np.array_equal(g.view(np.uint64), w[src].view(np.uint64))
    # best 5 by the tf-idf column as it lies on the device
    tf = sig_all.to_host()[1]
    src5, rank5 = best_ref.best_rows("score", h[0], h[1], h[2], 5, score=tf)
    best5 = c.best_hits(hits, 5, score=sig_all.tf_idf_ptr)
    _check(best5, h, src5, rank5)
    for o in (best5, sig_best, sig_all, best):
        o.free()


def test_match_positions_on_a_best_list(bcl2_all_vs_all):
    c, (res, off), S, Sh, _, hits, h = bcl2_all_vs_all
    best = c.best_hits(hits, 10, "jaccard", S, S)
    src = best.best_to_host()[1].astype(np.int64)
    pos = c.kmer_positions_table(res, off, 16, 5, "hp")
    full = c.match_positions(pos, pos, hits).to_host()
    got = c.match_positions(pos, pos, best).to_host()
    lens = (full[0][1:] - full[0][:-1]).astype(np.int64)
    assert np.array_equal((got[0][1:] - got[0][:-1]).astype(np.int64), lens[src])
    pick = np.concatenate([np.arange(int(full[0][r]), int(full[0][r + 1])) for r in src.tolist()]) if len(src) else np.zeros(0, np.int64)
    assert np.array_equal(got[1], full[1][pick]) and np.array_equal(got[2], full[2][pick])
    for g, w in zip(got[3:], full[3:]):
        assert np.array_equal(g, w[src])
    best.free(); pos.free()


def test_abundance_statistics_are_carried_through(bcl2_all_vs_all):
    c, _, S, Sh, ix, hits, _ = bcl2_all_vs_all
    thin = c.search(ix, S, abund_stats=True, min_containment=0.1)
    assert 0 < thin.count < hits.count and thin.has_abund_stats
    h = thin.to_host()
    m2, ss = thin.abund_stats_to_host()
    src, rank = best_ref.best_rows("jaccard", h[0], h[1], h[2], 5, Sh, Sh)
    best = c.best_hits(thin, 5, "jaccard", S, S)
    assert best.has_abund_stats
    _check(best, h, src, rank)
    g2, gs = best.abund_stats_to_host()
    assert np.array_equal(g2, m2[src]) and np.array_equal(gs.view(np.uint64), ss[src].view(np.uint64))
    best.free(); thin.free()


# ---- edges and refusals ----------------------------------------------------------------------------------------------------------
def test_edges():
    with ks.Context(0) as c:
        T = c.sketch_batch(*synth.proteome(50, stream=931), 10, 1, "protein")
        U = c.sketch_batch(*synth.proteome(20, stream=932), 10, 1, "protein")
        ix = c.index_build(T)
        none = c.search(ix, U)
        assert none.count == 0
        for key in KEYS:
            best = c.best_hits(none, 3, key, U, T)  # no rows: an empty list, not an error
            assert best.count == 0 and [len(x) for x in best.best_to_host()] == [0, 0] and all(len(x) == 0 for x in best.to_host())
        Th = T.to_host()
        n = int(Th[0][1])
        one_q = c.sketches_from_host(np.array([0, n - 5], np.uint64), Th[1][5:n].copy(), np.ones(n - 5, np.uint32), 10, 1, "protein")
        one_t = c.sketches_from_host(Th[0][:2].copy(), Th[1][:n].copy(), Th[2][:n].copy(), 10, 1, "protein")
        one = c.search(c.index_build(one_t), one_q)
        assert one.count == 1
        for key in KEYS:
            best = c.best_hits(one, 1, key, one_q, one_t)
            _check(best, one.to_host(), np.array([0], np.uint32), np.array([0], np.uint32))
        # k larger than every segment: the input plus the two columns
        q_res, q_off = synth.queries(40, *synth.proteome(50, stream=931), stream=933, frac_related=0.6)
        Q = c.sketch_batch(q_res, q_off, 10, 1, "protein")
        hits = c.search(ix, Q)
        h = hits.to_host()
        assert hits.count > 10
        best = c.best_hits(hits, 2 ** 32 - 1, "max_containment", Q, T)
        kept, rank = best_ref.best(h[0], h[1], best_ref.scores("max_containment", h[0], h[1], h[2], Q.to_host(), Th), 2 ** 32 - 1)
        assert kept.all()
        _check(best, h, np.arange(hits.count, dtype=np.uint32), rank)


def test_refusals_leave_the_context_usable():
    with ks.Context(0) as c:
        t_res, t_off = synth.proteome(120, stream=934)
        q_res, q_off = synth.queries(80, t_res, t_off, stream=935, frac_related=0.6)
        T = c.sketch_batch(t_res, t_off, 10, 1, "protein")
        Q = c.sketch_batch(q_res, q_off, 10, 1, "protein")
        fewer = c.sketch_batch(*synth.proteome(7, stream=936), 10, 1, "protein")
        q11 = c.sketch_batch(q_res, q_off, 11, 1, "protein")
        hits = c.search(c.index_build(T), Q)
        h = hits.to_host()
        assert hits.count > 0 and h[1].max() >= 7
        first_bad = int(np.nonzero(h[1] >= 7)[0][0])
        # a target set whose first hit target has an empty sketch
        Th = T.to_host()
        offs = Th[0].copy()
        t_empty = int(h[1][0])
        cut = int(offs[t_empty + 1] - offs[t_empty])
        keep = np.ones(len(Th[1]), bool); keep[int(offs[t_empty]):int(offs[t_empty + 1])] = False
        offs[t_empty + 1:] -= np.uint64(cut)
        hollow = c.sketches_from_host(offs, Th[1][keep], Th[2][keep], 10, 1, "protein")
        before = c.pool_stats()["bytes_in_use"]
        for key in KEYS + ("intersect",):
            with pytest.raises(ks.KmerseekError) as e:
                c.best_hits(hits, 3, key, Q, fewer)  # a target set that is too small
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and f"row {first_bad} " in str(e.value), str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.best_hits(hits, 3, "jaccard", q11, T)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "parameters" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.best_hits(hits, 3, "score")  # KS_BEST_SCORE without a column
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "score" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            c.best_hits(hits, 0)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG
        out = C.c_void_p()
        for words in ((0, 3, 1, 0), (0, 3, 0, 5), (9, 3, 0, 0)):
            st = c._L.ks_hits_best(c._h, hits._h, Q._h, T._h, None, C.byref(_lib.ks_best_opts(*words)), C.byref(out))
            assert st == _lib.KS_ERR_INVALID_ARG and not out.value and "options" in c._L.ks_last_error(c._h).decode()
        with pytest.raises(ks.KmerseekError) as e:
            c.best_hits(hits, 3, "target_containment", targets=hollow)  # |t| = 0 on a row whose key divides by it
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "row 0 " in str(e.value), str(e.value)
        c.best_hits(hits, 3, "intersect", targets=hollow).free()  # (the key does not read |t|)
        assert c.pool_stats()["bytes_in_use"] == before
        # the context stays usable
        src, rank = best_ref.best_rows("jaccard", h[0], h[1], h[2], 3, Q.to_host(), Th)
        _check(c.best_hits(hits, 3, "jaccard", Q, T), h, src, rank)


# ---- wire ----------------------------------------------------------------------------------------------------------------------
def _sig_pair(ctx, tmp_path):
    paths = []
    for name in ("ced9.fasta", BCL2_25):
        dst = tmp_path / name
        dst.write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
        paths.append(wire.sketch(str(dst), "hp", 16, 5, ctx=ctx))
    return paths


def _lines(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_do_manysearch_top_k(tmp_path):
    expected = load_golden("search_expected.json")
    with ks.Context(0) as c:
        q, t = _sig_pair(c, tmp_path)
        full, top = str(tmp_path / "full.csv"), str(tmp_path / "top.csv")
        assert wire.do_manysearch(q, t, full, 16, 5, "hp", ctx=c) == 5
        assert wire.do_manysearch(q, t, top, 16, 5, "hp", ctx=c, top_k=3) == 3
        assert wire.do_manysearch(q, t, str(tmp_path / "zero.csv"), 16, 5, "hp", ctx=c, top_k=0) == 5
    assert _lines(str(tmp_path / "zero.csv")) == _lines(full)
    rows = _lines(full)
    col = rows[0].index("intersect_hashes")
    isect = [int(r[col]) for r in rows[1:]]
    kept, _ = best_ref.best([0] * 5, list(range(5)), np.array(isect, np.float64), 3)  # (one query: CSV order is tid order)
    want = [rows[0]] + [r for r, k in zip(rows[1:], kept.tolist()) if k]
    assert _lines(top) == want
    golden = {r["match_name"]: r for r in expected["manysearch_rows"]}
    name = rows[0].index("match_name")
    for r in want[1:]:
        assert int(golden[r[name]]["intersect_hashes"]) == int(r[col])
    assert sorted(int(golden[r[name]]["intersect_hashes"]) for r in want[1:]) == sorted(int(g["intersect_hashes"]) for g in golden.values())[-3:]


def test_do_multisearch_top_k_by_tf_idf(tmp_path):
    expected = load_golden("multisearch_expected.json")
    with ks.Context(0) as c:
        q, t = _sig_pair(c, tmp_path)
        full, top = str(tmp_path / "full.csv"), str(tmp_path / "top.csv")
        assert wire.do_multisearch(q, t, full, 16, 5, "hp", ctx=c) == 5
        assert wire.do_multisearch(q, t, top, 16, 5, "hp", ctx=c, top_k=2, rank_by="tf_idf_score") == 2
        by_isect = str(tmp_path / "isect.csv")
        assert wire.do_multisearch(q, t, by_isect, 16, 5, "hp", ctx=c, top_k=2) == 2
    rows = _lines(full)
    col = rows[0].index("tf_idf_score")
    tf = np.array([float(r[col]) for r in rows[1:]])
    kept, _ = best_ref.best([0] * 5, list(range(5)), tf, 2)
    want = [rows[0]] + [r for r, k in zip(rows[1:], kept.tolist()) if k]
    assert _lines(top) == want
    golden = {r["match_name"]: r for r in expected["rows"]}
    name = rows[0].index("match_name")
    best2 = sorted(golden.values(), key=lambda r: -float(r["tf_idf_score"]))[:2]
    assert sorted(r[name] for r in want[1:]) == sorted(r["match_name"] for r in best2)
    for r in want[1:]:
        assert float(r[col]) == float(golden[r[name]]["tf_idf_score"])
    icol = rows[0].index("intersect_hashes")
    kept, _ = best_ref.best([0] * 5, list(range(5)), np.array([float(r[icol]) for r in rows[1:]]), 2)
    assert _lines(by_isect) == [rows[0]] + [r for r, k in zip(rows[1:], kept.tolist()) if k]
