"""GPU: ks_hits_gather — per query the greedy non-redundant targets of a hit list.

Everything is exact, no tolerance: kept rows, rank, src_row and the three gather columns are compared as integers with the numpy
restatement of tests/gather_ref.py, every other column with input[src_row].  The hits always come from a real search, so
`intersect` is the library's own.  Every gather runs on each value of KS_DEBUG_GATHER_PATH (unset: segments by length; 1 every
segment by a wave; 2 by a workgroup; 3 by a workgroup whose live bitmap holds 256 positions in LDS and lies in global memory
above) and must give the same output on all four."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import gather_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
MODES = (None, "1", "2", "3")
KNOB = "KS_DEBUG_GATHER_PATH"
# (rows of the segment, hashes of its query): both sides of the wave's 64 rows, of the bitmap's words and of the 256 LDS
# positions of path 3; every length of {1, 2, 63, 64, 65, 255, 256, 257, 600} and every size of {1, 63, 64, 65, 255, 256, 257, 600}
LADDER = ((1, 600), (2, 257), (63, 256), (64, 255), (65, 65), (255, 64), (256, 63), (257, 1), (600, 600), (64, 64), (600, 1), (1, 1))


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, mode)


def _upload(ctx, S, k=10, scaled=1, mol="protein"):
    return ctx.sketches_from_host(S[0], S[1], S[2], k, scaled, mol)


def _check(g, hits, h, want, stats=None):
    """g: a Hits of Context.gather; hits / h: its input and the input's host columns; want: gather_ref's result"""
    src_w, rank_w, uniq_w, rem_w, uw_w = want
    got = g.to_host()
    rank, src = g.best_to_host()
    uniq, rem, uw = g.gather_to_host()
    assert g.count == len(src_w), (g.count, len(src_w))
    assert np.array_equal(src, src_w) and np.array_equal(rank, rank_w)
    assert np.array_equal(uniq, uniq_w) and np.array_equal(rem, rem_w)
    assert uw.dtype == np.uint64 and np.array_equal(uw, uw_w)
    for a, b in zip(got, h):
        assert a.dtype == b.dtype and np.array_equal(a, b[src])
    order = (got[0].astype(np.uint64) << np.uint64(32)) | got[1].astype(np.uint64)
    assert np.all(order[1:] > order[:-1])
    assert (g.n_pair_instances, g.partition_path, g.bucket_posting_bytes, g.has_abund_stats) == \
           (hits.n_pair_instances, hits.partition_path, hits.bucket_posting_bytes, hits.has_abund_stats)
    if stats is not None:
        m2, ss = g.abund_stats_to_host()
        assert np.array_equal(m2, stats[0][src]) and np.array_equal(ss.view(np.uint64), stats[1][src].view(np.uint64))
    L = g._ctx._L
    assert all(p != 0 for p in g.device_ptrs())
    assert all(f(g._h) for f in (L.ks_hits_device_rank, L.ks_hits_device_src_row, L.ks_hits_device_unique_intersect,
                                 L.ks_hits_device_remaining, L.ks_hits_device_unique_weighted))


def _on_every_path(monkeypatch, c, hits, h, dQ, dT, want, stats=None, **opts):
    try:
        for mode in MODES:
            _set_mode(monkeypatch, mode)
            g = c.gather(hits, dQ, dT, **opts)
            _check(g, hits, h, want, stats)
            g.free()
    finally:
        _set_mode(monkeypatch, None)


# ---- segments whose answer is known by construction -----------------------------------------------------------------------------
def _hand_made():
    """query 0: t0 inside t1 inside q.  1: no row.  2: three disjoint targets of 3, 5 and 4 hashes.  3: A = 10 hashes, B = 9 of
    which 8 are A's, C = 5 disjoint.  4: two identical targets.  5 (the last): one target.  Query q's hashes: 1000 q + 1 .."""
    def H(q, idx):
        return [1000 * q + 1 + i for i in idx]
    targets = [H(0, range(0, 4)), H(0, range(0, 9)),                 # t0, t1
               H(2, range(0, 3)), H(2, range(3, 8)), H(2, range(8, 12)),  # t2 t3 t4
               H(3, range(0, 10)), H(3, list(range(2, 10)) + [10]), H(3, range(11, 16)),  # A B C
               H(4, range(0, 6)), H(4, range(0, 6)),                 # t8 == t9
               H(5, range(1, 3)) + [999999]]                         # t10
    sizes = [12, 7, 14, 18, 8, 4]
    qs, qh, qa = [], [], []
    for q, n in enumerate(sizes):
        qs += [q] * n; qh += H(q, range(n)); qa += [q + 1 + i for i in range(n)]
    ts = [t for t, x in enumerate(targets) for _ in x]
    th = [v for x in targets for v in x]
    Q = cs._csr(qs, qh, qa, len(sizes))
    T = cs._csr(ts, th, [1] * len(th), len(targets))
    cs.check_valid(Q, 1); cs.check_valid(T, 1)

    def w(q, idx):  # the query's abundances over positions idx
        return sum(q + 1 + i for i in idx)
    # (qid, tid) -> (rank, unique_intersect, remaining, unique_weighted); absent: dropped
    want = {(0, 1): (0, 9, 3, w(0, range(0, 9))),
            (2, 3): (0, 5, 9, w(2, range(3, 8))), (2, 4): (1, 4, 5, w(2, range(8, 12))), (2, 2): (2, 3, 2, w(2, range(0, 3))),
            (3, 5): (0, 10, 8, w(3, range(0, 10))), (3, 7): (1, 5, 3, w(3, range(11, 16))), (3, 6): (2, 1, 2, w(3, [10])),
            (4, 8): (0, 6, 2, w(4, range(0, 6))),
            (5, 10): (0, 2, 2, w(5, range(1, 3)))}
    return Q, T, want


def test_hand_made_segments(monkeypatch):
    Q, T, want = _hand_made()
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        assert list(zip(h[0].tolist(), h[1].tolist())) == [(0, 0), (0, 1), (2, 2), (2, 3), (2, 4), (3, 5), (3, 6), (3, 7), (4, 8), (4, 9), (5, 10)]
        assert hits.gather_to_host() is None
        ref = gather_ref.gather(Q, T, h[0], h[1], h[2])
        kept = [(int(h[0][r]), int(h[1][r])) for r in ref[0].tolist()]
        assert {k: (int(a), int(b), int(cc), int(d)) for k, a, b, cc, d in zip(kept, ref[1], ref[2], ref[3], ref[4])} == want
        _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref)
        assert np.array_equal(hits.to_host()[2], h[2]) and hits.count == 11  # the input is unchanged


# ---- the ladder ------------------------------------------------------------------------------------------------------------------
def _ladder():
    """Query j holds LADDER[j][1] hashes of its own, and target t < LADDER[j][0] a window of them: 1 + (3 t + j) % 9 hashes (at
    most all) from position 7 t on, wrapping round — overlapping windows: many rounds, many rows that die at 0, ties everywhere.
    Query abundances are mixed."""
    n_q, n_t = len(LADDER), max(l for l, _ in LADDER)
    qs, qh, qa, ts, th = [], [], [], [], []
    for j, (length, nq) in enumerate(LADDER):
        own = [10_000_000 * (j + 1) + 7 * i for i in range(nq)]
        qs += [j] * nq; qh += own; qa += [1 + (i * i + j) % 11 for i in range(nq)]
        for t in range(length):
            wd = min(nq, 1 + (3 * t + j) % 9)
            ts += [t] * wd; th += [own[(7 * t + i) % nq] for i in range(wd)]
    Q = cs._csr(qs, qh, qa, n_q)
    T = cs._csr(ts, th, [1] * len(th), n_t)
    cs.check_valid(Q, 1); cs.check_valid(T, 1)
    return Q, T


@pytest.fixture(scope="module")
def ladder():
    """(Q, T, the reference's result per (min_unique, max_results)) — the rows are the search's, checked against ref_join"""
    Q, T = _ladder()
    rows = cs.ref_join(T, Q)
    assert np.bincount(rows[0].astype(np.int64)).tolist() == [l for l, _ in LADDER]
    opts = [(1, 0), (0, 0), (2, 0), (5, 0), (1, 1), (1, 2), (1, 3)]
    return Q, T, rows, {o: gather_ref.gather(Q, T, rows[0], rows[1], rows[2], *o) for o in opts}


def test_segment_length_ladder(monkeypatch, ladder):
    Q, T, rows, refs = ladder
    ref = refs[(1, 0)]
    rounds = np.bincount(rows[0][ref[0]].astype(np.int64), minlength=len(LADDER))
    assert rounds.max() > 64 and rounds.min() == 1 and len(ref[0]) < len(rows[0]) // 2  # many rounds, and many rows never kept
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        for a, b in zip(h, rows):
            assert np.array_equal(a, b)
        _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref)


def test_options(monkeypatch, ladder):
    Q, T, rows, refs = ladder
    assert np.array_equal(refs[(0, 0)][0], refs[(1, 0)][0])
    assert len(refs[(5, 0)][0]) < len(refs[(2, 0)][0]) < len(refs[(1, 0)][0])
    assert len(refs[(1, 1)][0]) == len(LADDER) < len(refs[(1, 2)][0]) < len(refs[(1, 3)][0]) < len(refs[(1, 0)][0])
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        for (min_unique, max_results), ref in refs.items():
            _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref, min_unique=min_unique, max_results=max_results)
        # max_results = 1 keeps the rows of the best hit by intersect
        best = c.best_hits(hits, 1, "intersect")
        one = c.gather(hits, dQ, dT, max_results=1)
        assert np.array_equal(one.best_to_host()[1], best.best_to_host()[1]) and one.count == len(LADDER)
        for a, b in zip(one.to_host(), best.to_host()):
            assert np.array_equal(a, b)
        assert np.array_equal(one.gather_to_host()[0], one.to_host()[2])  # the first pick adds all it shares
        assert best.gather_to_host() is None  # a pass that copies rows does not carry the gather columns


def test_wide_abundances(monkeypatch):
    """5 shared hashes of abundance 2^32 - 1 in the query: unique_weighted = 5 (2^32 - 1) > 2^32, exactly"""
    top = cs.U32_MAX
    Q = cs._csr([0] * 8, [11, 12, 13, 14, 15, 16, 17, 18], [top] * 5 + [1, 2, 3], 1)
    T = cs._csr([0] * 5 + [1] * 4, [11, 12, 13, 14, 15, 14, 15, 16, 17], [1] * 9, 2)
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        ref = gather_ref.gather(Q, T, h[0], h[1], h[2])
        assert ref[4].tolist() == [5 * top, 3] and ref[2].tolist() == [5, 2] and ref[3].tolist() == [3, 1]
        _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref)


# ---- the edges of the shared-hash walk (ks_shared_walk_lane / _wave: the significance pass's walk) -----------------------------------
def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _searched(c, Q, T):
    """(the uploaded sets, the search's hits, their host columns) — the rows are ref_join's"""
    dQ, dT = _upload(c, Q), _upload(c, T)
    hits = c.search(c.index_build(dT), dQ)
    h = hits.to_host()
    for a, b in zip(h, cs.ref_join(T, Q)):
        assert np.array_equal(a, b)
    return dQ, dT, hits, h


def test_row_length_edges(monkeypatch):
    """crafted_sketches.row_lengths: query 0 (193 hashes) shares 1, 2, 63, 64, 65, 127, 128, 129, 192 and 193 hashes with its ten
    targets — the count at every chunk edge, a miscount is a refusal; query 1 (64 hashes) is the walked run of both its rows,
    one by a lane (|q| + |t| = 128) and one by a wave (129), and its second pick counts positions of both."""
    name, k, scaled, mol, T, Q = cs.family("row_lengths")
    assert (k, scaled, mol) == (10, 1, "protein")
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT, hits, h = _searched(c, Q, T)
        assert h[0].tolist() == [0] * 10 + [1, 1] and h[2].tolist() == list(cs.ROW_SHARED) + [40, 41]
        sizes_q, sizes_t = np.diff(Q[0]).astype(np.int64), np.diff(T[0]).astype(np.int64)
        assert [int(sizes_q[1] + sizes_t[t]) for t in (10, 11)] == [cs.SG_CUT, cs.SG_CUT + 1] and sizes_q[1] <= sizes_t[10:].min()
        ref = gather_ref.gather(Q, T, h[0], h[1], h[2])
        assert _same(ref, gather_ref.gather_sets(Q, T, h[0], h[1], h[2]))
        # in row order: row 9 explains query 0 at once; query 1 takes row 11 (41 shared) first, then row 10 adds 11
        assert [x.tolist() for x in ref[:4]] == [[9, 10, 11], [0, 1, 0], [193, 11, 41], [0, 12, 23]]
        _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref)


def _staggered():
    """One query of 193 hashes h[0 .. 193) and six targets: the windows h[0:65], h[1:65], h[2:65], h[64:193], h[65:193], h[66:193],
    each with three hashes of its own above every h: target hashes ascend, so a window's hashes sit in the lanes 0 .. of its walk."""
    h = [2 * (1000 + 7 * i) for i in range(193)]
    windows = [(0, 65), (1, 65), (2, 65), (64, 193), (65, 193), (66, 193)]
    ts, th = [], []
    for t, (a, b) in enumerate(windows):
        own = [h[-1] + 1 + 2 * (3 * t + j) for j in range(3)]
        ts += [t] * (b - a + 3); th += h[a:b] + own
    Q = cs._csr([0] * 193, h, [1 + (i * i) % 13 for i in range(193)], 1)
    T = cs._csr(ts, th, [1] * len(th), len(windows))
    cs.check_valid(Q, 1); cs.check_valid(T, 1)
    return Q, T, windows


def test_staggered_windows_around_a_chunk_edge(monkeypatch):
    """Every row takes the wave walk (|q| + |t| > GA_CUT) and searches the query (|t| < |q|).  The first pick is h[64:193], the
    second what h[0:65] has left: 64 — one more or less if the position written for lane 63 of a chunk or lane 0 of the next is
    off by one on either side.  Then nothing is left."""
    Q, T, windows = _staggered()
    assert all(n < 193 for n in np.diff(T[0]).tolist())
    with ks.Context(0, follow_debug_env=True) as c:
        dQ, dT, hits, h = _searched(c, Q, T)
        assert h[1].tolist() == [0, 1, 2, 3, 4, 5] and h[2].tolist() == [b - a for a, b in windows] == [65, 64, 63, 129, 128, 127]
        ref = gather_ref.gather(Q, T, h[0], h[1], h[2])
        assert _same(ref, gather_ref.gather_sets(Q, T, h[0], h[1], h[2]))
        assert [x.tolist() for x in ref[:4]] == [[0, 3], [1, 0], [64, 129], [0, 64]]
        assert ref[4].tolist() == [int(Q[2][:64].sum()), int(Q[2][64:].sum())]
        _on_every_path(monkeypatch, c, hits, h, dQ, dT, ref)


# ---- real data, and inputs from other passes --------------------------------------------------------------------------------------
def _records(name):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    return ks.pack([s.upper() for _, s in recs])


@pytest.fixture(scope="module")
def bcl2():
    """the 25 golden BCL2 proteins against the BCL2 file, hp k=16 scaled=5"""
    with ks.Context(0, follow_debug_env=True) as c:
        q_rec, t_rec = _records(BCL2_25), _records(BCL2_300)
        Q = c.sketch_batch(*q_rec, 16, 5, "hp")
        T = c.sketch_batch(*t_rec, 16, 5, "hp")
        ix = c.index_build(T)
        hits = c.search(ix, Q)
        assert hits.count > 100
        yield c, q_rec, t_rec, Q, T, Q.to_host(), T.to_host(), ix, hits, hits.to_host()


def test_bcl2_against_the_reference(monkeypatch, bcl2):
    c, _, _, Q, T, Qh, Th, _, hits, h = bcl2
    ref = gather_ref.gather(Qh, Th, h[0], h[1], h[2])
    assert 25 <= len(ref[0]) < hits.count  # (every query is in the target file too: its own row explains it at once)
    _on_every_path(monkeypatch, c, hits, h, Q, T, ref)
    ref3 = gather_ref.gather(Qh, Th, h[0], h[1], h[2], 3, 4)
    _on_every_path(monkeypatch, c, hits, h, Q, T, ref3, min_unique=3, max_results=4)


def test_thresholded_search_with_statistics(monkeypatch, bcl2):
    c, _, _, Q, T, Qh, Th, ix, hits, _ = bcl2
    thin = c.search(ix, Q, abund_stats=True, min_containment=0.1)
    assert 0 < thin.count < hits.count and thin.has_abund_stats
    h = thin.to_host()
    ref = gather_ref.gather(Qh, Th, h[0], h[1], h[2])
    _on_every_path(monkeypatch, c, thin, h, Q, T, ref, stats=thin.abund_stats_to_host())
    thin.free()


def test_best_hits_list_as_input_and_output_into_other_passes(monkeypatch, bcl2):
    c, q_rec, t_rec, Q, T, Qh, Th, _, hits, _ = bcl2
    best = c.best_hits(hits, 10, "intersect")
    h = best.to_host()
    assert 0 < best.count < hits.count
    ref = gather_ref.gather(Qh, Th, h[0], h[1], h[2])
    _on_every_path(monkeypatch, c, best, h, Q, T, ref)
    g = c.gather(best, Q, T)
    src = g.best_to_host()[1].astype(np.int64)
    sig_all, sig_g = c.significance(Q, T, best), c.significance(Q, T, g)
    for a, b in zip(sig_g.to_host(), sig_all.to_host()):
        assert np.array_equal(a.view(np.uint64), b[src].view(np.uint64))
    qp, tp = c.kmer_positions_table(*q_rec, 16, 5, "hp"), c.kmer_positions_table(*t_rec, 16, 5, "hp")
    full, got = c.match_positions(qp, tp, best).to_host(), c.match_positions(qp, tp, g).to_host()
    assert np.array_equal(np.diff(got[0].astype(np.int64)), np.diff(full[0].astype(np.int64))[src])
    again = c.best_hits(g, 2, "intersect")  # the output is a hit list like any other
    assert 0 < again.count <= g.count and again.gather_to_host() is None
    for o in (again, qp, tp, sig_g, sig_all, g, best):
        o.free()


def _concat(a, b):
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1][1:] + a[1][-1]])


def test_seeded_random_families(monkeypatch):
    """about 2k x 2k, protein k=7 scaled=1: the targets are 400 proteins and four mutated copies of each, the queries mutated
    copies of the targets — every query meets a family of redundant targets"""
    base = synth.proteome(400, stream=941, hi=400)
    T_rec = _concat(base, synth.queries(1600, *base, stream=942, frac_related=1.0, p_sub=0.05))
    Q_rec = synth.queries(2000, *T_rec, stream=943, frac_related=0.8, p_sub=0.05)
    with ks.Context(0, follow_debug_env=True) as c:
        T = c.sketch_batch(*T_rec, 7, 1, "protein")
        Q = c.sketch_batch(*Q_rec, 7, 1, "protein")
        hits = c.search(c.index_build(T), Q)
        h = hits.to_host()
        ref = gather_ref.gather(Q.to_host(), T.to_host(), h[0], h[1], h[2])
        print(f"rows {hits.count}, kept {len(ref[0])}, most rounds {int(ref[1].max()) + 1}")
        assert hits.count > 4000 and len(ref[0]) < hits.count and ref[1].max() >= 2
        _on_every_path(monkeypatch, c, hits, h, Q, T, ref)


# ---- edges and refusals -------------------------------------------------------------------------------------------------------
def test_empty_hit_list(monkeypatch):
    with ks.Context(0, follow_debug_env=True) as c:
        T = c.sketch_batch(*synth.proteome(50, stream=931), 10, 1, "protein")
        U = c.sketch_batch(*synth.proteome(20, stream=932), 10, 1, "protein")
        none = c.search(c.index_build(T), U)
        assert none.count == 0
        for mode in MODES:
            _set_mode(monkeypatch, mode)
            g = c.gather(none, U, T)
            assert g.count == 0 and all(len(x) == 0 for x in g.to_host())
            assert [len(x) for x in g.best_to_host()] == [0, 0] and [len(x) for x in g.gather_to_host()] == [0, 0, 0]
            assert c._L.ks_hits_device_unique_intersect(g._h) and c._L.ks_hits_device_unique_weighted(g._h)
            g.free()
        _set_mode(monkeypatch, None)


def test_refusals_leave_the_context_usable():
    Q, T, _ = _hand_made()
    with ks.Context(0) as c:
        dQ, dT = _upload(c, Q), _upload(c, T)
        hits = c.search(c.index_build(dT), dQ)
        h = hits.to_host()
        ref = gather_ref.gather(Q, T, h[0], h[1], h[2])
        # targets 5 and 6 (A and B of query 3) change places: row 5 (3, 5) then shares 9 hashes where the list says 10
        other = [5 if t == 6 else 6 if t == 5 else t for t in np.repeat(np.arange(11), np.diff(T[0]).astype(np.int64)).tolist()]
        swapped = _upload(c, cs._csr(other, T[1], T[2], 11))
        n8 = int(T[0][8])
        fewer = c.sketches_from_host(T[0][:9].copy(), T[1][:n8].copy(), T[2][:n8].copy(), 10, 1, "protein")  # targets 0 .. 7
        q11 = c.sketches_from_host(Q[0], Q[1], Q[2], 11, 1, "protein")
        before = c.pool_stats()["bytes_in_use"]

        def usable():
            g = c.gather(hits, dQ, dT)
            _check(g, hits, h, ref)
            g.free()

        out = C.c_void_p()
        for words in ((1, 0, 1, 0), (1, 0, 0, 5)):
            st = c._L.ks_hits_gather(c._h, hits._h, dQ._h, dT._h, C.byref(_lib.ks_gather_opts(*words)), C.byref(out))
            assert st == _lib.KS_ERR_INVALID_ARG and not out.value and "options" in c._L.ks_last_error(c._h).decode()
            usable()
        for args in ((hits._h, None, dT._h), (hits._h, dQ._h, None), (None, dQ._h, dT._h)):
            assert c._L.ks_hits_gather(c._h, *args, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG and not out.value
            assert "NULL" in c._L.ks_last_error(c._h).decode()
        usable()
        with pytest.raises(ks.KmerseekError) as e:
            c.gather(hits, q11, dT)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "parameters" in str(e.value)
        usable()
        with pytest.raises(ks.KmerseekError) as e:
            c.gather(hits, dQ, swapped)  # hits searched on another target set
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "row 5 " in str(e.value), str(e.value)
        usable()
        with pytest.raises(ks.KmerseekError) as e:
            c.gather(hits, dQ, fewer)  # a target set shorter than the largest tid: rows 8 .. 10 name targets 8 .. 10
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "row 8 " in str(e.value), str(e.value)
        usable()
        with pytest.raises(ks.KmerseekError) as e:
            c.gather(hits, fewer, dT)  # a query set of 8 sequences is enough (queries 0 .. 5) but not the hits' own
        assert e.value.status == _lib.KS_ERR_INVALID_ARG
        usable()
        assert c.pool_stats()["bytes_in_use"] == before
        # an opts pointer of NULL: the defaults
        assert c._L.ks_hits_gather(c._h, hits._h, dQ._h, dT._h, None, C.byref(out)) == _lib.KS_OK and out.value
        g = ks.engine.Hits(c, out)
        _check(g, hits, h, ref)
        g.free()


# ---- wire ----------------------------------------------------------------------------------------------------------------------
def test_do_gather_on_the_golden_pair(tmp_path):
    with ks.Context(0) as c:
        paths = []
        for name in (BCL2_25, BCL2_300):
            dst = tmp_path / name
            dst.write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
            paths.append(wire.sketch(str(dst), "hp", 16, 5, ctx=c))
        q, t = paths
        out, out2 = str(tmp_path / "gather.csv"), str(tmp_path / "gather2.csv")
        n = wire.do_gather(q, t, out, 16, 5, "hp", ctx=c)
        n2 = wire.do_gather(q, t, out2, 16, 5, "hp", min_unique=2, max_results=3, min_containment=0.1, ctx=c)
    qn, qo, qm, qa, *_ = wire.read_sig_zip(q)
    tn, to, tm, ta, *_ = wire.read_sig_zip(t)
    Q, T = (qo, qm, qa), (to, tm, ta)
    rows = cs.ref_join(T, Q)

    def want(rows, *opts):
        src, rank, uniq, rem, uw = gather_ref.gather(Q, T, rows[0], rows[1], rows[2], *opts)
        text = wire.gather_rows(qn, qo, qm, qa, tn, to, tm, tuple(x[src] for x in rows), rank, (uniq, rem, uw), 16, 5, "hp")
        return [wire.GATHER_COLUMNS] + [[str(r[k]) for k in wire.GATHER_COLUMNS] for r in text]

    def lines(path):
        with open(path, newline="") as f:
            return list(csv.reader(f))

    assert lines(out) == want(rows) and n == len(lines(out)) - 1 >= 25
    thin = tuple(x[cs.keep(rows, Q, 0.1)] for x in rows)
    assert lines(out2) == want(thin, 2, 3) and 0 < n2 == len(lines(out2)) - 1 <= n
    body = lines(out)[1:]  # ordered by (query, rank): a rank is 0, or follows its query's previous one
    assert all(int(r[4]) == 0 or (r[1] == p[1] and int(r[4]) == int(p[4]) + 1) for p, r in zip([body[0]] + body, body))
