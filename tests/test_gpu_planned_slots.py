"""GPU: CSR slots taken from the tile plan (scaled = 1, packed tiles) against the oracle and against the look-back path.

At scaled = 1 a sequence's CSR slot is as long as its k-mer windows, so the plan pass hands every tile the start of its slots
(`tile_wbase`) and no tile waits for its predecessors.  Every case here runs the same call twice on one context — as it is, and
under KS_DEBUG_TILE_LOOKBACK=1 — and wants the oracle's sketches from both, equal `n_hashes`, and the path counter
(`sketch_stats(paths=True)["planned_slots"]`) to say which path ran.  Where no sequence repeats a k-mer the raw device offsets
must be cumsum(max(len - k + 1, 0)): that checks the plan's bases directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import synth
from oracle import oracle

PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
PK_MAX_LEN = 4064  # longest sequence a packed tile holds (ks_sketch.hip)


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    res = np.concatenate(seqs).astype(np.uint8) if len(seqs) and int(offs[-1]) else np.zeros(0, np.uint8)
    return res, offs


def _random(lens, seed):
    rng = np.random.default_rng(seed)
    return _pack([rng.choice(PROTEIN, int(L)).astype(np.uint8) for L in lens])


def _proteins(seed, n=200):
    rng = np.random.default_rng(seed)
    return list(np.clip(np.rint(rng.lognormal(np.log(280.0), 0.4, n)), 30, 1500).astype(int))


def _with_repeats(seed, n=200):
    """homopolymer and tandem runs inside ordinary proteins: kept > distinct, slots longer than counts"""
    rng = np.random.default_rng(seed)
    seqs = []
    for L in _proteins(seed, n):
        s = rng.choice(PROTEIN, L).astype(np.uint8)
        kind = int(rng.integers(0, 3))
        if kind == 0 and L > 60:
            s[10:10 + L // 3] = rng.choice(PROTEIN)
        elif kind == 1 and L > 60:
            unit = rng.choice(PROTEIN, int(rng.integers(2, 9)))
            m = L // 2
            s[5:5 + m] = np.tile(unit, m // len(unit) + 1)[:m]
        seqs.append(s)
    return _pack(seqs)


def _windows_cumsum(offs, k):
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    out = np.zeros(len(offs), np.int64)
    np.cumsum(np.maximum(lens - k + 1, 0), out=out[1:])
    return out


def _maxlen(offs):
    return int((offs[1:] - offs[:-1]).max()) if len(offs) > 1 else 0


def _eq(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{what}: array {i} differs"


def _planned(ctx):
    return ctx.sketch_stats(paths=True)["planned_slots"]


def _both_paths(monkeypatch, res, offs, k, scaled, mol, hints=(0,), planned=True, env=None, raw=True):
    """The batch through sketch_batch_device on either path, for every max_seq_len hint; returns the oracle's sketches."""
    import torch
    from kmerseek_amd import dist as ksd
    want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
    n = len(offs) - 1
    no_repeats = not np.any(want[2] > 1)
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        d_res, d_off = ctx.to_device(res if len(res) else np.zeros(16, np.uint8)), ctx.to_device(offs)
        for hint in hints:
            what = f"{mol} k={k} scaled={scaled} hint={hint}"
            p0 = _planned(ctx)
            S = ctx.sketch_batch_device(d_res.ptr, d_off.ptr, n, len(res), k, scaled, mol, max_seq_len=hint)
            p1 = _planned(ctx)
            assert (p1 > p0) == planned, (what, p0, p1)
            monkeypatch.setenv("KS_DEBUG_TILE_LOOKBACK", "1")
            L = ctx.sketch_batch_device(d_res.ptr, d_off.ptr, n, len(res), k, scaled, mol, max_seq_len=hint)
            monkeypatch.delenv("KS_DEBUG_TILE_LOOKBACK")
            assert _planned(ctx) == p1, (what, "the forced look-back took the planned path")
            assert S.n_hashes == L.n_hashes == len(want[1]), what
            if raw and planned and no_repeats and S.n_hashes:
                cols = ksd.sketch_columns_as_torch(S, torch.device("cuda:0"))
                ctx.synchronize()
                torch.cuda.synchronize()
                assert np.array_equal(cols[0].cpu().numpy(), _windows_cumsum(offs, k)), f"{what}: raw offsets"
                del cols
            got_s, got_l = S.to_host(), L.to_host()
            _eq(got_s, want, what + " planned")
            _eq(got_l, want, what + " look-back")
            S.free(); L.free()
        st = ctx.sketch_stats()
        assert st["ticket_fallbacks"] == 0 and st["uses_ticket"] == 0, st
        d_res.free(); d_off.free()
    finally:
        ctx.close()
    return want


# (moltype, k): the folded kernels (protein 10 / 7), the k < 8 walk (hp 5), the generic kernel (protein 12)
KERNELS = [("protein", 10), ("protein", 7), ("hp", 5), ("protein", 12)]


@pytest.mark.parametrize("mol,k", KERNELS)
def test_proteins_across_tiles_and_chunks(monkeypatch, mol, k):
    """200 proteins of ~300 aa: four chunks of 64 and a dozen tiles, so bases cross tile and chunk boundaries.  With and
    without max_seq_len (pk_bound with surplus tiles that return at once; the read-back plan)."""
    lens = _proteins(11)
    res, offs = _random(lens, 11)
    _both_paths(monkeypatch, res, offs, k, 1, mol, hints=(0, _maxlen(offs)))


@pytest.mark.parametrize("mol,k", KERNELS)
@pytest.mark.parametrize("empty_ends", [False, True])
def test_sequences_without_windows_interleaved(monkeypatch, mol, k, empty_ends):
    """Lengths 0, k - 1 and k among the proteins (a sequence shorter than k counts 0 windows: a real prefix sum, no closed
    form over residue offsets); once with the first and the last sequence empty."""
    rng = np.random.default_rng(12)
    lens = []
    for L in _proteins(12):
        lens.append(L)
        lens.append(int(rng.choice([0, k - 1, k])))
    if empty_ends:
        lens = [0] + lens + [0]
    res, offs = _random(lens, 12)
    _both_paths(monkeypatch, res, offs, k, 1, mol, hints=(0, _maxlen(offs)))


@pytest.mark.parametrize("mol,k", [("protein", 10), ("hp", 5)])
@pytest.mark.parametrize("lo,hi,homopolymers", [(20, 40, False), (10, 15, False), (10, 15, True)])
def test_many_short_sequences(monkeypatch, mol, k, lo, hi, homopolymers):
    """40,000 sequences of 20-40 aa: chunks of 256, tiles of well over a hundred sequences.  At 10-15 aa a whole chunk of 256
    fits one tile, more than the 254 boundaries a tile stages in LDS (`!in_lds`: offsets and counts come from the bucket
    starts); with a homopolymer every 50 sequences those tiles also hold repeats and leave sequence by sequence."""
    rng = np.random.default_rng(13)
    seqs = [rng.choice(PROTEIN, int(L)).astype(np.uint8) for L in rng.integers(lo, hi + 1, 40000)]
    if homopolymers:
        for i in range(7, len(seqs), 50):
            seqs[i][:] = PROTEIN[i % 20]
    res, offs = _pack(seqs)
    _both_paths(monkeypatch, res, offs, k, 1, mol, hints=(0, hi))


@pytest.mark.parametrize("mol,k", KERNELS)
def test_repeated_kmers_leave_gapped_slots(monkeypatch, mol, k):
    """Homopolymer and tandem runs: slots are longer than counts, `gapped` is set, and the index build and union() run from
    the gapped object."""
    res, offs = _with_repeats(14)
    want = _both_paths(monkeypatch, res, offs, k, 1, mol, hints=(0, _maxlen(offs)))
    assert np.any(want[2] > 1), "the batch must repeat k-mers inside its sequences"
    ctx = ks.Context(0)
    try:
        S = ctx.sketch_batch(res, offs, k, 1, mol)
        assert _planned(ctx) == 1 and S.n_hashes == len(want[1])
        ix = ctx.index_build(S)  # (gapped slots: made dense on the way)
        u, inv = np.unique(want[1], return_inverse=True)
        U = S.union().to_host()
        assert np.array_equal(U[0], np.array([0, len(u)], np.uint64)) and np.array_equal(U[1], u)
        assert np.array_equal(U[2].astype(np.int64), np.bincount(inv, weights=want[2].astype(np.float64)).astype(np.int64))
        n = len(offs) - 1
        qo = want[0][n - 30:] - want[0][n - 30]
        qm, qa = want[1][int(want[0][n - 30]):], want[2][int(want[0][n - 30]):]
        H = ctx.search(ix, ctx.sketches_from_host(qo, qm, qa, k, 1, mol)).to_host()
        _eq(H, oracle.manysearch(qo, qm, *want, n_threads=8), "hits against the index of the gapped sketches")
    finally:
        ctx.close()


@pytest.mark.parametrize("mol,k", [("protein", 10), ("hp", 5)])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("repeats", [False, True])
def test_long_and_medium_sequences_ride_along(monkeypatch, mol, k, where, repeats):
    """One sequence longer than PK_MAX_LEN (the deferred tail of a tile: its term in the tile's offsets is its window count)
    and one of medium length among short ones; the long one first / last in its chunk of 64.  With repeats inside the long
    one its slot is longer than its run."""
    rng = np.random.default_rng(15)
    seqs = [rng.choice(PROTEIN, int(L)).astype(np.uint8) for L in rng.integers(30, 400, 128)]
    long_seq = rng.choice(PROTEIN, PK_MAX_LEN + 900).astype(np.uint8)
    if repeats:
        long_seq[100:1500] = PROTEIN[3]
    seqs[64 if where == "first" else 127] = long_seq
    seqs[20] = rng.choice(PROTEIN, 3000).astype(np.uint8)
    res, offs = _pack(seqs)
    _both_paths(monkeypatch, res, offs, k, 1, mol, hints=(0, _maxlen(offs)))


def test_thresholded_sketch_keeps_the_lookback(monkeypatch):
    """dayhoff k=16 scaled=5 (the compacting tiles) and the same without them (a thresholded plain launch): the counter shows
    the look-back path."""
    res, offs = _random(_proteins(16), 16)
    _both_paths(monkeypatch, res, offs, 16, 5, "dayhoff", hints=(0, _maxlen(offs)), planned=False)
    _both_paths(monkeypatch, res, offs, 16, 5, "dayhoff", planned=False, env={"KS_DEBUG_NO_COMPACT": "1"})


def test_plain_tiles_keep_the_lookback(monkeypatch):
    res, offs = _random(_proteins(17), 17)
    _both_paths(monkeypatch, res, offs, 10, 1, "protein", planned=False, env={"KS_DEBUG_NO_PACK": "1"})


@pytest.mark.parametrize("repeats", [False, True])
def test_bounded_output_repeat_on_the_planned_path(monkeypatch, repeats):
    """KS_DEBUG_OUT_CAP below the batch's windows: the launch reports the window total, the batch is repeated with outputs of
    that size, both on the planned path."""
    res, offs = _with_repeats(18) if repeats else _random(_proteins(18), 18)
    k, mol = 10, "protein"
    want = oracle.sketch_batch(res, offs, k, 1, mol, n_threads=8)
    monkeypatch.setenv("KS_DEBUG_OUT_CAP", "20000")
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        assert int(_windows_cumsum(offs, k)[-1]) > 20000
        S = ctx.sketch_batch(res, offs, k, 1, mol)
        assert ctx.sketch_stats()["cap_fallbacks"] == 1 and _planned(ctx) == 2
        assert S.n_hashes == len(want[1])
        _eq(S.to_host(), want, "after the bounded-output repeat")
    finally:
        ctx.close()


@pytest.mark.parametrize("lookback", [False, True])
def test_query_side_postings_and_hits(monkeypatch, lookback):
    """2,500 queries against a 3,000-protein index: sketch_queries_device + search and the one-call sketch_search_device give
    the hit rows of the unfused search, on either path."""
    k, mol = 10, "protein"
    t_res, t_off = synth.proteome(3000, stream=300)
    q_res, q_off = synth.queries(2500, t_res, t_off, stream=301)
    n, nr, mx = len(q_off) - 1, len(q_res), _maxlen(q_off)
    want = oracle.sketch_batch(q_res, q_off, k, 1, mol, n_threads=8)
    if lookback:
        monkeypatch.setenv("KS_DEBUG_TILE_LOOKBACK", "1")
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, 1, mol))
        plain = ctx.search(ix, ctx.sketches_from_host(*want, k, 1, mol)).to_host()
        assert len(plain[0]) > 0
        d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
        for hint in (0, mx):
            p0 = _planned(ctx)
            Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n, nr, max_seq_len=hint)
            assert (_planned(ctx) > p0) == (not lookback)
            H = ctx.search(ix, Q)
            assert H.partition_path != 3, "the search must read the sketch's postings"
            _eq(H.to_host(), plain, f"two calls, hint {hint}")
            _eq(Q.to_host(), want, f"query sketches, hint {hint}")
            p0 = _planned(ctx)
            Q2, H2 = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n, nr, max_seq_len=hint)
            assert (_planned(ctx) > p0) == (not lookback)
            _eq(H2.to_host(), plain, f"one call, hint {hint}")
            _eq(Q2.to_host(), want, f"one call sketches, hint {hint}")
            assert Q2.n_hashes == len(want[1])
            for o in (Q, H, Q2, H2):
                o.free()
        assert ctx.fused_stats()["redos"] == 0
    finally:
        ctx.close()
