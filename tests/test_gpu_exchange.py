"""GPU: the device path of the multi-GPU hit exchange (kmerseek_amd/dist.py) on rank shards that DIFFER — the pack kernel, one
ks_hits_unpack64_device call per rank at pointer offsets into the gathered columns, the torch-side patch of escaped rows and the
counting merge ks_hits_merge_by_qid_device — held, exactly, against references that run none of that code.

* The exchange (tests/exchange_ranks.py stands in for the collective: W ranks one after another in this process, every rank's
  receive buffer built from the W real send blocks).  The per-rank hit lists are real searches of one crafted job whose targets
  (or queries) are split W ways by id range; the expected result is the oracle's unsharded search of the same sketches — which
  is also the numpy reference of the gather applied to the oracle's per-shard rows.  W in {2, 3, 8, 64}; unequal counts, so the
  smaller blocks carry padding; ranks without rows first, in the middle and last; index- and query-sharded, qid and shard
  order; packed and unpacked transport; one call and begin / finish; escapes in one middle rank only, within the escape list and
  beyond it (every rank then repeats with unpacked columns); values at the all-ones marker and one above.  Each case runs on
  a context with a stream of its own and on one that launches on torch's current stream.
* The counting merge alone on crafted columns, against a stable argsort: intersect and n_weighted carry the row's serial
  number (n_weighted above 2^32 on some rows), so a misplaced row shows whatever its ids are.
* Pack and unpack at the edges of the id fields, at pointer offsets between guard values, and word for word against the numpy
  packing dist.py uses for host columns.

All comparisons are integer equality."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import _lib, dist as ksd
from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import exchange_ranks as xr  # noqa: E402

DEV = torch.device("cuda", 0)
U32 = (np.uint32, np.uint32, np.uint32, np.uint64)


@pytest.fixture(scope="module", params=["own_stream", "torch_stream"])
def ctx(request):
    c = ks.Context(0, stream=None if request.param == "own_stream" else torch.cuda.current_stream(DEV).cuda_stream)
    assert (c.stream == torch.cuda.current_stream(DEV).cuda_stream) == (request.param == "torch_stream")
    yield c
    c.close()


def _torch_done():
    torch.cuda.current_stream(DEV).synchronize()


def _eq(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w), (label, j, g.dtype, w.dtype, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (label, "column", j, "first bad row", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), "bad rows", len(bad))


# ---- the job: 300 queries against 1000 targets, hand-made sketches -----------------------------------------------------------
N_T, N_Q = 1000, 300
KSIZE, SCALED, MOL = 7, 1, "protein"
T_QUIET = ((0, 40), (500, 540), (960, 1000))  # targets that share no hash with any query: a shard inside holds no row
Q_QUIET = ((0, 20), (140, 160), (280, 300))   # queries that share no hash with any target
MARK_Q, MARK_T = 25, (600, 601, 602)          # three targets of one posting each, met by one query: n_weighted = their abundance
WIDE_IDS = (1 << 24, 1 << 24)                 # 24 + 24 id bits leave 8 value bits: the all-ones marker is 255
_JOB = {}


def _in(ranges, i):
    return any(a <= i < b for a, b in ranges)


def _job():
    """(T offsets, T hashes, Q = (offsets, hashes, abundances)): even pool hashes are shared, odd ones are private"""
    if not _JOB:
        rng = np.random.default_rng(3107)
        pool = np.unique(rng.integers(1 << 20, 1 << 62, 2000, dtype=np.uint64) * np.uint64(2))
        seq, h = [], []
        for t in range(N_T):
            if t in MARK_T:
                hs = [2 + 2 * MARK_T.index(t)]
            elif _in(T_QUIET, t):
                hs = [8 * t + 1, 8 * t + 3, 8 * t + 5]
            else:
                hs = rng.choice(pool, 8, replace=False).tolist() + [8 * t + 1]
            seq += [t] * len(hs); h += hs
        To, Tm, _ = cs._csr(seq, h, np.ones(len(h)), N_T)
        seq, h = [], []
        for q in range(N_Q):
            if _in(Q_QUIET, q):
                hs = [8 * (N_T + q) + 1, 8 * (N_T + q) + 3]
            else:
                hs = rng.choice(pool, 20, replace=False).tolist() + [8 * (N_T + q) + 7] + ([2, 4, 6] if q == MARK_Q else [])
            seq += [q] * len(hs); h += hs
        Q = cs._csr(seq, h, np.ones(len(h)), N_Q)
        cs.check_valid(Q, SCALED)
        _JOB["job"] = (To, Tm, Q)
    return _JOB["job"]


def _abundances(esc, v):
    """esc = None: abundances 1 .. 3 by posting, so intersect and n_weighted differ.  esc = (s0, s1): every target 1, except
    the targets [s0, s1) — at or above 2^v — and, inside that range, the three marker targets: 2^v - 2 (the largest value that
    travels in the word), 2^v - 1 (the all-ones marker itself) and 2^v (one above it)."""
    To, Tm, _ = _job()
    if esc is None:
        return (1 + np.arange(len(Tm)) % 3).astype(np.uint32)
    ab = np.ones(len(Tm), np.uint32)
    b, e = int(To[esc[0]]), int(To[esc[1]])
    ab[b:e] = (1 << v) + np.arange(e - b) % 5
    assert esc[0] <= MARK_T[0] and MARK_T[-1] < esc[1]
    for t, a in zip(MARK_T, ((1 << v) - 2, (1 << v) - 1, 1 << v)):
        assert int(To[t + 1]) - int(To[t]) == 1
        ab[int(To[t])] = a
    return ab


def _slice(S, s0, s1):
    o, m, a = S
    b, e = int(o[s0]), int(o[s1])
    return (o[s0:s1 + 1] - o[s0]).astype(np.uint64), m[b:e], a[b:e]


W64_CUTS = [4 * i for i in range(61)] + [400, 700, 960, 1000]  # 60 shards of four targets, then four larger ones
# name -> (sharded, order, cuts, ids, api, escape shard, escapes expected, shards without rows)
#   ids: "job" = (N_Q, N_T) -> packed, 22 value bits; "wide" = WIDE_IDS -> packed, 8 value bits; None -> unpacked columns
CASES = {
    "w2_packed":                ("index", "qid", [0, 300, 1000], "job", "gather", None, "none", []),
    "w2_zero_first_begin":      ("index", "qid", [0, 40, 1000], "job", "begin", None, "none", [0]),
    "w2_zero_last_unpacked":    ("index", "qid", [0, 960, 1000], None, "gather", None, "none", [1]),
    "w3_zero_middle_begin":     ("index", "qid", [0, 500, 540, 1000], "job", "begin", None, "none", [1]),
    "w3_zero_middle_unpacked":  ("index", "qid", [0, 500, 540, 1000], None, "begin", None, "none", [1]),
    "w3_shard_order":           ("index", "shard", [0, 200, 650, 1000], "job", "gather", None, "none", []),
    "w3_shard_order_unpacked":  ("index", "shard", [0, 200, 650, 1000], None, "gather", None, "none", []),
    "w2_queries":               ("queries", "qid", [0, 100, 300], "job", "gather", None, "none", []),
    "w3_queries_zero_first":    ("queries", "qid", [0, 20, 170, 300], "job", "begin", None, "none", [0]),
    "w3_queries_unpacked":      ("queries", "qid", [0, 150, 280, 300], None, "gather", None, "none", [2]),
    "w8_begin":                 ("index", "qid", [0, 40, 100, 350, 500, 540, 700, 960, 1000], "job", "begin", None, "none", [0, 4, 7]),
    "w8_unpacked":              ("index", "qid", [0, 40, 100, 350, 500, 540, 700, 960, 1000], None, "gather", None, "none", [0, 4, 7]),
    "w8_shard_order":           ("index", "shard", [0, 40, 100, 350, 500, 540, 700, 960, 1000], "job", "gather", None, "none", [0, 4, 7]),
    "w64_begin":                ("index", "qid", W64_CUTS, "job", "begin", None, "none", list(range(10)) + [63]),
    "w3_escapes_gather":        ("index", "qid", [0, 590, 615, 1000], "wide", "gather", 1, "within", []),
    "w3_escapes_shard_order":   ("index", "shard", [0, 590, 615, 1000], "wide", "begin", 1, "within", []),
    "w8_escapes_begin":         ("index", "qid", [0, 40, 300, 590, 615, 700, 960, 1000], "wide", "begin", 3, "within", [0, 6]),
    "w3_overflow_begin":        ("index", "qid", [0, 560, 700, 1000], "wide", "begin", 1, "overflow", []),
    "w3_overflow_gather":       ("index", "qid", [0, 560, 700, 1000], "wide", "gather", 1, "overflow", []),
    "w8_overflow_begin":        ("index", "qid", [0, 40, 300, 560, 700, 800, 960, 1000], "wide", "begin", 3, "overflow", [0, 6]),
}
_PLANS = {}


def _plan(name):
    """Everything a case knows before the GPU is touched, from the oracle alone and computed once: the sketches, the shards,
    the oracle's rows per shard, the expected gathered columns — and the assertions that the input is what the name says."""
    if name in _PLANS:
        return _PLANS[name]
    sharded, order, cuts, ids, api, esc_shard, esc_kind, zero = CASES[name]
    W = len(cuts) - 1
    assert cuts[0] == 0 and cuts[-1] == (N_T if sharded == "index" else N_Q) and all(a < b for a, b in zip(cuts, cuts[1:]))
    id_counts = {"job": (N_Q, N_T), "wide": WIDE_IDS, None: None}[ids]
    v = xr.value_bits(id_counts)[2] if id_counts else None
    To, Tm, Q = _job()
    esc_range = (cuts[esc_shard], cuts[esc_shard + 1]) if esc_shard is not None else None
    T = (To, Tm, _abundances(esc_range, v))
    cs.check_valid(T, SCALED)
    full = oracle.manysearch(Q[0], Q[1], T[0], T[1], T[2])
    assert len(full[0]) > 10000
    shards = [(cuts[r], cuts[r + 1]) for r in range(W)]
    if sharded == "index":
        per = [oracle.manysearch(Q[0], Q[1], *_slice(T, s0, s1)) for s0, s1 in shards]
        qb, tb = [0] * W, [s0 for s0, _ in shards]
    else:
        per = [oracle.manysearch(*_slice(Q, s0, s1)[:2], T[0], T[1], T[2]) for s0, s1 in shards]
        qb, tb = [s0 for s0, _ in shards], [0] * W
    counts = [len(h[0]) for h in per]
    want = xr.gathered_reference(per, qb, tb, sharded, order)
    if order == "qid":  # the gather of the shards is the unsharded search
        _eq(want, full, (name, "reference of the gather vs the unsharded oracle"))
    else:
        o = np.lexsort((want[1], want[0]))
        _eq([c[o] for c in want], full, (name, "rank-major reference, sorted, vs the unsharded oracle"))
        assert not np.array_equal(want[0], full[0])
    # the properties of the input
    assert [r for r, c in enumerate(counts) if c == 0] == zero, (name, counts)
    cap = xr.padded_cap(counts)
    nonzero = sorted(c for c in counts if c)  # unequal counts: every block but the largest carries padding
    assert counts.count(max(counts)) == 1 and all(cap - c > 0 for c in counts if c != max(counts)), (name, counts)
    assert len(set(nonzero)) >= min(len(nonzero), 3)
    if W == 64:
        assert sum(1 for s0, s1 in shards if s1 - s0 <= 4) >= 60
    esc_cap = xr.escape_cap(counts)
    n_esc = [len(xr.escapes(h, v)) for h in per] if v else [0] * W
    if esc_kind == "none":
        assert max(n_esc) == 0
    else:
        assert all(n == 0 for r, n in enumerate(n_esc) if r != esc_shard) and 0 < esc_shard < W - 1, (name, n_esc)
        assert (0 < n_esc[esc_shard] <= esc_cap) if esc_kind == "within" else (n_esc[esc_shard] > esc_cap), (name, n_esc, esc_cap)
        vmax = (1 << v) - 1
        mark = {int(t): int(w) for q, t, w in zip(full[0], full[1], full[3]) if q == MARK_Q and t in MARK_T}
        assert mark == {MARK_T[0]: vmax - 1, MARK_T[1]: vmax, MARK_T[2]: vmax + 1}  # below, at and above the all-ones marker
        assert n_esc[esc_shard] == counts[esc_shard] - 1  # (every row of the shard but the one below the marker)
    _PLANS[name] = dict(sharded=sharded, order=order, shards=shards, id_counts=id_counts, api=api, T=T, Q=Q, full=full, per=per, qb=qb,
                        tb=tb, counts=counts, want=want, cap=cap, esc_cap=esc_cap, overflow=esc_kind == "overflow", W=W)
    return _PLANS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_exchange_on_different_shards(monkeypatch, ctx, name):
    P = _plan(name)
    W, counts = P["W"], P["counts"]
    dQ = ctx.sketches_from_host(*P["Q"], KSIZE, SCALED, MOL)
    dT = ctx.sketches_from_host(*P["T"], KSIZE, SCALED, MOL)
    ix = ctx.index_build(dT)
    unsharded = ctx.search(ix, dQ)
    _eq(unsharded.to_host(), P["full"], (name, "unsharded search on the device"))
    keep, hits = [], []
    for r, (s0, s1) in enumerate(P["shards"]):  # every rank's own search: a slice of the targets (or of the queries)
        if P["sharded"] == "index":
            sT = ctx.sketches_from_host(*_slice(P["T"], s0, s1), KSIZE, SCALED, MOL)
            six = ctx.index_build(sT)
            h = ctx.search(six, dQ)
            keep += [sT, six]
        else:
            sQ = ctx.sketches_from_host(*_slice(P["Q"], s0, s1), KSIZE, SCALED, MOL)
            h = ctx.search(ix, sQ)
            keep.append(sQ)
        assert h.count == counts[r], (name, r, h.count, counts[r])
        hits.append(h)
    for r in sorted({0, W // 2, W - 1}):
        _eq(hits[r].to_host(), P["per"][r], (name, "search of shard", r))
    ranks = xr.Ranks(counts).install(monkeypatch, ksd)
    kw = dict(device=DEV, sharded=P["sharded"], order=P["order"], id_counts=P["id_counts"])

    def one(r):
        if P["api"] == "gather":
            return ksd.all_gather_hits_device(hits[r], qid_base=P["qb"][r], tid_base=P["tb"][r], **kw)
        pend = ksd.begin_all_gather_hits_device(hits[r], qid_base=P["qb"][r], tid_base=P["tb"][r], **kw)
        if P["id_counts"] is not None:
            assert ranks.data_calls(r)[-1][2] is True and hits[r]._pins == 1  # started in the background, the list pinned
        got = pend.finish()
        assert hits[r]._pins == 0 and got is pend.finish()
        return got
    out = ranks.run(one)
    words = P["cap"] + 1 + 2 * P["esc_cap"]
    for r, got in enumerate(out):
        assert all(g.device.type == "cuda" for g in got)
        assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.int32, torch.int64]
        _eq(xr.as_host(got), P["want"], (name, "rank", r))
        sizes = [n for _, n, _ in ranks.data_calls(r)]
        assert sizes == ([words, 5 * P["cap"]] if P["overflow"] else [words] if P["id_counts"] else [5 * P["cap"]]), (name, r, sizes)
    _eq(ctx.search(ix, dQ).to_host(), P["full"], (name, "the context afterwards"))
    for x in hits + keep + [unsharded, ix, dT, dQ]:
        x.free()


# ---- the counting merge on crafted columns --------------------------------------------------------------------------------
SCAN_TILE = 2048  # ks_prims.hip: SCAN_THREADS * SCAN_IPT; the merge scans n_queries * W run lengths


def _qids(rng, n, nq, ends=False):
    q = np.sort(rng.integers(0, nq, n)).astype(np.uint32)
    if ends and n >= 2:
        q[0], q[-1] = 0, nq - 1
    return q


def _blocks_of(sizes, nq, seed, ends=True):
    rng = np.random.default_rng([11, seed])
    return [_qids(rng, n, nq, ends and r == int(np.argmax(sizes))) for r, n in enumerate(sizes)], nq  # (the ends: in the largest block)


def _merge_cases():
    c = {}
    c["w1"] = _blocks_of([700], 300, 1)
    c["w2"] = _blocks_of([700, 130], 300, 2)
    c["w3"] = _blocks_of([300, 900, 77], 300, 3)
    c["w7"] = _blocks_of([64, 1, 1500, 129, 640, 2, 333], 300, 7)
    c["w64"] = _blocks_of([(37 * r) % 91 for r in range(64)], 300, 64)
    c["empty_first"] = _blocks_of([0, 500, 300], 200, 10)
    c["empty_middle"] = _blocks_of([400, 0, 300], 200, 11)
    c["empty_last"] = _blocks_of([400, 300, 0], 200, 12)
    c["w7_all_empty_but_one"] = _blocks_of([0, 0, 0, 600, 0, 0, 0], 200, 13)
    c["w64_all_empty_but_first"] = _blocks_of([90] + [0] * 63, 50, 14)
    c["w64_all_empty_but_last"] = _blocks_of([0] * 63 + [90], 50, 15)
    c["launch_block_edges"] = _blocks_of([255, 256, 257, 3000], 300, 16)    # boundaries at 255, 511, 768: inside, and on the edge
    c["launch_block_edges_2"] = _blocks_of([256, 256, 3001, 255, 257], 300, 17)  # boundaries at 256 and 512: on the edges
    c["sparse_queries"] = _blocks_of([13, 20, 7], 5000, 18)                 # 40 rows, 5000 queries
    rng = np.random.default_rng(19)
    c["queries_in_some_blocks"] = ([np.sort(rng.choice(np.arange(r, 300, 3), 250)).astype(np.uint32) for r in range(3)], 300)
    c["one_query"] = ([np.full(n, 17, np.uint32) for n in (300, 1, 513)], 40)
    c["first_and_last_query"] = ([np.array([0] * 5 + [39] * 3, np.uint32), np.array([0, 39], np.uint32), np.array([39], np.uint32),
                                 np.array([0], np.uint32)], 40)
    for W, nq in ((2, 1023), (2, 1024), (2, 1025), (64, 31), (64, 32), (64, 33), (7, 1000), (3, 5000)):
        assert (W, nq) not in ((2, 1024), (64, 32)) or nq * W == SCAN_TILE
        c[f"scan_{W}x{nq}"] = _blocks_of([50 + (29 * r) % 200 for r in range(W)], nq, 100 + W + nq)
    assert max(nq * len(b) for b, nq in c.values()) > 7 * SCAN_TILE
    return c


MERGE_CASES = _merge_cases()


def _merge_inputs(blocks):
    """the gathered columns of the blocks: tid random, intersect and n_weighted the row's serial number"""
    n = sum(len(b) for b in blocks)
    qid = np.concatenate(blocks).astype(np.uint32) if n else np.zeros(0, np.uint32)
    serial = np.arange(n, dtype=np.uint64)
    tid = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    nw = serial + np.where(serial % 3 == 1, np.uint64(1 << 33), np.uint64(0))
    return qid, tid, serial.astype(np.uint32), nw


GUARD = 0x5A5A5A5A


def _run_merge(ctx, cols, counts, nq, pad=8):
    ins = [torch.from_numpy(c.view(s)).to(DEV) for c, s in zip(cols, (np.int32, np.int32, np.int32, np.int64))]
    n = len(cols[0])
    outs = [torch.full((n + pad,), GUARD, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.int32, torch.int64)]
    _torch_done()
    try:
        ctx.merge_hits_by_qid_device(*[x.data_ptr() for x in ins], counts, nq, *[o.data_ptr() for o in outs])
    finally:
        ctx.synchronize()
    got = [o.cpu().numpy().view(dt) for o, dt in zip(outs, U32)]
    assert all(np.all(g[n:] == GUARD) for g in got), "the merge wrote behind its outputs"
    return [g[:n] for g in got]


@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_counting_merge_equals_stable_argsort(ctx, name):
    blocks, nq = MERGE_CASES[name]
    assert all(np.all(b[1:] >= b[:-1]) for b in blocks) and all(int(b.max()) < nq for b in blocks if len(b))
    cols = _merge_inputs(blocks)
    assert np.any(cols[3] >= np.uint64(1 << 32))
    if name not in ("one_query", "queries_in_some_blocks"):
        assert cols[0].min() == 0 and cols[0].max() == nq - 1  # rows of the first and of the last query
    o = np.argsort(cols[0], kind="stable")
    got = _run_merge(ctx, cols, [len(b) for b in blocks], nq)
    _eq(got, [c[o] for c in cols], name)


def test_counting_merge_no_rows_and_bad_arguments(ctx):
    empty = _merge_inputs([])
    for counts in ([0], [0, 0, 0]):  # nothing to merge: the call succeeds and writes nothing
        assert all(len(g) == 0 for g in _run_merge(ctx, empty, counts, 100))
    blocks, nq = _blocks_of([300, 200, 100], 150, 40)
    cols = _merge_inputs(blocks)
    want = [c[np.argsort(cols[0], kind="stable")] for c in cols]
    for counts in ([], [4] * 65):  # 0 and 65 rank blocks
        with pytest.raises(ks.KmerseekError) as e:
            _run_merge(ctx, cols, counts, nq)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "64" in str(e.value)
    # two rows of the middle block with a query id beyond n_queries: the call fails and says how many
    bad = [blocks[0], np.concatenate([blocks[1][:-2], np.array([nq, nq + 7], np.uint32)]), blocks[2]]
    assert all(np.all(b[1:] >= b[:-1]) for b in bad)
    with pytest.raises(ks.KmerseekError) as e:
        _run_merge(ctx, _merge_inputs(bad), [len(b) for b in bad], nq)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "2 rows" in str(e.value) and f"n_queries = {nq}" in str(e.value)
    _eq(_run_merge(ctx, cols, [len(b) for b in blocks], nq), want, "the context afterwards")


# ---- pack and unpack at the field edges --------------------------------------------------------------------------------------
_WIDE = {}


def _wide():
    """the hit list of crafted_sketches.wide_records, 2^20 query sequences (ids up to 2^20 - 1 and 4095, values up to 2^36),
    and of its first two queries against its first two targets (ids 0 and 1)"""
    if not _WIDE:
        _, k, scaled, mol, T, Q = cs.family("wide_records")
        Q = cs.wide_batches(Q)[0]
        T2, Q2 = _slice(T, 0, 2), _slice(Q, 0, 2)
        _WIDE["big"] = (k, scaled, mol, T, Q, cs.ref_join(T, Q))
        _WIDE["two"] = (k, scaled, mol, T2, Q2, cs.ref_join(T2, Q2))
        rows = _WIDE["big"][5]
        assert int(rows[0].max()) == cs.WIDE_N_Q - 1 and int(rows[1].max()) == cs.WIDE_N_T - 1
        assert _WIDE["two"][5][0].tolist() == [0, 1] and _WIDE["two"][5][1].tolist() == [0, 1]
    return _WIDE


def _search(ctx, which):
    k, scaled, mol, T, Q, rows = _wide()[which]
    dT, dQ = ctx.sketches_from_host(*T, k, scaled, mol), ctx.sketches_from_host(*Q, k, scaled, mol)
    H = ctx.search(ctx.index_build(dT), dQ)
    assert H.count == len(rows[0])
    return H, rows


def _pack(ctx, H, qbits, tbits, qid_base, tid_base, esc_cap):
    """ks_hits_pack64_to_device into one torch buffer laid out as a rank block of dist.py -> (words, raw escape counter,
    escape rows, intersects, n_weighteds as far as the list holds them)"""
    n = H.count
    buf = torch.zeros(n + 1 + 2 * esc_cap, dtype=torch.int64, device=DEV)
    _torch_done()
    b = buf.data_ptr()
    H.pack64_to_device(b, b + 8 * (n + 1), b + 8 * (n + 1) + 4 * esc_cap, b + 8 * (n + 1 + esc_cap), b + 8 * n, esc_cap, qbits, tbits,
                       qid_base=qid_base, tid_base=tid_base)
    ctx.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    raw = int(host[n])
    k = min(raw & 0x7fffffff, esc_cap)
    return (host[:n], raw, host[n + 1:n + 1 + esc_cap // 2].view(np.uint32)[:k], host[n + 1 + esc_cap // 2:n + 1 + esc_cap].view(np.uint32)[:k],
            host[n + 1 + esc_cap:][:k])


def _unpack(ctx, words, qbits, tbits, at=0, room=0):
    """ks_hits_unpack64_device of host words into columns of len(words) + room elements, at element offset `at`"""
    n = len(words)
    d_w = torch.from_numpy(words.view(np.int64).copy()).to(DEV)
    cols = [torch.full((n + room,), GUARD, dtype=t, device=DEV) for t in (torch.int32, torch.int32, torch.int32, torch.int64)]
    _torch_done()
    ctx.unpack_hits64_device(d_w.data_ptr(), n, qbits, tbits, cols[0].data_ptr() + 4 * at, cols[1].data_ptr() + 4 * at,
                             cols[2].data_ptr() + 4 * at, cols[3].data_ptr() + 8 * at)
    ctx.synchronize()
    return [c.cpu().numpy().view(dt) for c, dt in zip(cols, U32)]


def _words(rows, qid_base, tid_base, qbits, tbits):
    """the transport words in numpy (ids that fit): escaped rows carry all-ones in both value fields"""
    v = (64 - qbits - tbits) // 2
    vmax = np.uint64((1 << v) - 1)
    q, t, a, b = (np.asarray(x).astype(np.uint64) for x in rows)
    esc = (a >= vmax) | (b >= vmax)
    a, b = np.where(esc, vmax, a), np.where(esc, vmax, b)
    w = ((((q + np.uint64(qid_base)) << np.uint64(tbits)) | (t + np.uint64(tid_base))) << np.uint64(2 * v)) | (a << np.uint64(v)) | b
    return w, np.flatnonzero(esc)


@pytest.mark.parametrize("which,qbits,tbits", [("big", 23, 24), ("big", 24, 23), ("big", 24, 24), ("big", 20, 12), ("big", 21, 13),
                                               ("two", 1, 1), ("two", 1, 2)])
def test_pack_unpack_field_widths(ctx, which, qbits, tbits):
    """odd and even spare widths, the fewest id bits and the most: ids placed so that the largest one is all ones in its field"""
    H, rows = _search(ctx, which)
    n = len(rows[0])
    v = (64 - qbits - tbits) // 2
    assert (64 - qbits - tbits) % 2 == {(23, 24): 1, (24, 23): 1, (24, 24): 0, (20, 12): 0, (21, 13): 0, (1, 1): 0, (1, 2): 1}[(qbits, tbits)]
    qb, tb = (1 << qbits) - 1 - int(rows[0].max()), (1 << tbits) - 1 - int(rows[1].max())
    want_w, want_esc = _words(rows, qb, tb, qbits, tbits)
    assert 0 < len(want_esc) < n
    words, raw, er, ei, en = _pack(ctx, H, qbits, tbits, qb, tb, n + (n & 1))
    assert raw == len(want_esc), (raw, len(want_esc))  # every id fits: the high bit of the counter is clear
    assert np.array_equal(words, want_w)
    o = np.argsort(er)
    assert np.array_equal(er[o], want_esc) and np.array_equal(ei[o], rows[2][want_esc]) and np.array_equal(en[o], rows[3][want_esc])
    got = _unpack(ctx, words, qbits, tbits)
    vmax = (1 << v) - 1
    assert np.all(got[2][want_esc] == vmax) and np.all(got[3][want_esc] == vmax)
    got[2][er], got[3][er] = ei, en
    _eq(got, (rows[0] + np.uint32(qb), rows[1] + np.uint32(tb), rows[2], rows[3]), ("round trip", qbits, tbits))
    H.free()


@pytest.mark.parametrize("qbits,tbits", [(23, 24), (24, 24), (20, 12)])
def test_pack_flags_an_id_one_beyond_its_field(ctx, qbits, tbits):
    H, rows = _search(ctx, "big")
    qb, tb = (1 << qbits) - 1 - int(rows[0].max()), (1 << tbits) - 1 - int(rows[1].max())
    n_esc = len(_words(rows, 0, 0, qbits, tbits)[1])
    assert 0 < n_esc < 1 << 31
    for dq, dt, flagged in ((0, 0, False), (1, 0, True), (0, 1, True), (1, 1, True)):
        raw = _pack(ctx, H, qbits, tbits, qb + dq, tb + dt, 64)[1]
        assert (raw >> 31) == int(flagged) and (raw & 0x7fffffff) == n_esc, (dq, dt, hex(raw), n_esc)
        assert raw < 1 << 32
    H.free()


@pytest.mark.parametrize("at,c", [(1, 1), (3, 255), (255, 256), (257, 257), (64, 1000), (1, 4097)])
def test_unpack_at_pointer_offsets_between_guards(ctx, at, c):
    rows = [x[1000:1000 + c] for x in _wide()["big"][5]]
    qbits, tbits = 23, 24
    words, esc = _words(rows, 5, 9, qbits, tbits)
    got = _unpack(ctx, words, qbits, tbits, at=at, room=at + 5)
    vmax = (1 << ((64 - qbits - tbits) // 2)) - 1
    for g, w in zip(got, (rows[0] + np.uint32(5), rows[1] + np.uint32(9), np.where(np.isin(np.arange(c), esc), vmax, rows[2]).astype(np.uint32),
                          np.where(np.isin(np.arange(c), esc), vmax, rows[3]).astype(np.uint64))):
        assert np.all(g[:at] == GUARD) and np.all(g[at + c:] == GUARD) and len(g[at + c:]) == 5
        assert np.array_equal(g[at:at + c], w)


def _block_of_dist(monkeypatch, ctx, hits, n, qid_base, tid_base, qbits, tbits):
    """the send block dist.py builds for one rank's rows, device-resident or host columns, and what it unpacks from it"""
    on_device = hasattr(hits, "copy_to_device")
    ranks = xr.Ranks([n]).install(monkeypatch, ksd)
    dev = DEV if on_device else torch.device("cpu")
    out = ranks.run(lambda r: ksd._gather_packed_begin(hits, on_device, n, [n], qid_base, tid_base, qbits, tbits, dev, ctx.synchronize,
                                                       _torch_done, async_op=False)())
    return ranks.blocks[0][0].cpu().numpy().view(np.uint64), out[0]


@pytest.mark.parametrize("case", ["big", "two", "job"])
def test_device_block_equals_the_host_packing_of_dist(monkeypatch, ctx, case):
    """word for word: the block ks_hits_pack64_to_device fills inside dist.py against the block dist.py packs in numpy from the
    same rows as host columns — transport words, escape count, and (sorted by row: the device appends in any order) the
    escape lists where they hold every escape"""
    if case == "job":
        P = _plan("w3_escapes_gather")
        dQ, dT = ctx.sketches_from_host(*P["Q"], KSIZE, SCALED, MOL), ctx.sketches_from_host(*_slice(P["T"], 560, 640), KSIZE, SCALED, MOL)
        H, rows = ctx.search(ctx.index_build(dT), dQ), oracle.manysearch(P["Q"][0], P["Q"][1], *_slice(P["T"], 560, 640))
        qbits, tbits, qb, tb = 24, 24, 77, 560
    else:
        H, rows = _search(ctx, case)
        qbits, tbits, qb, tb = {"big": (23, 24, 7 << 20, (1 << 24) - 4096), "two": (1, 1, 0, 0)}[case]
    n = len(rows[0])
    _eq(H.to_host(), rows, (case, "search"))
    cap, esc_cap = xr.padded_cap([n]), xr.escape_cap([n])
    n_esc = len(_words(rows, qb, tb, qbits, tbits)[1])
    assert (n_esc <= esc_cap) == (case != "big") and n_esc > 0
    dev_block, dev_out = _block_of_dist(monkeypatch, ctx, H, n, qb, tb, qbits, tbits)
    host_block, host_out = _block_of_dist(monkeypatch, ctx, rows, n, qb, tb, qbits, tbits)
    assert len(dev_block) == len(host_block) == cap + 1 + 2 * esc_cap
    assert np.array_equal(dev_block[:cap], host_block[:cap])  # the words, and the padding behind them
    assert int(dev_block[cap]) == int(host_block[cap]) == n_esc
    if n_esc <= esc_cap:
        def lists(b):
            er = b[cap + 1:cap + 1 + esc_cap // 2].view(np.uint32)
            ei = b[cap + 1 + esc_cap // 2:cap + 1 + esc_cap].view(np.uint32)
            en = b[cap + 1 + esc_cap:]
            o = np.argsort(er[:n_esc])
            return er[:n_esc][o], ei[:n_esc][o], en[:n_esc][o], er[n_esc:], ei[n_esc:], en[n_esc:]
        for d, h in zip(lists(dev_block), lists(host_block)):
            assert np.array_equal(d, h)
        want = (rows[0] + np.uint32(qb), rows[1] + np.uint32(tb), rows[2], rows[3])
        _eq(xr.as_host(dev_out), want, (case, "device block unpacked"))
        _eq(xr.as_host(host_out), want, (case, "host block unpacked"))
    else:
        assert dev_out is None and host_out is None
    H.free()
