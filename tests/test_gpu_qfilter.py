"""GPU: the presence filter of the bucket scatter.  A fingerprint-layout index carries a bitmap over hash
prefixes; the scatter of the query postings drops those whose bit is clear.  A dropped posting could not have matched, so every
search gives the same rows with the filter forced on (KS_DEBUG_QFILTER = 1) as with it forced off (= 0), and the rows of the
oracle's manysearch on a sample of the queries.

The fingerprint layout and a join on 16 prefix bits are forced on a 16k-protein index (KS_DEBUG_JOIN_FP, KS_DEBUG_BUCKET), as in
test_nine_byte_bucket_postings_equal_plain_search.  The batches: the targets themselves (every posting survives: the filter's
counter of dropped postings stays 0 — a false negative would show there before it shows in a row), unrelated random proteins
(nearly nothing survives: empty buckets, hardly a hit), a mixed batch, and a batch with 1,200 copies of one target (a bucket
overflows: the dense fall-back, which is not filtered).  Each under the three posting widths and both join kernels, through the
two plain calls and the one-call entry.  The sub-regions' fills are no multiples of the tile, so every one ends in a partial tile.
Indexes of one and of two postings build their one-word bitmap.  The hand-made index puts its hashes where the bitmap's
arithmetic has its edges (see there)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import synth
from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402

K, SCALED, MOL = 10, 1, "protein"
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
SAMPLE = 150  # queries of each batch that are held against the oracle
WIDTHS = {9: {}, 10: {"KS_DEBUG_POSTINGS10": "1"}, 12: {"KS_DEBUG_POSTINGS12": "1"}}


@pytest.fixture(scope="module")
def ctx():
    c = ks.Context(0, follow_debug_env=True)
    yield c
    c.close()


def _random_proteins(rng, n, lo=60, hi=400):
    return [AA[rng.integers(0, 20, int(m))].tobytes() for m in rng.integers(lo, hi, n)]


_DATA = {}


def _data():
    """targets, the query batches and the oracle's rows for the first SAMPLE queries of each: made once"""
    if _DATA:
        return _DATA
    t_res, t_off = synth.proteome(16000, stream=410)
    tseq = [bytes(t_res[int(t_off[i]):int(t_off[i + 1])]) for i in range(len(t_off) - 1)]
    rng = np.random.default_rng(411)
    m_res, m_off = synth.queries(1500, t_res, t_off, stream=412)
    mseq = [bytes(m_res[int(m_off[i]):int(m_off[i + 1])]) for i in range(1500)]
    foreign = _random_proteins(rng, 3000)
    mixed = [s for pair in zip(mseq, foreign[:1500]) for s in pair] + [s[:45] for s in mseq]
    batches = {"self": tseq[:3000], "foreign": foreign, "mixed": mixed,
               "overflow": tseq[:64] + [tseq[7]] * 1200 + foreign[:500]}
    wt = oracle.sketch_batch(t_res, t_off, K, SCALED, MOL, n_threads=8)
    _DATA["targets"] = (t_res, t_off)
    for name, seqs in batches.items():
        res, off = ks.pack(seqs)
        s_res, s_off = ks.pack(seqs[:SAMPLE])
        wq = oracle.sketch_batch(s_res, s_off, K, SCALED, MOL, n_threads=8)
        _DATA[name] = (res, off, oracle.manysearch(wq[0], wq[1], wt[0], wt[1], wt[2], n_threads=8))
    return _DATA


def _eq(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (label, j, len(g), len(w))


def _dropped(ctx, fn):
    """fn() and what the filtered scatters read / dropped meanwhile"""
    a = ctx.qfilter_stats()
    out = fn()
    b = ctx.qfilter_stats()
    return out, b["seen"] - a["seen"], b["dropped"] - a["dropped"]


@pytest.mark.parametrize("sparse", ["0", "1"])
@pytest.mark.parametrize("width", [9, 10, 12])
@pytest.mark.parametrize("batch", ["self", "foreign", "mixed", "overflow"])
def test_filtered_search_equals_unfiltered_and_oracle(ctx, monkeypatch, batch, width, sparse):
    D = _data()
    for k_, v in dict(WIDTHS[width], KS_DEBUG_JOIN_FP="1", KS_DEBUG_BUCKET="64", KS_DEBUG_JOIN_SPARSE=sparse).items():
        monkeypatch.setenv(k_, v)
    t_res, t_off = D["targets"]
    q_res, q_off, want_sample = D[batch]
    n_q = len(q_off) - 1
    ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    monkeypatch.setenv("KS_DEBUG_QFILTER", "0")
    Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
    assert Q.posting_bytes == (12 if width == 12 else 10)
    H0, seen0, _ = _dropped(ctx, lambda: ctx.search(ix, Q))
    assert seen0 == 0  # (forced off: no filtered scatter ran)
    off_rows = H0.to_host()
    sel = off_rows[0] < SAMPLE
    _eq([c[sel] for c in off_rows], want_sample, (batch, "oracle"))
    monkeypatch.setenv("KS_DEBUG_QFILTER", "1")
    H1, seen, dropped = _dropped(ctx, lambda: ctx.search(ix, Q))
    _eq(H1.to_host(), off_rows, (batch, "two calls"))
    assert H1.n_pair_instances == H0.n_pair_instances
    (_, H2), seen2, dropped2 = _dropped(ctx, lambda: ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res)))
    _eq(H2.to_host(), off_rows, (batch, "one call"))
    if batch == "overflow":  # a bucket overflowed: the rows come from the dense partition (unfiltered), nothing is counted
        assert H1.partition_path != 1 and H0.partition_path != 1 and seen == 0
        return
    assert H1.partition_path == 1 and H1.bucket_posting_bytes == width and H2.bucket_posting_bytes == width
    assert seen == Q.n_hashes and (seen2, dropped2) == (seen, dropped)
    if batch == "self":
        assert dropped == 0 and len(off_rows[0]) >= n_q
    elif batch == "foreign":  # ~5 M index postings under 2^24 bits: at most 28 % of the bits are set
        assert dropped > 0.6 * seen and len(off_rows[0]) < n_q
    else:
        assert 0 < dropped < seen


@pytest.mark.parametrize("n_postings", [1, 2])
def test_index_of_one_and_two_postings(ctx, monkeypatch, n_postings):
    """an index of one k-mer, or two: a bitmap of one word; no bucket scatter runs against it (no prefix bits), the rows stand"""
    monkeypatch.setenv("KS_DEBUG_JOIN_FP", "1")
    monkeypatch.setenv("KS_DEBUG_QFILTER", "1")
    target = b"MKVLAAGIWQRT"[:K + n_postings - 1]
    t_res, t_off = ks.pack([target])
    rng = np.random.default_rng(413)
    seqs = _random_proteins(rng, 300) + [b"AAC" + target + b"WW", target[:K], target[1:] + b"A"]
    q_res, q_off = ks.pack(seqs)
    ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
    assert ix.n_postings == n_postings
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    got = ctx.search(ix, ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, len(seqs), len(q_res))).to_host()
    wq = oracle.sketch_batch(q_res, q_off, K, SCALED, MOL, n_threads=8)
    wt = oracle.sketch_batch(t_res, t_off, K, SCALED, MOL, n_threads=8)
    want = oracle.manysearch(wq[0], wq[1], wt[0], wt[1], wt[2], n_threads=8)
    assert len(want[0]) >= 2
    _eq(got, want, n_postings)


def _presence_bits(n_postings, pbits):
    """the bitmap's width, replayed from ks_search.hip's host code: the first power of two >= 3 bits per posting"""
    bits = pbits
    while bits < 31 and (1 << bits) < 3 * n_postings:
        bits += 1
    return bits


@pytest.mark.parametrize("sparse", ["0", "1"])
def test_hand_made_index_on_the_bitmaps_edges(ctx, monkeypatch, sparse):
    """The query postings come from the sketch kernel (only those reach the bucket scatter), so the INDEX is the hand-made side:
    2.3 M random hashes (a join on 16 prefix bits, a bitmap of 2^23 bits: 128 per bucket) and, chosen among the hashes the query
    batch really has: those on the first and the last bit of a bucket's chunk of the bitmap, those in the first and the last
    bucket of a region (top byte 0x00 / 0xff), and for every 40th other query hash h the hash h ^ 1 — the same bit of the
    bitmap, another key: h survives the filter and must not make a hit.  Rows against the numpy join."""
    monkeypatch.setenv("KS_DEBUG_JOIN_FP", "1")
    monkeypatch.setenv("KS_DEBUG_BUCKET", "64")
    monkeypatch.setenv("KS_DEBUG_JOIN_SPARSE", sparse)
    rng = np.random.default_rng(414)
    q_res, q_off = ks.pack(_random_proteins(rng, 3000))
    Qh = oracle.sketch_batch(q_res, q_off, K, SCALED, MOL, n_threads=8)
    Qh = (Qh[0].astype(np.uint64), Qh[1].astype(np.uint64), Qh[2].astype(np.uint32))
    qh = np.unique(Qh[1])
    bulk = rng.integers(1, cs.U64_MAX, 2_300_000, dtype=np.uint64)
    pbits, m = 16, 7  # (asserted below, once the index has its size)
    low = (qh >> np.uint64(64 - pbits - m)) & np.uint64((1 << m) - 1)
    top = qh >> np.uint64(56)
    chunk_edges = qh[(low == 0) | (low == (1 << m) - 1)]
    bucket_edges = qh[(top == 0) | (top == 255)]
    assert len(chunk_edges) > 1000 and len(bucket_edges) > 1000 and (low == 0).any() and (top == 255).any()
    rest = np.setdiff1d(qh, np.concatenate([chunk_edges, bucket_edges]))[::40]
    near = np.setdiff1d(rest ^ np.uint64(1), qh)
    assert len(near) > 1000
    t_h = np.unique(np.concatenate([bulk, chunk_edges, bucket_edges, near]))
    T = cs._deal(rng, t_h, 500, 1)
    cs.check_valid(T, SCALED)
    assert (len(T[1]) >> 15) > 64 and _presence_bits(len(T[1]), pbits) == pbits + m
    want = cs.ref_join(T, Qh)
    ix = ctx.index_build(ctx.sketches_from_host(T[0], T[1], T[2], K, SCALED, MOL))
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    rows = {}
    for flt in ("0", "1"):
        monkeypatch.setenv("KS_DEBUG_QFILTER", flt)
        Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, len(q_off) - 1, len(q_res))
        H, seen, dropped = _dropped(ctx, lambda: ctx.search(ix, Q))
        assert H.partition_path == 1 and H.bucket_posting_bytes == 9
        rows[flt] = H.to_host()
        _eq(rows[flt], want, ("hand-made", flt))
    # every query posting whose hash (or whose bit's other owner, `near`) is in the index survived
    kept = np.isin(Qh[1], t_h) | np.isin(Qh[1] ^ np.uint64(1), near)
    assert seen == len(Qh[1]) and seen - dropped >= int(kept.sum()) and dropped > 0.5 * seen
