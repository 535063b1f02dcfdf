"""GPU: the two-bit presence filter of the bucket scatter and the join kernel chosen by its survivors (DESIGN.md section 3.2 [r7]).

The filter is an array of 32-bit words with 2^pres_bits bits in all.  A hash with prefix p = umulhi(hash >> 32, pres_K) owns two
bits of word p >> 5: bit p & 31 and bit (hash >> 8) & 31 (bits [8, 13) of the low hash word; 32-bit words, so that a probe stays a
4-byte load — `_bits` numbers them inside 64-bit words, pairs of those, which is the same bitmap).  The index build sets both for every
posting; the scatter of the query postings keeps a posting if and only if both of its bits are set.  `_replay` is that definition
in numpy: the number of postings a filtered scatter keeps (`seen - dropped` of Context.qfilter_stats) must EQUAL its count — no
false negative, and the second bit really tested (testing the first bit alone keeps more, asserted on the same data).

As in test_gpu_qfilter.py the fingerprint layout and a join on 16 prefix bits are forced on a small index (KS_DEBUG_JOIN_FP,
KS_DEBUG_BUCKET = 64).  The join choice: behind a filtered scatter the join kernel is picked from the kept fraction of the
context's previous filtered search (Context.search_stats(paths=True)["join_table"] counts the searches that took the table
kernel); a context's first search and an unfiltered one go by the posting count before the filter.  An index carries the filter
at 3 and at 6 bits per posting; a search takes the big one when its batch has more than 768 postings per join bucket
(KS_DEBUG_QFILTER_OCC builds the one size it names, as most cases here do)."""
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
WIDTHS = {9: {}, 10: {"KS_DEBUG_POSTINGS10": "1"}, 12: {"KS_DEBUG_POSTINGS12": "1"}}
PBITS = 16           # join prefix bits of every index here but the tiny ones (asserted where an index is built)
JS_QCAP_FILL = 768   # JS_QCAP * 3 / 4 (ks_search.hip): the expected bucket fill up to which the table kernel joins
U = np.uint64

_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    c = ks.Context(0, follow_debug_env=True)
    yield c
    _CACHE.clear()
    c.close()


def _random_proteins(rng, n, lo=60, hi=400):
    return [AA[rng.integers(0, 20, int(m))].tobytes() for m in rng.integers(lo, hi, n)]


def _presence_bits(n_postings, pbits, occ=3):
    """the filter's width, replayed from ks_search.hip's host code: the first power of two >= occ bits per posting"""
    bits = pbits
    while bits < 31 and (1 << bits) < occ * n_postings:
        bits += 1
    return bits


def _bits(h, pres_bits):
    """(word, first bit, second bit) of the hashes h in a filter of 2^pres_bits bits (scaled = 1)"""
    p = ((h >> U(32)) * U(cs.prefix_mul(pres_bits, cs.max_hash(SCALED)))) >> U(32)
    return (p >> U(6)).astype(np.int64), p & U(63), (p & U(32)) | ((h >> U(8)) & U(31))


def _replay(t_hashes, q_hashes, pres_bits, second=True):
    """the filter's definition: both bits set for every index hash, then both tested for every query hash -> keep mask
    (second = False: what a scatter that forgot to test the second bit would keep, for comparison)"""
    bm = np.zeros(max(1, 1 << max(pres_bits - 6, 0)), U)
    w, a, b = _bits(np.unique(t_hashes), pres_bits)
    np.bitwise_or.at(bm, w, (U(1) << a) | (U(1) << b))
    w, a, b = _bits(q_hashes, pres_bits)
    keep = (bm[w] >> a) & U(1)
    if second:
        keep &= bm[w] >> b
    return keep.astype(bool)


def _kept(ctx, fn):
    """fn() and what the filtered scatters read / kept meanwhile"""
    a = ctx.qfilter_stats()
    out = fn()
    b = ctx.qfilter_stats()
    seen, dropped = b["seen"] - a["seen"], b["dropped"] - a["dropped"]
    return out, seen, seen - dropped


def _eq(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (label, j, len(g), len(w))


def _hand_made():
    """The query batch (3,000 random proteins, sketched by the oracle), the hand-made index and the numpy join's rows: made once.
    The index: 4.3 M random hashes (a join on 16 prefix bits, a filter of 2^24 bits at 3 bits per posting — KS_DEBUG_QFILTER_OCC —:
    256 per bucket, four words) and, chosen among
    the hashes the query batch really has, every second hash of each edge family — first bit 0 or 63, second bit 0 or 63, both
    bits the same, first or last word of a bucket's chunk (every eighth such hash), first or last bucket of a region (top byte
    0x00 / 0xff) — the other half of each family stays foreign on the same edges; and for every 40th other query hash h the
    hash h ^ (1 << 10): the same word and first bit, another second bit."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    rng = np.random.default_rng(514)
    q_res, q_off = ks.pack(_random_proteins(rng, 3000))
    Qh = oracle.sketch_batch(q_res, q_off, K, SCALED, MOL, n_threads=8)
    Qh = (Qh[0].astype(U), Qh[1].astype(U), Qh[2].astype(np.uint32))
    qh = np.unique(Qh[1])
    bulk = rng.integers(1, cs.U64_MAX, 4_300_000, dtype=U)
    pres_bits = PBITS + 8  # (asserted below, once the index has its size)
    w, first, second = _bits(qh, pres_bits)
    chunk_word = w & 3  # four words per bucket
    top = qh >> U(56)
    fam = {"first bit 0": first == 0, "first bit 63": first == 63, "second bit 0": second == 0, "second bit 63": second == 63,
           "one bit": first == second, "first word": (chunk_word == 0) & (qh % U(8) == 0),
           "last word": (chunk_word == 3) & (qh % U(8) == 0), "first bucket": top == 0, "last bucket": top == 255}
    for name, m in fam.items():
        assert int(m.sum()) > 500, (name, int(m.sum()))
    edge = np.zeros(len(qh), bool)
    for m in fam.values():
        edge |= m
    edges_in = qh[edge][::2]
    for name, m in fam.items():  # each family on both sides: in the index, and foreign to it
        assert np.isin(qh[m], edges_in).any() and not np.isin(qh[m], edges_in).all(), name
    flipped = qh[~edge][::40]
    near = np.setdiff1d(flipped ^ U(1 << 10), qh)
    assert len(near) > 1000
    t_h = np.unique(np.concatenate([bulk, edges_in, near]))
    T = cs._deal(rng, t_h, 500, 1)
    cs.check_valid(T, SCALED)
    assert (len(T[1]) >> 15) > 64 and _presence_bits(len(T[1]), PBITS) == pres_bits
    keep2, keep1 = _replay(T[1], Qh[1], pres_bits), _replay(T[1], Qh[1], pres_bits, second=False)
    assert not (keep2 & ~keep1).any() and np.isin(Qh[1], t_h)[~keep2].sum() == 0  # (the replay itself: no false negative)
    # the flipped hashes are where a filter that forgot its second bit shows: the first bit of every one is set
    fl = np.isin(Qh[1], near ^ U(1 << 10))
    assert keep1[fl].all() and 0 < int(keep2[fl].sum()) < int(fl.sum()) and int(keep2.sum()) < int(keep1.sum())
    _CACHE["hand"] = (q_res, q_off, Qh, T, cs.ref_join(T, Qh), int(keep2.sum()))
    return _CACHE["hand"]


@pytest.mark.parametrize("sparse", ["0", "1"])
@pytest.mark.parametrize("width", [9, 10, 12])
def test_the_filter_is_what_it_says(ctx, monkeypatch, width, sparse):
    """rows = the numpy join, filter off and on, in every posting width under both joins; the scatter keeps exactly the postings
    the definition keeps"""
    for k_, v in dict(WIDTHS[width], KS_DEBUG_JOIN_FP="1", KS_DEBUG_BUCKET="64", KS_DEBUG_JOIN_SPARSE=sparse, KS_DEBUG_QFILTER_OCC="3").items():
        monkeypatch.setenv(k_, v)
    q_res, q_off, Qh, T, want, want_kept = _hand_made()
    if "hand_ix" not in _CACHE:  # (the index does not depend on the posting width or the join: built once)
        _CACHE["hand_ix"] = ctx.index_build(ctx.sketches_from_host(T[0], T[1], T[2], K, SCALED, MOL))
    ix = _CACHE["hand_ix"]
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    n_q = len(q_off) - 1
    Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
    assert Q.posting_bytes == (12 if width == 12 else 10) and Q.n_hashes == len(Qh[1])
    rows = {}
    for flt in ("0", "1"):
        monkeypatch.setenv("KS_DEBUG_QFILTER", flt)
        H, seen, kept = _kept(ctx, lambda: ctx.search(ix, Q))
        assert H.partition_path == 1 and H.bucket_posting_bytes == width
        print(f"width {width} sparse {sparse} filter {flt}: seen {seen} kept {kept} (replay {want_kept})")
        rows[flt] = H.to_host()
        _eq(rows[flt], want, ("hand-made", width, sparse, flt))
        if flt == "0":
            assert seen == 0  # (forced off: no filtered scatter ran)
        else:
            assert seen == len(Qh[1]) and kept == want_kept, (seen, kept, want_kept)
    _eq(rows["1"], rows["0"], "filter on / off")
    (_, H2), seen2, kept2 = _kept(ctx, lambda: ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res)))
    _eq(H2.to_host(), want, ("hand-made, one call", width, sparse))
    assert (seen2, kept2) == (len(Qh[1]), want_kept) and H2.bucket_posting_bytes == width


def _proteome():
    if "proteome" not in _CACHE:
        t_res, t_off = synth.proteome(8000, stream=510)
        _CACHE["proteome"] = (t_res, t_off, oracle.sketch_batch(t_res, t_off, K, SCALED, MOL, n_threads=8))
    return _CACHE["proteome"]


@pytest.mark.parametrize("occ", [3, 6])
def test_self_batch_drops_nothing(ctx, monkeypatch, occ):
    """the targets searched against their own index at both filter sizes: every posting survives; foreign proteins against the
    same index keep what the definition keeps at that size"""
    for k_, v in dict(KS_DEBUG_JOIN_FP="1", KS_DEBUG_BUCKET="64", KS_DEBUG_QFILTER="1", KS_DEBUG_QFILTER_OCC=str(occ)).items():
        monkeypatch.setenv(k_, v)
    t_res, t_off, wt = _proteome()
    n_post = int(wt[0][-1])
    assert 2_000_000 < n_post < 5_000_000 and (n_post >> 15) > 64
    pres_bits = _presence_bits(n_post, PBITS, occ)
    assert pres_bits == _presence_bits(n_post, PBITS, 3) + (occ == 6)  # (the two sizes differ)
    ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
    assert ix.n_postings == n_post
    n_self = 3000
    s_res, s_off = t_res[:int(t_off[n_self])], t_off[:n_self + 1]
    d_res, d_off = ctx.to_device(s_res), ctx.to_device(s_off)
    Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_self, len(s_res))
    H, seen, kept = _kept(ctx, lambda: ctx.search(ix, Q))
    assert H.partition_path == 1 and seen == Q.n_hashes == int(wt[0][n_self]) and kept == seen
    assert H.count >= n_self
    f_res, f_off = ks.pack(_random_proteins(np.random.default_rng(511), 3000))
    wf = oracle.sketch_batch(f_res, f_off, K, SCALED, MOL, n_threads=8)
    d_res, d_off = ctx.to_device(f_res), ctx.to_device(f_off)
    Qf = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, 3000, len(f_res))
    Hf, seen, kept = _kept(ctx, lambda: ctx.search(ix, Qf))
    want_kept = int(_replay(wt[1].astype(U), wf[1].astype(U), pres_bits).sum())
    print(f"occ {occ}: 2^{pres_bits} bits, foreign batch seen {seen} kept {kept} (replay {want_kept})")
    assert Hf.partition_path == 1 and seen == len(wf[1]) and kept == want_kept


@pytest.mark.parametrize("n_postings", [1, 2])
def test_index_of_one_and_two_postings(ctx, monkeypatch, n_postings):
    """an index of one k-mer, or two: a filter of one word, the rows stand"""
    monkeypatch.setenv("KS_DEBUG_JOIN_FP", "1")
    monkeypatch.setenv("KS_DEBUG_QFILTER", "1")
    target = b"MKVLAAGIWQRT"[:K + n_postings - 1]
    t_res, t_off = ks.pack([target])
    rng = np.random.default_rng(513)
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


def test_join_kernel_is_chosen_by_the_survivors(monkeypatch):
    """A foreign batch of more than 768 postings per join bucket (2^16 buckets: 135,000 random proteins of 400 residues, 52.8 M
    postings) against the 8,000-protein index, of which the filter keeps a fraction: under 768 per bucket.  The context's first
    search knows no fraction yet and goes by the posting count (the staged join); the second expects the first one's fraction
    (the table kernel); with the filter forced off the count before the filter decides again.  Rows: equal throughout, and
    equal to those of the staged join forced.  Then the filter's size: an index built without KS_DEBUG_QFILTER_OCC keeps, of
    this batch, what the index built at 6 bits per posting keeps (fewer than at 3), and of a batch of 3,000 of these
    proteins — 18 postings per bucket — what the index built at 3 keeps (more than at 6)."""
    for k_, v in dict(KS_DEBUG_JOIN_FP="1", KS_DEBUG_BUCKET="64", KS_DEBUG_QFILTER="1", KS_DEBUG_QFILTER_OCC="3").items():
        monkeypatch.setenv(k_, v)
    t_res, t_off, wt = _proteome()
    rng = np.random.default_rng(512)
    n_q, length = 135_000, 400
    q_res = AA[rng.integers(0, 20, n_q * length, dtype=np.uint8)]
    q_res[:int(t_off[50])] = t_res[:int(t_off[50])]  # (some residues of the targets: a few rows to compare)
    q_off = (np.arange(n_q + 1, dtype=np.uint64) * np.uint64(length))
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
        assert (ix.n_postings >> 15) > 64  # 2^16 join buckets
        d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
        Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
        n_buckets = 1 << PBITS
        assert Q.n_hashes // n_buckets > JS_QCAP_FILL

        def table(fn):
            a = ctx.search_stats(paths=True)["join_table"]
            out = fn()
            return out, ctx.search_stats(paths=True)["join_table"] - a

        (H1, seen, kept), took1 = table(lambda: _kept(ctx, lambda: ctx.search(ix, Q)))
        print(f"postings per bucket {Q.n_hashes / n_buckets:.0f}, kept per bucket {kept / n_buckets:.0f}")
        assert H1.partition_path == 1 and seen == Q.n_hashes and 0 < kept // n_buckets < JS_QCAP_FILL
        assert took1 == 0  # (a context's first filtered search: by the count before the filter)
        rows = H1.to_host()
        assert len(rows[0]) > 0
        H2, took2 = table(lambda: ctx.search(ix, Q))
        assert took2 == 1 and "join_table" not in ctx.search_stats()
        _eq(H2.to_host(), rows, "table kernel by the survivors")
        f0 = ctx.fused_stats()["table_joined"]
        (_, H3), took3 = table(lambda: ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res)))
        assert took3 == 1 and ctx.fused_stats()["table_joined"] == f0 + 1
        _eq(H3.to_host(), rows, "one call")
        monkeypatch.setenv("KS_DEBUG_JOIN_SPARSE", "0")
        H4, took4 = table(lambda: ctx.search(ix, Q))
        assert took4 == 0
        _eq(H4.to_host(), rows, "staged join forced")
        monkeypatch.delenv("KS_DEBUG_JOIN_SPARSE")
        monkeypatch.setenv("KS_DEBUG_QFILTER", "0")
        H5, took5 = table(lambda: ctx.search(ix, Q))
        assert took5 == 0  # (unfiltered: by the posting count)
        _eq(H5.to_host(), rows, "filter off")
        monkeypatch.setenv("KS_DEBUG_QFILTER", "1")
        monkeypatch.setenv("KS_DEBUG_QFILTER_OCC", "6")
        ix6 = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
        monkeypatch.delenv("KS_DEBUG_QFILTER_OCC")
        ix_auto = ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
        n_small = 3000
        Qs = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_small, n_small * length)
        assert 0 < Qs.n_hashes // n_buckets < JS_QCAP_FILL
        k = {}
        for name, index in (("3", ix), ("6", ix6), ("auto", ix_auto)):
            for size, q in (("big", Q), ("small", Qs)):
                H, seen_, k[name, size] = _kept(ctx, lambda: ctx.search(index, q))
                assert seen_ == q.n_hashes
                _eq(H.to_host(), rows if size == "big" else [c[rows[0] < n_small] for c in rows], ("filter size", name, size))
        print("kept by filter size and batch:", k)
        assert k["auto", "big"] == k["6", "big"] < k["3", "big"] == kept
        assert k["auto", "small"] == k["3", "small"] > k["6", "small"]
    finally:
        ctx.close()
