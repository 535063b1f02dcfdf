"""GPU: the rows of a search by hash aggregation of the match sort's level-1 regions (k_pairs_aggregate, DESIGN.md section 3.2
[r6]) against the rows of the full sort + run-length pass (k_pair_rows_fused).  Both paths read the same match list, so every
search gives the same four columns, the same row count and the same n_pair_instances with the path forced either way
(KS_DEBUG_ROWS_PATH = agg / sort), and the rows of the oracle's manysearch on a sample of the queries.

A 16k-protein index and batches of 12,000 synth.queries: about one in five of them hits a target, with about a hundred
records per row, so the list holds about 240k match records and the match sort's partition path applies, which the aggregate
pass starts from (3,000 of these queries make 62k records, under that path's 65,536).  `Context.search_stats(paths=True)` tells which path made the rows: `agg_used` counts
the searches the aggregate pass served, `agg_overflows` those in which a region's table overflowed and the sort resumed;
`Context.fused_stats()["aggregated"]` counts the one-call searches among the former."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import synth
from oracle import oracle

K, SCALED, MOL = 10, 1, "protein"
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
SAMPLE = 150  # queries of each batch that are held against the oracle
N_T = 16000
N_Q = 12000
POLY = b"W" * 4074  # one k-mer, 4,065 times: the abundance field of every record widens to 12 bits
FP_SEGS = {"KS_DEBUG_JOIN_FP": "1", "KS_DEBUG_BUCKET": "64", "KS_DEBUG_JOIN_SEGS": "1"}  # the join's segmented list


@pytest.fixture(scope="module")
def ctx():
    c = ks.Context(0, follow_debug_env=True)
    yield c
    c.close()


def _random_proteins(rng, n, lo=60, hi=400):
    return [AA[rng.integers(0, 20, int(m))].tobytes() for m in rng.integers(lo, hi, n)]


_DATA = {}


def _data():
    """targets and the query batches (residues, offsets, the first SAMPLE queries packed on their own): made once"""
    if _DATA:
        return _DATA
    t_res, t_off = synth.proteome(N_T, stream=610)
    q_res, q_off = synth.queries(N_Q, t_res, t_off, stream=611)
    qseq = [bytes(q_res[int(q_off[i]):int(q_off[i + 1])]) for i in range(N_Q)]
    rng = np.random.default_rng(612)
    foreign = _random_proteins(rng, N_Q // 2)
    mixed = [s for pair in zip(qseq[:N_Q // 2], foreign) for s in pair] + [s[:45] for s in qseq[:N_Q // 2]]
    # 300 queries of sixteen proteins each: few query bits (fewer than 256 regions hold a record), a list long enough to partition
    few = [b"".join(qseq[16 * i:16 * i + 16]) for i in range(300)]
    tseq = [bytes(t_res[int(t_off[i]):int(t_off[i + 1])]) for i in range(N_T)]
    snips = [s[5:5 + K] if len(s) >= 5 + K else s[:K] for s in tseq[:3000]]  # one k-mer each: hardly more records than rows
    batches = {"queries": qseq, "foreign": foreign, "mixed": mixed, "few": few, "poly": [POLY] + qseq[:N_Q - 1], "snips": snips}
    _DATA["targets"] = (t_res, t_off)
    _DATA["targets_poly"] = ks.pack(tseq[:N_T - 1] + [POLY])
    for name, seqs in batches.items():
        _DATA[name] = ks.pack(seqs) + (ks.pack(seqs[:SAMPLE]),)
    return _DATA


_WANT = {}


def _oracle_sample(batch):
    """the oracle's rows for the first SAMPLE queries of a batch: made once"""
    if batch not in _WANT:
        D = _data()
        tr, to = D["targets_poly" if batch == "poly" else "targets"]
        s_res, s_off = D[batch][2]
        wt = oracle.sketch_batch(tr, to, K, SCALED, MOL, n_threads=8)
        wq = oracle.sketch_batch(s_res, s_off, K, SCALED, MOL, n_threads=8)
        _WANT[batch] = oracle.manysearch(wq[0], wq[1], wt[0], wt[1], wt[2], n_threads=8)
    return _WANT[batch]


def _eq(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (label, j, len(g), len(w))


def _stats(ctx):
    s = ctx.search_stats(paths=True)
    return s["agg_used"], s["agg_overflows"]


def _index(ctx, name="targets"):
    t_res, t_off = _data()[name]
    return ctx.index_build(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))


def _both_paths(ctx, monkeypatch, ix, batch, expect_agg=True, **kw):
    """the batch searched with the path forced either way, through the two plain calls and the one-call entry; returns the rows"""
    q_res, q_off, _ = _data()[batch]
    n_q = len(q_off) - 1
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "sort")
    u0, o0 = _stats(ctx)
    Hs = ctx.search(ix, Q, **kw)
    assert _stats(ctx) == (u0, o0), "forced sort: the aggregate pass must not run"
    rows = Hs.to_host()
    if not kw:
        sel = rows[0] < SAMPLE
        _eq([c[sel] for c in rows], _oracle_sample(batch), (batch, "oracle"))
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "agg")
    Ha = ctx.search(ix, Q, **kw)
    _eq(Ha.to_host(), rows, (batch, "agg, two calls"))
    assert Ha.count == Hs.count == len(rows[0]) and Ha.n_pair_instances == Hs.n_pair_instances
    f0 = ctx.fused_stats()["aggregated"]
    _, H1 = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res), **kw)
    _eq(H1.to_host(), rows, (batch, "agg, one call"))
    assert H1.count == Hs.count and H1.n_pair_instances == Hs.n_pair_instances
    u1, o1 = _stats(ctx)
    if expect_agg:
        assert (u1 - u0, o1 - o0) == (2, 0), (batch, u1 - u0, o1 - o0)
        assert ctx.fused_stats()["aggregated"] == f0 + 1  # (the one-call entry counts its own: the figure bench.py prints)
    return rows, Hs.n_pair_instances


@pytest.mark.parametrize("segs", [False, True])
@pytest.mark.parametrize("batch", ["queries", "mixed", "few"])
def test_aggregate_rows_equal_sorted_rows_and_oracle(ctx, monkeypatch, batch, segs):
    """dense and segmented list input; `mixed`: queries without a hit between those with one and 45-residue prefixes (regions
    without a record, regions of one row); `few`: 300 queries, fewer than 256 regions in use"""
    for k_, v in (FP_SEGS if segs else {}).items():
        monkeypatch.setenv(k_, v)
    rows, n_pairs = _both_paths(ctx, monkeypatch, _index(ctx), batch)
    assert n_pairs >= 65536 and n_pairs > 8 * len(rows[0])


def test_foreign_batch_hardly_a_hit(ctx, monkeypatch):
    """unrelated random proteins: a list too short for the partition path — forcing the aggregate pass changes nothing"""
    rows, n_pairs = _both_paths(ctx, monkeypatch, _index(ctx), "foreign", expect_agg=False)
    assert n_pairs < 65536


def test_long_single_letter_protein_sums_in_64_bits(ctx, monkeypatch):
    """a 4,074-residue single-letter protein as target and as query: one shared k-mer of abundance 4,065, 12 abundance bits in
    every record of the list (the sum itself fits 32 bits: a sketch made from residues cannot pass 2^32 short of a sequence of
    2^32 windows — test_hand_made_sketches_sum_beyond_32_bits has the sums that do)"""
    rows, _ = _both_paths(ctx, monkeypatch, _index(ctx, "targets_poly"), "poly")
    poly = (rows[0] == 0) & (rows[1] == N_T - 1)  # (query 0 is in the oracle's sample)
    assert poly.sum() == 1 and int(rows[2][poly][0]) == 1 and int(rows[3][poly][0]) == len(POLY) - K + 1


def test_hand_made_sketches_sum_beyond_32_bits_and_sparse_regions(ctx, monkeypatch):
    """Sketches from the host (ks_sketches_from_host), 1,024 targets and 1,024 queries of 80 hashes, query i sharing all of its
    hashes with target i alone: 20 id bits, so a level-1 region is four queries.  Target 0's abundances are all 2^32 - 1: row
    (0, 0) sums 80 of them, 37 bits — a 32-bit sum loses it — and the other targets' are random 32-bit values, so most rows pass
    2^32.  Every sixteenth region is empty (its four queries have no hash), every sixteenth holds ONE record (one query with one
    hash).  The expected rows are written down here, not computed by either path."""
    n, m = 1024, 80
    rng = np.random.default_rng(613)
    hashes = np.unique(rng.integers(1, 2 ** 63, 2 * n * m, dtype=np.uint64))[:n * m]
    assert len(hashes) == n * m
    hashes = np.sort(rng.permutation(hashes).reshape(n, m), axis=1)  # target i: row i, ascending
    abunds = rng.integers(1, 2 ** 32, (n, m), dtype=np.uint64).astype(np.uint32)
    abunds[0, :] = 0xFFFFFFFF
    region = np.arange(n) >> 2
    take = np.full(n, m)
    take[region % 16 == 3] = 0
    take[region % 16 == 7] = 0
    take[(region % 16 == 7) & (np.arange(n) % 4 == 1)] = 1
    t_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)
    q_off = np.concatenate([[0], np.cumsum(take)]).astype(np.uint64)
    q_hashes = np.concatenate([hashes[i, :take[i]] for i in range(n)])
    T = ctx.sketches_from_host(t_off, hashes.reshape(-1), abunds.reshape(-1), K, SCALED, MOL)
    Q = ctx.sketches_from_host(q_off, q_hashes, np.ones(len(q_hashes), np.uint32), K, SCALED, MOL)
    ix = ctx.index_build(T)
    hit = np.nonzero(take)[0]
    want = (hit.astype(np.uint32), hit.astype(np.uint32), take[hit].astype(np.uint32),
            np.array([int(abunds[i, :take[i]].astype(np.uint64).sum()) for i in hit], np.uint64))
    assert int(want[3][0]) == m * 0xFFFFFFFF and (want[3] > 2 ** 32).sum() > len(hit) // 2
    assert int(take.sum()) >= 65536
    for path in ("sort", "agg"):
        monkeypatch.setenv("KS_DEBUG_ROWS_PATH", path)
        u0, o0 = _stats(ctx)
        H = ctx.search(ix, Q)
        _eq(H.to_host(), want, ("hand-made", path))
        assert H.n_pair_instances == int(take.sum())
        assert _stats(ctx) == (u0 + (path == "agg"), o0)


def test_overflow_is_remembered(monkeypatch):
    """no path forced, 16 usable slots per table: the second search of a fresh context tries the aggregate pass and overflows,
    the third does not try again — nor does the fourth with whole tables (the context remembers the row count that overflowed,
    not why); a batch of a third of the queries, under half as many rows, is tried again and fits"""
    monkeypatch.delenv("KS_DEBUG_ROWS_PATH", raising=False)
    monkeypatch.setenv("KS_DEBUG_AGG_CAP", "16")
    c = ks.Context(0)
    try:
        ix = _index(c)
        q_res, q_off, _ = _data()["queries"]
        Q = c.sketch_batch(q_res, q_off, K, SCALED, MOL)
        third = ks.pack([bytes(q_res[int(q_off[i]):int(q_off[i + 1])]) for i in range(N_Q // 3)])
        Q3 = c.sketch_batch(third[0], third[1], K, SCALED, MOL)
        first = c.search(ix, Q).to_host()
        assert _stats(c) == (0, 0)
        _eq(c.search(ix, Q).to_host(), first, "overflowing search")
        assert _stats(c) == (0, 1)
        _eq(c.search(ix, Q).to_host(), first, "after the overflow")
        assert _stats(c) == (0, 1)
        monkeypatch.delenv("KS_DEBUG_AGG_CAP")
        c.reload_debug_env()
        _eq(c.search(ix, Q).to_host(), first, "whole tables, same rows expected")
        assert _stats(c) == (0, 1)
        H3 = c.search(ix, Q3)
        assert H3.n_pair_instances >= 65536 and 2 * H3.count < len(first[0])
        assert _stats(c) == (1, 1)
        sel = first[0] < N_Q // 3
        _eq(H3.to_host(), [col[sel] for col in first], "a third of the queries")
    finally:
        c.close()


def _region_fill(rows, n_q):
    """distinct rows of the fullest level-1 region: the top 8 of the qbits + tbits id bits"""
    qbits, tbits = max(1, (n_q - 1).bit_length()), max(1, (N_T - 1).bit_length())
    key = (rows[0].astype(np.uint64) << np.uint64(tbits)) | rows[1].astype(np.uint64)
    return int(np.bincount((key >> np.uint64(qbits + tbits - 8)).astype(np.int64), minlength=256).max())


def test_nearly_full_table_wraps_and_small_table_overflows(ctx, monkeypatch):
    ix = _index(ctx)
    q_res, q_off, _ = _data()["queries"]
    n_q = len(q_off) - 1
    d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
    Q = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "sort")
    want = ctx.search(ix, Q).to_host()
    fill = _region_fill(want, n_q)
    assert 16 < fill < 4096
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "agg")
    # one free slot in the fullest region's table: probe chains run to the table's end and wrap
    monkeypatch.setenv("KS_DEBUG_AGG_CAP", str(fill + 1))
    u0, o0 = _stats(ctx)
    _eq(ctx.search(ix, Q).to_host(), want, "cap = fill + 1")
    assert _stats(ctx) == (u0 + 1, o0)
    # exactly full: still every row has its slot
    monkeypatch.setenv("KS_DEBUG_AGG_CAP", str(fill))
    _eq(ctx.search(ix, Q).to_host(), want, "cap = fill")
    assert _stats(ctx) == (u0 + 2, o0)
    # 16 slots: the fullest region overflows, the sort resumes on the level-1 output — same rows, no aggregate pass counted
    monkeypatch.setenv("KS_DEBUG_AGG_CAP", "16")
    H = ctx.search(ix, Q)
    _eq(H.to_host(), want, "cap = 16")
    assert _stats(ctx) == (u0 + 2, o0 + 1)
    _, H1 = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, n_q, len(q_res))
    _eq(H1.to_host(), want, "cap = 16, one call")
    assert _stats(ctx) == (u0 + 2, o0 + 2)


def test_query_slices(ctx, monkeypatch):
    """records narrowed to slices of 8,192 queries (KS_DEBUG_RECORD_BITS): every slice is a search of its own"""
    ix = _index(ctx)
    q_res, q_off, _ = _data()["queries"]
    n_q = len(q_off) - 1
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "sort")
    Q = ctx.sketch_batch(q_res, q_off, K, SCALED, MOL)
    want = ctx.search(ix, Q).to_host()
    abits = int(ctx.sketch_batch(*_data()["targets"], K, SCALED, MOL).to_host()[2].max()).bit_length()
    monkeypatch.setenv("KS_DEBUG_RECORD_BITS", str((N_T - 1).bit_length() + abits + 13))
    _eq(ctx.search(ix, Q).to_host(), want, "sliced, sort")
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "agg")
    u0, o0 = _stats(ctx)
    _eq(ctx.search(ix, Q).to_host(), want, "sliced, agg")
    u1, o1 = _stats(ctx)
    assert u1 - u0 >= 1 and o1 == o0
    assert n_q > 8192


@pytest.mark.parametrize("min_c", [0.05, 0.5])
def test_min_containment_on_both_paths(ctx, monkeypatch, min_c):
    rows, _ = _both_paths(ctx, monkeypatch, _index(ctx), "queries", min_containment=min_c)
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "agg")
    q_res, q_off, _ = _data()["queries"]
    Q = ctx.sketch_batch(q_res, q_off, K, SCALED, MOL)
    every = ctx.search(_index(ctx), Q).to_host()
    sizes = (Q.to_host()[0][1:] - Q.to_host()[0][:-1]).astype(np.float64)
    keep = every[2].astype(np.float64) / sizes[every[0]] >= min_c
    assert 0 < keep.sum() <= len(keep)
    _eq(rows, [c[keep] for c in every], ("min_containment", min_c))


def test_abund_stats_take_the_sort(ctx, monkeypatch):
    """the statistics read the sorted list: the aggregate pass is not taken even when forced"""
    ix = _index(ctx)
    q_res, q_off, _ = _data()["queries"]
    Q = ctx.sketch_batch(q_res, q_off, K, SCALED, MOL)
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "sort")
    Hs = ctx.search(ix, Q, abund_stats=True)
    monkeypatch.setenv("KS_DEBUG_ROWS_PATH", "agg")
    before = _stats(ctx)
    Ha = ctx.search(ix, Q, abund_stats=True)
    assert _stats(ctx) == before
    _eq(Ha.to_host(), Hs.to_host(), "rows")
    _eq(Ha.abund_stats_to_host(), Hs.abund_stats_to_host(), "statistics")


def test_history_decides_the_path(monkeypatch):
    """a fresh context: the first search sorts, the second aggregates (the first had many records per row); a batch with hardly
    more records than rows sends the next search back to the sort, after which the history is high again"""
    monkeypatch.delenv("KS_DEBUG_ROWS_PATH", raising=False)
    c = ks.Context(0)
    try:
        ix = _index(c)
        D = _data()
        Q = c.sketch_batch(D["queries"][0], D["queries"][1], K, SCALED, MOL)
        F = c.sketch_batch(D["snips"][0], D["snips"][1], K, SCALED, MOL)
        first = c.search(ix, Q).to_host()
        assert _stats(c) == (0, 0)
        _eq(c.search(ix, Q).to_host(), first, "second search")
        assert _stats(c) == (1, 0)
        low = c.search(ix, F)
        assert 0 < low.n_pair_instances < 8 * low.count
        assert _stats(c) == (1, 0)
        _eq(c.search(ix, Q).to_host(), first, "after the low-multiplicity batch")
        assert _stats(c) == (1, 0)
        _eq(c.search(ix, Q).to_host(), first, "history high again")
        assert _stats(c) == (2, 0)
        assert "agg_used" not in c.search_stats() and c.search_stats()["agg_overflows"] == 0
    finally:
        c.close()
