"""CPU: the stand-in collective of tests/exchange_ranks.py, proven on the host path of the hit exchange before the GPU tests
(tests/test_gpu_exchange.py) lean on it — and that host path (numpy packing, torch unpack, escape patch, torch.sort) pinned down
with more than two ranks: W in {2, 3, 5}, unequal counts, a rank with no rows first / in the middle / last, escapes in a middle
rank only, and an escape overflow in one rank only, after which every rank repeats the exchange with unpacked columns.
Every simulated rank must return the numpy reference, exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exchange_ranks as xr  # noqa: E402
from kmerseek_amd import dist as ksd  # noqa: E402

WIDE_IDS = (1 << 20, 1 << 20)  # 20 + 20 id bits: 12 value bits, the all-ones marker is 4095
N_Q = 1000

# name -> (rows per rank, rank with escapes or None, escaping rows in it)
SHARDS = {
    "w2": ([700, 130], None, 0),
    "w3_zero_first": ([0, 500, 77], None, 0),
    "w3_zero_middle": ([300, 0, 900], None, 0),
    "w3_zero_last": ([500, 77, 0], None, 0),
    "w5": ([64, 0, 1500, 129, 640], None, 0),
    "w3_escapes_middle": ([400, 350, 90], 1, 40),
    "w5_escapes_middle": ([65, 0, 1200, 300, 31], 2, 1024),  # (exactly the capacity of the list: no overflow)
    "w3_overflow_middle": ([200, 1300, 64], 1, 1100),
    "w5_overflow_last_but_one": ([10, 1300, 0, 1026, 3], 3, 1025),  # (one more than the list takes)
}
SPLITS = [("index", "qid"), ("index", "shard"), ("queries", "qid")]


def _shards(name, sharded):
    """per-rank host hit lists (local ids, each ordered by (qid, tid)), their id bases, and the escapes of every rank"""
    counts, esc_rank, n_esc = SHARDS[name]
    rng = np.random.default_rng([7, len(counts), sum(counts)])
    _, _, v = xr.value_bits(WIDE_IDS)
    vmax = (1 << v) - 1
    hits, qb, tb = [], [], []
    serial = 0
    for r, n in enumerate(counts):
        n_t_local = 100 + 13 * r if sharded == "index" else 400
        n_q_local = N_Q if sharded == "index" else 60 + 9 * r
        key = np.sort(rng.choice(n_q_local * n_t_local, n, replace=False))
        s = serial + np.arange(n, dtype=np.uint64)
        serial += n
        isect = (1 + s % 200).astype(np.uint32)
        nw = isect.astype(np.uint64) + s % 7
        if r == esc_rank:
            rows = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), n_esc - 2, replace=False)]))  # first and last row too
            nw[rows] = (1 << 40) + s[rows]
            isect[rows[::2]] = 5000 + (s[rows[::2]] % 100000).astype(np.uint32)
            nw[rows[1]], isect[rows[1]] = vmax, 3      # the marker itself
            nw[rows[2]], isect[rows[2]] = vmax + 1, 3  # and one above it
            isect[rows[3]], nw[rows[3]] = vmax, vmax   # intersect alone at the marker
        hits.append(((key // n_t_local).astype(np.uint32), (key % n_t_local).astype(np.uint32), isect, nw))
        qb.append(0 if sharded == "index" else sum(60 + 9 * i for i in range(r)))
        tb.append(sum(100 + 13 * i for i in range(r)) if sharded == "index" else 0)
    want_esc = [n_esc if r == esc_rank else 0 for r in range(len(counts))]
    assert [len(xr.escapes(h, v)) for h in hits] == want_esc  # (from the rows themselves)
    return counts, hits, qb, tb, want_esc


@pytest.mark.parametrize("api", ["all_gather", "begin_finish"])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("sharded,order", SPLITS)
@pytest.mark.parametrize("name", list(SHARDS))
def test_host_exchange_on_different_shards(monkeypatch, name, sharded, order, packed, api):
    counts, hits, qb, tb, n_esc = _shards(name, sharded)
    want = xr.gathered_reference(hits, qb, tb, sharded, order)
    assert len(want[0]) == sum(counts) and len(set(counts)) > 1
    cap = xr.padded_cap(counts)
    assert all(c == max(counts) or cap - c > 0 for c in counts) and min(counts) < cap  # the smaller blocks carry padding
    esc_cap = xr.escape_cap(counts)
    assert esc_cap == 1024
    overflow = packed and max(n_esc) > esc_cap
    assert ("overflow" in name) == (max(n_esc) > esc_cap) and ("escapes" in name) == (0 < max(n_esc) <= esc_cap)
    ranks = xr.Ranks(counts).install(monkeypatch, ksd)
    call = ksd.all_gather_hits_device if api == "all_gather" else (lambda *a, **k: ksd.begin_all_gather_hits_device(*a, **k).finish())

    def one(r):
        return call(hits[r], qid_base=qb[r], tid_base=tb[r], sharded=sharded, order=order, id_counts=WIDE_IDS if packed else None)
    out = ranks.run(one)
    # (ranks behind the overflowing one see its escape count in the first pass already; a rank between rank 0 and that one
    # sends its unpacked columns in the second pass for the first time, and the third pass is the complete one)
    assert ranks.passes == (3 if overflow and SHARDS[name][1] >= 2 else 2)
    _, _, v = xr.value_bits(WIDE_IDS)
    words = cap + 1 + 2 * esc_cap
    for r, got in enumerate(out):
        assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.int32, torch.int64]
        for j, (g, w) in enumerate(zip(xr.as_host(got), want)):
            assert np.array_equal(g, w), (name, "rank", r, "column", j)
        sizes = [n for _, n, _ in ranks.data_calls(r)]
        assert sizes == ([words, 5 * cap] if overflow else [words] if packed else [5 * cap]), (r, sizes)


def test_reference_orders_by_qid_then_rank():
    a = (np.array([0, 2, 2], np.uint32), np.array([1, 0, 3], np.uint32), np.array([1, 2, 3], np.uint32), np.array([1, 2, 3], np.uint64))
    b = (np.array([1, 2], np.uint32), np.array([0, 1], np.uint32), np.array([4, 5], np.uint32), np.array([4, 1 << 40], np.uint64))
    q, t, i, w = xr.gathered_reference([a, b], [0, 0], [0, 10], "index", "qid")
    assert q.tolist() == [0, 1, 2, 2, 2] and t.tolist() == [1, 10, 0, 3, 11] and i.tolist() == [1, 4, 2, 3, 5]
    assert w.tolist() == [1, 4, 2, 3, 1 << 40] and w.dtype == np.uint64 and q.dtype == np.uint32
    q, t, i, w = xr.gathered_reference([a, b], [0, 0], [0, 10], "index", "shard")
    assert q.tolist() == [0, 2, 2, 1, 2] and t.tolist() == [1, 0, 3, 10, 11]
    q, t, i, w = xr.gathered_reference([a, b], [0, 3], [0, 0], "queries", "qid")
    assert q.tolist() == [0, 2, 2, 4, 5] and t.tolist() == [1, 0, 3, 0, 1]


def test_stand_in_serves_every_rank_the_other_ranks_blocks(monkeypatch):
    """the stand-in by itself: three ranks with different blocks, a synchronous and an asynchronous call"""
    ranks = xr.Ranks([3, 0, 5])
    seen = {}

    def one(r):
        c = torch.zeros(3, dtype=torch.int64)
        assert ranks.all_gather_into_tensor(c, torch.tensor([ranks.counts[r]])) is None
        assert c.tolist() == [3, 0, 5] and ranks.world_info() == (r, 3)
        send = torch.arange(4, dtype=torch.int32) + 10 * (r + 1)
        recv = torch.full((12,), -1, dtype=torch.int32)
        work = ranks.all_gather_into_tensor(recv, send, async_op=True)
        assert recv.tolist() == [-1] * 12  # (filled by wait(), not before)
        assert work.wait() is True
        recv2 = torch.full((12,), -1, dtype=torch.int32)
        ranks.all_gather_into_tensor(recv2, send + 100)
        seen[r] = (recv.tolist(), recv2.tolist())
        return r
    assert ranks.run(one) == [0, 1, 2] and ranks.passes == 2
    blocks = sum(([10 * (r + 1) + i for i in range(4)] for r in range(3)), [])
    for r in range(3):
        assert seen[r] == (blocks, [b + 100 for b in blocks])
        assert ranks.data_calls(r) == [(0, 4, True), (1, 4, False)]
    with pytest.raises(AssertionError):  # a count that is not the one announced
        ranks.rank = 1
        ranks.all_gather_into_tensor(torch.zeros(3, dtype=torch.int64), torch.tensor([4]))
    lazy = xr.Ranks([1, 1])
    with pytest.raises(AssertionError):  # a collective that was started and never waited for
        lazy.run(lambda r: lazy.all_gather_into_tensor(torch.zeros(4), torch.ones(2), async_op=True))
