"""W different ranks of the hit exchange (kmerseek_amd/dist.py) in one process, and a numpy reference of what they gather.

``Ranks`` stands in for ``dist._dist`` and ``dist.world_info`` (install() monkeypatches both).  It is given the W per-rank row
counts up front and answers the 1-element count all-gather from them; the layout of a send block depends on the counts alone,
so every rank's block is well-formed from its first run.  run(fn) then plays the ranks one after another, in passes:

* in a pass, rank r runs fn(r) once; the stand-in keeps a clone of the send block of every data all-gather, per rank and per
  call index (the packed exchange is call 0; the unpacked repeat after an escape overflow is call 1), and fills ``recv`` from
  the blocks recorded so far — the calling rank's own block from its live ``send``, a block nobody has recorded yet with zeros;
* the passes repeat until one of them found every block it asked for, and the results of that pass are the ones returned.
  Without an overflow that is the second pass.  With an overflow in one rank only, the ranks in front of it learn of it in the
  second pass and send their unpacked columns there for the first time, so the complete pass is the second or the third.

So every rank's ``recv`` is built from W different, real send blocks.  With ``async_op=True`` the call returns an object with
``wait()`` and ``recv`` is filled only there: a finish() that reads before it waits reads what torch.empty left.

gathered_reference() is the expected result in plain numpy: ids shifted, blocks concatenated in rank order, and for an
index-sharded gather in qid order a stable argsort on qid."""
import numpy as np

MAX_PASSES = 4


class _Work:
    def __init__(self, fill):
        self._fill = fill

    def wait(self):
        if self._fill is not None:
            fill, self._fill = self._fill, None
            fill()
        return True


class Ranks:
    def __init__(self, counts):
        self.counts = [int(c) for c in counts]
        self.world = len(self.counts)
        self.rank = 0
        self.blocks = [dict() for _ in range(self.world)]  # blocks[r][call index] = clone of rank r's send block
        self.calls = []      # (rank, call index, elements of the send block, async_op) of the pass that is running
        self.passes = 0
        self._missing = 0
        self._call = 0
        self._pending = []

    # ---- what dist.py asks of torch.distributed ----------------------------------------------------------------------
    def __call__(self):  # dist._dist()
        return self

    def world_info(self):
        return self.rank, self.world

    @staticmethod
    def is_available():
        return True

    @staticmethod
    def is_initialized():
        return True

    def all_gather_into_tensor(self, recv, send, async_op=False):
        n = send.numel()
        assert recv.numel() == self.world * n and recv.dtype == send.dtype and recv.device == send.device
        if n == 1:  # the count exchange
            assert int(send[0]) == self.counts[self.rank], (self.rank, int(send[0]), self.counts[self.rank])
            recv.copy_(recv.new_tensor(self.counts))
            return _Work(None) if async_op else None
        idx, self._call = self._call, self._call + 1
        self.calls.append((self.rank, idx, n, bool(async_op)))
        mine = send.clone()
        sources = []
        for r in range(self.world):
            blk = mine if r == self.rank else self.blocks[r].get(idx)
            if blk is None:
                self._missing += 1
            else:
                assert blk.numel() == n and blk.dtype == send.dtype, (r, idx, blk.numel(), n)
            sources.append(blk)
        self.blocks[self.rank][idx] = mine

        def fill():
            for r, blk in enumerate(sources):
                if blk is None:
                    recv[r * n:(r + 1) * n].zero_()
                else:
                    recv[r * n:(r + 1) * n].copy_(blk)
        if not async_op:
            fill()
            return None
        work = _Work(fill)
        self._pending.append(work)
        return work

    # ---- the driver --------------------------------------------------------------------------------------------------
    def install(self, monkeypatch, ksd):
        monkeypatch.setattr(ksd, "_dist", self)
        monkeypatch.setattr(ksd, "world_info", self.world_info)
        return self

    def run(self, fn):
        """fn(rank) -> that rank's gathered result.  Returns the W results of the first pass that found every block."""
        while True:
            assert self.passes < MAX_PASSES, "the exchange keeps asking for blocks nobody sent"
            self.passes += 1
            self._missing = 0
            self.calls = []
            out = []
            for r in range(self.world):
                self.rank, self._call, self._pending = r, 0, []
                out.append(fn(r))
                assert all(w._fill is None for w in self._pending), f"rank {r} never waited for a collective it started"
            if self._missing == 0:
                return out

    def data_calls(self, rank):
        """(call index, elements, async_op) of rank's data all-gathers in the last pass"""
        return [c[1:] for c in self.calls if c[0] == rank]


def gathered_reference(per_rank, qid_bases, tid_bases, sharded, order):
    """per_rank: the W host hit lists (qid, tid, intersect, n_weighted), local ids.  Returns the expected gathered columns
    (qid u32, tid u32, intersect u32, n_weighted u64)."""
    assert sharded in ("queries", "index") and order in ("qid", "shard")
    assert len(per_rank) == len(qid_bases) == len(tid_bases)
    qid = np.concatenate([np.asarray(h[0]).astype(np.int64) + int(b) for h, b in zip(per_rank, qid_bases)])
    tid = np.concatenate([np.asarray(h[1]).astype(np.int64) + int(b) for h, b in zip(per_rank, tid_bases)])
    assert (len(qid) == 0) or (qid.max() < 1 << 32 and tid.max() < 1 << 32)
    isect = np.concatenate([np.asarray(h[2]).astype(np.uint32) for h in per_rank])
    nw = np.concatenate([np.asarray(h[3]).astype(np.uint64) for h in per_rank])
    cols = [qid.astype(np.uint32), tid.astype(np.uint32), isect, nw]
    if sharded == "index" and order == "qid":
        o = np.argsort(cols[0], kind="stable")
        cols = [c[o] for c in cols]
    return tuple(cols)


def padded_cap(counts):
    """rows per rank block of either exchange: the largest count, rounded up to 64"""
    return (max(max(counts), 1) + 63) // 64 * 64


def escape_cap(counts):
    """entries of a rank's escape list (dist._gather_packed_begin)"""
    return max(1024, padded_cap(counts) // 64) // 2 * 2


def value_bits(id_counts):
    """(qbits, tbits, v) of the transport word for a job of id_counts = (n_queries, n_targets)"""
    def bits(n):
        return max(1, int(n - 1).bit_length()) if n > 1 else 1
    q, t = bits(id_counts[0]), bits(id_counts[1])
    return q, t, (64 - q - t) // 2


def escapes(hits, v):
    """rows of a host hit list that take the escape list with v value bits (the all-ones value is the marker: it escapes too)"""
    vmax = (1 << v) - 1
    return np.flatnonzero((np.asarray(hits[2]).astype(np.uint64) >= vmax) | (np.asarray(hits[3]).astype(np.uint64) >= vmax))


def as_host(cols):
    """gathered torch columns (i32, i32, i32, i64) -> numpy (u32, u32, u32, u64)"""
    return tuple(c.cpu().numpy().view(dt) for c, dt in zip(cols, (np.uint32, np.uint32, np.uint32, np.uint64)))
