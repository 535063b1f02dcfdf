"""GPU: ks_frames_fold_device — the frame rows of a translated search folded per (record, strand, target), their regions on the
strand's bases — the chain over the fold, and the translated search of the wire.

Every column and the folded hit list are compared exactly with the plain-loop restatement of tests/ffold_ref.py.  The synthetic
hit lists come from a real search of crafted sketches (one private hash per wanted row, as tests/crafted_sketches.py builds its
families), with intersect and n_weighted then uploaded into the list's device columns: a few thousand rows over 300 records and 40
targets, strand runs across the workgroup boundaries of the fold's kernels and across a tile boundary of the one-launch scan.
The end-to-end case plants one gene per contig, half of them on the reverse strand, half of them with a frameshift."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as crafted  # noqa: E402
import ffold_ref  # noqa: E402
import rchain_cases as RH  # noqa: E402
import rchain_ref  # noqa: E402
import translate_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MOL = 7, "protein"
N_REC, N_T = 300, 40
INVALID, CAPACITY, OOM = _lib.KS_ERR_INVALID_ARG, _lib.KS_ERR_CAPACITY, _lib.KS_ERR_OOM
WORKGROUP = 256  # threads of a workgroup of the fold's kernels (FF_THREADS, ks_ffold.hip)


def scan_tile():
    """the tile of the one-launch scan, from ks_prims.hip"""
    src = open(os.path.join(ROOT, "kmerseek_amd", "csrc", "ks_prims.hip")).read()
    threads, ipt = (int(re.search(r"#define\s+%s\s+(\d+)" % n, src).group(1)) for n in ("SCAN_THREADS", "SCAN_IPT"))
    assert re.search(r"#define\s+SCAN_TILE\s+\(SCAN_THREADS \* SCAN_IPT\)", src)
    return threads * ipt


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


def upload_into(ctx, d_ptr, a):
    a = np.ascontiguousarray(a)
    ctx._check(ctx._L.ks_dev_upload(ctx._h, C.c_void_p(int(d_ptr)), a.ctypes.data_as(C.c_void_p), a.nbytes))


def make_hits(ctx, qid, tid, isect, nw, n_q, n_t):
    """A Hits with exactly the rows (qid[i], tid[i]) — ascending — from a search of crafted sketches in which every row has one
    private hash; intersect and n_weighted are then uploaded into the list's device columns."""
    n = len(qid)
    h = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))  # (an odd multiplier: distinct, never 0)
    one = np.ones(n, np.uint32)
    if n:
        Q, T = crafted._csr(qid, h, one, n_q), crafted._csr(tid, h, one, n_t)
    else:  # no row: two sketches that share nothing
        Q, T = crafted._csr([0], [2], [1], n_q), crafted._csr([0], [4], [1], n_t)
    sq, st = ctx.sketches_from_host(*Q, 10, 1, MOL), ctx.sketches_from_host(*T, 10, 1, MOL)
    ix = ctx.index_build(st)
    hits = ctx.search(ix, sq)
    for o in (ix, sq, st):
        o.free()
    got = hits.to_host()
    assert np.array_equal(got[0], np.asarray(qid, np.uint32)) and np.array_equal(got[1], np.asarray(tid, np.uint32))
    p = hits.device_ptrs()
    if n:
        upload_into(ctx, p[2], np.asarray(isect, np.uint32)); upload_into(ctx, p[3], np.asarray(nw, np.uint64))
    ctx.synchronize()
    return hits


@functools.lru_cache(maxsize=None)
def synthetic():
    """-> dict: the hit rows, record offsets, region CSR and columns of the synthetic input, and its reference folds"""
    rng = np.random.default_rng(20261)
    lengths = rng.integers(60, 400, N_REC)
    lengths[:3] = (90, 91, 92)
    nt_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    silent = set(range(100, 111)) | {5, 250}  # records without rows
    rows = []
    for s in range(N_REC):
        if s in silent:
            continue
        p = 0.2 if s in (0, N_REC - 1) else 0.09
        for f6 in range(6):
            for t in np.flatnonzero(rng.random(N_T) < p):
                rows.append((6 * s + f6, int(t)))
    rows += [(0, 3), (2, 3), (6 * (N_REC - 1) + 5, N_T - 1), (6 * (N_REC - 1) + 3, N_T - 1), (6 * (N_REC - 1) + 4, N_T - 1)]
    rows = sorted(set(rows))
    qid = np.array([q for q, _ in rows], np.uint32)
    tid = np.array([t for _, t in rows], np.uint32)
    n_rows = len(rows)
    counts = rng.integers(0, 6, n_rows)
    counts[rng.random(n_rows) < 0.1] = 0
    counts[n_rows // 2] = 300
    counts[0], counts[-1] = 2, 0
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(row_off[-1])
    row_of = np.repeat(np.arange(n_rows), counts)
    flen = np.array([ffold_ref.frame_len(int(lengths[q // 6]), q % 3) for q in qid.tolist()])[row_of]
    ql = 1 + (rng.random(n) * flen).astype(np.int64)
    ql = np.minimum(ql, flen)
    qs = (rng.random(n) * (flen - ql + 1)).astype(np.int64)
    edge = rng.random(n)
    qs[edge < 0.1] = 0
    qs[edge > 0.9] = (flen - ql)[edge > 0.9]
    assert np.all(qs + ql <= flen) and np.any(qs + ql == flen) and np.any(qs == 0)
    cols = dict(q_start=qs.astype(np.uint32), q_length=ql.astype(np.uint32), t_start=rng.integers(0, 1000, n).astype(np.uint32),
                t_length=rng.integers(1, 60, n).astype(np.uint32), score=rng.integers(-1000, 1000, n).astype(np.int64),
                identities=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), aln_length=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    isect = rng.integers(1, 50, n_rows).astype(np.uint32)
    nw = rng.integers(0, 2 ** 40, n_rows, dtype=np.uint64)
    isect[rows.index((0, 3))], isect[rows.index((2, 3))] = 2 ** 32 - 1, 7  # two members of one folded row: the sum saturates
    last = [rows.index((6 * (N_REC - 1) + f, N_T - 1)) for f in (3, 4, 5)]      # ... and three whose sum is exactly 2^32 - 1
    isect[last] = (2 ** 31, 2 ** 31 - 1, 0)
    nw[last] = (2 ** 63, 2 ** 62, 5)
    # the geometry the case is for: strand runs across a workgroup boundary and across a tile boundary of the scan
    tile = scan_tile()
    strand = (qid // 3).tolist()
    assert 3 * tile < n_rows < 8000, n_rows  # (four scan tiles: a tile in the middle has a predecessor and a successor)
    assert any(strand[b - 1] == strand[b] for b in range(WORKGROUP, n_rows, WORKGROUP))
    assert any(strand[b - 1] == strand[b] and tid[b - 1] != tid[b] for b in range(tile, n_rows, tile)), "no strand run across a scan tile"
    assert strand[0] == 0 and strand[-1] == 2 * N_REC - 1 and not any(s in silent for s in (qid // 6).tolist())
    D = dict(qid=qid, tid=tid, isect=isect, nw=nw, nt_off=nt_off, row_off=row_off, n=n, **cols)
    base = (qid, tid, isect, nw, nt_off, row_off, cols["q_start"], cols["q_length"], cols["t_start"])
    D["want"] = {
        "full": ffold_ref.fold(*base, cols["t_length"], score=cols["score"], identities=cols["identities"], aln_length=cols["aln_length"]),
        "bare": ffold_ref.fold(*base, cols["t_length"]),
        "no_t_length": ffold_ref.fold(*base, None, score=cols["score"]),
    }
    fq, ft, fi, fw = D["want"]["full"][0]
    assert (int(fq[-1]), int(ft[-1]), int(fi[-1]), int(fw[-1])) == (2 * N_REC - 1, N_T - 1, 2 ** 32 - 1, 2 ** 63 + 2 ** 62 + 5)
    assert int(fi[np.flatnonzero((fq == 0) & (ft == 3))[0]]) == 2 ** 32 - 1
    return D


def device_fold(ctx, hits, nt_off, row_off, cols, variant="full"):
    """the columns uploaded with Context.to_device and folded by fold_frames_device -> (FrameFold, the device buffers)"""
    names = ["q_start", "q_length", "t_start", "t_length", "score", "identities", "aln_length"]
    if variant == "bare":
        names = names[:4]
    if variant == "no_t_length":
        names = ["q_start", "q_length", "t_start", "score"]
    bufs = {k: ctx.to_device(cols[k] if len(cols[k]) else np.zeros(1, cols[k].dtype)) for k in names}
    bufs["nt_off"], bufs["row_off"] = ctx.to_device(nt_off), ctx.to_device(row_off)
    p = {k: b.ptr for k, b in bufs.items()}
    try:
        fold = ctx.fold_frames_device(hits, p["nt_off"], len(nt_off) - 1, p["row_off"], p["q_start"], p["q_length"], p["t_start"], p.get("t_length"),
                                      len(cols["q_start"]), d_score=p.get("score"), d_identities=p.get("identities"), d_aln_length=p.get("aln_length"))
    finally:
        for b in bufs.values():
            b.free()
    return fold


@pytest.fixture(scope="module")
def synth_hits(ctx):
    D = synthetic()
    hits = make_hits(ctx, D["qid"], D["tid"], D["isect"], D["nw"], 6 * N_REC, N_T)
    yield hits
    hits.free()


@pytest.mark.parametrize("variant", ["full", "bare", "no_t_length"])
def test_synthetic_fold_equals_reference(ctx, synth_hits, variant):
    D = synthetic()
    before = ctx.pool_stats()["bytes_in_use"]
    fold = device_fold(ctx, synth_hits, D["nt_off"], D["row_off"], D, variant)
    want_hits, want = D["want"][variant]
    assert (fold.n_rows, fold.n_regions, fold.n_src_rows) == (len(want_hits[0]), D["n"], len(D["qid"])) and fold.hits.count == fold.n_rows
    assert (fold.has_score, fold.has_identities, fold.has_aln_length) == tuple(want[i] is not None for i in (9, 10, 11))
    ptrs = fold.device_ptrs()
    assert all((p != 0) == (w is not None) for p, w in zip(ptrs, want))
    ffold_ref.assert_same(fold.hits.to_host(), fold.to_host(), want_hits, want, variant)
    assert not fold.hits.has_abund_stats and fold.hits.best_to_host() is None
    assert (fold.hits.n_pair_instances, fold.hits.partition_path, fold.hits.bucket_posting_bytes) == (
        synth_hits.n_pair_instances, synth_hits.partition_path, synth_hits.bucket_posting_bytes)
    if variant == "bare":
        with pytest.raises(ValueError):
            ctx.chain_frames(fold)
    else:  # the chain over the fold is the reference chain over the reference fold
        opts = {"max_overlap": 30, "skew_cost": 1, "link_cost": 3}
        ch = ctx.chain_frames(fold, **opts)
        c = dict(zip(ffold_ref.NAMES, want))
        sums = {"identities": c["identities"], "aln_length": c["aln_length"]} if variant == "full" else {}
        RH.assert_same(ch.to_host(), rchain_ref.chain(c["row_offsets"], c["s_start"], c["nt_length"], c["t_start3"], c["t_length3"], c["score"], **sums, **opts), variant)
        assert ch.n_rows == fold.n_rows
        ch.free()
    fold.free()
    assert ctx.pool_stats()["bytes_in_use"] == before


def test_empty_inputs(ctx):
    z32, z64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    cols = dict(q_start=z32, q_length=z32, t_start=z32, t_length=z32, score=np.zeros(0, np.int64))
    empty = make_hits(ctx, z32, z32, z32, z64, 12, 3)
    fold = device_fold(ctx, empty, np.array([0, 30, 61], np.uint64), np.zeros(1, np.uint64), cols, "no_t_length")
    assert (fold.n_rows, fold.n_regions, fold.n_src_rows, fold.hits.count) == (0, 0, 0, 0)
    got = fold.to_host()
    assert got[1].tolist() == [0] and all(len(c) == 0 for i, c in enumerate(got) if i != 1)
    ch = ctx.chain_frames(fold)
    assert ch.n_rows == 0
    ch.free(); fold.free(); empty.free()
    # rows, none of which has a region
    qid, tid = np.array([1, 2, 7], np.uint32), np.array([2, 2, 0], np.uint32)
    hits = make_hits(ctx, qid, tid, [1, 2, 3], [4, 5, 6], 12, 3)
    nt_off, row_off = np.array([0, 30, 61], np.uint64), np.zeros(4, np.uint64)
    fold = device_fold(ctx, hits, nt_off, row_off, cols, "no_t_length")
    want_hits, want = ffold_ref.fold(qid, tid, [1, 2, 3], [4, 5, 6], nt_off, row_off, z32, z32, z32, score=np.zeros(0, np.int64))
    ffold_ref.assert_same(fold.hits.to_host(), fold.to_host(), want_hits, want, "rows without regions")
    assert fold.n_rows == 2 and fold.to_host()[0].tolist() == [ffold_ref.NONE, 0, 1, ffold_ref.NONE, 2, ffold_ref.NONE]
    fold.free(); hits.free()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
SMALL_ROWS = [(0, 5), (0, 7), (1, 3), (1, 7), (2, 5), (2, 7), (3, 5), (4, 5), (13, 2), (17, 0), (22, 1)]
SMALL_COUNTS = [2, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1]
SMALL_REGIONS = [(0, 4, 1, 4), (6, 4, 8, 5), (2, 3, 0, 3), (0, 9, 3, 9), (5, 4, 20, 4), (1, 2, 10, 2), (0, 10, 0, 10), (8, 1, 2, 1), (9, 1, 0, 1), (7, 3, 0, 3)]


def small_case():
    """the hand-written case of tests/test_ffold_cpu.py: 4 records of 30, 31, 32 and 31 bases, 11 rows, 10 regions"""
    qid, tid = np.array([q for q, _ in SMALL_ROWS], np.uint32), np.array([t for _, t in SMALL_ROWS], np.uint32)
    cols = {k: np.array([g[i] for g in SMALL_REGIONS], np.uint32) for i, k in enumerate(("q_start", "q_length", "t_start", "t_length"))}
    cols["score"] = np.arange(10, dtype=np.int64)
    return dict(qid=qid, tid=tid, isect=np.arange(1, 12, dtype=np.uint32), nw=np.arange(10, 120, 10, dtype=np.uint64),
                nt_off=np.array([0, 30, 61, 93, 124], np.uint64), row_off=np.concatenate([[0], np.cumsum(SMALL_COUNTS)]).astype(np.uint64), cols=cols)


REFUSALS = [
    ("offsets", 0, dict(nt_off=[1, 30, 61, 93, 124])), ("offsets", 2, dict(nt_off=[0, 30, 61, 60, 124])),
    ("long", 1, dict(nt_off=[0, 30, 30 + 2 ** 32 - 15, 2 ** 32 + 100, 2 ** 32 + 200])),
    ("qid", 10, dict(nt_off=[0, 30, 61, 93])), ("order", 4, dict(swap=(3, 4))), ("order", 6, dict(dup=6)),
    ("csr", 0, dict(row_off={0: 1})), ("csr", 3, dict(row_off={4: 2})), ("csr", 10, dict(row_off={11: 9})),
    ("qend", 7, dict(reg=(7, "q_length", 2))), ("qend", 3, dict(reg=(3, "q_start", 1))), ("tend", 5, dict(reg=(5, "t_start", (2 ** 32 - 1) // 3 - 1))),
]
WORDS = {"offsets": "record offsets", "long": "longer than", "qid": "names a query beyond", "order": "ascend strictly", "csr": "row_offsets is not a CSR",
         "qend": "last residue of its frame", "tend": "target position"}
NAMED = {"offsets": "record", "long": "record", "qid": "hit row", "order": "hit row", "csr": "hit row", "qend": "region", "tend": "region"}


@pytest.mark.parametrize("kind,index,change", REFUSALS, ids=[f"{k}_{i}" for k, i, _ in REFUSALS])
def test_refusals_name_the_first_offender(ctx, kind, index, change):
    S = small_case()
    idle = ctx.pool_stats()["bytes_in_use"]
    hits = make_hits(ctx, S["qid"], S["tid"], S["isect"], S["nw"], 24, 8)
    qid, tid = S["qid"].copy(), S["tid"].copy()
    if "nt_off" in change:
        S["nt_off"] = np.array(change["nt_off"], np.uint64)
    if "swap" in change:
        a, b = change["swap"]
        qid[[a, b]], tid[[a, b]] = qid[[b, a]], tid[[b, a]]
    if "dup" in change:
        qid[change["dup"]], tid[change["dup"]] = qid[change["dup"] - 1], tid[change["dup"] - 1]
    if "swap" in change or "dup" in change:  # (no search returns such a list: the rows are uploaded into the list's columns)
        upload_into(ctx, hits.device_ptrs()[0], qid); upload_into(ctx, hits.device_ptrs()[1], tid)
        ctx.synchronize()
    for i, v in change.get("row_off", {}).items():
        S["row_off"][i] = v
    if "reg" in change:
        g, c, v = change["reg"]
        S["cols"][c][g] = v
    with pytest.raises(ffold_ref.FoldError) as ref:  # the reference refuses the same input for the same reason
        ffold_ref.fold(qid, tid, S["isect"], S["nw"], S["nt_off"], S["row_off"], S["cols"]["q_start"], S["cols"]["q_length"], S["cols"]["t_start"],
                       S["cols"]["t_length"])
    assert (ref.value.kind, ref.value.index) == (kind, index)
    before = ctx.pool_stats()["bytes_in_use"]
    with pytest.raises(ks.KmerseekError) as e:
        device_fold(ctx, hits, S["nt_off"], S["row_off"], S["cols"], "bare")
    assert e.value.status == INVALID and WORDS[kind] in str(e.value) and re.search(r"\b%s %d\b" % (NAMED[kind], index), str(e.value)), str(e.value)
    assert ctx.pool_stats()["bytes_in_use"] == before
    hits.free()
    # the context works afterwards
    S = small_case()
    hits = make_hits(ctx, S["qid"], S["tid"], S["isect"], S["nw"], 24, 8)
    fold = device_fold(ctx, hits, S["nt_off"], S["row_off"], S["cols"], "no_t_length")
    want_hits, want = ffold_ref.fold(S["qid"], S["tid"], S["isect"], S["nw"], S["nt_off"], S["row_off"], S["cols"]["q_start"], S["cols"]["q_length"],
                                     S["cols"]["t_start"], None, score=S["cols"]["score"])
    ffold_ref.assert_same(fold.hits.to_host(), fold.to_host(), want_hits, want, "after a refusal")
    fold.free(); hits.free()
    assert ctx.pool_stats()["bytes_in_use"] == idle


def pool_class(b):
    """the pool's size classes (ks_ctx.hip): multiples of 256 bytes up to 4 KiB, then quarter steps of the power of two below"""
    if b <= 4096:
        return (b + 255) & ~255
    step = 1 << ((b - 1).bit_length() - 3)
    return (b + step - 1) & ~(step - 1)


class DirtyPool:
    """Fills every idle pool block of the size of the fold's head flags and region counts (n_rows u32) with all ones.  A fold of
    ONE hit row with n_rows regions owns eight u32 columns of exactly that size; such folds are made and kept until one of them
    has to allocate all eight (and its score column) afresh, so that no idle block of the size is left; their columns are then
    overwritten with 0xff and they are freed."""

    def __init__(self, ctx, n_rows):
        self.ctx, self.R = ctx, n_rows
        R = n_rows
        self.one = make_hits(ctx, [0], [0], [1], [1], 6, 1)
        self.cols = dict(q_start=np.zeros(R, np.uint32), q_length=np.ones(R, np.uint32), t_start=np.zeros(R, np.uint32), t_length=np.ones(R, np.uint32),
                         score=np.ones(R, np.int64), identities=np.ones(R, np.uint32), aln_length=np.ones(R, np.uint32))
        assert pool_class(13364) == 14336 and pool_class(3341) == 3584 and pool_class(4097) == 5120
        self.fresh = 8 * pool_class(4 * R) + pool_class(8 * R)
        assert 6 * 256 + pool_class(R) < pool_class(4 * R)  # a holder's other blocks together are smaller than one such column

    def __call__(self):
        ctx, R, holders = self.ctx, self.R, []
        for _ in range(24):
            before = ctx.pool_stats()["bytes_held"]
            holders.append(device_fold(ctx, self.one, np.array([0, 30], np.uint64), np.array([0, R], np.uint64), self.cols, "full"))
            if ctx.pool_stats()["bytes_held"] - before >= self.fresh:
                break
        else:
            raise AssertionError("idle blocks of the scratch's size never ran out")
        ones = np.full(R, 0xFFFFFFFF, np.uint32)
        for h in holders:
            p = h.device_ptrs()
            for i in (2, 4, 5, 6, 7, 8, 10, 11):  # the u32 columns of n_regions entries
                upload_into(ctx, p[i], ones)
        ctx.synchronize()
        for h in holders:
            h.free()


def refused_on_dirty_scratch(ctx, dirty, hits, D, nt_off, qid, tid, variant):
    """the fold of the (bad) list on a dirtied pool is refused as the reference refuses it, row named -> the kind"""
    with pytest.raises(ffold_ref.FoldError) as ref:
        ffold_ref.check(qid.tolist(), tid.tolist(), nt_off.tolist(), D["row_off"].tolist(), D["q_start"].tolist(), D["q_length"].tolist(),
                        D["t_start"].tolist(), D["t_length"].tolist())
    assert ref.value.index > scan_tile()
    dirty()
    before = ctx.pool_stats()["bytes_in_use"]
    with pytest.raises(ks.KmerseekError) as e:
        device_fold(ctx, hits, nt_off, D["row_off"], D, variant)
    assert e.value.status == INVALID and re.search(r"\bhit row %d\b" % ref.value.index, str(e.value)), str(e.value)
    assert ctx.pool_stats()["bytes_in_use"] == before
    return ref.value.kind, ref.value.index


def test_refusals_beyond_a_scan_tile_on_dirty_scratch():
    """A refused row writes no head flag and no region count at a merged position, so the scans must not read what the pool
    blocks held before: every idle block of their size holds all ones when the refused calls run (DirtyPool).  The bad rows lie
    beyond the first scan tile of the four-tile synthetic list."""
    D = synthetic()
    n_rows, tile = len(D["qid"]), scan_tile()
    with ks.Context(0) as ctx:
        hits = make_hits(ctx, D["qid"], D["tid"], D["isect"], D["nw"], 6 * N_REC, N_T)
        dirty = DirtyPool(ctx, n_rows)
        # too few records: every row from the second tile on names a frame that does not exist, and writes nothing in tiles 1, 2, 3
        n_rec = int(D["qid"][tile + 300]) // 6
        assert n_rows > 3 * tile and int(D["qid"][tile]) // 6 < n_rec
        assert refused_on_dirty_scratch(ctx, dirty, hits, D, D["nt_off"][:n_rec + 1], D["qid"], D["tid"], "full")[0] == "qid"
        # two rows in each other's place, far behind the first tile
        at = tile + 400
        qid, tid = D["qid"].copy(), D["tid"].copy()
        qid[[at, at + 1]], tid[[at, at + 1]] = qid[[at + 1, at]], tid[[at + 1, at]]
        upload_into(ctx, hits.device_ptrs()[0], qid); upload_into(ctx, hits.device_ptrs()[1], tid)
        ctx.synchronize()
        assert refused_on_dirty_scratch(ctx, dirty, hits, D, D["nt_off"], qid, tid, "full") == ("order", at + 1)
        # the list as it was folds as before
        upload_into(ctx, hits.device_ptrs()[0], D["qid"]); upload_into(ctx, hits.device_ptrs()[1], D["tid"])
        ctx.synchronize()
        dirty()
        fold = device_fold(ctx, hits, D["nt_off"], D["row_off"], D, "full")
        ffold_ref.assert_same(fold.hits.to_host(), fold.to_host(), *D["want"]["full"], "after the refusals")
        fold.free(); hits.free(); dirty.one.free()


def test_refusal_where_stale_head_flags_would_overflow_the_look_back():
    """The size at which stale head flags can break the one-launch scan: its status word carries a running sum of 38 bits and a
    tile of u32 flags adds less than 2^32, so more than 2^38 / 2^32 = 64 tiles (131,072 rows) of unwritten flags are needed.
    300,000 rows without regions, three quarters of them naming frames of records that are not there: 109 tiles whose flags the
    plan does not write, over pool blocks that hold all ones.  The call must name the first such row."""
    n, tile = 300_000, scan_tile()
    i = np.arange(n, dtype=np.uint32)
    n_rec = n // 12
    z = np.zeros(0, np.uint32)
    D = dict(qid=i // 2, tid=i % 2, isect=np.ones(n, np.uint32), nw=np.ones(n, np.uint64), nt_off=30 * np.arange(n_rec + 1, dtype=np.uint64),
             row_off=np.zeros(n + 1, np.uint64), q_start=z, q_length=z, t_start=z, t_length=z)
    with ks.Context(0) as ctx:
        hits = make_hits(ctx, D["qid"], D["tid"], D["isect"], D["nw"], 6 * n_rec, 2)
        dirty = DirtyPool(ctx, n)
        # A sum that passes 2^38 runs into the LOWEST bit of the word's tile tag, which is ORed over it: the word is lost only where
        # that tag bit is 0, so the call runs with the scan's global tile numbers starting at an even and at an odd number.
        for base in (1 << 12, (1 << 12) + 1):
            ctx.debug_scan_seek(base)
            kind, first = refused_on_dirty_scratch(ctx, dirty, hits, D, D["nt_off"][:n_rec // 4 + 1], D["qid"], D["tid"], "bare")
            assert kind == "qid" and first == 12 * (n_rec // 4) and (n - first) // tile > 2 ** 38 // 2 ** 32
        dirty()
        fold = device_fold(ctx, hits, D["nt_off"], D["row_off"], D, "bare")  # the same list with all its records folds
        assert (fold.n_rows, fold.n_regions, fold.hits.count) == (n // 3, 0, n // 3)  # every strand has both targets in all three frames
        fq, ft, fi, _ = fold.hits.to_host()
        r = np.arange(n // 3, dtype=np.uint32)
        assert np.array_equal(fq, r // 2) and np.array_equal(ft, r % 2) and np.all(fi == 3)
        want_src = 2 * (3 * (r // 2)[:, None] + np.arange(3, dtype=np.uint32)[None, :]) + (r % 2)[:, None]  # row of (frame 3x + j, tid t): 2 (3x + j) + t
        assert np.array_equal(fold.to_host()[0].reshape(n // 3, 3), want_src)
        fold.free(); hits.free(); dirty.one.free()


def test_argument_refusals(ctx):
    L = ctx._L
    S = small_case()
    hits = make_hits(ctx, S["qid"], S["tid"], S["isect"], S["nw"], 24, 8)
    bufs = [ctx.to_device(a) for a in (S["nt_off"], S["row_off"], S["cols"]["q_start"], S["cols"]["q_length"], S["cols"]["t_start"])]
    p = [C.c_void_p(b.ptr) for b in bufs]
    oh, of = C.c_void_p(), C.c_void_p()

    def call(c=ctx._h, h=hits._h, off=p[0], ro=p[1], qs=p[2], opts=None, out_hits=C.byref(oh), out=C.byref(of), n=10):
        return L.ks_frames_fold_device(c, h, off, 4, ro, qs, p[3], p[4], None, None, None, None, n, opts, out_hits, out)
    three = C.c_uint32 * 3
    for opts in (_lib.ks_ffold_opts(1, three(0, 0, 0)), _lib.ks_ffold_opts(0, three(0, 0, 1)), _lib.ks_ffold_opts(0, three(1, 0, 0))):
        assert call(opts=C.byref(opts)) == INVALID and "frame fold options" in L.ks_last_error(ctx._h).decode()
        assert call(c=None, opts=C.byref(opts)) == INVALID  # the options are checked first, also without a context
        assert not oh.value and not of.value
    assert call(c=None) == INVALID
    for kw in (dict(h=None), dict(off=None), dict(ro=None), dict(qs=None), dict(out_hits=None), dict(out=None)):
        assert call(**kw) == INVALID and "NULL" in L.ks_last_error(ctx._h).decode(), kw
    assert call(n=2 ** 32) == CAPACITY
    with ks.Context(0) as other:
        assert L.ks_frames_fold_device(other._h, hits._h, p[0], 4, p[1], p[2], p[3], p[4], None, None, None, None, 10, None, C.byref(oh), C.byref(of)) == INVALID
        assert "another context" in L.ks_last_error(other._h).decode()
    ok = _lib.ks_ffold_opts(0, three(0, 0, 0))
    assert call(opts=C.byref(ok)) == _lib.KS_OK and oh.value and of.value
    L.ks_ffold_free(of); L.ks_hits_free(oh)
    # the object form takes a RegionScores or a RegionAlignments and nothing else (a scored object of another row count: the planted test)
    with pytest.raises(TypeError):
        ctx.fold_frames(hits, hits, S["nt_off"])
    for b in bufs:
        b.free()
    hits.free()


RUNGS = 6


def test_pool_refusals_leave_nothing_behind(monkeypatch):
    """The pool-cap walk of tests/test_gpu_error_paths.py over the fold's driver: a ladder of KS_DEBUG_POOL_CAP values between the
    pool's bytes_in_use before the call and its bytes_held after it, a fresh context per rung."""
    D = synthetic()
    want_hits, want = D["want"]["full"]

    class Run:
        def __init__(self):
            self.ctx = ks.Context(0, follow_debug_env=True)
            self.hits = make_hits(self.ctx, D["qid"], D["tid"], D["isect"], D["nw"], 6 * N_REC, N_T)
            names = ["nt_off", "row_off", "q_start", "q_length", "t_start", "t_length", "score", "identities", "aln_length"]
            self.bufs = [self.ctx.to_device(D[k]) for k in names]
            self.before = self.ctx.pool_stats()["bytes_in_use"]

        def go(self, **env):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            try:
                p = [b.ptr for b in self.bufs]
                fold = self.ctx.fold_frames_device(self.hits, p[0], N_REC, p[1], p[2], p[3], p[4], p[5], D["n"], d_score=p[6], d_identities=p[7],
                                                   d_aln_length=p[8])
                ffold_ref.assert_same(fold.hits.to_host(), fold.to_host(), want_hits, want, "pool walk")
                fold.free()
                return None
            except ks.KmerseekError as e:
                return e
            finally:
                for k in env:
                    monkeypatch.delenv(k)

        def close(self):
            self.ctx.close()

    first = Run()
    try:
        assert first.go() is None and first.ctx.pool_stats()["bytes_in_use"] == first.before
        lo, hi = max(first.before, 1), first.ctx.pool_stats()["bytes_held"]
    finally:
        first.close()
    assert hi > lo
    refused = []
    for cap in [lo + (hi - lo) * i // (RUNGS - 1) for i in range(RUNGS)]:
        run = Run()
        try:
            err = run.go(KS_DEBUG_POOL_CAP=str(cap))
            refused.append(err is not None)
            if err is not None:
                assert err.status == OOM and "pool cap" in str(err), (cap, str(err))
                assert run.ctx.pool_stats()["bytes_in_use"] == run.before, cap
                assert run.go() is None, cap
        finally:
            run.close()
    print(f"frame fold: bytes_in_use {lo}, bytes_held {hi}, refused rungs {refused}")
    assert any(refused) and not refused[-1], refused


# ---- planted genes, half of them with a frameshift, end to end -----------------------------------------------------------------------
N_CONTIGS = 24
# A chance match beside the frameshift lets an extension run a few residues into the other frame's part: the two members then
# overlap on the target.  An overhang of x residues needs a net-positive run of chance matches (1 in 20 each under +1 / -1), so
# 5 residues = 15 bases of allowed overlap is out of reach of a fixed 24-contig case (< 1e-5 per junction).
CHAIN_OPTS = {"max_overlap": 15}


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(4242)
    aa = b"ACDEFGHIKLMNPQRSTVWY"
    proteins = [bytes(aa[i] for i in rng.integers(0, 20, int(rng.integers(60, 121)))) for _ in range(20)]
    flank = lambda n: bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    contigs, truth = [], []
    for c in range(N_CONTIGS):
        t = c % 20
        prot = proteins[t]
        reverse, shifted = c % 2 == 1, (c // 2) % 2 == 1
        gene = translate_ref.reverse_translate(prot, rng)
        if shifted:
            m = int(rng.integers(20, len(prot) - 20 + 1))
            gene = gene[:3 * m] + flank(1) + gene[3 * m:]
        left, right = (10, 11, 12)[c % 3], (10, 11, 12)[(c // 3) % 3]
        contigs.append(flank(left) + (translate_ref.reverse_complement(gene) if reverse else gene) + flank(right))
        truth.append(dict(record=c, target=t, reverse=reverse, shifted=shifted, start=left, end=left + len(gene), length=len(prot)))
    assert {(t["reverse"], t["shifted"]) for t in truth} == {(a, b) for a in (False, True) for b in (False, True)}
    return proteins, contigs, truth


def check_planted_rows(rows, truth):
    by = {(r["query_name"], r["strand"], r["match_name"]): r for r in rows}
    for t in truth:
        r = by.get((f"contig{t['record']}", "-" if t["reverse"] else "+", f"prot{t['target']}"))
        assert r is not None, t
        frames = r["frames"].split(",")
        if t["shifted"]:
            assert r["n_alns"] == 2 and frames[0] != frames[1] and r["n_frameshifts"] == 1, (t, r)
        else:
            assert r["n_alns"] == 1 and r["n_frameshifts"] == 0, (t, r)
        assert all((f[0] == "-") == t["reverse"] for f in frames)
        assert t["start"] <= r["nt_start"] < r["nt_end"] <= t["end"], (t, r)
        assert r["nt_end"] - r["nt_start"] >= 3 * (t["length"] - 2 * K), (t, r)


def test_planted_frameshifts_end_to_end(ctx, tmp_path):
    proteins, contigs, truth = planted()
    nt, nt_off = ks.pack(contigs)
    t_res, t_off = ks.pack(proteins)
    n6, n_t = 6 * len(contigs), len(proteins)
    start = ctx.pool_stats()["bytes_in_use"]
    frames, foff, n_res = ctx.translate6(nt, nt_off)
    Q = ctx.sketch_batch_device(frames.ptr, foff.ptr, n6, n_res, K, 1, MOL)
    T = ctx.sketch_batch(t_res, t_off, K, 1, MOL)
    ix = ctx.index_build(T)
    hits = ctx.search(ix, Q)
    qp = ctx.kmer_positions_table_device(frames.ptr, foff.ptr, n6, n_res, K, 1, MOL)
    tp = ctx.kmer_positions_table(t_res, t_off, K, 1, MOL)
    mp = ctx.match_positions(qp, tp, hits)
    rg = ctx.match_regions(mp)
    d_t, d_to = ctx.to_device(t_res), ctx.to_device(t_off)
    sc = ctx.score_regions_device(rg, hits, frames.ptr, foff.ptr, n6, n_res, d_t.ptr, d_to.ptr, n_t, len(t_res), extend=True, x_drop=20)
    cu = ctx.cull_regions(sc)
    kept = cu.take(sc)
    before = ctx.pool_stats()["bytes_in_use"]
    fold = ctx.fold_frames(hits, kept, nt_off)
    chain = ctx.chain_frames(fold, **CHAIN_OPTS)
    # the device fold and chain against the references on the host copies of the same regions
    h, k = hits.to_host(), kept.to_host()  # RegionScores: row_offsets, q_start, t_start, length, score, identities, ...
    want_hits, want = ffold_ref.fold(h[0], h[1], h[2], h[3], nt_off, k[0], k[1], k[3], k[2], None, score=k[4], identities=k[5], aln_length=k[3])
    fold_host, chain_host = fold.to_host(), chain.to_host()
    ffold_ref.assert_same(fold.hits.to_host(), fold_host, want_hits, want, "planted")
    c = dict(zip(ffold_ref.NAMES, want))
    RH.assert_same(chain_host, rchain_ref.chain(c["row_offsets"], c["s_start"], c["nt_length"], c["t_start3"], c["t_length3"], c["score"],
                                                identities=c["identities"], aln_length=c["aln_length"], **CHAIN_OPTS), "planted chain")
    nt_recs = [(f"contig{i}", s) for i, s in enumerate(contigs)]
    t_recs = [(f"prot{i}", s) for i, s in enumerate(proteins)]
    rows = wire.frame_chain_rows(nt_recs, t_recs, fold.hits.to_host(), fold_host, chain_host)
    check_planted_rows(rows, truth)
    with pytest.raises(ks.KmerseekError) as e:  # regions of another hit list: the folded list has fewer rows than the frame hits
        ctx.fold_frames(fold.hits, kept, nt_off)
    assert e.value.status == INVALID and "another list" in str(e.value) and fold.n_rows < hits.count
    # composition: the best chain of every (record, strand) is the planted target's
    best = ctx.best_hits(fold.hits, k=1, score=chain.row_chain_score_ptr)
    bq, bt, _, _ = best.to_host()
    top = dict(zip(bq.tolist(), bt.tolist()))
    assert all(top.get(2 * t["record"] + int(t["reverse"])) == t["target"] for t in truth)
    assert best.count == len(set(want_hits[0].tolist()))
    best.free(); chain.free(); fold.free()
    assert ctx.pool_stats()["bytes_in_use"] == before  # fold, its hits and the chain are all the three calls held
    for o in (kept, cu, sc, d_t, d_to, rg, mp, qp, tp, hits, ix, Q, T, frames, foff):
        o.free()
    assert ctx.pool_stats()["bytes_in_use"] == start
    # the same through the wire, from the two FASTA files
    nt_fa, t_fa = tmp_path / "contigs.fa", tmp_path / "proteins.fa"
    nt_fa.write_bytes(b"".join(b">contig%d\n%s\n" % (i, s) for i, s in enumerate(contigs)))
    t_fa.write_bytes(b"".join(b">prot%d\n%s\n" % (i, s) for i, s in enumerate(proteins)))
    wired = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, ctx=ctx, chain_max_overlap=CHAIN_OPTS["max_overlap"])
    assert wired == rows
    assert ctx.pool_stats()["bytes_in_use"] == start  # every object it made is freed
    top1 = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, ctx=ctx, chain_max_overlap=CHAIN_OPTS["max_overlap"], top_k=1)
    check_planted_rows(top1, truth)
    per_strand = [(r["query_name"], r["strand"]) for r in top1]
    assert len(set(per_strand)) == len(per_strand) and set(per_strand) == {(r["query_name"], r["strand"]) for r in rows}  # one row each
    assert all(r in rows for r in top1)
    # ... and with gapped alignments in place of the extended regions (ks_raligns_fold_frames)
    gapped = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, ctx=ctx, gapped=True, chain_max_overlap=CHAIN_OPTS["max_overlap"])
    check_planted_rows(gapped, truth)
    assert ctx.pool_stats()["bytes_in_use"] == start
