"""GPU: the device-wide primitives called directly (ks_debug_scan / ks_debug_radix_sort / ks_debug_msd_sort) against the numpy
references of tests/prims_ref.py, on the named inputs of tests/prims_cases.py.  Integers and exact equality throughout.

- scans, u32 -> u64 (bounded and wide) and u32 -> u32, on the one-launch (look-back) path and with KS_DEBUG_SCAN_3PASS: sizes around the tile, the
  3-pass recursion, single nonzero values at the tile edges, sums at the very top of the status word's 38-bit field and of u32;
  the path taken is asserted through the ticket base.  The status ring across its end (2^20), the tag period (2^24) and the
  ticket's wrap (2^32), with real left-overs in the slots;
- the stable LSD sort with no, 4-byte and 8-byte values (the values are the input positions, so stability shows): sizes around the
  wave, the tile and several tiles, odd / even / non-monotone shift lists, the in-place form, key families (among them a partial
  tile of digit 255 only: the scatter ranks its padding as digit 255), join-prefix digits, the segmented first pass;
- the MSD match sort: the reported layout against the table, short lists with wide second levels (most records outliers of the
  level-2 window), skew into the large-bucket kernel's LDS and global-memory ends, segmented level 1, the 1024-bin window.

Every input is a valid one (tests/test_prims_ref_cpu.py holds the tables to that); refusals are host-side checks only."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import prims_cases as PC  # noqa: E402
import prims_ref as PR  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib  # noqa: E402

POISON64 = np.uint64(PC.POISON_KEY)
POISON32 = np.uint32(PC.POISON_VAL)
TAIL = 8  # poisoned entries behind every output: nothing may be written there
KNOBS = (None, "1")  # KS_DEBUG_SCAN_3PASS
KINDS, KIND_IDS = (0, 1, 2), ("u64", "u32", "u64wide")  # ks_debug_scan: u32 -> u64, u32 -> u32, u32 -> u64 without the bound on the sum
U32_MOD = 1 << 32


@pytest.fixture(scope="module")
def ctx():
    c = ks.Context(0, follow_debug_env=True)
    yield c
    c.close()


def _knob(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _padded(a, fill):
    return np.concatenate([a, np.full(TAIL, fill, a.dtype)])


# ================================================================================================ scans
def _scan(ctx, kind, a, lookback, with_total=True):
    """one scan through the entry, checked against the reference and for the path it took"""
    a = np.ascontiguousarray(a, np.uint32)
    n = len(a)
    d_in = ctx.to_device(a)
    before = ctx.debug_scan_ticket()
    if kind != 1:
        d_out = ctx.to_device(np.full(n + 1 + TAIL, POISON64, np.uint64))
        ctx.debug_scan(kind, d_in.ptr, d_out.ptr, n)
        got = d_out.to_host(np.uint64)
        assert np.array_equal(got[:n + 1], PR.scan_ref(a, kind)), f"u32 -> u64 scan of {n} values"
        assert (got[n + 1:] == POISON64).all()
    else:
        d_out = ctx.to_device(np.full(n + TAIL, POISON32, np.uint32))
        d_tot = ctx.to_device(np.array([POISON32], np.uint32)) if with_total else None
        ctx.debug_scan(1, d_in.ptr, d_out.ptr, n, d_tot.ptr if with_total else 0)
        got = d_out.to_host(np.uint32)
        want, total = PR.scan_ref(a, 1)
        assert np.array_equal(got[:n], want), f"u32 -> u32 scan of {n} values"
        assert (got[n:] == POISON32).all()
        if with_total:
            assert int(d_tot.to_host(np.uint32)[0]) == total
        assert np.array_equal(d_in.to_host(np.uint32), a)  # the input of the copy-then-scan form is only read
    tiles = PR.scan_tiles(n)
    advanced = (ctx.debug_scan_ticket() - before) % U32_MOD
    assert advanced == (tiles if lookback and kind != 2 and tiles >= 2 else 0), "the scan did not take the path this case is about"
    return tiles


@pytest.mark.parametrize("n", PC.SCAN_NS)
@pytest.mark.parametrize("knob", KNOBS, ids=("lookback", "3pass"))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_scan_sizes(ctx, monkeypatch, kind, knob, n):
    _knob(monkeypatch, "KS_DEBUG_SCAN_3PASS", knob)
    a = PC.scan_random(n, kind)
    _scan(ctx, kind, a, lookback=knob is None)
    if kind == 1:
        _scan(ctx, kind, a, lookback=knob is None, with_total=False)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_scan_3pass_recursion(ctx, monkeypatch, kind):
    """more block sums than one tile holds: the sums are scanned by the generic scan again"""
    monkeypatch.setenv("KS_DEBUG_SCAN_3PASS", "1")
    assert PR.scan_tiles(PC.SCAN_RECURSE_N) > PR.SCAN_TILE
    _scan(ctx, kind, PC.scan_random(PC.SCAN_RECURSE_N, kind), lookback=False)


@pytest.mark.parametrize("pattern", PC.SCAN_PATTERNS)
@pytest.mark.parametrize("knob", KNOBS, ids=("lookback", "3pass"))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_scan_values(ctx, monkeypatch, kind, knob, pattern):
    _knob(monkeypatch, "KS_DEBUG_SCAN_3PASS", knob)
    _scan(ctx, kind, PC.scan_pattern(pattern), lookback=knob is None)


@pytest.mark.parametrize("kind,case", [(k, c) for k in KINDS for c in PC.SCAN_SUM_CASES[k]])
@pytest.mark.parametrize("knob", KNOBS, ids=("lookback", "3pass"))
def test_scan_sums_at_the_top_of_the_field(ctx, monkeypatch, knob, kind, case):
    """u32 -> u64: 2^38 - 1, every bit of the status word's value field set, next to the tag it must not touch.
    u32 -> u32: 2^32 - 1.  The wide u32 -> u64 (never the look-back path): sums far beyond 2^38."""
    _knob(monkeypatch, "KS_DEBUG_SCAN_3PASS", knob)
    _scan(ctx, kind, PC.scan_sum_case(case), lookback=knob is None)


def test_scan_ring_end_tag_period_and_ticket_wrap(monkeypatch):
    """The look-back scan across the end of its ring (2^20 slots), the period of the tag (2^24) and the wrap of the ticket (2^32),
    each time with the words of earlier scans in the slots it uses.  ks_debug_scan_seek puts the counter there; before the two
    far seeks the same scans run one lap (2^20 tiles) earlier, which is what the counter would have left in those slots had it
    counted its way — the RingModel asserts that no scan here meets its own tag as a left-over, a state counting cannot reach."""
    monkeypatch.delenv("KS_DEBUG_SCAN_3PASS", raising=False)
    c = ks.Context(0, follow_debug_env=True)
    try:
        model = PR.RingModel()

        def scans(seed):
            base = c.debug_scan_ticket()
            a = PC.scan_random(10 * PR.SCAN_TILE - 7, 0, seed)     # 10 tiles of random data
            model.scan(base, 10)
            assert _scan(c, 0, a, lookback=True) == 10
            b = PC.scan_random(5 * PR.SCAN_TILE + 1, 1, seed)      # ... and one ordinary multi-tile scan behind it
            model.scan(base + 10, 6)
            assert _scan(c, 1, b, lookback=True) == 6

        # 1. a few hundred tiles from 0: the ring's low slots hold real words
        assert c.debug_scan_ticket() == 0
        for seed in range(3):
            a = PC.scan_random(100 * PR.SCAN_TILE + 3, seed % 2, seed)
            model.scan(c.debug_scan_ticket(), 101)
            _scan(c, seed % 2, a, lookback=True)
        assert c.debug_scan_ticket() == 303
        # 2. the ring's end, exactly as the counter reaches it first: nothing above slot 303 was ever written
        c.debug_scan_seek(2 ** 20 - 3)
        assert c.debug_scan_ticket() == 2 ** 20 - 3
        scans(10)
        assert c.debug_scan_ticket() == 2 ** 20 + 13
        # 3. the tag's period and 4. the ticket's wrap, each behind the lap before it
        for g, seed in ((2 ** 24 - 3, 20), (2 ** 32 - 3, 30)):
            c.debug_scan_seek(g - PR.SCAN_RING)
            scans(seed)
            c.debug_scan_seek(g)
            scans(seed + 1)
            assert c.debug_scan_ticket() == (g + 16) % U32_MOD
        assert c.debug_scan_ticket() == 13
    finally:
        c.close()


# ================================================================================================ LSD radix sort
VDTYPE = {0: None, 4: np.uint32, 8: np.uint64}


def _lsd(ctx, vbytes, keys, shifts, alias, pfx_k=0):
    keys = np.ascontiguousarray(keys, np.uint64)
    n = len(keys)
    vals = None if vbytes == 0 else np.arange(n, dtype=VDTYPE[vbytes])
    d_k = ctx.to_device(keys)
    d_ko = ctx.to_device(np.full(n + TAIL, POISON64, np.uint64))
    d_v = d_vo = None
    if vbytes:
        d_v = ctx.to_device(vals)
        d_vo = ctx.to_device(np.full(n + TAIL, PC.POISON_VAL, VDTYPE[vbytes]))
    ctx.debug_radix_sort(vbytes, d_k.ptr, d_v.ptr if vbytes else 0, n, shifts, d_ko.ptr, d_vo.ptr if vbytes else 0, pfx_k=pfx_k,
                         alias_in=alias)
    want_k, want_v = PR.lsd_sort_ref(keys, vals, shifts, pfx_k)
    got_k = d_ko.to_host(np.uint64)
    assert np.array_equal(got_k[:n], want_k), "keys"
    assert (got_k[n:] == POISON64).all()
    if vbytes:
        got_v = d_vo.to_host(VDTYPE[vbytes])
        assert np.array_equal(got_v[:n], want_v), "values: the sort is not stable, or moved a value away from its key"
        assert (got_v[n:] == PC.POISON_VAL).all()
        assert np.array_equal(d_v.to_host(VDTYPE[vbytes]), vals)
    assert np.array_equal(d_k.to_host(np.uint64), keys)  # the caller's input is only ever read


@pytest.mark.parametrize("n", PC.LSD_NS)
@pytest.mark.parametrize("alias", (0, 1), ids=("copy", "inplace"))
@pytest.mark.parametrize("vbytes", (0, 4, 8), ids=("keys", "v32", "v64"))
def test_lsd_sizes(ctx, vbytes, alias, n):
    _lsd(ctx, vbytes, PC.lsd_uniform(n), [0, 8], alias)
    _lsd(ctx, vbytes, PC.lsd_uniform(n, seed=1), [24], alias)


@pytest.mark.parametrize("shifts", list(PC.LSD_SHIFT_LISTS))
@pytest.mark.parametrize("alias", (0, 1), ids=("copy", "inplace"))
@pytest.mark.parametrize("vbytes", (0, 4, 8), ids=("keys", "v32", "v64"))
def test_lsd_shift_lists(ctx, vbytes, alias, shifts):
    _lsd(ctx, vbytes, PC.lsd_uniform(PC.LSD_FAMILY_N, seed=2), PC.LSD_SHIFT_LISTS[shifts], alias)
    _lsd(ctx, vbytes, PC.lsd_uniform(1025, seed=3), PC.LSD_SHIFT_LISTS[shifts], alias)


@pytest.mark.parametrize("family", PC.LSD_FAMILIES)
@pytest.mark.parametrize("shifts", list(PC.LSD_FAMILY_SHIFTS))
@pytest.mark.parametrize("alias", (0, 1), ids=("copy", "inplace"))
@pytest.mark.parametrize("vbytes", (0, 4, 8), ids=("keys", "v32", "v64"))
def test_lsd_key_families(ctx, vbytes, alias, shifts, family):
    sh = PC.LSD_FAMILY_SHIFTS[shifts]
    _lsd(ctx, vbytes, PC.lsd_family(family, sh), sh, alias)


@pytest.mark.parametrize("n", (1, 63, 1025, PR.RS_TILE - 1, PR.RS_TILE + 1))
@pytest.mark.parametrize("vbytes", (0, 4, 8), ids=("keys", "v32", "v64"))
def test_lsd_partial_tile_of_digit_255_only(ctx, vbytes, n):
    """a partial tile whose real keys all have the digit the padding is ranked under, at other fills than the family's"""
    for sh in ([8], [0, 8, 16]):
        _lsd(ctx, vbytes, PC.lsd_family("digit_255_partial_tile", sh, n=n), sh, 0)


@pytest.mark.parametrize("scaled", (1, 5))
@pytest.mark.parametrize("alias", (0, 1), ids=("copy", "inplace"))
def test_lsd_join_prefix_digits(ctx, scaled, alias):
    K = cs.prefix_mul(16, cs.max_hash(scaled))
    keys = PC.lsd_prefix_keys(scaled)
    _lsd(ctx, 4, keys, [0, 8], alias, pfx_k=K)
    _lsd(ctx, 4, keys, [8], alias, pfx_k=K)


def _seg_cases():
    out = []
    for regions in PC.SEG_REGIONS:
        for cap in PC.SEG_CAPS:
            for name in PC.seg_fill_patterns(regions, cap):
                out.append(pytest.param(regions, cap, name, id=f"r{regions}-cap{cap}-{name}"))
    return out


@pytest.mark.parametrize("regions,cap,pattern", _seg_cases())
def test_lsd_segmented_first_pass(ctx, regions, cap, pattern):
    fills = PC.seg_fill_patterns(regions, cap)[pattern]
    keys, vals, lens, vk, vv = PC.seg_case(regions, cap, fills)
    n = len(vk)
    d_k, d_v, d_len = ctx.to_device(keys), ctx.to_device(vals), ctx.to_device(lens)
    for shifts in ([0, 8], [8], [0, 8, 16]):
        d_ko = ctx.to_device(np.full(n + TAIL, POISON64, np.uint64))
        d_vo = ctx.to_device(np.full(n + TAIL, POISON32, np.uint32))
        ctx.debug_radix_sort(4, d_k.ptr, d_v.ptr, n, shifts, d_ko.ptr, d_vo.ptr, d_seg_len=d_len.ptr, seg_cap=cap, seg_regions=regions)
        want_k, want_v = PR.lsd_sort_ref(vk, vv, shifts)
        got_k, got_v = d_ko.to_host(np.uint64), d_vo.to_host(np.uint32)
        assert not (got_k[:n] == POISON64).any() and not (got_v[:n] == POISON32).any(), "slack of a region among the records"
        assert np.array_equal(got_k[:n], want_k) and np.array_equal(got_v[:n], want_v)
        assert (got_k[n:] == POISON64).all() and (got_v[n:] == POISON32).all()
    assert np.array_equal(d_k.to_host(np.uint64), keys) and np.array_equal(d_v.to_host(np.uint32), vals)


# ================================================================================================ MSD match sort
def _msd(ctx, keys, lo_bit, nbits, lds_cap=PR.ML_CAP, seg=None, what=""):
    """seg = (counts, seg_cap, valid records): keys is then the segmented buffer"""
    keys = np.ascontiguousarray(keys, np.uint64)
    valid = keys if seg is None else seg[2]
    n = len(valid)
    d = ctx.to_device(_padded(keys, POISON64))
    if seg is None:
        info = ctx.debug_msd_sort(d.ptr, n, lo_bit, nbits)
    else:
        info = ctx.debug_msd_sort(d.ptr, n, lo_bit, nbits, seg_count=seg[0], seg_cap=seg[1])
    print(f"msd {what}: n={n} lo_bit={lo_bit} nbits={nbits} -> bits2={info['bits2']} n_buckets={info['n_buckets']} big={info['big']}")
    got = d.to_host(np.uint64)
    want = PR.msd_info_ref(valid, lo_bit, nbits, lds_cap)
    assert info == want, f"reported {info}, the layout restated gives {want}"
    assert (got[len(keys):] == POISON64).all()
    if not info["done"]:
        assert np.array_equal(got[:len(keys)], keys), "not applicable, but the list was touched"
    else:
        assert not (got[:n] == POISON64).any(), "slack of a segment among the records"
        PR.msd_check(valid, got[:n], lo_bit, nbits)
    return info


@pytest.mark.parametrize("case", list(PC.MSD_NOT_APPLICABLE))
def test_msd_not_applicable(ctx, case):
    n, nbits = PC.MSD_NOT_APPLICABLE[case]
    for lo_bit in PC.MSD_LO_BITS:
        info = _msd(ctx, PC.msd_uniform(n, nbits, lo_bit), lo_bit, nbits, what=case)
        assert info == {"done": 0, "bits2": 0, "n_buckets": 0, "big": 0}


@pytest.mark.parametrize("n", PC.MSD_NS)
@pytest.mark.parametrize("nbits,lo_bit", PC.MSD_COMBOS)
def test_msd_uniform(ctx, nbits, lo_bit, n):
    info = _msd(ctx, PC.msd_uniform(n, nbits, lo_bit), lo_bit, nbits, what="uniform")
    assert info["done"] == 1 and info["bits2"] == PC.MSD_BITS2[nbits] and info["n_buckets"] == 256 << PC.MSD_BITS2[nbits]
    assert info["big"] == 0


@pytest.mark.parametrize("skew", ("tiny_level1_regions", "three_level1_digits"))
def test_msd_outlier_regime(ctx, skew):
    """65,536 records over 65,536 buckets: a level-2 tile spans ~32 level-1 regions, its window covers two — most records leave
    through the outlier path.  The same with three level-1 regions: most records inside the window."""
    for lo_bit in PC.MSD_LO_BITS:
        info = _msd(ctx, PC.msd_skew(skew, 24, lo_bit), lo_bit, 24, what=skew)
        assert info["bits2"] == 8 and info["n_buckets"] == 65536


@pytest.mark.parametrize("lds_cap", (None, "64"), ids=("lds4096", "lds64"))
@pytest.mark.parametrize("nbits,lo_bit", ((24, 0), (32, 12), (40, 12)), ids=("1pass", "2passes", "3passes"))
@pytest.mark.parametrize("skew", ("all_equal", "one_key_5000", "one_bucket_6000"))
def test_msd_skew_into_the_large_bucket_kernel(ctx, monkeypatch, skew, nbits, lo_bit, lds_cap):
    """buckets beyond what one wave / LDS sorts: k_msd_local_big's in-LDS end and its serial passes over memory, with an odd
    number of passes (the bucket ends in the scratch list and is copied back) and an even one"""
    _knob(monkeypatch, "KS_DEBUG_MSD_LDS_CAP", lds_cap)
    info = _msd(ctx, PC.msd_skew(skew, nbits, lo_bit), lo_bit, nbits, lds_cap=int(lds_cap or PR.ML_CAP), what=skew)
    assert info["bits2"] == PC.MSD_BITS2[nbits] and info["big"] >= 1


@pytest.mark.parametrize("lds_cap", (None, "64"), ids=("lds4096", "lds64"))
def test_msd_medium_buckets_take_the_lds_end(ctx, monkeypatch, lds_cap):
    """buckets of 1025 .. 4096 records: listed for the large-bucket kernel, sorted inside LDS there (unset knob)"""
    _knob(monkeypatch, "KS_DEBUG_MSD_LDS_CAP", lds_cap)
    k = PC.msd_uniform(3 * 65536 + 11, 17, 12)  # 512 buckets of ~384 ... and one of them 3000 records heavier
    f = PR.msd_field(k, 12, 17)
    k[:3000] = (k[:3000] & np.uint64(0xFFF)) | (((f[:3000] & np.uint64(0xFF)) | np.uint64(0x1AB00)) << np.uint64(12))
    info = _msd(ctx, k, 12, 17, lds_cap=int(lds_cap or PR.ML_CAP), what="medium bucket")
    assert info["big"] >= 1


@pytest.mark.parametrize("case", list(PC.MSD_SEG_CASES))
@pytest.mark.parametrize("nbits,lo_bit", ((28, 12), (40, 0)))
def test_msd_segmented_level1(ctx, case, nbits, lo_bit):
    keys, counts, cap, valid = PC.msd_seg_case(case, nbits, lo_bit)
    info = _msd(ctx, keys, lo_bit, nbits, seg=(counts, cap, valid), what=case)
    assert info["done"] == 1


@pytest.mark.parametrize("skew", (False, True), ids=("uniform", "half_in_one_level1_digit"))
def test_msd_1024_bin_window(ctx, skew):
    """the shortest list whose second level is 9 bits wide (131,072 buckets through the 1024-bin window); generated, sorted and
    checked on the device"""
    import torch
    dev = torch.device("cuda", 0)
    n, nbits, lo_bit = PC.MSD_BIG_N, PC.MSD_BIG_NBITS, 12
    t0 = time.perf_counter()
    g = torch.Generator(device=dev)
    g.manual_seed(20260 + int(skew))
    k = torch.randint(0, 1 << (nbits + lo_bit), (n,), dtype=torch.int64, device=dev, generator=g)  # (below 2^63: int64 orders as u64)
    if skew:
        k[:n // 2] = (k[:n // 2] & ((1 << (nbits + lo_bit - 8)) - 1)) | (0x5B << (nbits + lo_bit - 8))
        k = k[torch.randperm(n, device=dev, generator=g)]
    want = torch.sort(k).values
    bucket = (k >> (lo_bit + nbits - 8 - PC.MSD_BIG_BITS2)) & ((1 << (8 + PC.MSD_BIG_BITS2)) - 1)
    want_big = int((torch.bincount(bucket, minlength=1 << (8 + PC.MSD_BIG_BITS2)) > PR.ML_WCAP).sum())
    del bucket
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    info = ctx.debug_msd_sort(k.data_ptr(), n, lo_bit, nbits)
    t2 = time.perf_counter()
    print(f"msd 1024-bin window ({'skewed' if skew else 'uniform'}): n={n} nbits={nbits} -> bits2={info['bits2']} "
          f"n_buckets={info['n_buckets']} big={info['big']}")
    assert info == {"done": 1, "bits2": PC.MSD_BIG_BITS2, "n_buckets": 131072, "big": want_big}
    assert (want_big > 0) == skew
    f = k >> lo_bit
    assert bool((f[1:] >= f[:-1]).all()), "key field descends"
    del f
    assert torch.equal(torch.sort(k).values, want), "not a permutation of the input"
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"  generate {t1 - t0:.2f} s, sort {(t2 - t1) * 1e3:.2f} ms, check {t3 - t2:.2f} s, all {t3 - t0:.2f} s")


# ================================================================================================ refusals (host-side checks only)
def test_entries_refuse_bad_arguments_before_any_launch(ctx):
    a = ctx.to_device(np.arange(64, dtype=np.uint64))
    b = ctx.to_device(np.zeros(80, np.uint64))
    before = ctx.debug_scan_ticket()

    def refused(f, *args, **kw):
        with pytest.raises(ks.KmerseekError) as e:
            f(*args, **kw)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG

    too_many = 2 ** 32 - 1
    # scans
    refused(ctx.debug_scan, 0, 0, b.ptr, 8)
    refused(ctx.debug_scan, 0, a.ptr, 0, 8)
    refused(ctx.debug_scan, 3, a.ptr, b.ptr, 8)
    refused(ctx.debug_scan, -1, a.ptr, b.ptr, 8)
    refused(ctx.debug_scan, 1, a.ptr, b.ptr, too_many)
    # LSD sort
    rs = ctx.debug_radix_sort
    refused(rs, 0, 0, 0, 8, [0], b.ptr, 0)
    refused(rs, 0, a.ptr, 0, 8, [0], 0, 0)
    refused(rs, 4, a.ptr, 0, 8, [0], b.ptr, b.ptr)
    refused(rs, 4, a.ptr, a.ptr, 8, [0], b.ptr, 0)
    refused(rs, 3, a.ptr, a.ptr, 8, [0], b.ptr, b.ptr)
    refused(rs, 0, a.ptr, 0, too_many, [0], b.ptr, 0)
    refused(rs, 0, a.ptr, 0, 8, [], b.ptr, 0)
    refused(rs, 0, a.ptr, 0, 8, [0] * 9, b.ptr, 0)
    refused(rs, 0, a.ptr, 0, 8, [57], b.ptr, 0)
    refused(rs, 0, a.ptr, 0, 8, [0, -1], b.ptr, 0)
    refused(rs, 8, a.ptr, a.ptr, 8, [0], b.ptr, b.ptr, pfx_k=12345)
    refused(rs, 0, a.ptr, 0, 8, [0], b.ptr, 0, d_seg_len=a.ptr, seg_cap=8, seg_regions=1)
    refused(rs, 4, a.ptr, a.ptr, 8, [0], b.ptr, b.ptr, d_seg_len=a.ptr, seg_cap=0, seg_regions=1)
    # MSD sort
    ms = ctx.debug_msd_sort
    refused(ms, 0, 8, 0, 24)
    refused(ms, a.ptr, too_many, 0, 24)
    refused(ms, a.ptr, 8, -1, 24)
    refused(ms, a.ptr, 8, 0, 0)
    refused(ms, a.ptr, 8, 12, 53)
    refused(ms, a.ptr, 8, 0, 65)
    refused(ms, a.ptr, 8, 0, 24, seg_count=[0] * 65, seg_cap=8)
    refused(ms, a.ptr, 8, 0, 24, seg_count=[], seg_cap=8)
    refused(ms, a.ptr, 8, 0, 24, seg_count=[8], seg_cap=0)
    refused(ms, a.ptr, 8, 0, 24, seg_count=[9], seg_cap=8)      # a segment beyond its capacity
    refused(ms, a.ptr, 8, 0, 24, seg_count=[4, 3], seg_cap=8)   # the segments do not hold n records
    # nothing ran, nothing broke: the arrays are as they were and the context still sorts
    assert ctx.debug_scan_ticket() == before
    assert np.array_equal(a.to_host(np.uint64), np.arange(64, dtype=np.uint64)) and not b.to_host(np.uint64).any()
    _lsd(ctx, 4, PC.lsd_uniform(1025), [0, 8], 0)
