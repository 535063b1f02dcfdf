"""CPU: the case tables of the primitive tests (tests/prims_cases.py) hold what their names claim, and the numpy references
(tests/prims_ref.py) agree with numpy's own sorts — so that tests/test_gpu_prims.py cannot pass on a vacuous input or against a
wrong reference.  The entries' refusals that need no context are here too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import prims_cases as PC  # noqa: E402
import prims_ref as PR  # noqa: E402


# ---------------------------------------------------------------------------------------------- scans
def test_scan_reference_is_a_running_sum():
    a = np.array([3, 0, 0xFFFFFFFF, 7, 0xFFFFFFFF], np.uint32)
    assert PR.scan_ref(a, 0).tolist() == [0, 3, 3, 3 + 0xFFFFFFFF, 10 + 0xFFFFFFFF, 10 + 2 * 0xFFFFFFFF]
    out, total = PR.scan_ref(a, 1)
    want = [0, 3, 3, (3 + 0xFFFFFFFF) % 2 ** 32, (10 + 0xFFFFFFFF) % 2 ** 32]
    assert out.tolist() == want and total == (10 + 2 * 0xFFFFFFFF) % 2 ** 32
    assert PR.scan_ref(np.zeros(0, np.uint32), 0).tolist() == [0]
    assert PR.scan_ref(np.zeros(0, np.uint32), 1)[1] == 0
    for n in (1, 2047, 5000):
        a = PC.scan_random(n, 0)
        py = [0]
        for v in a.tolist():
            py.append(py[-1] + v)
        assert PR.scan_ref(a, 0).tolist() == py


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_scan_inputs_stay_below_the_sum_bound(kind):
    """every scan input of the GPU tests is a valid one: u32 -> u64 sums below 2^38 (the status word's field), u32 -> u32 below 2^32"""
    bound = PC.scan_sum_bound(kind)
    for n in PC.SCAN_NS + (PC.SCAN_RECURSE_N, 10 * 2048 - 7, 5 * 2048 + 1):
        a = PC.scan_random(n, kind)
        assert len(a) == n and int(a.astype(np.uint64).sum()) < bound
        if n > 1:
            assert int(a.max()) > 0
    big = PC.scan_random(2 ** 20 + 3, kind)
    assert int(big.astype(np.uint64).sum()) > min(bound, 1 << 52) // 4  # ... and not by being tiny
    for name in PC.SCAN_PATTERNS:
        assert int(PC.scan_pattern(name).astype(np.uint64).sum()) < bound
    for name in PC.SCAN_SUM_CASES[kind]:
        assert int(PC.scan_sum_case(name).astype(np.uint64).sum()) < bound


def test_scan_sum_cases_hit_the_top_of_their_fields():
    for name in PC.SCAN_SUM_CASES[0]:
        a = PC.scan_sum_case(name).astype(np.uint64)
        assert int(a.sum()) == 2 ** 38 - 1 and PR.scan_tiles(len(a)) >= 2
    a = PC.scan_sum_case("sum38_tile0").astype(np.uint64)
    assert int(a[:PR.SCAN_TILE].sum()) == 2 ** 38 - 1 and len(a) == 2049  # tile 0 publishes all 38 bits set
    a = PC.scan_sum_case("sum38_split").astype(np.uint64)
    assert int(a[:PR.SCAN_TILE].sum()) == 2 ** 38 - 2 and int(a[PR.SCAN_TILE]) == 1
    a = PC.scan_sum_case("sum38_spread").astype(np.uint64)
    tiles = [int(a[t * PR.SCAN_TILE:(t + 1) * PR.SCAN_TILE].sum()) for t in range(PR.scan_tiles(len(a)))]
    assert len(tiles) == 5 and all(t > 0 for t in tiles) and np.cumsum(tiles)[1] >= 2 ** 36
    for name in PC.SCAN_SUM_CASES[1]:
        a = PC.scan_sum_case(name).astype(np.uint64)
        assert int(a.sum()) == 2 ** 32 - 1 and PR.scan_tiles(len(a)) >= 2
    # the wide scan's inputs do pass 2^38 (only that entry may be given them)
    assert int(PC.scan_sum_case("sum_all_max").astype(np.uint64).sum()) > 2 ** 44
    assert "sum_all_max" not in PC.SCAN_SUM_CASES[0] + PC.SCAN_SUM_CASES[1]
    assert int(PC.scan_random(4097, 2).astype(np.uint64).sum()) > 2 ** 38


def test_scan_patterns_sit_where_they_say():
    assert PC.SCAN_VALUES_N == 3 * 2048 + 5
    want = {0, PC.SCAN_VALUES_N - 1, 2047, 2048, 4095, 4096, 6143, 6144}
    assert set(PC.SCAN_SINGLES.values()) == want
    for name, at in PC.SCAN_SINGLES.items():
        a = PC.scan_pattern(name)
        assert np.flatnonzero(a).tolist() == [at] and a[at] == 0xFFFFFFFF
    assert not PC.scan_pattern("zeros").any() and (PC.scan_pattern("ones") == 1).all()


def test_ring_model_refuses_a_left_over_with_the_expected_tag():
    m = PR.RingModel()
    m.scan(0, 300)
    m.scan(2 ** 20 - 3, 10)          # slots 0 .. 6 again, other tags
    m.scan(2 ** 24 - 3 - 2 ** 20, 10)
    m.scan(2 ** 24 - 3, 10)
    with pytest.raises(AssertionError):
        m.scan(2 ** 32 - 3, 10)      # same slots, same 24-bit tags as the scan before: not a state counting reaches
    m.scan(2 ** 32 - 3 - 2 ** 20, 10)
    m.scan(2 ** 32 - 3, 10)          # ... with the lap before it in the ring, it is


# ---------------------------------------------------------------------------------------------- LSD sort
def test_lsd_reference_agrees_with_numpy_sorts():
    rng = np.random.default_rng(11)
    k = rng.integers(0, 1 << 63, 5000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000, dtype=np.uint64)
    v = np.arange(5000, dtype=np.uint32)
    gk, gv = PR.lsd_sort_ref(k, v, PC.LSD_SHIFT_LISTS["all8"])
    o = np.argsort(k, kind="stable")
    assert np.array_equal(gk, np.sort(k)) and np.array_equal(gk, k[o]) and np.array_equal(gv, v[o])
    # two digits: lexsort with the LAST listed shift as the primary key; ties in input order
    k[::3] = k[0]
    gk, gv = PR.lsd_sort_ref(k, v, [16, 40])
    o = np.lexsort((v, PR.lsd_digit(k, 16), PR.lsd_digit(k, 40)))
    assert np.array_equal(gk, k[o]) and np.array_equal(gv, v[o])
    gk, gv = PR.lsd_sort_ref(k, None, [0])
    assert gv is None and np.array_equal(gk, k[np.argsort(k & np.uint64(255), kind="stable")])


def test_lsd_prefix_digit_is_the_join_prefix():
    for scaled in (1, 5):
        mh = PC.max_hash(scaled)
        assert mh == cs.max_hash(scaled)
        K = cs.prefix_mul(16, mh)
        keys = PC.lsd_prefix_keys(scaled)
        for h in (0, 1, mh, 2 ** 64 - 1):
            assert (keys == np.uint64(h)).any()
        for s in (0, 8):
            d = PR.lsd_digit(keys, s, K)
            assert d.tolist() == [(cs.join_prefix(int(h), K) >> s) & 255 for h in keys.tolist()]
        pref = [cs.join_prefix(int(h), K) for h in keys.tolist()]
        assert min(pref) == 0 and max(p for p, h in zip(pref, keys.tolist()) if h <= mh) == 2 ** 16 - 1
        assert len(set(PR.lsd_digit(keys, 8, K).tolist())) == 256


def test_lsd_sizes_and_shift_lists():
    assert set(PC.LSD_NS) == {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 5}
    assert PC.LSD_SHIFT_LISTS["all8"] == list(range(0, 64, 8)) and len(PC.LSD_SHIFT_LISTS["s0_8_16"]) % 2 == 1
    assert PC.LSD_SHIFT_LISTS["s16_0_40"] != sorted(PC.LSD_SHIFT_LISTS["s16_0_40"])
    for sh in PC.LSD_SHIFT_LISTS.values():
        assert 1 <= len(sh) <= 8 and all(0 <= s <= 56 for s in sh)


@pytest.mark.parametrize("shifts", list(PC.LSD_FAMILY_SHIFTS.values()), ids=list(PC.LSD_FAMILY_SHIFTS))
def test_lsd_families_are_what_they_say(shifts):
    n = PC.LSD_FAMILY_N
    assert n % PR.RS_TILE != 0 and n > 2 * PR.RS_TILE
    fam = {name: PC.lsd_family(name, shifts) for name in PC.LSD_FAMILIES}
    for name, k in fam.items():
        assert k.dtype == np.uint64 and len(k) == n and not (k == np.uint64(PC.POISON_KEY)).any()
    for s in shifts:
        d = {name: PR.lsd_digit(k, s) for name, k in fam.items()}
        assert len(set(d["uniform"].tolist())) == 256
        assert set(d["two_digits"].tolist()) == {3, 200} and (d["two_digits"][::2] == 200).all() and (d["two_digits"][1::2] == 3).all()
        assert (d["digit_0"] == 0).all()
        # the padding edge: the last tile is partial and every key of it (of every tile, here) has digit 255
        last = d["digit_255_partial_tile"][n // PR.RS_TILE * PR.RS_TILE:]
        assert 0 < len(last) < PR.RS_TILE and (last == 255).all() and (d["digit_255_partial_tile"] == 255).all()
        assert (d["one_digit_but_3"] == 77).sum() == n - 3
        assert (d["differ_outside"] == 0x5A).all()
    assert len(set(fam["all_equal"].tolist())) == 1
    assert len(set(fam["digit_255_partial_tile"].tolist())) > n // 2 and len(set(fam["differ_outside"].tolist())) > n // 2
    assert (np.diff(fam["sorted"].astype(object)) >= 0).all() and (np.diff(fam["reverse_sorted"].astype(object)) <= 0).all()
    # keys that differ only outside the sorted bits: the reference leaves the input order
    gk, gv = PR.lsd_sort_ref(fam["differ_outside"], np.arange(n), shifts)
    assert np.array_equal(gv, np.arange(n))


@pytest.mark.parametrize("regions", PC.SEG_REGIONS)
@pytest.mark.parametrize("cap", PC.SEG_CAPS)
def test_segmented_builders(regions, cap):
    menu = PC.seg_fill_menu(cap)
    assert {0, 1, cap, cap - 1, PR.RS_TILE - 1} <= set(menu) and ((PR.RS_TILE + 1 in menu) == (cap > PR.RS_TILE))
    pats = PC.seg_fill_patterns(regions, cap)
    seen = set()
    for name, fills in pats.items():
        assert len(fills) == regions and all(0 <= f <= cap for f in fills)
        seen |= set(fills)
        keys, vals, lens, vk, vv = PC.seg_case(regions, cap, fills)
        assert len(keys) == len(vals) == regions * cap and lens.tolist() == list(fills)
        assert not (vk == np.uint64(PC.POISON_KEY)).any() and np.array_equal(vv, np.arange(len(vk)))
        at = 0
        for r, f in enumerate(fills):
            assert np.array_equal(keys[r * cap:r * cap + f], vk[at:at + f]) and np.array_equal(vals[r * cap:r * cap + f], vv[at:at + f])
            assert (keys[r * cap + f:(r + 1) * cap] == np.uint64(PC.POISON_KEY)).all()
            assert (vals[r * cap + f:(r + 1) * cap] == PC.POISON_VAL).all()
            at += f
        assert at == len(vk)
    if regions == 1:
        assert seen == set(menu)
    else:
        assert pats["one_record_in_last_region"] == [0] * (regions - 1) + [1]
        if regions >= len(menu):
            assert set(menu) <= set(pats["mixed_a"]) and set(menu) <= set(pats["mixed_b"])


# ---------------------------------------------------------------------------------------------- MSD sort
def test_msd_layout_table_matches_the_restated_layout():
    for n in PC.MSD_NS:
        for nbits, want in PC.MSD_BITS2.items():
            assert PR.msd_bits2(n, nbits) == want, (n, nbits)
    assert PC.MSD_BITS2 == {17: 1, 24: 8, 28: 4, 32: 8, 40: 8, 56: 8}
    assert PR.msd_bits2(PC.MSD_BIG_N, PC.MSD_BIG_NBITS) == PC.MSD_BIG_BITS2 == 9
    assert PR.msd_bits2(PC.MSD_BIG_N - 1, PC.MSD_BIG_NBITS) == 8 and PC.MSD_BIG_N == 561 << 16
    # "level 1 alone" (bits2 == 0) cannot happen for any key this sort takes: the second loop always finds a width of 1 .. 8 bits
    # that saves a local pass
    for nbits in range(17, 65):
        for n in (65536, 10 ** 5, 10 ** 6, 10 ** 7, PC.MSD_BIG_N, 2 ** 32 - 2):
            b2 = PR.msd_bits2(n, nbits)
            assert 1 <= b2 <= 9 and nbits - 8 - b2 >= 1
    for name, (n, nbits) in PC.MSD_NOT_APPLICABLE.items():
        assert not PR.msd_applies(n, nbits)
    assert PC.MSD_NOT_APPLICABLE == {"n_65535_nbits_40": (65535, 40), "n_70000_nbits_16": (70000, 16)}


def test_msd_check_catches_what_it_should():
    k = PC.msd_uniform(70000, 24, 12)
    good = k[np.argsort(PR.msd_field(k, 12, 24), kind="stable")]
    PR.msd_check(k, good, 12, 24)
    PR.msd_check(k, np.sort(k), 12, 24)       # any order among equal keys
    with pytest.raises(AssertionError):
        PR.msd_check(k, k, 12, 24)            # unsorted
    lost = good.copy()
    lost[100] = lost[101]
    with pytest.raises(AssertionError):
        PR.msd_check(k, lost, 12, 24)         # a record doubled over another
    pay = good.copy()
    pay[5] ^= np.uint64(1)
    with pytest.raises(AssertionError):
        PR.msd_check(k, pay, 12, 24)          # payload bits altered


@pytest.mark.parametrize("nbits,lo_bit", PC.MSD_COMBOS)
def test_msd_uniform_inputs(nbits, lo_bit):
    for n in PC.MSD_NS:
        k = PC.msd_uniform(n, nbits, lo_bit)
        assert len(k) == n and int(k.max()) < 1 << (nbits + lo_bit) and not (k == np.uint64(PC.POISON_KEY)).any()
        f = PR.msd_field(k, lo_bit, nbits)
        assert len(set((f >> np.uint64(nbits - 8)).tolist())) == 256
        if lo_bit:
            assert len(set((k & np.uint64((1 << lo_bit) - 1)).tolist())) > 1000
        assert PR.msd_info_ref(k, lo_bit, nbits)["big"] == 0


def test_msd_skews_are_what_they_say():
    n = 65536
    k = PC.msd_skew("tiny_level1_regions", 24, 0)
    d1 = np.bincount((PR.msd_field(k, 0, 24) >> np.uint64(16)).astype(np.int64), minlength=256)
    assert len(k) == n and (d1 > 0).all() and d1.max() <= PR.MS_TILE // 2  # a level-2 tile spans many level-1 regions
    assert len(set(PR.msd_field(k, 0, 24).tolist())) > n * 0.99
    k = PC.msd_skew("three_level1_digits", 24, 0)
    assert set((PR.msd_field(k, 0, 24) >> np.uint64(16)).tolist()) == {5, 6, 200}
    for nbits, lo_bit in ((24, 0), (32, 12), (40, 12)):
        b2 = PC.MSD_BITS2[nbits]
        bucket = lambda k: np.bincount((PR.msd_field(k, lo_bit, nbits) >> np.uint64(nbits - 8 - b2)).astype(np.int64))  # noqa: E731
        k = PC.msd_skew("all_equal", nbits, lo_bit)
        assert len(set(PR.msd_field(k, lo_bit, nbits).tolist())) == 1 and PR.msd_info_ref(k, lo_bit, nbits)["big"] == 1
        if lo_bit:
            assert len(set(k.tolist())) > 1000  # the payload differs: a lost or doubled record shows
        k = PC.msd_skew("one_key_5000", nbits, lo_bit)
        _, c = np.unique(PR.msd_field(k, lo_bit, nbits), return_counts=True)
        assert c.max() >= 5000 > PR.ML_CAP and PR.msd_info_ref(k, lo_bit, nbits)["big"] >= 1
        k = PC.msd_skew("one_bucket_6000", nbits, lo_bit)
        assert bucket(k).max() >= 6000 > PR.ML_CAP                      # more than ML_CAP records in one (d1, d2) bin
        _, c = np.unique(PR.msd_field(k, lo_bit, nbits), return_counts=True)
        assert c.max() < 64 and PR.msd_info_ref(k, lo_bit, nbits)["big"] >= 1  # ... that differ below it
    # the large-bucket kernel's passes over memory: an odd number (copy back) and an even one
    passes = {nbits: (nbits - 8 - PC.MSD_BITS2[nbits] + 7) // 8 for nbits in (24, 32, 40)}
    assert passes == {24: 1, 32: 2, 40: 3}


@pytest.mark.parametrize("name", list(PC.MSD_SEG_CASES))
def test_msd_segmented_builders(name):
    cap, fills = PC.MSD_SEG_CASES[name]
    keys, counts, seg_cap, valid = PC.msd_seg_case(name, 28, 12)
    assert counts == list(fills) and seg_cap == cap and len(keys) == len(fills) * cap
    assert len(fills) == {"segs_1": 1, "segs_5": 5, "segs_64": 64}[name] and sum(fills) >= 65536 and max(fills) <= cap
    if len(fills) > 1:
        assert {0, 1, 8192, 8193} <= set(fills)
    at = 0
    for s, f in enumerate(fills):
        assert np.array_equal(keys[s * cap:s * cap + f], valid[at:at + f])
        assert (keys[s * cap + f:(s + 1) * cap] == np.uint64(PC.POISON_KEY)).all()
        at += f
    assert at == len(valid) and not (valid == np.uint64(PC.POISON_KEY)).any()


# ---------------------------------------------------------------------------------------------- refusals without a context
def test_entries_refuse_a_null_context():
    from kmerseek_amd import _lib, build as ks_build
    ks_build.build()
    L = _lib.load()
    sh = (C.c_int * 1)(0)
    info = (C.c_uint32 * 4)()
    base = C.c_uint32(0)
    assert L.ks_debug_scan(None, 0, None, None, 0, None) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_debug_scan_seek(None, 0) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_debug_scan_ticket(None, C.byref(base)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_debug_radix_sort(None, 0, None, None, 0, sh, 1, 0, None, 0, 0, 0, None, None) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_debug_msd_sort(None, None, 0, 0, 24, None, 0, 0, C.byref(info)) == _lib.KS_ERR_INVALID_ARG
