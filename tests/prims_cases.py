"""Named inputs of the primitive tests, as builders with fixed seeds: tests/test_prims_ref_cpu.py holds every one of them to what
its name claims (so that no GPU test passes on a vacuous input), tests/test_gpu_prims.py feeds them to the kernels.
Imports nothing of the library."""
import numpy as np

from prims_ref import ML_CAP, MS_TILE, RS_TILE, SCAN_TILE, SCAN_VAL_BITS, U32

U64_MAX = (1 << 64) - 1
POISON_KEY = 0xDEADBEEFDEADBEEF  # fills the slack of segmented inputs; no builder below emits it as a record
POISON_VAL = 0xDEADBEEF


def _rng(*seed):
    return np.random.default_rng([0x5eed] + [int(s) for s in seed])


def _u64(rng, n, hi=None):
    """n uniform u64 values below hi (default: all 64 bits), never the poison"""
    if hi is None:
        a = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    else:
        a = rng.integers(0, hi, n, dtype=np.uint64)
    a[a == np.uint64(POISON_KEY)] = np.uint64(12345)
    return a


# ------------------------------------------------------------------------------------------------ scans
SCAN_NS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 5, 2 ** 20 + 3)
SCAN_RECURSE_N = 2048 * 2048 + 1  # 3-pass: more block sums than one tile, they are scanned by scan_generic again


def scan_sum_bound(kind):
    """what the sum of a valid input stays below: the status word's value field (u32 -> u64), the output type (u32 -> u32 and the
    wide u32 -> u64, kind 2)"""
    return {0: 1 << SCAN_VAL_BITS, 1: 1 << 32, 2: 1 << 64}[kind]


def scan_random(n, kind, seed=0):
    """n random u32 values, as large as the sum bound of the kind allows"""
    top = min(U32, (scan_sum_bound(kind) - 1) // max(n, 1))
    return _rng(1, n, kind, seed).integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)


SCAN_VALUES_N = 3 * SCAN_TILE + 5
# name -> index of the single nonzero value (0xffffffff) among SCAN_VALUES_N zeros: index 0, the last one, either side of every
# tile boundary
SCAN_SINGLES = {"at_0": 0, "at_last": SCAN_VALUES_N - 1}
for _t in (1, 2, 3):
    SCAN_SINGLES[f"before_tile_{_t}"] = _t * SCAN_TILE - 1
    SCAN_SINGLES[f"first_of_tile_{_t}"] = _t * SCAN_TILE
SCAN_PATTERNS = ("zeros", "ones") + tuple(SCAN_SINGLES)


def scan_pattern(name):
    if name == "zeros":
        return np.zeros(SCAN_VALUES_N, np.uint32)
    if name == "ones":
        return np.ones(SCAN_VALUES_N, np.uint32)
    a = np.zeros(SCAN_VALUES_N, np.uint32)
    a[SCAN_SINGLES[name]] = U32
    return a


SCAN_SUM_CASES = {0: ("sum38_tile0", "sum38_split", "sum38_spread"), 1: ("sum32_three_tiles", "sum32_tile0"),
                  2: ("sum38_tile0", "sum_all_max")}


def scan_sum_case(name):
    """u32 -> u64: sums of exactly 2^38 - 1 = 64 * (2^32 - 1) + 63.  u32 -> u32: sums of exactly 2^32 - 1."""
    if name.startswith("sum38"):
        a = np.zeros(SCAN_TILE + 1, np.uint32)
        # 64 values of 2^32 - 1 and one of 63, in every wave of tile 0
        a[np.arange(64) * 32 + 5] = U32
        a[777] = 63
        if name == "sum38_tile0":      # tile 0 publishes a value with all 38 bits set; tile 1 adds nothing to it
            return a
        if name == "sum38_split":      # ... 2^38 - 2, and tile 1's own 1 completes it
            a[777] = 62
            a[SCAN_TILE] = 1
            return a
        if name == "sum38_spread":     # the same total over five tiles: every tile's inclusive prefix has high bits set
            b = np.zeros(4 * SCAN_TILE + 9, np.uint32)
            b[np.arange(64) * 128 + 3] = U32
            b[4 * SCAN_TILE + 8] = 63
            return b
    if name == "sum_all_max":          # the wide scan only: far beyond the 38 bits of a status word
        return np.full(SCAN_VALUES_N, U32, np.uint32)
    if name == "sum32_three_tiles":
        a = np.zeros(2 * SCAN_TILE + 1, np.uint32)
        a[5], a[SCAN_TILE], a[2 * SCAN_TILE] = 0x7FFFFFFF, 0x40000000, 0x40000000
        return a
    if name == "sum32_tile0":
        a = np.zeros(SCAN_TILE + 1, np.uint32)
        a[SCAN_TILE - 1] = U32
        return a
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ LSD radix sort
LSD_NS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 5)
LSD_SHIFT_LISTS = {"s0": [0], "s56": [56], "s0_8": [0, 8], "s0_8_16": [0, 8, 16], "all8": [0, 8, 16, 24, 32, 40, 48, 56],
                   "s16_0_40": [16, 0, 40]}
LSD_FAMILIES = ("uniform", "all_equal", "two_digits", "digit_0", "digit_255_partial_tile", "sorted", "reverse_sorted",
                "one_digit_but_3", "differ_outside")
LSD_FAMILY_N = 2 * RS_TILE + 37       # two full tiles and a partial one
LSD_FAMILY_SHIFTS = {"one": [8], "three": [0, 8, 16]}


def _set_digits(keys, shifts, digit):
    """the digit at every listed shift := digit (array or scalar)"""
    d = np.broadcast_to(np.asarray(digit, np.uint64), keys.shape)
    for s in shifts:
        keys &= ~(np.uint64(255) << np.uint64(s))
        keys |= d << np.uint64(s)
    return keys


def lsd_uniform(n, seed=0):
    return _u64(_rng(2, n, seed), n)


def lsd_family(name, shifts, n=LSD_FAMILY_N):
    """keys of a family; the families that speak of a digit mean the digit at EVERY shift of the list"""
    rng = _rng(3, LSD_FAMILIES.index(name), len(shifts))
    k = _u64(rng, n)
    if name == "uniform":
        return k
    if name == "all_equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if name == "two_digits":
        return _set_digits(k, shifts, np.where(np.arange(n) % 2 == 0, 200, 3))
    if name == "digit_0":
        return _set_digits(k, shifts, 0)
    if name == "digit_255_partial_tile":
        return _set_digits(k, shifts, 255)
    if name == "sorted":
        return np.sort(k)
    if name == "reverse_sorted":
        return np.sort(k)[::-1].copy()
    if name == "one_digit_but_3":
        d = np.full(n, 77, np.uint64)
        d[[1, n // 2, n - 1]] = (0, 78, 255)
        return _set_digits(k, shifts, d)
    if name == "differ_outside":
        return _set_digits(k, shifts, 0x5A)
    raise KeyError(name)


def max_hash(scaled):
    if scaled == 1:
        return U64_MAX
    v = 18446744073709551616.0 / float(scaled)
    return U64_MAX if v >= 18446744073709551616.0 else int(v)


def lsd_prefix_keys(scaled, n=RS_TILE + 1500):
    """hashes as a join on a prefix sees them: uniform below max_hash, with the edges 0, 1, max_hash and 2^64 - 1 among them"""
    mh = max_hash(scaled)
    k = _u64(_rng(4, scaled), n, hi=mh)
    edges = np.array([0, 1, mh, U64_MAX, mh - 1, 1 << 32, (1 << 32) - 1], np.uint64)
    k[np.linspace(0, n - 1, len(edges)).astype(int)] = edges
    return k


# segmented first pass: region r lies at r * cap, fill[r] records valid, poison behind them
SEG_REGIONS = (1, 3, 256)
SEG_CAPS = (RS_TILE, 2 * RS_TILE)


def seg_fill_menu(cap):
    return [0, 1, cap, cap - 1, RS_TILE - 1] + ([RS_TILE + 1] if cap > RS_TILE else [])


def seg_fill_patterns(regions, cap):
    """name -> fill per region"""
    menu = seg_fill_menu(cap)
    if regions == 1:
        return {f"fill_{f}": [f] for f in menu}
    return {"mixed_a": [menu[r % len(menu)] for r in range(regions)],        # 0, 1, cap, ...
            "mixed_b": [menu[(r + 3) % len(menu)] for r in range(regions)],  # cap - 1, tile - 1, (tile + 1,) 0, ...
            "one_record_in_last_region": [0] * (regions - 1) + [1]}


def seg_case(regions, cap, fills, seed=0):
    """-> (keys[regions * cap], vals[regions * cap] u32, len[regions] u32, valid keys concatenated, their values = 0 .. n - 1)"""
    fills = np.asarray(fills, np.uint32)
    n = int(fills.sum())
    rng = _rng(5, regions, cap, seed)
    vk = _u64(rng, n)
    vv = np.arange(n, dtype=np.uint32)
    keys = np.full(regions * cap, POISON_KEY, np.uint64)
    vals = np.full(regions * cap, POISON_VAL, np.uint32)
    at = 0
    for r, f in enumerate(fills.tolist()):
        keys[r * cap:r * cap + f] = vk[at:at + f]
        vals[r * cap:r * cap + f] = vv[at:at + f]
        at += f
    return keys, vals, fills, vk, vv


# ------------------------------------------------------------------------------------------------ MSD match sort
MSD_NS = (65536, 65537, 8 * 8192 + 5)
# nbits -> bits of the second partition level for the three lengths above, by hand from ms_layout_of: no length reaches 768
# records per level-1 bin, so level 2 is exactly as wide as it takes to leave a multiple of 8 bits to the local sort
MSD_BITS2 = {17: 1, 24: 8, 28: 4, 32: 8, 40: 8, 56: 8}
MSD_LO_BITS = (0, 12)
MSD_COMBOS = [(nbits, lo) for nbits in MSD_BITS2 for lo in MSD_LO_BITS if nbits + lo <= 64]  # (56 key bits: no room for 12 more)
MSD_BIG_N = 36765696  # the shortest list with a 9-bit second level: n >> 16 = 561 > 560
MSD_BIG_NBITS, MSD_BIG_BITS2 = 40, 9
MSD_NOT_APPLICABLE = {"n_65535_nbits_40": (65535, 40), "n_70000_nbits_16": (70000, 16)}


def _msd_pack(field, lo_bit, rng):
    """key field -> records: the field at lo_bit, random payload under it"""
    k = field.astype(np.uint64) << np.uint64(lo_bit)
    if lo_bit:
        k |= rng.integers(0, 1 << lo_bit, len(field), dtype=np.uint64)
    return k


def msd_uniform(n, nbits, lo_bit, seed=0):
    rng = _rng(6, n, nbits, lo_bit, seed)
    return _msd_pack(rng.integers(0, 1 << nbits, n, dtype=np.uint64), lo_bit, rng)


MSD_SKEWS = ("tiny_level1_regions", "three_level1_digits", "all_equal", "one_key_5000", "one_bucket_6000")


def msd_skew(name, nbits, lo_bit, n=65536):
    rng = _rng(7, MSD_SKEWS.index(name), nbits, lo_bit)
    f = rng.integers(0, 1 << nbits, n, dtype=np.uint64)
    top = np.uint64(nbits - 8)
    low = (np.uint64(1) << top) - np.uint64(1)
    if name == "tiny_level1_regions":        # uniform over every value of the field
        pass
    elif name == "three_level1_digits":      # every record in 3 of the 256 level-1 digits
        f = (f & low) | (np.array([5, 6, 200], np.uint64)[rng.integers(0, 3, n)] << top)
    elif name == "all_equal":
        f[:] = (0xA5A5A5A5A5A5A5A5 >> (64 - nbits))
    elif name == "one_key_5000":             # one key holds more records than a bucket sorted inside LDS may
        f[rng.choice(n, 5000, replace=False)] = f[0]
    elif name == "one_bucket_6000":          # ... one (d1, d2) bin does, with keys that differ below it: the passes over memory
        b2 = MSD_BITS2[nbits]
        rem = np.uint64(nbits - 8 - b2)
        at = rng.choice(n, 6000, replace=False)
        f[at] = (f[at] & ((np.uint64(1) << rem) - np.uint64(1))) | ((f[0] >> rem) << rem)
    else:
        raise KeyError(name)
    return _msd_pack(f, lo_bit, rng)


# segmented level 1: name -> (seg_cap, fill per segment); every list has at least 65,536 records
MSD_SEG_CASES = {
    "segs_1": (9 * MS_TILE - 3, [8 * MS_TILE + 5]),
    "segs_5": (50011, [0, 1, MS_TILE, MS_TILE + 1, 50000]),
    "segs_64": (MS_TILE + 8, [(0, 1, MS_TILE, MS_TILE + 1)[(s + s // 4) % 4] for s in range(64)]),
}


def msd_seg_case(name, nbits, lo_bit):
    """-> (keys[n_segs * seg_cap] with poison in the slack, counts, seg_cap, the valid records concatenated)"""
    cap, fills = MSD_SEG_CASES[name]
    n = sum(fills)
    valid = msd_uniform(n, nbits, lo_bit, seed=len(fills))
    keys = np.full(len(fills) * cap, POISON_KEY, np.uint64)
    at = 0
    for s, f in enumerate(fills):
        keys[s * cap:s * cap + f] = valid[at:at + f]
        at += f
    return keys, list(fills), cap, valid
