"""Plain numpy restatements of the device-wide primitives (ks_prims.hip, ks_msd.hip): what tests/test_gpu_prims.py holds the
kernels to.  Imports nothing of the library.  Everything is integers and exact equality.

- exclusive scans: np.cumsum in uint64 (u32 -> u64), or reduced mod 2^32 (u32 -> u32);
- the stable LSD sort: one stable argsort of the 8-bit digit per listed shift, in the order listed;
- the MSD match sort: no order is promised among equal keys, so the reference is a pair of properties — the output is a
  permutation of the input as full 64-bit words, and the key field never descends;
- ms_layout_of's choice of the second partition level, restated, and the number of buckets that go to the large-bucket kernel."""
import numpy as np

U32 = 0xFFFFFFFF
SCAN_TILE = 2048   # ks_prims.hip: SCAN_THREADS * SCAN_IPT
SCAN_RING = 1 << 20
SCAN_VAL_BITS = 38
RS_TILE = 8192     # ks_prims.hip: RS_THREADS * RS_IPT
MS_TILE = 8192     # ks_msd.hip
ML_CAP = 4096      # ks_msd.hip: records of a bucket sorted inside LDS
ML_WCAP = 1024     # ... by one wave
MSD_MIN_N = 65536  # shorter lists (and keys of 16 bits or fewer) take the LSD sort


def scan_ref(a, kind):
    """kind 0 (and 2, the same without a bound on the sum): out[n + 1] uint64, out[n] = total.  kind 1: (out[n] uint32, total) mod 2^32."""
    a = np.asarray(a, np.uint32)
    incl = np.cumsum(a, dtype=np.uint64)
    excl = np.zeros(len(a) + 1, np.uint64)
    excl[1:] = incl
    if kind != 1:
        return excl
    return (excl[:-1] & np.uint64(U32)).astype(np.uint32), int(excl[-1]) & U32


def scan_tiles(n):
    return (n + SCAN_TILE - 1) // SCAN_TILE


def lsd_digit(keys, shift, pfx_k=0):
    """the digit of a pass (ks_rs_digit): bits [shift, shift + 8) of the key, or of umulhi(key >> 32, pfx_k)"""
    keys = np.asarray(keys, np.uint64)
    if pfx_k:
        v = ((keys >> np.uint64(32)) * np.uint64(pfx_k)) >> np.uint64(32)
    else:
        v = keys
    return ((v >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)


def lsd_sort_ref(keys, vals, shifts, pfx_k=0):
    """-> (keys, vals) after one stable pass per listed shift; vals may be None"""
    keys = np.asarray(keys, np.uint64)
    order = np.arange(len(keys))
    for s in shifts:
        order = order[np.argsort(lsd_digit(keys[order], s, pfx_k), kind="stable")]
    return keys[order], (None if vals is None else np.asarray(vals)[order])


def msd_field(keys, lo_bit, nbits):
    keys = np.asarray(keys, np.uint64)
    mask = np.uint64((1 << nbits) - 1)
    return (keys >> np.uint64(lo_bit)) & mask


def msd_check(inp, out, lo_bit, nbits):
    """the contract of the match sort: a permutation of the input whose key field never descends"""
    inp, out = np.asarray(inp, np.uint64), np.asarray(out, np.uint64)
    assert out.shape == inp.shape
    assert np.array_equal(np.sort(out), np.sort(inp)), "not a permutation of the input (records lost, doubled or altered)"
    f = msd_field(out, lo_bit, nbits)
    bad = np.flatnonzero(f[1:] < f[:-1])
    assert bad.size == 0, f"key field descends at {bad[:5]} ({bad.size} places)"


def msd_applies(n, nbits):
    return nbits > 16 and n >= MSD_MIN_N


def msd_bits2(n, nbits):
    """ms_layout_of (ks_msd.hip): ~768 records per bucket, then as wide as it takes to save a local 8-bit pass, one bit left"""
    b2 = 0
    while b2 < 9 and (n >> (8 + b2)) > (768 if b2 < 8 else 560):
        b2 += 1
    for b in range(b2 + 1, 9):
        if nbits - 8 - b <= 0:
            break
        if (nbits - 8 - b + 7) // 8 < (nbits - 8 - b2 + 7) // 8:
            b2 = b
            break
    if nbits - 8 - b2 <= 0:
        b2 = max(nbits - 9, 0)
    return b2


def msd_big_buckets(keys, lo_bit, nbits, lds_cap=ML_CAP):
    """buckets k_msd_local leaves to k_msd_local_big: those of more than min(lds_cap, ML_WCAP) records"""
    b2 = msd_bits2(len(keys), nbits)
    shift2 = lo_bit + nbits - 8 - b2
    if shift2 - lo_bit <= 0:
        return 0
    bucket = ((np.asarray(keys, np.uint64) >> np.uint64(shift2)) & np.uint64((1 << (8 + b2)) - 1)).astype(np.int64)
    return int((np.bincount(bucket, minlength=1 << (8 + b2)) > min(lds_cap, ML_WCAP)).sum())


def msd_info_ref(keys, lo_bit, nbits, lds_cap=ML_CAP):
    """what ks_debug_msd_sort reports for a dense list `keys`"""
    n = len(keys)
    if not msd_applies(n, nbits):
        return {"done": 0, "bits2": 0, "n_buckets": 0, "big": 0}
    b2 = msd_bits2(n, nbits)
    return {"done": 1, "bits2": b2, "n_buckets": 1 << (8 + b2), "big": msd_big_buckets(keys, lo_bit, nbits, lds_cap)}


class RingModel:
    """Which tag each slot of the scans' status ring holds, kept alongside a context: a one-launch scan of `tiles` tiles from
    global tile number `base` is a valid input only if no slot it uses still holds the tag it is about to expect there (the
    counter cannot reach such a state by counting; a seek can)."""

    def __init__(self):
        self.slot_tag = {}

    def scan(self, base, tiles):
        use = [(base + t) & U32 for t in range(tiles)]
        for g in use:
            assert self.slot_tag.get(g % SCAN_RING) != (g & 0xFFFFFF), f"tile {g:#x} would meet its own tag as a left-over"
        for g in use:
            self.slot_tag[g % SCAN_RING] = g & 0xFFFFFF
