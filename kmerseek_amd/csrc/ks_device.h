// ks_device.h — device-side building blocks: MurmurHash3_x64_128.h1, wave/block scans.
// Written for gfx950: 64-lane waves, DPP/shuffle wave scans, LDS cross-wave combine.
#pragma once
#include "ks_common.h"

#define KS_DEV __device__ __forceinline__

// rotl by a compile-time count, as the two v_alignbit_b32 it is (the generic shift / or form costs four instructions here)
KS_DEV u64 ks_rotl64(u64 x, int r) {
#ifndef KS_NO_OPAQUE
    if (__builtin_constant_p(r) && r > 0 && r < 64 && r != 32) {
        const u32 lo = (u32)x, hi = (u32)(x >> 32);
        const u32 s = (u32)(r < 32 ? 32 - r : 64 - r);
        const u32 a = __builtin_amdgcn_alignbit(lo, hi, s), b = __builtin_amdgcn_alignbit(hi, lo, s);
        return r < 32 ? (((u64)b << 32) | a) : (((u64)a << 32) | b);
    }
#endif
    return (x << r) | (x >> (64 - r));
}

KS_DEV u64 ks_fmix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

#define KS_C1 0x87c37b91114253d5ULL
#define KS_C2 0x4cf5ad432745937fULL

// A product that is rotated next: the compiler folds the rotation's left shift into the multiplication — rotl(x * c, 31) becomes
// (x * (c << 31)) | ((x * c) >> 33), five 32-bit multiplies (half-rate instructions on gfx950: tools/gpu/valu_rates.hip) where
// three and two v_alignbit do.  An empty asm statement hides the product from that rewrite; it costs no instruction.
#ifndef KS_NO_OPAQUE
#define KS_OPAQUE64(x) asm("" : "+v"(x))
#else
#define KS_OPAQUE64(x) do { } while (0)
#endif

// Streaming state of MurmurHash3_x64_128 (both lanes seeded), as sourmash::_hash_murmur uses it
// (reference call site src/rust/index.rs:766; add_protein via src/rust/signature.rs:274).
struct ks_murmur {
    u64 h1, h2;
    KS_DEV void init(u64 seed) { h1 = seed; h2 = seed; }
    KS_DEV void block(u64 k1, u64 k2) {
        k1 *= KS_C1; KS_OPAQUE64(k1); k1 = ks_rotl64(k1, 31); k1 *= KS_C2; h1 ^= k1;
        h1 = ks_rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729ULL;
        k2 *= KS_C2; KS_OPAQUE64(k2); k2 = ks_rotl64(k2, 33); k2 *= KS_C1; h2 ^= k2;
        h2 = ks_rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5ULL;
    }
    // tail: k1 = bytes 0..7 (already masked), k2 = bytes 8..14 (already masked); t = len & 15
    KS_DEV void tail(u64 k1, u64 k2, u32 t) {
        if (t > 8) {
#ifndef KS_NO_OPAQUE
            if (__builtin_constant_p(t) && t <= 12) { // a tail of <= 4 bytes behind the first word: 32 x 64 bits = one v_mad_u64_u32, one v_mul_lo_u32, one add
                const u32 x = (u32)k2;
                u64 p = (u64)x * (u32)KS_C2;
                u32 xh = x * (u32)(KS_C2 >> 32);
                asm("" : "+v"(xh)); // (keeps the compiler from re-fusing the two into a chain of two v_mad_u64_u32 with moves between them)
                k2 = p + ((u64)xh << 32);
            } else
#endif
            k2 *= KS_C2;
            KS_OPAQUE64(k2); k2 = ks_rotl64(k2, 33); k2 *= KS_C1; h2 ^= k2;
        }
        if (t > 0) { k1 *= KS_C1; KS_OPAQUE64(k1); k1 = ks_rotl64(k1, 31); k1 *= KS_C2; h1 ^= k1; }
    }
    KS_DEV u64 finish(u64 len) {
        h1 ^= len; h2 ^= len;
        h1 += h2; h2 += h1;
        h1 = ks_fmix64(h1); h2 = ks_fmix64(h2);
        return h1 + h2;
    }
};

// bytes [8*I, 8*I+8) of the 16-byte little-endian pair (a, b): a funnel shift with a
// compile-time byte count, which hipcc lowers to v_alignbit/v_perm.
template <int I>
KS_DEV u64 ks_funnel(u64 a, u64 b) {
    if constexpr (I == 0) return a;
#ifndef KS_NO_OPAQUE
    else { // on the 32-bit words: two v_alignbyte_b32 at most (the 64-bit shift / or form takes three or four instructions)
        const u32 w0 = (u32)a, w1 = (u32)(a >> 32), w2 = (u32)b, w3 = (u32)(b >> 32);
        u32 lo, hi;
        if constexpr (I < 4) { lo = __builtin_amdgcn_alignbyte(w1, w0, (u32)I); hi = __builtin_amdgcn_alignbyte(w2, w1, (u32)I); }
        else if constexpr (I == 4) { lo = w1; hi = w2; }
        else { lo = __builtin_amdgcn_alignbyte(w2, w1, (u32)(I - 4)); hi = __builtin_amdgcn_alignbyte(w3, w2, (u32)(I - 4)); }
        return ((u64)hi << 32) | lo;
    }
#else
    else return (a >> (8 * I)) | (b << (64 - 8 * I));
#endif
}

KS_DEV u64 ks_funnel_rt(u64 a, u64 b, u32 byte_shift) {
    u32 s = byte_shift * 8;
    return s ? ((a >> s) | (b << (64 - s))) : a;
}

KS_DEV u64 ks_mask_bytes(u32 n) { return n >= 8 ? ~0ULL : ((1ULL << (8 * n)) - 1ULL); }

// Workgroups of a launch go round-robin to the 8 XCDs of the MI355X (each with its own L2).  Kernels whose neighbouring
// tiles touch the same cache lines (partition scatters: a tile's digit runs end where the next tile's begin) take their
// tile id from this instead of blockIdx.x: XCD x works through a contiguous eighth of the tiles, so the lines two tiles
// share are assembled in ONE L2 (measured on the bucket scatter: 1.58 -> 1.29 ms, and the join that reads its output
// 2.17 -> 1.80 ms).  A bijection on [0, gridDim.x) for any grid size: XCD x = b & 7 owns g/8 tiles (one more for the
// first g%8 XCDs), its j-th workgroup (j = b >> 3) takes the j-th of them.
KS_DEV u32 ks_xcd_block() {
    const u32 b = blockIdx.x, g = gridDim.x, x = b & 7u, q = g >> 3, rem = g & 7u;
    return x * q + (x < rem ? x : rem) + (b >> 3);
}

// Decoupled look-back spins are bounded by TIME — the constant-rate wall clock (100 MHz on gfx950), read only every 1024
// polls — not by an iteration count: a predecessor that is merely slow (a shared GPU, several ranks rehearsing on one
// device) must not look like a protocol violation.  ~2 s.
#define KS_SPIN_TICKS 200000000LL
struct ks_spin { long long t0; u32 polls; }; // one per look-back: all its rounds share the bound
KS_DEV ks_spin ks_spin_begin() { return {wall_clock64(), 0u}; }
KS_DEV bool ks_spin_expired(ks_spin &s) {
    return ((++s.polls) & 1023u) == 0 && wall_clock64() - s.t0 > KS_SPIN_TICKS;
}

// ---- wave / block exclusive scans (u32) ----
// Inclusive scan over the 64 lanes of a wave with DPP moves only (no LDS crossbar round trips: __shfl_up lowers to
// ds_bpermute_b32): four row_shr steps scan each row of 16, row_bcast:15 carries row 0 -> 1 and row 2 -> 3, row_bcast:31
// carries the first half into the second.  Lanes without a source add 0.
KS_DEV u32 ks_wave_incl_scan(u32 v) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1 and 3
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2 and 3
    return v;
}
// Sum of a 64-bit value over the 64 lanes of a wave (uniform result), DPP moves only: the look-backs' reduce used to be
// `v += __shfl_xor(v, d)` — twelve ds_bpermute in a row on the critical path of every tile.
KS_DEV u64 ks_wave_sum64(u64 v) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#define KS_SUM64_STEP(CTRL, RMASK, BC) do { \
        const u32 ol_ = (u32)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, RMASK, 0xf, BC); \
        const u32 oh_ = (u32)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, RMASK, 0xf, BC); \
        const u64 s_ = (((u64)hi << 32) | lo) + (((u64)oh_ << 32) | ol_); \
        lo = (u32)s_; hi = (u32)(s_ >> 32); } while (0)
    KS_SUM64_STEP(0x111, 0xf, true);  // row_shr:1
    KS_SUM64_STEP(0x112, 0xf, true);  // row_shr:2
    KS_SUM64_STEP(0x114, 0xf, true);  // row_shr:4
    KS_SUM64_STEP(0x118, 0xf, true);  // row_shr:8
    KS_SUM64_STEP(0x142, 0xa, false); // row_bcast:15 into rows 1 and 3
    KS_SUM64_STEP(0x143, 0xc, false); // row_bcast:31 into rows 2 and 3
#undef KS_SUM64_STEP
    return ((u64)(u32)__builtin_amdgcn_readlane((int)hi, 63) << 32) | (u32)__builtin_amdgcn_readlane((int)lo, 63);
}
// Sum of a 32-bit value over the 64 lanes of a wave, in every lane: the end of a row's re-scoring, once per wave
KS_DEV u32 ks_wave_sum32(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (u32)__shfl_xor((int)v, d);
    return v;
}
// the quiet NaN of a row that has no value in a double column
KS_DEV double ks_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// Largest of a 64-bit value over the 64 lanes of a wave (uniform result), the same DPP moves: a lane without a source compares
// with 0.  The argmax of ks_hits_gather: its keys are (count << 32) | ~row.
KS_DEV u64 ks_wave_max64(u64 v) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#define KS_MAX64_STEP(CTRL, RMASK, BC) do { \
        const u32 ol_ = (u32)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, RMASK, 0xf, BC); \
        const u32 oh_ = (u32)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, RMASK, 0xf, BC); \
        const u64 m_ = ((u64)hi << 32) | lo, o_ = ((u64)oh_ << 32) | ol_; \
        const u64 s_ = o_ > m_ ? o_ : m_; \
        lo = (u32)s_; hi = (u32)(s_ >> 32); } while (0)
    KS_MAX64_STEP(0x111, 0xf, true);  // row_shr:1
    KS_MAX64_STEP(0x112, 0xf, true);  // row_shr:2
    KS_MAX64_STEP(0x114, 0xf, true);  // row_shr:4
    KS_MAX64_STEP(0x118, 0xf, true);  // row_shr:8
    KS_MAX64_STEP(0x142, 0xa, false); // row_bcast:15 into rows 1 and 3
    KS_MAX64_STEP(0x143, 0xc, false); // row_bcast:31 into rows 2 and 3
#undef KS_MAX64_STEP
    return ((u64)(u32)__builtin_amdgcn_readlane((int)hi, 63) << 32) | (u32)__builtin_amdgcn_readlane((int)lo, 63);
}
// inclusive running maximum over the 64 lanes of a wave, the DPP moves of ks_wave_incl_scan; lanes without a source compare with 0
KS_DEV u32 ks_wave_incl_max(u32 v) {
#define KS_MAX_STEP(CTRL, RMASK, BC) do { \
        const u32 o_ = (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RMASK, 0xf, BC); \
        v = o_ > v ? o_ : v; } while (0)
    KS_MAX_STEP(0x111, 0xf, true);  // row_shr:1
    KS_MAX_STEP(0x112, 0xf, true);  // row_shr:2
    KS_MAX_STEP(0x114, 0xf, true);  // row_shr:4
    KS_MAX_STEP(0x118, 0xf, true);  // row_shr:8
    KS_MAX_STEP(0x142, 0xa, false); // row_bcast:15 into rows 1 and 3
    KS_MAX_STEP(0x143, 0xc, false); // row_bcast:31 into rows 2 and 3
#undef KS_MAX_STEP
    return v;
}
// value of the lane below (lane 0: 0)
KS_DEV u32 ks_lane_below(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); } // wave_shr:1
// largest value over the 64 lanes of a wave (every lane gets it)
KS_DEV u32 ks_wave_max_u32(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const u32 o = (u32)__shfl_xor((int)v, d); v = o > v ? o : v; }
    return v;
}
// number of entries of the ascending a[0, n) below x = the first i with a[i] >= x
template <typename T> KS_DEV u32 ks_lower_bound(const T *a, u32 n, T x) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
KS_DEV u32 ks_lower_bound_u64(const u64 *a, u32 n, u64 x) { return ks_lower_bound<u64>(a, n, x); }
KS_DEV u32 ks_lower_bound_u32(const u32 *a, u32 n, u32 x) { return ks_lower_bound<u32>(a, n, x); }
// last index in [lo, hi] whose off[] is <= p (off[lo] <= p holds): the owner of element p in a CSR
KS_DEV u32 ks_last_le_u64(const u64 *off, u32 lo, u32 hi, u64 p) {
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same among n ascending u32 (a tile's offsets relative to its begin, staged in LDS); a[0] <= x holds
KS_DEV u32 ks_last_le_u32(const u32 *a, u32 n, u32 x) {
    u32 lo = 0, hi = n - 1;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo + 1) >> 1);
        if (a[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// Hit rows are ordered by (qid, tid): the rows of query q are the segment [ks_query_row_begin(q), ks_query_row_begin(q + 1)).
// The first row whose qid is >= q (n_rows: none) — ks_match_positions' row_begin table and the segments of ks_hits_best.
KS_DEV u32 ks_query_row_begin(const u32 *qid, u32 n_rows, u32 q) { return ks_lower_bound_u32(qid, n_rows, q); }
// sum of the abundances of one run [b, e) of a sorted posting list (the union's and the corpus's record per distinct hash)
KS_DEV u64 ks_run_abund_sum(const u32 *vals, u64 b, u64 e) { u64 w = 0; for (u64 j = b; j < e; j++) w += vals[j]; return w; }

// ---- the move of one row of a hit list (rf_cols, ks_common.h: the compactions of min_containment and of ks_hits_best) ----
KS_DEV void rf_move(const rf_cols &in, u32 r, u32 o, u32 *qid, u32 *tid, u32 *isect, u64 *nw, u64 *median2, double *ss) {
    qid[o] = in.qid[r]; tid[o] = in.tid[r]; isect[o] = in.isect[r]; nw[o] = in.nw[r];
    if (median2) { median2[o] = in.median2[r]; ss[o] = in.ss[r]; }
}

// the first row that is wrong for reason `why` (a control block's words, ks_ctl; all ones: none)
KS_DEV void ks_first_bad(unsigned long long *bad, u32 why, u32 r) { atomicMin(&bad[why], (unsigned long long)r); }

// ---- short rows by a lane, long rows by a wave ----
// A pass with a lane per row pushes the rows that are too long for one lane onto a list (list[0] counts, the rows follow:
// ks_row_list_alloc on the host); a fixed grid of 4-wave workgroups strides over it, a wave per row, 64 elements per chunk, and
// adds what it sums serially in lane order through readlane (every lane keeps the same sums): a host loop's f64 results.
KS_DEV void ks_row_list_push(u32 *list, u32 r) { list[1 + atomicAdd(&list[0], 1u)] = r; }
// row(r) for every listed row, one wave each (r is wave-uniform); a count beyond n_rows — the most the list can hold — is cut
template <typename Row> KS_DEV void ks_row_list_walk(const u32 *list, u32 n_rows, Row row) {
    const u32 n_waves = gridDim.x * (blockDim.x / 64);
    const u32 n_list = list[0] < n_rows ? list[0] : n_rows;
    for (u32 w = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w < n_list; w += n_waves) row(list[1 + w]);
}
KS_DEV double ks_readlane_f64(double v, int j) {
    const u64 b = (u64)__double_as_longlong(v);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)b, j), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(b >> 32), j);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
// acc += lane j's x (and acc2 += lane j's x2, in the same walk) for every set bit j of m, ascending.  m is wave-uniform; it
// is taken from the first lane so that the walk runs on the scalar unit also where the compiler cannot see that.
KS_DEV void ks_wave_add_ordered(u64 m, double &acc, double x, double &acc2, double x2) {
#pragma clang fp contract(off)
    m = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(m >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)m);
    while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        acc += ks_readlane_f64(x, j); acc2 += ks_readlane_f64(x2, j);
    }
}
KS_DEV void ks_wave_add_ordered(u64 m, double &acc, double x) { double none = 0.0; ks_wave_add_ordered(m, acc, x, none, 0.0); }
// the mask of the lanes below n (n <= 64)
KS_DEV u64 ks_lanes_below(u32 n) { return n >= 64u ? ~0ULL : (1ULL << n) - 1ULL; }

// ---- a query's rows by a wave or by a workgroup ----
// A query's rows are one segment.  The lane of its first row finds its length and pushes (first row, rows) onto the list of the
// kernel that takes it (list[0] counts, also past `cap`: only a list of rows that are not a hit list's can; ks_seg_list_alloc on
// the host); a fixed grid strides over a list: for (ks_seg_walk seg = ks_seg_list_by_wave(list, cap); seg.next();), or _by_wg.
// The loop stays in the kernel's own body, unlike ks_row_list_walk's callable: a workgroup's segment code reads the block size
// (ks_block_excl_scan) in every round, and inside a callable of a function template the compiler reads it with a vector load.
KS_DEV u32 ks_readfirst(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
// rows of the segment of query q that begins at row r (q + 1 does not wrap: the last id there is ends the list)
KS_DEV u32 ks_seg_len(const u32 *qid, u32 n_rows, u32 r, u32 q) {
    return q == 0xffffffffu ? n_rows - r : ks_query_row_begin(qid + r, n_rows - r, q + 1);
}
KS_DEV void ks_seg_list_push(u32 *list, u32 cap, u32 b, u32 len) {
    const u32 i = atomicAdd(&list[0], 1u);
    if (i < cap) { list[1 + 2 * i] = b; list[2 + 2 * i] = len; }
}
// The same for a whole workgroup (every thread enters; `want`: this thread has a segment to list; s: two u32 of LDS, the caller's
// again on return): the waves reserve their places on an LDS counter, one atomic per workgroup goes to the list's.  For a pass
// that lists a large part of its rows: every atomic on the one counter takes ~10 ns on gfx950, so 50,000 pushes of single
// lanes are 0.55 ms of a launch and 30,000 pushes of single waves still 0.3 ms (ks_rcull.hip's plan, measured).
KS_DEV void ks_seg_list_push_block(u32 *list, u32 cap, bool want, u32 b, u32 len, u32 *s) {
    if (threadIdx.x == 0) s[0] = 0;
    __syncthreads();
    const u64 m = __ballot(want);
    u32 at = 0;
    if (m) {
        const u32 lane = threadIdx.x & 63, leader = ks_readfirst((u32)__ffsll((long long)m) - 1u);
        if (lane == leader) at = atomicAdd(&s[0], (u32)__popcll((long long)m));
        at = (u32)__builtin_amdgcn_readlane((int)at, (int)leader) + (u32)__popcll((long long)(m & ks_lanes_below(lane)));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s[0]) s[1] = atomicAdd(&list[0], s[0]);
    __syncthreads();
    const u32 i = s[1] + at;
    if (want && i < cap) { list[1 + 2 * i] = b; list[2 + 2 * i] = len; }
    __syncthreads();
}
struct ks_seg_walk {
    const u32 *list;
    u32 n, w, step, b, len; // (b and len: wave-uniform, in scalar registers)
    KS_DEV bool next() {
        if (w >= n) return false;
        b = ks_readfirst(list[1 + 2 * w]); len = ks_readfirst(list[2 + 2 * w]);
        w += step;
        return true;
    }
};
KS_DEV ks_seg_walk ks_seg_list_by_wg(const u32 *list, u32 cap) { return {list, list[0] < cap ? list[0] : cap, blockIdx.x, gridDim.x, 0u, 0u}; }
KS_DEV ks_seg_walk ks_seg_list_by_wave(const u32 *list, u32 cap) {
    const u32 per_wg = blockDim.x / 64;
    return {list, list[0] < cap ? list[0] : cap, blockIdx.x * per_wg + (threadIdx.x >> 6), gridDim.x * per_wg, 0u, 0u};
}

// ---- the hashes the two sketches of a hit row share ----
// The shorter run is walked, the longer one searched: both ascend.  Positions are reported INSIDE q's sketch, whichever is walked.
struct ks_run_pair {
    const u64 *wh, *sh; // the walked run, the searched run
    u32 nw, ns;         // their lengths
    bool walk_q;        // the query's is the walked one
    u64 qb;             // where q's sketch begins in the query arrays
};
KS_DEV ks_run_pair ks_run_pair_of(const u64 *q_off, const u64 *q_hash, const u64 *t_off, const u64 *t_hash, u32 q, u32 t) {
    const u64 qb = q_off[q], tb = t_off[t];
    const u32 nq = (u32)(q_off[q + 1] - qb), nt = (u32)(t_off[t + 1] - tb);
    const bool walk_q = nq <= nt;
    return {walk_q ? q_hash + qb : t_hash + tb, walk_q ? t_hash + tb : q_hash + qb, walk_q ? nq : nt, walk_q ? nt : nq, walk_q, qb};
}
// One lane walks: every search starts where the last one ended.  shared(position, shared hashes before it) once per shared
// hash, ascending.  Returns their count.
template <typename Shared> KS_DEV u32 ks_shared_walk_lane(const ks_run_pair &P, Shared shared) {
    u32 cnt = 0, from = 0;
    for (u32 i = 0; i < P.nw && from < P.ns; i++) {
        const u64 h = P.wh[i];
        from += ks_lower_bound_u64(P.sh + from, P.ns - from, h);
        if (from < P.ns && P.sh[from] == h) {
            shared(P.walk_q ? i : from, cnt);
            cnt++;
        }
    }
    return cnt;
}
// One wave walks (all 64 lanes enter), 64 hashes of the walked run per chunk, loaded coalesced; every lane searches the whole
// other run for its own.  chunk(this lane's hash is shared, its position, the ballot of the lanes that share, shared hashes
// before the chunk) once per chunk: lane order is ascending hash order.  Returns the count (uniform).
template <typename Chunk> KS_DEV u32 ks_shared_walk_wave(const ks_run_pair &P, u32 lane, Chunk chunk) {
    u32 cnt = 0;
    for (u32 c = 0; c < P.nw; c += 64) {
        const u32 i = c + lane;
        bool found = false;
        u32 at = 0;
        if (i < P.nw) {
            const u64 h = P.wh[i];
            at = ks_lower_bound_u64(P.sh, P.ns, h);
            found = at < P.ns && P.sh[at] == h;
        }
        const u64 m = __ballot(found);
        chunk(found, P.walk_q ? i : at, m, cnt);
        cnt += (u32)__popcll((long long)m);
    }
    return cnt;
}

// Block-wide exclusive scan; `smem` must hold (blockDim.x/64 + 1) u32.  Returns the exclusive
// prefix of v; *total receives the block sum.  Contains three __syncthreads().
// The scan a new kernel should take: any block size, and smem is the caller's again on return.  sk_block_excl_scan1 / 2
// (ks_sketch.hip) are for SK_THREADS-thread kernels that count barriers and registers: one barrier, but smem stays in use
// until the caller's next barrier.
KS_DEV u32 ks_block_excl_scan(u32 v, u32 *smem, u32 *total) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u32 incl = ks_wave_incl_scan(v);
    if (lane == 63) smem[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        u32 w = lane < nw ? smem[lane] : 0;
        u32 wi = ks_wave_incl_scan(w);
        if (lane < nw) smem[lane] = wi - w;
        if (lane == nw - 1) smem[nw] = wi;
    }
    __syncthreads();
    u32 base = smem[wave];
    *total = smem[nw];
    __syncthreads(); // smem may be reused by the caller right away
    return base + incl - v;
}

KS_DEV u64 ks_ballot(bool p) { return __ballot(p); }
KS_DEV u32 ks_lane_lt_count(u64 mask) {
    // number of set bits of mask in lanes below this one
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0));
}

// ---- decoupled look-back ----
// Tiles that place their output behind their predecessors' (k_sketch_tiles, k_kmerpos_tiles, k_pair_rows_fused,
// k_scan_lookback) chain their totals through one 8-byte status word per tile, `flag << 62 | value`: a tile publishes its
// aggregate (flag 1; tile 0 its inclusive prefix at once), one wave sums its predecessors' words back to the nearest
// inclusive prefix (flag 2), 64 at a time, and the tile re-publishes aggregate + that sum as its own inclusive prefix.
// A word that is not published yet (flag 0) is polled under the bound of ks_spin_expired; when the bound expires the lane
// raises bit 0 of *gave_up, counts the word as prefix 0 and goes on — the launch's output is wrong, nothing hangs, and the
// host repeats the launch with tile ids from an atomic ticket.  Publishing, re-publishing and what the prefix is used for
// stay with the kernels; the words are stored and loaded relaxed at agent scope.
#define KS_LB_AGG (1ULL << 62)
#define KS_LB_PRE (2ULL << 62)
#define KS_LB_VAL_MASK ((1ULL << 62) - 1)

// One wave's round: lane l looks at predecessor idx - l (none before tile 0: inclusive prefix 0).  `word(i)` returns
// predecessor i's status word, 0 while it is not published.  Returns the sum over the lanes at or before the wave's first
// inclusive prefix (uniform); *is_pre = the lanes that saw one (0: none, the walk goes on at idx - 64).  Holds a ballot and
// DPP moves: EVERY lane of the wave must enter, so the caller's guard is wave-uniform.
template <typename Word>
KS_DEV u64 ks_lookback_round(i64 idx, u32 lane, Word word, ks_spin &spin, u32 *gave_up, u64 *is_pre) {
    const i64 mine = idx - (i64)lane;
    u64 v = KS_LB_PRE;
    if (mine >= 0) {
        v = word(mine);
        while ((v >> 62) == 0 && !ks_spin_expired(spin)) {
            __builtin_amdgcn_s_sleep(1);
            v = word(mine);
        }
    }
    if ((v >> 62) == 0) { atomicOr(gave_up, 1u); v = KS_LB_PRE; }
    *is_pre = __ballot((v >> 62) == 2);
    const u32 first = *is_pre ? (u32)__ffsll((long long)*is_pre) - 1u : 64u;
    return ks_wave_sum64(lane <= first ? (v & KS_LB_VAL_MASK) : 0);
}
// The walk of a single wave (all 64 lanes enter): exclusive prefix of tile > 0.
template <typename Word>
KS_DEV u64 ks_lookback_walk(u32 tile, u32 lane, Word word, u32 *gave_up) {
    u64 excl = 0;
    ks_spin spin = ks_spin_begin();
    u64 is_pre = 0;
    for (i64 idx = (i64)tile - 1; !is_pre; idx -= 64) excl += ks_lookback_round(idx, lane, word, spin, gave_up, &is_pre);
    return excl;
}
// status words in a plain array
KS_DEV auto ks_lookback_words(const unsigned long long *status) {
    return [status](i64 i) -> u64 { return __hip_atomic_load(&status[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
}

// Stable rank of an 8-bit digit inside one wave ("match-any" by eight ballots): returns d << 16 | (records of digit d the wave
// counted before this round + lanes below mine that hold d), and adds the round's count to the wave's counter wc[d].
// Per bit: the lane's bit as a mask (v_bfe_i32: 0 / -1), one ballot, and peers &= ~(ballot ^ mask) on each half — a three-input
// boolean, one v_bitop3_b32 (the generic select form `bit ? m : ~m` compiled to nine vector instructions per bit).  The lowest
// lane of a group of peers (no peer below it) publishes the new count; EVERY lane reads the old one first — the LDS operations
// of a wave execute in order, so no lane-to-lane exchange (ds_bpermute) is needed for it.
KS_DEV u32 ks_match8_rank(u32 d, u32 *wc) {
    u32 plo = ~0u, phi = ~0u;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const u32 bm = (u32)__builtin_amdgcn_sbfe((int)d, (u32)b, 1u);
        const u64 m = __ballot(bm != 0u);
        plo &= ~((u32)m ^ bm);
        phi &= ~((u32)(m >> 32) ^ bm);
    }
    const u32 below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0));
    const u32 pre = wc[d];
    if (below == 0) wc[d] = pre + (u32)__popc(plo) + (u32)__popc(phi);
    return (d << 16) | (pre + below);
}

// Join prefix of a kept hash: floor(h * 2^pbits / (max_hash + 1)) computed on the top 32 bits — uniform over
// [0, 2^pbits) for every `scaled` (kept hashes only span [0, max_hash], so plain top bits are NOT uniform for scaled > 1).
// K = floor(2^(pbits+32) / ((max_hash >> 32) + 1)); for scaled = 1 this is exactly h >> (64 - pbits).  Monotone in h.
KS_DEV u32 ks_join_prefix(u64 h, u32 K) { return __umulhi((u32)(h >> 32), K); }
// The presence filter (ks_index::d_presence) tests two bits of one 32-bit word per hash: with p = the hash's join prefix at the
// bitmap's width, bit p & 31 of word p >> 5 and the bit this names — bits [8, 13) of the LOW hash word, which every posting
// width carries intact (the 10-byte form rewrites a field of the high word only) and which a hash shares with its neighbour
// h ^ 1.  32-bit words, so that a probe stays a 4-byte gather (8-byte ones measured slower: DESIGN.md §3.2 [r7]).
KS_DEV u32 ks_presence_bit2(u64 h) { return ((u32)h >> 8) & 31u; }
// digit of a radix pass: plain key bits (K == 0) or bits [shift, shift + 8) of the join prefix
KS_DEV u32 ks_rs_digit(u64 key, int shift, u32 K) {
    return K ? ((ks_join_prefix(key, K) >> shift) & 255u) : ((u32)(key >> shift) & 255u);
}
