// ks_mask.hip — low-complexity masking of a residue batch on the device, the split of the batch into its unmasked segments, and
// the masked sketch and masked k-mer positions built on them.  The rule (include/kmerseek_amd.h) is this library's own, defined in
// integers: the first stage of SEG — trigger windows, extension over contiguous windows — without the second-stage trimming.
// NCBI seg is not part of the build and NO PARITY IS CLAIMED.
//
//   classes   rk_class (ks_rkit.h): 26 letters without case, '*', everything else: 28.
//   e(p)      T[W] - sum over classes of T[count] for the W residues from p on, T[c] = floor(c log2(c) 65536 + 0.5) (mk_T, literal).
//             Computed as T[W] - sum over j of D[rank_j], D[r] = T[r] - T[r - 1], rank_j = how often the class of residue j has
//             occurred in the window up to and including j: a class with n members adds D[1] + ... + D[n] = T[n].
//   lo2 / lo1 e(p) <= floor(k W 65536 / 1000) for k2 / k1 and the window valid (it ends inside p's record).
//
//   bounds    k_mask_bounds, a lane per record: the offsets checked (0 first, ascending, n_res last, no record beyond 2^32 - 16
//             residues: the first bad record comes back with the call's one wait) and bound[first residue] = 1 for every record
//             that has one.  No later kernel looks a record up: "the window ends inside its record" is "no bound byte in (p, p + W)
//             and p + W <= n_res", "a segment begins here" needs bound[p] — plain bytes beside the residues.
//   flags     k_mask_flags, a workgroup per MK_CHUNK residues: classes and bound bytes of the chunk and a right halo of MK_HALO
//             >= W - 1 into LDS (four per 32-bit load where the pointer allows), D in LDS; a lane owns four consecutive window
//             starts and stores their four flag bytes (bit 0 lo2, bit 1 lo1) as one word.  Lanes 4 bytes apart: the LDS byte
//             reads of a wave fall into 64 consecutive banks.
//   runs      heads (lo2 and the start before is not) -> ks_scan_u32_inplace -> run ids; a lo1 start stores 1 into hot[run]
//             (plain vector stores of the same value).
//   mask      k_mask_apply, a workgroup per MK_CHUNK residues: "lo2 and its run is hot" for the chunk's starts and a LEFT halo
//             into LDS; residue p is masked iff one of the W starts (p - W, p] is set (a valid window never reaches over a record
//             end, so none of another record can cover p).  One word of four mask bytes per lane and store.
//   counts    a wave per record sums its mask bytes (counting, no order shows).
//   split     heads of unmasked stretches (unmasked, and first of the batch / bound / behind a masked one) -> scan -> the stretch
//             number of every head and, by the same scan, of every tail; lengths >= min_len -> scan -> kept segments; per kept
//             segment its record (a binary search over the offsets), its start in the record, its length -> scan to u64 offsets;
//             a wave per segment copies its residues; group_offsets[r] = kept segments of records below r, a binary search over
//             seg_record (counting, not atomics).
// Every index that leads to a store is held against the capacity of what it writes: offsets that lie cannot make a kernel
// write outside its buffers.  No inline assembly and no scalar memory writes anywhere in this file.
//
// ks_sketch_masked*: mask and split queued behind one another, ONE wait -> ks_sketch_device_impl on the segments, unchanged ->
// ks_union_groups_impl by record (a record with more than UN_RANK_MAX segments sends the batch down the union's sort path).
#include "ks_rkit.h"

#define MK_THREADS 256
#define MK_CHUNK 4096u // residues a workgroup owns
#define MK_HALO 32u    // staged beside the chunk: >= KS_MASK_MAX_WINDOW - 1, a multiple of 4
#define MK_SPAN (MK_CHUNK + MK_HALO)
#define MK_MAX_LEN 0xfffffff0ULL
#define MK_MAX_RES 0xffffffc0ULL // the scans of heads are 32-bit
#define MK_PAD_CLASS 255u
static_assert(MK_HALO + 1 >= KS_MASK_MAX_WINDOW && MK_HALO % 4 == 0 && MK_CHUNK % (4 * MK_THREADS) == 0, "mask geometry");

// T[c] = floor(c log2(c) 65536 + 0.5) for c <= KS_MASK_MAX_WINDOW
__device__ const u32 mk_T[KS_MASK_MAX_WINDOW + 1] = {
    0, 0, 131072, 311616, 524288, 760849, 1016449, 1287880, 1572864, 1869698, 2177059, 2493890, 2819329, 3152656, 3493263, 3840630, 4194304,
    4553891, 4919044, 5289451, 5664838, 6044953, 6429573, 6818492, 7211522, 7608494, 8009248, 8413640, 8821535, 9232807, 9647339, 10065024,
    10485760};

// the control block of a mask / split call (ks_ctl): one first-offender word, then the counters
enum { MK_BAD = 0, MK_MASKED = 1, MK_RUNS = 2, MK_RAW = 3, MK_SEGS = 4, MK_CTL_WORDS = 5 };

// bad[0] = the first record whose offsets are not 0 first, ascending, n_res last and at most MK_MAX_LEN apart; bound[p] = 1 where a record begins
__global__ __launch_bounds__(256) void k_mask_bounds(const u64 *off, u32 n_seqs, u64 n_res, u8 *bound, unsigned long long *bad) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    const u64 a = off[s], e = off[s + 1];
    if (e < a || e > n_res || e - a > MK_MAX_LEN || (s == 0 && a != 0) || (s == n_seqs - 1 && e != n_res)) ks_first_bad(bad, MK_BAD, s);
    else if (a < e) bound[a] = 1; // (a < e <= n_res)
}

// four staged bytes from position p on: the bytes of src where they exist (one load where `words` and all four do), `pad` elsewhere
template <class Map> KS_DEV u32 mk_stage4(const u8 *src, bool words, u64 p, u64 n, u32 pad, Map map) {
    if (words && p < n && p + 3 < n) {
        const u32 v = *(const u32 *)(src + p);
        return map(v & 255u) | (map((v >> 8) & 255u) << 8) | (map((v >> 16) & 255u) << 16) | (map(v >> 24) << 24);
    }
    u32 packed = 0;
#pragma unroll
    for (u32 k = 0; k < 4; k++) packed |= (p + k < n ? map(src[p + k]) : pad) << (8 * k);
    return packed;
}

// flags[p]: bit 0 lo2, bit 1 lo1 of the window that starts at p.  `cap`: bytes flags holds (a multiple of 4, >= n_res).
// WT: the window length at compile time (the default, 12: the two loops unroll and the window's bytes are read from LDS once), or
// 0 for any length, Wrt.  Same arithmetic either way.
template <u32 WT>
__global__ __launch_bounds__(MK_THREADS) void k_mask_flags(const u8 *res, const u8 *bound, u64 n_res, u32 Wrt, u32 thr1, u32 thr2, u8 *flags, u64 cap) {
    const u32 W = WT ? WT : Wrt;
    __shared__ __attribute__((aligned(16))) u8 s_cls[MK_SPAN]; // s_cls[i]: the class of the residue at c0 + i
    __shared__ __attribute__((aligned(16))) u8 s_bnd[MK_SPAN]; // 1: a record begins there (or the batch has ended)
    __shared__ u32 s_D[KS_MASK_MAX_WINDOW + 1];
    const u32 tid = threadIdx.x;
    const u64 c0 = (u64)blockIdx.x * MK_CHUNK;
    if (tid >= 1 && tid <= KS_MASK_MAX_WINDOW) s_D[tid] = mk_T[tid] - mk_T[tid - 1];
    const bool words = ((uintptr_t)res & 3u) == 0; // (c0 is a multiple of 4; bound is a pool block)
    for (u32 w = tid; w < MK_SPAN / 4; w += MK_THREADS) {
        const u64 p = c0 + 4 * (u64)w;
        *(u32 *)(s_cls + 4 * w) = mk_stage4(res, words, p, n_res, MK_PAD_CLASS, [](u32 b) { return rk_class(b); });
        *(u32 *)(s_bnd + 4 * w) = mk_stage4(bound, true, p, n_res, 1u, [](u32 b) { return b; });
    }
    __syncthreads();
    const u32 full = mk_T[W];
    for (u32 w = tid; w < MK_CHUNK / 4; w += MK_THREADS) {
        const u64 p0 = c0 + 4 * (u64)w;
        if (p0 >= n_res) break;
        u32 packed = 0;
#pragma unroll
        for (u32 q = 0; q < 4; q++) {
            const u32 i = 4 * w + q;
            u32 sum = 0, brk = 0;
            for (u32 j = 0; j < W; j++) {
                const u32 cj = s_cls[i + j];
                if (j) brk |= s_bnd[i + j];
                u32 r = 1;
                for (u32 l = 0; l < j; l++) r += s_cls[i + l] == cj ? 1u : 0u;
                sum += s_D[r];
            }
            const u32 e = full - sum;
            const bool valid = brk == 0 && p0 + q + W <= n_res;
            packed |= (valid ? (e <= thr2 ? 1u : 0u) | (e <= thr1 ? 2u : 0u) : 0u) << (8 * q);
        }
        if (p0 + 4 <= cap) *(u32 *)(flags + p0) = packed;
    }
}

KS_DEV bool mk_run_head(const u8 *flags, u64 p) { return (flags[p] & 1u) && (p == 0 || !(flags[p - 1] & 1u)); }

__global__ __launch_bounds__(256) void k_mask_run_heads(const u8 *flags, u64 n_res, u32 *heads) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_res) heads[p] = mk_run_head(flags, p) ? 1u : 0u;
}

// ranks: the scanned heads.  The run of a lo2 start p is ranks[p] + head(p) - 1.
__global__ __launch_bounds__(256) void k_mask_hot(const u8 *flags, const u32 *ranks, u64 n_res, u8 *hot, u64 hot_cap) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_res || (flags[p] & 3u) != 3u) return;
    const u64 run = (u64)ranks[p] + (mk_run_head(flags, p) ? 1u : 0u) - 1u;
    if (run < hot_cap) hot[run] = 1;
}

// `cap`: bytes mask holds (a multiple of 4, >= n_res)
__global__ __launch_bounds__(MK_THREADS) void k_mask_apply(const u8 *flags, const u32 *ranks, const u8 *hot, u64 hot_cap, u64 n_res, u32 W, u8 *mask,
                                                           u64 cap) {
    __shared__ __attribute__((aligned(16))) u8 s_hw[MK_SPAN]; // s_hw[i]: the window that starts at c0 - MK_HALO + i is lo2 and of a hot run
    const u32 tid = threadIdx.x;
    const u64 c0 = (u64)blockIdx.x * MK_CHUNK;
    for (u32 i = tid; i < MK_SPAN; i += MK_THREADS) {
        u32 v = 0;
        if (c0 + i >= MK_HALO && c0 + i - MK_HALO < n_res) {
            const u64 p = c0 + i - MK_HALO;
            if (flags[p] & 1u) {
                const u64 run = (u64)ranks[p] + (mk_run_head(flags, p) ? 1u : 0u) - 1u;
                v = run < hot_cap ? hot[run] : 0u;
            }
        }
        s_hw[i] = (u8)v;
    }
    __syncthreads();
    for (u32 w = tid; w < MK_CHUNK / 4; w += MK_THREADS) {
        const u64 p0 = c0 + 4 * (u64)w;
        if (p0 >= n_res) break;
        u32 packed = 0;
#pragma unroll
        for (u32 q = 0; q < 4; q++) {
            const u32 i = MK_HALO + 4 * w + q; // (i - j >= MK_HALO - (W - 1) >= 1)
            u32 m = 0;
            for (u32 j = 0; j < W; j++) m |= s_hw[i - j];
            packed |= (p0 + q < n_res ? (m & 1u) : 0u) << (8 * q);
        }
        if (p0 + 4 <= cap) *(u32 *)(mask + p0) = packed;
    }
}

// a wave per record: its masked residues; their sum over the batch into *total
__global__ __launch_bounds__(256) void k_mask_counts(const u8 *mask, const u64 *off, u32 n_seqs, u64 n_res, u32 *counts, unsigned long long *total) {
    const u32 s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_seqs) return;
    const u64 a = off[s], e = off[s + 1];
    u64 c = 0;
    if (a <= e && e <= n_res)
        for (u64 p = a + lane; p < e; p += 64) c += mask[p];
    c = ks_wave_sum64(c);
    if (lane == 0) {
        counts[s] = (u32)c;
        if (c) atomicAdd(total, (unsigned long long)c);
    }
}

// ---- split ----
KS_DEV bool mk_seg_head(const u8 *mask, const u8 *bound, u64 p) { return !mask[p] && (p == 0 || bound[p] || mask[p - 1]); }

__global__ __launch_bounds__(256) void k_seg_heads(const u8 *mask, const u8 *bound, u64 n_res, u32 *heads) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_res) heads[p] = mk_seg_head(mask, bound, p) ? 1u : 0u;
}

// the first and the last residue of unmasked stretch i (numbered by the scanned heads) into raw_head[i], raw_tail[i]
__global__ __launch_bounds__(256) void k_seg_ends(const u8 *mask, const u8 *bound, const u32 *ranks, u64 n_res, u32 *raw_head, u32 *raw_tail, u64 raw_cap) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_res || mask[p]) return;
    const bool head = mk_seg_head(mask, bound, p);
    const u64 i = (u64)ranks[p] + (head ? 1u : 0u) - 1u; // (an unmasked residue lies behind a head: never -1 on honest input)
    if (i >= raw_cap) return;
    if (head) raw_head[i] = (u32)p;
    if (p + 1 == n_res || bound[p + 1] || mask[p + 1]) raw_tail[i] = (u32)p;
}

KS_DEV bool mk_seg_kept(const u32 *raw_head, const u32 *raw_tail, u64 i, u64 n_raw, u32 min_len) {
    return i < n_raw && raw_tail[i] >= raw_head[i] && raw_tail[i] - raw_head[i] + 1u >= min_len;
}

__global__ __launch_bounds__(256) void k_seg_keep(const u32 *raw_head, const u32 *raw_tail, const u32 *n_raw, u64 raw_cap, u32 min_len, u32 *keep) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= raw_cap) return;
    const u64 n = *n_raw < raw_cap ? *n_raw : raw_cap;
    keep[i] = mk_seg_kept(raw_head, raw_tail, i, n, min_len) ? 1u : 0u;
}

// kranks: the scanned keep flags.  seg_len was zeroed: entries behind the last kept segment add nothing to the scan that follows.
__global__ __launch_bounds__(256) void k_seg_emit(const u32 *raw_head, const u32 *raw_tail, const u32 *kranks, const u32 *n_raw, u64 raw_cap, u32 min_len,
                                                  const u64 *off, u32 n_seqs, u64 seg_cap, u32 *seg_record, u32 *seg_start, u32 *seg_len) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= raw_cap) return;
    const u64 n = *n_raw < raw_cap ? *n_raw : raw_cap;
    if (!mk_seg_kept(raw_head, raw_tail, i, n, min_len)) return;
    const u64 k = kranks[i];
    if (k >= seg_cap) return;
    const u32 h = raw_head[i], r = ks_last_le_u64(off, 0, n_seqs - 1, h);
    seg_record[k] = r;
    seg_start[k] = (u32)(h - off[r]);
    seg_len[k] = raw_tail[i] - h + 1u;
}

// a wave per kept segment: its residues to their place in the compacted buffer (`cap` bytes)
__global__ __launch_bounds__(256) void k_seg_copy(const u8 *res, const u64 *off, u64 n_res, const u32 *seg_record, const u32 *seg_start, const u64 *seg_off,
                                                  const u32 *n_segs, u64 seg_cap, u8 *out, u64 cap) {
    const u64 k = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63;
    if (k >= seg_cap || k >= *n_segs) return;
    const u64 src = off[seg_record[k]] + seg_start[k], dst = seg_off[k], len = seg_off[k + 1] - dst;
    if (src > n_res || len > n_res - src) return; // (offsets that lie)
    for (u64 j = lane; j < len && dst + j < cap; j += 64) out[dst + j] = res[src + j];
}

// group_offsets[r] = the kept segments of the records below r (seg_record ascends)
__global__ __launch_bounds__(256) void k_seg_groups(const u32 *seg_record, const u32 *n_segs, u64 seg_cap, u32 n_records, u32 *group_offsets) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_records) return;
    const u32 n = (u32)(*n_segs < seg_cap ? *n_segs : seg_cap);
    group_offsets[r] = ks_lower_bound_u32(seg_record, n, r);
}

// one lane per triple of a table made on the segments: back to the record and to positions counted from its first residue
__global__ __launch_bounds__(256) void k_kmerpos_remap(u32 *seq, u32 *start, u64 n, const u32 *seg_record, const u32 *seg_start, u64 n_segs) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 g = seq[i];
    if (g >= n_segs) return;
    seq[i] = seg_record[g];
    start[i] += seg_start[g];
}

// ---- host ----
struct mk_opts { u32 W, k1, k2, thr1, thr2; };

static u32 mk_threshold(u32 k, u32 W) {
    const u64 t = (u64)k * W * 65536ULL / 1000ULL;
    return t > 0xffffffffULL ? 0xffffffffu : (u32)t; // (no window's complexity passes T[32] < 2^24)
}

static int mk_opts_check(ks_ctx *ctx, const char *what, const ks_mask_opts *o, mk_opts *out) {
    mk_opts R{12u, 2200u, 2500u, 0u, 0u};
    if (o && (o->window || o->k1_millibits || o->k2_millibits)) {
        R.W = o->window ? o->window : 12u;
        R.k1 = o->k1_millibits; R.k2 = o->k2_millibits;
    }
    if (R.W < 2 || R.W > KS_MASK_MAX_WINDOW)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s options: window = %u is not in [2, %u]", what, R.W, (unsigned)KS_MASK_MAX_WINDOW);
    if (R.k2 < R.k1) return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s options: k2 = %u millibits is below k1 = %u", what, R.k2, R.k1);
    R.thr1 = mk_threshold(R.k1, R.W); R.thr2 = mk_threshold(R.k2, R.W);
    *out = R;
    return KS_OK;
}

int ks_mask_opts_check(ks_ctx *ctx, const char *what, const ks_mask_opts *opts) { mk_opts O; return mk_opts_check(ctx, what, opts, &O); }

// what every entry point refuses before any device work
static int mk_args_check(ks_ctx *ctx, const char *what, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res) {
    if (!d_offs || (!d_res && n_res)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (n_res >= MK_MAX_RES) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: %llu residues in one batch (at most 2^32 - 65)", what, (unsigned long long)n_res);
    if (n_seqs == 0 && n_res) return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: %llu residues in a batch of 0 records", what, (unsigned long long)n_res);
    return KS_OK;
}

static inline u64 mk_words(u64 n) { return (n + 3) / 4 * 4 + 4; } // bytes of a per-residue byte array the word stores may fill

// The launches of a mask, queued: d_mask (mk_words(n_res) bytes) and d_counts filled, bound (n_res + 1 bytes) left for a split that
// follows, ctl[MK_BAD] and ctl[MK_MASKED] set.  The caller waits and looks at ctl.
static int mask_enqueue(ks_ctx *ctx, ks_scratch &sc, const ks_ctl &ctl, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const mk_opts &O,
                        u8 *d_mask, u32 *d_counts, u8 *bound) {
    KS_HIP(ctx, hipMemsetAsync(bound, 0, (size_t)n_res + 1, ctx->stream));
    if (n_seqs) KS_LAUNCH(ctx, "mask_bounds", k_mask_bounds, (n_seqs + 255) / 256, 256, d_offs, n_seqs, n_res, bound, ctl.words());
    if (n_res == 0) {
        if (n_seqs) KS_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_seqs * sizeof(u32), ctx->stream));
        return KS_OK;
    }
    u8 *flags = nullptr, *hot = nullptr;
    u32 *ranks = nullptr;
    const u64 cap = mk_words(n_res), hot_cap = n_res / 2 + 2; // (two runs are at least one start apart)
    KS_TRY(sc.alloc(&flags, (size_t)cap));
    KS_TRY(sc.alloc(&ranks, (size_t)n_res));
    KS_TRY(sc.alloc(&hot, (size_t)hot_cap));
    KS_HIP(ctx, hipMemsetAsync(hot, 0, (size_t)hot_cap, ctx->stream));
    const u32 chunks = (u32)((n_res + MK_CHUNK - 1) / MK_CHUNK), per_res = (u32)((n_res + 255) / 256);
    if (O.W == 12) KS_LAUNCH(ctx, "mask_flags", k_mask_flags<12>, chunks, MK_THREADS, d_res, (const u8 *)bound, n_res, O.W, O.thr1, O.thr2, flags, cap);
    else KS_LAUNCH(ctx, "mask_flags", k_mask_flags<0>, chunks, MK_THREADS, d_res, (const u8 *)bound, n_res, O.W, O.thr1, O.thr2, flags, cap);
    KS_LAUNCH(ctx, "mask_run_heads", k_mask_run_heads, per_res, 256, (const u8 *)flags, n_res, ranks);
    KS_TRY(ks_scan_u32_inplace(ctx, ranks, n_res, ctl.low32(MK_RUNS)));
    KS_LAUNCH(ctx, "mask_hot", k_mask_hot, per_res, 256, (const u8 *)flags, (const u32 *)ranks, n_res, hot, hot_cap);
    KS_LAUNCH(ctx, "mask_apply", k_mask_apply, chunks, MK_THREADS, (const u8 *)flags, (const u32 *)ranks, (const u8 *)hot, hot_cap, n_res, O.W, d_mask, cap);
    KS_LAUNCH(ctx, "mask_counts", k_mask_counts, (n_seqs + 3) / 4, 256, (const u8 *)d_mask, d_offs, n_seqs, n_res, d_counts, ctl.words() + MK_MASKED);
    return KS_OK;
}

static int mk_fail_offsets(ks_ctx *ctx, const char *what, u64 record) {
    return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: offsets must start at 0, ascend and end at n_residues, a record holds at most 2^32 - 16 residues (record %llu)",
                   what, (unsigned long long)record);
}

// The launches of a split, queued behind a mask of the same batch (d_mask) and its bound bytes: S's five arrays allocated and
// filled, ctl[MK_RAW] and ctl[MK_SEGS] set, *d_total = where the residue count of the segments lies (two 32-bit words).
static int split_enqueue(ks_ctx *ctx, ks_scratch &sc, const ks_ctl &ctl, const u8 *d_mask, const u8 *bound, const u8 *d_res, const u64 *d_offs, u32 n_seqs,
                         u64 n_res, u32 min_len, ks_segments *S, const u64 **d_total) {
    if (min_len == 0) min_len = 1;
    u64 raw_cap = n_res / 2 + n_seqs + 1; // (a stretch begins at a record's first residue or behind a masked residue)
    if (raw_cap > n_res) raw_cap = n_res;
    u64 seg_cap = n_res / min_len;
    if (seg_cap > raw_cap) seg_cap = raw_cap;
    S->n_records = n_seqs; S->min_len = min_len;
    KS_TRY(ks_alloc(ctx, &S->d_seg_record, (size_t)seg_cap));
    KS_TRY(ks_alloc(ctx, &S->d_seg_start, (size_t)seg_cap));
    KS_TRY(ks_alloc(ctx, &S->d_seg_offsets, (size_t)seg_cap + 1));
    KS_TRY(ks_alloc(ctx, &S->d_residues, (size_t)n_res + 16));
    KS_TRY(ks_alloc(ctx, &S->d_group_offsets, (size_t)n_seqs + 1));
    *d_total = S->d_seg_offsets + seg_cap;
    if (n_res == 0 || seg_cap == 0) { // no residue, or none of the records can hold a segment
        KS_HIP(ctx, hipMemsetAsync(S->d_seg_offsets, 0, ((size_t)seg_cap + 1) * sizeof(u64), ctx->stream));
        KS_HIP(ctx, hipMemsetAsync(S->d_group_offsets, 0, ((size_t)n_seqs + 1) * sizeof(u32), ctx->stream));
        return KS_OK;
    }
    u32 *ranks = nullptr, *raw_head = nullptr, *raw_tail = nullptr, *keep = nullptr, *seg_len = nullptr;
    KS_TRY(sc.alloc(&ranks, (size_t)n_res));
    KS_TRY(sc.alloc(&raw_head, (size_t)raw_cap));
    KS_TRY(sc.alloc(&raw_tail, (size_t)raw_cap));
    KS_TRY(sc.alloc(&keep, (size_t)raw_cap));
    KS_TRY(sc.alloc(&seg_len, (size_t)seg_cap));
    KS_HIP(ctx, hipMemsetAsync(raw_head, 0xff, (size_t)raw_cap * sizeof(u32), ctx->stream)); // (head > tail: a stretch nobody wrote is not kept)
    KS_HIP(ctx, hipMemsetAsync(raw_tail, 0, (size_t)raw_cap * sizeof(u32), ctx->stream));
    KS_HIP(ctx, hipMemsetAsync(seg_len, 0, (size_t)seg_cap * sizeof(u32), ctx->stream));
    const u32 per_res = (u32)((n_res + 255) / 256), per_raw = (u32)((raw_cap + 255) / 256);
    const u32 *n_raw = ctl.low32(MK_RAW), *n_segs = ctl.low32(MK_SEGS);
    KS_LAUNCH(ctx, "seg_heads", k_seg_heads, per_res, 256, d_mask, bound, n_res, ranks);
    KS_TRY(ks_scan_u32_inplace(ctx, ranks, n_res, ctl.low32(MK_RAW)));
    KS_LAUNCH(ctx, "seg_ends", k_seg_ends, per_res, 256, d_mask, bound, (const u32 *)ranks, n_res, raw_head, raw_tail, raw_cap);
    KS_LAUNCH(ctx, "seg_keep", k_seg_keep, per_raw, 256, (const u32 *)raw_head, (const u32 *)raw_tail, n_raw, raw_cap, min_len, keep);
    KS_TRY(ks_scan_u32_inplace(ctx, keep, raw_cap, ctl.low32(MK_SEGS)));
    KS_LAUNCH(ctx, "seg_emit", k_seg_emit, per_raw, 256, (const u32 *)raw_head, (const u32 *)raw_tail, (const u32 *)keep, n_raw, raw_cap, min_len, d_offs, n_seqs,
              seg_cap, S->d_seg_record, S->d_seg_start, seg_len);
    KS_TRY(ks_scan_u32_to_u64(ctx, seg_len, S->d_seg_offsets, seg_cap));
    KS_LAUNCH(ctx, "seg_copy", k_seg_copy, (u32)((seg_cap + 3) / 4), 256, d_res, d_offs, n_res, (const u32 *)S->d_seg_record, (const u32 *)S->d_seg_start,
              (const u64 *)S->d_seg_offsets, n_segs, seg_cap, S->d_residues, n_res);
    KS_LAUNCH(ctx, "seg_groups", k_seg_groups, n_seqs / 256 + 1, 256, (const u32 *)S->d_seg_record, n_segs, seg_cap, n_seqs, S->d_group_offsets);
    return KS_OK;
}

// behind the one wait of a call that split: the counts of S from the control block and the fetched residue total
static int split_finish(ks_ctx *ctx, const char *what, const ks_ctl &ctl, const u64 *total, u64 n_res, ks_segments *S) {
    if (ctl.bad(MK_BAD)) return mk_fail_offsets(ctx, what, ctl[MK_BAD]);
    S->n_segs = ctl[MK_SEGS] & 0xffffffffULL;
    S->n_res = *total;
    if (S->n_res > n_res || S->n_segs * S->min_len > S->n_res)
        return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu segments of %llu residues from %llu residues", (unsigned long long)S->n_segs,
                       (unsigned long long)S->n_res, (unsigned long long)n_res);
    return KS_OK;
}

extern "C" uint32_t ks_debug_mask_chunk(void) { return MK_CHUNK; }

int ks_mask_device_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_mask_opts *opts, ks_mask **out) {
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "mask: out is NULL");
    *out = nullptr;
    mk_opts O;
    KS_TRY(mk_opts_check(ctx, "mask", opts, &O));
    KS_TRY(mk_args_check(ctx, "mask", d_res, d_offs, n_seqs, n_res));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_mask> M(ctx, out, ks_mask_free);
    M->n_seqs = n_seqs; M->n_res = n_res; M->window = O.W; M->k1 = O.k1; M->k2 = O.k2;
    KS_TRY(ks_alloc(ctx, &M->d_mask, (size_t)mk_words(n_res)));
    KS_TRY(ks_alloc(ctx, &M->d_counts, (size_t)n_seqs));
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u8 *bound = nullptr;
    KS_TRY(sc.alloc(&bound, (size_t)n_res + 1));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_MASK, 1, MK_CTL_WORDS - 1));
    KS_TRY(mask_enqueue(ctx, sc, ctl, d_res, d_offs, n_seqs, n_res, O, M->d_mask, M->d_counts, bound));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    if (ctl.bad(MK_BAD)) return mk_fail_offsets(ctx, "mask", ctl[MK_BAD]);
    M->n_masked = ctl[MK_MASKED];
    if (M->n_masked > n_res) return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu of %llu residues masked", (unsigned long long)M->n_masked, (unsigned long long)n_res);
    return M.commit();
}

extern "C" int ks_mask_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                              const ks_mask_opts *opts, ks_mask **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_mask_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, opts, out);
    });
}

extern "C" uint32_t ks_mask_n_seqs(const ks_mask *m) { return m ? m->n_seqs : 0; }
extern "C" uint64_t ks_mask_n_residues(const ks_mask *m) { return m ? m->n_res : 0; }
extern "C" uint64_t ks_mask_n_masked(const ks_mask *m) { return m ? m->n_masked : 0; }
extern "C" const uint8_t *ks_mask_device_mask(const ks_mask *m) { return m ? m->d_mask : nullptr; }
extern "C" const uint32_t *ks_mask_device_masked_counts(const ks_mask *m) { return m ? m->d_counts : nullptr; }
extern "C" int ks_mask_copy_to_host(ks_ctx *ctx, const ks_mask *m, uint8_t *mask, uint32_t *masked_counts) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, m, mask, masked_counts); });
}
extern "C" void ks_mask_free(ks_mask *m) { ks_obj_free(m); }

extern "C" int ks_mask_split_device(ks_ctx *ctx, const ks_mask *mask, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                                    uint64_t n_residues, uint32_t min_len, ks_segments **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "mask_split: out is NULL");
    *out = nullptr;
    if (!mask) return ks_fail(ctx, KS_ERR_INVALID_ARG, "mask_split: NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "mask_split", mask));
    KS_TRY(mk_args_check(ctx, "mask_split", d_residues, d_seq_offsets, n_seqs, n_residues));
    if (mask->n_seqs != n_seqs || mask->n_res != n_residues)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "mask_split: the mask was made of %u records and %llu residues, the batch holds %u and %llu", mask->n_seqs,
                       (unsigned long long)mask->n_res, n_seqs, (unsigned long long)n_residues);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_segments> S(ctx, out, ks_segments_free);
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u8 *bound = nullptr;
    const u64 *d_total = nullptr;
    KS_TRY(sc.alloc(&bound, (size_t)n_residues + 1));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_MASK, 1, MK_CTL_WORDS - 1));
    KS_HIP(ctx, hipMemsetAsync(bound, 0, (size_t)n_residues + 1, ctx->stream));
    if (n_seqs) KS_LAUNCH(ctx, "mask_bounds", k_mask_bounds, (n_seqs + 255) / 256, 256, d_seq_offsets, n_seqs, n_residues, bound, ctl.words());
    KS_TRY(split_enqueue(ctx, sc, ctl, mask->d_mask, bound, d_residues, d_seq_offsets, n_seqs, n_residues, min_len, S, &d_total));
    u64 *const total = ctx->h_pin + KS_PIN_MASK + MK_CTL_WORDS;
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(d_total, total, 2)}));
    KS_TRY(split_finish(ctx, "mask_split", ctl, total, n_residues, S));
    return S.commit();
    });
}

extern "C" uint64_t ks_segments_n_segs(const ks_segments *s) { return s ? s->n_segs : 0; }
extern "C" uint64_t ks_segments_n_residues(const ks_segments *s) { return s ? s->n_res : 0; }
extern "C" uint32_t ks_segments_n_records(const ks_segments *s) { return s ? s->n_records : 0; }
extern "C" const uint32_t *ks_segments_device_seg_record(const ks_segments *s) { return s ? s->d_seg_record : nullptr; }
extern "C" const uint32_t *ks_segments_device_seg_start(const ks_segments *s) { return s ? s->d_seg_start : nullptr; }
extern "C" const uint64_t *ks_segments_device_seg_offsets(const ks_segments *s) { return s ? s->d_seg_offsets : nullptr; }
extern "C" const uint8_t *ks_segments_device_residues(const ks_segments *s) { return s ? s->d_residues : nullptr; }
extern "C" const uint32_t *ks_segments_device_group_offsets(const ks_segments *s) { return s ? s->d_group_offsets : nullptr; }
extern "C" int ks_segments_copy_to_host(ks_ctx *ctx, const ks_segments *s, uint32_t *seg_record, uint32_t *seg_start, uint64_t *seg_offsets,
                                        uint8_t *residues, uint32_t *group_offsets) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, s, seg_record, seg_start, seg_offsets, residues, group_offsets); });
}
extern "C" void ks_segments_free(ks_segments *s) { ks_obj_free(s); }

// mask and split of one batch behind ONE wait: the segments at min_len (a ks_segments the caller owns through `S`)
static int masked_segments(ks_ctx *ctx, const char *what, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const mk_opts &O, u32 min_len,
                           ks_segments **out) {
    ks_result<ks_segments> S(ctx, out, ks_segments_free);
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u8 *bound = nullptr, *d_mask = nullptr;
    u32 *d_counts = nullptr;
    const u64 *d_total = nullptr;
    KS_TRY(sc.alloc(&bound, (size_t)n_res + 1));
    KS_TRY(sc.alloc(&d_mask, (size_t)mk_words(n_res)));
    KS_TRY(sc.alloc(&d_counts, (size_t)n_seqs));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_MASK, 1, MK_CTL_WORDS - 1));
    KS_TRY(mask_enqueue(ctx, sc, ctl, d_res, d_offs, n_seqs, n_res, O, d_mask, d_counts, bound));
    KS_TRY(split_enqueue(ctx, sc, ctl, d_mask, bound, d_res, d_offs, n_seqs, n_res, min_len, S, &d_total));
    u64 *const total = ctx->h_pin + KS_PIN_MASK + MK_CTL_WORDS;
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(d_total, total, 2)}));
    KS_TRY(split_finish(ctx, what, ctl, total, n_res, S));
    return S.commit();
}

struct mk_seg_owner { ks_segments *s = nullptr; ~mk_seg_owner() { ks_segments_free(s); } };

int ks_sketch_masked_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, u32 max_seq_len, const ks_params *p,
                          const ks_mask_opts *opts, ks_sketches **out) {
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketch_masked: out is NULL");
    *out = nullptr;
    KS_TRY(ks_check_params(ctx, p));
    mk_opts O;
    KS_TRY(mk_opts_check(ctx, "sketch_masked", opts, &O));
    KS_TRY(mk_args_check(ctx, "sketch_masked", d_res, d_offs, n_seqs, n_res));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    mk_seg_owner G;
    KS_TRY(masked_segments(ctx, "sketch_masked", d_res, d_offs, n_seqs, n_res, O, p->ksize, &G.s));
    // The union takes the group offsets on the host: n_seqs + 1 words, too many for the pinned slots.  Their copy is queued here and
    // rides on the wait the sketch of the segments makes anyway (ks_sketch_device_impl without deferral always waits for the
    // stream before it returns): no wait of its own.
    std::vector<u32> groups((size_t)n_seqs + 1);
    KS_HIP(ctx, hipMemcpyAsync(groups.data(), G.s->d_group_offsets, groups.size() * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    // the sketch of the segments lives until the union has read it
    struct sk_owner { ks_sketches *s = nullptr; ~sk_owner() { ks_sketches_free(s); } } parts;
    const int st = ks_sketch_device_impl(ctx, G.s->d_residues, G.s->d_seg_offsets, (u32)G.s->n_segs, G.s->n_res, max_seq_len, p, 0, 0, 0, &parts.s);
    if (st != KS_OK) { // (it may have failed before its wait: the copy must not outlive `groups`)
        (void)hipStreamSynchronize(ctx->stream);
        return st;
    }
    if (groups[0] != 0 || groups[n_seqs] != (u32)G.s->n_segs)
        return ks_fail(ctx, KS_ERR_HIP, "internal error: the records own %u of %llu segments", groups[n_seqs], (unsigned long long)G.s->n_segs);
    return ks_union_groups_impl(ctx, parts.s, groups.data(), n_seqs, out);
}

extern "C" int ks_sketch_masked_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                                       uint32_t max_seq_len, const ks_params *params, const ks_mask_opts *opts, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_sketch_masked_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, params, opts, out);
    });
}

int ks_kmerpos_masked_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_params *p, const ks_mask_opts *opts,
                           ks_kmerpos **out) {
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "kmer_positions_masked: out is NULL");
    *out = nullptr;
    KS_TRY(ks_check_params(ctx, p));
    mk_opts O;
    KS_TRY(mk_opts_check(ctx, "kmer_positions_masked", opts, &O));
    KS_TRY(mk_args_check(ctx, "kmer_positions_masked", d_res, d_offs, n_seqs, n_res));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    mk_seg_owner G;
    KS_TRY(masked_segments(ctx, "kmer_positions_masked", d_res, d_offs, n_seqs, n_res, O, p->ksize, &G.s));
    struct kp_owner { ks_kmerpos *k = nullptr; ~kp_owner() { ks_kmerpos_free(k); } } K;
    KS_TRY(ks_kmerpos_device_impl(ctx, G.s->d_residues, G.s->d_seg_offsets, (u32)G.s->n_segs, G.s->n_res, p, &K.k));
    if (K.k->n) {
        KS_LAUNCH(ctx, "kmerpos_remap", k_kmerpos_remap, (u32)((K.k->n + 255) / 256), 256, K.k->d_seq, K.k->d_start, K.k->n, (const u32 *)G.s->d_seg_record,
                  (const u32 *)G.s->d_seg_start, G.s->n_segs);
        KS_TRY(ks_stream_wait(ctx)); // (the segments go back to the pool when this scope ends)
    }
    K.k->n_seqs = n_seqs;
    *out = K.k; K.k = nullptr;
    return KS_OK;
}

extern "C" int ks_kmer_positions_masked_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                                               uint64_t n_residues, const ks_params *params, const ks_mask_opts *opts, ks_kmerpos **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_kmerpos_masked_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, params, opts, out);
    });
}
