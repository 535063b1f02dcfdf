// ks_sketch_long.hip — the rare path of a sketch call (ks_sketch.hip): sequences longer than a tile.
//   * k_sketch_long: the tile kernel's algorithm (hash, bucket, order inside the bucket, unique + count) with its arrays in a
//     global scratch slab instead of LDS, one workgroup per sequence, staged and hashed with the tile kit (ks_tile.h).  It
//     runs BEFORE the shared tiles, into side buffers: the tiles' look-back needs the sequence's kept count to leave its slot.
//   * k_place_long: once the shared tiles have fixed the CSR, the runs of the deferred sequences — the long ones and the
//     "medium" ones, which a tile of their own sketched into the same side buffers — are copied into their slots.
#include "ks_tile.h"

struct sk_long_args {
    sk_args a;
    const u32 *long_ids;
    const u32 *n_long;
    u32 long_cap;  // allocated entries of long_ids
    u32 max_len;   // slab sizing
    u64 *slab_keys; // [grid][max_len]   window-order hashes (0 = dropped)
    u64 *slab_tmp;  // [grid][max_len]   bucket-ordered hashes
    u64 *slab_sorted; // [grid][max_len]
    u32 *slab_cnt;  // [grid][max_len+1] bucket counts -> starts
    u32 *slab_ord;  // [grid][max_len]   arrival slot per window
    u32 *slab_flag; // [grid][max_len+1] representative flags -> distinct ranks
    u32 *slab_ab;   // [grid][max_len]
    u64 *lg_hash;   // [n_res] output of long sequences (own buffer: a tile-packed run may overlap a long span)
    u32 *lg_abund;  // [n_res]
};

// block-wide exclusive scan of a global u32 array in place; returns the total (uniform)
KS_DEV u32 sk_block_scan_global(u32 *a, u32 n, u32 *scan_smem) {
    u32 carry = 0;
    for (u32 base = 0; base < n; base += SK_THREADS) {
        u32 i = base + threadIdx.x;
        u32 v = i < n ? a[i] : 0;
        u32 total;
        u32 ex = ks_block_excl_scan(v, scan_smem, &total);
        if (i < n) a[i] = carry + ex;
        carry += total;
    }
    return carry;
}

// All cross-thread traffic goes through global memory inside ONE workgroup: barriers carry
// agent-scope fences so L1-resident lines written by atomics / other waves are re-read (rare path).
#define SK_LONG_SYNC() do { __threadfence(); __syncthreads(); } while (0)

__global__ __launch_bounds__(SK_THREADS) void k_sketch_long(sk_long_args L) {
    __shared__ __attribute__((aligned(16))) u64 res_w[(SK_TILE + SK_PAD) / 8];
    __shared__ u32 scan_smem[SK_THREADS / 64 + 1];
    __shared__ u8 lut_s[256];
    const sk_args &A = L.a;
    const u32 tid = threadIdx.x;
    u8 *res_b = (u8 *)res_w;
    if (tid < 256) lut_s[tid] = A.lut[tid];
    const u32 n_long = L.n_long[1] < L.long_cap ? L.n_long[1] : L.long_cap;
    const u64 slab = (u64)blockIdx.x * ((u64)L.max_len + 1);
    u64 *keys = L.slab_keys + slab, *tmp = L.slab_tmp + slab, *sorted = L.slab_sorted + slab;
    u32 *cnt = L.slab_cnt + slab, *ord = L.slab_ord + slab, *flag = L.slab_flag + slab, *abd = L.slab_ab + slab;

    for (u32 li = blockIdx.x; li < n_long; li += gridDim.x) {
        const u32 s = L.long_ids[li];
        const u64 b = A.offs[s], e = A.offs[s + 1];
        if (e - b > L.max_len) { // the caller's max_seq_len hint was too small: the host reports it (real maximum != hint)
            if (tid == 0) { A.counts[s] = 0; A.kept[s] = 0; }
            continue;
        }
        const u32 len = (u32)(e - b);
        const u32 nw = len >= A.k ? len - A.k + 1 : 0;
        const u32 mul = sk_bucket_mul(nw, A.sfix);
        for (u32 i = tid; i <= nw; i += SK_THREADS) { cnt[i] = 0; flag[i] = 0; }
        SK_LONG_SYNC();
        // hash in chunks of SK_TILE windows staged through LDS
        for (u32 w0 = 0; w0 < nw; w0 += SK_TILE) {
            const u64 gbase = b + w0;
            const u64 g0 = gbase & ~15ULL;
            const u32 shift = (u32)(gbase - g0);
            for (u32 c = tid; c < (SK_TILE + SK_PAD) / 16; c += SK_THREADS) {
                const u64 g = g0 + (u64)c * 16;
                *(uint4 *)(res_b + (size_t)c * 16) = g < e ? sk_encode16(sk_load16(A.res, A.n_res, g), lut_s, false) : make_uint4(0, 0, 0, 0);
            }
            __syncthreads();
            // window w = w0 + j lives at LDS byte shift + j; j strided over threads
            for (u32 j = tid; j < SK_TILE && w0 + j < nw; j += SK_THREADS) {
                const u32 pos = shift + j;
                const u64 *w = res_w + (pos >> 3);
                const u64 h = sk_hash_window_rt(w, pos & 7, A.k, A.seed);
                const bool keep = h != 0 && h <= A.max_hash;
                keys[w0 + j] = keep ? h : 0;
                if (keep) ord[w0 + j] = atomicAdd(&cnt[__umulhi((u32)(h >> 32), mul)], 1u);
            }
            __syncthreads();
        }
        SK_LONG_SYNC();
        const u32 n_kept = sk_block_scan_global(cnt, nw + 1, scan_smem);
        SK_LONG_SYNC();
        for (u32 w = tid; w < nw; w += SK_THREADS) {
            u64 h = keys[w];
            if (h) tmp[cnt[__umulhi((u32)(h >> 32), mul)] + ord[w]] = h;
        }
        SK_LONG_SYNC();
        for (u32 w = tid; w < nw; w += SK_THREADS) {
            u64 h = keys[w];
            if (!h) continue;
            const u32 bk = __umulhi((u32)(h >> 32), mul), o = ord[w];
            const u32 sb = cnt[bk], c = cnt[bk + 1] - sb;
            u32 less = 0, eq = 0, eqb = 0;
            for (u32 j = 0; j < c; j++) {
                u64 x = tmp[sb + j];
                less += x < h;
                eq += x == h;
                eqb += (x == h) & (j < o);
            }
            if (eqb == 0) {
                const u32 p = sb + less;
                sorted[p] = h;
                abd[p] = eq;
                flag[p] = 1;
            }
        }
        SK_LONG_SYNC();
        const u32 n_distinct = sk_block_scan_global(flag, n_kept + 1, scan_smem);
        SK_LONG_SYNC();
        for (u32 p = tid; p < n_kept; p += SK_THREADS) {
            if (flag[p + 1] != flag[p]) {
                L.lg_hash[b + flag[p]] = sorted[p];
                L.lg_abund[b + flag[p]] = abd[p];
            }
        }
        if (tid == 0) {
            A.counts[s] = n_distinct; A.kept[s] = n_kept;
            if (n_kept != n_distinct) atomicAdd((unsigned long long *)A.drops_out, (unsigned long long)(n_kept - n_distinct));
        }
        SK_LONG_SYNC();
    }
}

// slab: 3 u64 + 4 u32 arrays of (max_len + 1) per workgroup, capped at ~2 GiB total
int ks_sketch_long_launch(ks_ctx *ctx, const sk_args &A, const ks_deferred &D, u64 n_long, u32 max_len, ks_scratch &sc) {
    const u64 stride = (u64)max_len + 1;
    const u64 per_wg = stride * (3 * 8 + 4 * 4);
    u64 grid = (2ULL << 30) / per_wg;
    if (grid < 1) grid = 1;
    if (grid > n_long) grid = n_long;
    if (grid > 512) grid = 512;
    u64 *slab64 = nullptr;
    u32 *slab32 = nullptr;
    KS_TRY(sc.alloc(&slab64, (size_t)(grid * stride * 3)));
    KS_TRY(sc.alloc(&slab32, (size_t)(grid * stride * 4)));
    sk_long_args L;
    L.a = A; L.long_ids = D.long_ids; L.n_long = D.n_cls; L.long_cap = (u32)n_long; L.max_len = max_len;
    L.slab_keys = slab64; L.slab_tmp = slab64 + grid * stride; L.slab_sorted = slab64 + 2 * grid * stride;
    L.slab_cnt = slab32; L.slab_ord = slab32 + grid * stride; L.slab_flag = slab32 + 2 * grid * stride;
    L.slab_ab = slab32 + 3 * grid * stride;
    L.lg_hash = D.lg_hash; L.lg_abund = D.lg_abund;
    KS_LAUNCH(ctx, "sketch_long", k_sketch_long, (u32)grid, SK_THREADS, L);
    return KS_OK;
}

// ---------------------------------------------------------------------------------------------
// CSR assembly: only medium / long sequences need a copy (their runs were produced in side buffers
// before the tile kernel fixed their CSR positions); one workgroup per such sequence.
// A: the shared tiles' launch (the batch, the final arrays and their capacity, the status word, the posting regions).
// with_postings: also emit the sequences' postings (the long ones; a medium tile has emitted its own).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_place_long(const sk_args A, const u32 *ids, const u32 *n_ids_dev, u32 ids_cap, const u64 *lg_hash,
                                                    const u32 *lg_abund, const u64 *csr, bool with_postings) {
    // a compacting tile that overflowed wrote no CSR offsets for its sequences (the host repeats the batch): nothing
    // here may be trusted then
    if (__hip_atomic_load(&A.ticket[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4u) return;
    const u32 n_ids = *n_ids_dev < ids_cap ? *n_ids_dev : ids_cap; // (only known on the device: a fixed grid strides over the list)
    for (u32 li = blockIdx.x; li < n_ids; li += gridDim.x) {
    const u32 s = ids[li];
    const u64 dst = csr[s], src = A.offs[s];
    u64 n = A.counts[s]; // (distinct hashes: the head of the sequence's slot)
    if (n > A.offs[s + 1] - src) n = A.offs[s + 1] - src; // (a run is never longer than its sequence)
    for (u64 i = threadIdx.x; i < n; i += 256) {
        const u64 h = lg_hash[src + i];
        if (dst + i < A.out_cap) {
            A.out_hash[dst + i] = h;
            A.out_abund[dst + i] = lg_abund[src + i];
        }
        if (with_postings) { // long sequences are rare: one device atomic per posting is fine here
            const u32 dg = ((ks_join_prefix(h, A.part_K) & A.part_mask) << A.part_sub_shift) | (blockIdx.x & ((1u << A.part_sub_shift) - 1u));
            const u64 slot = atomicAdd(&A.part_cursor[dg], 1u);
            if (slot < A.part_cap) {
                if (A.part_s) {
                    A.part_keys[(u64)dg * A.part_cap + slot] = (h & ~(0xffULL << A.part_s)) | ((u64)(s & 0xffu) << A.part_s);
                    ((u16 *)A.part_vals)[(u64)dg * A.part_cap + slot] = (u16)(s >> 8);
                } else {
                    A.part_keys[(u64)dg * A.part_cap + slot] = h;
                    A.part_vals[(u64)dg * A.part_cap + slot] = s;
                }
            } else {
                atomicOr(&A.ticket[1], 2u);
            }
        }
    }
    }
}

// medium runs: copy only (their tiles emitted their own postings); long runs: with their postings, if the call makes any
int ks_sketch_place_launch(ks_ctx *ctx, const sk_args &A, const ks_deferred &D, u64 n_med, u64 n_long) {
    if (n_med > 0)
        KS_LAUNCH(ctx, "place_long", k_place_long, (u32)(n_med < 1024 ? n_med : 1024), 256, A, (const u32 *)D.med_ids, (const u32 *)D.n_cls,
                  (u32)n_med, (const u64 *)D.lg_hash, (const u32 *)D.lg_abund, (const u64 *)A.csr, false);
    if (n_long > 0)
        KS_LAUNCH(ctx, "place_long", k_place_long, (u32)(n_long < 1024 ? n_long : 1024), 256, A, (const u32 *)D.long_ids,
                  (const u32 *)(D.n_cls + 1), (u32)n_long, (const u64 *)D.lg_hash, (const u32 *)D.lg_abund, (const u64 *)A.csr,
                  A.part_keys != nullptr);
    return KS_OK;
}
