// ks_kmerpos.hip — k-mer position table (ProteomeIndex::process_kmers, src/rust/index.rs:749-786; KmerInfo of kmer.rs:6-12):
// (sequence, start, hash) of every kept window, ordered by (sequence, start), in ONE pass.
// A tile is a fixed range of KP_R residue positions (windows of any sequence: there is no per-sequence sort here, so
// no deferral): residues staged through the LUT and 8 windows hashed per thread from LDS with the tile kit (ks_tile.h), kept
// windows compacted in position order, and the tile's slice of the output found by the same decoupled look-back
// (ticket-ordered tiles, 8-byte {flag, value} status words; ks_device.h) the sketch kernel uses for its CSR.
// Not fused into the sketch's tile kernel on purpose: that kernel is instruction-bound at its register limit (78 of 80
// VGPRs), and this one re-hashes at the rate the 16 B per window of output allow anyway.
#include "ks_tile.h"

#define KP_R SK_TILE
struct kp_args {
    const u8 *res;
    const u64 *offs;
    const u8 *lut;
    const u32 *tile_first;          // first sequence whose END lies beyond the tile's first position
    unsigned long long *tile_status;
    u32 *ticket;                    // [0] tile ids, [1] look-back gave up
    u64 *total;                     // kept windows of the whole batch (written by the last tile)
    u32 *out_seq, *out_start;
    u64 *out_hash;
    u64 n_res, max_hash, seed;
    u32 n_seqs, k, n_tiles;
    u32 use_ticket;                 // tile ids from the atomic ticket (1) or from blockIdx.x (0), as sk_args::use_ticket (ks_tile.h)
};

__global__ __launch_bounds__(256) void k_kmerpos_plan(const u64 *offs, u32 n_seqs, u32 n_tiles, u32 *tile_first) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    // first s with offs[s + 1] > t * KP_R
    tile_first[t] = ks_lower_bound_u64(offs + 1, n_seqs, (u64)t * KP_R + 1);
}

__global__ __launch_bounds__(SK_THREADS) void k_kmerpos_tiles(kp_args A) {
    __shared__ __attribute__((aligned(16))) u64 res_w[(SK_TILE + SK_PAD) / 8];
    __shared__ __attribute__((aligned(16))) u64 stage[SK_TILE]; // compacted output staging: hashes, then (seq, start)
    __shared__ u32 lend[SK_SEQ_CAP + 2]; // local END of the tile's sequences (clamped)
    __shared__ u8 lut_s[256];
    __shared__ u32 scan_smem[SK_THREADS / 64 + 1];
    __shared__ u32 tile_s;
    __shared__ unsigned long long base_s;
    const u32 tid = threadIdx.x;
    constexpr u32 NCH = (SK_TILE + SK_PAD) / 16;
    // (tile ids in dispatch order; a launch whose look-back gave up is repeated with ticket ids: 73k tickets on one address
    // were 0.9 ms of queueing for a 1M-protein batch)
    u32 tile = blockIdx.x;
    if (A.use_ticket) { // (uniform; the repeat launch only)
        if (tid == 0) tile_s = atomicAdd(&A.ticket[0], 1u);
        __syncthreads();
        tile = tile_s;
    }
    // the encode table's byte, the tile's residues and its sequence range are requested together (the table byte used to be
    // stored — i.e. waited for — before anything else was asked for: see sk_load16, ks_tile.h)
    u32 lut_v = 0;
    if (tid < 256) lut_v = A.lut[tid];
    const u64 g0 = (u64)tile * KP_R;
    uint4 rv = make_uint4(0, 0, 0, 0);
    if (tid < NCH) rv = sk_load16(A.res, A.n_res, g0 + (u64)tid * 16);
    const u32 s_first = A.tile_first[tile];
    u32 s_last = A.tile_first[tile + 1]; // the sequence that holds the next tile's first position also ends here or later
    if (s_last >= A.n_seqs) s_last = A.n_seqs ? A.n_seqs - 1 : 0;
    const u32 ns = s_first < A.n_seqs ? s_last - s_first + 1 : 0;
    const bool in_lds = ns <= SK_SEQ_CAP;
    if (in_lds)
        for (u32 i = tid; i < ns; i += SK_THREADS) {
            const u64 v = A.offs[s_first + i + 1] - g0; // ends beyond the tile's first position: never negative
            lend[i] = v > 0x7fffffffULL ? 0x7fffffffu : (u32)v;
        }
    if (tid < 256) lut_s[tid] = (u8)lut_v;
    __syncthreads(); // the table
    if (tid < NCH) *(uint4 *)((u8 *)res_w + (size_t)tid * 16) = sk_encode16(rv, lut_s, false);
    __syncthreads();
    auto end_of = [&](u32 s) -> u32 { // local end of sequence s (s_first <= s <= s_last)
        if (in_lds) return lend[s - s_first];
        const u64 v = A.offs[s + 1] - g0;
        return v > 0x7fffffffULL ? 0x7fffffffu : (u32)v;
    };

    const u32 q0 = tid * SK_E;
    u64 h[SK_E];
    u32 sq[SK_E]; // sequence of a kept window, ~0 = not kept
    u32 n_keep = 0;
#pragma unroll
    for (int i = 0; i < SK_E; i++) { h[i] = 0; sq[i] = 0xffffffffu; }
    if (ns && g0 + q0 < A.n_res) {
        // the sequence that holds position q0: first one (from s_first) whose end lies beyond q0
        u32 s = sk_seq_beyond(s_first, s_last, q0, end_of), e = end_of(s); // (s_last is inclusive: the answer when no earlier one is)
        const u64 *wl = res_w + tid;
        sk_hash_windows<0, SK_E>(h, wl, A.k, A.seed);
#pragma unroll
        for (int i = 0; i < SK_E; i++) {
            const u32 p = q0 + i;
            while (s < s_last && p >= e) { s++; e = end_of(s); }
            // offsets are cumulative, so p lies inside sequence s as soon as p < e; the window must fit before e
            const bool keep = p < e && p + A.k <= e && h[i] != 0 && h[i] <= A.max_hash;
            if (keep) { sq[i] = s; n_keep++; }
        }
    }
    u32 total;
    const u32 ex = ks_block_excl_scan(n_keep, scan_smem, &total);
    // ---- decoupled look-back over the tiles' kept counts (protocol: ks_device.h)
    if (tid == 0)
        __hip_atomic_store(&A.tile_status[tile], (tile == 0 ? KS_LB_PRE : KS_LB_AGG) | (u64)total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        u64 excl = 0;
        if (tile > 0) {
            excl = ks_lookback_walk(tile, tid, ks_lookback_words(A.tile_status), &A.ticket[1]);
            if (tid == 0)
                __hip_atomic_store(&A.tile_status[tile], KS_LB_PRE | (excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) {
            base_s = excl;
            if (tile == A.n_tiles - 1) *A.total = excl + total;
        }
    }
    __syncthreads();
    // kept windows leave through LDS in compacted order, so the three output streams are written as whole cache lines
    // (per-thread runs of <= 8 entries would touch 64 different 32-byte sectors per store instruction)
    const u64 base = base_s;
    {
        u32 o = ex;
#pragma unroll
        for (int i = 0; i < SK_E; i++)
            if (sq[i] != 0xffffffffu) stage[o++] = h[i];
    }
    __syncthreads();
    for (u32 i = tid; i < total; i += SK_THREADS) A.out_hash[base + i] = stage[i];
    __syncthreads();
    {
        u32 *st_seq = (u32 *)stage, *st_start = st_seq + SK_TILE;
        u32 o = ex;
#pragma unroll
        for (int i = 0; i < SK_E; i++)
            if (sq[i] != 0xffffffffu) {
                st_seq[o] = sq[i];
                st_start[o] = (u32)(g0 + q0 + i - A.offs[sq[i]]);
                o++;
            }
        __syncthreads();
        for (u32 i = tid; i < total; i += SK_THREADS) {
            A.out_seq[base + i] = st_seq[i];
            A.out_start[base + i] = st_start[i];
        }
    }
}

// d_seq / d_start / d_hash are sized by the batch's window count (an upper bound on the kept windows)
int ks_kmerpos_tiles_launch(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_params *p, u32 *d_seq,
                            u32 *d_start, u64 *d_hash, u64 *n_out) {
    const u64 n_tiles64 = (n_res + KP_R - 1) / KP_R;
    if (n_tiles64 > 0x7ffffff0ULL) return ks_fail(ctx, KS_ERR_INVALID_ARG, "batch too large");
    const u32 n_tiles = (u32)n_tiles64;
    u32 *tile_first = nullptr, *ticket = nullptr;
    unsigned long long *status = nullptr;
    u64 *total = nullptr;
    ks_scratch sc(ctx);
    KS_TRY(sc.alloc(&tile_first, (size_t)n_tiles + 1));
    KS_TRY(sc.alloc((u64 **)&status, (size_t)n_tiles));
    KS_TRY(sc.alloc(&ticket, 2));
    KS_TRY(sc.alloc(&total, 1));
    KS_LAUNCH(ctx, "kmerpos_plan", k_kmerpos_plan, (n_tiles + 256) / 256, 256, d_offs, n_seqs, n_tiles, tile_first);
    u64 *const rb = ctx->h_pin + KS_PIN_READ; // total | ticket pair
    for (int attempt = 0; attempt < 2; attempt++) {
        const bool use_ticket = ctx->sketch_use_ticket || attempt == 1;
        (void)hipMemsetAsync(status, 0, (size_t)n_tiles * sizeof(u64), ctx->stream);
        (void)hipMemsetAsync(ticket, 0, 2 * sizeof(u32), ctx->stream);
        (void)hipMemsetAsync(total, 0, sizeof(u64), ctx->stream);
        kp_args A;
        memset(&A, 0, sizeof A);
        A.res = d_res; A.offs = d_offs; A.lut = ctx->d_lut + 256 * p->moltype; A.tile_first = tile_first;
        A.tile_status = status; A.ticket = ticket; A.total = total; A.out_seq = d_seq; A.out_start = d_start; A.out_hash = d_hash;
        A.n_res = n_res; A.max_hash = ks_max_hash(p->scaled); A.seed = p->seed; A.n_seqs = n_seqs; A.k = p->ksize; A.n_tiles = n_tiles;
        A.use_ticket = use_ticket ? 1u : 0u;
        KS_LAUNCH(ctx, "kmerpos_tiles", k_kmerpos_tiles, n_tiles, SK_THREADS, A);
        KS_HIP(ctx, hipMemcpyAsync(rb, total, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        KS_HIP(ctx, hipMemcpyAsync(rb + 1, ticket, 2 * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool gave_up = ((u32 *)(rb + 1))[1] != 0;
        if (!use_ticket && ks_dbg(ctx, KS_DBG_FORCE_TICKET_RETRY)) gave_up = true; // exercises the repeat
        if (!gave_up) { *n_out = rb[0]; break; }
        if (use_ticket) return ks_fail(ctx, KS_ERR_HIP, "k-mer positions: look-back gave up waiting for a predecessor tile");
        ctx->sketch_use_ticket = true; // dispatch order did not hold here: tickets from now on (shared with the sketch tiles)
        ctx->sketch_ticket_fallbacks++;
    }
    return KS_OK;
}
