// ks_rcull.hip — ks_regions_cull_device: per hit row the regions (alignments, extended regions) that no better region of the
// row covers (include/kmerseek_amd.h has the contract).  A pass over extents and scores: 28 bytes per region, no residues, all
// of it in 64-bit integers.  Bound by latency and lane use, not by memory.
//
//   plan    k_rc_plan, a thread per hit row and per region: row_offsets is checked — 0 first, n_regions last, never
//           descending — before anything is indexed by it (a row that breaks it is named and taken by no kernel: every row a
//           kernel sees lies inside [0, n_regions)), and a region with a length of 0 is named.  Rows of 0 and 1 regions are
//           settled here; every other row goes onto one of three segment lists as (row, regions), by length, with one atomic
//           per workgroup and list (ks_seg_list_push_block):
//   lanes   k_rc_lanes<8>: 2 .. 8 regions, a group of 8 lanes per row, 8 rows per wave; k_rc_lanes<64>: 9 .. 64 regions, a wave
//           per row.  One program: a lane holds a region; its priority rank is the number of lanes that beat it (all pairs,
//           width-W shuffles / v_readlane); the greedy loop runs over the ranks: the lane of rank p, if still undecided, is
//           kept (or dropped once the row keeps max_per_row) and broadcasts its extents, the undecided lanes test `covers` and
//           record it as their keeper.  rank = the kept regions before it, n_merged = 1 + the bits of that step's ballot.
//   wg      k_rc_wg, a workgroup of 256 threads per row: rank by counting over the row's scores, order[rank] = region, then the
//           same loop: decided regions are skipped without a barrier (every thread reads the same word), a kept candidate costs
//           two barriers and one sweep of the row by all threads.  A row of up to RC_LDS_ROWS regions is staged in LDS (32 bytes
//           per region: 32 KiB); a longer one runs the SAME function on the input columns and two u32 per region of global
//           scratch — O(len^2 / 256) score reads for the ranks, O(len * kept / 256) extent reads for the loop, from L2.
//           n_merged comes from integer atomic adds on the keepers (a zeroed column): any order gives the same count.
//   emit    the keep flags -> one-launch exclusive scan -> src_region, rank, n_merged of the kept regions and the result's
//           row_offsets (the scan at the input's row_offsets).
// Every decision compares (i64 score, input index) and 64-bit products of u32 extents: the result does not depend on the path
// a row took (KS_DEBUG_CULL_PATH = 1 every row of <= 64 regions by a wave, 2 every row by a workgroup, 3 as 2 with
// RC_LDS_ROWS_SMALL so that small rows take the global path) or on the launch geometry.  One host wait.
#include "ks_rkit.h"

#define RC_THREADS 256
#define RC_PLAN_THREADS 1024 // k_rc_plan: one atomic per workgroup and list
#define RC_GROUP 8          // lanes of a group of k_rc_lanes<8>
#ifndef RC_GROUP_MAX
#define RC_GROUP_MAX RC_GROUP // the longest row k_rc_lanes<8> takes (a variant build with 1 sends every short row to a wave: DESIGN 3.3m)
#endif
static_assert(RC_GROUP_MAX <= RC_GROUP, "a group holds a row");
#define RC_LDS_ROWS 1024    // regions of a row k_rc_wg stages in LDS (32 bytes each)
#define RC_LDS_ROWS_SMALL 32 // ... under KS_DEBUG_CULL_PATH = 3
#define RC_LANES_GRID 1024  // workgroups of k_rc_lanes (4 waves each, striding over the listed rows)
#define RC_WG_GRID 2048     // workgroups of k_rc_wg (striding likewise)
#define RC_NONE KS_RCULL_NONE
enum : u32 { RC_BAD_CSR = 0, RC_BAD_LEN = 1, RC_N_BAD = 2 };
enum : u32 { RC_UND = 0, RC_KEPT = 1, RC_REMOVED = 2, RC_DROPPED = 3, RC_OFF = 4 }; // a region's state; RC_OFF: a lane without one

struct rc_in {
    const u64 *row_offs;
    const u32 *qs, *ql, *ts, *tl;
    const i64 *score;
    u32 n_rows, n;
    u32 P, N; // overlap_pct in [1, 100]; max_per_row, 0: no limit
    u32 use_min;
    i64 min_score;
};
struct rc_out {
    u32 *keeper, *flag, *rank, *nm; // per input region; flag: kept; rank and nm are read only where flag is set
    double *best;                   // per row
};

// region k covers region g: the overlap is at least P percent of g on both sequences (ends in u64: start + length may be 2^32)
KS_DEV bool rc_covers(u32 P, u32 kqs, u32 kql, u32 kts, u32 ktl, u32 gqs, u32 gql, u32 gts, u32 gtl) {
    const u64 kqe = (u64)kqs + kql, gqe = (u64)gqs + gql, kte = (u64)kts + ktl, gte = (u64)gts + gtl;
    const u64 qlo = kqs > gqs ? kqs : gqs, qhi = kqe < gqe ? kqe : gqe, tlo = kts > gts ? kts : gts, thi = kte < gte ? kte : gte;
    const u64 ovq = qhi > qlo ? qhi - qlo : 0, ovt = thi > tlo ? thi - tlo : 0; // (<= 2^32: the products below fit 64 bits)
    return ovq * 100u >= (u64)P * gql && ovt * 100u >= (u64)P * gtl;
}
// score si at input index i comes before score sj at index j
KS_DEV u32 rc_before(i64 si, u32 i, i64 sj, u32 j) { return (si > sj || (si == sj && i < j)) ? 1u : 0u; }

// mode: 0 by length, 1 every row of <= 64 regions to k_rc_lanes<64>, 2 every row to k_rc_wg.  (No thread leaves early: the
// pushes are the workgroup's.)
__global__ __launch_bounds__(RC_PLAN_THREADS) void k_rc_plan(rc_in I, int mode, u32 *seg8, u32 *seg64, u32 *segwg, rc_out O, unsigned long long *bad) {
    __shared__ u32 s_push[2];
    const u64 i = (u64)blockIdx.x * RC_PLAN_THREADS + threadIdx.x;
    if (i < I.n && (I.ql[i] == 0 || I.tl[i] == 0)) ks_first_bad(bad, RC_BAD_LEN, (u32)i);
    const u32 r = (u32)i;
    u32 len = 0, to = 0; // the list the row goes onto: 1 seg8, 2 seg64, 3 segwg, 0 none
    if (i < I.n_rows) {
        const u64 b = I.row_offs[r], e = I.row_offs[r + 1];
        if ((r == 0 && b != 0) || b > e || e > I.n || (r == I.n_rows - 1 && e != I.n)) ks_first_bad(bad, RC_BAD_CSR, r);
        else if (e == b) O.best[r] = ks_nan();
        else if (e - b == 1 && mode == 0) { // [b, e) lies inside [0, n)
            const i64 s = I.score[b];
            const bool keep = !(I.use_min && s < I.min_score); // (max_per_row >= 1 where it limits at all)
            O.keeper[b] = keep ? (u32)b : RC_NONE; O.flag[b] = keep ? 1u : 0u; O.rank[b] = 0u; O.nm[b] = 1u;
            O.best[r] = keep ? (double)s : ks_nan();
        } else {
            len = (u32)(e - b);
            to = mode == 2 || len > 64 ? 3u : (mode == 1 || len > RC_GROUP_MAX) ? 2u : 1u;
        }
    }
    ks_seg_list_push_block(seg8, I.n_rows, to == 1u, r, len, s_push);
    ks_seg_list_push_block(seg64, I.n_rows, to == 2u, r, len, s_push);
    ks_seg_list_push_block(segwg, I.n_rows, to == 3u, r, len, s_push);
}

// lane j's value inside the group of W lanes (W == 64, j wave-uniform: v_readlane; else a width-W shuffle)
template <u32 W> KS_DEV u32 rc_from(u32 v, u32 j) {
    if constexpr (W == 64) return (u32)__builtin_amdgcn_readlane((int)v, (int)ks_readfirst(j));
    else return (u32)__shfl((int)v, (int)j, (int)W);
}

// A group of W lanes per listed row, 64 / W rows per wave (all 64 lanes run every step: the ballots and shuffles see whole
// waves; a group without a row, or past its row's ranks, decides nothing).
template <u32 W> __global__ __launch_bounds__(RC_THREADS) void k_rc_lanes(rc_in I, const u32 *segs, rc_out O) {
    constexpr u32 G = 64 / W;
    const u32 lane = threadIdx.x & 63, sub = lane % W, gsh = (lane / W) * W;
    const u64 gmask = W == 64 ? ~0ULL : (1ULL << (W & 63)) - 1ULL;
    const u32 n_list = segs[0] < I.n_rows ? segs[0] : I.n_rows;
    const u64 n_waves = (u64)gridDim.x * (RC_THREADS / 64);
    for (u64 w = (u64)blockIdx.x * (RC_THREADS / 64) + (threadIdx.x >> 6); w * G < n_list; w += n_waves) { // (wave-uniform)
        const u64 si = w * G + lane / W;
        u32 r = 0, len = 0;
        u64 b = 0;
        if (si < n_list) {
            r = segs[1 + 2 * si]; len = segs[2 + 2 * si];
            if (r < I.n_rows && len <= W) b = I.row_offs[r]; else len = 0; // (the plan lists nothing else)
        }
        const bool valid = sub < len;
        const u32 g = (u32)(b + sub);
        u32 qs = 0, ql = 1, ts = 0, tl = 1;
        i64 sc = 0;
        if (valid) { qs = I.qs[g]; ql = I.ql[g]; ts = I.ts[g]; tl = I.tl[g]; sc = I.score[g]; }
        u32 rk = 0; // the lanes of the row that come before this one
        for (u32 j = 0; j < W; j++) {
            if (!__ballot(j < len)) break;
            const i64 sj = (i64)(((u64)rc_from<W>((u32)((u64)sc >> 32), j) << 32) | rc_from<W>((u32)(u64)sc, j));
            rk += j < len ? rc_before(sj, j, sc, sub) : 0u;
        }
        u32 state = !valid ? RC_OFF : (I.use_min && sc < I.min_score) ? RC_DROPPED : RC_UND;
        u32 keeper = RC_NONE, krank = 0, nm = 0, nkept = 0;
        for (u32 p = 0; p < W; p++) {
            if (!__ballot(p < len)) break;
            const u64 own = (__ballot(valid && rk == p) >> gsh) & gmask, und = __ballot(state == RC_UND) >> gsh;
            const u32 src = own ? (u32)__ffsll((long long)own) - 1u : 0u; // the lane of rank p
            const bool okept = own && ((und >> src) & 1ULL) && (I.N == 0 || nkept < I.N);
            const u32 kqs = rc_from<W>(qs, src), kql = rc_from<W>(ql, src), kts = rc_from<W>(ts, src), ktl = rc_from<W>(tl, src);
            const bool hit = okept && state == RC_UND && sub != src && rc_covers(I.P, kqs, kql, kts, ktl, qs, ql, ts, tl);
            const u64 hm = (__ballot(hit) >> gsh) & gmask;
            if (hit) { state = RC_REMOVED; keeper = (u32)(b + src); }
            if (okept && sub == src) { state = RC_KEPT; keeper = g; krank = nkept; nm = 1u + (u32)__popcll((long long)hm); }
            if (okept) nkept++;
        }
        if (valid) {
            O.keeper[g] = keeper; O.flag[g] = state == RC_KEPT ? 1u : 0u; O.rank[g] = krank; O.nm[g] = nm;
            if (state == RC_KEPT && krank == 0) O.best[r] = (double)sc;
            if (sub == 0 && nkept == 0) O.best[r] = ks_nan();
        }
    }
}

// One row by the workgroup (all 256 threads enter; everything but the array contents is uniform).  The seven arrays hold the
// row's `len` regions — LDS copies, or the input columns and global scratch at the row's first region.  b: that region.
KS_DEV void rc_wg_row(const rc_in &I, const rc_out &O, u32 r, u32 b, u32 len, const u32 *qs, const u32 *ql, const u32 *ts, const u32 *tl,
                      const i64 *sc, u32 *order, u32 *state) {
    const u32 t = threadIdx.x;
    for (u32 j = t; j < len; j += RC_THREADS) {
        const i64 sj = sc[j];
        u32 cnt = 0;
        for (u32 i = 0; i < len; i++) cnt += rc_before(sc[i], i, sj, j);
        if (cnt < len) order[cnt] = j; // (a permutation: the ranks are distinct)
        state[j] = (I.use_min && sj < I.min_score) ? RC_DROPPED : RC_UND;
    }
    __syncthreads();
    u32 nkept = 0;
    for (u32 p = 0; p < len; p++) {
        const u32 i = order[p];
        if (i >= len || state[i] != RC_UND) continue; // (the same word for every thread, not written since the last barrier)
        if (I.N != 0 && nkept >= I.N) break;
        const u32 kqs = qs[i], kql = ql[i], kts = ts[i], ktl = tl[i];
        __syncthreads(); // every thread has read state[i]
        for (u32 j = t; j < len; j += RC_THREADS) {
            if (j == i) {
                state[j] = RC_KEPT;
                O.keeper[b + j] = b + j; O.rank[b + j] = nkept;
                if (nkept == 0) O.best[r] = (double)sc[j];
            } else if (state[j] == RC_UND && rc_covers(I.P, kqs, kql, kts, ktl, qs[j], ql[j], ts[j], tl[j])) {
                state[j] = RC_REMOVED;
                O.keeper[b + j] = b + i;
            }
        }
        nkept++;
        __syncthreads();
    }
    for (u32 j = t; j < len; j += RC_THREADS) {
        const u32 st = state[j];
        O.flag[b + j] = st == RC_KEPT ? 1u : 0u;
        if (st == RC_KEPT || st == RC_REMOVED) atomicAdd(&O.nm[O.keeper[b + j]], 1u); // (this thread's own store; a keeper of this row)
        else O.keeper[b + j] = RC_NONE;
    }
    if (nkept == 0 && t == 0) O.best[r] = ks_nan();
}

// chunk: the longest row that is staged (<= RC_LDS_ROWS); order / state: one u32 per input region, for the longer rows
__global__ __launch_bounds__(RC_THREADS) void k_rc_wg(rc_in I, const u32 *segs, u32 chunk, u32 *g_order, u32 *g_state, rc_out O) {
    __shared__ u32 s_qs[RC_LDS_ROWS], s_ql[RC_LDS_ROWS], s_ts[RC_LDS_ROWS], s_tl[RC_LDS_ROWS], s_order[RC_LDS_ROWS], s_state[RC_LDS_ROWS];
    __shared__ i64 s_sc[RC_LDS_ROWS];
    for (ks_seg_walk seg = ks_seg_list_by_wg(segs, I.n_rows); seg.next();) {
        const u32 r = seg.b, len = seg.len;
        if (r >= I.n_rows) continue;
        const u64 b64 = rk_readfirst64(I.row_offs[r]);
        if (b64 + len > I.n) continue; // (the plan lists nothing else)
        const u32 b = (u32)b64;
        __syncthreads(); // (the previous row's last readers of the staged arrays)
        if (len <= chunk) {
            for (u32 j = threadIdx.x; j < len; j += RC_THREADS) {
                s_qs[j] = I.qs[b + j]; s_ql[j] = I.ql[b + j]; s_ts[j] = I.ts[b + j]; s_tl[j] = I.tl[b + j]; s_sc[j] = I.score[b + j];
            }
            __syncthreads();
            rc_wg_row(I, O, r, b, len, s_qs, s_ql, s_ts, s_tl, s_sc, s_order, s_state);
        } else rc_wg_row(I, O, r, b, len, I.qs + b, I.ql + b, I.ts + b, I.tl + b, I.score + b, g_order + b, g_state + b);
    }
}

// the kept regions to their places, and the result's row_offsets: the kept regions before each row's first region
__global__ __launch_bounds__(RC_THREADS) void k_rc_emit(rc_in I, rc_out O, const u64 *pos, u32 *o_src, u32 *o_rank, u32 *o_nm, u64 *o_offs) {
    const u64 i = (u64)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < I.n && O.flag[i]) {
        const u64 o = pos[i];
        if (o < I.n) { o_src[o] = (u32)i; o_rank[o] = O.rank[i]; o_nm[o] = O.nm[i]; }
    }
    if (i <= I.n_rows) {
        const u64 b = I.row_offs[i];
        o_offs[i] = pos[b < I.n ? b : I.n];
    }
}

int ks_regions_cull_impl(ks_ctx *ctx, const ks_rcull_cols &cols, u64 n_rows, u64 ng, const ks_rcull_opts *o, ks_rcull *K) {
    K->n_rows = n_rows; K->n_regions = ng; K->n_kept = 0;
    KS_TRY(rk_counts_check(ctx, "region cull", n_rows, ng));
    KS_TRY(ks_alloc(ctx, &K->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, K, K->n_rows));
    KS_TRY(ks_obj_alloc(ctx, K, K->n_regions));
    KS_TRY(ks_alloc(ctx, &K->d_src_region, (size_t)ng)); KS_TRY(ks_alloc(ctx, &K->d_rank, (size_t)ng)); KS_TRY(ks_alloc(ctx, &K->d_n_merged, (size_t)ng));
    if (n_rows == 0 || ng == 0) KS_HIP(ctx, hipMemsetAsync(K->d_row_offsets, 0, ((size_t)n_rows + 1) * sizeof(u64), ctx->stream));
    if (n_rows == 0) return ks_stream_wait(ctx); // (ng == 0: the caller has checked)

    bool small; // (tests: every row one way; 3 = the workgroup path with a small LDS capacity)
    const int mode = ks_seg_path_knob(ctx, KS_DBG_CULL_PATH, &small);
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u32 *seg8 = nullptr, *seg64 = nullptr, *segwg = nullptr, *flag = nullptr, *rank = nullptr, *nm = nullptr, *g_order = nullptr, *g_state = nullptr;
    u64 *pos = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RCULL, RC_N_BAD, 0));
    KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &seg8)); KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &seg64));
    KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &segwg));
    KS_TRY(sc.alloc(&flag, (size_t)ng)); KS_TRY(sc.alloc(&rank, (size_t)ng)); KS_TRY(sc.alloc(&nm, (size_t)ng));
    KS_TRY(sc.alloc(&g_order, (size_t)ng)); KS_TRY(sc.alloc(&g_state, (size_t)ng)); KS_TRY(sc.alloc(&pos, (size_t)ng + 1));
    if (ng) KS_HIP(ctx, hipMemsetAsync(nm, 0, (size_t)ng * sizeof(u32), ctx->stream)); // (k_rc_wg counts into it)

    const rc_in I = {cols.row_offs, cols.qs, cols.ql, cols.ts, cols.tl, cols.score, (u32)n_rows, (u32)ng, o->overlap_pct ? o->overlap_pct : 100u,
                     o->max_per_row, (o->flags & KS_RCULL_MIN_SCORE) ? 1u : 0u, o->min_score};
    const rc_out O = {K->d_keeper, flag, rank, nm, K->d_row_best};
    const u64 n_plan = n_rows > ng ? n_rows : ng;
    KS_LAUNCH(ctx, "rcull_plan", k_rc_plan, (u32)((n_plan + RC_PLAN_THREADS - 1) / RC_PLAN_THREADS), RC_PLAN_THREADS, I, mode, seg8, seg64, segwg, O, ctl.words());
    u64 *const hk = ctx->h_pin + KS_PIN_RCULL + RC_N_BAD;
    *hk = 0;
    if (ng == 0) KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    else {
        if (mode == 0) KS_LAUNCH(ctx, "rcull_lanes8", k_rc_lanes<RC_GROUP>, RC_LANES_GRID, RC_THREADS, I, (const u32 *)seg8, O);
        if (mode != 2) KS_LAUNCH(ctx, "rcull_lanes64", k_rc_lanes<64>, RC_LANES_GRID, RC_THREADS, I, (const u32 *)seg64, O);
        KS_LAUNCH(ctx, "rcull_wg", k_rc_wg, RC_WG_GRID, RC_THREADS, I, (const u32 *)segwg, small ? RC_LDS_ROWS_SMALL : RC_LDS_ROWS, g_order, g_state, O);
        KS_TRY(ks_scan_u32_to_u64(ctx, flag, pos, ng));
        const u64 n_emit = n_rows + 1 > ng ? n_rows + 1 : ng;
        KS_LAUNCH(ctx, "rcull_emit", k_rc_emit, (u32)((n_emit + RC_THREADS - 1) / RC_THREADS), RC_THREADS, I, O, (const u64 *)pos, K->d_src_region,
                  K->d_rank, K->d_n_merged, K->d_row_offsets);
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(pos + ng, hk, 2)}));
    }
    if (ctl.bad(RC_BAD_CSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region cull: row_offsets is not a CSR from 0 to %llu regions that never descends: hit row %llu breaks it",
                       (unsigned long long)ng, (unsigned long long)ctl[RC_BAD_CSR]);
    if (ctl.bad(RC_BAD_LEN))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region cull: region %llu has a length of 0: it covers nothing and nothing covers it",
                       (unsigned long long)ctl[RC_BAD_LEN]);
    K->n_kept = *hk;
    return KS_OK;
}

__global__ __launch_bounds__(RC_THREADS) void k_rc_take(ks_take_cols C, const u32 *src, u64 n, u64 n_src) {
    const u64 i = (u64)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n) return;
    const u32 g = src[i];
    if (g >= n_src) return; // (a cull's own column: never)
    for (u32 c = 0; c < C.n32; c++) C.out[c][i] = C.in[c][g];
    if (C.in64) C.out64[i] = C.in64[g];
}
int ks_rcull_take_launch(ks_ctx *ctx, const ks_rcull *K, const ks_take_cols &cols) {
    if (K->n_kept == 0) return KS_OK;
    KS_LAUNCH(ctx, "rcull_take", k_rc_take, (u32)((K->n_kept + RC_THREADS - 1) / RC_THREADS), RC_THREADS, cols, (const u32 *)K->d_src_region, K->n_kept,
              K->n_regions);
    return KS_OK;
}

extern "C" uint32_t ks_debug_rcull_lds_rows(uint32_t *small_rows) {
    if (small_rows) *small_rows = RC_LDS_ROWS_SMALL;
    return RC_LDS_ROWS;
}
