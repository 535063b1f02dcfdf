// ks_rtrace.hip — ks_regions_traceback: the path of every alignment of a ks_raligns, as a CIGAR (include/kmerseek_amd.h has
// the semantics; ks_regions_traceback_profile: k_rt_trace with the scorer the alignments were made with, ra_by_profile).  The forward program is the one of ks_regions_align — ra_extend<true> of ks_ralign_kit.h, the same row step
// with the counts left out — run again to the end cell the alignment names, writing one direction byte per cell; then a walk
// back from the end cell to (0, 0).  All of it in integers.
//
//   plan     k_rt_plan, a wave per region: rk_locate (ks_rkit.h) and rt_geometry — the one place that decides whether an
//            alignment lies inside its region's sequences, with its anchor inside it and both end cells inside the band —
//            before anything is indexed by them.  Per region the rows of directions it needs and its columns (aln_length); two
//            exclusive scans (ks_prims.hip) lay both out, one wait brings the totals and the first refused region.
//   slices   consecutive regions whose directions fit the scratch budget run in one launch; the launches of a call share one
//            block of the context's pool, in stream order.  A region's slot is rows of RA_DIR_ROW bytes, the right extension's
//            then the left one's, each an even number of rows: a slot begins on a 128-byte line and shares none.
//   trace    k_rt_trace, a wave per region, lanes as diagonals.  Per side: forward rows 1 .. x_end, rp_publish, then the walk —
//            rp_walk<false> of ks_rpath_kit.h, which has the fence's argument, the stage and the bounds of every step.  It
//            writes one byte per alignment column (M, I, D) into the region's column slot (an exclusive scan of aln_length):
//            the left walk forward from column 0 — walking back from the left end cell IS forward sequence order — the right
//            walk backward from column aln_length - 1, the anchor between them.
//   verify   left columns + 1 + right columns == aln_length, and anchor + H(left end cell) + H(right end cell) == score: a
//            ks_raligns used with other sequences than its own is refused, the first such region named.
//   encode   k_rt_runs, a wave per region, 64 columns at a time: with KS_RTRACE_EQX an M column becomes = or X from the two
//            residues (rp_places); a run begins where a column differs from the one
//            before.  Once to count the runs, a scan — its output IS op_offsets — and once to write len << 4 | op.
#include "ks_rpath_kit.h"

#define RT_THREADS 256
enum : u32 { RT_BAD_ROW = 0, RT_BAD_LEN = 1, RT_BAD_ALN = 2, RT_BAD_WALK = 3, RT_N_BAD = 4 };

struct rt_args {
    rk_in in;
    u32 W, o, e, x_drop;
    const u32 *s_qs, *s_ql, *s_ts, *s_tl, *s_len;
    const i64 *s_score;
    unsigned long long *bad; // RT_BAD_*: [0], [1] hit rows as in k_ralign, [2], [3] regions
};

// Region g's alignment against its sequences (wave-uniform; P.ok, P.n >= 1 and both sequences <= RA_MAX_LEN hold: nothing
// wraps).  ok: the extent lies inside the sequences, the anchor inside the extent, both end cells inside the band and
// aln_length between the longer extent and their sum — everything the forward rows and the column slot are sized by.
struct rt_geo { bool ok; u32 ai, bj, qs, ql, ts, tl, alen, xl, yl, xr, yr; };
KS_DEV u32 rt_absdiff(u32 a, u32 b) { return a > b ? a - b : b - a; }
KS_DEV rt_geo rt_geometry(const rt_args &A, const rk_at &P, u32 g) {
    rt_geo G;
    G.qs = ks_readfirst(A.s_qs[g]); G.ql = ks_readfirst(A.s_ql[g]); G.ts = ks_readfirst(A.s_ts[g]); G.tl = ks_readfirst(A.s_tl[g]);
    G.alen = ks_readfirst(A.s_len[g]);
    G.ai = P.a + P.n / 2; G.bj = P.b + P.n / 2;
    G.ok = G.ql >= 1 && G.tl >= 1 && (u64)G.qs + G.ql <= P.Lq && (u64)G.ts + G.tl <= P.Lt && G.ai >= G.qs && G.ai - G.qs < G.ql &&
           G.bj >= G.ts && G.bj - G.ts < G.tl;
    G.xl = G.ai - G.qs; G.yl = G.bj - G.ts; G.xr = G.ql - 1 - G.xl; G.yr = G.tl - 1 - G.yl;
    G.ok = G.ok && rt_absdiff(G.xl, G.yl) <= A.W && rt_absdiff(G.xr, G.yr) <= A.W && G.alen >= (G.ql > G.tl ? G.ql : G.tl) &&
           (u64)G.alen <= (u64)G.ql + G.tl - 1;
    return G;
}
// what both kernels skip alike: the plan has named it
KS_DEV bool rt_row_ok(const rk_at &P) { return P.ok && P.n != 0 && P.Lq <= RA_MAX_LEN && P.Lt <= RA_MAX_LEN; }

__global__ __launch_bounds__(RT_THREADS) void k_rt_plan(rt_args A, u32 *rows, u32 *ncols) {
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 g64 = (u64)blockIdx.x * (RT_THREADS / 64) + wave;
    if (g64 >= A.in.n_regions) return;
    const u32 g = (u32)g64;
    const rk_at P = rk_locate(A.in, g);
    u32 nr = 0, nc = 0;
    if (!rt_row_ok(P)) {
        if (lane == 0) ks_first_bad(A.bad, P.ok && P.n != 0 ? RT_BAD_LEN : RT_BAD_ROW, P.row);
    } else {
        const rt_geo G = rt_geometry(A, P, g);
        if (G.ok) { nr = rp_even(G.xr) + rp_even(G.xl); nc = G.alen; }
        else if (lane == 0) ks_first_bad(A.bad, RT_BAD_ALN, g);
    }
    if (lane == 0) { rows[g] = nr; ncols[g] = nc; }
}

struct rt_slice {
    const u64 *dir_off, *col_off; // n_regions + 1: rows of directions / columns before region g
    u8 *dir, *cols;
    u64 dir_base;                 // dir_off[g0]
    u32 g0, g1;
};

template <bool PROFILE> __global__ __launch_bounds__(RT_THREADS) void k_rt_trace(rt_args A, rt_slice Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[PROFILE ? 4 : RK_A * RK_A];
    __shared__ unsigned short s_strip[RT_THREADS / 64][RA_STRIP];
    __shared__ uint4 s_stage[RT_THREADS / 64][RP_STAGE * RA_DIR_ROW / 16];
    __shared__ u32 s_rows[RT_THREADS / 64][PROFILE ? RA_CHUNK * RA_ROW_WORDS : 1];
    if (PROFILE) rk_stage_classes(s_cls);
    else rk_stage_tables(A.in.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 g64 = (u64)Z.g0 + (u64)blockIdx.x * (RT_THREADS / 64) + wave;
    if (g64 >= Z.g1) return;
    const u32 g = (u32)g64;
    const rk_at P = rk_locate(A.in, g); // nothing below reads outside the two sequences it names
    if (!rt_row_ok(P)) return;
    const rt_geo G = rt_geometry(A, P, g);
    if (!G.ok) return;
    u8 *const dR = Z.dir + (rk_readfirst64(Z.dir_off[g]) - Z.dir_base) * RA_DIR_ROW, *const dL = dR + (u64)rp_even(G.xr) * RA_DIR_ROW;
    u8 *const col = Z.cols + rk_readfirst64(Z.col_off[g]);
    const u32 Lq = (u32)P.Lq, Lt = (u32)P.Lt;
    const u8 *qa = A.in.q_res + P.qb + G.ai, *ta = A.in.t_res + P.tb + G.bj;
    const u32 cq = ks_readfirst(*qa), ct = ks_readfirst(*ta);
    const ra_scorer<PROFILE> sc = ra_scorer_of<PROFILE>(A.in.matrix, P.qb + G.ai, s_M, s_rows[wave]);
    const int s = ra_anchor_score<PROFILE>(A.in.matrix, P.qb + G.ai, s_cls, s_M, cq, ct);
    const ra_ext R = ra_extend<true>(qa, ta, 1, Lq - 1 - G.ai, Lt - 1 - G.bj, A, s_cls, sc, s_strip[wave], lane, dR, G.xr, G.yr);
    rp_publish();
    // (the lane of an end cell, y + W - x, is 0 .. 2W: rt_geometry)
    const u32 nR = rp_walk<false>(dR, G.xr, G.yr + A.W - G.xr, A.W, 2 * A.W, RP_D, RP_I, col + (G.alen - 1), -1, G.alen - 1, s_stage[wave], lane);
    bool ok = nR != RP_BAD;
    if (ok) {
        const ra_ext L = ra_extend<true>(qa, ta, -1, G.ai, G.bj, A, s_cls, sc, s_strip[wave], lane, dL, G.xl, G.yl);
        rp_publish();
        const u32 nL = rp_walk<false>(dL, G.xl, G.yl + A.W - G.xl, A.W, 2 * A.W, RP_D, RP_I, col, 1, G.alen - 1 - nR, s_stage[wave], lane);
        ok = nL != RP_BAD && nL + 1 + nR == G.alen && (i64)s + L.score + R.score == A.s_score[g];
        if (ok && lane == 0) col[nL] = (u8)RP_M; // the anchor pair
    }
    if (!ok && lane == 0) ks_first_bad(A.bad, RT_BAD_WALK, g);
}

struct rt_rle {
    const u64 *col_off;
    const u8 *cols;
    u32 *runs;         // !WRITE: the runs of region g
    const u64 *op_off; // WRITE: their exclusive scan, and the ops
    u32 *ops;
    u32 eqx;
};

template <bool WRITE> __global__ __launch_bounds__(RT_THREADS) void k_rt_runs(rt_args A, rt_rle Z) {
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 g64 = (u64)blockIdx.x * (RT_THREADS / 64) + wave;
    if (g64 >= A.in.n_regions) return;
    const u32 g = (u32)g64;
    const rk_at P = rk_locate(A.in, g);
    rt_geo G;
    G.ok = false;
    if (rt_row_ok(P)) G = rt_geometry(A, P, g);
    if (!G.ok) { // (refused by the plan: never reached behind its wait)
        if (!WRITE && lane == 0) Z.runs[g] = 0;
        return;
    }
    const u8 *col = Z.cols + rk_readfirst64(Z.col_off[g]);
    const u8 *q = A.in.q_res + P.qb + G.qs, *t = A.in.t_res + P.tb + G.ts;
    const u32 n = G.alen;
    u64 o = 0, room = 0;
    if (WRITE) { o = rk_readfirst64(Z.op_off[g]); room = rk_readfirst64(Z.op_off[g + 1]) - o; }
    u32 nq = 0, nt = 0, prev = 0xffu, base = 0; // residues before the chunk, the last code before it, the runs begun before it
    u32 pk = 0, pstart = 0, pop = 0;            // the run that is still open: its index, first column and op
    bool open = false;
    for (u32 c = 0; c < n; c += 64) {
        const u32 i = c + lane;
        const bool valid = i < n;
        u32 code = valid ? col[i] : 0xffu;
        const rp_place at = rp_places(valid, code, lane, nq, nt);
        if (Z.eqx && code == RP_M) {
            code = RP_X;
            if (at.q < G.ql && at.t < G.tl && rk_upper(q[at.q]) == rk_upper(t[at.t])) code = RP_EQ; // (inside the extents: rt_geometry)
        }
        const u32 below = ks_lane_below(code); // (a DPP move: all lanes take part)
        const bool start = valid && code != (lane ? below : prev);
        const u64 mask = __ballot(start);
        if (WRITE && mask) {
            const u32 f = (u32)__ffsll((long long)mask) - 1u, l = 63u - (u32)__clzll((long long)mask);
            if (open && lane == f && pk < room) Z.ops[o + pk] = ((c + f - pstart) << 4) | pop; // the open run ends where the first new one begins
            const u32 idx = base + (u32)__popcll(mask & ks_lanes_below(lane));
            if (start && lane != l && idx < room) {
                const u64 later = mask & ~ks_lanes_below(lane + 1);
                Z.ops[o + idx] = (((u32)__ffsll((long long)later) - 1u - lane) << 4) | code;
            }
            pk = base + (u32)__popcll(mask) - 1u; pstart = c + l; pop = (u32)__shfl((int)code, (int)l);
            open = true;
        }
        base += (u32)__popcll(mask);
        prev = (u32)__shfl((int)code, 63);
    }
    if (WRITE) {
        if (open && lane == 0 && pk < room) Z.ops[o + pk] = ((n - pstart) << 4) | pop;
    } else if (lane == 0) Z.runs[g] = base;
}

int ks_regions_traceback_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                              const ks_raligns *S, const ks_profile *prof, u32 flags, u64 max_scratch_bytes, ks_cigars *C) {
    const u64 n_rows = R->n_rows, ng = R->n_regions;
    C->n_rows = n_rows; C->n_regions = ng;
    KS_TRY(ks_alloc(ctx, &C->d_op_offsets, (size_t)ng + 1));
    if (ng == 0) {
        KS_HIP(ctx, hipMemsetAsync(C->d_op_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    KS_TRY(rk_counts_check(ctx, "region traceback", n_rows, ng));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    ks_ctl ctl;
    u32 *rows = nullptr, *ncols = nullptr;
    u64 *dir_off = nullptr, *col_off = nullptr;
    if (!prof) KS_TRY(rk_upload_matrix(ctx, sc, S->matrix, &d_M));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RTRACE, RT_N_BAD, 0));
    KS_TRY(sc.alloc(&rows, (size_t)ng)); KS_TRY(sc.alloc(&ncols, (size_t)ng));
    KS_TRY(sc.alloc(&dir_off, (size_t)ng + 1)); KS_TRY(sc.alloc(&col_off, (size_t)ng + 1));

    rt_args A;
    A.in = rk_in_of(R, H, Q, T, prof ? (const signed char *)prof->d_scores : d_M);
    A.W = S->band; A.o = S->gap_open; A.e = S->gap_extend; A.x_drop = S->x_drop;
    A.s_qs = S->d_qstart; A.s_ql = S->d_qlength; A.s_ts = S->d_tstart; A.s_tl = S->d_tlength; A.s_len = S->d_aln_length;
    A.s_score = S->d_score;
    A.bad = ctl.words();
    const u32 grid = (u32)((ng + RT_THREADS / 64 - 1) / (RT_THREADS / 64));
    KS_LAUNCH(ctx, "rtrace_plan", k_rt_plan, grid, RT_THREADS, A, rows, ncols);
    KS_TRY(ks_scan_u32_to_u64_wide(ctx, rows, dir_off, ng)); // (the directions are made in slices: no allocation bounds their sum)
    KS_TRY(ks_scan_u32_to_u64(ctx, ncols, col_off, ng));
    u64 *const rb = ctx->h_pin + KS_PIN_RTRACE + RT_N_BAD; // direction rows | columns | ops
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(dir_off + ng, rb, 2), ks_fetch_words(col_off + ng, rb + 1, 2)}));
    if (ctl.bad(RT_BAD_ROW)) return rk_fail_bad_row(ctx, "region traceback", ctl[RT_BAD_ROW], Q, T);
    if (ctl.bad(RT_BAD_LEN))
        return ks_fail(ctx, KS_ERR_CAPACITY, "region traceback: hit row %llu has a query or target sequence of more than 2^20 residues",
                       (unsigned long long)ctl[RT_BAD_LEN]);
    if (ctl.bad(RT_BAD_ALN))
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "region traceback: the alignment of region %llu does not lie inside its two sequences around its seed's "
                       "anchor: alignments, regions and batches do not belong together", (unsigned long long)ctl[RT_BAD_ALN]);
    const u64 total_rows = rb[0], total_cols = rb[1];

    // slices of consecutive regions whose directions fit the budget
    const u64 budget_rows = (max_scratch_bytes ? max_scratch_bytes : (u64)1 << 30) / RA_DIR_ROW;
    rp_slices Sl;
    KS_TRY(rp_slices_of(ctx, dir_off, ng, total_rows, budget_rows, &Sl));
    if (Sl.bad < ng)
        return ks_fail(ctx, KS_ERR_CAPACITY, "region traceback: region %llu needs %llu bytes of directions, max_scratch_bytes allows %llu",
                       (unsigned long long)Sl.bad, (unsigned long long)(Sl.bad_rows * RA_DIR_ROW), (unsigned long long)(budget_rows * RA_DIR_ROW));
    const std::vector<u64> &cut = Sl.cut, &first_row = Sl.first_row;
    const u64 slice_rows = Sl.max_rows;
    u8 *dir = nullptr, *cols = nullptr;
    KS_TRY(sc.alloc(&dir, (size_t)(slice_rows * RA_DIR_ROW)));
    KS_TRY(sc.alloc(&cols, (size_t)total_cols));
    C->dir_bytes = slice_rows * RA_DIR_ROW; C->n_slices = (u32)(cut.size() - 1);
    for (size_t i = 0; i + 1 < cut.size(); i++) { // (one block for all slices: the launches are ordered by the stream)
        const rt_slice Z{dir_off, col_off, dir, cols, first_row[i], (u32)cut[i], (u32)cut[i + 1]};
        const u32 slice_grid = (u32)((cut[i + 1] - cut[i] + RT_THREADS / 64 - 1) / (RT_THREADS / 64));
        if (prof) KS_LAUNCH(ctx, "rtrace_profile", k_rt_trace<true>, slice_grid, RT_THREADS, A, Z);
        else KS_LAUNCH(ctx, "rtrace", k_rt_trace<false>, slice_grid, RT_THREADS, A, Z);
    }

    // the runs per region (`rows` is free again), their scan = op_offsets, the ops
    rt_rle E{col_off, cols, rows, C->d_op_offsets, nullptr, (flags & KS_RTRACE_EQX) ? 1u : 0u};
    KS_LAUNCH(ctx, "rtrace_runs", k_rt_runs<false>, grid, RT_THREADS, A, E);
    KS_TRY(ks_scan_u32_to_u64(ctx, rows, C->d_op_offsets, ng));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(C->d_op_offsets + ng, rb + 2, 2)}));
    if (ctl.bad(RT_BAD_WALK))
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "region traceback: the path of region %llu does not give the alignment's length and score: the alignments "
                       "were not made from these regions and batches", (unsigned long long)ctl[RT_BAD_WALK]);
    C->n_ops = rb[2];
    KS_TRY(ks_alloc(ctx, &C->d_ops, (size_t)C->n_ops));
    E.ops = C->d_ops;
    KS_LAUNCH(ctx, "rtrace_runs", k_rt_runs<true>, grid, RT_THREADS, A, E);
    return ks_stream_wait(ctx);
}

extern "C" uint32_t ks_debug_rtrace_stage(void) { return RP_STAGE; }
