// ks_rstitch.hip — ks_regions_stitch: the chain of every hit row (ks_rchain.hip) made into ONE gapped alignment with one CIGAR
// (include/kmerseek_amd.h has the contract).  The members keep the paths ks_regions_traceback gave them; what lies between two
// consecutive members — the link — is aligned globally when its shorter side fits the lanes of a wave, and left open otherwise.
// All of it in integers.
//
//   plan     k_rs_plan, a thread per chain member: everything is checked before it is indexed — the member lies in its row's
//            regions and inside its two sequences, its ops consume exactly its extents and carry the right pair codes, its ends
//            do not lie before those of the member before it.  The same walk over the member's ops (a handful) finds the trim:
//            the leading columns that lie before the previous member's ends, the first op that is kept and what is left of it.
//            Then the link's rectangle and its class, and for a filled link the rows of directions and the columns it needs;
//            two exclusive scans (ks_prims.hip) lay both out, one wait brings the totals and the first refused member.
//   slices   consecutive members whose directions fit the scratch budget run in one launch (as ks_rtrace.hip does).
//   fill     k_rs_fill, a wave per filled link: rf_fill of ks_rfill_kit.h on the link's two stretches — the global affine
//            program with lanes as the columns of the SHORTER stretch, its walk back into the link's column slot and the
//            = / X pass — which ks_fstitch.hip runs too: one program, the orientation is part of the contract.
//   emit     k_rs_emit<false / true>, a thread per hit row: the pieces of the row in order — member ops from the first kept
//            one, link runs or the link's columns — through one run merger; once to count the ops (and the row's link
//            counts and span), a scan — its output IS op_offsets — and once to write len << 4 | code.
//   rescore  k_rs_rescore, a wave per hit row: the final ops replayed on the residues, the pairs of an op 64 at a time.
#include "ks_rfill_kit.h"

#define RS_THREADS 256
#define RS_SHORT_MAX RF_SHORT_MAX
#define RS_MAX_FILL 4096u
enum : u32 { RS_BAD_SRC = 0, RS_BAD_ROW = 1, RS_BAD_LEN = 2, RS_BAD_EXT = 3, RS_BAD_OPS = 4, RS_BAD_CODE = 5, RS_BAD_ASC = 6, RS_BAD_WALK = 7, RS_N_BAD = 8 };
enum : u32 { RS_L_NONE = 0, RS_L_I = 1, RS_L_D = 2, RS_L_FILL = 3, RS_L_FILL_SWAP = 4, RS_L_OPEN = 5 };

// per chain member: its trim and the link in front of it
struct rs_link {
    u32 trim;      // leading columns removed
    u32 kop, krem; // the first op that is kept (inside the member's ops) and what is left of it
    u32 X, Y;      // the link's rectangle: query and target residues between the previous member's ends and (q', t')
    u32 cls;       // RS_L_*
    u32 ncol;      // filled: the columns of the path (k_rs_fill)
    u32 pad;
};

struct rs_args {
    const u64 *c_offs; const u32 *c_src;                      // the chain: n_rows + 1, n_chained
    const u64 *a_offs; const u32 *a_qs, *a_ql, *a_ts, *a_tl;  // the alignments
    const u64 *g_offs; const u32 *g_ops;                      // their CIGARs
    const u32 *qid, *tid;
    const u8 *q_res, *t_res;
    const u64 *q_offs, *t_offs;
    const signed char *matrix;
    u64 n_q_res, n_t_res, n_gops;
    u32 n_rows, n_chained, n_regions, n_q, n_t;
    u32 o, e, max_fill, eqx;
    unsigned long long *bad;
};

KS_DEV bool rs_is_pair(u32 c) { return c == RP_M || c == RP_EQ || c == RP_X; }
KS_DEV u32 rs_even(u32 v) { return (v + 1u) & ~1u; }
KS_DEV double rs_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__global__ __launch_bounds__(RS_THREADS) void k_rs_plan(rs_args A, rs_link *links, u32 *rows, u32 *ncols) {
    const u64 j64 = (u64)blockIdx.x * RS_THREADS + threadIdx.x;
    if (j64 >= A.n_chained) return;
    const u32 j = (u32)j64;
    rs_link L{0u, 0u, 0u, 0u, 0u, RS_L_NONE, 0u, 0u};
    u32 nr = 0, nc = 0;
    [&]() {
        const u32 r = ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j); // (c_offs[0] == 0 <= j)
        const bool first = A.c_offs[r] == j;
        const u32 g = A.c_src[j];
        if (g >= A.n_regions || g < A.a_offs[r] || g >= A.a_offs[r + 1]) { ks_first_bad(A.bad, RS_BAD_SRC, j); return; }
        const u32 q = A.qid[r], t = A.tid[r];
        if (q >= A.n_q || t >= A.n_t) { ks_first_bad(A.bad, RS_BAD_ROW, r); return; }
        const rk_seqs S = rk_row_seqs<false>(A, q, t);
        if (!S.ok) { ks_first_bad(A.bad, RS_BAD_ROW, r); return; }
        if (S.Lq > RA_MAX_LEN || S.Lt > RA_MAX_LEN) { ks_first_bad(A.bad, RS_BAD_LEN, r); return; }
        const u64 qs = A.a_qs[g], ql = A.a_ql[g], ts = A.a_ts[g], tl = A.a_tl[g];
        if (ql == 0 || tl == 0 || qs + ql > S.Lq || ts + tl > S.Lt) { ks_first_bad(A.bad, RS_BAD_EXT, g); return; }
        u64 pqe = 0, pte = 0;
        if (!first) {
            const u32 gp = A.c_src[j - 1];
            if (gp >= A.n_regions) return; // (its own thread names it)
            pqe = (u64)A.a_qs[gp] + A.a_ql[gp]; pte = (u64)A.a_ts[gp] + A.a_tl[gp];
            if (qs + ql < pqe || ts + tl < pte) { ks_first_bad(A.bad, RS_BAD_ASC, j); return; }
        }
        const u64 ob = A.g_offs[g], oe = A.g_offs[g + 1];
        if (ob > oe || oe > A.n_gops) { ks_first_bad(A.bad, RS_BAD_OPS, g); return; }
        const u32 nops = (u32)(oe - ob < 0xffffffffULL ? oe - ob : 0xffffffffULL);
        // one walk: what the ops consume, their codes, and the trim
        u64 cq = 0, ct = 0, qpos = qs, tpos = ts;
        bool done = first, bad_code = false, bad_op = false;
        if (first) { L.kop = 0; L.krem = nops ? A.g_ops[ob] >> 4 : 0u; }
        for (u32 k = 0; k < nops; k++) {
            const u32 op = A.g_ops[ob + k], len = op >> 4, code = op & 15u;
            const bool pair = rs_is_pair(code);
            if (!pair && code != RP_I && code != RP_D) bad_op = true;
            if (pair && (A.eqx ? code == RP_M : code != RP_M)) bad_code = true;
            const u64 dq = pair || code == RP_I ? 1u : 0u, dt = pair || code == RP_D ? 1u : 0u;
            cq += len * dq; ct += len * dt;
            if (done) continue;
            const u64 needq = qpos >= pqe ? 0 : pqe - qpos, needt = tpos >= pte ? 0 : pte - tpos;
            const u64 n = needq > needt ? needq : needt;
            if ((needq == 0 || dq) && (needt == 0 || dt) && n <= len) {
                done = true;
                L.kop = k; L.krem = len - (u32)n; L.trim += (u32)n;
                qpos += n * dq; tpos += n * dt;
            } else { L.trim += len; qpos += len * dq; tpos += len * dt; }
        }
        if (bad_op || cq != ql || ct != tl) { ks_first_bad(A.bad, RS_BAD_OPS, g); return; }
        if (bad_code) { ks_first_bad(A.bad, RS_BAD_CODE, g); return; }
        if (!done) { L.kop = nops; L.krem = 0; } // (no column is left: the position is the member's end)
        if (first) return;
        // (ends that do not descend and ops that consume the extents: qpos >= pqe and tpos >= pte hold)
        const u64 X = qpos - pqe, Y = tpos - pte;
        L.X = (u32)X; L.Y = (u32)Y;
        const u64 lo = X < Y ? X : Y, hi = X < Y ? Y : X;
        if (hi == 0) L.cls = RS_L_NONE;
        else if (Y == 0) L.cls = RS_L_I;
        else if (X == 0) L.cls = RS_L_D;
        else if (lo <= RS_SHORT_MAX && hi <= A.max_fill) {
            L.cls = X < Y ? RS_L_FILL_SWAP : RS_L_FILL;
            nr = rs_even((u32)hi); nc = (u32)(X + Y);
        } else L.cls = RS_L_OPEN;
    }();
    links[j] = L; rows[j] = nr; ncols[j] = nc;
}

struct rs_slice {
    const u64 *dir_off, *col_off; // n_chained + 1: rows of directions / columns before member j
    u8 *dir, *cols;
    u64 dir_base;                 // dir_off[j0]
    u32 j0, j1;
};

__global__ __launch_bounds__(RS_THREADS) void k_rs_fill(rs_args A, rs_link *links, rs_slice Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    __shared__ uint4 s_stage[RS_THREADS / 64][RP_STAGE * RA_DIR_ROW / 16];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 j64 = (u64)Z.j0 + (u64)blockIdx.x * (RS_THREADS / 64) + wave;
    if (j64 >= Z.j1) return;
    const u32 j = (u32)j64;
    const u32 cls = ks_readfirst(links[j].cls);
    if (cls != RS_L_FILL && cls != RS_L_FILL_SWAP) return;
    // (behind the plan's wait: the member, the one before it and their row have passed every check)
    const bool swap = cls == RS_L_FILL_SWAP;
    const u32 X = ks_readfirst(links[j].X), Y = ks_readfirst(links[j].Y);
    const rf_rect R = rf_rect_of(X, Y, swap);
    const u32 r = ks_readfirst(ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j));
    const u32 gp = ks_readfirst(A.c_src[j - 1]);
    const u32 pqe = ks_readfirst(A.a_qs[gp]) + ks_readfirst(A.a_ql[gp]), pte = ks_readfirst(A.a_ts[gp]) + ks_readfirst(A.a_tl[gp]);
    const u32 q = ks_readfirst(A.qid[r]), t = ks_readfirst(A.tid[r]);
    const u8 *const qst = A.q_res + rk_readfirst64(A.q_offs[q]) + pqe, *const tst = A.t_res + rk_readfirst64(A.t_offs[t]) + pte;
    u8 *const dir = Z.dir + (rk_readfirst64(Z.dir_off[j]) - Z.dir_base) * RA_DIR_ROW;
    const u32 cap = X + Y;
    u8 *const col = Z.cols + rk_readfirst64(Z.col_off[j]);
    rf_fill(R, qst, tst, A.o, A.e, A.eqx, dir, col, cap, s_cls, s_M, s_stage[wave], lane, [=](u32 n) {
        if (n == RP_BAD) {
            if (lane == 0) { ks_first_bad(A.bad, RS_BAD_WALK, j); links[j].ncol = 0; }
        } else if (lane == 0) links[j].ncol = n;
    });
}

struct rs_out {
    const u64 *col_off;
    const u8 *cols;
    u32 *n_ops;        // !WRITE: the ops of row r
    const u64 *op_off; // WRITE: their exclusive scan, and the ops
    u32 *ops;
    u32 *q_start, *q_length, *t_start, *t_length, *n_members, *n_filled, *n_open, *n_trimmed;
};

template <bool WRITE> __global__ __launch_bounds__(RS_THREADS) void k_rs_emit(rs_args A, const rs_link *links, rs_out Z) {
    const u64 r64 = (u64)blockIdx.x * RS_THREADS + threadIdx.x;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    const u64 b = A.c_offs[r], e = A.c_offs[r + 1];
    u64 o = 0, room = 0;
    if (WRITE) { o = Z.op_off[r]; room = Z.op_off[r + 1] - o; }
    u32 cur = 0xffu, len = 0, n = 0;
    auto flush = [&]() {
        if (cur == 0xffu) return;
        if (WRITE && n < room) Z.ops[o + n] = (len << 4) | cur;
        n++;
    };
    auto push = [&](u32 code, u32 cnt) {
        if (cnt == 0) return;
        if (code == cur) { len += cnt; return; } // (a joint merges)
        flush();
        cur = code; len = cnt;
    };
    u32 n_filled = 0, n_open = 0, n_trim = 0;
    for (u64 j = b; j < e; j++) {
        const rs_link L = links[j];
        const u32 g = A.c_src[j];
        n_trim += L.trim;
        if (j > b) {
            if (L.cls == RS_L_I) push(RP_I, L.X);
            else if (L.cls == RS_L_D) push(RP_D, L.Y);
            else if (L.cls == RS_L_OPEN) { push(RP_I, L.X); push(RP_D, L.Y); n_open++; }
            else if (L.cls == RS_L_FILL || L.cls == RS_L_FILL_SWAP) {
                const u8 *path = Z.cols + Z.col_off[j] + (L.X + L.Y - L.ncol);
                for (u32 c = 0; c < L.ncol; c++) push(path[c], 1u);
                n_filled++;
            }
        }
        const u64 ob = A.g_offs[g];
        const u32 nops = (u32)(A.g_offs[g + 1] - ob);
        for (u32 k = L.kop; k < nops; k++) {
            const u32 op = A.g_ops[ob + k];
            push(op & 15u, k == L.kop ? L.krem : op >> 4);
        }
    }
    flush();
    if (WRITE) return;
    Z.n_ops[r] = n;
    u32 qs = 0, qe = 0, ts = 0, te = 0;
    if (e > b) {
        const u32 g0 = A.c_src[b], g1 = A.c_src[e - 1];
        qs = A.a_qs[g0]; ts = A.a_ts[g0]; qe = A.a_qs[g1] + A.a_ql[g1]; te = A.a_ts[g1] + A.a_tl[g1];
    }
    Z.q_start[r] = qs; Z.q_length[r] = qe - qs; Z.t_start[r] = ts; Z.t_length[r] = te - ts;
    Z.n_members[r] = (u32)(e - b); Z.n_filled[r] = n_filled; Z.n_open[r] = n_open; Z.n_trimmed[r] = n_trim;
}

struct rs_cols {
    const u64 *op_off;
    const u32 *ops, *q_start, *t_start;
    i64 *score;
    u32 *identities, *positives, *gap_opens, *gaps, *aln_length;
    double *row_score;
};

KS_DEV u32 rs_wave_sum(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (u32)__shfl_xor((int)v, d);
    return v;
}

__global__ __launch_bounds__(RS_THREADS) void k_rs_rescore(rs_args A, rs_cols Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 r64 = (u64)blockIdx.x * (RS_THREADS / 64) + wave;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    const u64 ob = rk_readfirst64(Z.op_off[r]), oe = rk_readfirst64(Z.op_off[r + 1]);
    const bool empty = rk_readfirst64(A.c_offs[r]) == rk_readfirst64(A.c_offs[r + 1]);
    int sc = 0; // (at most 2^21 columns of |M| <= 128 over the lanes: 32 bits)
    u32 id = 0, po = 0, opens = 0, gaps = 0, alen = 0;
    i64 gap_cost = 0;
    if (!empty) {
        // (a row with members has passed the plan: its ops stay inside [q_start, q_end) x [t_start, t_end) of its sequences)
        const u32 q = ks_readfirst(A.qid[r]), t = ks_readfirst(A.tid[r]);
        const u8 *qp = A.q_res + rk_readfirst64(A.q_offs[q]) + ks_readfirst(Z.q_start[r]);
        const u8 *tp = A.t_res + rk_readfirst64(A.t_offs[t]) + ks_readfirst(Z.t_start[r]);
        for (u64 k = ob; k < oe; k++) {
            const u32 op = ks_readfirst(Z.ops[k]), len = op >> 4, code = op & 15u;
            alen += len;
            if (rs_is_pair(code)) {
                for (u32 c = lane; c < len; c += 64) {
                    const u32 a = qp[c], b = tp[c];
                    const int s = s_M[s_cls[a] * RK_A + s_cls[b]];
                    sc += s; id += rk_upper(a) == rk_upper(b) ? 1u : 0u; po += s > 0 ? 1u : 0u;
                }
                qp += len; tp += len;
            } else {
                opens++; gaps += len; gap_cost += (i64)A.o + (i64)len * A.e;
                if (code == RP_I) qp += len; else tp += len;
            }
        }
    }
    const i64 total = (i64)(int)rs_wave_sum((u32)sc) - gap_cost;
    id = rs_wave_sum(id); po = rs_wave_sum(po);
    if (lane == 0) {
        Z.score[r] = total; Z.identities[r] = id; Z.positives[r] = po; Z.gap_opens[r] = opens; Z.gaps[r] = gaps; Z.aln_length[r] = alen;
        Z.row_score[r] = empty ? rs_nan() : (double)total;
    }
}

int ks_regions_stitch_impl(ks_ctx *ctx, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G, const ks_hits *H, const ks_res_batch &Q,
                           const ks_res_batch &T, u32 max_fill, u32 flags, u64 max_scratch_bytes, ks_hitalns *R) {
    const u64 n_rows = K->n_rows, nm = K->n_chained;
    R->n_rows = n_rows; R->n_ops = 0; R->dir_bytes = 0; R->n_slices = 0;
    KS_TRY(ks_alloc(ctx, &R->d_op_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, R, R->n_rows));
    if (n_rows == 0) {
        KS_HIP(ctx, hipMemsetAsync(R->d_op_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    KS_TRY(rk_counts_check(ctx, "region stitch", n_rows, S->n_regions));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    ks_ctl ctl;
    rs_link *links = nullptr;
    u32 *rows = nullptr, *ncols = nullptr, *row_ops = nullptr;
    u64 *dir_off = nullptr, *col_off = nullptr;
    KS_TRY(rk_upload_matrix(ctx, sc, S->matrix, &d_M));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RSTITCH, RS_N_BAD, 0));
    KS_TRY(sc.alloc(&links, (size_t)nm)); KS_TRY(sc.alloc(&rows, (size_t)nm)); KS_TRY(sc.alloc(&ncols, (size_t)nm));
    KS_TRY(sc.alloc(&dir_off, (size_t)nm + 1)); KS_TRY(sc.alloc(&col_off, (size_t)nm + 1));
    KS_TRY(sc.alloc(&row_ops, (size_t)n_rows));

    rs_args A;
    A.c_offs = K->d_row_offsets; A.c_src = K->d_src_region;
    A.a_offs = S->d_row_offsets; A.a_qs = S->d_qstart; A.a_ql = S->d_qlength; A.a_ts = S->d_tstart; A.a_tl = S->d_tlength;
    A.g_offs = G->d_op_offsets; A.g_ops = G->d_ops;
    A.qid = H->d_qid; A.tid = H->d_tid;
    A.q_res = Q.res; A.t_res = T.res; A.q_offs = Q.offs; A.t_offs = T.offs;
    A.matrix = d_M;
    A.n_q_res = Q.n_res; A.n_t_res = T.n_res; A.n_gops = G->n_ops;
    A.n_rows = (u32)n_rows; A.n_chained = (u32)nm; A.n_regions = (u32)S->n_regions; A.n_q = Q.n_seqs; A.n_t = T.n_seqs;
    A.o = S->gap_open; A.e = S->gap_extend; A.max_fill = max_fill; A.eqx = (flags & KS_RSTITCH_EQX) ? 1u : 0u;
    A.bad = ctl.words();

    u64 *const rb = ctx->h_pin + KS_PIN_RSTITCH + RS_N_BAD; // direction rows | columns | ops
    rb[0] = rb[1] = rb[2] = 0;
    u8 *dir = nullptr, *cols = nullptr;
    if (nm) {
        KS_LAUNCH(ctx, "rstitch_plan", k_rs_plan, (u32)((nm + RS_THREADS - 1) / RS_THREADS), RS_THREADS, A, links, rows, ncols);
        KS_TRY(ks_scan_u32_to_u64_wide(ctx, rows, dir_off, nm)); // (the directions are made in slices: no allocation bounds their sum)
        KS_TRY(ks_scan_u32_to_u64(ctx, ncols, col_off, nm));
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(dir_off + nm, rb, 2), ks_fetch_words(col_off + nm, rb + 1, 2)}));
        if (ctl.bad(RS_BAD_SRC))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: chain member %llu names a region outside its hit row's alignments: the chain was not made from these alignments",
                           (unsigned long long)ctl[RS_BAD_SRC]);
        if (ctl.bad(RS_BAD_ROW)) return rk_fail_bad_row(ctx, "region stitch", ctl[RS_BAD_ROW], Q, T);
        if (ctl.bad(RS_BAD_LEN))
            return ks_fail(ctx, KS_ERR_CAPACITY, "region stitch: hit row %llu has a query or target sequence of more than 2^20 residues",
                           (unsigned long long)ctl[RS_BAD_LEN]);
        if (ctl.bad(RS_BAD_EXT))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: the alignment of region %llu does not lie inside its two sequences: alignments, hits and batches do not belong together",
                           (unsigned long long)ctl[RS_BAD_EXT]);
        if (ctl.bad(RS_BAD_OPS))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: the ops of region %llu do not consume exactly its q_length and t_length: the CIGARs were not traced from these alignments",
                           (unsigned long long)ctl[RS_BAD_OPS]);
        if (ctl.bad(RS_BAD_CODE))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, A.eqx ? "region stitch: KS_RSTITCH_EQX is set and the ops of region %llu hold M: trace with KS_RTRACE_EQX"
                                                          : "region stitch: the ops of region %llu hold = or X: set KS_RSTITCH_EQX",
                           (unsigned long long)ctl[RS_BAD_CODE]);
        if (ctl.bad(RS_BAD_ASC))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: chain member %llu ends before the member in front of it on one of the sequences: the chain was not made from these alignments",
                           (unsigned long long)ctl[RS_BAD_ASC]);
        const u64 total_rows = rb[0], total_cols = rb[1];

        // slices of consecutive members whose directions fit the budget
        const u64 budget_rows = (max_scratch_bytes ? max_scratch_bytes : (u64)1 << 30) / RA_DIR_ROW;
        rp_slices Sl;
        KS_TRY(rp_slices_of(ctx, dir_off, nm, total_rows, budget_rows, &Sl));
        if (Sl.bad < nm)
            return ks_fail(ctx, KS_ERR_CAPACITY, "region stitch: the link in front of chain member %llu needs %llu bytes of directions, max_scratch_bytes allows %llu",
                           (unsigned long long)Sl.bad, (unsigned long long)(Sl.bad_rows * RA_DIR_ROW), (unsigned long long)(budget_rows * RA_DIR_ROW));
        const std::vector<u64> &cut = Sl.cut, &first_row = Sl.first_row;
        const u64 slice_rows = Sl.max_rows;
        KS_TRY(sc.alloc(&dir, (size_t)(slice_rows * RA_DIR_ROW)));
        KS_TRY(sc.alloc(&cols, (size_t)total_cols));
        R->dir_bytes = slice_rows * RA_DIR_ROW; R->n_slices = (u32)(cut.size() - 1);
        if (total_rows)
            for (size_t i = 0; i + 1 < cut.size(); i++) { // (one block for all slices: the launches are ordered by the stream)
                const rs_slice Z{dir_off, col_off, dir, cols, first_row[i], (u32)cut[i], (u32)cut[i + 1]};
                KS_LAUNCH(ctx, "rstitch_fill", k_rs_fill, (u32)((cut[i + 1] - cut[i] + RS_THREADS / 64 - 1) / (RS_THREADS / 64)), RS_THREADS, A, links, Z);
            }
    }

    // the ops per row, their scan = op_offsets, the ops, the columns
    const u32 grid = (u32)((n_rows + RS_THREADS - 1) / RS_THREADS);
    rs_out E{col_off, cols, row_ops, R->d_op_offsets, nullptr, R->d_q_start, R->d_q_length, R->d_t_start, R->d_t_length,
             R->d_n_members, R->d_n_filled, R->d_n_open, R->d_n_trimmed};
    KS_LAUNCH(ctx, "rstitch_count", k_rs_emit<false>, grid, RS_THREADS, A, (const rs_link *)links, E);
    KS_TRY(ks_scan_u32_to_u64(ctx, row_ops, R->d_op_offsets, n_rows));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(R->d_op_offsets + n_rows, rb + 2, 2)}));
    if (ctl.bad(RS_BAD_WALK))
        return ks_fail(ctx, KS_ERR_HIP, "region stitch: internal error: the fill in front of chain member %llu did not walk back to its origin",
                       (unsigned long long)ctl[RS_BAD_WALK]);
    R->n_ops = rb[2];
    KS_TRY(ks_alloc(ctx, &R->d_ops, (size_t)R->n_ops));
    E.ops = R->d_ops;
    KS_LAUNCH(ctx, "rstitch_ops", k_rs_emit<true>, grid, RS_THREADS, A, (const rs_link *)links, E);
    const rs_cols C{R->d_op_offsets, R->d_ops, R->d_q_start, R->d_t_start, R->d_score, R->d_identities, R->d_positives, R->d_gap_opens,
                    R->d_gaps, R->d_aln_length, R->d_row_score};
    KS_LAUNCH(ctx, "rstitch_rescore", k_rs_rescore, (u32)((n_rows + RS_THREADS / 64 - 1) / (RS_THREADS / 64)), RS_THREADS, A, C);
    return ks_stream_wait(ctx);
}

extern "C" uint32_t ks_debug_rstitch_stage(void) { return RP_STAGE; }
