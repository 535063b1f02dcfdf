// ks_stitch_kit.h — the stitch of a chain into ONE alignment with one CIGAR, shared by ks_regions_stitch (ks_rstitch.hip: the
// members of one protein pair) and ks_frames_stitch (ks_fstitch.hip: members in the three frames of one strand).  The members
// keep the paths ks_regions_traceback gave them; what lies between two consecutive members — the link — is aligned globally
// when its shorter side fits the lanes of a wave, and left open otherwise.  All of it in integers.  One definition of the checks'
// order, the trim, the link classes, the run merger, the re-scoring and the host driver: as for the fill (ks_rfill_kit.h),
// none of them can differ between the two passes.
//
// The frame stitch is the region stitch under a coordinate map, the policy C.  The query axis is counted in units of which a
// column that consumes the query takes C::UNIT: 1, residues, or 3, the bases of a strand.  A member starts at phase + UNIT *
// q_start of its alignment, and position p of the axis is residue p / UNIT of sequence C::seq_at(q, p).  A link of X units is
// c = X / UNIT columns and r = X % UNIT skipped units, the N op (KS_CIGAR_FSHIFT); with UNIT = 1, r is 0 and every trace of it
// compiles away.  A policy supplies
//   UNIT, ext, spans, result     the unit, its extra kernel arguments (UNIT > 1: with fcost, what an N op costs the score), the
//                                span columns it writes, its result object
//   link, keep(..), ends_of(..)  the record of a chain member and the link in front of it: g, trim, kop, krem, c, Y, cls, ncol
//                                as below (UNIT > 1: and r); what else the plan has of the link is the policy's to keep, and
//                                the fill asks it for the ends of the member in front.  The record is the policy's own, down to
//                                the order of its words: one 48-byte record for both passes cost the region stitch of 2 M
//                                members 7 % in the plan and the fill and 20 % in the count, and the frame stitch's words in
//                                another order 5 % in the ops (the kernel waits for the whole record before its first use).
//   member<NAME>(..)             chain member j of a row as st_member, with its own checks; NAME: the refused member is named
//                                (ks_first_bad), else it is the member in front of the thread's own, which its own thread names
//   seq_at(q, p)                 the sequence of the query batch that position p of row qid q's axis lies in
//   write_spans(..)              the span columns of a row on the query axis (st_emit<C, false>)
//   pass, pin, k_*, refuse(..)   the pass's name, its pinned slot, its ks_timing names and its sentences: every text is the pass's
//   spans_of(R), axis_start(R)   on the host: the span columns of a result, and the one that holds a row's start on the axis
//
//   plan     st_plan, a thread per chain member: everything is checked before it is indexed — the member as its policy
//            resolves it, its two sequences inside their batches, its extents inside them, its ops consume exactly its extents
//            and carry the right pair codes, its ends do not lie before those of the member before it.  The same walk over the
//            member's ops (a handful) finds the trim: the leading columns that lie before the previous member's ends, the first
//            op that is kept and what is left of it.  Then the link's rectangle (c, Y) and its class, and for a filled link the
//            rows of directions and the columns it needs; two exclusive scans (ks_prims.hip) lay both out, one wait brings the
//            totals and the first refused member.
//   slices   consecutive members whose directions fit the scratch budget run in one launch (as ks_rtrace.hip does).
//   fill     st_fill, a wave per filled link: rf_fill of ks_rfill_kit.h on the link's two stretches, the query stretch taken
//            from the PREVIOUS member's sequence directly after its end.
//   emit     st_emit<C, false / true>, a thread per row: the pieces of the row in order — member ops from the first kept one,
//            link runs or the link's columns, the N op — through one run merger that never merges N; once to count the ops
//            (and the row's link counts and spans), a scan — its output IS op_offsets — and once to write len << 4 | code.
//   rescore  st_rescore, a wave per row: the final ops replayed on the residues, the pairs of an op 64 at a time; each lane's
//            column computes its own position on the axis and from it the sequence and the residue.
// No atomics but the first-offender words; the result does not depend on the launch geometry, the slices or the stage.
#pragma once
#include "ks_rfill_kit.h"

#define ST_THREADS 256
#define ST_N KS_CIGAR_FSHIFT
// the first-offender words of both passes, in the order they are reported; the region stitch never raises FSRC, FOLD, STRAND
enum : u32 { ST_BAD_SRC = 0, ST_BAD_FSRC = 1, ST_BAD_FOLD = 2, ST_BAD_STRAND = 3, ST_BAD_ROW = 4, ST_BAD_LEN = 5, ST_BAD_EXT = 6, ST_BAD_OPS = 7,
              ST_BAD_CODE = 8, ST_BAD_ASC = 9, ST_BAD_WALK = 10, ST_N_BAD = 11 };
enum : u32 { ST_L_NONE = 0, ST_L_I = 1, ST_L_D = 2, ST_L_FILL = 3, ST_L_FILL_SWAP = 4, ST_L_OPEN = 5 };

// What C::link holds per chain member — its alignment, its trim and the link in front of it:
//   g           the member's region in the alignments and the CIGARs
//   trim        leading columns removed
//   kop, krem   the first op that is kept (inside the member's ops) and what is left of it
//   c, Y        the link's rectangle: query columns (X = UNIT c + r units) and target residues
//   cls         ST_L_* of the rectangle
//   ncol        filled: the columns of the path (st_fill)
// a chain member as its policy resolves it: region g of the alignments, in sequence seq of the query batch, phase units into the axis
struct st_member { u32 g, seq, phase; };

struct st_args {
    const u64 *c_offs; const u32 *c_src;     // the chain: n_rows + 1, n_chained
    const u32 *a_qs, *a_ql, *a_ts, *a_tl;    // the alignments
    const u64 *g_offs; const u32 *g_ops;     // their CIGARs
    const u32 *qid, *tid;                    // the hits
    const u8 *q_res, *t_res;                 // the query batch (of a frame stitch: the frames), the target batch
    const u64 *q_offs, *t_offs;
    const signed char *matrix;
    u64 n_q_res, n_t_res, n_gops;
    u32 n_rows, n_chained, n_regions, n_q, n_t;
    u32 o, e, max_fill, eqx;
    unsigned long long *bad;
};

template <class C> __global__ __launch_bounds__(ST_THREADS) void st_plan(st_args A, typename C::ext F, typename C::link *links, u32 *rows, u32 *ncols) {
    constexpr u32 U = C::UNIT;
    const u64 j64 = (u64)blockIdx.x * ST_THREADS + threadIdx.x;
    if (j64 >= A.n_chained) return;
    const u32 j = (u32)j64;
    typename C::link L{}; // (zeros: ST_L_NONE)
    u32 nr = 0, nc = 0;
    [&]() {
        const u32 row = ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j); // (c_offs[0] == 0 <= j)
        const bool first = A.c_offs[row] == j;
        const u32 q = A.qid[row], t = A.tid[row];
        st_member M;
        if (!C::template member<true>(A, F, row, j, q, t, M)) return;
        const u32 g = M.g;
        L.g = g;
        const rk_seqs S = rk_row_seqs<false>(A, M.seq, t);
        if (!S.ok) { ks_first_bad(A.bad, ST_BAD_ROW, row); return; }
        if (S.Lq > RA_MAX_LEN || S.Lt > RA_MAX_LEN) { ks_first_bad(A.bad, ST_BAD_LEN, row); return; }
        const u64 qs = A.a_qs[g], ql = A.a_ql[g], ts = A.a_ts[g], tl = A.a_tl[g];
        if (ql == 0 || tl == 0 || qs + ql > S.Lq || ts + tl > S.Lt) { ks_first_bad(A.bad, ST_BAD_EXT, g); return; }
        const u64 p_start = M.phase + U * qs, p_end = p_start + U * ql; // (<= 3 * 2^20 + 2)
        u64 E = 0, pte = 0, Lqp = S.Lq;
        if (!first) {
            st_member P;
            if (!C::template member<false>(A, F, row, j - 1, q, t, P)) return; // (its own thread names it, as below)
            E = P.phase + U * ((u64)A.a_qs[P.g] + A.a_ql[P.g]); pte = (u64)A.a_ts[P.g] + A.a_tl[P.g];
            if (U > 1) { // (the member in front may lie in another sequence of the row)
                const rk_seqs Sp = rk_row_seqs<false>(A, P.seq, t);
                if (!Sp.ok || Sp.Lq > RA_MAX_LEN) return;
                Lqp = Sp.Lq;
                if (E / U > Lqp) return;
            }
            if (p_end < E || ts + tl < pte) { ks_first_bad(A.bad, ST_BAD_ASC, j); return; }
        }
        const u64 ob = A.g_offs[g], oe = A.g_offs[g + 1];
        if (ob > oe || oe > A.n_gops) { ks_first_bad(A.bad, ST_BAD_OPS, g); return; }
        const u32 nops = (u32)(oe - ob < 0xffffffffULL ? oe - ob : 0xffffffffULL);
        // one walk: what the ops consume, their codes, and the trim (a query-consuming column moves the position by U)
        u64 cq = 0, ct = 0, pos = p_start, tpos = ts;
        bool done = first, bad_code = false, bad_op = false;
        if (first) { L.kop = 0; L.krem = nops ? A.g_ops[ob] >> 4 : 0u; }
        for (u32 k = 0; k < nops; k++) {
            const u32 op = A.g_ops[ob + k], len = op >> 4, code = op & 15u;
            const bool pair = rp_is_pair(code);
            if (!pair && code != RP_I && code != RP_D) bad_op = true;
            if (pair && (A.eqx ? code == RP_M : code != RP_M)) bad_code = true;
            const u64 dq = pair || code == RP_I ? 1u : 0u, dt = pair || code == RP_D ? 1u : 0u;
            cq += len * dq; ct += len * dt;
            if (done) continue;
            const u64 needq = pos >= E ? 0 : (E - pos + U - 1u) / U, needt = tpos >= pte ? 0 : pte - tpos; // columns
            const u64 n = needq > needt ? needq : needt;
            if ((needq == 0 || dq) && (needt == 0 || dt) && n <= len) {
                done = true;
                L.kop = k; L.krem = len - (u32)n; L.trim += (u32)n;
                pos += U * n * dq; tpos += n * dt;
            } else { L.trim += len; pos += U * len * dq; tpos += len * dt; }
        }
        if (bad_op || cq != ql || ct != tl) { ks_first_bad(A.bad, ST_BAD_OPS, g); return; }
        if (bad_code) { ks_first_bad(A.bad, ST_BAD_CODE, g); return; }
        if (!done) { L.kop = nops; L.krem = 0; } // (no column is left: the position is the member's end)
        if (first) return;
        // (ends that do not descend and ops that consume the extents: pos >= E and tpos >= pte hold)
        const u64 X = pos - E, Y = tpos - pte, c = X / U;
        L.c = (u32)c; L.Y = (u32)Y;
        C::keep(L, (u32)(X % U), (u32)E, (u32)pte);
        if (U > 1 && E / U + c > Lqp) { ks_first_bad(A.bad, ST_BAD_EXT, g); return; } // (the link's columns lie inside the previous member's sequence)
        const u64 lo = c < Y ? c : Y, hi = c < Y ? Y : c;
        if (hi == 0) L.cls = ST_L_NONE;
        else if (Y == 0) L.cls = ST_L_I;
        else if (c == 0) L.cls = ST_L_D;
        else if (lo <= RF_SHORT_MAX && hi <= A.max_fill) {
            L.cls = c < Y ? ST_L_FILL_SWAP : ST_L_FILL;
            nr = rp_even((u32)hi); nc = (u32)(c + Y);
        } else L.cls = ST_L_OPEN;
    }();
    links[j] = L; rows[j] = nr; ncols[j] = nc;
}

struct st_slice {
    const u64 *dir_off, *col_off; // n_chained + 1: rows of directions / columns before member j
    u8 *dir, *cols;
    u64 dir_base;                 // dir_off[j0]
    u32 j0, j1;
};

template <class C> __global__ __launch_bounds__(ST_THREADS) void st_fill(st_args A, typename C::link *links, st_slice Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    __shared__ uint4 s_stage[ST_THREADS / 64][RP_STAGE * RA_DIR_ROW / 16];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 j64 = (u64)Z.j0 + (u64)blockIdx.x * (ST_THREADS / 64) + wave;
    if (j64 >= Z.j1) return;
    const u32 j = (u32)j64;
    const u32 cls = ks_readfirst(links[j].cls);
    if (cls != ST_L_FILL && cls != ST_L_FILL_SWAP) return;
    // (behind the plan's wait: the member, the one before it and their row have passed every check)
    const u32 c = ks_readfirst(links[j].c), Y = ks_readfirst(links[j].Y);
    u32 E, pte; // the ends of the member in front
    C::ends_of(A, links, j, E, pte);
    const u32 row = ks_readfirst(ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j));
    const u32 q = ks_readfirst(A.qid[row]), t = ks_readfirst(A.tid[row]);
    const u8 *const qst = A.q_res + rk_readfirst64(A.q_offs[C::seq_at(q, E)]) + E / C::UNIT, *const tst = A.t_res + rk_readfirst64(A.t_offs[t]) + pte;
    u8 *const dir = Z.dir + (rk_readfirst64(Z.dir_off[j]) - Z.dir_base) * RA_DIR_ROW;
    u8 *const col = Z.cols + rk_readfirst64(Z.col_off[j]);
    rf_fill(rf_rect_of(c, Y, cls == ST_L_FILL_SWAP), qst, tst, A.o, A.e, A.eqx, dir, col, c + Y, s_cls, s_M, s_stage[wave], lane, [=](u32 n) {
        if (n == RP_BAD) {
            if (lane == 0) { ks_first_bad(A.bad, ST_BAD_WALK, j); links[j].ncol = 0; }
        } else if (lane == 0) links[j].ncol = n;
    });
}

struct st_out {
    const u64 *col_off;
    const u8 *cols;
    u32 *n_ops;        // !WRITE: the ops of row r
    const u64 *op_off; // WRITE: their exclusive scan, and the ops
    u32 *ops;
    u32 *t_start, *t_length, *n_members, *n_filled, *n_open, *n_trimmed;
};

template <class C, bool WRITE>
__global__ __launch_bounds__(ST_THREADS) void st_emit(st_args A, typename C::ext F, const typename C::link *links, st_out Z, typename C::spans P) {
    const u64 r64 = (u64)blockIdx.x * ST_THREADS + threadIdx.x;
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
        cur = 0xffu;
    };
    auto push = [&](u32 code, u32 cnt) {
        if (cnt == 0) return;
        if (code == cur) { len += cnt; return; } // (a joint merges)
        flush();
        cur = code; len = cnt;
    };
    u32 n_filled = 0, n_open = 0, n_trim = 0, n_shift = 0;
    for (u64 j = b; j < e; j++) {
        const typename C::link L = links[j];
        n_trim += L.trim;
        if (j > b) {
            if (L.cls == ST_L_I) push(RP_I, L.c);
            else if (L.cls == ST_L_D) push(RP_D, L.Y);
            else if (L.cls == ST_L_OPEN) { push(RP_I, L.c); push(RP_D, L.Y); n_open++; }
            else if (L.cls == ST_L_FILL || L.cls == ST_L_FILL_SWAP) {
                const u8 *path = Z.cols + Z.col_off[j] + (L.c + L.Y - L.ncol);
                for (u32 k = 0; k < L.ncol; k++) push(path[k], 1u);
                n_filled++;
            }
            if constexpr (C::UNIT > 1)
                if (L.r) { // the skipped units: an op of its own, merged with nothing
                    flush();
                    if (WRITE && n < room) Z.ops[o + n] = (L.r << 4) | ST_N;
                    n++; n_shift++;
                }
        }
        const u64 ob = A.g_offs[L.g];
        const u32 nops = (u32)(A.g_offs[L.g + 1] - ob);
        for (u32 k = L.kop; k < nops; k++) {
            const u32 op = A.g_ops[ob + k];
            push(op & 15u, k == L.kop ? L.krem : op >> 4);
        }
    }
    flush();
    if (WRITE) return;
    Z.n_ops[r] = n;
    u32 g0 = 0, g1 = 0, ts = 0, te = 0;
    if (e > b) {
        g0 = links[b].g; g1 = links[e - 1].g;
        ts = A.a_ts[g0]; te = A.a_ts[g1] + A.a_tl[g1];
    }
    C::write_spans(A, F, P, r, b, e, g0, g1, n_shift);
    Z.t_start[r] = ts; Z.t_length[r] = te - ts;
    Z.n_members[r] = (u32)(e - b); Z.n_filled[r] = n_filled; Z.n_open[r] = n_open; Z.n_trimmed[r] = n_trim;
}

struct st_cols {
    const u64 *op_off;
    const u32 *ops, *p_start, *t_start; // p_start: a row's start on the query axis
    i64 *score;
    u32 *identities, *positives, *gap_opens, *gaps, *aln_length;
    double *row_score;
};

template <class C> __global__ __launch_bounds__(ST_THREADS) void st_rescore(st_args A, typename C::ext F, st_cols Z) {
    constexpr u32 U = C::UNIT;
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 r64 = (u64)blockIdx.x * (ST_THREADS / 64) + wave;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    const u64 ob = rk_readfirst64(Z.op_off[r]), oe = rk_readfirst64(Z.op_off[r + 1]);
    const bool empty = rk_readfirst64(A.c_offs[r]) == rk_readfirst64(A.c_offs[r + 1]);
    int sc = 0; // (at most 2^21 columns of |M| <= 128 over the lanes: 32 bits)
    u32 id = 0, po = 0, opens = 0, gaps = 0, alen = 0;
    i64 cost = 0;
    if (!empty) {
        // (a row with members has passed the plan: every pair of its ops lies inside a sequence of the row's axis and inside the target)
        const u32 q = ks_readfirst(A.qid[r]), t = ks_readfirst(A.tid[r]);
        const u8 *const f0 = A.q_res + rk_readfirst64(A.q_offs[C::seq_at(q, 0u)]);
        const u8 *const f1 = U > 1 ? A.q_res + rk_readfirst64(A.q_offs[C::seq_at(q, 1u)]) : f0;
        const u8 *const f2 = U > 2 ? A.q_res + rk_readfirst64(A.q_offs[C::seq_at(q, 2u)]) : f0;
        u32 p0 = ks_readfirst(Z.p_start[r]); // the position of the next column on the query axis
        const u8 *tp = A.t_res + rk_readfirst64(A.t_offs[t]) + ks_readfirst(Z.t_start[r]);
        for (u64 k = ob; k < oe; k++) {
            const u32 op = ks_readfirst(Z.ops[k]), len = op >> 4, code = op & 15u;
            if constexpr (U > 1) // (F.fcost: what an N op costs the score)
                if (code == ST_N) { p0 += len; cost += (i64)F.fcost; continue; }
            alen += len;
            if (rp_is_pair(code)) {
                for (u32 c = lane; c < len; c += 64) {
                    const u32 p = p0 + U * c, f = p % U; // this column's residue: p / U of the sequence p lies in
                    const u32 a = (f == 0 ? f0 : f == 1 ? f1 : f2)[p / U], b = tp[c];
                    const int s = s_M[s_cls[a] * RK_A + s_cls[b]];
                    sc += s; id += rk_upper(a) == rk_upper(b) ? 1u : 0u; po += s > 0 ? 1u : 0u;
                }
                p0 += U * len; tp += len;
            } else {
                opens++; gaps += len; cost += (i64)A.o + (i64)len * A.e;
                if (code == RP_I) p0 += U * len; else tp += len;
            }
        }
    }
    const i64 total = (i64)(int)ks_wave_sum32((u32)sc) - cost;
    id = ks_wave_sum32(id); po = ks_wave_sum32(po);
    if (lane == 0) {
        Z.score[r] = total; Z.identities[r] = id; Z.positives[r] = po; Z.gap_opens[r] = opens; Z.gaps[r] = gaps; Z.aln_length[r] = alen;
        Z.row_score[r] = empty ? ks_nan() : (double)total;
    }
}

// The driver of both passes, from the result's allocation to the last wait.  F: the policy's extra kernel arguments.
template <class C>
int st_run(ks_ctx *ctx, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
           u32 max_fill, u32 flags, u64 max_scratch_bytes, const typename C::ext &F, typename C::result *R) {
    const u64 n_rows = K->n_rows, nm = K->n_chained;
    R->n_rows = n_rows; R->n_ops = 0; R->dir_bytes = 0; R->n_slices = 0;
    KS_TRY(ks_alloc(ctx, &R->d_op_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, R, R->n_rows));
    if (n_rows == 0) {
        KS_HIP(ctx, hipMemsetAsync(R->d_op_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    KS_TRY(rk_counts_check(ctx, C::pass, n_rows, S->n_regions));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    ks_ctl ctl;
    typename C::link *links = nullptr;
    u32 *rows = nullptr, *ncols = nullptr, *row_ops = nullptr;
    u64 *dir_off = nullptr, *col_off = nullptr;
    KS_TRY(rk_upload_matrix(ctx, sc, S->matrix, &d_M));
    KS_TRY(ctl.init(ctx, sc, C::pin, ST_N_BAD, 0));
    KS_TRY(sc.alloc(&links, (size_t)nm)); KS_TRY(sc.alloc(&rows, (size_t)nm)); KS_TRY(sc.alloc(&ncols, (size_t)nm));
    KS_TRY(sc.alloc(&dir_off, (size_t)nm + 1)); KS_TRY(sc.alloc(&col_off, (size_t)nm + 1));
    KS_TRY(sc.alloc(&row_ops, (size_t)n_rows));

    st_args A;
    A.c_offs = K->d_row_offsets; A.c_src = K->d_src_region;
    A.a_qs = S->d_qstart; A.a_ql = S->d_qlength; A.a_ts = S->d_tstart; A.a_tl = S->d_tlength;
    A.g_offs = G->d_op_offsets; A.g_ops = G->d_ops;
    A.qid = H->d_qid; A.tid = H->d_tid;
    A.q_res = Q.res; A.t_res = T.res; A.q_offs = Q.offs; A.t_offs = T.offs;
    A.matrix = d_M;
    A.n_q_res = Q.n_res; A.n_t_res = T.n_res; A.n_gops = G->n_ops;
    A.n_rows = (u32)n_rows; A.n_chained = (u32)nm; A.n_regions = (u32)S->n_regions; A.n_q = Q.n_seqs; A.n_t = T.n_seqs;
    A.o = S->gap_open; A.e = S->gap_extend; A.max_fill = max_fill; A.eqx = (flags & KS_RSTITCH_EQX) ? 1u : 0u;
    A.bad = ctl.words();

    u64 *const rb = ctx->h_pin + C::pin + ST_N_BAD; // direction rows | columns | ops
    rb[0] = rb[1] = rb[2] = 0;
    u8 *dir = nullptr, *cols = nullptr;
    if (nm) {
        KS_LAUNCH(ctx, C::k_plan, st_plan<C>, (u32)((nm + ST_THREADS - 1) / ST_THREADS), ST_THREADS, A, F, links, rows, ncols);
        KS_TRY(ks_scan_u32_to_u64_wide(ctx, rows, dir_off, nm)); // (the directions are made in slices: no allocation bounds their sum)
        KS_TRY(ks_scan_u32_to_u64(ctx, ncols, col_off, nm));
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(dir_off + nm, rb, 2), ks_fetch_words(col_off + nm, rb + 1, 2)}));
        for (u32 why = 0; why < ST_BAD_WALK; why++)
            if (ctl.bad(why)) return C::refuse(ctx, why, ctl[why], A.eqx != 0, S->n_regions, Q, T);
        const u64 total_rows = rb[0], total_cols = rb[1];

        // slices of consecutive members whose directions fit the budget
        const u64 budget_rows = (max_scratch_bytes ? max_scratch_bytes : (u64)1 << 30) / RA_DIR_ROW;
        rp_slices Sl;
        KS_TRY(rp_slices_of(ctx, dir_off, nm, total_rows, budget_rows, &Sl));
        if (Sl.bad < nm)
            return ks_fail(ctx, KS_ERR_CAPACITY, C::budget_fmt, (unsigned long long)Sl.bad, (unsigned long long)(Sl.bad_rows * RA_DIR_ROW),
                           (unsigned long long)(budget_rows * RA_DIR_ROW));
        const std::vector<u64> &cut = Sl.cut, &first_row = Sl.first_row;
        const u64 slice_rows = Sl.max_rows;
        KS_TRY(sc.alloc(&dir, (size_t)(slice_rows * RA_DIR_ROW)));
        KS_TRY(sc.alloc(&cols, (size_t)total_cols));
        R->dir_bytes = slice_rows * RA_DIR_ROW; R->n_slices = (u32)(cut.size() - 1);
        if (total_rows)
            for (size_t i = 0; i + 1 < cut.size(); i++) { // (one block for all slices: the launches are ordered by the stream)
                const st_slice Z{dir_off, col_off, dir, cols, first_row[i], (u32)cut[i], (u32)cut[i + 1]};
                KS_LAUNCH(ctx, C::k_fill, st_fill<C>, (u32)((cut[i + 1] - cut[i] + ST_THREADS / 64 - 1) / (ST_THREADS / 64)), ST_THREADS, A, links, Z);
            }
    }

    // the ops per row, their scan = op_offsets, the ops, the columns
    const u32 grid = (u32)((n_rows + ST_THREADS - 1) / ST_THREADS);
    st_out E{col_off, cols, row_ops, R->d_op_offsets, nullptr, R->d_t_start, R->d_t_length, R->d_n_members, R->d_n_filled, R->d_n_open, R->d_n_trimmed};
    const typename C::spans P = C::spans_of(R);
    KS_LAUNCH(ctx, C::k_count, (st_emit<C, false>), grid, ST_THREADS, A, F, (const typename C::link *)links, E, P);
    KS_TRY(ks_scan_u32_to_u64(ctx, row_ops, R->d_op_offsets, n_rows));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(R->d_op_offsets + n_rows, rb + 2, 2)}));
    if (ctl.bad(ST_BAD_WALK)) return ks_fail(ctx, KS_ERR_HIP, C::walk_fmt, (unsigned long long)ctl[ST_BAD_WALK]);
    R->n_ops = rb[2];
    KS_TRY(ks_alloc(ctx, &R->d_ops, (size_t)R->n_ops));
    E.ops = R->d_ops;
    KS_LAUNCH(ctx, C::k_ops, (st_emit<C, true>), grid, ST_THREADS, A, F, (const typename C::link *)links, E, P);
    const st_cols Y{R->d_op_offsets, R->d_ops, C::axis_start(R), R->d_t_start, R->d_score, R->d_identities, R->d_positives, R->d_gap_opens,
                    R->d_gaps, R->d_aln_length, R->d_row_score};
    KS_LAUNCH(ctx, C::k_rescore, st_rescore<C>, (u32)((n_rows + ST_THREADS / 64 - 1) / (ST_THREADS / 64)), ST_THREADS, A, F, Y);
    return ks_stream_wait(ctx);
}
