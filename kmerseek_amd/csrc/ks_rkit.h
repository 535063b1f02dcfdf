// ks_rkit.h — what the passes over a ks_regions share (ks_rscore.hip, ks_ralign.hip): the inputs of such a pass as its kernel
// takes them, a region's hit row and its two sequences with the one check that nothing lies outside the batches, the residue
// classes, and the substitution matrix on the device.  One definition: two passes can never disagree on what a bad row is.
#pragma once
#include "ks_device.h"

#define RK_A KS_RSCORE_ALPHABET

struct rk_in {
    const u64 *row_offs;  // n_rows + 1
    const u32 *qid, *tid; // n_rows
    const u32 *a, *b, *n; // n_regions: q_start, t_start, length
    const u8 *q_res, *t_res;
    const u64 *q_offs, *t_offs;
    const signed char *matrix; // device, RK_A x RK_A; in a pass against a profile its scores, n_q_res x RK_A (rk_by_profile)
    u64 n_q_res, n_t_res;
    u32 n_rows, n_regions, n_q, n_t;
};
static inline rk_in rk_in_of(const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T, const signed char *d_M) {
    return rk_in{R->d_row_offsets, H->d_qid, H->d_tid, R->d_qstart, R->d_tstart, R->d_length, Q.res, T.res, Q.offs, T.offs, d_M,
                 Q.n_res, T.n_res, (u32)R->n_rows, (u32)R->n_regions, Q.n_seqs, T.n_seqs};
}

KS_DEV u64 rk_readfirst64(u64 v) { return ((u64)ks_readfirst((u32)(v >> 32)) << 32) | ks_readfirst((u32)v); }
KS_DEV u32 rk_upper(u32 c) { return c - 'a' < 26u ? c - 32u : c; }
KS_DEV u32 rk_class(u32 x) {
    const u32 c = rk_upper(x);
    return c - 'A' < 26u ? c - 'A' : c == '*' ? 26u : 27u;
}
// the class table (256 B) and the matrix (RK_A * RK_A B) into LDS, by a workgroup of 256 threads; the caller synchronises
KS_DEV void rk_stage_tables(const signed char *matrix, u8 *s_cls, signed char *s_M) {
    s_cls[threadIdx.x] = (u8)rk_class(threadIdx.x);
    for (u32 i = threadIdx.x; i < RK_A * RK_A; i += 256) s_M[i] = matrix[i];
}

// The scorer of a pass: what the pair of the query residue at batch position qx (its byte cq) and a target byte ct scores.  Two
// policies on ONE code path (rs_extend and the core loop of k_rscore; ra_by_matrix / ra_by_profile of ks_ralign_kit.h are the
// same pair for ra_extend): the pass against a profile can never break a tie in another way than the pass under a matrix.
//   rk_by_matrix   M[class(Q_x)][class(T_y)], the matrix in LDS; the position is not read
//   rk_by_profile  P[qx][class(T_y)], the profile's rows in global memory; the query byte is not read
struct rk_by_matrix {
    static constexpr bool PROFILE = false;
    const u8 *s_cls;
    const signed char *s_M;
    KS_DEV int pair(u64, u32 cq, u32 ct) const { return s_M[s_cls[cq] * RK_A + s_cls[ct]]; }
};
struct rk_by_profile {
    static constexpr bool PROFILE = true;
    const u8 *s_cls;
    const signed char *P;
    KS_DEV int pair(u64 qx, u32, u32 ct) const { return P[qx * RK_A + s_cls[ct]]; }
};
// the class table alone (a pass against a profile stages no matrix)
KS_DEV void rk_stage_classes(u8 *s_cls) { s_cls[threadIdx.x] = (u8)rk_class(threadIdx.x); }

// Sequences q < I.n_q and t < I.n_t — the caller has checked the two ids — of the batches of I (any struct with q_offs, t_offs,
// n_q_res, n_t_res): their first residues in the batches and their lengths.  ok: both lie inside their batches.  UNIFORM: q
// and t are wave-uniform and every value comes back in scalar registers; a pass with a thread per item asks without it.
struct rk_seqs { u64 qb, tb, Lq, Lt; bool ok; };
template <bool UNIFORM, class In> KS_DEV rk_seqs rk_row_seqs(const In &I, u32 q, u32 t) {
    rk_seqs S;
    S.qb = I.q_offs[q]; S.tb = I.t_offs[t];
    u64 qe = I.q_offs[q + 1], te = I.t_offs[t + 1];
    if (UNIFORM) { S.qb = rk_readfirst64(S.qb); S.tb = rk_readfirst64(S.tb); qe = rk_readfirst64(qe); te = rk_readfirst64(te); }
    S.ok = S.qb <= qe && qe <= I.n_q_res && S.tb <= te && te <= I.n_t_res;
    S.Lq = qe - S.qb; S.Lt = te - S.tb;
    return S;
}

// Region g (wave-uniform; every value comes back in scalar registers): its hit row — the last row whose offset is <= g: rows
// without a region are never found, a row with thousands of regions is found by each of them alike — and its two sequences.
// ok: the region lies inside its two sequences and the sequences inside their batches: a + n <= Lq and b + n <= Lt hold, and
// [qb, qb + Lq) x [tb, tb + Lt) is all a caller may read.
struct rk_at {
    u32 row, a, b, n;
    u64 qb, tb, Lq, Lt; // the sequences' first residues in the batches, their lengths
    bool ok;
};
KS_DEV rk_at rk_locate(const rk_in &I, u32 g) {
    rk_at P;
    P.row = ks_readfirst(ks_last_le_u64(I.row_offs, 0, I.n_rows - 1, g)); // (row_offs[0] == 0 <= g)
    const u32 q = ks_readfirst(I.qid[P.row]), t = ks_readfirst(I.tid[P.row]);
    P.a = ks_readfirst(I.a[g]); P.b = ks_readfirst(I.b[g]); P.n = ks_readfirst(I.n[g]);
    P.ok = q < I.n_q && t < I.n_t;
    P.qb = P.tb = P.Lq = P.Lt = 0;
    if (P.ok) {
        const rk_seqs S = rk_row_seqs<true>(I, q, t);
        P.qb = S.qb; P.tb = S.tb; P.Lq = S.Lq; P.Lt = S.Lt;
        P.ok = S.ok && P.Lq <= 0xffffffffULL && P.Lt <= 0xffffffffULL && (u64)P.a + P.n <= P.Lq && (u64)P.b + P.n <= P.Lt;
    }
    return P;
}

// ---- host side (ks_rscore.hip) ----
// what both passes refuse before any device work beyond the row-offset copy: more rows or regions than 32 bits index
int rk_counts_check(ks_ctx *ctx, const char *pass, u64 n_rows, u64 n_regions);
// the caller's host matrix (NULL: +1 / -1) into a block of `sc`
int rk_upload_matrix(ks_ctx *ctx, ks_scratch &sc, const int8_t *h_matrix, signed char **d_M);
// KS_ERR_INVALID_ARG naming `row`, the first row rk_locate refused
int rk_fail_bad_row(ks_ctx *ctx, const char *pass, u64 row, const ks_res_batch &Q, const ks_res_batch &T);
