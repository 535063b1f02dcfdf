// ks_ralign.hip — ks_regions_align: every region of a ks_regions extended WITH gaps from the middle pair of its seed, in both
// directions, by a banded affine-gap dynamic program under a row-level X-drop rule (include/kmerseek_amd.h has the semantics;
// all of it in integers).  The gapped stage behind ks_rscore.hip's ungapped one.  The path itself is ks_rtrace.hip's
// (ks_regions_traceback), from the options this pass records in its result.
//
// One kernel, a wave per region, the shape of k_rscore: the class table and the matrix in LDS, the region's row and sequences
// through rk_locate (ks_rkit.h), everything a wave decides in scalar registers.  The extension itself — lanes, state, residues,
// result, and why 32 bits are enough — is ra_extend<false> of ks_ralign_kit.h.
//
// ks_regions_align_profile is the same kernel with the other scorer (ra_by_profile): no matrix in LDS, the chunk's profile rows
// in the wave's own LDS rows, the anchor pair from the profile's row of the anchor.
#include "ks_ralign_kit.h"

struct ra_args {
    rk_in in;
    u32 W, o, e, x_drop;
    u32 *o_qs, *o_ql, *o_ts, *o_tl, *o_ident, *o_pos, *o_gopen, *o_gaps, *o_len;
    i64 *o_score;
    unsigned long long *bad; // [0] the first row rk_locate refuses, [1] the first row with a sequence longer than RA_MAX_LEN
};

template <bool PROFILE> __global__ __launch_bounds__(RA_THREADS) void k_ralign(ra_args A) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[PROFILE ? 4 : RK_A * RK_A];
    __shared__ unsigned short s_strip[RA_THREADS / 64][RA_STRIP];
    __shared__ u32 s_rows[RA_THREADS / 64][PROFILE ? RA_CHUNK * RA_ROW_WORDS : 1];
    if (PROFILE) rk_stage_classes(s_cls);
    else rk_stage_tables(A.in.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 g64 = (u64)blockIdx.x * (RA_THREADS / 64) + wave;
    if (g64 >= A.in.n_regions) return;
    const u32 g = (u32)g64;
    const rk_at P = rk_locate(A.in, g); // nothing below reads outside the two sequences it names
    const bool too_long = P.ok && (P.Lq > RA_MAX_LEN || P.Lt > RA_MAX_LEN);
    if (!P.ok || P.n == 0 || too_long) { // (a seed of no residues has no middle pair; ks_match_regions makes none)
        if (lane == 0) {
            ks_first_bad(A.bad, too_long ? 1 : 0, P.row);
            A.o_qs[g] = P.a; A.o_ql[g] = 0; A.o_ts[g] = P.b; A.o_tl[g] = 0; A.o_score[g] = 0; A.o_ident[g] = 0; A.o_pos[g] = 0;
            A.o_gopen[g] = 0; A.o_gaps[g] = 0; A.o_len[g] = 0;
        }
        return;
    }
    const u32 ai = P.a + P.n / 2, bj = P.b + P.n / 2, Lq = (u32)P.Lq, Lt = (u32)P.Lt; // the anchor pair: inside the seed
    const u8 *qa = A.in.q_res + P.qb + ai, *ta = A.in.t_res + P.tb + bj;
    const u32 cq = ks_readfirst(*qa), ct = ks_readfirst(*ta);
    const ra_scorer<PROFILE> sc = ra_scorer_of<PROFILE>(A.in.matrix, P.qb + ai, s_M, s_rows[wave]);
    const int s = ra_anchor_score<PROFILE>(A.in.matrix, P.qb + ai, s_cls, s_M, cq, ct);
    const ra_ext R = ra_extend<false>(qa, ta, 1, Lq - 1 - ai, Lt - 1 - bj, A, s_cls, sc, s_strip[wave], lane);
    const ra_ext L = ra_extend<false>(qa, ta, -1, ai, bj, A, s_cls, sc, s_strip[wave], lane);
    if (lane == 0) {
        const u32 gaps = L.c.ga + R.c.ga;
        A.o_qs[g] = ai - L.x; A.o_ql[g] = L.x + 1 + R.x; A.o_ts[g] = bj - L.y; A.o_tl[g] = L.y + 1 + R.y;
        A.o_score[g] = (i64)s + L.score + R.score;
        A.o_ident[g] = (rk_upper(cq) == rk_upper(ct) ? 1u : 0u) + L.c.id + R.c.id;
        A.o_pos[g] = (s > 0 ? 1u : 0u) + L.c.po + R.c.po;
        A.o_gopen[g] = L.c.go + R.c.go; A.o_gaps[g] = gaps;
        A.o_len[g] = 1u + (L.x + L.y + R.x + R.y - gaps) / 2u + gaps; // aligned pairs + gap residues
    }
}

int ks_regions_align_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                          const ks_ralign_opts *opts, const ks_profile *prof, ks_raligns *S) {
    const u64 n_rows = R->n_rows, ng = R->n_regions;
    S->n_rows = n_rows; S->n_regions = ng;
    S->band = opts->band; S->gap_open = opts->gap_open; S->gap_extend = opts->gap_extend; S->x_drop = opts->x_drop;
    S->by_profile = prof != nullptr;
    if (prof) memcpy(S->matrix, prof->matrix, sizeof S->matrix);
    else for (int i = 0; i < RK_A * RK_A; i++) S->matrix[i] = opts->matrix ? opts->matrix[i] : (i / RK_A == i % RK_A) ? 1 : -1;
    KS_TRY(ks_alloc(ctx, &S->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, S, S->n_regions));
    KS_HIP(ctx, hipMemcpyAsync(S->d_row_offsets, R->d_row_offsets, ((size_t)n_rows + 1) * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    if (ng == 0) return ks_stream_wait(ctx);
    KS_TRY(rk_counts_check(ctx, "region alignments", n_rows, ng));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    ks_ctl ctl;
    if (!prof) KS_TRY(rk_upload_matrix(ctx, sc, opts->matrix, &d_M));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RALIGN, 2, 0));

    ra_args A;
    A.in = rk_in_of(R, H, Q, T, prof ? (const signed char *)prof->d_scores : d_M);
    A.W = opts->band; A.o = opts->gap_open; A.e = opts->gap_extend; A.x_drop = opts->x_drop;
    A.o_qs = S->d_qstart; A.o_ql = S->d_qlength; A.o_ts = S->d_tstart; A.o_tl = S->d_tlength; A.o_ident = S->d_identities;
    A.o_pos = S->d_positives; A.o_gopen = S->d_gap_opens; A.o_gaps = S->d_gaps; A.o_len = S->d_aln_length; A.o_score = S->d_score;
    A.bad = ctl.words();
    const u32 grid = (u32)((ng + RA_THREADS / 64 - 1) / (RA_THREADS / 64));
    if (prof) KS_LAUNCH(ctx, "ralign_profile", k_ralign<true>, grid, RA_THREADS, A);
    else KS_LAUNCH(ctx, "ralign", k_ralign<false>, grid, RA_THREADS, A);
    const ks_fetch_seg f = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (ctl.bad(0)) return rk_fail_bad_row(ctx, "region alignments", ctl[0], Q, T);
    if (ctl.bad(1))
        return ks_fail(ctx, KS_ERR_CAPACITY, "region alignments: hit row %llu has a query or target sequence of more than 2^20 residues",
                       (unsigned long long)ctl[1]);
    return KS_OK;
}

extern "C" uint32_t ks_debug_ralign_chunk(void) { return RA_CHUNK; }

int ks_refuse_by_profile(ks_ctx *ctx, const char *pass, const ks_raligns *S) {
    if (!S || !S->by_profile) return KS_OK;
    return ks_fail(ctx, KS_ERR_INVALID_ARG,
                   "%s: the alignments were made against a profile (ks_regions_align_profile): this pass reads residues under a matrix; "
                   "their path is ks_regions_traceback_profile's", pass);
}
