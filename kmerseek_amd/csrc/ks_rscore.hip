// ks_rscore.hip — ks_regions_score: every region of a ks_regions scored under a substitution matrix and, on request, extended
// without gaps in both directions under an X-drop rule (include/kmerseek_amd.h has the semantics; all of it in integers).
//
// One kernel, a wave per region.  The class table (256 B) and the matrix (784 B) sit in LDS.  The region's hit row — its
// (qid, tid) — is the last row whose offset is <= the region's index (rows without a region are never found, a row with
// thousands of regions is found by each of them alike).  Lanes take consecutive positions: each side is one coalesced byte
// stream, the left extension reads descending addresses.
//   core       lane l sums the pairs l, l + 64, ...; one wave reduction for the score, one for the two counts
//   extension  in steps of RS_STEP = 64 positions: inclusive scan of s -> the running sum S_j relative to the step's start; a
//              running-max scan of that -> B_j; a ballot of B_j - S_j > x_drop -> the first terminating lane, where the walk
//              ends.  The best prefix (its sum, its length, its counts) is carried across steps and replaced only by a
//              strictly larger sum: a maximum attained again later never wins against the shorter extension.
// The sums inside a step fit 32 bits (64 x 128); across steps S and B are i64.  Everything a wave decides is wave-uniform and
// kept in scalar registers (readfirstlane): the ballots and the DPP scans see whole waves.
//
// ks_regions_score_profile is the same kernel with the other scorer (ks_rkit.h: rk_by_matrix / rk_by_profile): no matrix in LDS,
// a pair reads P[batch position of Q_x][class(T_y)] from the profile's rows, a gather behind the target byte.
#include "ks_rkit.h"

#define RS_THREADS 256
#define RS_STEP 64     // positions a wave examines per extension step (ks_debug_rscore_step)
#define RS_A RK_A
#define RS_BIAS 8192   // RS_STEP * 128: a step's relative sums + RS_BIAS are >= 0, so a max scan may fill with 0

struct rs_args {
    rk_in in;
    u32 extend, x_drop;
    u32 *o_a, *o_b, *o_n, *o_ident, *o_pos, *o_core_ident;
    i64 *o_score;
    unsigned long long *bad; // the first row whose regions do not lie inside its sequences
};

struct rs_ext { u32 len; i64 score; u32 ident, pos; };

// One side's extension (all 64 lanes enter; every argument but `lane` is wave-uniform).  Pair j = 1 .. e_max is
// (qp[sgn * j], tp[sgn * j]): the caller points qp / tp at the position next to the core on the other side of the walk; qx is
// the batch position of qp[0].
template <class SC>
KS_DEV rs_ext rs_extend(const u8 *qp, const u8 *tp, u64 qx, i64 sgn, u32 e_max, u32 x_drop, const SC &sc, u32 lane) {
    i64 S = 0, B = 0;                  // the sum before this step; the best prefix sum so far (S_0 = 0 is one)
    u32 best = 0, id_best = 0, po_best = 0, id_seen = 0, po_seen = 0; // the best prefix's length and counts; the counts before this step
    for (u32 base = 0; base < e_max; base += RS_STEP) {
        const u32 left = e_max - base, nv = left < RS_STEP ? left : RS_STEP; // lanes with a pair
        const bool valid = lane < nv;
        int s = 0;
        bool idt = false;
        if (valid) {
            const i64 o = sgn * (i64)((u64)base + lane + 1);
            const u32 cq = qp[o], ct = tp[o];
            s = sc.pair(qx + (u64)o, cq, ct);
            idt = rk_upper(cq) == rk_upper(ct);
        }
        const u32 rel = ks_wave_incl_scan((u32)s); // S_j - S, an i32
        const u32 biased = rel + RS_BIAS;
        const u32 rmax = ks_wave_incl_max(biased);
        const i64 Sj = S + (i32)rel, Bs = S + (i64)rmax - RS_BIAS, Bj = Bs > B ? Bs : B;
        const u64 term = __ballot(valid && Bj - Sj > (i64)x_drop);
        const u32 last = ks_readfirst(term ? (u32)__ffsll((long long)term) - 1u : nv - 1u); // the lane of J, or of e_max
        const u32 rmax_last = (u32)__builtin_amdgcn_readlane((int)rmax, (int)last);
        const u64 in = ks_lanes_below(last + 1);
        const u64 idm = __ballot(idt) & in, pom = __ballot(valid && s > 0) & in;
        const i64 Bstep = S + (i64)rmax_last - RS_BIAS;
        if (Bstep > B) { // (strictly: an equal sum of an earlier step is the shorter extension)
            const u64 at = __ballot(biased == rmax_last) & in; // (not empty: the maximum over the lanes <= last is attained there)
            const u32 l = (u32)__ffsll((long long)at) - 1u;
            const u64 upto = ks_lanes_below(l + 1);
            B = Bstep; best = base + l + 1;
            id_best = id_seen + (u32)__popcll((long long)(idm & upto)); po_best = po_seen + (u32)__popcll((long long)(pom & upto));
        }
        if (term) break;
        id_seen += (u32)__popcll((long long)idm); po_seen += (u32)__popcll((long long)pom);
        S += (i32)(u32)__builtin_amdgcn_readlane((int)rel, 63);
    }
    return {best, B, id_best, po_best};
}

template <bool PROFILE> __global__ __launch_bounds__(RS_THREADS) void k_rscore(rs_args A) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[PROFILE ? 4 : RS_A * RS_A];
    if (PROFILE) rk_stage_classes(s_cls);
    else rk_stage_tables(A.in.matrix, s_cls, s_M);
    __syncthreads();
    const std::conditional_t<PROFILE, rk_by_profile, rk_by_matrix> sc{s_cls, PROFILE ? A.in.matrix : s_M};
    const u32 lane = threadIdx.x & 63;
    const u64 g64 = (u64)blockIdx.x * (RS_THREADS / 64) + ks_readfirst(threadIdx.x >> 6);
    if (g64 >= A.in.n_regions) return;
    const u32 g = (u32)g64;
    const rk_at P = rk_locate(A.in, g); // nothing below reads outside the two sequences it names
    const u32 a = P.a, b = P.b, n = P.n;
    const u64 Lq = P.Lq, Lt = P.Lt;
    if (!P.ok) {
        if (lane == 0) {
            ks_first_bad(A.bad, 0, P.row);
            A.o_a[g] = a; A.o_b[g] = b; A.o_n[g] = n; A.o_score[g] = 0; A.o_ident[g] = 0; A.o_pos[g] = 0; A.o_core_ident[g] = 0;
        }
        return;
    }
    const u8 *qc = A.in.q_res + P.qb + a, *tc = A.in.t_res + P.tb + b; // the core's first pair
    i64 sum = 0;
    u32 id = 0, po = 0;
    for (u64 i = lane; i < n; i += 64) {
        const u32 cq = qc[i], ct = tc[i];
        const int s = sc.pair(P.qb + a + i, cq, ct);
        sum += s; id += rk_upper(cq) == rk_upper(ct) ? 1u : 0u; po += s > 0 ? 1u : 0u;
    }
    i64 score = (i64)ks_wave_sum64((u64)sum);
    const u64 counts = ks_wave_sum64(((u64)id << 32) | po); // (each below 2^32: n is a u32)
    const u32 core_ident = (u32)(counts >> 32);
    u32 ident = core_ident, pos = (u32)counts, left = 0, right = 0;
    if (A.extend) {
        const u64 er = Lq - ((u64)a + n) < Lt - ((u64)b + n) ? Lq - ((u64)a + n) : Lt - ((u64)b + n);
        const rs_ext R = rs_extend(qc + n - 1, tc + n - 1, P.qb + a + n - 1, 1, (u32)er, A.x_drop, sc, lane);
        const rs_ext L = rs_extend(qc, tc, P.qb + a, -1, a < b ? a : b, A.x_drop, sc, lane);
        left = L.len; right = R.len;
        score += L.score + R.score; ident += L.ident + R.ident; pos += L.pos + R.pos;
    }
    if (lane == 0) {
        A.o_a[g] = a - left; A.o_b[g] = b - left; A.o_n[g] = left + n + right;
        A.o_score[g] = score; A.o_ident[g] = ident; A.o_pos[g] = pos; A.o_core_ident[g] = core_ident;
    }
}

int ks_regions_score_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                          const ks_rscore_opts *opts, const ks_profile *prof, ks_rscores *S) {
    const u64 n_rows = R->n_rows, ng = R->n_regions;
    S->n_rows = n_rows; S->n_regions = ng;
    KS_TRY(ks_alloc(ctx, &S->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, S, S->n_regions));
    KS_HIP(ctx, hipMemcpyAsync(S->d_row_offsets, R->d_row_offsets, ((size_t)n_rows + 1) * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    if (ng == 0) return ks_stream_wait(ctx);
    KS_TRY(rk_counts_check(ctx, "region scores", n_rows, ng));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    u64 *bad = nullptr;
    if (!prof) KS_TRY(rk_upload_matrix(ctx, sc, opts ? opts->matrix : nullptr, &d_M));
    KS_TRY(sc.alloc(&bad, 1));
    KS_HIP(ctx, hipMemsetAsync(bad, 0xff, sizeof(u64), ctx->stream));

    rs_args A;
    A.in = rk_in_of(R, H, Q, T, prof ? (const signed char *)prof->d_scores : d_M);
    A.extend = opts && (opts->flags & KS_RSCORE_EXTEND) ? 1u : 0u; A.x_drop = opts ? opts->x_drop : 0u;
    A.o_a = S->d_qstart; A.o_b = S->d_tstart; A.o_n = S->d_length; A.o_ident = S->d_identities; A.o_pos = S->d_positives;
    A.o_core_ident = S->d_core_ident; A.o_score = S->d_score; A.bad = (unsigned long long *)bad;
    const u32 grid = (u32)((ng + RS_THREADS / 64 - 1) / (RS_THREADS / 64));
    if (prof) KS_LAUNCH(ctx, "rscore_profile", k_rscore<true>, grid, RS_THREADS, A);
    else KS_LAUNCH(ctx, "rscore", k_rscore<false>, grid, RS_THREADS, A);
    u64 *const hb = ctx->h_pin + KS_PIN_RSCORE;
    const ks_fetch_seg f = ks_fetch_words(bad, hb, 2);
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (*hb != ~0ULL) return rk_fail_bad_row(ctx, "region scores", *hb, Q, T);
    return KS_OK;
}

extern "C" uint32_t ks_debug_rscore_step(void) { return RS_STEP; }

// ---- the host side of ks_rkit.h ----
int rk_counts_check(ks_ctx *ctx, const char *pass, u64 n_rows, u64 n_regions) {
    if (n_rows >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: 2^32 - 2 or more hit rows", pass);
    if (n_regions > 0xffffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: more than 2^32 - 1 regions", pass);
    return KS_OK;
}
int rk_upload_matrix(ks_ctx *ctx, ks_scratch &sc, const int8_t *h_matrix, signed char **d_M) {
    KS_TRY(sc.alloc(d_M, (size_t)RK_A * RK_A));
    signed char h_M[RK_A * RK_A];
    if (h_matrix) memcpy(h_M, h_matrix, sizeof h_M);
    else for (int i = 0; i < RK_A * RK_A; i++) h_M[i] = (i / RK_A == i % RK_A) ? 1 : -1;
    return ks_copy_h2d(ctx, *d_M, h_M, sizeof h_M); // (a pageable source: consumed on return)
}
int rk_profile_check(ks_ctx *ctx, const char *pass, const ks_profile *prof, const ks_res_batch &Q) {
    if (!prof) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, pass, prof));
    if (prof->n_residues != Q.n_res)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: the profile holds %llu residues, the query batch %llu: a profile of another batch", pass,
                       (unsigned long long)prof->n_residues, (unsigned long long)Q.n_res);
    return KS_OK;
}
int rk_fail_bad_row(ks_ctx *ctx, const char *pass, u64 row, const ks_res_batch &Q, const ks_res_batch &T) {
    return ks_fail(ctx, KS_ERR_INVALID_ARG,
                   "%s: hit row %llu names a query or target beyond the batches (%u queries, %u targets) or owns a region that "
                   "does not lie inside its two sequences: regions, hits and batches do not belong together",
                   pass, (unsigned long long)row, Q.n_seqs, T.n_seqs);
}
