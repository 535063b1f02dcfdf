// ks_profile.hip — ks_profile_build_device: the counts of a query-side pileup (ks_pileup.hip, KS_PILEUP_PROFILE) made into one
// row of 28 scores per query residue, with a consensus byte and the observations behind the row (include/kmerseek_amd.h has the
// rule; tests/profile_ref.py restates it in plain loops).  The rows are what ks_regions_score_profile, ks_regions_align_profile
// and ks_regions_traceback_profile read where their siblings read a matrix.
//
// The rule is f64 arithmetic in a fixed order, every operation rounded on its own: the pragma below keeps the compiler from
// contracting a multiply and an add into one fused operation, and a division is the correctly rounded one.  No log, no exp: the
// likelihood ratios and the thresholds come from the host, and a score is a count of thresholds — a binary search.
//
//   build   k_pf_build, a wave takes two residues, 28 lanes each (the lanes 28 .. 31 of a half idle): lane c of a half makes
//           scores[p][c].  The 28 counts of a residue are one coalesced read into the half's own LDS row, from where every lane
//           reads all of them (a broadcast) — for n0 and for the sum g, lane 0 also for the consensus — so no lane waits for
//           another.  One ballot per half-wave tells a residue without any count: it keeps its matrix row and walks nothing.  R,
//           bg, the thresholds and the fallback matrix sit in LDS, staged once by a workgroup that then strides over the batch.
//   weighted  k_pf_build_weighted, the same shape for the weighted rule: a second LDS row holds the residue's 28 weighted
//           counts (u64), the evidence is the number of classes seen and the frequencies are quotients of weight sums.
// One wait before the launch (the batch's last offset against n_q_res: nothing is indexed by a count nobody checked), one after.
#include "ks_rkit.h"

#pragma clang fp contract(off)

#define PF_THREADS 256
#define PF_A RK_A
#define PF_PER_BLOCK (PF_THREADS / 32) // residues a workgroup takes at a time
#define PF_GRID 4096
#define PF_THR KS_PROFILE_MAX_THRESHOLDS

struct pf_tables { // the options on the device, one upload
    double R[PF_A * PF_A], bg[PF_A], thr[PF_THR];
    signed char M[PF_A * PF_A];
};
struct pf_args {
    const u32 *counts, *depth;
    const u8 *q_res;
    u64 n_res;
    const pf_tables *tab;
    double beta;
    u32 n_thr, include_query;
    int base;
    signed char *scores;
    u8 *consensus;
    u32 *n_obs;
    const u64 *wcounts; // the weighted build alone
};

__global__ __launch_bounds__(PF_THREADS) void k_pf_build(pf_args A) {
    __shared__ double s_R[PF_A * PF_A], s_bg[PF_A], s_thr[PF_THR];
    __shared__ signed char s_M[PF_A * PF_A];
    __shared__ u32 s_cnt[PF_PER_BLOCK][32];
    for (u32 i = threadIdx.x; i < PF_A * PF_A; i += PF_THREADS) { s_R[i] = A.tab->R[i]; s_M[i] = A.tab->M[i]; }
    if (threadIdx.x < PF_A) s_bg[threadIdx.x] = A.tab->bg[threadIdx.x];
    if (threadIdx.x < A.n_thr) s_thr[threadIdx.x] = A.tab->thr[threadIdx.x]; // (n_thr <= PF_THR < PF_THREADS)
    __syncthreads();
    const u32 half = threadIdx.x >> 5, c = threadIdx.x & 31;
    u32 *const cnt = s_cnt[half];
    for (u64 p0 = (u64)blockIdx.x * PF_PER_BLOCK; p0 < A.n_res; p0 += (u64)gridDim.x * PF_PER_BLOCK) {
        const u64 p = p0 + half;
        const bool mine = p < A.n_res && c < PF_A;
        __builtin_amdgcn_wave_barrier(); // (the residue before has read the row; same wave: LDS operations execute in order)
        const u32 mine_cnt = mine ? A.counts[p * PF_A + c] : 0u;
        cnt[c] = mine_cnt;
        // one vote per half: a residue nobody was aligned to — most of a batch — keeps its matrix row and walks no counts
        const u64 seen = __ballot(mine_cnt != 0);
        const bool observed = (u32)(seen >> (threadIdx.x & 32)) != 0;
        __builtin_amdgcn_wave_barrier();
        if (!mine) continue;
        const u32 byte = A.q_res[p], a = rk_class(byte);
        // n0 over the modelled classes; the consensus (lane 0 alone) over all of them, the residue's own class counted once more
        u64 n0 = 0;
        u32 top_j = a;
        if (observed) {
            for (u32 j = 0; j < PF_A; j++)
                if (s_bg[j] > 0.0) n0 += cnt[j];
            if (c == 0) {
                u64 top = 0;
                for (u32 j = 0; j < PF_A; j++) {
                    const u64 cc = (u64)cnt[j] + (j == a ? 1u : 0u);
                    if (cc > top) { top = cc; top_j = j; } // (ascending j: a tie stays with the smaller class)
                }
            }
        }
        int score = s_M[a * PF_A + c];
        u64 n = 0;
        if (n0 != 0) {
            const bool inc = A.include_query && s_bg[a] > 0.0;
            n = n0 + (inc ? 1u : 0u);
            if (s_bg[c] > 0.0) {
                double g = 0.0;
                for (u32 j = 0; j < PF_A; j++) {
                    if (!(s_bg[j] > 0.0)) continue;
                    const u64 cj = (u64)cnt[j] + (inc && j == a ? 1u : 0u);
                    g = g + (double)cj * s_R[j * PF_A + c];
                }
                double t = g / (double)n;
                t = s_bg[c] * t;
                t = A.beta * t;
                const u64 cc = (u64)cnt[c] + (inc && c == a ? 1u : 0u);
                const double num = (double)cc + t, den = (double)n + A.beta;
                const double r = (num / den) / s_bg[c];
                u32 lo = 0, hi = A.n_thr; // the thresholds <= r (ascending; a NaN is at or above none)
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if (s_thr[mid] <= r) lo = mid + 1;
                    else hi = mid;
                }
                const i64 v = (i64)A.base + lo;
                score = (int)(v < -127 ? -127 : v > 127 ? 127 : v);
            }
        }
        A.scores[p * PF_A + c] = (signed char)score;
        if (c == 0) {
            A.consensus[p] = (u8)(A.depth[p] == 0 ? rk_upper(byte) : top_j < 26u ? 'A' + top_j : top_j == 26u ? '*' : 'X');
            A.n_obs[p] = n > 0xffffffffULL ? 0xffffffffu : (u32)n;
        }
    }
}

// the classes of cnt[] with a count (own: one class counted once more, PF_A for none), all of them or the modelled ones
KS_DEV u32 pf_classes_seen(const u32 *cnt, const double *bg, u32 own, bool modelled_only) {
    u32 k = 0;
    for (u32 j = 0; j < PF_A; j++)
        if ((!modelled_only || bg[j] > 0.0) && (cnt[j] != 0 || j == own)) k++;
    return k;
}

__global__ __launch_bounds__(PF_THREADS) void k_pf_build_weighted(pf_args A) {
    __shared__ double s_R[PF_A * PF_A], s_bg[PF_A], s_thr[PF_THR];
    __shared__ signed char s_M[PF_A * PF_A];
    __shared__ u32 s_cnt[PF_PER_BLOCK][32];
    __shared__ u64 s_w[PF_PER_BLOCK][32];
    __shared__ double s_x[PF_PER_BLOCK][32]; // x_j of the residue: lane j divides once, every lane reads all of them
    for (u32 i = threadIdx.x; i < PF_A * PF_A; i += PF_THREADS) { s_R[i] = A.tab->R[i]; s_M[i] = A.tab->M[i]; }
    if (threadIdx.x < PF_A) s_bg[threadIdx.x] = A.tab->bg[threadIdx.x];
    if (threadIdx.x < A.n_thr) s_thr[threadIdx.x] = A.tab->thr[threadIdx.x];
    __syncthreads();
    const u32 half = threadIdx.x >> 5, c = threadIdx.x & 31;
    u32 *const cnt = s_cnt[half];
    u64 *const wc = s_w[half];
    double *const xs = s_x[half];
    for (u64 p0 = (u64)blockIdx.x * PF_PER_BLOCK; p0 < A.n_res; p0 += (u64)gridDim.x * PF_PER_BLOCK) {
        const u64 p = p0 + half;
        const bool mine = p < A.n_res && c < PF_A;
        __builtin_amdgcn_wave_barrier();
        const u32 mine_cnt = mine ? A.counts[p * PF_A + c] : 0u;
        cnt[c] = mine_cnt;
        const u64 seen = __ballot(mine_cnt != 0);
        const bool observed = (u32)(seen >> (threadIdx.x & 32)) != 0;
        wc[c] = (mine && observed) ? A.wcounts[p * PF_A + c] : 0ull; // (a class without a count has no weight: not read)
        __builtin_amdgcn_wave_barrier();
        if (!mine) continue;
        const u32 byte = A.q_res[p], a = rk_class(byte);
        u64 n0 = 0;
        u32 top_j = a;
        if (observed) {
            for (u32 j = 0; j < PF_A; j++)
                if (s_bg[j] > 0.0) n0 += cnt[j];
            if (c == 0) { // the consensus: all 28 classes, the query's own column term whatever the flag
                const u32 kq = pf_classes_seen(cnt, s_bg, a, false);
                const u64 own = (u64)KS_WEIGHT_ONE / ((u64)kq * ((u64)cnt[a] + 1u));
                u64 top = 0;
                for (u32 j = 0; j < PF_A; j++) {
                    const u64 v = wc[j] + (j == a ? own : 0ull);
                    if (v > top) { top = v; top_j = j; }
                }
            }
        }
        int score = s_M[a * PF_A + c];
        u64 n = 0;
        if (n0 != 0) {
            const bool inc = A.include_query && s_bg[a] > 0.0;
            const u32 k = pf_classes_seen(cnt, s_bg, inc ? a : PF_A, true); // (n0 != 0: k >= 1)
            const u64 own = inc ? (u64)KS_WEIGHT_ONE / ((u64)k * ((u64)cnt[a] + 1u)) : 0ull;
            u64 W = own;
            for (u32 j = 0; j < PF_A; j++)
                if (s_bg[j] > 0.0) W += wc[j];
            if (W != 0) {
                n = n0 + (inc ? 1u : 0u);
                // (n0, W: one value in the 28 lanes of a residue, which are all here; same wave: LDS operations execute in order)
                const double fk = (double)k;
                const double xc = ((double)(wc[c] + (inc && c == a ? own : 0ull)) / (double)W) * fk;
                xs[c] = xc;
                __builtin_amdgcn_wave_barrier();
                if (s_bg[c] > 0.0) {
                    double g = 0.0;
                    for (u32 j = 0; j < PF_A; j++) {
                        if (!(s_bg[j] > 0.0)) continue;
                        g = g + xs[j] * s_R[j * PF_A + c];
                    }
                    double t = g / fk;
                    t = s_bg[c] * t;
                    t = A.beta * t;
                    const double num = xc + t, den = fk + A.beta;
                    const double r = (num / den) / s_bg[c];
                    u32 lo = 0, hi = A.n_thr;
                    while (lo < hi) {
                        const u32 mid = (lo + hi) >> 1;
                        if (s_thr[mid] <= r) lo = mid + 1;
                        else hi = mid;
                    }
                    const i64 v = (i64)A.base + lo;
                    score = (int)(v < -127 ? -127 : v > 127 ? 127 : v);
                }
            }
        }
        A.scores[p * PF_A + c] = (signed char)score;
        if (c == 0) {
            A.consensus[p] = (u8)(A.depth[p] == 0 ? rk_upper(byte) : top_j < 26u ? 'A' + top_j : top_j == 26u ? '*' : 'X');
            A.n_obs[p] = n > 0xffffffffULL ? 0xffffffffu : (u32)n;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// what the options are refused for (ctx may be NULL), and the tables they make
static int pf_opts_check(ks_ctx *ctx, const ks_profile_opts *o, pf_tables *tab) {
    const auto refuse = [&](const char *why) { return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "profile options: %s", why) : KS_ERR_INVALID_ARG; };
    if (!o) return refuse("NULL: there are no default ratios or thresholds");
    KS_TRY(ks_opts_words_check(ctx, "profile", o->flags, KS_PROFILE_INCLUDE_QUERY, o->reserved));
    if (o->n_thr > KS_PROFILE_MAX_THRESHOLDS) return refuse("n_thr is beyond KS_PROFILE_MAX_THRESHOLDS (254)");
    if (!o->bg || !o->ratio || (o->n_thr && !o->thresholds)) return refuse("bg, ratio or thresholds is NULL");
    if (o->beta != o->beta) return refuse("beta is NaN");
    if (o->beta < 0) return refuse("beta is negative");
    for (int i = 0; i < PF_A; i++) {
        if (o->bg[i] != o->bg[i]) return refuse("a NaN in bg");
        if (o->bg[i] < 0) return refuse("a negative bg");
    }
    for (int i = 0; i < PF_A * PF_A; i++)
        if (o->ratio[i] != o->ratio[i]) return refuse("a NaN in ratio");
    for (u32 k = 0; k < o->n_thr; k++) {
        if (o->thresholds[k] != o->thresholds[k]) return refuse("a NaN among the thresholds");
        if (k && !(o->thresholds[k - 1] < o->thresholds[k])) return refuse("the thresholds do not ascend strictly");
    }
    memset(tab, 0, sizeof *tab);
    memcpy(tab->R, o->ratio, sizeof tab->R);
    memcpy(tab->bg, o->bg, sizeof tab->bg);
    if (o->n_thr) memcpy(tab->thr, o->thresholds, o->n_thr * sizeof(double));
    for (int i = 0; i < PF_A * PF_A; i++) tab->M[i] = o->matrix ? (signed char)o->matrix[i] : (i / PF_A == i % PF_A) ? 1 : -1;
    return KS_OK;
}

// a profile of n_q sequences and n_res residues, its columns allocated, the fallback recorded
static int pf_alloc(ks_ctx *ctx, ks_profile *P, u32 n_q, u64 n_res, const signed char *M) {
    P->n_seqs = n_q; P->n_residues = n_res; P->n_scores = n_res * PF_A;
    memcpy(P->matrix, M, sizeof P->matrix);
    KS_TRY(ks_alloc(ctx, &P->d_scores, (size_t)P->n_scores));
    return ks_obj_alloc(ctx, P, P->n_residues);
}

// weighted: d_wcounts holds the weighted counts, and the rule is the weighted one
static int pf_build(ks_ctx *ctx, const u32 *d_counts, const u32 *d_depth, const ks_res_batch &Q, const ks_profile_opts &o, const pf_tables &tab,
                    ks_profile **out, bool weighted = false, const u64 *d_wcounts = nullptr) {
    if (!out || !Q.offs || (Q.n_res && (!d_counts || !d_depth || !Q.res || (weighted && !d_wcounts)))) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    u64 *const last = ctx->h_pin + KS_PIN_PROFILE;
    const ks_fetch_seg f = ks_fetch_words(Q.offs + Q.n_seqs, last, 2);
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (*last != Q.n_res)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the offsets of the %u sequences end at %llu, n_q_res is %llu: counts of another batch", Q.n_seqs,
                       (unsigned long long)*last, (unsigned long long)Q.n_res);
    ks_result<ks_profile> P(ctx, out, ks_profile_free);
    KS_TRY(pf_alloc(ctx, P, Q.n_seqs, Q.n_res, tab.M));
    if (Q.n_res == 0) return P.commit();
    ks_scratch sc(ctx);
    pf_tables *d_tab = nullptr;
    KS_TRY(sc.alloc(&d_tab, 1));
    KS_TRY(ks_copy_h2d(ctx, d_tab, &tab, sizeof tab)); // (a pageable source: consumed on return)
    const pf_args A = {d_counts, d_depth, Q.res, Q.n_res, d_tab, o.beta, o.n_thr, (o.flags & KS_PROFILE_INCLUDE_QUERY) ? 1u : 0u, o.base,
                       (signed char *)P->d_scores, P->d_consensus, P->d_n_obs, d_wcounts};
    const u64 blocks = (Q.n_res + PF_PER_BLOCK - 1) / PF_PER_BLOCK;
    if (weighted) KS_LAUNCH(ctx, "profile_build_weighted", k_pf_build_weighted, (u32)(blocks < PF_GRID ? blocks : PF_GRID), PF_THREADS, A);
    else KS_LAUNCH(ctx, "profile_build", k_pf_build, (u32)(blocks < PF_GRID ? blocks : PF_GRID), PF_THREADS, A);
    KS_TRY(ks_stream_wait(ctx));
    return P.commit();
}

// What the two builds do alike, in their order: the options (also without a context), the context, *out, the objects (`in`: not
// NULL, of ctx), then `run`.
template <typename Run, typename... In>
static int pf_entry(ks_ctx *ctx, const ks_profile_opts *opts, ks_profile **out, Run &&run, const In *...in) {
    return ks_guard(ctx, [&]() -> int {
    pf_tables tab;
    KS_TRY(pf_opts_check(ctx, opts, &tab));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if ((!in || ...)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if constexpr (sizeof...(In) != 0) KS_TRY(ks_inputs_check_ctx(ctx, "profile", in...));
    return run(tab);
    });
}

extern "C" int ks_profile_build_device(ks_ctx *ctx, const uint32_t *d_counts, const uint32_t *d_depth, const uint8_t *d_q_res,
                                       const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out) {
    return pf_entry(ctx, opts, out, [&](const pf_tables &tab) {
        return pf_build(ctx, d_counts, d_depth, ks_res_batch{d_q_res, d_q_offs, n_q, n_q_res}, *opts, tab, out);
    });
}
extern "C" int ks_profile_build_pileup(ks_ctx *ctx, const ks_pileup *pileup, const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q,
                                       uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out) {
    return pf_entry(ctx, opts, out, [&](const pf_tables &tab) {
        if (pileup->n_profile != pileup->n_residues * PF_A)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the pileup was made without KS_PILEUP_PROFILE: it holds no counts");
        if (pileup->n_seqs != n_q || pileup->n_residues != n_q_res)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the pileup is of %llu sequences and %llu residues, the query batch of %u and %llu: a pileup "
                                                    "of another batch or of the target side",
                           (unsigned long long)pileup->n_seqs, (unsigned long long)pileup->n_residues, n_q, (unsigned long long)n_q_res);
        return pf_build(ctx, pileup->d_counts, pileup->d_depth, ks_res_batch{d_q_res, d_q_offs, n_q, n_q_res}, *opts, tab, out);
    }, pileup);
}
extern "C" int ks_profile_build_weighted_device(ks_ctx *ctx, const uint32_t *d_counts, const uint64_t *d_wcounts, const uint32_t *d_depth,
                                                const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res,
                                                const ks_profile_opts *opts, ks_profile **out) {
    return pf_entry(ctx, opts, out, [&](const pf_tables &tab) {
        return pf_build(ctx, d_counts, d_depth, ks_res_batch{d_q_res, d_q_offs, n_q, n_q_res}, *opts, tab, out, true, d_wcounts);
    });
}
extern "C" int ks_profile_build_weighted_pileup(ks_ctx *ctx, const ks_pileup *pileup, const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q,
                                                uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out) {
    return pf_entry(ctx, opts, out, [&](const pf_tables &tab) {
        if (pileup->n_profile != pileup->n_residues * PF_A)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the pileup was made without KS_PILEUP_PROFILE: it holds no counts");
        if (pileup->n_weighted != pileup->n_residues || pileup->n_wprofile != pileup->n_profile)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the pileup was made without weights: it holds no weighted counts (ks_wpileup_device)");
        if (pileup->n_seqs != n_q || pileup->n_residues != n_q_res)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "profile: the pileup is of %llu sequences and %llu residues, the query batch of %u and %llu: a pileup "
                                                    "of another batch or of the target side",
                           (unsigned long long)pileup->n_seqs, (unsigned long long)pileup->n_residues, n_q, (unsigned long long)n_q_res);
        return pf_build(ctx, pileup->d_counts, pileup->d_depth, ks_res_batch{d_q_res, d_q_offs, n_q, n_q_res}, *opts, tab, out, true, pileup->d_wcounts);
    }, pileup);
}
extern "C" int ks_profile_from_host(ks_ctx *ctx, const int8_t *scores, const uint8_t *consensus, const uint32_t *n_obs, uint32_t n_q,
                                    uint64_t n_q_res, const int8_t *matrix, ks_profile **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!out || (n_q_res && !scores)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    signed char M[PF_A * PF_A];
    for (int i = 0; i < PF_A * PF_A; i++) M[i] = matrix ? (signed char)matrix[i] : (i / PF_A == i % PF_A) ? 1 : -1;
    ks_result<ks_profile> P(ctx, out, ks_profile_free);
    KS_TRY(pf_alloc(ctx, P, n_q, n_q_res, M));
    if (n_q_res) {
        KS_TRY(ks_copy_h2d(ctx, P->d_scores, scores, (size_t)P->n_scores));
        if (consensus) KS_TRY(ks_copy_h2d(ctx, P->d_consensus, consensus, (size_t)n_q_res));
        else KS_HIP(ctx, hipMemsetAsync(P->d_consensus, 0, (size_t)n_q_res, ctx->stream));
        if (n_obs) KS_TRY(ks_copy_h2d(ctx, P->d_n_obs, n_obs, (size_t)n_q_res * sizeof(u32)));
        else KS_HIP(ctx, hipMemsetAsync(P->d_n_obs, 0, (size_t)n_q_res * sizeof(u32), ctx->stream));
    }
    KS_TRY(ks_stream_wait(ctx));
    return P.commit();
    });
}

extern "C" uint32_t ks_profile_n_seqs(const ks_profile *p) { return p ? (u32)p->n_seqs : 0; }
extern "C" uint64_t ks_profile_n_residues(const ks_profile *p) { return p ? p->n_residues : 0; }
extern "C" uint64_t ks_profile_n_scores(const ks_profile *p) { return p ? p->n_scores : 0; }
extern "C" const uint8_t *ks_profile_device_scores(const ks_profile *p) { return p ? (const uint8_t *)p->d_scores : nullptr; }
extern "C" const uint8_t *ks_profile_device_consensus(const ks_profile *p) { return p ? p->d_consensus : nullptr; }
extern "C" const uint32_t *ks_profile_device_n_obs(const ks_profile *p) { return p ? p->d_n_obs : nullptr; }
extern "C" int ks_profile_copy_to_host(ks_ctx *ctx, const ks_profile *p, uint8_t *scores, uint8_t *consensus, uint32_t *n_obs) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, p, scores, consensus, n_obs); });
}
extern "C" void ks_profile_free(ks_profile *p) { ks_obj_free(p); }
