// ks_astats.hip — alignment statistics (include/kmerseek_amd.h has the contract): the residue composition of a batch
// (ks_residue_composition_device), the ungapped Karlin-Altschul parameters of a matrix on the host (ks_karlin_ungapped) and the
// pass that turns a column of raw scores into bit scores and E-values, rescaled per hit row by the pair's own ungapped lambda
// (ks_scores_stats_device and its three wrappers).
//
//   composition  k_ac_wave, a wave per sequence: the offsets are checked before anything is read through them, the length is
//                written, a short sequence is counted on the spot into the wave's 28 LDS counters (ds_add_u32), a longer one is
//                listed for k_ac_group — once as a whole (one workgroup, four private LDS histograms, plain stores), or beyond
//                AC_GROUP_MAX residues once per chunk of that many (the workgroups add to the sequence's 28 zeroed counters:
//                integer atomics, any order gives the same counts).  k_ac_totals sums the columns in u64.
//   histogram    k_as_hist, a wave per hit row over a fixed grid: the 2 x 20 standard-class counts through LDS, the 400 products —
//                the pairs come sorted by power smax - s, seven consecutive ones to a lane, pre-summed per power in registers —
//                added into the wave's u64 bins (ds_add_u64), the three integer tests of a regular row from wave sums, the d + 1
//                coefficients as f64 into the slice's scratch.
//   root         k_as_root, a lane per hit row: the coefficients of 64 rows transposed into LDS (conflict-free: lane j reads
//                word k * 64 + j) where d + 1 <= AS_LDS_COEF, else read where they lie; ~55 Horner evaluations, no contraction.
//                The rows run in slices of AS_SLICE_WORDS / (d + 1) so that the coefficient scratch stays at 32 MiB.
//   emit         k_as_emit, a lane per hit row: the CSR is checked before a score is read through it; per entry the bit score
//                and the E-value, per row their best.
// One host wait.  Everything a kernel indexes with is checked on the device first; a refused row is named by its first offender.
#include "ks_rkit.h"

#include <cmath>

#define AC_THREADS 256
#define AC_A RK_A
#define AC_WAVE_MAX 1024u    // the longest sequence a wave counts (ks_debug_rcomp_limits)
#define AC_GROUP_MAX 65536u  // the longest sequence one workgroup counts; the chunk of a split one
#define AC_GROUP_GRID 2048
#define AC_TOTALS_GRID 512
#define AC_WHOLE 0xffffffffu // a listed sequence that one workgroup takes whole
enum : u32 { AC_BAD_OFFS = 0, AC_BAD_LONG = 1, AC_N_BAD = 2 };

#define AS_STD 20            // the standard classes
#define AS_BINS 256          // powers smax - s of an int8 matrix
#define AS_LDS_COEF 64       // d + 1 up to which k_as_root stages the coefficients (64 rows x 64 x 8 B = 32 KiB)
#define AS_SLICE_WORDS (1u << 22)
#define AS_HIST_GRID 4096   // workgroups of k_as_hist (4 waves each, striding over the rows)
enum : u32 { AS_BAD_CSR = 0, AS_BAD_ID = 1, AS_BAD_LONG = 2, AS_N_BAD = 3, AS_FALLBACK = 3 };

// the classes of ACDEFGHIKLMNPQRSTVWY
static const u8 as_std_host[AS_STD] = {0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18, 19, 21, 22, 24};
__constant__ u8 as_std[AS_STD] = {0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18, 19, 21, 22, 24};

// ---------------------------------------------------------------------------------------------
// residue composition
// ---------------------------------------------------------------------------------------------
struct ac_args {
    const u8 *res;
    const u64 *offs;
    u32 n_seqs;
    u64 n_res;
    u32 *counts, *length;
    u32 *list, list_cap; // (sequence, chunk | AC_WHOLE) for k_ac_group
    unsigned long long *bad;
};

// mode: 0 by length, 1 every sequence by a wave, 2 every sequence whole by a workgroup, 3 every sequence in chunks
__global__ __launch_bounds__(AC_THREADS) void k_ac_wave(ac_args A, int mode) {
    __shared__ u32 s_h[AC_THREADS / 64][32];
    const u32 lane = threadIdx.x & 63, w = ks_readfirst(threadIdx.x >> 6);
    const u64 s64 = (u64)blockIdx.x * (AC_THREADS / 64) + w;
    const u32 s = (u32)s64;
    if (lane < 32) s_h[w][lane] = 0;
    u64 b = 0, len = 0;
    bool mine = false;
    if (s64 < A.n_seqs) {
        b = rk_readfirst64(A.offs[s]);
        const u64 e = rk_readfirst64(A.offs[s64 + 1]);
        if (b > e || e > A.n_res) {
            if (lane == 0) { ks_first_bad(A.bad, AC_BAD_OFFS, s); A.length[s] = 0; }
        } else if (e - b > 0xffffffffULL) {
            if (lane == 0) { ks_first_bad(A.bad, AC_BAD_LONG, s); A.length[s] = 0; }
        } else { // [b, e) lies inside the batch: all anybody reads of this sequence
            len = e - b;
            mine = mode == 1 || (mode == 0 && len <= AC_WAVE_MAX);
            if (lane == 0) {
                A.length[s] = (u32)len;
                if (!mine) {
                    if (mode == 2 || (mode == 0 && len <= AC_GROUP_MAX)) ks_seg_list_push(A.list, A.list_cap, s, AC_WHOLE);
                    else for (u64 c = 0; c * AC_GROUP_MAX < len; c++) ks_seg_list_push(A.list, A.list_cap, s, (u32)c);
                }
            }
        }
    }
    __syncthreads();
    if (mine)
        for (u64 i = lane; i < len; i += 64) atomicAdd(&s_h[w][rk_class(A.res[b + i])], 1u);
    __syncthreads();
    if (mine && lane < AC_A) A.counts[s64 * AC_A + lane] = s_h[w][lane];
}

__global__ __launch_bounds__(AC_THREADS) void k_ac_group(ac_args A) {
    __shared__ u32 s_h[AC_THREADS / 64][32];
    const u32 t = threadIdx.x, w = t >> 6;
    for (ks_seg_walk seg = ks_seg_list_by_wg(A.list, A.list_cap); seg.next();) {
        const u32 s = seg.b, c = seg.len;
        if (s >= A.n_seqs) continue; // (the list holds nothing else; uniform, as every `continue` here)
        const u64 b = rk_readfirst64(A.offs[s]), e = rk_readfirst64(A.offs[(u64)s + 1]);
        if (b > e || e > A.n_res) continue;
        u64 lo = b, hi = e;
        if (c != AC_WHOLE) {
            lo = b + (u64)c * AC_GROUP_MAX;
            if (lo >= e) continue;
            hi = e - lo > AC_GROUP_MAX ? lo + AC_GROUP_MAX : e;
        }
        __syncthreads(); // (the previous item's readers)
        if (t < (AC_THREADS / 64) * 32) s_h[t >> 5][t & 31] = 0;
        __syncthreads();
        for (u64 i = lo + t; i < hi; i += AC_THREADS) atomicAdd(&s_h[w][rk_class(A.res[i])], 1u);
        __syncthreads();
        if (t < AC_A) {
            u32 v = 0;
            for (u32 k = 0; k < AC_THREADS / 64; k++) v += s_h[k][t];
            if (c == AC_WHOLE) A.counts[(u64)s * AC_A + t] = v;
            else if (v) atomicAdd(&A.counts[(u64)s * AC_A + t], v);
        }
    }
}

// thread t < 252 = 9 x 28 adds class t % 28 of the sequences t / 28, + 9, ...: a workgroup reads consecutive words
__global__ __launch_bounds__(AC_THREADS) void k_ac_totals(const u32 *counts, u32 n_seqs, unsigned long long *totals) {
    __shared__ unsigned long long s_t[AC_A];
    const u32 t = threadIdx.x;
    constexpr u32 G = AC_THREADS / AC_A;
    if (t < AC_A) s_t[t] = 0;
    __syncthreads();
    if (t < G * AC_A) {
        const u32 c = t % AC_A;
        u64 acc = 0;
        for (u64 s = (u64)blockIdx.x * G + t / AC_A; s < n_seqs; s += (u64)gridDim.x * G) acc += counts[s * AC_A + c];
        if (acc) atomicAdd(&s_t[c], (unsigned long long)acc);
    }
    __syncthreads();
    if (t < AC_A && s_t[t]) atomicAdd(&totals[t], s_t[t]);
}

int ks_residue_composition_impl(ks_ctx *ctx, const ks_res_batch &B, ks_rcomp *C) {
    const u64 ns = B.n_seqs;
    C->n_seqs = B.n_seqs; C->n_res = B.n_res;
    memset(C->h_totals, 0, sizeof C->h_totals);
    KS_TRY(ks_alloc(ctx, &C->d_counts, (size_t)ns * AC_A));
    KS_TRY(ks_alloc(ctx, &C->d_totals, (size_t)AC_A));
    KS_TRY(ks_alloc(ctx, &C->d_length, (size_t)ns));
    KS_HIP(ctx, hipMemsetAsync(C->d_totals, 0, AC_A * sizeof(u64), ctx->stream));
    if (ns == 0) return ks_stream_wait(ctx);
    const u64 cap = ns + B.n_res / AC_GROUP_MAX + 1; // a listed sequence of len residues owns at most 1 + len / AC_GROUP_MAX items
    if (cap > 0x7fffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "residue composition: a batch of %llu sequences and %llu residues", (unsigned long long)ns, (unsigned long long)B.n_res);
    KS_HIP(ctx, hipMemsetAsync(C->d_counts, 0, (size_t)ns * AC_A * sizeof(u32), ctx->stream)); // (the split path adds to them)

    bool chunks;
    int mode = ks_seg_path_knob(ctx, KS_DBG_COMP_PATH, &chunks);
    if (chunks) mode = 3;
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u32 *list = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RCOMP, AC_N_BAD, 0));
    KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)cap, &list));
    const ac_args A = {B.res, B.offs, B.n_seqs, B.n_res, C->d_counts, C->d_length, list, (u32)cap, ctl.words()};
    KS_LAUNCH(ctx, "rcomp_wave", k_ac_wave, (u32)((ns + AC_THREADS / 64 - 1) / (AC_THREADS / 64)), AC_THREADS, A, mode);
    if (mode != 1) KS_LAUNCH(ctx, "rcomp_group", k_ac_group, AC_GROUP_GRID, AC_THREADS, A);
    constexpr u32 G = AC_THREADS / AC_A;
    const u64 tg = (ns + G - 1) / G;
    KS_LAUNCH(ctx, "rcomp_totals", k_ac_totals, (u32)(tg < AC_TOTALS_GRID ? tg : AC_TOTALS_GRID), AC_THREADS, (const u32 *)C->d_counts, B.n_seqs,
              (unsigned long long *)C->d_totals);
    const ks_fetch_seg f = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (ctl.bad(AC_BAD_OFFS))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "residue composition: the offsets of sequence %llu descend or pass the batch's %llu residues",
                       (unsigned long long)ctl[AC_BAD_OFFS], (unsigned long long)B.n_res);
    if (ctl.bad(AC_BAD_LONG))
        return ks_fail(ctx, KS_ERR_CAPACITY, "residue composition: sequence %llu has 2^32 residues or more", (unsigned long long)ctl[AC_BAD_LONG]);
    return ks_copy_d2h(ctx, C->h_totals, C->d_totals, sizeof C->h_totals);
}

extern "C" int ks_residue_composition_device(ks_ctx *ctx, const uint8_t *d_res, const uint64_t *d_offs, uint32_t n_seqs, uint64_t n_res,
                                             ks_rcomp **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!out || !d_offs || (!d_res && n_res)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_rcomp> C(ctx, out, ks_rcomp_free);
    KS_TRY(ks_residue_composition_impl(ctx, ks_res_batch{d_res, d_offs, n_seqs, n_res}, C));
    return C.commit();
    });
}
extern "C" uint32_t ks_rcomp_n_seqs(const ks_rcomp *c) { return c ? c->n_seqs : 0; }
extern "C" uint64_t ks_rcomp_n_residues(const ks_rcomp *c) { return c ? c->n_res : 0; }
extern "C" const uint32_t *ks_rcomp_device_counts(const ks_rcomp *c) { return c ? c->d_counts : nullptr; }
extern "C" const uint64_t *ks_rcomp_device_totals(const ks_rcomp *c) { return c ? c->d_totals : nullptr; }
extern "C" const uint32_t *ks_rcomp_device_length(const ks_rcomp *c) { return c ? c->d_length : nullptr; }
extern "C" int ks_rcomp_copy_to_host(ks_ctx *ctx, const ks_rcomp *c, uint32_t *counts, uint64_t *totals, uint32_t *length) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, counts, totals, length); });
}
extern "C" void ks_rcomp_free(ks_rcomp *c) { ks_obj_free(c); }
extern "C" void ks_debug_rcomp_limits(uint32_t *wave_max, uint32_t *group_max) {
    if (wave_max) *wave_max = AC_WAVE_MAX;
    if (group_max) *group_max = AC_GROUP_MAX;
}

// ---------------------------------------------------------------------------------------------
// ungapped Karlin-Altschul parameters (host)
// ---------------------------------------------------------------------------------------------
static thread_local const char *as_karlin_err = "";
static int as_karlin_fail(const char *why) { as_karlin_err = why; return KS_ERR_INVALID_ARG; }
extern "C" const char *ks_karlin_last_error(void) { return as_karlin_err; }

// the 20 standard weights of w, renormalised
static bool as_std_freq(const double *w, double *f) {
    double sum = 0.0;
    for (int i = 0; i < AS_STD; i++) {
        const double v = w[as_std_host[i]];
        if (!(v >= 0.0) || !std::isfinite(v)) return false;
        f[i] = v; sum += v;
    }
    for (int i = 0; i < AC_A; i++)
        if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return false;
    if (!(sum > 0.0)) return false;
    for (int i = 0; i < AS_STD; i++) f[i] /= sum;
    return true;
}
static int as_m(const int8_t *M, int i, int j) { return M ? (int)M[i * AC_A + j] : (i == j ? 1 : -1); }

static int as_karlin(const int8_t *M, const double *freq_q, const double *freq_t, double *o_lambda, double *o_K, double *o_H) {
    if (!freq_q || !freq_t) return as_karlin_fail("NULL argument");
    double fq[AS_STD], ft[AS_STD];
    if (!as_std_freq(freq_q, fq) || !as_std_freq(freq_t, ft))
        return as_karlin_fail("the weights must be finite and not negative, with a positive one on a standard class");
    double P[256];
    for (double &p : P) p = 0.0;
    for (int i = 0; i < AS_STD; i++)
        for (int j = 0; j < AS_STD; j++) P[as_m(M, as_std_host[i], as_std_host[j]) + 128] += fq[i] * ft[j];
    int lo = 0, hi = 0;
    bool any = false;
    double mean = 0.0;
    for (int s = -128; s <= 127; s++) {
        if (!(P[s + 128] > 0.0)) continue;
        if (!any) lo = s;
        hi = s; any = true;
        mean += s * P[s + 128];
    }
    if (!any || hi <= 0) return as_karlin_fail("no positive score has positive probability");
    if (!(mean < 0.0)) return as_karlin_fail("the expected score is not negative");
    // lambda: phi(l) = sum P(s) e^(l s) - 1 is 0 at 0, negative up to the root, positive beyond it
    auto phi = [&](double l) { double v = 0.0; for (int s = lo; s <= hi; s++) v += P[s + 128] * std::exp(l * s); return v - 1.0; };
    double up = 0.5;
    while (!(phi(up) > 0.0)) up *= 2.0; // (P(hi) e^(up hi) alone passes 1 long before anything overflows)
    double a = 0.0, b = up;
    for (int step = 0; step < 200; step++) {
        const double mid = 0.5 * (a + b);
        if (mid == a || mid == b) break;
        if (phi(mid) > 0.0) b = mid; else a = mid;
    }
    double lambda = b;
    for (int it = 0; it < 2; it++) { // two Newton steps on the bracketed root
        double v = -1.0, dv = 0.0;
        for (int s = lo; s <= hi; s++) { const double t = P[s + 128] * std::exp(lambda * s); v += t; dv += s * t; }
        const double nl = lambda - v / dv;
        if (nl > a && nl <= up && std::isfinite(nl)) lambda = nl;
    }
    double hs = 0.0; // sum s P(s) e^(lambda s)
    for (int s = lo; s <= hi; s++) hs += s * P[s + 128] * std::exp(lambda * s);
    const double H = lambda * hs;
    if (o_lambda) *o_lambda = lambda;
    if (o_H) *o_H = H;
    if (!o_K) return KS_OK;
    int delta = 0;
    for (int s = lo; s <= hi; s++) {
        if (!(P[s + 128] > 0.0)) continue;
        int x = s < 0 ? -s : s, y = delta;
        while (y) { const int r = x % y; x = y; y = r; }
        delta = x;
    }
    const int l1 = lo / delta, h1 = hi / delta, width = h1 - l1 + 1;
    const double lp = lambda * delta;
    std::vector<double> Q((size_t)width), Pk, next;
    for (int j = l1; j <= h1; j++) Q[(size_t)(j - l1)] = P[j * delta + 128];
    Pk = Q;
    double sigma = 0.0;
    bool done = false;
    for (int k = 1; k <= 400 && !done; k++) {
        if (k > 1) { // P_k = P_(k-1) * Q over [k l1, k h1]
            next.assign((size_t)(k * (h1 - l1) + 1), 0.0);
            for (size_t i = 0; i < Pk.size(); i++) {
                const double p = Pk[i];
                if (p == 0.0) continue;
                for (int j = 0; j < width; j++) next[i + (size_t)j] += p * Q[(size_t)j];
            }
            Pk.swap(next);
        }
        double neg = 0.0, pos = 0.0;
        for (size_t i = 0; i < Pk.size(); i++) {
            const long j = (long)k * l1 + (long)i;
            if (j < 0) neg += Pk[i] * std::exp(lp * (double)j); else pos += Pk[i];
        }
        const double term = (neg + pos) / (double)k;
        sigma += term;
        done = term < 0x1p-60;
    }
    if (!done) return as_karlin_fail("expected score too close to zero");
    *o_K = -std::exp(-2.0 * sigma) / ((H / lp) * std::expm1(-lp));
    return KS_OK;
}
extern "C" int ks_karlin_ungapped(const int8_t *matrix, const double *freq_q, const double *freq_t, double *lambda, double *K, double *H) {
    return ks_guard(nullptr, [&]() -> int {
    as_karlin_err = "";
    return as_karlin(matrix, freq_q, freq_t, lambda, K, H);
    });
}

// ---------------------------------------------------------------------------------------------
// the statistics pass
// ---------------------------------------------------------------------------------------------
struct as_args {
    const u64 *row_offs; // n_rows + 1, or NULL: one entry per row
    const i64 *score;
    const u32 *qid, *tid;
    const u32 *q_counts, *t_counts, *q_len, *t_len; // t_*: NULL without a target composition
    const u16 *tab_pair;                            // device: the 400 standard pairs (i << 8 | j) by ascending power ...
    const u8 *tab_pw;                               // ... and their powers smax - M[i][j]
    u32 n_rows, n, n_q, n_t;
    int smin, smax;
    u32 row0, n_slice;   // the rows of this launch of k_as_hist / k_as_root
    double *coef;        // n_slice x (d + 1)
    u32 composition, pairwise, length_adjust;
    u64 n_eff;
    double lambda_std, ratio_min, ratio_max, lambda_c, K_c, ln_K, ln_2;
    u8 *status;
    double *x, *ratio, *bit, *evalue, *row_bit, *row_evalue;
    unsigned long long *ctl; // AS_BAD_*, then the fallback rows
};


// The pairs (i, j) of the standard block ordered by power smax - M[i][j] (the host sorts them once per call): lane l takes the
// AS_RUN consecutive pairs from l * AS_RUN, sums those of one power in registers and sends one atomic per power it meets, so a
// matrix of few scores (+1 / -1: two powers) costs the wave two colliding LDS atomics, not seven.
#define AS_RUN 7 // 64 * 7 >= 400
static_assert(64 * AS_RUN >= AS_STD * AS_STD, "a wave covers the standard block");
__global__ __launch_bounds__(AC_THREADS) void k_as_hist(as_args A) {
    __shared__ u16 s_pair[AS_STD * AS_STD]; // i << 8 | j, positions in the standard order
    __shared__ u8 s_pw[AS_STD * AS_STD];    // the pair's power, ascending
    __shared__ unsigned long long s_h[AC_THREADS / 64][AS_BINS];
    __shared__ u32 s_cq[AC_THREADS / 64][AS_STD], s_ct[AC_THREADS / 64][AS_STD];
    for (u32 i = threadIdx.x; i < AS_STD * AS_STD; i += AC_THREADS) { s_pair[i] = A.tab_pair[i]; s_pw[i] = A.tab_pw[i]; }
    __syncthreads();
    const u32 lane = threadIdx.x & 63, w = ks_readfirst(threadIdx.x >> 6);
    const u32 d = (u32)(A.smax - A.smin);
    // a wave per row, striding; from here on a wave only meets itself: its LDS operations execute in order
    for (u32 rl = blockIdx.x * (AC_THREADS / 64) + w; rl < A.n_slice; rl += gridDim.x * (AC_THREADS / 64)) {
        const u32 row = A.row0 + rl;
        const u32 q = ks_readfirst(A.qid[row]), t = ks_readfirst(A.tid[row]);
        if (q >= A.n_q || t >= A.n_t || A.q_len[q] > KS_ASTATS_MAX_SEQ_LEN || A.t_len[t] > KS_ASTATS_MAX_SEQ_LEN) { // (the call fails: nobody reads the row)
            if (lane == 0) { ks_first_bad(A.ctl, (q >= A.n_q || t >= A.n_t) ? AS_BAD_ID : AS_BAD_LONG, row); A.status[row] = KS_ASTATS_ROW_FALLBACK; }
            continue;
        }
        for (u32 k = lane; k <= d; k += 64) s_h[w][k] = 0;
        if (lane < AS_STD) { s_cq[w][lane] = A.q_counts[(u64)q * RK_A + as_std[lane]]; s_ct[w][lane] = A.t_counts[(u64)t * RK_A + as_std[lane]]; }
        __builtin_amdgcn_wave_barrier();
        i64 es = 0;
        bool pos = false;
        u64 acc = 0;
        u32 cur = 0;
        for (u32 k = 0; k < AS_RUN; k++) {
            const u32 p = lane * AS_RUN + k;
            if (p >= AS_STD * AS_STD) break;
            const u32 pr = s_pair[p], pw = s_pw[p];
            const u64 v = (u64)s_cq[w][pr >> 8] * s_ct[w][pr & 255u]; // (each count <= 2^20)
            if (pw != cur) {
                if (acc) atomicAdd(&s_h[w][cur], (unsigned long long)acc);
                acc = 0; cur = pw;
            }
            const int sc = A.smax - (int)pw;
            acc += v; es += (i64)sc * (i64)v; pos |= sc > 0 && v != 0;
        }
        if (acc) atomicAdd(&s_h[w][cur], (unsigned long long)acc);
        __builtin_amdgcn_wave_barrier();
        const i64 ES = (i64)ks_wave_sum64((u64)es); // |ES| <= 128 * 2^40
        const u64 nq = ks_wave_sum64(lane < AS_STD ? s_cq[w][lane] : 0u), nt = ks_wave_sum64(lane < AS_STD ? s_ct[w][lane] : 0u);
        const u64 N = nq * nt;
        const bool regular = N > 0 && ES < 0 && __ballot(pos) != 0;
        if (lane == 0) {
            A.status[row] = regular ? KS_ASTATS_ROW_REGULAR : KS_ASTATS_ROW_FALLBACK;
            if (!regular) atomicAdd(&A.ctl[AS_FALLBACK], 1ULL);
        }
        for (u32 k = lane; k <= d; k += 64) {
            i64 c = (i64)s_h[w][k];
            if (k == (u32)A.smax) c -= (i64)N; // (0 < smax < d: the power of s = 0)
            A.coef[(u64)rl * (d + 1) + k] = (double)c; // |c| <= 2^40: exact
        }
        __builtin_amdgcn_wave_barrier(); // (the next row zeroes the bins and replaces the counts)
    }
}

// f at x by Horner from power d down; c[k * stride]: the coefficient of power k
KS_DEV double as_horner(const double *c, u32 stride, u32 d, double x) {
#pragma clang fp contract(off)
    double v = c[(size_t)d * stride];
    for (u32 k = d; k-- > 0;) v = v * x + c[(size_t)k * stride];
    return v;
}

__global__ __launch_bounds__(64) void k_as_root(as_args A, u32 staged) {
#pragma clang fp contract(off)
    extern __shared__ double s_c[]; // staged: (d + 1) x 64, power-major
    const u32 lane = threadIdx.x, d = (u32)(A.smax - A.smin), D1 = d + 1;
    const u32 base = blockIdx.x * 64u;
    const u32 nb = A.n_slice - base < 64u ? A.n_slice - base : 64u;
    if (staged) {
        for (u32 f = lane; f < nb * D1; f += 64) s_c[(f % D1) * 64 + f / D1] = A.coef[(u64)base * D1 + f];
        __syncthreads();
    }
    if (lane >= nb) return;
    const u32 row = A.row0 + base + lane;
    double x = 0.0, rho = 1.0;
    if (A.status[row] == KS_ASTATS_ROW_REGULAR) {
        const double *c = staged ? s_c + lane : A.coef + (u64)(base + lane) * D1;
        const u32 stride = staged ? 64u : 1u;
        double lo = 0.0, hi = 1.0;
        for (int step = 0; step < 128; step++) {
            const double mid = 0.5 * (lo + hi);
            if (mid == lo || mid == hi) break;
            if (as_horner(c, stride, d, mid) > 0.0) lo = mid; else hi = mid;
        }
        x = lo;
        rho = -log(x) / A.lambda_std;
        rho = rho < A.ratio_min ? A.ratio_min : rho;
        rho = rho > A.ratio_max ? A.ratio_max : rho;
    }
    A.x[row] = x; A.ratio[row] = rho;
}

__global__ __launch_bounds__(AC_THREADS) void k_as_emit(as_args A) {
#pragma clang fp contract(off)
    const u64 r64 = (u64)blockIdx.x * AC_THREADS + threadIdx.x;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    u64 b = r, e = r64 + 1;
    if (A.row_offs) {
        b = A.row_offs[r]; e = A.row_offs[r64 + 1];
        if ((r == 0 && b != 0) || b > e || e > A.n || (r == A.n_rows - 1 && e != A.n)) { ks_first_bad(A.ctl, AS_BAD_CSR, r); return; }
    }
    const u32 q = A.qid[r], t = A.tid[r];
    if (q >= A.n_q || (A.t_len && t >= A.n_t)) { ks_first_bad(A.ctl, AS_BAD_ID, r); return; }
    double rho = 1.0;
    if (A.composition) rho = A.ratio[r];
    else { A.status[r] = KS_ASTATS_ROW_SKIPPED; A.x[r] = 0.0; A.ratio[r] = 1.0; }
    const u32 Lq = A.q_len[q], adj = A.length_adjust;
    const u32 m_eff = Lq > adj && Lq - adj > 1u ? Lq - adj : 1u;
    u64 n_eff = A.n_eff;
    if (A.pairwise) { const u32 Lt = A.t_len[t]; n_eff = Lt > adj && Lt - adj > 1u ? Lt - adj : 1u; }
    const double km = (A.K_c * (double)n_eff) * (double)m_eff;
    double best_bit = ks_nan(), best_e = ks_nan();
    for (u64 i = b; i < e; i++) { // [b, e) lies inside [0, n)
        const double Sp = rho * (double)A.score[i];
        const double bit = (A.lambda_c * Sp - A.ln_K) / A.ln_2;
        const double ev = km * exp(-(A.lambda_c * Sp));
        A.bit[i] = bit; A.evalue[i] = ev;
        if (i == b || bit > best_bit) best_bit = bit;
        if (i == b || ev < best_e) best_e = ev;
    }
    A.row_bit[r] = best_bit; A.row_evalue[r] = best_e;
}

int ks_scores_stats_impl(ks_ctx *ctx, const u64 *d_row_offs, const i64 *d_score, u64 n_rows, u64 n, const ks_hits *H, const ks_rcomp *Q,
                         const ks_rcomp *T, const ks_astats_opts &o, ks_astats *S) {
    S->n_rows = n_rows; S->n = n; S->n_fallback = 0;
    KS_TRY(rk_counts_check(ctx, "alignment statistics", n_rows, n));
    const bool composition = !(o.flags & KS_ASTATS_NO_COMPOSITION), own = o.lambda == 0.0;
    // the host's share: the extremes of the standard block, the standard lambda (and K), the search space
    int smin = 127, smax = -128;
    for (int i = 0; i < AS_STD; i++)
        for (int j = 0; j < AS_STD; j++) {
            const int m = as_m(o.matrix, as_std_host[i], as_std_host[j]);
            smin = m < smin ? m : smin; smax = m > smax ? m : smax;
        }
    if (smax <= 0 || smin >= 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: the standard 20 x 20 block of the matrix spans %d .. %d: it needs a negative and a positive score", smin, smax);
    double bg[AC_A], lambda_std = 0.0, K_std = 0.0;
    for (int i = 0; i < AC_A; i++) bg[i] = o.background ? o.background[i] : (double)T->h_totals[i];
    if (composition || own) {
        if (ks_karlin_ungapped(o.matrix, bg, bg, &lambda_std, own ? &K_std : nullptr, nullptr) != KS_OK)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: the matrix under the background composition: %s", ks_karlin_last_error());
    }
    S->lambda_std = lambda_std;
    S->lambda_used = own ? lambda_std : o.lambda; S->K_used = own ? K_std : o.K; S->params_source = own ? 0u : 1u;
    const u64 db_res = o.db_residues ? o.db_residues : T->n_res, db_seqs = o.db_seqs ? o.db_seqs : T->n_seqs;
    u64 off = 0;
    if (__builtin_mul_overflow(db_seqs, (u64)o.length_adjust, &off)) off = ~0ULL;
    const u64 n_eff = db_res > off && db_res - off > 1 ? db_res - off : 1;

    KS_TRY(ks_alloc(ctx, &S->d_status, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &S->d_x, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &S->d_ratio, (size_t)n_rows));
    KS_TRY(ks_alloc(ctx, &S->d_row_bit, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &S->d_row_evalue, (size_t)n_rows));
    KS_TRY(ks_alloc(ctx, &S->d_bit, (size_t)n)); KS_TRY(ks_alloc(ctx, &S->d_evalue, (size_t)n));
    if (n_rows == 0) return ks_stream_wait(ctx);

    ks_scratch sc(ctx);
    ks_ctl ctl;
    u8 *d_tab = nullptr;
    double *coef = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_ASTATS, AS_N_BAD, 1));
    as_args A;
    A.row_offs = d_row_offs; A.score = d_score; A.qid = H->d_qid; A.tid = H->d_tid;
    A.q_counts = Q->d_counts; A.q_len = Q->d_length; A.t_counts = T ? T->d_counts : nullptr; A.t_len = T ? T->d_length : nullptr;
    A.tab_pair = nullptr; A.tab_pw = nullptr; A.n_rows = (u32)n_rows; A.n = (u32)n; A.n_q = Q->n_seqs; A.n_t = T ? T->n_seqs : 0u;
    A.smin = smin; A.smax = smax; A.row0 = 0; A.n_slice = 0; A.coef = nullptr;
    A.composition = composition ? 1u : 0u; A.pairwise = (o.flags & KS_ASTATS_PAIRWISE) ? 1u : 0u; A.length_adjust = o.length_adjust;
    A.n_eff = n_eff; A.lambda_std = lambda_std; A.ratio_min = o.ratio_min; A.ratio_max = o.ratio_max;
    A.lambda_c = S->lambda_used; A.K_c = S->K_used; A.ln_K = std::log(S->K_used); A.ln_2 = std::log(2.0);
    A.status = S->d_status; A.x = S->d_x; A.ratio = S->d_ratio; A.bit = S->d_bit; A.evalue = S->d_evalue;
    A.row_bit = S->d_row_bit; A.row_evalue = S->d_row_evalue; A.ctl = ctl.words();
    if (composition) {
        const u32 D1 = (u32)(smax - smin) + 1u;
        u64 per = AS_SLICE_WORDS / D1;
        per = per > n_rows ? n_rows : per;
        per = (per + 63) / 64 * 64;
        // the standard pairs by ascending power (a counting sort: stable, so equal powers keep the order of the block)
        constexpr u32 NP = AS_STD * AS_STD;
        struct { u16 pair[NP]; u8 pw[NP]; } tab;
        u32 at[AS_BINS + 1] = {0};
        for (u32 p = 0; p < NP; p++) at[(u32)(smax - as_m(o.matrix, as_std_host[p / AS_STD], as_std_host[p % AS_STD])) + 1]++;
        for (u32 k = 0; k < AS_BINS; k++) at[k + 1] += at[k];
        for (u32 p = 0; p < NP; p++) {
            const u32 pw = (u32)(smax - as_m(o.matrix, as_std_host[p / AS_STD], as_std_host[p % AS_STD])), i = at[pw]++;
            tab.pair[i] = (u16)((p / AS_STD) << 8 | (p % AS_STD)); tab.pw[i] = (u8)pw;
        }
        KS_TRY(sc.alloc(&d_tab, sizeof tab));
        KS_TRY(ks_copy_h2d(ctx, d_tab, &tab, sizeof tab)); // (a pageable source: consumed on return)
        KS_TRY(sc.alloc(&coef, (size_t)(per * D1)));
        A.tab_pair = (const u16 *)d_tab; A.tab_pw = d_tab + sizeof tab.pair; A.coef = coef;
        const u32 staged = D1 <= AS_LDS_COEF ? 1u : 0u;
        for (u64 r0 = 0; r0 < n_rows; r0 += per) {
            A.row0 = (u32)r0; A.n_slice = (u32)(n_rows - r0 < per ? n_rows - r0 : per);
            const u32 hg = (A.n_slice + AC_THREADS / 64 - 1) / (AC_THREADS / 64);
            KS_LAUNCH(ctx, "astats_hist", k_as_hist, hg < AS_HIST_GRID ? hg : AS_HIST_GRID, AC_THREADS, A);
            ks_timer_begin(ctx, "astats_root");
            hipLaunchKernelGGL(k_as_root, dim3((A.n_slice + 63) / 64), dim3(64), staged ? (size_t)D1 * 64 * sizeof(double) : 0, ctx->stream, A, staged);
            ks_timer_end(ctx);
            KS_HIP(ctx, hipGetLastError());
        }
    }
    KS_LAUNCH(ctx, "astats_emit", k_as_emit, (u32)((n_rows + AC_THREADS - 1) / AC_THREADS), AC_THREADS, A);
    const ks_fetch_seg f = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (ctl.bad(AS_BAD_CSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: row_offsets is not a CSR from 0 to %llu scores that never descends: hit row %llu breaks it",
                       (unsigned long long)n, (unsigned long long)ctl[AS_BAD_CSR]);
    if (ctl.bad(AS_BAD_ID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: hit row %llu names a query or target beyond its composition (%u queries, %u targets)",
                       (unsigned long long)ctl[AS_BAD_ID], Q->n_seqs, T ? T->n_seqs : 0u);
    if (ctl.bad(AS_BAD_LONG))
        return ks_fail(ctx, KS_ERR_CAPACITY, "alignment statistics: hit row %llu has a sequence of more than 2^20 residues", (unsigned long long)ctl[AS_BAD_LONG]);
    S->n_fallback = ctl[AS_FALLBACK];
    return KS_OK;
}

// the options, defaults filled in; refused before any device work, also with ctx == NULL.  recorded: the matrix of the
// alignments the scores came from (NULL: none); gapped: the scores are gapped ones
static int as_refuse(ks_ctx *ctx, const char *why) { return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics options: %s", why) : KS_ERR_INVALID_ARG; }
static int as_opts_check(ks_ctx *ctx, const ks_astats_opts *opts, const int8_t *recorded, bool gapped, ks_astats_opts *o) {
    if (opts) *o = *opts; else memset(o, 0, sizeof *o);
    KS_TRY(ks_opts_words_check(ctx, "alignment statistics", o->flags, KS_ASTATS_NO_COMPOSITION | KS_ASTATS_PAIRWISE | KS_ASTATS_ALLOW_UNGAPPED,
                               o->reserved ? 1u : 0u));
    if (!(o->lambda >= 0.0) || !(o->K >= 0.0) || !std::isfinite(o->lambda) || !std::isfinite(o->K)) return as_refuse(ctx, "lambda and K must be finite and not negative");
    if ((o->lambda == 0.0) != (o->K == 0.0)) return as_refuse(ctx, "lambda and K come together: both 0 or both positive");
    if (!(o->ratio_min >= 0.0) || !(o->ratio_max >= 0.0) || !std::isfinite(o->ratio_min) || !std::isfinite(o->ratio_max))
        return as_refuse(ctx, "ratio_min and ratio_max must be finite and not negative");
    if (o->ratio_min == 0.0 && o->ratio_max == 0.0) { o->ratio_min = 0.5; o->ratio_max = 1.0; }
    if (o->ratio_min > o->ratio_max) return as_refuse(ctx, "ratio_min is larger than ratio_max");
    if (recorded) {
        if (o->matrix && memcmp(o->matrix, recorded, (size_t)AC_A * AC_A) != 0)
            return as_refuse(ctx, "the matrix differs from the one the alignments were made with");
        o->matrix = recorded;
    }
    if (gapped && o->lambda == 0.0 && !(o->flags & KS_ASTATS_ALLOW_UNGAPPED))
        return as_refuse(ctx, "gapped scores need the caller's gapped lambda and K (KS_ASTATS_ALLOW_UNGAPPED: the ungapped ones, which understate E-values)");
    return KS_OK;
}
static int as_run(ks_ctx *ctx, const u64 *d_row_offs, const i64 *d_score, u64 n_rows, u64 n, const ks_hits *H, const ks_rcomp *Q, const ks_rcomp *T,
                  const ks_astats_opts &o, ks_astats **out) {
    const bool t_free = (o.flags & KS_ASTATS_NO_COMPOSITION) && !(o.flags & KS_ASTATS_PAIRWISE) && o.db_residues && o.db_seqs && o.background;
    if (!out || !H || !Q || (!T && !t_free) || (n && !d_score)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "alignment statistics", H, Q, T));
    if (n_rows != H->n_hits)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: the scores lie in %llu hit rows, the hit list has %llu: scores of another search",
                       (unsigned long long)n_rows, (unsigned long long)H->n_hits);
    if (n_rows == 0 && n != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: %llu scores in no hit row: row_offsets is not a CSR from 0 to n", (unsigned long long)n);
    if (!d_row_offs && n != n_rows)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "alignment statistics: %llu scores for %llu hit rows without row_offsets", (unsigned long long)n, (unsigned long long)n_rows);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_astats> S(ctx, out, ks_astats_free);
    KS_TRY(ks_scores_stats_impl(ctx, d_row_offs, d_score, n_rows, n, H, Q, T, o, S));
    return S.commit();
}

// What the four entries do alike, in their order: the options (also without a context), the context, *out, the objects the scores
// come from (`in`: not NULL, of ctx), then `run`, which reads them.  recorded: the gapped alignments behind the scores, or NULL
template <typename Run, typename... In>
static int as_entry(ks_ctx *ctx, const ks_astats_opts *opts, const ks_raligns *recorded, bool gapped, ks_astats **out, Run &&run, const In *...in) {
    return ks_guard(ctx, [&]() -> int {
    ks_astats_opts o;
    KS_TRY(as_opts_check(ctx, opts, recorded ? recorded->matrix : nullptr, gapped, &o));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if ((!in || ...)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if constexpr (sizeof...(In) != 0) KS_TRY(ks_inputs_check_ctx(ctx, "alignment statistics", in...));
    return run(o);
    });
}
extern "C" int ks_scores_stats_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const int64_t *d_score, uint64_t n_rows, uint64_t n,
                                      const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp, const ks_astats_opts *opts,
                                      ks_astats **out) {
    return as_entry(ctx, opts, nullptr, false, out,
                    [&](const ks_astats_opts &o) { return as_run(ctx, d_row_offsets, d_score, n_rows, n, hits, q_comp, t_comp, o, out); });
}
extern "C" int ks_rscores_stats(ks_ctx *ctx, const ks_rscores *scores, const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp,
                                const ks_astats_opts *opts, ks_astats **out) {
    return as_entry(ctx, opts, nullptr, false, out, [&](const ks_astats_opts &o) {
        return as_run(ctx, scores->d_row_offsets, scores->d_score, scores->n_rows, scores->n_regions, hits, q_comp, t_comp, o, out);
    }, scores);
}
extern "C" int ks_raligns_stats(ks_ctx *ctx, const ks_raligns *alignments, const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp,
                                const ks_astats_opts *opts, ks_astats **out) {
    return as_entry(ctx, opts, alignments, true, out, [&](const ks_astats_opts &o) {
        KS_TRY(ks_refuse_by_profile(ctx, "alignment statistics", alignments)); // ((lambda, K) belong to a matrix, not to a profile's rows)
        return as_run(ctx, alignments->d_row_offsets, alignments->d_score, alignments->n_rows, alignments->n_regions, hits, q_comp, t_comp, o, out);
    }, alignments);
}
extern "C" int ks_hitalns_stats(ks_ctx *ctx, const ks_hitalns *stitched, const ks_raligns *alignments, const ks_hits *hits, const ks_rcomp *q_comp,
                                const ks_rcomp *t_comp, const ks_astats_opts *opts, ks_astats **out) {
    return as_entry(ctx, opts, alignments, true, out, [&](const ks_astats_opts &o) {
        return as_run(ctx, nullptr, stitched->d_score, stitched->n_rows, stitched->n_rows, hits, q_comp, t_comp, o, out);
    }, stitched, alignments);
}

extern "C" uint64_t ks_astats_n_rows(const ks_astats *s) { return s ? s->n_rows : 0; }
extern "C" uint64_t ks_astats_n_entries(const ks_astats *s) { return s ? s->n : 0; }
extern "C" uint64_t ks_astats_n_fallback(const ks_astats *s) { return s ? s->n_fallback : 0; }
extern "C" double ks_astats_lambda_std(const ks_astats *s) { return s ? s->lambda_std : 0.0; }
extern "C" double ks_astats_lambda_used(const ks_astats *s) { return s ? s->lambda_used : 0.0; }
extern "C" double ks_astats_k_used(const ks_astats *s) { return s ? s->K_used : 0.0; }
extern "C" uint32_t ks_astats_params_source(const ks_astats *s) { return s ? s->params_source : 0; }
extern "C" const uint8_t *ks_astats_device_status(const ks_astats *s) { return s ? s->d_status : nullptr; }
extern "C" const double *ks_astats_device_x(const ks_astats *s) { return s ? s->d_x : nullptr; }
extern "C" const double *ks_astats_device_lambda_ratio(const ks_astats *s) { return s ? s->d_ratio : nullptr; }
extern "C" const double *ks_astats_device_bit_score(const ks_astats *s) { return s ? s->d_bit : nullptr; }
extern "C" const double *ks_astats_device_evalue(const ks_astats *s) { return s ? s->d_evalue : nullptr; }
extern "C" const double *ks_astats_device_row_bit_score(const ks_astats *s) { return s ? s->d_row_bit : nullptr; }
extern "C" const double *ks_astats_device_row_evalue(const ks_astats *s) { return s ? s->d_row_evalue : nullptr; }
extern "C" int ks_astats_copy_to_host(ks_ctx *ctx, const ks_astats *s, uint8_t *status, double *x, double *lambda_ratio, double *bit_score,
                                      double *evalue, double *row_bit_score, double *row_evalue) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, s, status, x, lambda_ratio, bit_score, evalue, row_bit_score, row_evalue); });
}
extern "C" void ks_astats_free(ks_astats *s) { ks_obj_free(s); }
