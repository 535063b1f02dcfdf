// ks_signif.hip — ks_corpus_build / ks_hits_significance: does a hit's overlap mean anything?  Per hit row (qid, tid) the two
// sums that branchwater multisearch prints as prob_overlap and tf_idf_score (src/python/kmerseek/search.py:144-158,
// "calculate probability of overlap between target and query" switched on), over the hashes the two sketches share, in
// ascending hash order, starting from 0.0:
//     prob_overlap += ((double)abund_sum_Q(h) / (double)total(Q)) * ((double)abund_sum_T(h) / (double)total(T))
//     tf_idf       += ((double)abund_q(h) / (double)sum of q's abundances) * idf[doc_freq_T(h)]
// IEEE f64, one rounding per operation (no contraction into fma), no reassociation: bit-identical to a host loop that does
// the same.  idf[] is made on the host with libm's log and uploaded — the device never evaluates a logarithm.
//
//   corpus   per sketch set, once: the hashes sorted and cut into runs (ks_sorted_runs) -> per distinct hash its abundance
//            sum (u64, exact), the number of sketches that hold it, and the set's grand total
//   weights  one pass over the query CSR (a wave per query): the query's abundance sum, then per posting both corpus tables
//            searched and the two products stored as f64 (pw, tw) — a row only adds
//   rows     hit rows are ordered by (qid, tid).  A lane per short row walks the shorter run and searches the longer one from
//            where the last search ended; a row with |q| + |t| above SG_CUT is listed for k_sg_rows_wave, where the lanes of
//            one wave take 64 consecutive hashes of the shorter run, a ballot marks the shared ones, and their terms are added
//            serially in lane order through readlane (every lane keeps the same sums).  No f64 atomics, no tree reductions.
// The row pass counts what it adds: a count that is not the row's intersect means hits, sketches and corpora do not belong
// together (KS_ERR_INVALID_ARG; ks_last_error names the first such row).
#include <cmath>

#include "ks_device.h"

#define SG_CUT 128        // |q| + |t| above this: the wave path (KS_DEBUG_SIGNIF_WAVE_ROWS = 1 / 0 sends every row one way)
#define SG_WAVE_GRID 1024 // workgroups of k_sg_rows_wave (4 waves each, striding over the listed rows; see RA_LONG_GRID, ks_rows.hip)
enum { SG_BAD_ID = 0, SG_BAD_COUNT = 1, SG_BAD_CORPUS = 2 }; // words of the control block

struct ks_corpus {
    ks_ctx *ctx;
    ks_params params;
    u32 n_docs;      // sketches of the set, empty ones included
    u64 n_postings;  // (hash, sketch) pairs of the set: what it was built from
    u64 n_hashes;    // distinct hashes
    u64 total;       // sum of all abundances
    u32 max_doc_freq;
    u64 *d_hash, *d_sum;
    u32 *d_df;
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_hash, s.n_hashes); f(s.d_sum, s.n_hashes); f(s.d_df, s.n_hashes); }
};

struct ks_signif {
    ks_ctx *ctx;
    u64 n_rows;
    double *d_prob, *d_tfidf;
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_prob, s.n_rows); f(s.d_tfidf, s.n_rows); }
};

// ---- corpus ----------------------------------------------------------------------------------------------------------------
// acc[0] += the abundances of the whole set, acc[1] = the largest doc_freq (both exact: integer atomics, one per wave)
__global__ __launch_bounds__(256) void k_corpus_emit(const u64 *keys, const u32 *vals, const u64 *row_start, u32 n_rows, u64 *hashes,
                                                     u64 *sums, u32 *df, unsigned long long *acc) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x; // (no early return: the wave sum takes all 64 lanes)
    u64 w = 0;
    u32 d = 0;
    if (r < n_rows) {
        const u64 b = row_start[r], e = row_start[r + 1];
        w = ks_run_abund_sum(vals, b, e);
        d = (u32)(e - b); // a sketch holds a hash once: postings of the run = sketches that hold it
        hashes[r] = keys[b]; sums[r] = w; df[r] = d;
    }
    const u64 ws = ks_wave_sum64(w);
    d = ks_wave_max_u32(d);
    if ((threadIdx.x & 63) == 0) {
        if (ws) atomicAdd(&acc[0], (unsigned long long)ws);
        atomicMax(&acc[1], (unsigned long long)d);
    }
}

static int corpus_run(ks_ctx *ctx, const ks_sketches *in, ks_corpus *C) {
    const u64 n = in->n_hashes;
    if (n == 0) { // no hash anywhere: an empty table, total 0
        KS_TRY(ks_alloc(ctx, &C->d_hash, 1)); KS_TRY(ks_alloc(ctx, &C->d_sum, 1)); KS_TRY(ks_alloc(ctx, &C->d_df, 1));
        return KS_OK;
    }
    if (n >= 0xfffffff0ULL) return ks_fail(ctx, KS_ERR_CAPACITY, "corpus: %llu postings exceed one sort", (unsigned long long)n);
    ks_scratch sc(ctx);
    ks_runs R;
    KS_TRY(ks_sorted_runs(ctx, in, sc, &R));
    const u32 n_rows = R.n_rows;
    u64 *acc = nullptr;
    KS_TRY(sc.alloc(&acc, 2));
    KS_HIP(ctx, hipMemsetAsync(acc, 0, 2 * sizeof(u64), ctx->stream));
    C->n_hashes = n_rows;
    KS_TRY(ks_alloc(ctx, &C->d_hash, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &C->d_sum, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &C->d_df, (size_t)n_rows));
    KS_LAUNCH(ctx, "corpus_emit", k_corpus_emit, (n_rows + 255) / 256, 256, (const u64 *)R.keys, (const u32 *)R.vals, (const u64 *)R.row_start,
              n_rows, C->d_hash, C->d_sum, C->d_df, (unsigned long long *)acc);
    u64 *const rb = ctx->h_pin + KS_PIN_READ;
    KS_HIP(ctx, hipMemcpyAsync(rb, acc, 2 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    C->total = rb[0];
    C->max_doc_freq = (u32)rb[1];
    return KS_OK;
}

extern "C" int ks_corpus_build(ks_ctx *ctx, const ks_sketches *sketches, ks_corpus **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!sketches || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (sketches->ctx != ctx) return ks_fail(ctx, KS_ERR_INVALID_ARG, "corpus: sketches of another context");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(sketches))); // (the sort reads the hashes as one dense array)
    ks_result<ks_corpus> C(ctx, out, ks_corpus_free);
    C->params = sketches->params; C->n_docs = sketches->n_seqs; C->n_postings = sketches->n_hashes;
    KS_TRY(corpus_run(ctx, sketches, C));
    return C.commit();
    });
}

extern "C" uint64_t ks_corpus_n_hashes(const ks_corpus *c) { return c ? c->n_hashes : 0; }
extern "C" uint32_t ks_corpus_n_docs(const ks_corpus *c) { return c ? c->n_docs : 0; }
extern "C" uint64_t ks_corpus_total_abund(const ks_corpus *c) { return c ? c->total : 0; }

extern "C" int ks_corpus_copy_to_host(ks_ctx *ctx, const ks_corpus *c, uint64_t *hashes, uint64_t *abund_sum, uint32_t *doc_freq) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, hashes, abund_sum, doc_freq); });
}

extern "C" void ks_corpus_free(ks_corpus *c) { ks_obj_free(c); }

// ---- weights ---------------------------------------------------------------------------------------------------------------
struct sg_table {
    const u64 *hash, *sum;
    const u32 *df;
    u32 n;
    double total; // (double)total(S)
};

// One wave per query: its abundance sum, then per posting the two products.  A hash that the target corpus does not hold gets
// 0 twice (no row can use it); one that the QUERY corpus does not hold raises *flag: that corpus is not this set's.
__global__ __launch_bounds__(256) void k_sg_weights(const u64 *q_off, const u64 *q_hash, const u32 *q_abund, u32 n_seqs, sg_table CQ, sg_table CT,
                                                    const double *idf, double *pw, double *tw, unsigned long long *flag) {
#pragma clang fp contract(off)
    const u32 s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_seqs) return; // (uniform per wave)
    const u64 b = q_off[s], e = q_off[s + 1];
    u64 part = 0;
    for (u64 j = b + lane; j < e; j += 64) part += q_abund[j];
    const double q_sum = (double)ks_wave_sum64(part);
    for (u64 j = b + lane; j < e; j += 64) {
        const u64 h = q_hash[j];
        const u32 iq = ks_lower_bound_u64(CQ.hash, CQ.n, h), it = ks_lower_bound_u64(CT.hash, CT.n, h);
        const bool in_q = iq < CQ.n && CQ.hash[iq] == h, in_t = it < CT.n && CT.hash[it] == h;
        if (!in_q) atomicOr(flag, 1ULL);
        double p = 0.0, t = 0.0;
        if (in_q && in_t) {
            const double fq = (double)CQ.sum[iq] / CQ.total, ft = (double)CT.sum[it] / CT.total;
            p = fq * ft;
            const double tf = (double)q_abund[j] / q_sum;
            t = tf * idf[CT.df[it]];
        }
        pw[j] = p; tw[j] = t;
    }
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
struct sg_rows_in {
    const u64 *q_off, *q_hash, *t_off, *t_hash;
    const double *pw, *tw;
    const u32 *qid, *tid, *isect;
    u32 n_rows, n_q, n_t;
};

// A lane per row.  mode: 0 every row here, 1 every row to the wave kernel, 2 by length.  wave_rows[0] counts the listed rows.
__global__ __launch_bounds__(256) void k_sg_rows(sg_rows_in R, int mode, double *prob, double *tfidf, u32 *wave_rows, unsigned long long *bad) {
#pragma clang fp contract(off)
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R.n_rows) return;
    const u32 q = R.qid[r], t = R.tid[r];
    if (q >= R.n_q || t >= R.n_t) { ks_first_bad(bad, SG_BAD_ID, r); prob[r] = 0.0; tfidf[r] = 0.0; return; }
    const ks_run_pair P = ks_run_pair_of(R.q_off, R.q_hash, R.t_off, R.t_hash, q, t);
    if (mode == 1 || (mode == 2 && (u64)P.nw + P.ns > SG_CUT)) { ks_row_list_push(wave_rows, r); return; }
    double po = 0.0, tf = 0.0;
    const u32 cnt = ks_shared_walk_lane(P, [&](u32 pos, u32) { // the QUERY posting: the weights are its
        po += R.pw[P.qb + pos];
        tf += R.tw[P.qb + pos];
    });
    if (cnt != R.isect[r]) ks_first_bad(bad, SG_BAD_COUNT, r);
    prob[r] = po; tfidf[r] = tf;
}

// The listed rows, a wave per row (ks_row_list_walk, ks_shared_walk_wave): the terms of a chunk's shared hashes are added in lane
// order: ascending hash.
__global__ __launch_bounds__(256) void k_sg_rows_wave(sg_rows_in R, const u32 *wave_rows, double *prob, double *tfidf, unsigned long long *bad) {
    const u32 lane = threadIdx.x & 63;
    ks_row_list_walk(wave_rows, R.n_rows, [&](u32 r) {
        const ks_run_pair P = ks_run_pair_of(R.q_off, R.q_hash, R.t_off, R.t_hash, R.qid[r], R.tid[r]); // (in range: k_sg_rows lists no other row)
        double po = 0.0, tf = 0.0;
        const u32 cnt = ks_shared_walk_wave(P, lane, [&](bool found, u32 pos, u64 m, u32) {
            const double x = found ? R.pw[P.qb + pos] : 0.0, y = found ? R.tw[P.qb + pos] : 0.0;
            ks_wave_add_ordered(m, po, x, tf, y);
        });
        if (lane == 0) {
            if (cnt != R.isect[r]) ks_first_bad(bad, SG_BAD_COUNT, r);
            prob[r] = po; tfidf[r] = tf;
        }
    });
}

static int signif_run(ks_ctx *ctx, const ks_sketches *Q, const ks_sketches *T, const ks_corpus *CQ, const ks_corpus *CT, const ks_hits *H,
                      ks_signif *S) {
    const u64 n_rows = H->n_hits;
    S->n_rows = n_rows;
    KS_TRY(ks_alloc(ctx, &S->d_prob, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &S->d_tfidf, (size_t)n_rows));
    if (n_rows == 0) return KS_OK;
    if (n_rows >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "significance: 2^32 - 2 or more hit rows");
    if (Q->n_hashes == 0 || T->n_hashes == 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "significance: %llu hit rows, but a sketch set is empty: the inputs do not belong together",
                       (unsigned long long)n_rows);

    ks_scratch sc(ctx);
    double *pw = nullptr, *tw = nullptr, *idf = nullptr;
    u32 *wave_rows = nullptr; // the rows of k_sg_rows_wave
    ks_ctl ctl; // [SG_BAD_ID], [SG_BAD_COUNT]: the first such row; [SG_BAD_CORPUS]: a query hash outside the query corpus
    KS_TRY(sc.alloc(&pw, (size_t)Q->n_hashes)); KS_TRY(sc.alloc(&tw, (size_t)Q->n_hashes));
    KS_TRY(sc.alloc(&idf, (size_t)CT->max_doc_freq + 1));
    KS_TRY(ks_row_list_alloc(ctx, sc, (size_t)n_rows, &wave_rows));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_SIGNIF, 2, 1));
    // smooth idf over the document frequencies the target corpus holds: libm's log, here on the host
    std::vector<double> h_idf((size_t)CT->max_doc_freq + 1);
    for (size_t d = 0; d < h_idf.size(); d++) h_idf[d] = std::log(((double)1 + (double)T->n_seqs) / ((double)1 + (double)d)) + 1.0;
    KS_TRY(ks_copy_h2d(ctx, idf, h_idf.data(), h_idf.size() * sizeof(double)));

    const sg_table tq = {CQ->d_hash, CQ->d_sum, CQ->d_df, (u32)CQ->n_hashes, (double)CQ->total};
    const sg_table tt = {CT->d_hash, CT->d_sum, CT->d_df, (u32)CT->n_hashes, (double)CT->total};
    KS_LAUNCH(ctx, "signif_weights", k_sg_weights, (Q->n_seqs + 3) / 4, 256, (const u64 *)Q->d_offsets, (const u64 *)Q->d_hashes,
              (const u32 *)Q->d_abunds, Q->n_seqs, tq, tt, (const double *)idf, pw, tw, ctl.words() + SG_BAD_CORPUS);
    int mode = 2;
    if (const char *f = ks_dbg(ctx, KS_DBG_SIGNIF_WAVE_ROWS)) mode = atoi(f) != 0 ? 1 : 0; // (tests: small inputs take both paths)
    const sg_rows_in R = {Q->d_offsets, Q->d_hashes, T->d_offsets, T->d_hashes, pw, tw, H->d_qid, H->d_tid, H->d_isect,
                          (u32)n_rows, Q->n_seqs, T->n_seqs};
    KS_LAUNCH(ctx, "signif_rows", k_sg_rows, (u32)((n_rows + 255) / 256), 256, R, mode, S->d_prob, S->d_tfidf, wave_rows,
              ctl.words());
    if (mode != 0)
        KS_LAUNCH(ctx, "signif_rows_wave", k_sg_rows_wave, SG_WAVE_GRID, 256, R, (const u32 *)wave_rows, S->d_prob, S->d_tfidf,
                  ctl.words());
    const ks_fetch_seg f = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (ctl.bad(SG_BAD_ID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "significance: hit row %llu names a query or target beyond the sketch sets (%u queries, %u targets)",
                       (unsigned long long)ctl[SG_BAD_ID], Q->n_seqs, T->n_seqs);
    if (ctl[SG_BAD_CORPUS] != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "significance: a query hash is not in the query corpus: the corpus was built from another set");
    if (ctl.bad(SG_BAD_COUNT))
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "significance: hit row %llu does not share `intersect` hashes in these sketches: hits and sketches do not belong together",
                       (unsigned long long)ctl[SG_BAD_COUNT]);
    return KS_OK;
}

extern "C" int ks_hits_significance(ks_ctx *ctx, const ks_sketches *queries, const ks_sketches *targets, const ks_corpus *q_corpus,
                                    const ks_corpus *t_corpus, const ks_hits *hits, const ks_signif_opts *opts, ks_signif **out) {
    return ks_guard(ctx, [&]() -> int {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "significance", opts->flags, 0, opts->reserved));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!queries || !targets || !q_corpus || !t_corpus || !hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    KS_TRY(ks_inputs_check_ctx(ctx, "significance", queries, targets, q_corpus, t_corpus, hits));
    KS_TRY(ks_params_check_same(ctx, "significance", "the sketch sets", queries->params, targets->params));
    const struct { const ks_corpus *c; const ks_sketches *s; const char *side; } pairs[2] = {{q_corpus, queries, "query"}, {t_corpus, targets, "target"}};
    for (const auto &p : pairs) {
        if (p.c->n_docs != p.s->n_seqs)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "significance: the %s corpus counts %u sketches, the %s set holds %u: a corpus of another set",
                           p.side, p.c->n_docs, p.side, p.s->n_seqs);
        if (!ks_same_params(p.c->params, p.s->params) || p.c->n_postings != p.s->n_hashes)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "significance: the %s corpus was built from another set (parameters or size differ)", p.side);
    }
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(queries))); // (the passes read both sets as plain CSRs)
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(targets)));
    ks_result<ks_signif> S(ctx, out, ks_signif_free);
    KS_TRY(signif_run(ctx, queries, targets, q_corpus, t_corpus, hits, S));
    if (hits->n_hits == 0) KS_TRY(ks_stream_wait(ctx));
    return S.commit();
    });
}

extern "C" uint64_t ks_signif_n_rows(const ks_signif *s) { return s ? s->n_rows : 0; }
extern "C" const double *ks_signif_device_prob_overlap(const ks_signif *s) { return s ? s->d_prob : nullptr; }
extern "C" const double *ks_signif_device_tf_idf(const ks_signif *s) { return s ? s->d_tfidf : nullptr; }

extern "C" int ks_signif_copy_to_host(ks_ctx *ctx, const ks_signif *s, double *prob_overlap, double *tf_idf) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, s, prob_overlap, tf_idf); });
}

extern "C" void ks_signif_free(ks_signif *s) { ks_obj_free(s); }
