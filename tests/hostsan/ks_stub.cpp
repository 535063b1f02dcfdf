// ks_stub.cpp — the ks_* entry points the host layer calls, on the CPU oracle (see stub_common.h).
// TEST INFRASTRUCTURE ONLY.  Each function keeps the contract of include/kmerseek_amd.h (statuses, NULL handling, the
// union's saturation at 2^32 - 1) and computes with kso_sketch_batch / kso_kmer_positions / kso_manysearch /
// kso_intersect.  "Device" pointers are heap pointers of hip_stub.cpp.  The four pure-host entry points
// (ks_status_string, ks_moltype_from_string, ks_max_hash, ks_validate_and_resolve) are NOT here: the sanitizer
// programs link the product's own kmerseek_amd/csrc/ks_hostfn.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "../../include/kmerseek_amd.h"
#include "../../oracle/ks_oracle.h"
#include "stub_common.h"

struct ks_ctx {
    int device = 0;
    std::string err;
};
struct ks_sketches {
    ks_params p{};
    uint32_t n = 0;
    uint64_t n_windows = 0;
    std::vector<uint64_t> offs, hashes;
    std::vector<uint32_t> abunds;
};
struct ks_kmerpos {
    std::vector<uint32_t> seq, start;
    std::vector<uint64_t> hash;
};
struct ks_index {
    ks_sketches targets; // a copy: the index does not borrow the caller's set
};
struct ks_hits {
    bool stats = false;
    std::vector<uint32_t> qid, tid, isect;
    std::vector<uint64_t> nw, median2;
    std::vector<double> ss;
};

namespace {
bool g_capture = false; // (set between runs, read by the one thread that issues device batches)
std::vector<uint8_t> g_cap_res;
std::vector<uint64_t> g_cap_len;

int fail(ks_ctx *ctx, int status, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return status;
}
// stub_enter + the guard of the real boundary: nothing throws out of an entry point
template <typename F>
int entry(ks_ctx *ctx, const char *fn, F &&body) noexcept {
    try {
        if (const int e = stub_enter(fn)) return fail(ctx, e, "%s: injected failure", fn);
        return body();
    } catch (const std::bad_alloc &) {
        return fail(ctx, KS_ERR_OOM, "out of host memory (std::bad_alloc)");
    } catch (...) {
        return fail(ctx, KS_ERR_HIP, "internal error");
    }
}
int check_params(ks_ctx *ctx, const ks_params *p) {
    if (!p) return fail(ctx, KS_ERR_INVALID_ARG, "params is NULL");
    if (p->moltype > KS_HP)
        return fail(ctx, KS_ERR_INVALID_MOLTYPE, "Invalid moltype: %u, only 'protein', 'hp', or 'dayhoff' are supported", p->moltype);
    if (p->ksize < 1 || p->ksize > KS_MAX_KSIZE) return fail(ctx, KS_ERR_INVALID_KSIZE, "Invalid k-mer size: %u", p->ksize);
    if (p->scaled < 1) return fail(ctx, KS_ERR_INVALID_SCALED, "Invalid scaled: %u", p->scaled);
    return KS_OK;
}
int check_offsets(ks_ctx *ctx, const uint64_t *offs, uint32_t n) {
    if (offs[0] != 0) return fail(ctx, KS_ERR_INVALID_ARG, "seq_offsets[0] must be 0");
    for (uint32_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i]) return fail(ctx, KS_ERR_INVALID_ARG, "seq_offsets must ascend");
    return KS_OK;
}
// the batch's sketches into S (params checked by the caller)
void sketch_into(ks_sketches &S, const uint8_t *res, const uint64_t *offs, uint32_t n, const ks_params &p) {
    static const uint8_t none = 0;
    S.p = p;
    S.n = n;
    S.offs.assign((size_t)n + 1, 0);
    uint64_t windows = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = offs[i + 1] - offs[i];
        if (len >= p.ksize) windows += len - p.ksize + 1;
    }
    S.n_windows = windows;
    S.hashes.assign((size_t)windows + 1, 0);
    S.abunds.assign((size_t)windows + 1, 0);
    const uint64_t tot = kso_sketch_batch(res ? res : &none, offs, n, p.ksize, p.scaled, (int)p.moltype, p.seed, S.offs.data(),
                                          S.hashes.data(), S.abunds.data(), 1);
    S.hashes.resize((size_t)tot);
    S.abunds.resize((size_t)tot);
}
} // namespace

extern "C" {

void stub_capture(int on) {
    g_capture = on != 0;
    if (on) { g_cap_res.clear(); g_cap_len.clear(); }
}
const uint8_t *stub_captured_residues(uint64_t *n) { *n = g_cap_res.size(); return g_cap_res.data(); }
const uint64_t *stub_captured_lengths(uint64_t *n) { *n = g_cap_len.size(); return g_cap_len.data(); }

int ks_ctx_create(int device, void *, ks_ctx **out) {
    if (!out) return KS_ERR_INVALID_ARG;
    *out = nullptr;
    if (const int e = stub_enter("ks_ctx_create")) return e;
    if (device != 0) return KS_ERR_INVALID_ARG; // one device
    ks_ctx *ctx = new (std::nothrow) ks_ctx();
    if (!ctx) return KS_ERR_OOM;
    ctx->device = device;
    *out = ctx;
    return KS_OK;
}
void ks_ctx_destroy(ks_ctx *ctx) {
    (void)stub_enter("ks_ctx_destroy");
    delete ctx;
}
const char *ks_last_error(const ks_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int ks_sketch_batch(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_params *params,
                    ks_sketches **out) {
    return entry(ctx, "ks_sketch_batch", [&]() -> int {
        if (!ctx || !out || !seq_offsets) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_batch: NULL argument");
        *out = nullptr;
        if (const int st = check_params(ctx, params)) return st;
        if (const int st = check_offsets(ctx, seq_offsets, n_seqs)) return st;
        if (!residues && seq_offsets[n_seqs]) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_batch: residues is NULL");
        ks_sketches *S = new ks_sketches();
        try { sketch_into(*S, residues, seq_offsets, n_seqs, *params); } catch (...) { delete S; throw; }
        *out = S;
        return KS_OK;
    });
}

int ks_sketch_batch_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                           uint32_t max_seq_len, const ks_params *params, ks_sketches **out) {
    return entry(ctx, "ks_sketch_batch_device", [&]() -> int {
        if (!ctx || !out || !d_seq_offsets) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_batch_device: NULL argument");
        *out = nullptr;
        if (const int st = check_params(ctx, params)) return st;
        if (const int st = check_offsets(ctx, d_seq_offsets, n_seqs)) return st;
        if (d_seq_offsets[n_seqs] != n_residues) return fail(ctx, KS_ERR_INVALID_ARG, "n_residues is not seq_offsets[n_seqs]");
        if (!d_residues && n_residues) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_batch_device: residues is NULL");
        if (max_seq_len)
            for (uint32_t i = 0; i < n_seqs; i++)
                if (d_seq_offsets[i + 1] - d_seq_offsets[i] > max_seq_len)
                    return fail(ctx, KS_ERR_INVALID_ARG, "max_seq_len is smaller than the longest sequence");
        if (g_capture) {
            if (n_residues) g_cap_res.insert(g_cap_res.end(), d_residues, d_residues + n_residues);
            for (uint32_t i = 0; i < n_seqs; i++) g_cap_len.push_back(d_seq_offsets[i + 1] - d_seq_offsets[i]);
        }
        ks_sketches *S = new ks_sketches();
        try { sketch_into(*S, d_residues, d_seq_offsets, n_seqs, *params); } catch (...) { delete S; throw; }
        *out = S;
        return KS_OK;
    });
}

uint64_t ks_sketches_n_hashes(const ks_sketches *s) { return s ? s->hashes.size() : 0; }
uint64_t ks_sketches_n_windows(const ks_sketches *s) { return s ? s->n_windows : 0; }

int ks_sketches_copy_to_host(ks_ctx *ctx, const ks_sketches *s, uint64_t *offsets, uint64_t *hashes, uint32_t *abunds) {
    return entry(ctx, "ks_sketches_copy_to_host", [&]() -> int {
        if (!ctx || !s) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketches_copy_to_host: NULL argument");
        if (offsets) std::copy(s->offs.begin(), s->offs.end(), offsets);
        if (hashes) std::copy(s->hashes.begin(), s->hashes.end(), hashes);
        if (abunds) std::copy(s->abunds.begin(), s->abunds.end(), abunds);
        return KS_OK;
    });
}

int ks_sketches_from_host(ks_ctx *ctx, const uint64_t *offsets, const uint64_t *hashes, const uint32_t *abunds, uint32_t n_seqs,
                          const ks_params *params, ks_sketches **out) {
    return entry(ctx, "ks_sketches_from_host", [&]() -> int {
        if (!ctx || !out || !offsets) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketches_from_host: NULL argument");
        *out = nullptr;
        if (const int st = check_params(ctx, params)) return st;
        if (const int st = check_offsets(ctx, offsets, n_seqs)) return st;
        const uint64_t tot = offsets[n_seqs];
        if (tot && (!hashes || !abunds)) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketches_from_host: NULL argument");
        ks_sketches *S = new ks_sketches();
        try {
            S->p = *params;
            S->n = n_seqs;
            S->offs.assign(offsets, offsets + n_seqs + 1);
            S->hashes.assign(hashes, hashes + tot);
            S->abunds.assign(abunds, abunds + tot);
        } catch (...) { delete S; throw; }
        *out = S;
        return KS_OK;
    });
}

int ks_sketches_union(ks_ctx *ctx, const ks_sketches *in, ks_sketches **out) {
    return entry(ctx, "ks_sketches_union", [&]() -> int {
        if (!ctx || !in || !out) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketches_union: NULL argument");
        *out = nullptr;
        std::vector<std::pair<uint64_t, uint32_t>> all(in->hashes.size());
        for (size_t i = 0; i < all.size(); i++) all[i] = {in->hashes[i], in->abunds[i]};
        std::sort(all.begin(), all.end());
        ks_sketches *U = new ks_sketches();
        try {
            U->p = in->p;
            U->n = 1;
            U->n_windows = in->n_windows;
            for (size_t i = 0; i < all.size();) {
                uint64_t sum = 0;
                size_t j = i;
                for (; j < all.size() && all[j].first == all[i].first; j++) sum += all[j].second;
                U->hashes.push_back(all[i].first);
                U->abunds.push_back((uint32_t)std::min<uint64_t>(sum, 0xffffffffULL)); // saturates at 2^32 - 1
                i = j;
            }
            U->offs = {0, (uint64_t)U->hashes.size()};
        } catch (...) { delete U; throw; }
        *out = U;
        return KS_OK;
    });
}

void ks_sketches_free(ks_sketches *s) {
    (void)stub_enter("ks_sketches_free");
    delete s;
}

int ks_kmer_positions(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_params *params,
                      ks_kmerpos **out) {
    return entry(ctx, "ks_kmer_positions", [&]() -> int {
        if (!ctx || !out || !seq_offsets) return fail(ctx, KS_ERR_INVALID_ARG, "ks_kmer_positions: NULL argument");
        *out = nullptr;
        if (const int st = check_params(ctx, params)) return st;
        if (const int st = check_offsets(ctx, seq_offsets, n_seqs)) return st;
        if (!residues && seq_offsets[n_seqs]) return fail(ctx, KS_ERR_INVALID_ARG, "ks_kmer_positions: residues is NULL");
        ks_sketches S;
        sketch_into(S, residues, seq_offsets, n_seqs, *params);
        ks_kmerpos *K = new ks_kmerpos();
        try {
            std::vector<uint32_t> starts;
            std::vector<uint64_t> hashes;
            for (uint32_t i = 0; i < n_seqs; i++) {
                const uint64_t len = seq_offsets[i + 1] - seq_offsets[i];
                if (len < params->ksize) continue;
                if (len > 0xfffffff0ULL) { delete K; return fail(ctx, KS_ERR_INVALID_ARG, "sequence too long for u32 starts"); }
                const size_t cap = (size_t)(len - params->ksize + 1);
                starts.assign(cap, 0);
                hashes.assign(cap, 0);
                const size_t c = kso_kmer_positions(residues + seq_offsets[i], (size_t)len, params->ksize, (int)params->moltype, params->seed,
                                                    S.hashes.data() + S.offs[i], (size_t)(S.offs[i + 1] - S.offs[i]), 0, starts.data(),
                                                    hashes.data());
                for (size_t j = 0; j < c; j++) { K->seq.push_back(i); K->start.push_back(starts[j]); K->hash.push_back(hashes[j]); }
            }
        } catch (...) { delete K; throw; }
        *out = K;
        return KS_OK;
    });
}
uint64_t ks_kmerpos_count(const ks_kmerpos *p) { return p ? p->seq.size() : 0; }
int ks_kmerpos_copy_to_host(ks_ctx *ctx, const ks_kmerpos *p, uint32_t *seq, uint32_t *start, uint64_t *hash) {
    return entry(ctx, "ks_kmerpos_copy_to_host", [&]() -> int {
        if (!ctx || !p) return fail(ctx, KS_ERR_INVALID_ARG, "ks_kmerpos_copy_to_host: NULL argument");
        if (seq) std::copy(p->seq.begin(), p->seq.end(), seq);
        if (start) std::copy(p->start.begin(), p->start.end(), start);
        if (hash) std::copy(p->hash.begin(), p->hash.end(), hash);
        return KS_OK;
    });
}
void ks_kmerpos_free(ks_kmerpos *p) {
    (void)stub_enter("ks_kmerpos_free");
    delete p;
}

int ks_index_build(ks_ctx *ctx, const ks_sketches *targets, ks_index **out) {
    return entry(ctx, "ks_index_build", [&]() -> int {
        if (!ctx || !targets || !out) return fail(ctx, KS_ERR_INVALID_ARG, "ks_index_build: NULL argument");
        *out = nullptr;
        ks_index *ix = new ks_index();
        try { ix->targets = *targets; } catch (...) { delete ix; throw; }
        *out = ix;
        return KS_OK;
    });
}
void ks_index_free(ks_index *ix) {
    (void)stub_enter("ks_index_free");
    delete ix;
}

int ks_sketch_search_ex(ks_ctx *ctx, const ks_index *index, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs,
                        const ks_search_opts *opts, ks_sketches **sketches_out, ks_hits **hits_out) {
    return entry(ctx, "ks_sketch_search_ex", [&]() -> int {
        if (sketches_out) *sketches_out = nullptr;
        if (hits_out) *hits_out = nullptr;
        // options first, before any work
        if (opts) {
            if (opts->reserved) return fail(ctx, KS_ERR_INVALID_ARG, "search options: reserved must be 0");
            if (opts->flags & ~KS_SEARCH_ABUND_STATS) return fail(ctx, KS_ERR_INVALID_ARG, "search options: unknown flags");
            if (!(opts->min_containment >= 0.0)) return fail(ctx, KS_ERR_INVALID_ARG, "search options: min_containment must be >= 0");
        }
        if (!ctx || !index || !hits_out || !seq_offsets) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_search_ex: NULL argument");
        if (const int st = check_offsets(ctx, seq_offsets, n_seqs)) return st;
        if (!residues && seq_offsets[n_seqs]) return fail(ctx, KS_ERR_INVALID_ARG, "ks_sketch_search_ex: residues is NULL");
        const bool stats = opts && (opts->flags & KS_SEARCH_ABUND_STATS);
        const double mc = opts ? opts->min_containment : 0.0;
        const ks_sketches &T = index->targets;
        ks_sketches *Q = new ks_sketches();
        ks_hits *H = nullptr;
        try {
            sketch_into(*Q, residues, seq_offsets, n_seqs, T.p);
            H = new ks_hits();
            H->stats = stats;
            static const uint64_t z64 = 0;
            static const uint32_t z32 = 0;
            const uint64_t *qm = Q->hashes.empty() ? &z64 : Q->hashes.data();
            const uint64_t *tm = T.hashes.empty() ? &z64 : T.hashes.data();
            const uint32_t *ta = T.abunds.empty() ? &z32 : T.abunds.data();
            const uint64_t n = kso_manysearch(Q->offs.data(), qm, 0, n_seqs, T.offs.data(), tm, ta, T.n, nullptr, nullptr, nullptr, nullptr, 0, 1);
            std::vector<uint32_t> qid((size_t)n + 1), tid((size_t)n + 1), isect((size_t)n + 1);
            std::vector<uint64_t> nw((size_t)n + 1);
            kso_manysearch(Q->offs.data(), qm, 0, n_seqs, T.offs.data(), tm, ta, T.n, qid.data(), tid.data(), isect.data(), nw.data(), n, 1);
            std::vector<uint32_t> shared;
            for (uint64_t r = 0; r < n; r++) {
                const uint32_t q = qid[r], t = tid[r];
                const size_t nq = (size_t)(Q->offs[q + 1] - Q->offs[q]), nt = (size_t)(T.offs[t + 1] - T.offs[t]);
                if ((double)isect[r] / (double)nq < mc) continue; // kept iff intersect / |q| >= min_containment
                H->qid.push_back(q); H->tid.push_back(t); H->isect.push_back(isect[r]); H->nw.push_back(nw[r]);
                if (!stats) continue;
                // median2 and ss computed plainly from the shared target abundances, ascending (ks_search_opts)
                shared.assign(std::min(nq, nt) + 1, 0);
                uint64_t w = 0;
                const uint64_t c = kso_intersect(qm + Q->offs[q], nq, tm + T.offs[t], ta + T.offs[t], nt, &w, shared.data());
                shared.resize((size_t)c);
                std::sort(shared.begin(), shared.end());
                const size_t m = shared.size();
                H->median2.push_back(m % 2 ? 2ULL * shared[m / 2] : (uint64_t)shared[m / 2 - 1] + shared[m / 2]);
                double sum = 0.0;
                for (uint32_t a : shared) sum += (double)a;
                const double mean = sum / (double)m;
                double ss = 0.0;
                for (uint32_t a : shared) { const double d = (double)a - mean; ss += d * d; }
                H->ss.push_back(ss);
            }
        } catch (...) { delete Q; delete H; throw; }
        if (sketches_out) *sketches_out = Q; else delete Q;
        *hits_out = H;
        return KS_OK;
    });
}

uint64_t ks_hits_count(const ks_hits *h) { return h ? h->qid.size() : 0; }
int ks_hits_copy_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *qid, uint32_t *tid, uint32_t *intersect, uint64_t *n_weighted) {
    return entry(ctx, "ks_hits_copy_to_host", [&]() -> int {
        if (!ctx || !h) return fail(ctx, KS_ERR_INVALID_ARG, "ks_hits_copy_to_host: NULL argument");
        if (qid) std::copy(h->qid.begin(), h->qid.end(), qid);
        if (tid) std::copy(h->tid.begin(), h->tid.end(), tid);
        if (intersect) std::copy(h->isect.begin(), h->isect.end(), intersect);
        if (n_weighted) std::copy(h->nw.begin(), h->nw.end(), n_weighted);
        return KS_OK;
    });
}
int ks_hits_copy_abund_stats_to_host(ks_ctx *ctx, const ks_hits *h, uint64_t *median2, double *ss) {
    return entry(ctx, "ks_hits_copy_abund_stats_to_host", [&]() -> int {
        if (!ctx || !h) return fail(ctx, KS_ERR_INVALID_ARG, "ks_hits_copy_abund_stats_to_host: NULL argument");
        if (!h->stats) return fail(ctx, KS_ERR_INVALID_ARG, "hits were searched without KS_SEARCH_ABUND_STATS");
        if (median2) std::copy(h->median2.begin(), h->median2.end(), median2);
        if (ss) std::copy(h->ss.begin(), h->ss.end(), ss);
        return KS_OK;
    });
}
void ks_hits_free(ks_hits *h) {
    (void)stub_enter("ks_hits_free");
    delete h;
}

} // extern "C"
