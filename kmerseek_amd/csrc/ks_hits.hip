// ks_hits.hip — the hit list (ks_hits, ks_common.h): its column set (ks_hit_cols: who owns and frees what), its accessors and copies
// across the ABI, and what the passes that make a list from a list share — the move of the kept rows (ks_hits_best, ks_hits_gather),
// the concatenation of a sliced search's lists, the host halves of the row and segment lists.
#include "ks_device.h"

// ---- the column set ----
int ks_hit_cols::alloc(ks_ctx *ctx, size_t n, bool with_stats, u32 extra) {
    KS_TRY(ks_alloc(ctx, &d_qid, n)); KS_TRY(ks_alloc(ctx, &d_tid, n));
    KS_TRY(ks_alloc(ctx, &d_isect, n)); KS_TRY(ks_alloc(ctx, &d_nw, n));
    if (with_stats) { KS_TRY(ks_alloc(ctx, &d_median2, n)); KS_TRY(ks_alloc(ctx, &d_ss, n)); }
    if (extra & KS_COLS_RANKED) { KS_TRY(ks_alloc(ctx, &d_rank, n)); KS_TRY(ks_alloc(ctx, &d_src_row, n)); }
    if (extra & KS_COLS_GATHER) {
        KS_TRY(ks_alloc(ctx, &d_ga_unique, n)); KS_TRY(ks_alloc(ctx, &d_ga_remaining, n)); KS_TRY(ks_alloc(ctx, &d_ga_weighted, n));
    }
    return KS_OK;
}

void ks_hit_cols::release(ks_ctx *ctx) {
    if (d_block) { d_isect = nullptr; d_nw = nullptr; } // (they lie inside the block)
    void *const cols[] = {d_qid, d_tid, d_block, d_isect, d_nw, d_median2, d_ss, d_rank, d_src_row, d_ga_unique, d_ga_remaining, d_ga_weighted};
    for (void *p : cols) ks_pool_free(ctx, p); // (NULL: nothing happens)
    *this = ks_hit_cols{};
}

int ks_hit_cols::append(ks_ctx *ctx, u64 at, const ks_hit_cols &from, u64 n, bool stats) {
    const ks_column cols[] = {{d_qid + at, from.d_qid, n * sizeof(u32)},     {d_tid + at, from.d_tid, n * sizeof(u32)},
                              {d_isect + at, from.d_isect, n * sizeof(u32)}, {d_nw + at, from.d_nw, n * sizeof(u64)},
                              {stats ? d_median2 + at : nullptr, from.d_median2, n * sizeof(u64)},
                              {stats ? d_ss + at : nullptr, from.d_ss, n * sizeof(double)}};
    for (const ks_column &c : cols)
        if (c.dst) KS_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return KS_OK;
}

// ---- the object across the ABI ----
extern "C" void ks_hits_free(ks_hits *h) {
    if (h) h->release(h->ctx);
    delete h;
}
extern "C" uint64_t ks_hits_count(const ks_hits *h) { return h ? h->n_hits : 0; }
extern "C" uint64_t ks_hits_n_pair_instances(const ks_hits *h) { return h ? h->n_pair_instances : 0; }
extern "C" int ks_hits_partition_path(const ks_hits *h) {
    return ks_guard(nullptr, [&]() -> int { return h ? h->partition_path : -1;
    });
}
extern "C" int ks_hits_bucket_posting_bytes(const ks_hits *h) {
    return ks_guard(nullptr, [&]() -> int { return h ? h->bucket_posting_bytes : -1;
    });
}
extern "C" int ks_hits_copy_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *qid, uint32_t *tid, uint32_t *intersect,
                                    uint64_t *n_weighted) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !h) return KS_ERR_INVALID_ARG;
    const size_t n = (size_t)h->n_hits;
    return ks_columns_to_host(ctx, {{qid, h->d_qid, n * sizeof(u32)}, {tid, h->d_tid, n * sizeof(u32)},
                                    {intersect, h->d_isect, n * sizeof(u32)}, {n_weighted, h->d_nw, n * sizeof(u64)}});
    });
}
extern "C" const uint32_t *ks_hits_device_qid(const ks_hits *h) { return h ? h->d_qid : nullptr; }
extern "C" const uint32_t *ks_hits_device_tid(const ks_hits *h) { return h ? h->d_tid : nullptr; }
extern "C" const uint32_t *ks_hits_device_intersect(const ks_hits *h) { return h ? h->d_isect : nullptr; }
extern "C" const uint64_t *ks_hits_device_n_weighted(const ks_hits *h) { return h ? h->d_nw : nullptr; }

__global__ __launch_bounds__(256) void k_copy_add_u32(const u32 *in, u32 *out, u64 n, u32 add) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + add;
}

extern "C" int ks_hits_copy_to_device(ks_ctx *ctx, const ks_hits *h, uint32_t qid_base, uint32_t tid_base, uint32_t *d_qid,
                                      uint32_t *d_tid, uint32_t *d_intersect, uint64_t *d_n_weighted) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !h) return KS_ERR_INVALID_ARG;
    KS_HIP(ctx, hipSetDevice(ctx->device));
    const u64 n = h->n_hits;
    if (n == 0) return KS_OK;
    const u32 g = (u32)((n + 255) / 256);
    if (d_qid) KS_LAUNCH(ctx, "hits_copy", k_copy_add_u32, g, 256, (const u32 *)h->d_qid, d_qid, n, qid_base);
    if (d_tid) KS_LAUNCH(ctx, "hits_copy", k_copy_add_u32, g, 256, (const u32 *)h->d_tid, d_tid, n, tid_base);
    if (d_intersect) KS_HIP(ctx, hipMemcpyAsync(d_intersect, h->d_isect, (size_t)n * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_n_weighted) KS_HIP(ctx, hipMemcpyAsync(d_n_weighted, h->d_nw, (size_t)n * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    return KS_OK;
    });
}

extern "C" int ks_hits_has_abund_stats(const ks_hits *h) { return h && h->has_stats ? 1 : 0; }
extern "C" const uint64_t *ks_hits_device_median2(const ks_hits *h) { return h && h->has_stats ? h->d_median2 : nullptr; }
extern "C" const double *ks_hits_device_abund_ss(const ks_hits *h) { return h && h->has_stats ? h->d_ss : nullptr; }
extern "C" int ks_hits_copy_abund_stats_to_host(ks_ctx *ctx, const ks_hits *h, uint64_t *median2, double *ss) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!h) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (!h->has_stats) return ks_fail(ctx, KS_ERR_INVALID_ARG, "these hits were searched without KS_SEARCH_ABUND_STATS");
    const size_t n = (size_t)h->n_hits;
    return ks_columns_to_host(ctx, {{median2, h->d_median2, n * sizeof(u64)}, {ss, h->d_ss, n * sizeof(double)}});
    });
}

extern "C" const uint32_t *ks_hits_device_rank(const ks_hits *h) { return h ? h->d_rank : nullptr; }
extern "C" const uint32_t *ks_hits_device_src_row(const ks_hits *h) { return h ? h->d_src_row : nullptr; }

extern "C" int ks_hits_copy_best_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *rank, uint32_t *src_row) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!h) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (!h->d_rank) return ks_fail(ctx, KS_ERR_INVALID_ARG, "these hits did not come from ks_hits_best");
    const size_t n = (size_t)h->n_hits;
    return ks_columns_to_host(ctx, {{rank, h->d_rank, n * sizeof(u32)}, {src_row, h->d_src_row, n * sizeof(u32)}});
    });
}

extern "C" const uint32_t *ks_hits_device_unique_intersect(const ks_hits *h) { return h ? h->d_ga_unique : nullptr; }
extern "C" const uint32_t *ks_hits_device_remaining(const ks_hits *h) { return h ? h->d_ga_remaining : nullptr; }
extern "C" const uint64_t *ks_hits_device_unique_weighted(const ks_hits *h) { return h ? h->d_ga_weighted : nullptr; }

extern "C" int ks_hits_copy_gather_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *unique_intersect, uint32_t *remaining,
                                           uint64_t *unique_weighted) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!h) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (!h->d_ga_unique) return ks_fail(ctx, KS_ERR_INVALID_ARG, "these hits did not come from ks_hits_gather");
    const size_t n = (size_t)h->n_hits;
    return ks_columns_to_host(ctx, {{unique_intersect, h->d_ga_unique, n * sizeof(u32)}, {remaining, h->d_ga_remaining, n * sizeof(u32)},
                                    {unique_weighted, h->d_ga_weighted, n * sizeof(u64)}});
    });
}

// ---- a pass that keeps some rows of a hit list and returns a hit list (ks_hits_best, ks_hits_gather) ----
void ks_hits_inherit(ks_hits *B, const ks_hits *H) {
    B->n_pair_instances = H->n_pair_instances;
    B->partition_path = H->partition_path;
    B->bucket_posting_bytes = H->bucket_posting_bytes;
    B->has_stats = H->has_stats;
}

// the kept rows to their places: all columns, the rank and the row's index in the input (+ the gather columns: ks_hits_gather)
__global__ __launch_bounds__(256) void k_best_move(rf_cols in, u32 n_rows, const u32 *dst, const u32 *rank, u32 cap, u32 *qid, u32 *tid, u32 *isect,
                                                   u64 *nw, u64 *median2, double *ss, u32 *o_rank, u32 *o_src, ks_gather_cols ga, u32 *o_unique,
                                                   u32 *o_remaining, u64 *o_weighted) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u32 rk = rank[r], o = dst[r];
    if (rk == KS_RANK_NONE || o >= cap) return;
    rf_move(in, r, o, qid, tid, isect, nw, median2, ss);
    o_rank[o] = rk;
    o_src[o] = r;
    if (ga.unique) { o_unique[o] = ga.unique[r]; o_remaining[o] = ga.remaining[r]; o_weighted[o] = ga.weighted[r]; }
}

int ks_hits_move_ranked(ks_ctx *ctx, const ks_hits *H, u32 n_rows, const u32 *dst, const u32 *rank, u32 cap, ks_hits *B,
                        const ks_gather_cols *ga) {
    KS_LAUNCH(ctx, "best_move", k_best_move, (n_rows + 255) / 256, 256, H->rows(), n_rows, dst, rank, cap, B->d_qid, B->d_tid, B->d_isect, B->d_nw,
              B->d_median2, B->d_ss, B->d_rank, B->d_src_row, ga ? *ga : ks_gather_cols{nullptr, nullptr, nullptr}, B->d_ga_unique,
              B->d_ga_remaining, B->d_ga_weighted);
    return KS_OK;
}

int ks_hits_select_plan(ks_ctx *ctx, const char *what, const ks_hits *H, const ks_sketches *Q, u32 per_query, u32 *n, u64 *cap) {
    if (H->n_hits >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: 2^32 - 2 or more hit rows", what);
    *n = (u32)H->n_hits;
    *cap = *n;
    if (Q && per_query && (u64)Q->n_seqs * per_query < *cap) *cap = (u64)Q->n_seqs * per_query;
    return KS_OK;
}

int ks_hits_select_tail(ks_ctx *ctx, const char *what, const ks_hits *H, u32 n_rows, u32 *flags, const u32 *rank, u64 cap,
                        const ks_gather_cols *ga, const ks_ctl &ctl, u32 kept, const std::function<int()> &checks, ks_hits *B) {
    KS_TRY(ks_scan_u32_inplace(ctx, flags, n_rows, ctl.low32(kept)));
    KS_TRY(ks_hits_move_ranked(ctx, H, n_rows, flags, rank, (u32)cap, B, ga));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    KS_TRY(checks());
    if (ctl[kept] > cap)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: %llu rows kept where at most %llu can be: the rows are not ordered by (qid, tid)", what,
                       (unsigned long long)ctl[kept], (unsigned long long)cap);
    B->n_hits = ctl[kept];
    return KS_OK;
}

// ---- the lists of a sliced search in one ----
__global__ __launch_bounds__(256) void k_add_u32(u32 *a, u64 n, u32 v) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] += v;
}

int ks_hits_concat(ks_ctx *ctx, const std::vector<ks_hits *> &parts, const std::vector<u32> &firsts, bool has_stats, ks_hits **out) {
    ks_result<ks_hits> H(ctx, out, ks_hits_free);
    H->partition_path = 3;
    H->has_stats = has_stats;
    for (const ks_hits *h : parts) { H->n_hits += h->n_hits; H->n_pair_instances += h->n_pair_instances; }
    KS_TRY(H->alloc(ctx, (size_t)H->n_hits, has_stats, 0));
    u64 at = 0;
    for (size_t i = 0; i < parts.size(); i++) {
        ks_hits *const h = parts[i];
        const u64 n = h->n_hits;
        if (!n) continue;
        hipLaunchKernelGGL(k_add_u32, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, h->d_qid, n, firsts[i]);
        KS_TRY(H->append(ctx, at, *h, n, has_stats));
        at += n;
    }
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the copies read the parts, which their owner frees next)
    return H.commit();
}

// ---- row and segment lists (ks_device.h: ks_row_list_push, ks_seg_list_push), the host half ----
int ks_row_list_alloc(ks_ctx *ctx, ks_scratch &sc, size_t n_rows, u32 **list) {
    KS_TRY(sc.alloc(list, n_rows + 1));
    KS_HIP(ctx, hipMemsetAsync(*list, 0, sizeof(u32), ctx->stream));
    return KS_OK;
}
int ks_seg_list_alloc(ks_ctx *ctx, ks_scratch &sc, size_t cap, u32 **list) { return ks_row_list_alloc(ctx, sc, 2 * cap, list); }
int ks_seg_path_knob(const ks_ctx *ctx, int dbg_id, bool *small) {
    const char *f = ks_dbg(ctx, dbg_id);
    const int v = f ? atoi(f) : 0;
    *small = v == 3;
    return v == 1 ? 1 : (v == 2 || v == 3) ? 2 : 0;
}
