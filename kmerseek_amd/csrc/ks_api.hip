// ks_api.hip — the extern "C" entry points of include/kmerseek_amd.h that move data across the
// boundary (host buffers <-> HBM) and own the opaque result objects (the hit list: ks_hits.hip), plus the k-mer
// position kernel.
#include "ks_device.h"

// ---------------------------------------------------------------------------------------------
// sketches
// ---------------------------------------------------------------------------------------------
extern "C" int ks_sketch_batch_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets,
                                      uint32_t n_seqs, uint64_t n_residues, uint32_t max_seq_len,
                                      const ks_params *params, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out || (!d_seq_offsets) || (!d_residues && n_residues)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    return ks_sketch_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, params, 0, 0, 0, out);
    });
}

extern "C" int ks_sketch_queries_device(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues,
                                        const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                                        uint32_t max_seq_len, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!index || !out || (!d_seq_offsets) || (!d_residues && n_residues)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    return ks_sketch_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, &index->params,
                                 index->pbits, (index->fp_layout && index->fp_shift == 32 - index->pbits) ? 1 : 0, 0, out);
    });
}

// A batch uploaded from host arrays for one call.  Its two blocks go back to the pool when the owner leaves scope, behind a
// wait: the uploads read the caller's arrays and the call's launches read the blocks.
struct ks_upload {
    ks_ctx *ctx;
    u8 *d_res = nullptr;
    u64 *d_offs = nullptr;
    u64 n_res = 0;
    u32 max_len = 0;
    explicit ks_upload(ks_ctx *c) : ctx(c) {}
    ks_upload(const ks_upload &) = delete;
    ~ks_upload() {
        (void)hipStreamSynchronize(ctx->stream);
        ks_pool_free(ctx, d_res);
        ks_pool_free(ctx, d_offs);
    }
    int upload(const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs);
};

int ks_upload::upload(const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs) {
    if (!seq_offsets) return ks_fail(ctx, KS_ERR_INVALID_ARG, "seq_offsets is NULL");
    u64 total = seq_offsets[n_seqs];
    u64 mx = 0;
    for (u32 s = 0; s < n_seqs; s++) {
        if (seq_offsets[s + 1] < seq_offsets[s]) return ks_fail(ctx, KS_ERR_INVALID_ARG, "seq_offsets must be ascending (record %u)", s);
        u64 l = seq_offsets[s + 1] - seq_offsets[s];
        mx = l > mx ? l : mx;
    }
    if (seq_offsets[0] != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "seq_offsets[0] must be 0");
    if (mx > 0xfffffff0ULL) return ks_fail(ctx, KS_ERR_INVALID_ARG, "sequence longer than 2^32 residues");
    if (total && !residues) return ks_fail(ctx, KS_ERR_INVALID_ARG, "residues is NULL");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_alloc(ctx, &d_res, (size_t)total + 16));
    KS_TRY(ks_alloc(ctx, &d_offs, (size_t)n_seqs + 1));
    if (total) KS_TRY(ks_copy_h2d(ctx, d_res, residues, (size_t)total));
    KS_HIP(ctx, hipMemcpyAsync(d_offs, seq_offsets, ((size_t)n_seqs + 1) * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    n_res = total;
    max_len = (u32)mx;
    return KS_OK;
}

extern "C" int ks_sketch_batch(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs,
                               const ks_params *params, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "out is NULL");
    KS_TRY(ks_check_params(ctx, params));
    ks_upload U(ctx);
    KS_TRY(U.upload(residues, seq_offsets, n_seqs));
    return ks_sketch_device_impl(ctx, U.d_res, U.d_offs, n_seqs, U.n_res, U.max_len, params, 0, 0, 0, out);
    });
}

extern "C" int ks_sketch_translated(ks_ctx *ctx, const uint8_t *nt, const uint64_t *offsets, uint32_t n_seqs, const ks_params *params,
                                    ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    KS_TRY(ks_check_params(ctx, params));
    if (6 * (u64)n_seqs > 0xffffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "sketch_translated: the six frames of %u records do not fit 32-bit sequence ids", n_seqs);
    ks_upload U(ctx);
    KS_TRY(U.upload(nt, offsets, n_seqs));
    return ks_sketch_translated_impl(ctx, U.d_res, U.d_offs, n_seqs, U.n_res, U.max_len, params, out);
    });
}

extern "C" int ks_mask_batch(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_mask_opts *opts,
                             ks_mask **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "mask: out is NULL");
    *out = nullptr;
    KS_TRY(ks_mask_opts_check(ctx, "mask", opts));
    ks_upload U(ctx);
    KS_TRY(U.upload(residues, seq_offsets, n_seqs));
    return ks_mask_device_impl(ctx, U.d_res, U.d_offs, n_seqs, U.n_res, opts, out);
    });
}

extern "C" int ks_sketch_masked(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_params *params,
                                const ks_mask_opts *opts, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketch_masked: out is NULL");
    *out = nullptr;
    KS_TRY(ks_check_params(ctx, params));
    KS_TRY(ks_mask_opts_check(ctx, "sketch_masked", opts));
    ks_upload U(ctx);
    KS_TRY(U.upload(residues, seq_offsets, n_seqs));
    return ks_sketch_masked_impl(ctx, U.d_res, U.d_offs, n_seqs, U.n_res, U.max_len, params, opts, out);
    });
}

// ---- slots -> plain CSR --------------------------------------------------------------------------------------------------
// A sketch call leaves every sequence a slot as long as its KEPT hashes (ks_common.h: ks_sketches); where a sequence repeats a
// k-mer its distinct hashes fill only the head of the slot.  One gather (one wave per sequence) closes the gaps: new offsets =
// exclusive scan of the distinct counts.  Only batches with repeats pay for it, and only when something reads the arrays as a
// plain CSR (copies to the host, the device accessors of the ABI, an index build, a search that starts from the CSR, a union).
// cap: entries nh / na hold (n_hashes); a scan total beyond it is a count mismatch, which the host reports — nothing lands behind cap.
__global__ __launch_bounds__(256) void k_dense_gather(const u64 *old_offs, const u64 *new_offs, const u64 *oh, const u32 *oa, u32 n_seqs,
                                                      u64 *nh, u32 *na, u64 cap) {
    const u32 s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_seqs) return;
    const u64 src = old_offs[s], dst = new_offs[s], n = new_offs[s + 1] - dst;
    for (u64 j = threadIdx.x & 63; j < n && dst + j < cap; j += 64) { nh[dst + j] = oh[src + j]; na[dst + j] = oa[src + j]; }
}

int ks_sketches_make_dense(ks_ctx *ctx, ks_sketches *S) {
    if (!S || !S->gapped) return KS_OK;
    if (S->pending) return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketches with a pending read-back cannot be made dense");
    if (!S->d_counts) return ks_fail(ctx, KS_ERR_HIP, "internal error: gapped sketches without per-sequence counts");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_scratch sc(ctx); // (the new arrays are scratch until they replace the old ones)
    u64 *no = nullptr, *nh = nullptr;
    u32 *na = nullptr;
    KS_TRY(sc.alloc(&no, (size_t)S->n_seqs + 1));
    KS_TRY(sc.alloc(&nh, (size_t)S->n_hashes));
    KS_TRY(sc.alloc(&na, (size_t)S->n_hashes));
    KS_TRY(ks_scan_u32_to_u64(ctx, S->d_counts, no, S->n_seqs));
    if (S->n_seqs)
        KS_LAUNCH(ctx, "dense_gather", k_dense_gather, (S->n_seqs + 3) / 4, 256, (const u64 *)S->d_offsets, (const u64 *)no,
                  (const u64 *)S->d_hashes, (const u32 *)S->d_abunds, S->n_seqs, nh, na, S->n_hashes);
    // the scan total (the distinct counts summed) must be the n_hashes the arrays were sized by: read with the scan status
    u64 *const total = ctx->h_pin + KS_PIN_DENSE;
    *total = 0;
    KS_HIP(ctx, hipMemcpyAsync(total, no + S->n_seqs, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    KS_TRY(ks_scan_status_fetch(ctx));
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    KS_TRY(ks_scan_status_check(ctx));
    if (*total != S->n_hashes)
        return ks_fail(ctx, KS_ERR_HIP, "internal error: sketch counts sum to %llu, but the batch holds %llu distinct hashes",
                       (unsigned long long)*total, (unsigned long long)S->n_hashes);
    ks_pool_free(ctx, S->d_offsets); ks_pool_free(ctx, S->d_hashes); ks_pool_free(ctx, S->d_abunds);
    S->d_offsets = sc.keep(no); S->d_hashes = sc.keep(nh); S->d_abunds = sc.keep(na);
    S->n_slots = S->n_hashes;
    S->gapped = false;
    return KS_OK;
}

extern "C" uint32_t ks_sketches_n_seqs(const ks_sketches *s) { return s ? s->n_seqs : 0; }
extern "C" uint64_t ks_sketches_n_hashes(const ks_sketches *s) { return s ? s->n_hashes : 0; }
extern "C" uint64_t ks_sketches_n_windows(const ks_sketches *s) { return s ? s->n_windows : 0; }
extern "C" int ks_sketches_has_postings(const ks_sketches *s) {
    return ks_guard(nullptr, [&]() -> int { return (s && s->part_keys) ? (s->part_s ? 2 : 1) : 0;
    });
}
extern "C" void ks_sketches_params(const ks_sketches *s, ks_params *out) { if (s && out) *out = s->params; }
// (the arrays the ABI shows are a plain CSR: a batch whose slots have gaps is made dense on first sight — the object is
// logically const: same sketches — and NULL comes back if that fails, with the reason in ks_last_error)
static const ks_sketches *dense_view(const ks_sketches *s) {
    if (!s || !s->gapped) return s;
    ks_sketches *m = const_cast<ks_sketches *>(s);
    return ks_guard(m->ctx, [&]() -> int { return ks_sketches_make_dense(m->ctx, m); }) == KS_OK ? s : nullptr;
}
extern "C" const uint64_t *ks_sketches_device_offsets(const ks_sketches *s) { s = dense_view(s); return s ? s->d_offsets : nullptr; }
extern "C" const uint64_t *ks_sketches_device_hashes(const ks_sketches *s) { s = dense_view(s); return s ? s->d_hashes : nullptr; }
extern "C" const uint32_t *ks_sketches_device_abunds(const ks_sketches *s) { s = dense_view(s); return s ? s->d_abunds : nullptr; }

extern "C" int ks_sketches_copy_to_host(ks_ctx *ctx, const ks_sketches *s, uint64_t *offsets, uint64_t *hashes,
                                        uint32_t *abunds) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !s) return KS_ERR_INVALID_ARG;
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(s)));
    const size_t n = (size_t)s->n_hashes;
    return ks_columns_to_host(ctx, {{offsets, s->d_offsets, ((size_t)s->n_seqs + 1) * sizeof(u64)},
                                    {hashes, s->d_hashes, n * sizeof(u64)},
                                    {abunds, s->d_abunds, n * sizeof(u32)}});
    });
}

extern "C" int ks_sketches_from_host(ks_ctx *ctx, const uint64_t *offsets, const uint64_t *hashes, const uint32_t *abunds,
                                     uint32_t n_seqs, const ks_params *params, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!offsets || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_check_params(ctx, params));
    if (offsets[0] != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "offsets[0] must be 0");
    const u64 n = offsets[n_seqs];
    if (n && (!hashes || !abunds)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "hashes/abunds is NULL");
    // the index / join arithmetic assumes 0 < h <= max_hash(scaled) (ks_join_prefix < 2^pbits, sort prefix < 2^S): a
    // sketch made with a smaller `scaled` than the one passed here would wrap into foreign buckets and lose matches silently
    const u64 max_hash = ks_max_hash(params->scaled);
    for (u32 s = 0; s < n_seqs; s++) {
        if (offsets[s + 1] < offsets[s]) return ks_fail(ctx, KS_ERR_INVALID_ARG, "offsets must be ascending");
        for (u64 j = offsets[s]; j < offsets[s + 1]; j++) {
            if (hashes[j] == 0 || hashes[j] > max_hash)
                return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketch %u holds hash %llu outside (0, max_hash(scaled=%u)]", s,
                               (unsigned long long)hashes[j], params->scaled);
            if (j > offsets[s] && hashes[j] <= hashes[j - 1])
                return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketch %u is not strictly ascending", s);
        }
    }
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_sketches> S(ctx, out, ks_sketches_free);
    S->params = *params; S->n_seqs = n_seqs; S->n_hashes = S->n_slots = n;
    KS_TRY(ks_alloc(ctx, &S->d_offsets, (size_t)n_seqs + 1));
    KS_TRY(ks_alloc(ctx, &S->d_hashes, (size_t)n));
    KS_TRY(ks_alloc(ctx, &S->d_abunds, (size_t)n));
    KS_HIP(ctx, hipMemcpyAsync(S->d_offsets, offsets, ((size_t)n_seqs + 1) * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    if (n) {
        KS_HIP(ctx, hipMemcpyAsync(S->d_hashes, hashes, (size_t)n * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
        KS_HIP(ctx, hipMemcpyAsync(S->d_abunds, abunds, (size_t)n * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
    }
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return S.commit();
    });
}

extern "C" int ks_sketches_union(ks_ctx *ctx, const ks_sketches *in, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_union_impl(ctx, in, out);
    });
}

extern "C" void ks_sketches_free(ks_sketches *s) {
    if (!s) return;
    ks_pool_free(s->ctx, s->d_offsets);
    ks_pool_free(s->ctx, s->d_hashes);
    ks_pool_free(s->ctx, s->d_abunds);
    ks_pool_free(s->ctx, s->d_counts);
    ks_pool_free(s->ctx, s->part_keys);
    ks_pool_free(s->ctx, s->part_vals);
    if (s->ctl_block) ks_pool_free(s->ctx, s->ctl_block); // (part_len lies inside it)
    else ks_pool_free(s->ctx, s->part_len);
    delete s;
}

// ---------------------------------------------------------------------------------------------
// k-mer positions (ProteomeIndex::process_kmers, src/rust/index.rs:749-786): k_kmerpos_tiles in ks_kmerpos.hip.
// NOTE: the Rust path hashes the validated sequence as given (no upper-casing inside process_kmers);
// inputs that reach it are already upper-case, so the LUT's case folding is unobservable.
// ---------------------------------------------------------------------------------------------
int ks_kmerpos_device_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_params *p,
                           ks_kmerpos **out) {
    KS_TRY(ks_check_params(ctx, p));
    if (((uintptr_t)d_res & 15) != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "d_residues must be 16-byte aligned");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_kmerpos> K(ctx, out, ks_kmerpos_free);
    K->params = *p; K->n_seqs = n_seqs;
    // every residue position starts at most one window: n_res bounds the table
    const size_t cap = (n_res == 0 || n_seqs == 0) ? 1 : (size_t)n_res;
    KS_TRY(ks_alloc(ctx, &K->d_seq, cap));
    KS_TRY(ks_alloc(ctx, &K->d_start, cap));
    KS_TRY(ks_alloc(ctx, &K->d_hash, cap));
    if (n_res != 0 && n_seqs != 0)
        KS_TRY(ks_kmerpos_tiles_launch(ctx, d_res, d_offs, n_seqs, n_res, p, K->d_seq, K->d_start, K->d_hash, &K->n));
    return K.commit();
}

extern "C" int ks_kmer_positions(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs,
                                 const ks_params *params, ks_kmerpos **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "out is NULL");
    KS_TRY(ks_check_params(ctx, params));
    ks_upload U(ctx);
    KS_TRY(U.upload(residues, seq_offsets, n_seqs));
    return ks_kmerpos_device_impl(ctx, U.d_res, U.d_offs, n_seqs, U.n_res, params, out);
    });
}

extern "C" int ks_kmer_positions_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                                        uint64_t n_residues, const ks_params *params, ks_kmerpos **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "out is NULL");
    if (n_seqs && (!d_seq_offsets || (n_residues && !d_residues))) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL device buffer");
    return ks_kmerpos_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, params, out);
    });
}

extern "C" uint64_t ks_kmerpos_count(const ks_kmerpos *p) { return p ? p->n : 0; }
extern "C" void ks_kmerpos_params(const ks_kmerpos *p, ks_params *out) { if (p && out) *out = p->params; }

extern "C" int ks_kmerpos_copy_to_host(ks_ctx *ctx, const ks_kmerpos *p, uint32_t *seq, uint32_t *start, uint64_t *hash) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, p, seq, start, hash); });
}

extern "C" void ks_kmerpos_free(ks_kmerpos *p) { ks_obj_free(p); }

// ---------------------------------------------------------------------------------------------
// index + search
// ---------------------------------------------------------------------------------------------
extern "C" int ks_index_build(ks_ctx *ctx, const ks_sketches *targets, ks_index **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_index_build_impl(ctx, targets, out);
    });
}
extern "C" uint32_t ks_index_n_targets(const ks_index *ix) { return ix ? ix->n_targets : 0; }
extern "C" uint64_t ks_index_n_postings(const ks_index *ix) { return ix ? ix->n_postings : 0; }
extern "C" void ks_index_free(ks_index *ix) {
    if (!ix) return;
    ks_pool_free(ix->ctx, ix->d_keys);
    ks_pool_free(ix->ctx, ix->d_tids);
    ks_pool_free(ix->ctx, ix->d_abunds);
    ks_pool_free(ix->ctx, ix->d_fp);
    ks_pool_free(ix->ctx, ix->d_post);
    ks_pool_free(ix->ctx, ix->d_bmeta);
    ks_pool_free(ix->ctx, ix->d_presence);
    ks_pool_free(ix->ctx, ix->d_presence_big);
    ks_pool_free(ix->ctx, ix->d_dir);
    delete ix;
}

extern "C" int ks_search(ks_ctx *ctx, const ks_index *index, const ks_sketches *queries, ks_hits **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_search_impl(ctx, index, queries, out);
    });
}
extern "C" int ks_search_ex(ks_ctx *ctx, const ks_index *index, const ks_sketches *queries, const ks_search_opts *opts, ks_hits **out) {
    return ks_guard(ctx, [&]() -> int {
    KS_TRY(ks_search_opts_check(ctx, opts));
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_search_impl(ctx, index, queries, out, nullptr, opts);
    });
}
// One call for "sketch this query batch and search it": the sketch launches are queued WITHOUT the wait at their end, the
// search's partition and join follow on the same stream with sizes taken from upper bounds, and the search's first wait
// brings the sketch's control block back together with the join's counts — two waits per step instead of three.  A batch whose
// sketch has to be repeated (an economy that did not fit, dropped postings, a look-back that gave up: all rare) is simply
// done again with the two plain calls.
static int sketch_search_impl(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                              uint64_t n_residues, uint32_t max_seq_len, const ks_search_opts *opts, ks_sketches **sketches_out,
                              ks_hits **hits_out) {
    *hits_out = nullptr;
    if (sketches_out) *sketches_out = nullptr;
    const int fmt10 = (index->fp_layout && index->fp_shift == 32 - index->pbits) ? 1 : 0;
    ks_sketches *S = nullptr;
    ks_hits *H = nullptr;
    const u64 agg_before = ctx->agg_used, table_before = ctx->join_table;
    int st = ks_sketch_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, &index->params, index->pbits, fmt10,
                                   ks_dbg(ctx, KS_DBG_NO_DEFER) ? 0 : 1, &S);
    if (st != KS_OK) return st;
    const bool deferred = S->pending != 0;
    int redo = 0;
    st = ks_search_impl(ctx, index, S, &H, &redo, opts);
    if (S->pending) { // (the search failed before its first wait)
        const ks_fetch_seg f = ks_sketch_pending_seg(S);
        int r2 = 0;
        int st2 = ks_stream_wait_fetch(ctx, &f, 1);
        if (st2 == KS_OK) st2 = ks_sketch_finish_pending(S, &r2);
        if (st == KS_OK) { st = st2; redo = r2; }
    }
    if (st == KS_OK && redo) { // the plain way: the sketch call repeats what it has to, the search starts from what it gets
        ks_hits_free(H); H = nullptr;
        ks_sketches_free(S); S = nullptr;
        ctx->fused_redos++;
        st = ks_sketch_device_impl(ctx, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, &index->params, index->pbits, fmt10, 0, &S);
        if (st == KS_OK) st = ks_search_impl(ctx, index, S, &H, nullptr, opts);
    }
    if (st != KS_OK) { ks_hits_free(H); ks_sketches_free(S); return st; }
    if (deferred) ctx->fused_deferred++;
    if (ctx->agg_used > agg_before) ctx->fused_aggregated++;
    if (ctx->join_table > table_before) ctx->fused_table_joined++;
    *hits_out = H;
    if (sketches_out) *sketches_out = S; else ks_sketches_free(S);
    return KS_OK;
}

extern "C" int ks_sketch_search_device_ex(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues,
                                          const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                                          uint32_t max_seq_len, const ks_search_opts *opts, ks_sketches **sketches_out,
                                          ks_hits **hits_out) {
    return ks_guard(ctx, [&]() -> int {
    KS_TRY(ks_search_opts_check(ctx, opts));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!index || !hits_out || (!d_seq_offsets) || (!d_residues && n_residues)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    return sketch_search_impl(ctx, index, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, opts, sketches_out, hits_out);
    });
}
extern "C" int ks_sketch_search_device(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues,
                                       const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                                       uint32_t max_seq_len, ks_sketches **sketches_out, ks_hits **hits_out) {
    return ks_guard(ctx, [&]() -> int {
    return ks_sketch_search_device_ex(ctx, index, d_residues, d_seq_offsets, n_seqs, n_residues, max_seq_len, nullptr, sketches_out,
                                      hits_out);
    });
}

// ... and from host arrays (the batch is uploaded, its longest record is known from the offsets: the read-back is always folded)
extern "C" int ks_sketch_search_ex(ks_ctx *ctx, const ks_index *index, const uint8_t *residues, const uint64_t *seq_offsets,
                                   uint32_t n_seqs, const ks_search_opts *opts, ks_sketches **sketches_out, ks_hits **hits_out) {
    return ks_guard(ctx, [&]() -> int {
    KS_TRY(ks_search_opts_check(ctx, opts));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!index || !hits_out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    ks_upload U(ctx);
    KS_TRY(U.upload(residues, seq_offsets, n_seqs));
    return sketch_search_impl(ctx, index, U.d_res, U.d_offs, n_seqs, U.n_res, U.max_len, opts, sketches_out, hits_out);
    });
}
extern "C" int ks_sketch_search(ks_ctx *ctx, const ks_index *index, const uint8_t *residues, const uint64_t *seq_offsets,
                                uint32_t n_seqs, ks_sketches **sketches_out, ks_hits **hits_out) {
    return ks_guard(ctx, [&]() -> int {
    return ks_sketch_search_ex(ctx, index, residues, seq_offsets, n_seqs, nullptr, sketches_out, hits_out);
    });
}
// ---- packed transport records (multi-GPU hit exchange) ---------------------------------------------------------------
// A COO row is 20 bytes (qid u32, tid u32, intersect u32, n_weighted u64); an all-vs-all of 200k proteins gathers 31 M of
// them, and over xGMI the exchange — not the kernels — is the step.  For transport a row travels as ONE 64-bit word
//     qid << (tbits + 2v) | tid << 2v | intersect << v | n_weighted,      v = (64 - qbits - tbits) / 2 value bits,
// ids in global numbering.  A row whose intersect or n_weighted does not fit v bits carries all-ones in both value fields and
// its true values go to a short escape list (row index, intersect, n_weighted), gathered beside the words.
__global__ __launch_bounds__(256) void k_hits_pack64(const u32 *qid, const u32 *tid, const u32 *isect, const u64 *nw, u64 n, u32 qid_base,
                                                     u32 tid_base, int qbits, int tbits, int vbits, u64 *packed, u32 *esc_row, u32 *esc_isect,
                                                     u64 *esc_nw, u32 *n_esc, u32 esc_cap) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 vmax = (1ULL << vbits) - 1ULL;
    u64 a = isect[i], b = nw[i];
    if (a >= vmax || b >= vmax) { // (all-ones itself is the escape marker, so a value equal to it escapes too)
        const u32 e = atomicAdd(n_esc, 1u);
        if (e < esc_cap) { esc_row[e] = (u32)i; esc_isect[e] = (u32)a; esc_nw[e] = b; }
        a = vmax; b = vmax;
    }
    const u64 q = (u64)qid[i] + qid_base, t = (u64)tid[i] + tid_base;
    // an id that does not fit its field (id_counts smaller than the real global range) would spill into its neighbour:
    // the escape count is pushed beyond any capacity instead, so every rank takes the unpacked exchange
    // (tested against qbits itself: 64 - tbits - 2v is one bit wider when 64 - qbits - tbits is odd, and the receiving side
    // masks with qbits)
    if ((q >> qbits) != 0 || (t >> tbits) != 0) atomicOr(n_esc, 0x80000000u);
    packed[i] = (((q << tbits) | t) << (2 * vbits)) | (a << vbits) | b;
}

extern "C" int ks_hits_pack64_to_device(ks_ctx *ctx, const ks_hits *h, uint32_t qid_base, uint32_t tid_base, int qbits, int tbits,
                                        uint64_t *d_packed, uint32_t *d_esc_row, uint32_t *d_esc_intersect, uint64_t *d_esc_n_weighted,
                                        uint32_t *d_n_esc, uint32_t esc_cap) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !h) return KS_ERR_INVALID_ARG;
    if (qbits < 1 || tbits < 1 || qbits + tbits > 48) return ks_fail(ctx, KS_ERR_INVALID_ARG, "pack64: %d + %d id bits leave fewer than 8 value bits", qbits, tbits);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    const u64 n = h->n_hits;
    if (!d_n_esc) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    // the escape counter is cleared HERE, on the context's stream: a caller that zeroes its buffer on another stream
    // (torch's) is not ordered before this launch
    KS_HIP(ctx, hipMemsetAsync(d_n_esc, 0, sizeof(u32), ctx->stream));
    if (n == 0) return KS_OK;
    if (n >= 0xffffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "pack64: %llu rows (escape rows are 32-bit indices)", (unsigned long long)n);
    if (!d_packed || (esc_cap && (!d_esc_row || !d_esc_intersect || !d_esc_n_weighted))) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_LAUNCH(ctx, "hits_pack", k_hits_pack64, (u32)((n + 255) / 256), 256, (const u32 *)h->d_qid, (const u32 *)h->d_tid, (const u32 *)h->d_isect,
              (const u64 *)h->d_nw, n, qid_base, tid_base, qbits, tbits, (64 - qbits - tbits) / 2, d_packed, d_esc_row, d_esc_intersect, d_esc_n_weighted,
              d_n_esc, esc_cap);
    return KS_OK;
    });
}

// the inverse, for the receiving side of the exchange: words -> columns (escaped rows keep the all-ones markers: the caller
// patches them from the escape lists)
__global__ __launch_bounds__(256) void k_hits_unpack64(const u64 *packed, u64 n, int qbits, int tbits, int vbits, u32 *qid, u32 *tid,
                                                       u32 *isect, u64 *nw) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 w = packed[i], vmax = (1ULL << vbits) - 1ULL;
    qid[i] = (u32)((w >> (tbits + 2 * vbits)) & ((1ULL << qbits) - 1ULL));
    tid[i] = (u32)((w >> (2 * vbits)) & ((1ULL << tbits) - 1ULL));
    isect[i] = (u32)((w >> vbits) & vmax);
    nw[i] = w & vmax;
}

extern "C" int ks_hits_unpack64_device(ks_ctx *ctx, const uint64_t *d_packed, uint64_t n, int qbits, int tbits, uint32_t *d_qid,
                                       uint32_t *d_tid, uint32_t *d_intersect, uint64_t *d_n_weighted) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (qbits < 1 || tbits < 1 || qbits + tbits > 48) return ks_fail(ctx, KS_ERR_INVALID_ARG, "unpack64: %d + %d id bits leave fewer than 8 value bits", qbits, tbits);
    if (n == 0) return KS_OK;
    if (!d_packed || !d_qid || !d_tid || !d_intersect || !d_n_weighted) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (n > 0xffffffffULL * 256ULL) return ks_fail(ctx, KS_ERR_INVALID_ARG, "unpack64: too many rows");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_LAUNCH(ctx, "hits_unpack", k_hits_unpack64, (u32)((n + 255) / 256), 256, (const u64 *)d_packed, n, qbits, tbits, (64 - qbits - tbits) / 2,
              d_qid, d_tid, d_intersect, (u64 *)d_n_weighted);
    return KS_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// Index-sharded exchange, global (qid, tid) order: the gathered list is W rank blocks, each ordered by (qid, tid) with the
// ranks' target ranges ascending — so the merged order is "by qid, then by rank", and a row's place follows from counting,
// not from sorting 10^7 keys: per (query, rank) the block's rows of that query are one run (found by binary search),
// an exclusive scan over (qid-major, rank-minor) run lengths gives every run its start, one pass moves the rows.
// Replaces a stable device sort on qid (torch.sort: ~8 passes over keys + 4 gathers).  Reference semantics: branchwater
// manysearch rows per query (src/python/kmerseek/search.py:125-141).
// ---------------------------------------------------------------------------------------------
struct hm_blocks { u64 base[65]; u32 n; }; // rank r's rows are [base[r], base[r + 1])

// first[r * (nq + 1) + q] = first row of block r whose qid is >= q (local to the block)
__global__ __launch_bounds__(256) void k_hm_starts(const u32 *qid, hm_blocks B, u32 nq, u32 *first) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 per = (u64)nq + 1;
    if (i >= per * B.n) return;
    const u32 r = (u32)(i / per), q = (u32)(i % per);
    u64 lo = B.base[r], hi = B.base[r + 1];
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (qid[mid] < q) lo = mid + 1; else hi = mid;
    }
    first[i] = (u32)(lo - B.base[r]);
}
// run[q * W + r] = rows of query q in block r
__global__ __launch_bounds__(256) void k_hm_runs(const u32 *first, u32 W, u32 nq, u32 *run) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (u64)nq * W) return;
    const u32 q = (u32)(i / W), r = (u32)(i % W);
    const u64 at = (u64)r * ((u64)nq + 1) + q;
    run[i] = first[at + 1] - first[at];
}
__global__ __launch_bounds__(256) void k_hm_move(const u32 *qid, const u32 *tid, const u32 *isect, const u64 *nw, hm_blocks B, u32 nq,
                                                 const u32 *first, const u32 *start, u32 *o_qid, u32 *o_tid, u32 *o_isect, u64 *o_nw,
                                                 u32 *n_dropped) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.base[B.n]) return;
    u32 r = 0;
    while (r + 1 < B.n && i >= B.base[r + 1]) r++; // (W <= 64 blocks)
    const u32 q = qid[i];
    if (q >= nq) { atomicAdd(n_dropped, 1u); return; } // (an id beyond the declared range: not written out of bounds, but counted — the call fails)
    const u64 pos = (u64)start[(u64)q * B.n + r] + ((i - B.base[r]) - first[(u64)r * ((u64)nq + 1) + q]);
    o_qid[pos] = q; o_tid[pos] = tid[i]; o_isect[pos] = isect[i]; o_nw[pos] = nw[i];
}

extern "C" int ks_hits_merge_by_qid_device(ks_ctx *ctx, const uint32_t *d_qid, const uint32_t *d_tid, const uint32_t *d_intersect,
                                           const uint64_t *d_n_weighted, const uint64_t *block_rows, uint32_t n_blocks, uint32_t n_queries,
                                           uint32_t *d_out_qid, uint32_t *d_out_tid, uint32_t *d_out_intersect, uint64_t *d_out_n_weighted) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!block_rows || n_blocks == 0 || n_blocks > 64) return ks_fail(ctx, KS_ERR_INVALID_ARG, "merge: 1 .. 64 rank blocks");
    hm_blocks B;
    B.n = n_blocks; B.base[0] = 0;
    for (u32 r = 0; r < n_blocks; r++) B.base[r + 1] = B.base[r] + block_rows[r];
    const u64 n = B.base[n_blocks];
    if (n == 0) return KS_OK;
    if (n >= 0xffffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "merge: %llu rows", (unsigned long long)n);
    if (!d_qid || !d_tid || !d_intersect || !d_n_weighted || !d_out_qid || !d_out_tid || !d_out_intersect || !d_out_n_weighted)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    // (the scratch blocks go back to the pool in stream order: the next allocation on this context's stream comes behind the kernels)
    ks_scratch sc(ctx);
    u32 *first = nullptr, *run = nullptr;
    const u64 n_first = ((u64)n_queries + 1) * n_blocks, n_run = (u64)n_queries * n_blocks;
    KS_TRY(sc.alloc(&first, (size_t)n_first));
    KS_TRY(sc.alloc(&run, (size_t)n_run + 2)); // (+ the scan's total, + the count of rows with an id out of range)
    u32 *const n_dropped = run + n_run + 1;
    KS_HIP(ctx, hipMemsetAsync(n_dropped, 0, sizeof(u32), ctx->stream));
    ks_timer_begin(ctx, "hits_merge"); // (one timing row for the two launches)
    hipLaunchKernelGGL(k_hm_starts, dim3((u32)((n_first + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)d_qid, B, n_queries, first);
    if (n_run) hipLaunchKernelGGL(k_hm_runs, dim3((u32)((n_run + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)first, n_blocks, n_queries, run);
    ks_timer_end(ctx);
    KS_HIP(ctx, hipGetLastError());
    if (n_run) KS_TRY(ks_scan_u32_inplace(ctx, run, n_run, nullptr));
    KS_LAUNCH(ctx, "hits_merge", k_hm_move, (u32)((n + 255) / 256), 256, (const u32 *)d_qid, (const u32 *)d_tid, (const u32 *)d_intersect,
              (const u64 *)d_n_weighted, B, n_queries, (const u32 *)first, (const u32 *)run, d_out_qid, d_out_tid, d_out_intersect,
              (u64 *)d_out_n_weighted, n_dropped);
    // a row whose query id lies beyond n_queries has no place in the merged order: the outputs would hold a gap
    const u32 *dropped = (const u32 *)(ctx->h_pin + KS_PIN_READ);
    const ks_fetch_seg f = ks_fetch_words(n_dropped, ctx->h_pin + KS_PIN_READ, 1);
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    if (*dropped != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "merge: %u rows carry a query id >= n_queries = %u", *dropped, n_queries);
    return KS_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// region scores (ks_rscore.hip): the regions of a hit list scored under a substitution matrix, extended without gaps
// ---------------------------------------------------------------------------------------------
// what the passes over a ks_regions check alike before any device work: the objects, their context, the row counts, the batches
static int ks_region_pass_check(ks_ctx *ctx, const char *pass, const ks_regions *regions, const ks_hits *hits, const void *out,
                                const ks_res_batch &Q, const ks_res_batch &T) {
    if (!regions || !hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, pass, regions, hits));
    if (regions->n_rows != hits->n_hits)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: the regions cover %llu hit rows, the hit list holds %llu: regions of another list",
                       pass, (unsigned long long)regions->n_rows, (unsigned long long)hits->n_hits);
    if (regions->n_regions && (!Q.res || !Q.offs || !T.res || !T.offs)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL device buffer");
    return KS_OK;
}
// The three passes under a matrix and against a profile are one body each; by_profile: `profile` scores the pairs (checked
// behind the pass's own arguments: not NULL, of ctx, of the query batch), otherwise it is NULL and not looked at.
static int ks_regions_score_any(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const ks_res_batch &Q, const ks_res_batch &T,
                                bool by_profile, const ks_profile *profile, const ks_rscore_opts *opts, ks_rscores **out) {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "region score", opts->flags, KS_RSCORE_EXTEND, opts->reserved ? 1u : 0u));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    KS_TRY(ks_region_pass_check(ctx, "region scores", regions, hits, out, Q, T));
    if (by_profile) KS_TRY(rk_profile_check(ctx, "region scores", profile, Q));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_rscores> S(ctx, out, ks_rscores_free);
    KS_TRY(ks_regions_score_impl(ctx, regions, hits, Q, T, opts, by_profile ? profile : nullptr, S));
    return S.commit();
}
extern "C" int ks_regions_score(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_rscore_opts *opts, ks_rscores **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_score_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, false, nullptr, opts, out);
    });
}
extern "C" int ks_regions_score_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                        const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                        const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_profile *profile,
                                        const ks_rscore_opts *opts, ks_rscores **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_score_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, true, profile, opts, out);
    });
}
extern "C" uint64_t ks_rscores_n_rows(const ks_rscores *s) { return s ? s->n_rows : 0; }
extern "C" uint64_t ks_rscores_n_regions(const ks_rscores *s) { return s ? s->n_regions : 0; }
extern "C" const uint64_t *ks_rscores_device_row_offsets(const ks_rscores *s) { return s ? s->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_rscores_device_q_start(const ks_rscores *s) { return s ? s->d_qstart : nullptr; }
extern "C" const uint32_t *ks_rscores_device_t_start(const ks_rscores *s) { return s ? s->d_tstart : nullptr; }
extern "C" const uint32_t *ks_rscores_device_length(const ks_rscores *s) { return s ? s->d_length : nullptr; }
extern "C" const int64_t *ks_rscores_device_score(const ks_rscores *s) { return s ? s->d_score : nullptr; }
extern "C" const uint32_t *ks_rscores_device_identities(const ks_rscores *s) { return s ? s->d_identities : nullptr; }
extern "C" const uint32_t *ks_rscores_device_positives(const ks_rscores *s) { return s ? s->d_positives : nullptr; }
extern "C" const uint32_t *ks_rscores_device_core_identities(const ks_rscores *s) { return s ? s->d_core_ident : nullptr; }

extern "C" int ks_rscores_copy_to_host(ks_ctx *ctx, const ks_rscores *s, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                                       uint32_t *length, int64_t *score, uint32_t *identities, uint32_t *positives,
                                       uint32_t *core_identities) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, s, row_offsets, q_start, t_start, length, score, identities, positives,
                                                              core_identities); });
}

extern "C" void ks_rscores_free(ks_rscores *s) { ks_obj_free(s); }

// ---------------------------------------------------------------------------------------------
// region alignments (ks_ralign.hip): the regions of a hit list extended with gaps from the middle of their seeds
// ---------------------------------------------------------------------------------------------
static int ks_regions_align_any(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const ks_res_batch &Q, const ks_res_batch &T,
                                bool by_profile, const ks_profile *profile, const ks_ralign_opts *opts, ks_raligns **out) {
    const ks_ralign_opts dflt = {nullptr, 16u, 11u, 1u, 30u, 0u};
    const ks_ralign_opts o = opts ? *opts : dflt;
    KS_TRY(ks_opts_words_check(ctx, "region alignment", o.flags, 0u, 0u));
    if (o.band > KS_RALIGN_MAX_BAND || o.gap_open > KS_RALIGN_MAX_GAP_COST || o.gap_extend > KS_RALIGN_MAX_GAP_COST || o.x_drop > KS_RALIGN_MAX_X_DROP) {
        if (!ctx) return KS_ERR_INVALID_ARG;
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region alignment options: band %u (at most %u), gap_open %u, gap_extend %u (at most %u), x_drop %u (at most %u)",
                       o.band, KS_RALIGN_MAX_BAND, o.gap_open, o.gap_extend, KS_RALIGN_MAX_GAP_COST, o.x_drop, KS_RALIGN_MAX_X_DROP);
    }
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    KS_TRY(ks_region_pass_check(ctx, "region alignments", regions, hits, out, Q, T));
    if (by_profile) KS_TRY(rk_profile_check(ctx, "region alignments", profile, Q));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_raligns> S(ctx, out, ks_raligns_free);
    KS_TRY(ks_regions_align_impl(ctx, regions, hits, Q, T, &o, by_profile ? profile : nullptr, S));
    return S.commit();
}
extern "C" int ks_regions_align(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_ralign_opts *opts, ks_raligns **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_align_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, false, nullptr, opts, out);
    });
}
extern "C" int ks_regions_align_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                        const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                        const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_profile *profile,
                                        const ks_ralign_opts *opts, ks_raligns **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_align_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, true, profile, opts, out);
    });
}
extern "C" int ks_raligns_by_profile(const ks_raligns *s) { return s && s->by_profile ? 1 : 0; }
extern "C" uint64_t ks_raligns_n_rows(const ks_raligns *s) { return s ? s->n_rows : 0; }
extern "C" uint64_t ks_raligns_n_regions(const ks_raligns *s) { return s ? s->n_regions : 0; }
extern "C" const uint64_t *ks_raligns_device_row_offsets(const ks_raligns *s) { return s ? s->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_raligns_device_q_start(const ks_raligns *s) { return s ? s->d_qstart : nullptr; }
extern "C" const uint32_t *ks_raligns_device_q_length(const ks_raligns *s) { return s ? s->d_qlength : nullptr; }
extern "C" const uint32_t *ks_raligns_device_t_start(const ks_raligns *s) { return s ? s->d_tstart : nullptr; }
extern "C" const uint32_t *ks_raligns_device_t_length(const ks_raligns *s) { return s ? s->d_tlength : nullptr; }
extern "C" const int64_t *ks_raligns_device_score(const ks_raligns *s) { return s ? s->d_score : nullptr; }
extern "C" const uint32_t *ks_raligns_device_identities(const ks_raligns *s) { return s ? s->d_identities : nullptr; }
extern "C" const uint32_t *ks_raligns_device_positives(const ks_raligns *s) { return s ? s->d_positives : nullptr; }
extern "C" const uint32_t *ks_raligns_device_gap_opens(const ks_raligns *s) { return s ? s->d_gap_opens : nullptr; }
extern "C" const uint32_t *ks_raligns_device_gaps(const ks_raligns *s) { return s ? s->d_gaps : nullptr; }
extern "C" const uint32_t *ks_raligns_device_aln_length(const ks_raligns *s) { return s ? s->d_aln_length : nullptr; }

extern "C" int ks_raligns_copy_to_host(ks_ctx *ctx, const ks_raligns *s, uint64_t *row_offsets, uint32_t *q_start, uint32_t *q_length,
                                       uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities, uint32_t *positives,
                                       uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, s, row_offsets, q_start, q_length, t_start, t_length, score, identities,
                                                              positives, gap_opens, gaps, aln_length); });
}

extern "C" void ks_raligns_free(ks_raligns *s) { ks_obj_free(s); }

// ---------------------------------------------------------------------------------------------
// region traceback (ks_rtrace.hip): the path of every alignment of a ks_raligns as a CIGAR
// ---------------------------------------------------------------------------------------------
static int ks_regions_traceback_any(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const ks_res_batch &Q, const ks_res_batch &T,
                                    const ks_raligns *alignments, bool by_profile, const ks_profile *profile, const ks_rtrace_opts *opts,
                                    ks_cigars **out) {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "region traceback", opts->flags, KS_RTRACE_EQX, opts->reserved));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    KS_TRY(ks_region_pass_check(ctx, "region traceback", regions, hits, out, Q, T));
    if (!alignments) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "region traceback", alignments));
    if (!by_profile) KS_TRY(ks_refuse_by_profile(ctx, "region traceback", alignments));
    else {
        if (!alignments->by_profile)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region traceback against a profile: the alignments were made under a matrix (ks_regions_align): "
                                                    "their path is ks_regions_traceback's");
        KS_TRY(rk_profile_check(ctx, "region traceback", profile, Q));
    }
    if (alignments->n_rows != regions->n_rows || alignments->n_regions != regions->n_regions)
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "region traceback: the alignments are of %llu regions in %llu hit rows, the regions are %llu in %llu: "
                       "alignments of other regions", (unsigned long long)alignments->n_regions, (unsigned long long)alignments->n_rows,
                       (unsigned long long)regions->n_regions, (unsigned long long)regions->n_rows);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_cigars> C(ctx, out, ks_cigars_free);
    KS_TRY(ks_regions_traceback_impl(ctx, regions, hits, Q, T, alignments, by_profile ? profile : nullptr, opts ? opts->flags : 0u,
                                     opts ? opts->max_scratch_bytes : 0, C));
    return C.commit();
}
extern "C" int ks_regions_traceback(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                    const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                    const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_raligns *alignments,
                                    const ks_rtrace_opts *opts, ks_cigars **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_traceback_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, alignments, false,
                                    nullptr, opts, out);
    });
}
extern "C" int ks_regions_traceback_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res,
                                            const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                            const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_raligns *alignments,
                                            const ks_profile *profile, const ks_rtrace_opts *opts, ks_cigars **out) {
    return ks_guard(ctx, [&]() -> int {
        return ks_regions_traceback_any(ctx, regions, hits, {d_q_res, d_q_offs, n_q, n_q_res}, {d_t_res, d_t_offs, n_t, n_t_res}, alignments, true,
                                    profile, opts, out);
    });
}
extern "C" uint64_t ks_cigars_n_rows(const ks_cigars *c) { return c ? c->n_rows : 0; }
extern "C" uint64_t ks_cigars_n_regions(const ks_cigars *c) { return c ? c->n_regions : 0; }
extern "C" uint64_t ks_cigars_n_ops(const ks_cigars *c) { return c ? c->n_ops : 0; }
extern "C" uint64_t ks_cigars_scratch_bytes(const ks_cigars *c) { return c ? c->dir_bytes : 0; }
extern "C" uint32_t ks_cigars_n_slices(const ks_cigars *c) { return c ? c->n_slices : 0; }
extern "C" const uint64_t *ks_cigars_device_op_offsets(const ks_cigars *c) { return c ? c->d_op_offsets : nullptr; }
extern "C" const uint32_t *ks_cigars_device_ops(const ks_cigars *c) { return c ? c->d_ops : nullptr; }

extern "C" int ks_cigars_copy_to_host(ks_ctx *ctx, const ks_cigars *c, uint64_t *op_offsets, uint32_t *ops) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, op_offsets, ops); });
}

extern "C" void ks_cigars_free(ks_cigars *c) { ks_obj_free(c); }

// ---------------------------------------------------------------------------------------------
// region cull (ks_rcull.hip): per hit row the regions no better region of the row covers; the objects of the kept regions
// ---------------------------------------------------------------------------------------------
// the options, defaults filled in; refused before any device work, also with ctx == NULL
static int ks_rcull_opts_check(ks_ctx *ctx, const ks_rcull_opts *opts, ks_rcull_opts *o) {
    const ks_rcull_opts dflt = {100u, 0u, 0, 0u, 0u};
    *o = opts ? *opts : dflt;
    KS_TRY(ks_opts_words_check(ctx, "region cull", o->flags, KS_RCULL_MIN_SCORE, o->reserved));
    if (o->overlap_pct <= 100u) return KS_OK;
    return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "region cull options: overlap_pct %u (1 .. 100, 0 = 100)", o->overlap_pct) : KS_ERR_INVALID_ARG;
}
static int ks_rcull_run(ks_ctx *ctx, const ks_rcull_cols &cols, u64 n_rows, u64 n_regions, const ks_rcull_opts &o, ks_rcull **out) {
    if (!out || !cols.row_offs || (n_regions && (!cols.qs || !cols.ql || !cols.ts || !cols.tl || !cols.score)))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (n_rows == 0 && n_regions != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region cull: %llu regions in no hit row: row_offsets is not a CSR from 0 to n", (unsigned long long)n_regions);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_rcull> K(ctx, out, ks_rcull_free);
    KS_TRY(ks_regions_cull_impl(ctx, cols, n_rows, n_regions, &o, K));
    return K.commit();
}
extern "C" int ks_regions_cull_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length,
                                      const uint32_t *d_t_start, const uint32_t *d_t_length, const int64_t *d_score, uint64_t n_rows,
                                      uint64_t n_regions, const ks_rcull_opts *opts, ks_rcull **out) {
    return ks_guard(ctx, [&]() -> int {
    ks_rcull_opts o;
    KS_TRY(ks_rcull_opts_check(ctx, opts, &o));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    return ks_rcull_run(ctx, {d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length ? d_t_length : d_q_length, d_score}, n_rows, n_regions, o, out);
    });
}
// the cull of an object's own columns (ks_rscores, ks_raligns)
template <typename T> static int ks_rcull_of(ks_ctx *ctx, const T *s, const ks_rcull_opts *opts, ks_rcull **out) {
    ks_rcull_opts o;
    KS_TRY(ks_rcull_opts_check(ctx, opts, &o));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!s) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "region cull", s));
    return ks_rcull_run(ctx, s->cols(), s->n_rows, s->n_regions, o, out);
}
extern "C" int ks_raligns_cull(ks_ctx *ctx, const ks_raligns *s, const ks_rcull_opts *opts, ks_rcull **out) {
    return ks_guard(ctx, [&]() -> int { return ks_rcull_of(ctx, s, opts, out); });
}
extern "C" int ks_rscores_cull(ks_ctx *ctx, const ks_rscores *s, const ks_rcull_opts *opts, ks_rcull **out) {
    return ks_guard(ctx, [&]() -> int { return ks_rcull_of(ctx, s, opts, out); });
}
extern "C" uint64_t ks_rcull_n_rows(const ks_rcull *c) { return c ? c->n_rows : 0; }
extern "C" uint64_t ks_rcull_n_regions(const ks_rcull *c) { return c ? c->n_regions : 0; }
extern "C" uint64_t ks_rcull_n_kept(const ks_rcull *c) { return c ? c->n_kept : 0; }
extern "C" const uint64_t *ks_rcull_device_row_offsets(const ks_rcull *c) { return c ? c->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_rcull_device_src_region(const ks_rcull *c) { return c ? c->d_src_region : nullptr; }
extern "C" const uint32_t *ks_rcull_device_rank(const ks_rcull *c) { return c ? c->d_rank : nullptr; }
extern "C" const uint32_t *ks_rcull_device_n_merged(const ks_rcull *c) { return c ? c->d_n_merged : nullptr; }
extern "C" const uint32_t *ks_rcull_device_keeper(const ks_rcull *c) { return c ? c->d_keeper : nullptr; }
extern "C" const double *ks_rcull_device_row_best_score(const ks_rcull *c) { return c ? c->d_row_best : nullptr; }

extern "C" int ks_rcull_copy_to_host(ks_ctx *ctx, const ks_rcull *c, uint64_t *row_offsets, uint32_t *src_region, uint32_t *rank,
                                     uint32_t *n_merged, uint32_t *keeper, double *row_best_score) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, row_offsets, src_region, rank, n_merged, keeper, row_best_score); });
}

extern "C" void ks_rcull_free(ks_rcull *c) { ks_obj_free(c); }

// what the three takes check alike, and their row_offsets: a copy of the cull's
template <typename T> static int ks_take_check(ks_ctx *ctx, const T *obj, const ks_rcull *cull, const void *out) {
    if (!obj || !cull || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "region take", obj, cull));
    if (obj->n_rows != cull->n_rows || obj->n_regions != cull->n_regions)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region take: the object holds %llu regions in %llu hit rows, the cull was made of %llu in %llu: a cull of other regions",
                       (unsigned long long)obj->n_regions, (unsigned long long)obj->n_rows, (unsigned long long)cull->n_regions, (unsigned long long)cull->n_rows);
    return KS_OK;
}
template <typename T> static int ks_take_offsets(ks_ctx *ctx, const ks_rcull *cull, T *o) {
    o->n_rows = cull->n_rows; o->n_regions = cull->n_kept;
    KS_TRY(ks_alloc(ctx, &o->d_row_offsets, (size_t)cull->n_rows + 1));
    KS_HIP(ctx, hipMemcpyAsync(o->d_row_offsets, cull->d_row_offsets, ((size_t)cull->n_rows + 1) * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    return KS_OK;
}
// the columns of o listed with n_regions: the 32-bit ones to c32[0 .. *n32), the 64-bit score to *c64
template <typename T, typename P32, typename P64> static constexpr void ks_take_list(T &o, P32 *c32, u32 *n32, P64 *c64) {
    T::each(o, [&](auto *p, const u64 &n, bool = true) {
        if (&n != &o.n_regions) return;
        if constexpr (std::is_convertible_v<decltype(p), P32>) c32[(*n32)++] = p;
        else if constexpr (std::is_convertible_v<decltype(p), P64>) *c64 = p;
    });
}
template <typename T> static constexpr u32 ks_take_n32() {
    T z{};
    const u32 *c32[64] = {};
    const i64 *c64 = nullptr;
    u32 k = 0;
    ks_take_list(z, c32, &k, &c64);
    return k;
}
// The regions a cull kept, of any of the three objects: every column listed with n_regions moves through the cull's src_region into
// a block of n_kept entries (ks_rcull_take_launch); take_from copies what else the type holds.
template <typename T> static int ks_obj_take(ks_ctx *ctx, const T *src, const ks_rcull *cull, T **out, void (*free_fn)(T *)) {
    static_assert(ks_take_n32<T>() <= KS_TAKE_COLS, "a take moves more 32-bit columns than ks_take_cols holds");
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    KS_TRY(ks_take_check(ctx, src, cull, out));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<T> R(ctx, out, free_fn);
    KS_TRY(ks_take_offsets(ctx, cull, R.obj));
    R->take_from(*src);
    KS_TRY(ks_obj_alloc(ctx, R.obj, R->n_regions));
    ks_take_cols C{};
    u32 n_out = 0;
    ks_take_list(*src, C.in, &C.n32, &C.in64);
    ks_take_list(*R.obj, C.out, &n_out, &C.out64);
    KS_TRY(ks_rcull_take_launch(ctx, cull, C));
    KS_TRY(ks_stream_wait(ctx));
    return R.commit();
}
extern "C" int ks_regions_take(ks_ctx *ctx, const ks_regions *regions, const ks_rcull *cull, ks_regions **out) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_take(ctx, regions, cull, out, ks_regions_free); });
}
extern "C" int ks_rscores_take(ks_ctx *ctx, const ks_rscores *scores, const ks_rcull *cull, ks_rscores **out) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_take(ctx, scores, cull, out, ks_rscores_free); });
}
extern "C" int ks_raligns_take(ks_ctx *ctx, const ks_raligns *s, const ks_rcull *cull, ks_raligns **out) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_take(ctx, s, cull, out, ks_raligns_free); });
}

// ---------------------------------------------------------------------------------------------
// region chain (ks_rchain.hip): per hit row the best colinear chain of its regions, and how much of the sequences it covers
// ---------------------------------------------------------------------------------------------
// the options, defaults filled in; refused before any device work, also with ctx == NULL
static int ks_rchain_opts_check(ks_ctx *ctx, const ks_rchain_opts *opts, ks_rchain_opts *o) {
    const ks_rchain_opts dflt = {0u, 0u, 0u, 0u, 0u, 0u, {0u, 0u}};
    *o = opts ? *opts : dflt;
    KS_TRY(ks_opts_words_check(ctx, "region chain", o->flags, 0, o->reserved[0] | o->reserved[1]));
    if (o->link_cost <= (1u << 30) && o->skew_cost <= (1u << 16) && o->overlap_cost <= (1u << 16)) return KS_OK;
    return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain options: link_cost %u (<= 2^30), skew_cost %u, overlap_cost %u (<= 2^16)", o->link_cost,
                         o->skew_cost, o->overlap_cost)
               : KS_ERR_INVALID_ARG;
}
static int ks_rchain_run(ks_ctx *ctx, const ks_rchain_cols &cols, u64 n_rows, u64 n_regions, const ks_rchain_opts &o, ks_rchain **out) {
    if (!out || !cols.row_offs || (n_regions && (!cols.qs || !cols.ql || !cols.ts || !cols.tl || !cols.score)))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if (n_rows == 0 && n_regions != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain: %llu regions in no hit row: row_offsets is not a CSR from 0 to n", (unsigned long long)n_regions);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_rchain> K(ctx, out, ks_rchain_free);
    KS_TRY(ks_regions_chain_impl(ctx, cols, n_rows, n_regions, &o, K));
    return K.commit();
}
extern "C" int ks_regions_chain_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length,
                                       const uint32_t *d_t_start, const uint32_t *d_t_length, const int64_t *d_score, const uint32_t *d_identities,
                                       const uint32_t *d_aln_length, uint64_t n_rows, uint64_t n_regions, const ks_rchain_opts *opts, ks_rchain **out) {
    return ks_guard(ctx, [&]() -> int {
    ks_rchain_opts o;
    KS_TRY(ks_rchain_opts_check(ctx, opts, &o));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    return ks_rchain_run(ctx, {{d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length ? d_t_length : d_q_length, d_score}, d_identities, d_aln_length},
                         n_rows, n_regions, o, out);
    });
}
// the chain of an object's own columns (ks_rscores, ks_raligns)
template <typename T> static int ks_rchain_of(ks_ctx *ctx, const T *s, const ks_rchain_opts *opts, ks_rchain **out) {
    ks_rchain_opts o;
    KS_TRY(ks_rchain_opts_check(ctx, opts, &o));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!s) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "region chain", s));
    return ks_rchain_run(ctx, s->cols(), s->n_rows, s->n_regions, o, out);
}
extern "C" int ks_raligns_chain(ks_ctx *ctx, const ks_raligns *s, const ks_rchain_opts *opts, ks_rchain **out) {
    return ks_guard(ctx, [&]() -> int { return ks_rchain_of(ctx, s, opts, out); });
}
extern "C" int ks_rscores_chain(ks_ctx *ctx, const ks_rscores *s, const ks_rchain_opts *opts, ks_rchain **out) {
    return ks_guard(ctx, [&]() -> int { return ks_rchain_of(ctx, s, opts, out); });
}
extern "C" uint64_t ks_rchain_n_rows(const ks_rchain *c) { return c ? c->n_rows : 0; }
extern "C" uint64_t ks_rchain_n_regions(const ks_rchain *c) { return c ? c->n_regions : 0; }
extern "C" uint64_t ks_rchain_n_chained(const ks_rchain *c) { return c ? c->n_chained : 0; }
extern "C" const uint64_t *ks_rchain_device_row_offsets(const ks_rchain *c) { return c ? c->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_rchain_device_src_region(const ks_rchain *c) { return c ? c->d_src_region : nullptr; }
extern "C" const int64_t *ks_rchain_device_best(const ks_rchain *c) { return c ? c->d_best : nullptr; }
extern "C" const uint32_t *ks_rchain_device_pred(const ks_rchain *c) { return c ? c->d_pred : nullptr; }
extern "C" const int64_t *ks_rchain_device_chain_score(const ks_rchain *c) { return c ? c->d_chain_score : nullptr; }
extern "C" const uint32_t *ks_rchain_device_q_start(const ks_rchain *c) { return c ? c->d_q_start : nullptr; }
extern "C" const uint32_t *ks_rchain_device_q_length(const ks_rchain *c) { return c ? c->d_q_length : nullptr; }
extern "C" const uint32_t *ks_rchain_device_t_start(const ks_rchain *c) { return c ? c->d_t_start : nullptr; }
extern "C" const uint32_t *ks_rchain_device_t_length(const ks_rchain *c) { return c ? c->d_t_length : nullptr; }
extern "C" const uint32_t *ks_rchain_device_q_aligned(const ks_rchain *c) { return c ? c->d_q_aligned : nullptr; }
extern "C" const uint32_t *ks_rchain_device_t_aligned(const ks_rchain *c) { return c ? c->d_t_aligned : nullptr; }
extern "C" const uint64_t *ks_rchain_device_identities(const ks_rchain *c) { return c ? c->d_identities : nullptr; }
extern "C" const uint64_t *ks_rchain_device_aln_length(const ks_rchain *c) { return c ? c->d_aln_length : nullptr; }
extern "C" const double *ks_rchain_device_row_chain_score(const ks_rchain *c) { return c ? c->d_row_score : nullptr; }
extern "C" const double *ks_rchain_device_row_coverage(const ks_rchain *c) { return c ? c->d_row_cov : nullptr; }

extern "C" int ks_rchain_copy_to_host(ks_ctx *ctx, const ks_rchain *c, uint64_t *row_offsets, uint32_t *src_region, int64_t *best, uint32_t *pred,
                                      int64_t *chain_score, uint32_t *q_start, uint32_t *q_length, uint32_t *t_start, uint32_t *t_length,
                                      uint32_t *q_aligned, uint32_t *t_aligned, uint64_t *identities, uint64_t *aln_length, double *row_chain_score) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, row_offsets, src_region, best, pred, chain_score, q_start, q_length, t_start,
                                                              t_length, q_aligned, t_aligned, identities, aln_length, row_chain_score); });
}

extern "C" void ks_rchain_free(ks_rchain *c) { ks_obj_free(c); }

extern "C" int ks_rchain_coverage(ks_ctx *ctx, ks_rchain *chain, const ks_hits *hits, const uint64_t *d_q_off, uint32_t n_q, const uint64_t *d_t_off,
                                  uint32_t n_t, uint32_t mode) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!chain || !hits || !d_q_off || !d_t_off) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "chain coverage", chain, hits));
    if (mode > 3u) return ks_fail(ctx, KS_ERR_INVALID_ARG, "chain coverage: mode %u (0 query, 1 target, 2 the smaller, 3 the larger)", mode);
    if (hits->n_hits != chain->n_rows)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "chain coverage: the hit list has %llu rows, the chain was made of %llu: hits of other regions",
                       (unsigned long long)hits->n_hits, (unsigned long long)chain->n_rows);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    return ks_rchain_coverage_impl(ctx, chain, hits, d_q_off, n_q, d_t_off, n_t, mode);
    });
}
extern "C" int ks_rchain_coverage_to_host(ks_ctx *ctx, const ks_rchain *c, double *row_coverage) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !c) return KS_ERR_INVALID_ARG;
    if (!c->d_row_cov) return ks_fail(ctx, KS_ERR_INVALID_ARG, "chain coverage: ks_rchain_coverage has not filled the column");
    const ks_column col{row_coverage, c->d_row_cov, (size_t)c->n_rows * sizeof(double)};
    return ks_columns_to_host(ctx, &col, 1);
    });
}

// ---------------------------------------------------------------------------------------------
// frame fold (ks_ffold.hip): the frame rows of a translated search as one row per (record, strand, target)
// ---------------------------------------------------------------------------------------------
// what both forms do first: the options (refused before anything else, also with ctx == NULL), the context, the outputs cleared
static int ks_ffold_begin(ks_ctx *ctx, const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out) {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "frame fold", opts->flags, 0u, opts->reserved[0] | opts->reserved[1] | opts->reserved[2]));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out_hits) *out_hits = nullptr;
    if (out) *out = nullptr;
    return KS_OK;
}
static int ks_ffold_run(ks_ctx *ctx, const ks_hits *hits, const u64 *d_nt_offsets, u32 n_records, const ks_rchain_cols &cols, u64 n_regions,
                        ks_hits **out_hits, ks_ffold **out) {
    if (!hits || !out_hits || !out || !d_nt_offsets || !cols.row_offs || (n_regions && (!cols.qs || !cols.ql || !cols.ts || !cols.tl)))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "frame fold", hits));
    if (hits->n_hits == 0 && n_regions != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: %llu regions in no hit row: row_offsets is not a CSR from 0 to n", (unsigned long long)n_regions);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_hits> F(ctx, out_hits, ks_hits_free);
    ks_result<ks_ffold> D(ctx, out, ks_ffold_free);
    KS_TRY(ks_frames_fold_impl(ctx, hits, d_nt_offsets, n_records, cols, n_regions, F, D));
    F.commit();
    return D.commit();
}
extern "C" int ks_frames_fold_device(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records,
                                     const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length, const uint32_t *d_t_start,
                                     const uint32_t *d_t_length, const int64_t *d_score, const uint32_t *d_identities, const uint32_t *d_aln_length,
                                     uint64_t n_regions, const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out) {
    return ks_guard(ctx, [&]() -> int {
    KS_TRY(ks_ffold_begin(ctx, opts, out_hits, out));
    return ks_ffold_run(ctx, frame_hits, d_nt_offsets, n_records,
                        {{d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length ? d_t_length : d_q_length, d_score}, d_identities, d_aln_length},
                        n_regions, out_hits, out);
    });
}
// the fold of an object's own columns (ks_rscores, ks_raligns): the views the chain reads
template <typename T> static int ks_ffold_of(ks_ctx *ctx, const ks_hits *hits, const u64 *d_nt_offsets, u32 n_records, const T *s, const ks_ffold_opts *opts,
                                             ks_hits **out_hits, ks_ffold **out) {
    KS_TRY(ks_ffold_begin(ctx, opts, out_hits, out));
    if (!s || !hits) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "frame fold", s));
    if constexpr (std::is_same_v<T, ks_raligns>) KS_TRY(ks_refuse_by_profile(ctx, "frame fold", s));
    if (s->n_rows != hits->n_hits)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: the regions cover %llu hit rows, the hit list holds %llu: regions of another list",
                       (unsigned long long)s->n_rows, (unsigned long long)hits->n_hits);
    return ks_ffold_run(ctx, hits, d_nt_offsets, n_records, s->cols(), s->n_regions, out_hits, out);
}
extern "C" int ks_rscores_fold_frames(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records, const ks_rscores *scores,
                                      const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out) {
    return ks_guard(ctx, [&]() -> int { return ks_ffold_of(ctx, frame_hits, d_nt_offsets, n_records, scores, opts, out_hits, out); });
}
extern "C" int ks_raligns_fold_frames(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records, const ks_raligns *alignments,
                                      const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out) {
    return ks_guard(ctx, [&]() -> int { return ks_ffold_of(ctx, frame_hits, d_nt_offsets, n_records, alignments, opts, out_hits, out); });
}
extern "C" uint64_t ks_ffold_n_rows(const ks_ffold *f) { return f ? f->n_rows : 0; }
extern "C" uint64_t ks_ffold_n_regions(const ks_ffold *f) { return f ? f->n_regions : 0; }
extern "C" uint64_t ks_ffold_n_src_rows(const ks_ffold *f) { return f ? f->n_src_rows : 0; }
extern "C" const uint32_t *ks_ffold_device_src_row(const ks_ffold *f) { return f ? f->d_src_row : nullptr; }
extern "C" const uint64_t *ks_ffold_device_row_offsets(const ks_ffold *f) { return f ? f->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_ffold_device_src_region(const ks_ffold *f) { return f ? f->d_src_region : nullptr; }
extern "C" const uint8_t *ks_ffold_device_frame(const ks_ffold *f) { return f ? f->d_frame : nullptr; }
extern "C" const uint32_t *ks_ffold_device_nt_length(const ks_ffold *f) { return f ? f->d_nt_length : nullptr; }
extern "C" const uint32_t *ks_ffold_device_s_start(const ks_ffold *f) { return f ? f->d_s_start : nullptr; }
extern "C" const uint32_t *ks_ffold_device_nt_start(const ks_ffold *f) { return f ? f->d_nt_start : nullptr; }
extern "C" const uint32_t *ks_ffold_device_t_start3(const ks_ffold *f) { return f ? f->d_t_start3 : nullptr; }
extern "C" const uint32_t *ks_ffold_device_t_length3(const ks_ffold *f) { return f ? f->d_t_length3 : nullptr; }
extern "C" const int64_t *ks_ffold_device_score(const ks_ffold *f) { return f ? f->d_score : nullptr; }
extern "C" const uint32_t *ks_ffold_device_identities(const ks_ffold *f) { return f ? f->d_identities : nullptr; }
extern "C" const uint32_t *ks_ffold_device_aln_length(const ks_ffold *f) { return f ? f->d_aln_length : nullptr; }
extern "C" int ks_ffold_copy_to_host(ks_ctx *ctx, const ks_ffold *f, uint32_t *src_row, uint64_t *row_offsets, uint32_t *src_region, uint8_t *frame,
                                     uint32_t *nt_length, uint32_t *s_start, uint32_t *nt_start, uint32_t *t_start3, uint32_t *t_length3, int64_t *score,
                                     uint32_t *identities, uint32_t *aln_length) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, f, src_row, row_offsets, src_region, frame, nt_length, s_start, nt_start, t_start3,
                                                              t_length3, score, identities, aln_length); });
}
extern "C" void ks_ffold_free(ks_ffold *f) { ks_obj_free(f); }

// ---------------------------------------------------------------------------------------------
// region stitch (ks_rstitch.hip): the chain of each hit row as one gapped alignment with one CIGAR
// ---------------------------------------------------------------------------------------------
// the options ks_regions_stitch and ks_frames_stitch share; *max_fill: 0 becomes the default
static int ks_stitch_opts_check(ks_ctx *ctx, const char *pass, u32 flags, u32 reserved, u32 *max_fill) {
    KS_TRY(ks_opts_words_check(ctx, pass, flags, KS_RSTITCH_EQX, reserved));
    if (*max_fill <= KS_RSTITCH_MAX_FILL) { *max_fill = *max_fill ? *max_fill : 1024u; return KS_OK; }
    return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "%s options: max_fill %u (at most %u, 0 = 1024)", pass, *max_fill, KS_RSTITCH_MAX_FILL) : KS_ERR_INVALID_ARG;
}
extern "C" int ks_regions_stitch(ks_ctx *ctx, const ks_rchain *chain, const ks_raligns *alignments, const ks_cigars *cigars, const ks_hits *hits,
                                 const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res,
                                 const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_rstitch_opts *opts, ks_hitalns **out) {
    return ks_guard(ctx, [&]() -> int {
    const ks_rstitch_opts dflt = {0u, 0u, 0u, {0u, 0u}};
    ks_rstitch_opts o = opts ? *opts : dflt;
    KS_TRY(ks_stitch_opts_check(ctx, "region stitch", o.flags, o.reserved[0] | o.reserved[1], &o.max_fill));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!chain || !alignments || !cigars || !hits || !out || !d_q_offs || !d_t_offs || (n_q_res && !d_q_res) || (n_t_res && !d_t_res))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "region stitch", chain, alignments, cigars, hits));
    KS_TRY(ks_refuse_by_profile(ctx, "region stitch", alignments));
    if (chain->n_rows != alignments->n_rows || cigars->n_rows != alignments->n_rows || hits->n_hits != alignments->n_rows ||
        chain->n_regions != alignments->n_regions || cigars->n_regions != alignments->n_regions)
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "region stitch: the chain is of %llu regions in %llu hit rows, the alignments are %llu in %llu, the CIGARs %llu in %llu, "
                       "the hit list has %llu rows: objects of other regions",
                       (unsigned long long)chain->n_regions, (unsigned long long)chain->n_rows, (unsigned long long)alignments->n_regions,
                       (unsigned long long)alignments->n_rows, (unsigned long long)cigars->n_regions, (unsigned long long)cigars->n_rows,
                       (unsigned long long)hits->n_hits);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    const ks_res_batch Q{d_q_res, d_q_offs, n_q, n_q_res}, T{d_t_res, d_t_offs, n_t, n_t_res};
    ks_result<ks_hitalns> R(ctx, out, ks_hitalns_free);
    KS_TRY(ks_regions_stitch_impl(ctx, chain, alignments, cigars, hits, Q, T, o.max_fill, o.flags, o.max_scratch_bytes, R));
    return R.commit();
    });
}
extern "C" uint64_t ks_hitalns_n_rows(const ks_hitalns *a) { return a ? a->n_rows : 0; }
extern "C" uint64_t ks_hitalns_n_ops(const ks_hitalns *a) { return a ? a->n_ops : 0; }
extern "C" uint64_t ks_hitalns_scratch_bytes(const ks_hitalns *a) { return a ? a->dir_bytes : 0; }
extern "C" uint32_t ks_hitalns_n_slices(const ks_hitalns *a) { return a ? a->n_slices : 0; }
extern "C" const uint64_t *ks_hitalns_device_op_offsets(const ks_hitalns *a) { return a ? a->d_op_offsets : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_ops(const ks_hitalns *a) { return a ? a->d_ops : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_q_start(const ks_hitalns *a) { return a ? a->d_q_start : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_q_length(const ks_hitalns *a) { return a ? a->d_q_length : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_t_start(const ks_hitalns *a) { return a ? a->d_t_start : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_t_length(const ks_hitalns *a) { return a ? a->d_t_length : nullptr; }
extern "C" const int64_t *ks_hitalns_device_score(const ks_hitalns *a) { return a ? a->d_score : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_identities(const ks_hitalns *a) { return a ? a->d_identities : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_positives(const ks_hitalns *a) { return a ? a->d_positives : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_gap_opens(const ks_hitalns *a) { return a ? a->d_gap_opens : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_gaps(const ks_hitalns *a) { return a ? a->d_gaps : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_aln_length(const ks_hitalns *a) { return a ? a->d_aln_length : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_n_members(const ks_hitalns *a) { return a ? a->d_n_members : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_n_filled(const ks_hitalns *a) { return a ? a->d_n_filled : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_n_open(const ks_hitalns *a) { return a ? a->d_n_open : nullptr; }
extern "C" const uint32_t *ks_hitalns_device_n_trimmed(const ks_hitalns *a) { return a ? a->d_n_trimmed : nullptr; }
extern "C" const double *ks_hitalns_device_row_score(const ks_hitalns *a) { return a ? a->d_row_score : nullptr; }

extern "C" int ks_hitalns_copy_to_host(ks_ctx *ctx, const ks_hitalns *a, uint64_t *op_offsets, uint32_t *ops, uint32_t *q_start, uint32_t *q_length,
                                       uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities, uint32_t *positives,
                                       uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length, uint32_t *n_members, uint32_t *n_filled,
                                       uint32_t *n_open, uint32_t *n_trimmed, double *row_score) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, a, op_offsets, ops, q_start, q_length, t_start, t_length, score, identities,
                                                              positives, gap_opens, gaps, aln_length, n_members, n_filled, n_open, n_trimmed,
                                                              row_score); });
}

extern "C" void ks_hitalns_free(ks_hitalns *a) { ks_obj_free(a); }

// ---------------------------------------------------------------------------------------------
// frame stitch (ks_fstitch.hip): the chain of each folded row as one alignment of the strand's bases, frameshifts as N ops
// ---------------------------------------------------------------------------------------------
extern "C" int ks_frames_stitch(ks_ctx *ctx, const ks_ffold *fold, const ks_hits *folded_hits, const ks_rchain *chain, const ks_raligns *alignments,
                                const ks_cigars *cigars, const uint8_t *d_f_res, const uint64_t *d_f_offs, uint32_t n_f, uint64_t n_f_res,
                                const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_fstitch_opts *opts,
                                ks_framealns **out) {
    return ks_guard(ctx, [&]() -> int {
    const ks_fstitch_opts dflt = {0u, 0u, 15u, 0u, 0u};
    ks_fstitch_opts o = opts ? *opts : dflt;
    KS_TRY(ks_stitch_opts_check(ctx, "frame stitch", o.flags, o.reserved, &o.max_fill));
    if (o.frameshift_cost > KS_FSTITCH_MAX_COST)
        return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch options: frameshift_cost %u (at most %u)", o.frameshift_cost, KS_FSTITCH_MAX_COST)
                   : KS_ERR_INVALID_ARG;
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!fold || !folded_hits || !chain || !alignments || !cigars || !out || !d_f_offs || !d_t_offs || (n_f_res && !d_f_res) || (n_t_res && !d_t_res))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "frame stitch", fold, folded_hits, chain, alignments, cigars));
    KS_TRY(ks_refuse_by_profile(ctx, "frame stitch", alignments));
    if (chain->n_rows != fold->n_rows || folded_hits->n_hits != fold->n_rows || chain->n_regions != fold->n_regions ||
        fold->n_regions != alignments->n_regions || fold->n_src_rows != alignments->n_rows || cigars->n_regions != alignments->n_regions ||
        cigars->n_rows != alignments->n_rows)
        return ks_fail(ctx, KS_ERR_INVALID_ARG,
                       "frame stitch: the fold is of %llu regions of %llu frame rows in %llu folded rows, the chain of %llu regions in %llu rows, the "
                       "folded hit list has %llu rows, the alignments are %llu in %llu frame rows, the CIGARs %llu in %llu: objects of other regions",
                       (unsigned long long)fold->n_regions, (unsigned long long)fold->n_src_rows, (unsigned long long)fold->n_rows,
                       (unsigned long long)chain->n_regions, (unsigned long long)chain->n_rows, (unsigned long long)folded_hits->n_hits,
                       (unsigned long long)alignments->n_regions, (unsigned long long)alignments->n_rows, (unsigned long long)cigars->n_regions,
                       (unsigned long long)cigars->n_rows);
    KS_HIP(ctx, hipSetDevice(ctx->device));
    const ks_res_batch Q{d_f_res, d_f_offs, n_f, n_f_res}, T{d_t_res, d_t_offs, n_t, n_t_res};
    ks_result<ks_framealns> R(ctx, out, ks_framealns_free);
    KS_TRY(ks_frames_stitch_impl(ctx, fold, folded_hits, chain, alignments, cigars, Q, T, o.max_fill, o.flags, o.frameshift_cost,
                                 o.max_scratch_bytes, R));
    return R.commit();
    });
}
extern "C" uint64_t ks_framealns_n_rows(const ks_framealns *a) { return a ? a->n_rows : 0; }
extern "C" uint64_t ks_framealns_n_ops(const ks_framealns *a) { return a ? a->n_ops : 0; }
extern "C" uint64_t ks_framealns_scratch_bytes(const ks_framealns *a) { return a ? a->dir_bytes : 0; }
extern "C" uint32_t ks_framealns_n_slices(const ks_framealns *a) { return a ? a->n_slices : 0; }
extern "C" const uint64_t *ks_framealns_device_op_offsets(const ks_framealns *a) { return a ? a->d_op_offsets : nullptr; }
extern "C" const uint32_t *ks_framealns_device_ops(const ks_framealns *a) { return a ? a->d_ops : nullptr; }
extern "C" const uint32_t *ks_framealns_device_s_start(const ks_framealns *a) { return a ? a->d_s_start : nullptr; }
extern "C" const uint32_t *ks_framealns_device_nt_length(const ks_framealns *a) { return a ? a->d_nt_length : nullptr; }
extern "C" const uint32_t *ks_framealns_device_nt_start(const ks_framealns *a) { return a ? a->d_nt_start : nullptr; }
extern "C" const uint32_t *ks_framealns_device_t_start(const ks_framealns *a) { return a ? a->d_t_start : nullptr; }
extern "C" const uint32_t *ks_framealns_device_t_length(const ks_framealns *a) { return a ? a->d_t_length : nullptr; }
extern "C" const int64_t *ks_framealns_device_score(const ks_framealns *a) { return a ? a->d_score : nullptr; }
extern "C" const uint32_t *ks_framealns_device_identities(const ks_framealns *a) { return a ? a->d_identities : nullptr; }
extern "C" const uint32_t *ks_framealns_device_positives(const ks_framealns *a) { return a ? a->d_positives : nullptr; }
extern "C" const uint32_t *ks_framealns_device_gap_opens(const ks_framealns *a) { return a ? a->d_gap_opens : nullptr; }
extern "C" const uint32_t *ks_framealns_device_gaps(const ks_framealns *a) { return a ? a->d_gaps : nullptr; }
extern "C" const uint32_t *ks_framealns_device_aln_length(const ks_framealns *a) { return a ? a->d_aln_length : nullptr; }
extern "C" const uint32_t *ks_framealns_device_n_members(const ks_framealns *a) { return a ? a->d_n_members : nullptr; }
extern "C" const uint32_t *ks_framealns_device_n_filled(const ks_framealns *a) { return a ? a->d_n_filled : nullptr; }
extern "C" const uint32_t *ks_framealns_device_n_open(const ks_framealns *a) { return a ? a->d_n_open : nullptr; }
extern "C" const uint32_t *ks_framealns_device_n_trimmed(const ks_framealns *a) { return a ? a->d_n_trimmed : nullptr; }
extern "C" const uint32_t *ks_framealns_device_n_frameshifts(const ks_framealns *a) { return a ? a->d_n_frameshifts : nullptr; }
extern "C" const double *ks_framealns_device_row_score(const ks_framealns *a) { return a ? a->d_row_score : nullptr; }
extern "C" int ks_framealns_copy_to_host(ks_ctx *ctx, const ks_framealns *a, uint64_t *op_offsets, uint32_t *ops, uint32_t *s_start, uint32_t *nt_length,
                                         uint32_t *nt_start, uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities,
                                         uint32_t *positives, uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length, uint32_t *n_members,
                                         uint32_t *n_filled, uint32_t *n_open, uint32_t *n_trimmed, uint32_t *n_frameshifts, double *row_score) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, a, op_offsets, ops, s_start, nt_length, nt_start, t_start, t_length, score,
                                                              identities, positives, gap_opens, gaps, aln_length, n_members, n_filled, n_open,
                                                              n_trimmed, n_frameshifts, row_score); });
}
extern "C" void ks_framealns_free(ks_framealns *a) { ks_obj_free(a); }
