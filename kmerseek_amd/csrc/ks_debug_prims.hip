// ks_debug_prims.hip — test hooks: the device-wide primitives (the exclusive scans and the LSD radix sort of ks_prims.hip, the
// MSD match sort of ks_msd.hip) called directly on the caller's device arrays, so that the tests choose the keys, the sizes and
// the state of the scan ring instead of taking what a sketch or a join happens to produce.  No kernel here: every entry checks
// its arguments on the host, borrows scratch from the pool, calls the internal function the pipelines call, makes ONE wait and
// reads the scans' give-up word (ks_scan_status_check) — synchronous on return, nothing of the hot path changes.
#include "ks_common.h"

#define DP_MAX_N 0xffffffffULL // records: n < 2^32 - 1 (the sorts' offsets are 32-bit)

extern "C" int ks_debug_scan(ks_ctx *ctx, int kind, const uint32_t *d_in, void *d_out, uint64_t n, uint32_t *d_total) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !d_in || !d_out || kind < 0 || kind > 2 || n >= DP_MAX_N) return KS_ERR_INVALID_ARG;
    KS_HIP(ctx, hipSetDevice(ctx->device));
    if (kind == 0) {
        KS_TRY(ks_scan_u32_to_u64(ctx, d_in, (u64 *)d_out, n));
    } else if (kind == 2) {
        KS_TRY(ks_scan_u32_to_u64_wide(ctx, d_in, (u64 *)d_out, n));
    } else {
        if (n) KS_HIP(ctx, hipMemcpyAsync(d_out, d_in, (size_t)n * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
        KS_TRY(ks_scan_u32_inplace(ctx, (u32 *)d_out, n, d_total));
    }
    return ks_stream_wait_fetch_scans(ctx, {});
    });
}

extern "C" int ks_debug_scan_seek(ks_ctx *ctx, uint32_t global_tile) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_scan_ring_make(ctx));
    // (the ring keeps its words: what earlier scans left in it is what the scans behind this call have to tell from their own)
    KS_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->scan_ticket, (int)global_tile, 1, ctx->stream));
    ctx->scan_ticket_base = global_tile;
    return ks_stream_wait_fetch_scans(ctx, {});
    });
}

extern "C" int ks_debug_scan_ticket(ks_ctx *ctx, uint32_t *base) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !base) return KS_ERR_INVALID_ARG;
    *base = ctx->scan_ticket_base;
    return KS_OK;
    });
}

extern "C" int ks_debug_radix_sort(ks_ctx *ctx, int vbytes, const uint64_t *d_keys, const void *d_vals, uint64_t n, const int *shifts,
                                   int n_shifts, uint32_t pfxK, const uint32_t *seg_len, uint64_t seg_cap, uint32_t seg_regions,
                                   int alias_in, uint64_t *d_keys_out, void *d_vals_out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !d_keys || !d_keys_out || !shifts || (vbytes != 0 && vbytes != 4 && vbytes != 8)) return KS_ERR_INVALID_ARG;
    if (vbytes && (!d_vals || !d_vals_out)) return KS_ERR_INVALID_ARG;
    if (n >= DP_MAX_N || n_shifts < 1 || n_shifts > 8) return KS_ERR_INVALID_ARG;
    for (int i = 0; i < n_shifts; i++)
        if (shifts[i] < 0 || shifts[i] > 56) return KS_ERR_INVALID_ARG;
    if ((pfxK || seg_len) && vbytes != 4) return KS_ERR_INVALID_ARG; // (join-prefix digits and segments: the u32-valued sort only)
    u64 n_in = n; // records the input arrays span
    if (seg_len) {
        if (seg_cap == 0 || seg_regions == 0 || seg_regions > 65536u || seg_cap * seg_regions >= DP_MAX_N) return KS_ERR_INVALID_ARG;
        n_in = seg_cap * seg_regions;
    }
    KS_HIP(ctx, hipSetDevice(ctx->device));
    if (seg_len) { // the fills as the kernels will read them: none beyond its region, n of them in all
        std::vector<u32> len(seg_regions);
        KS_HIP(ctx, hipMemcpyAsync(len.data(), seg_len, (size_t)seg_regions * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        u64 sum = 0;
        for (u32 r = 0; r < seg_regions; r++) {
            if (len[r] > seg_cap) return ks_fail(ctx, KS_ERR_INVALID_ARG, "debug radix sort: region %u holds more than its capacity", r);
            sum += len[r];
        }
        if (sum != n) return ks_fail(ctx, KS_ERR_INVALID_ARG, "debug radix sort: the regions hold %llu records, not n", (unsigned long long)sum);
    }
    ks_scratch sc(ctx);
    const size_t n_a = (size_t)(alias_in && n_in > n ? n_in : n);
    u64 *ka = nullptr, *kb = nullptr;
    void *va = nullptr, *vb = nullptr;
    KS_TRY(sc.alloc(&ka, n_a));
    KS_TRY(sc.alloc(&kb, (size_t)n));
    if (vbytes) {
        u8 *a = nullptr, *b = nullptr;
        KS_TRY(sc.alloc(&a, n_a * (size_t)vbytes));
        KS_TRY(sc.alloc(&b, (size_t)n * (size_t)vbytes));
        va = a; vb = b;
    }
    const u64 *kin = d_keys;
    const void *vin = d_vals;
    if (alias_in) { // the in-place form: the input IS the first scratch pair
        if (n_in) KS_HIP(ctx, hipMemcpyAsync(ka, d_keys, (size_t)n_in * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
        if (n_in && vbytes) KS_HIP(ctx, hipMemcpyAsync(va, d_vals, (size_t)n_in * (size_t)vbytes, hipMemcpyDeviceToDevice, ctx->stream));
        kin = ka; vin = va;
    }
    u64 *ko = nullptr;
    void *vo = nullptr;
    if (vbytes == 0) {
        KS_TRY(ks_radix_sort_keys(ctx, KS_SORT_PAIRS, kin, ka, kb, n, shifts, n_shifts, &ko));
    } else if (vbytes == 4) {
        ks_rs_segments seg;
        seg.len = seg_len; seg.cap = seg_cap; seg.regions = seg_regions; seg.sub_shift = 0;
        u32 *o = nullptr;
        KS_TRY(ks_radix_sort_u32(ctx, (seg_len || pfxK) ? KS_SORT_QPART : KS_SORT_PAIRS, kin, (const u32 *)vin, ka, (u32 *)va, kb, (u32 *)vb, n, shifts,
                                 n_shifts, &ko, &o, seg_len ? &seg : nullptr, pfxK));
        vo = o;
    } else {
        u64 *o = nullptr;
        KS_TRY(ks_radix_sort_u64(ctx, KS_SORT_INDEX, kin, (const u64 *)vin, ka, (u64 *)va, kb, (u64 *)vb, n, shifts, n_shifts, &ko, &o));
        vo = o;
    }
    // wherever the result lies: a scratch pair, or the input handed back (nothing to sort)
    if (n) KS_HIP(ctx, hipMemcpyAsync(d_keys_out, ko, (size_t)n * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    if (n && vbytes) KS_HIP(ctx, hipMemcpyAsync(d_vals_out, vo, (size_t)n * (size_t)vbytes, hipMemcpyDeviceToDevice, ctx->stream));
    return ks_stream_wait_fetch_scans(ctx, {});
    });
}

extern "C" int ks_debug_msd_sort(ks_ctx *ctx, uint64_t *d_keys, uint64_t n, int lo_bit, int nbits, const uint32_t *seg_count, uint32_t n_segs,
                                 uint64_t seg_cap, uint32_t info[4]) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx || !d_keys || !info || n >= DP_MAX_N) return KS_ERR_INVALID_ARG;
    if (lo_bit < 0 || lo_bit > 63 || nbits < 1 || nbits > 64 - lo_bit) return KS_ERR_INVALID_ARG;
    ks_msd_segs sg;
    if (seg_count) { // the table ks_search.hip makes of the join's segments: level-1 tiles of 8192 records, none across a segment's end
        if (n_segs < 1 || n_segs > KS_MSD_MAX_SEGS || seg_cap == 0 || seg_cap * n_segs >= DP_MAX_N) return KS_ERR_INVALID_ARG;
        sg.n = n_segs; sg.seg_cap = seg_cap;
        u32 t = 0;
        u64 sum = 0;
        for (u32 s = 0; s < n_segs; s++) {
            if (seg_count[s] > seg_cap) return KS_ERR_INVALID_ARG;
            sg.tile_start[s] = t; sg.count[s] = seg_count[s];
            t += (u32)(((u64)seg_count[s] + 8191) / 8192);
            sum += seg_count[s];
        }
        if (sum != n) return KS_ERR_INVALID_ARG;
        for (u32 s = n_segs; s <= KS_MSD_MAX_SEGS; s++) sg.tile_start[s] = t;
        for (u32 s = n_segs; s < KS_MSD_MAX_SEGS; s++) sg.count[s] = 0;
    }
    KS_HIP(ctx, hipSetDevice(ctx->device));
    info[0] = info[1] = info[2] = info[3] = 0;
    ks_scratch sc(ctx);
    u64 *kb = nullptr;
    KS_TRY(sc.alloc(&kb, (size_t)n));
    ks_msd_plan P;
    KS_TRY(ks_msd_level1(ctx, d_keys, kb, n, lo_bit, nbits, seg_count ? &sg : nullptr, &P));
    if (!P.blk) return ks_stream_wait_fetch_scans(ctx, {}); // not applicable: nothing was launched, the list is as it was
    int bits2 = 0;
    const ms_layout L = ms_layout_of(n, lo_bit, nbits, &bits2);
    // the counter of the buckets k_msd_local lists for k_msd_local_big: the word behind the histograms.  ks_msd_finish hands the
    // block back to the pool, which only marks it free: nothing is allocated between that and the fetch queued right behind it.
    const u32 *big = P.blk + (L.n_zero - 1);
    KS_TRY(ks_msd_finish(ctx, &P));
    u32 *h = (u32 *)(ctx->h_pin + KS_PIN_READ);
    *h = 0;
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ks_fetch_words(big, h, 1)}));
    info[0] = 1; info[1] = (u32)bits2; info[2] = L.n_buckets; info[3] = *h;
    return KS_OK;
    });
}
