// ks_regions.hip — ks_match_regions: every hit row's (query start, target start) pairs chained into maximal colinear regions
// (the `query:start-end` found in `target:start-end` line of a match; the reference's stitcher, src/python/kmerseek/search.py:37-121,
// assumes ONE such run per row).  A region: pairs of one row on one diagonal d = t_start - q_start whose query starts, ascending,
// step by at most ksize + max_gap.
//
//   1. k_rg_keys    a lane per pair: row | d + bias | q_start   (bias = the longest query start: the diagonal field is unsigned);
//                   the row comes from row_offsets, a workgroup's slice of it staged in LDS
//   2. the keys sorted on their live bits (ks_sort_live_keys): pairs of a region are neighbours, ascending by q_start
//   3. k_rg_heads   thread i compares key i with key i - 1 -> head flag, coverage term min(ksize, step); both scanned (one launch each)
//   4. k_rg_pos     head i -> pos[region index] = i, and the end of the slice's pairs behind the last head
//   5. k_rg_chain   a lane per region: the five columns from keys[pos[r]], keys[pos[r + 1] - 1] and the scanned terms; the regions
//                   with n_kmers >= min_kmers take a place in the list of kept regions — one atomicAdd per wave, the device-side
//                   running total over the slices — in no particular order
//   6. the kept count comes back (first wait); the kept regions are sorted by (row, q_start, t_start), a total order, through
//      a permutation column: one LSD sort when the three fields fit 64 bits, else by (q_start, t_start) and then, stably, by row
//   7. k_rg_gather  the five columns in that order, k_rg_csr row_offsets from the sorted row column (second wait)
// Row, diagonal and start that do not fit 64 bits together: slices of hit rows as in ks_matchpos.hip (steps 1 - 5 per slice).
#include "ks_device.h"

#define RG_THREADS 256
#define RG_IPT 4
#define RG_TILE (RG_THREADS * RG_IPT)
#define RG_STAGE 2048     // rows of a tile whose offsets are staged in LDS (8 KB); more (runs of rows without a pair): searched in memory
#define RG_CHAIN_GRID 2048 // workgroups of k_rg_chain, striding over the slice's regions (their number is known on the device only)

// Pair p belongs to the row r with off[r] <= p < off[r + 1]: the last row whose offset is <= p (rows without a pair are never found).
__global__ __launch_bounds__(RG_THREADS) void k_rg_keys(const u64 *off, u32 n_rows, const u32 *qs, const u32 *ts, u64 n, u32 bias, ks_slice_fmt F,
                                                        u64 *keys) {
    __shared__ u32 s_rel[RG_STAGE];
    __shared__ u32 s_w[2];
    const u32 tid = threadIdx.x;
    const u64 begin = (u64)blockIdx.x * RG_TILE;
    const u64 end = begin + RG_TILE < n ? begin + RG_TILE : n;
    if (tid < 2) s_w[tid] = ks_last_le_u64(off, 0, n_rows - 1, tid == 0 ? begin : end - 1); // (off[0] == 0 <= p)
    __syncthreads();
    const u32 r_first = s_w[0], r_last = s_w[1], span = r_last - r_first + 1;
    const bool staged = span <= RG_STAGE;
    if (staged) { // every row after the first starts inside the tile: its offset relative to `begin` is < RG_TILE
        for (u32 k = tid; k < span; k += RG_THREADS) s_rel[k] = k ? (u32)(off[r_first + k] - begin) : 0u;
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < RG_IPT; it++) {
        const u32 rel = (u32)it * RG_THREADS + tid;
        const u64 p = begin + rel;
        if (p >= end) continue;
        const u32 row = staged ? r_first + ks_last_le_u32(s_rel, span, rel) : ks_last_le_u64(off, r_first, r_last, p);
        const u32 a = qs[p], b = ts[p];
        const bool mine = row >= F.row0 && row - F.row0 < F.slice_rows;
        keys[p] = mine ? ((u64)(row - F.row0) << F.pqt) | (((u64)b + bias - a) << F.pt) | a : (u64)F.slice_rows << F.pqt;
    }
}

// Thread i < n: is key i the first pair of a region, and what it adds to its region's coverage; thread n closes both columns
// with 0 (their exclusive scans then hold the totals at [n]).
__global__ __launch_bounds__(256) void k_rg_heads(const u64 *keys, u64 n, ks_slice_fmt F, u32 ksize, u32 step, u32 *flag, u32 *term) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    u32 head = 0, add = 0;
    if (i < n) {
        const u64 key = keys[i];
        if ((key >> F.pqt) < F.slice_rows) {
            const u64 prev = i ? keys[i - 1] : 0;
            const u32 amask = (u32)((1ULL << F.pt) - 1ULL);
            const u32 da = ((u32)key & amask) - ((u32)prev & amask); // (same row and diagonal: pairs are distinct, the start grew)
            head = (i == 0 || (key >> F.pt) != (prev >> F.pt) || da > step) ? 1u : 0u;
            add = head ? 0u : (da < ksize ? da : ksize);
        }
    }
    flag[i] = head;
    term[i] = add;
}

// idx: the exclusive scan of the head flags.  pos[r] = the first pair of the slice's r-th region; pos[number of regions] = the end
// of the slice's pairs (the keys of other slices sort behind them).
__global__ __launch_bounds__(256) void k_rg_pos(const u64 *keys, u64 n, ks_slice_fmt F, const u32 *idx, u32 *pos) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const bool valid = i < n && (keys[i] >> F.pqt) < F.slice_rows;
    const u32 mine = idx[i];
    if (valid) { if (idx[i + 1] != mine) pos[mine] = (u32)i; }
    else if (i == 0 || (keys[i - 1] >> F.pqt) < F.slice_rows) pos[mine] = (u32)i;
}

struct rg_cols { u32 *row, *qs, *ts, *len, *nk, *cov; };

// A lane per region of the slice.  kept[0]: regions kept so far (all slices).
__global__ __launch_bounds__(256) void k_rg_chain(const u64 *keys, u64 n, ks_slice_fmt F, const u32 *idx, const u32 *pos, const u32 *cov_scan,
                                                  u32 ksize, u32 bias, u32 min_kmers, u32 *kept, rg_cols T) {
    const u32 cnt = idx[n], lane = threadIdx.x & 63;
    const u32 amask = (u32)((1ULL << F.pt) - 1ULL);
    const u64 dmask = (1ULL << (F.pqt - F.pt)) - 1ULL;
    for (u32 base = blockIdx.x * 256; base < cnt; base += gridDim.x * 256) { // (uniform trip count: the ballot sees whole waves)
        const u32 r = base + threadIdx.x;
        const bool live = r < cnt;
        u32 h = 0, e = 1;
        if (live) { h = pos[r]; e = pos[r + 1]; }
        const u64 kh = live ? keys[h] : 0, kl = live ? keys[e - 1] : 0;
        const u32 a = (u32)kh & amask, nk = e - h;
        const bool keep = live && nk >= min_kmers;
        const u64 m = __ballot(keep);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        u32 o = 0;
        if ((int)lane == leader) o = atomicAdd(kept, (u32)__popcll(m));
        o = (u32)__shfl((int)o, leader) + ks_lane_lt_count(m);
        if (keep) {
            T.row[o] = F.row0 + (u32)(kh >> F.pqt);
            T.qs[o] = a;
            T.ts[o] = (u32)((u64)a + ((kh >> F.pt) & dmask) - bias);
            T.len[o] = ((u32)kl & amask) + ksize - a;
            T.nk[o] = nk;
            T.cov[o] = cov_scan[e] - cov_scan[h] + ksize; // (the head's own term is 0)
        }
    }
}

// sort key of kept region j: (row, q_start, t_start), or the two starts alone (the row is sorted on afterwards); value: j
__global__ __launch_bounds__(256) void k_rg_order_keys(rg_cols T, u32 n, int pt, int pqt, int with_row, u64 *key, u32 *val) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const u64 k = ((u64)T.qs[j] << pt) | T.ts[j];
    key[j] = with_row ? ((u64)T.row[j] << pqt) | k : k;
    val[j] = j;
}
__global__ __launch_bounds__(256) void k_rg_row_keys(const u32 *row, const u32 *val, u32 n, u64 *key) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) key[j] = row[val[j]];
}
__global__ __launch_bounds__(256) void k_rg_gather(rg_cols T, const u32 *perm, u32 n, u32 *srow, u32 *qs, u32 *ts, u32 *len, u32 *nk, u32 *cov) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const u32 v = perm[j];
    srow[j] = T.row[v]; qs[j] = T.qs[v]; ts[j] = T.ts[v]; len[j] = T.len[v]; nk[j] = T.nk[v]; cov[j] = T.cov[v];
}
// row_offsets[r] = the regions of the rows before r, r = 0 .. n_rows
__global__ __launch_bounds__(256) void k_rg_csr(const u32 *srow, u32 n, u32 n_rows, u64 *row_offsets) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r <= n_rows) row_offsets[r] = ks_lower_bound_u32(srow, n, r);
}

static int rg_empty(ks_ctx *ctx, ks_regions *R) {
    KS_TRY(ks_obj_alloc(ctx, R, R->n_regions)); // (0 regions: blocks of one entry)
    KS_HIP(ctx, hipMemsetAsync(R->d_row_offsets, 0, ((size_t)R->n_rows + 1) * sizeof(u64), ctx->stream));
    return ks_stream_wait(ctx);
}

static int rg_run(ks_ctx *ctx, const ks_matchpos *M, u32 min_kmers, u32 max_gap, ks_regions *R) {
    const u64 n_rows = M->n_rows, n = M->n_pairs;
    R->n_rows = n_rows; R->n_regions = 0; R->n_slices = 0;
    KS_TRY(ks_alloc(ctx, &R->d_row_offsets, (size_t)n_rows + 1));
    if (n_rows == 0 || n == 0) return rg_empty(ctx, R);
    const u32 ksize = M->params.ksize;
    const u32 step = ksize + max_gap < ksize ? 0xffffffffu : ksize + max_gap; // (clamped: the sum stays a u32)
    if ((n + 1) * (u64)ksize >= (1ULL << 38)) // (the one-launch scan carries 38 value bits; k <= 64 never gets here)
        return ks_fail(ctx, KS_ERR_CAPACITY, "match regions: %llu pairs at k = %u exceed the coverage scan", (unsigned long long)n, ksize);

    // the key: row | diagonal + bias | query start
    const u32 bias = M->max_qs;
    const int pa = ks_key_bits(M->max_qs), pd = ks_key_bits((u64)M->max_qs + M->max_ts), pt = ks_key_bits(M->max_ts);
    ks_row_slices SL;
    KS_TRY(ks_row_slices_plan(ctx, KS_DBG_REGIONS_ROW_BITS, "match regions", pa + pd, n_rows, &SL));
    R->n_slices = (u32)SL.n_slices;

    ks_scratch sc(ctx);
    u64 *k0 = nullptr, *k1 = nullptr;
    u32 *idx = nullptr, *cov = nullptr, *pos = nullptr, *kept = nullptr;
    rg_cols T;
    KS_TRY(sc.alloc(&k0, (size_t)n)); KS_TRY(sc.alloc(&k1, (size_t)n));
    KS_TRY(sc.alloc(&idx, (size_t)n + 1)); KS_TRY(sc.alloc(&cov, (size_t)n + 1)); KS_TRY(sc.alloc(&pos, (size_t)n + 1));
    KS_TRY(sc.alloc(&kept, 2));
    KS_TRY(sc.alloc(&T.row, (size_t)n)); KS_TRY(sc.alloc(&T.qs, (size_t)n)); KS_TRY(sc.alloc(&T.ts, (size_t)n));
    KS_TRY(sc.alloc(&T.len, (size_t)n)); KS_TRY(sc.alloc(&T.nk, (size_t)n)); KS_TRY(sc.alloc(&T.cov, (size_t)n));
    KS_HIP(ctx, hipMemsetAsync(kept, 0, 2 * sizeof(u32), ctx->stream));
    const u32 g_keys = (u32)((n + RG_TILE - 1) / RG_TILE), g_n1 = (u32)((n + 1 + 255) / 256);
    const u32 g_chain = g_n1 < RG_CHAIN_GRID ? g_n1 : RG_CHAIN_GRID;
    for (u64 s = 0; s < SL.n_slices; s++) {
        const ks_slice_fmt F = SL.fmt(s, n_rows, pa);
        KS_LAUNCH(ctx, "regions_keys", k_rg_keys, g_keys, RG_THREADS, (const u64 *)M->d_row_offsets, (u32)n_rows, (const u32 *)M->d_qstart,
                  (const u32 *)M->d_tstart, n, bias, F, k0);
        u64 *sorted = nullptr;
        KS_TRY(ks_sort_live_keys(ctx, k0, k1, n, F.pqt + ks_key_bits(F.slice_rows), &sorted));
        KS_LAUNCH(ctx, "regions_heads", k_rg_heads, g_n1, 256, (const u64 *)sorted, n, F, ksize, step, idx, cov);
        KS_TRY(ks_scan_u32_inplace(ctx, idx, n + 1, nullptr));
        KS_TRY(ks_scan_u32_inplace(ctx, cov, n + 1, nullptr));
        KS_LAUNCH(ctx, "regions_pos", k_rg_pos, g_n1, 256, (const u64 *)sorted, n, F, (const u32 *)idx, pos);
        KS_LAUNCH(ctx, "regions_chain", k_rg_chain, g_chain, 256, (const u64 *)sorted, n, F, (const u32 *)idx, (const u32 *)pos, (const u32 *)cov,
                  ksize, bias, min_kmers, kept, T);
    }
    u64 *const rb = ctx->h_pin + KS_PIN_REGIONS;
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ks_fetch_words(kept, rb, 2)}));
    const u32 nr = *(const u32 *)rb;
    if (nr > n) return ks_fail(ctx, KS_ERR_HIP, "internal error: %u regions of %llu pairs", nr, (unsigned long long)n);
    if (nr == 0) return rg_empty(ctx, R);
    R->n_regions = nr;
    KS_TRY(ks_obj_alloc(ctx, R, R->n_regions));

    // the order: (row, q_start, t_start).  The chain's scratch holds the sort: keys in k0 / k1, the permutation in idx / cov.
    const int pqt = pa + pt, rbits = ks_key_bits(n_rows - 1);
    int row_room = 64 - pqt;
    if (const char *f = ks_dbg(ctx, KS_DBG_REGIONS_ROW_BITS)) { // (tests: the two-sort order on small inputs)
        const int v = atoi(f);
        if (v >= 1 && v < row_room) row_room = v;
    }
    const int with_row = rbits <= row_room;
    const u32 g_r = (nr + 255) / 256;
    int shifts[8], ns = 0;
    u64 *ks_ = nullptr;
    u32 *perm = nullptr;
    KS_LAUNCH(ctx, "regions_order_keys", k_rg_order_keys, g_r, 256, T, nr, pt, pqt, with_row, k0, idx);
    for (int sh = 0; sh < pqt + (with_row ? rbits : 0); sh += 8) shifts[ns++] = sh;
    KS_TRY(ks_radix_sort_u32(ctx, KS_SORT_PAIRS, k0, idx, k0, idx, k1, cov, nr, shifts, ns, &ks_, &perm));
    if (!with_row) { // a stable sort on the row alone keeps (q_start, t_start) ascending inside every row
        KS_LAUNCH(ctx, "regions_row_keys", k_rg_row_keys, g_r, 256, (const u32 *)T.row, (const u32 *)perm, nr, ks_);
        ns = 0;
        for (int sh = 0; sh < rbits; sh += 8) shifts[ns++] = sh;
        u32 *const v_in = perm;
        KS_TRY(ks_radix_sort_u32(ctx, KS_SORT_PAIRS, ks_, v_in, k0, idx, k1, cov, nr, shifts, ns, &ks_, &perm));
    }
    KS_LAUNCH(ctx, "regions_gather", k_rg_gather, g_r, 256, T, (const u32 *)perm, nr, pos, R->d_qstart, R->d_tstart, R->d_length, R->d_nkmers,
              R->d_covered);
    KS_LAUNCH(ctx, "regions_csr", k_rg_csr, (u32)((n_rows + 256) / 256), 256, (const u32 *)pos, nr, (u32)n_rows, R->d_row_offsets);
    return ks_stream_wait(ctx);
}

extern "C" int ks_match_regions(ks_ctx *ctx, const ks_matchpos *mp, const ks_regions_opts *opts, ks_regions **out) {
    return ks_guard(ctx, [&]() -> int {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "match region", opts->flags, 0, opts->reserved));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!mp || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    KS_TRY(ks_inputs_check_ctx(ctx, "match regions", mp));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_regions> R(ctx, out, ks_regions_free);
    KS_TRY(rg_run(ctx, mp, opts ? opts->min_kmers : 0, opts ? opts->max_gap : 0, R));
    return R.commit();
    });
}

extern "C" uint64_t ks_regions_n_rows(const ks_regions *r) { return r ? r->n_rows : 0; }
extern "C" uint64_t ks_regions_n_regions(const ks_regions *r) { return r ? r->n_regions : 0; }
extern "C" uint32_t ks_regions_n_slices(const ks_regions *r) { return r ? r->n_slices : 0; }
extern "C" const uint64_t *ks_regions_device_row_offsets(const ks_regions *r) { return r ? r->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_regions_device_q_start(const ks_regions *r) { return r ? r->d_qstart : nullptr; }
extern "C" const uint32_t *ks_regions_device_t_start(const ks_regions *r) { return r ? r->d_tstart : nullptr; }
extern "C" const uint32_t *ks_regions_device_length(const ks_regions *r) { return r ? r->d_length : nullptr; }
extern "C" const uint32_t *ks_regions_device_n_kmers(const ks_regions *r) { return r ? r->d_nkmers : nullptr; }
extern "C" const uint32_t *ks_regions_device_covered(const ks_regions *r) { return r ? r->d_covered : nullptr; }

extern "C" int ks_regions_copy_to_host(ks_ctx *ctx, const ks_regions *r, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                                       uint32_t *length, uint32_t *n_kmers, uint32_t *covered) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, r, row_offsets, q_start, t_start, length, n_kmers, covered); });
}

extern "C" void ks_regions_free(ks_regions *r) { ks_obj_free(r); }
