// ks_matchpos.hip — ks_match_positions: for every hit row (qid, tid) the (query start, target start) pairs of windows that
// share a kept hash (the k-mer join of `kmerseek search --extract-kmers`, src/python/kmerseek/search.py:195-240).
//
//   1. the target table ordered by hash: (hash, seq << 32 | start) through the stable LSD radix sort (ks_radix_sort_u64)
//   2. k_mp_count   per query window the run [lo, lo + cnt) of its hash in the sorted target hashes; one-launch scan of cnt
//                   -> the number of candidate pairs is known (and refused, KS_ERR_CAPACITY) before any pair array exists
//   3. k_mp_expand  balanced by OUTPUT: a workgroup owns MP_TILE consecutive candidate pairs, finds the query windows they
//                   belong to in the scanned counts (staged in LDS), and writes one key per pair,
//                       hit row << (pq + pt) | query start << pt | target start        (pq / pt: bits of the longest starts);
//                   the row comes from a search of tid among the query's rows of the hits.  A pair without a row (thresholded
//                   search) or with a row of another slice carries the row value one past the slice: the sort takes it to the end
//   4. the keys sorted on their live bits (ks_sort_pairs_msd, LSD passes for short lists)
//   5. k_mp_rows    row boundaries -> row_offsets, keys -> q_start / t_start, per row the four extents
// Row index and starts that do not fit 64 bits together: the hit rows are cut into slices, each with a key of its own
// (rows are independent; steps 3 - 5 run per slice, a device-side running total places every slice behind its predecessor).
#include "ks_device.h"

#define MP_THREADS 256
#define MP_IPT 4
#define MP_TILE (MP_THREADS * MP_IPT)
#define MP_STAGE 4096 // query windows of a tile whose scanned counts are staged in LDS (16 KB); more: searched in memory
#define MP_NONE 0xffffffffu

// targets: (seq, start) as the value column of the hash sort + the longest start
__global__ __launch_bounds__(256) void k_mp_pack(const u32 *seq, const u32 *start, u32 n, u64 *val, u32 *max_start) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    u32 s = 0;
    if (i < n) { s = start[i]; val[i] = ((u64)seq[i] << 32) | s; }
    s = ks_wave_max_u32(s);
    if ((threadIdx.x & 63) == 0 && s) atomicMax(max_start, s);
}

// Per query window: lo = sorted target hashes below its hash, cnt = those equal to it.  Both bounds advance in one loop of
// ceil(log2(n_t + 1)) steps: the two loads of a step are requested together, and every lane of a wave takes the same steps.
__global__ __launch_bounds__(256) void k_mp_count(const u64 *q_hash, const u32 *q_start, u32 n_q, const u64 *t_sorted, u32 n_t, u32 top_step,
                                                   u32 *lo, u32 *cnt, u32 *max_start) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    u32 s = 0;
    if (i < n_q) {
        const u64 h = q_hash[i];
        s = q_start[i];
        u32 a = 0, b = 0;
        for (u32 step = top_step; step; step >>= 1) {
            const u32 ia = a + step, ib = b + step; // (a, b <= n_t < 2^32 - 1 and step <= 2^31: a wrapped sum fails the range test)
            const bool in_a = ia <= n_t && ia > a, in_b = ib <= n_t && ib > b;
            const u64 ka = in_a ? t_sorted[ia - 1] : 0, kb = in_b ? t_sorted[ib - 1] : 0;
            if (in_a && ka < h) a = ia;
            if (in_b && kb <= h) b = ib;
        }
        lo[i] = a;
        cnt[i] = b - a;
    }
    s = ks_wave_max_u32(s);
    if ((threadIdx.x & 63) == 0 && s) atomicMax(max_start, s);
}

// row_begin[q] = first hit row whose qid is >= q, q = 0 .. n_qseqs (rows are ordered by (qid, tid))
__global__ __launch_bounds__(256) void k_mp_row_begin(const u32 *qid, u32 n_rows, u32 n_qseqs, u32 *row_begin) {
    const u32 q = blockIdx.x * 256 + threadIdx.x;
    if (q > n_qseqs) return;
    row_begin[q] = ks_query_row_begin(qid, n_rows, q);
}

typedef ks_slice_fmt mp_key_fmt; // pt / pqt: bits of the target start, of both starts

// The hot kernel.  Candidate pair p belongs to the query window i with off[i] <= p < off[i + 1] and is its (p - off[i])-th
// match: target record lo[i] + (p - off[i]) of the hash-sorted table.  Windows without a match have off[i] == off[i + 1] and
// are never found.  A tile's windows are [w_first, w_last]; their offsets relative to the tile go to LDS when they fit.
__global__ __launch_bounds__(MP_THREADS) void k_mp_expand(const u64 *off, u32 n_q, const u32 *lo, const u32 *q_seq, const u32 *q_start,
                                                          const u64 *t_val, const u32 *row_begin, const u32 *h_tid, mp_key_fmt F, u64 n_cand,
                                                          u64 *keys) {
    __shared__ u32 s_rel[MP_STAGE];
    __shared__ u32 s_w[2];
    const u32 tid = threadIdx.x;
    const u64 begin = (u64)blockIdx.x * MP_TILE;
    const u64 end = begin + MP_TILE < n_cand ? begin + MP_TILE : n_cand;
    if (tid < 2) s_w[tid] = ks_last_le_u64(off, 0, n_q - 1, tid == 0 ? begin : end - 1); // (off[0] == 0 <= p)
    __syncthreads();
    const u32 w_first = s_w[0], w_last = s_w[1], span = w_last - w_first + 1;
    const bool staged = span <= MP_STAGE;
    const u64 off_first = off[w_first];
    if (staged) { // every window after the first starts inside the tile: its offset relative to `begin` is < MP_TILE
        for (u32 k = tid; k < span; k += MP_THREADS) s_rel[k] = k ? (u32)(off[w_first + k] - begin) : 0u;
        __syncthreads();
    }
    u32 w[MP_IPT], j[MP_IPT];
    bool live[MP_IPT];
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) {
        const u32 rel = (u32)it * MP_THREADS + tid;
        const u64 p = begin + rel;
        live[it] = p < end;
        w[it] = w_first; j[it] = 0;
        if (!live[it]) continue;
        if (staged) {
            const u32 a = ks_last_le_u32(s_rel, span, rel);
            w[it] = w_first + a;
            j[it] = a ? rel - s_rel[a] : (u32)(p - off_first);
        } else {
            w[it] = ks_last_le_u64(off, w_first, w_last, p);
            j[it] = (u32)(p - off[w[it]]);
        }
    }
    // the window's columns, then the target record and the query's row range: each round of loads is requested for all items first
    u32 qs[MP_IPT], qq[MP_IPT], tl[MP_IPT];
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) { qs[it] = q_start[w[it]]; qq[it] = q_seq[w[it]]; tl[it] = lo[w[it]]; }
    u64 tv[MP_IPT];
    u32 a[MP_IPT], n[MP_IPT], re[MP_IPT], maxn = 0;
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) {
        tv[it] = live[it] ? t_val[tl[it] + j[it]] : 0;
        a[it] = row_begin[qq[it]]; re[it] = row_begin[qq[it] + 1];
    }
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) {
        n[it] = live[it] ? re[it] - a[it] : 0u;
        maxn = n[it] > maxn ? n[it] : maxn;
    }
    // lower bound of the target id among the query's rows: a window halves (at least) per step, so bits(maxn) steps end all
    for (; maxn; maxn >>= 1) {
        u32 v[MP_IPT];
#pragma unroll
        for (int it = 0; it < MP_IPT; it++) v[it] = n[it] ? h_tid[a[it] + (n[it] >> 1)] : 0u;
#pragma unroll
        for (int it = 0; it < MP_IPT; it++) {
            if (!n[it]) continue;
            const u32 half = n[it] >> 1;
            if (v[it] < (u32)(tv[it] >> 32)) { a[it] += half + 1; n[it] -= half + 1; } else n[it] = half;
        }
    }
    u32 hit[MP_IPT];
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) hit[it] = (live[it] && a[it] < re[it]) ? h_tid[a[it]] : MP_NONE;
#pragma unroll
    for (int it = 0; it < MP_IPT; it++) {
        if (!live[it]) continue;
        const u32 t_id = (u32)(tv[it] >> 32), row = a[it];
        const bool mine = a[it] < re[it] && hit[it] == t_id && row >= F.row0 && row - F.row0 < F.slice_rows;
        const u64 key = mine ? ((u64)(row - F.row0) << F.pqt) | ((u64)qs[it] << F.pt) | (u32)tv[it] : (u64)F.slice_rows << F.pqt;
        keys[begin + (u32)it * MP_THREADS + tid] = key;
    }
}

// Sorted keys of a slice -> the slice's part of the result.  Thread i looks at key i and at its predecessor (thread n_cand
// at a key one past the slice's rows: the end of the last row): a change of the row field is a row boundary.  The target-side
// extents are a segmented min / max over the wave; a row that lies inside one wave's 64 keys is written as it stands, a row
// that spans waves combines one partial per wave with atomicMin / atomicMax (t_lo / t_hi start as all-ones / 0).
// base[0]: pairs of the slices before this one; base[1] receives base[0] + this slice's pairs.
// flag: raised when the row fields do not count 0, 1, 2 ... slice_rows - 1 — a hit row without a pair.
__global__ __launch_bounds__(256) void k_mp_rows(const u64 *keys, u64 n_cand, mp_key_fmt F, u32 ksize, u64 *base, u64 *row_offsets, u32 *o_qs,
                                                 u32 *o_ts, u32 *q_lo, u32 *q_hi, u32 *t_lo, u32 *t_hi, u32 *flag, u64 *total_out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    const u64 sentinel = (u64)F.slice_rows << F.pqt, b0 = base[0];
    const u64 key = i < n_cand ? keys[i] : sentinel;
    const u32 row = (u32)(key >> F.pqt);
    const bool valid = row < F.slice_rows;
    const u32 qmask = (u32)((1ULL << (F.pqt - F.pt)) - 1ULL), tmask = (u32)((1ULL << F.pt) - 1ULL);
    const u32 qs = (u32)(key >> F.pt) & qmask, ts = (u32)key & tmask;
    // predecessor (none before key 0) and, for the wave's last lane, the successor
    u64 pkey = (u64)__shfl_up((long long)key, 1);
    if (lane == 0) pkey = (i > 0 && i <= n_cand) ? keys[i - 1] : sentinel;
    const u32 prow = i == 0 ? MP_NONE : (u32)(pkey >> F.pqt);
    const bool head = i <= n_cand && row != prow;
    u32 nrow = F.slice_rows;
    if (lane == 63 && valid && i + 1 < n_cand) nrow = (u32)(keys[i + 1] >> F.pqt);
    if (head) {
        if (prow + 1u != row) *flag = 1u; // (MP_NONE + 1 == 0: the first key must open row 0)
        if (valid) { row_offsets[F.row0 + row] = b0 + i; q_lo[F.row0 + row] = qs; }
        else { base[1] = b0 + i; if (total_out) *total_out = b0 + i; }
        if (prow != MP_NONE && prow < F.slice_rows) q_hi[F.row0 + prow] = ((u32)(pkey >> F.pt) & qmask) + ksize; // pairs are ordered by query start
    }
    if (valid) { o_qs[b0 + i] = qs; o_ts[b0 + i] = ts; }
    // segments of equal rows inside the wave
    const u64 genuine = __ballot(head), heads = genuine | 1ULL;
    const u64 upto = lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL);
    const u32 hl = 63u - (u32)__clzll((long long)(heads & upto));
    u32 mn = valid ? ts : MP_NONE, mx = valid ? ts : 0u;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const u32 om = (u32)__shfl_up((int)mn, d), ox = (u32)__shfl_up((int)mx, d);
        if (lane >= hl + d) { mn = om < mn ? om : mn; mx = ox > mx ? ox : mx; }
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ULL);
    if (valid && tail) {
        const bool whole = ((genuine >> hl) & 1ULL) && (lane < 63 || nrow != row);
        if (whole) { t_lo[F.row0 + row] = mn; t_hi[F.row0 + row] = mx + ksize; }
        else { atomicMin(&t_lo[F.row0 + row], mn); atomicMax(&t_hi[F.row0 + row], mx + ksize); }
    }
}

int ks_key_bits(u64 v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; }

int ks_sort_live_keys(ks_ctx *ctx, u64 *ka, u64 *kb, u64 n, int nbits, u64 **sorted) {
    int msd = 0;
    KS_TRY(ks_sort_pairs_msd(ctx, ka, kb, n, 0, nbits, &msd));
    if (msd) { *sorted = ka; return KS_OK; }
    int shifts[8], ns = 0;
    for (int sh = 0; sh < nbits; sh += 8) shifts[ns++] = sh;
    return ks_radix_sort_keys(ctx, KS_SORT_PAIRS, ka, ka, kb, n, shifts, ns, sorted);
}

int ks_row_slices_plan(ks_ctx *ctx, int dbg_id, const char *what, int low_bits, u64 n_rows, ks_row_slices *out) {
    int row_bits = 64 - low_bits;
    if (row_bits > 31) row_bits = 31;
    if (const char *f = ks_dbg(ctx, dbg_id)) { // (tests: small inputs take the slice path)
        const int v = atoi(f);
        if (v >= 1 && v < row_bits) row_bits = v;
    }
    if (row_bits < 1) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: the pair fields take %d key bits and leave none for a row", what, low_bits);
    out->low_bits = low_bits;
    out->per_slice = ((1ULL << row_bits) - 1ULL) < n_rows ? ((1ULL << row_bits) - 1ULL) : n_rows;
    out->n_slices = (n_rows + out->per_slice - 1) / out->per_slice;
    return KS_OK;
}

static int mp_run(ks_ctx *ctx, const ks_kmerpos *Q, const ks_kmerpos *T, const ks_hits *H, u64 max_pairs, ks_matchpos *M) {
    const u64 n_rows = H->n_hits;
    M->n_rows = n_rows; M->n_pairs = 0; M->n_slices = 0;
    KS_TRY(ks_alloc(ctx, &M->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_alloc(ctx, &M->d_qlo, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &M->d_qhi, (size_t)n_rows));
    KS_TRY(ks_alloc(ctx, &M->d_tlo, (size_t)n_rows)); KS_TRY(ks_alloc(ctx, &M->d_thi, (size_t)n_rows));
    if (n_rows == 0) { // no rows: no pairs, whatever the tables hold
        KS_TRY(ks_alloc(ctx, &M->d_qstart, 1)); KS_TRY(ks_alloc(ctx, &M->d_tstart, 1));
        KS_HIP(ctx, hipMemsetAsync(M->d_row_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    if (Q->n >= 0xfffffffeULL || T->n >= 0xfffffffeULL || n_rows >= 0xfffffffeULL)
        return ks_fail(ctx, KS_ERR_CAPACITY, "match positions: a table of 2^32 or more records");
    const u32 n_q = (u32)Q->n, n_t = (u32)T->n;
    if (n_q == 0 || n_t == 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "match positions: %llu hit rows, but a k-mer table is empty: the inputs do not belong together",
                       (unsigned long long)n_rows);

    ks_scratch sc(ctx);
    u32 *ctl = nullptr; // [0] longest query start, [1] longest target start, [2] row-gap flag
    KS_TRY(sc.alloc(&ctl, 4));
    KS_HIP(ctx, hipMemsetAsync(ctl, 0, 4 * sizeof(u32), ctx->stream));

    // 1. targets by hash
    u64 *tv0 = nullptr, *ka = nullptr, *va = nullptr, *kb = nullptr, *vb = nullptr, *t_hash = nullptr, *t_val = nullptr;
    KS_TRY(sc.alloc(&tv0, n_t)); KS_TRY(sc.alloc(&ka, n_t)); KS_TRY(sc.alloc(&va, n_t)); KS_TRY(sc.alloc(&kb, n_t)); KS_TRY(sc.alloc(&vb, n_t));
    KS_LAUNCH(ctx, "matchpos_pack", k_mp_pack, (n_t + 255) / 256, 256, (const u32 *)T->d_seq, (const u32 *)T->d_start, n_t, tv0, ctl + 1);
    {
        int shifts[8], ns = 0;
        const int hbits = ks_key_bits(ks_max_hash(T->params.scaled));
        for (int sh = 0; sh < hbits; sh += 8) shifts[ns++] = sh;
        KS_TRY(ks_radix_sort_u64(ctx, KS_SORT_INDEX, T->d_hash, tv0, ka, va, kb, vb, n_t, shifts, ns, &t_hash, &t_val));
    }
    // 2. runs per query window, scanned
    u32 *lo = nullptr, *cnt = nullptr;
    u64 *off = nullptr;
    KS_TRY(sc.alloc(&lo, n_q)); KS_TRY(sc.alloc(&cnt, n_q)); KS_TRY(sc.alloc(&off, (size_t)n_q + 1));
    u32 top_step = 1;
    while (top_step < 0x80000000u && (top_step << 1) <= n_t) top_step <<= 1;
    KS_LAUNCH(ctx, "matchpos_count", k_mp_count, (n_q + 255) / 256, 256, (const u64 *)Q->d_hash, (const u32 *)Q->d_start, n_q, (const u64 *)t_hash,
              n_t, top_step, lo, cnt, ctl);
    KS_TRY(ks_scan_u32_to_u64_wide(ctx, cnt, off, n_q)); // (candidate pairs, counted before the limit below is held against them)
    u64 *const rb = ctx->h_pin + KS_PIN_READ; // candidate pairs | longest starts
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ks_fetch_words(off + n_q, rb, 2), ks_fetch_words(ctl, rb + 1, 2)}));
    const u64 n_cand = rb[0];
    const u32 max_qs = ((const u32 *)(rb + 1))[0], max_ts = ((const u32 *)(rb + 1))[1];
    // the sort's scratch goes back; the value column of the sorted table stays (the passes end in one of the pairs, or — one
    // record — in the input itself)
    sc.free(cnt);
    if (t_val != tv0) sc.free(tv0);
    if (t_val != va) { sc.free(ka); sc.free(va); }
    if (t_val != vb) { sc.free(kb); sc.free(vb); }
    if (t_val == va) sc.free(ka);
    if (t_val == vb) sc.free(kb);

    // the limit: the caller's, or what one sort (32-bit offsets) and the device memory take: 8 bytes of key twice + 8 of output
    u64 limit = max_pairs;
    if (!limit) {
        size_t mem_free = 0, mem_total = 0;
        KS_HIP(ctx, hipMemGetInfo(&mem_free, &mem_total));
        u64 idle = 0;
        for (const auto &b : ctx->pool) if (!b.in_use) idle += b.size;
        limit = (mem_free + idle) / 32; // (24 bytes per pair, and the pool's size classes round up by up to a quarter)
        if (ctx->pool_cap) limit = ctx->pool_cap / 32;
        if (limit > 0xfffffff0ULL) limit = 0xfffffff0ULL;
    }
    if (n_cand > limit)
        return ks_fail(ctx, KS_ERR_CAPACITY, "match positions: the join yields %llu pairs, the limit is %llu%s", (unsigned long long)n_cand,
                       (unsigned long long)limit, max_pairs ? " (max_pairs)" : "");
    if (n_cand >= 0xfffffff0ULL) return ks_fail(ctx, KS_ERR_CAPACITY, "match positions: %llu pairs exceed one sort", (unsigned long long)n_cand);
    if (n_cand == 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "match positions: %llu hit rows, but the tables share no hash: the inputs do not belong together",
                       (unsigned long long)n_rows);

    // the key: row | query start | target start
    const int pq = ks_key_bits(max_qs), pt = ks_key_bits(max_ts);
    M->max_qs = max_qs; M->max_ts = max_ts;
    ks_row_slices SL;
    KS_TRY(ks_row_slices_plan(ctx, KS_DBG_MATCHPOS_ROW_BITS, "match positions", pq + pt, n_rows, &SL));
    const u64 n_slices = SL.n_slices;
    M->n_slices = (u32)n_slices;

    u32 *row_begin = nullptr;
    u64 *k0 = nullptr, *k1 = nullptr, *base = nullptr;
    KS_TRY(sc.alloc(&row_begin, (size_t)Q->n_seqs + 1));
    KS_TRY(sc.alloc(&k0, (size_t)n_cand)); KS_TRY(sc.alloc(&k1, (size_t)n_cand));
    KS_TRY(sc.alloc(&base, (size_t)n_slices + 2)); // running pair total per slice; the last word: the total
    KS_TRY(ks_alloc(ctx, &M->d_qstart, (size_t)n_cand)); KS_TRY(ks_alloc(ctx, &M->d_tstart, (size_t)n_cand));
    KS_HIP(ctx, hipMemsetAsync(base, 0, ((size_t)n_slices + 2) * sizeof(u64), ctx->stream));
    KS_HIP(ctx, hipMemsetAsync(M->d_tlo, 0xff, (size_t)n_rows * sizeof(u32), ctx->stream));
    KS_HIP(ctx, hipMemsetAsync(M->d_thi, 0, (size_t)n_rows * sizeof(u32), ctx->stream));
    KS_LAUNCH(ctx, "matchpos_row_begin", k_mp_row_begin, (Q->n_seqs + 256) / 256, 256, (const u32 *)H->d_qid, (u32)n_rows, Q->n_seqs, row_begin);
    const u32 g_expand = (u32)((n_cand + MP_TILE - 1) / MP_TILE), g_rows = (u32)((n_cand + 1 + 255) / 256);
    for (u64 s = 0; s < n_slices; s++) {
        const mp_key_fmt F = SL.fmt(s, n_rows, pt);
        KS_LAUNCH(ctx, "matchpos_expand", k_mp_expand, g_expand, MP_THREADS, (const u64 *)off, n_q, (const u32 *)lo, (const u32 *)Q->d_seq,
                  (const u32 *)Q->d_start, (const u64 *)t_val, (const u32 *)row_begin, (const u32 *)H->d_tid, F, n_cand, k0);
        u64 *sorted = nullptr;
        KS_TRY(ks_sort_live_keys(ctx, k0, k1, n_cand, F.pqt + ks_key_bits(F.slice_rows), &sorted));
        KS_LAUNCH(ctx, "matchpos_rows", k_mp_rows, g_rows, 256, (const u64 *)sorted, n_cand, F, Q->params.ksize, base + s, M->d_row_offsets,
                  M->d_qstart, M->d_tstart, M->d_qlo, M->d_qhi, M->d_tlo, M->d_thi, ctl + 2,
                  s + 1 == n_slices ? M->d_row_offsets + n_rows : (u64 *)nullptr);
    }
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ks_fetch_words(base + n_slices, rb, 2), ks_fetch_words(ctl + 2, rb + 1, 1)}));
    if (*(const u32 *)(rb + 1) != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "match positions: a hit row shares no k-mer in the tables: hits and tables do not belong together");
    M->n_pairs = rb[0];
    return KS_OK;
}

extern "C" int ks_match_positions(ks_ctx *ctx, const ks_kmerpos *q_pos, const ks_kmerpos *t_pos, const ks_hits *hits,
                                  const ks_matchpos_opts *opts, ks_matchpos **out) {
    return ks_guard(ctx, [&]() -> int {
    if (opts) KS_TRY(ks_opts_words_check(ctx, "match position", opts->flags, 0, opts->reserved));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!q_pos || !t_pos || !hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    KS_TRY(ks_inputs_check_ctx(ctx, "match positions", q_pos, t_pos, hits));
    KS_TRY(ks_params_check_same(ctx, "match positions", "the tables", q_pos->params, t_pos->params));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_matchpos> M(ctx, out, ks_matchpos_free);
    M->params = q_pos->params;
    KS_TRY(mp_run(ctx, q_pos, t_pos, hits, opts ? opts->max_pairs : 0, M));
    return M.commit();
    });
}

extern "C" uint64_t ks_matchpos_n_rows(const ks_matchpos *m) { return m ? m->n_rows : 0; }
extern "C" uint64_t ks_matchpos_n_pairs(const ks_matchpos *m) { return m ? m->n_pairs : 0; }
extern "C" uint32_t ks_matchpos_n_slices(const ks_matchpos *m) { return m ? m->n_slices : 0; }
extern "C" const uint64_t *ks_matchpos_device_row_offsets(const ks_matchpos *m) { return m ? m->d_row_offsets : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_q_start(const ks_matchpos *m) { return m ? m->d_qstart : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_t_start(const ks_matchpos *m) { return m ? m->d_tstart : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_q_lo(const ks_matchpos *m) { return m ? m->d_qlo : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_q_hi(const ks_matchpos *m) { return m ? m->d_qhi : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_t_lo(const ks_matchpos *m) { return m ? m->d_tlo : nullptr; }
extern "C" const uint32_t *ks_matchpos_device_t_hi(const ks_matchpos *m) { return m ? m->d_thi : nullptr; }

extern "C" int ks_matchpos_copy_to_host(ks_ctx *ctx, const ks_matchpos *m, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                                        uint32_t *q_lo, uint32_t *q_hi, uint32_t *t_lo, uint32_t *t_hi) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, m, row_offsets, q_start, t_start, q_lo, q_hi, t_lo, t_hi); });
}

extern "C" void ks_matchpos_free(ks_matchpos *m) { ks_obj_free(m); }
