// ks_best.hip — ks_hits_best: the k best rows of every query of a hit list (BLAST's max_target_seqs), by a rank key.
//
// Hit rows are ordered by (qid, tid), so a query's rows are one contiguous segment and row order inside it is tid order.
//   keys     one pass over the rows (a lane per row): the row's f64 score -> a u64 whose unsigned order is the contract's order
//            (bh_sortable: NaN lowest and canonical, -0.0 = +0.0), ids and sketch sizes checked on the way.  The lane of a
//            segment's first row finds its end (ks_query_row_begin from there) and lists the segment for one of:
//   wave     segments of up to BH_WAVE_MAX rows, a wave each: every lane holds one row's key and counts the rows that beat it while
//            the keys go round through v_readlane — the count IS the rank, no LDS, no sort;
//   wg       longer segments, a workgroup each: MSD radix select of the k-th best key (8-bit histograms in LDS, at most 8 passes;
//            a segment of up to BH_CHUNK rows is staged in LDS once, a longer one is streamed from memory — L2 — once per pass),
//            then one sweep in row order keeps the rows above the threshold and, of those equal to it, the first `quota` in row
//            order (= the smallest tids), then the kept rows are ranked among themselves by counting (every row that beats a
//            kept row is kept itself, so this is the rank inside the whole segment), BH_CHUNK opponents in LDS at a time;
//   move     ks_hits_select_tail (ks_hits.hip): keep flags -> one-launch exclusive scan -> one scatter of all columns (rf_move) + rank + src_row.
// Every comparison is on (u64 key, row index): integers.  No f64 atomics, no reductions of scores: a row's rank and whether it
// is kept do not depend on the path its segment took (KS_DEBUG_BEST_PATH = 1 every segment by a wave, 2 by a workgroup,
// 3 by a workgroup with a chunk of BH_CHUNK_SMALL rows — the tests reach the streamed case with a few hundred rows).
#include "ks_score.h" // bh_set, bh_size, bh_row_score: the scores, shared with ks_cluster.hip

#define BH_WAVE_MAX 64     // rows of a segment one wave holds in registers: the longest segment of the wave path
#define BH_CHUNK 1024      // keys of the workgroup path's LDS chunk (8 KB)
#define BH_CHUNK_SMALL 64  // ... under KS_DEBUG_BEST_PATH = 3
#define BH_WAVE_GRID 1024  // workgroups of k_best_wave (4 waves each, striding over the listed segments)
#define BH_WG_GRID 2048    // workgroups of k_best_wg (striding likewise)
#define BH_NONE KS_RANK_NONE // rank of a row that is not kept
enum { BH_BAD_ID = 0, BH_BAD_SIZE = 1, BH_KEPT = 2 }; // words of the control block

// a u64 that orders as the contract orders scores: NaN (every NaN) lowest, then -inf ... -0.0 = +0.0 ... +inf
KS_DEV u64 bh_sortable(double s) {
    if (s != s) return 0;
    u64 b = (u64)__double_as_longlong(s);
    if (s == 0.0) b = 0; // -0.0
    return (b >> 63) ? ~b : (b | (1ULL << 63));
}

struct bh_in {
    const u32 *qid, *tid, *isect;
    const double *score;
    u32 n_rows, rank_by, k;
    bh_set q, t;
};

// mode: 0 by length, 1 every segment to the wave kernel, 2 every segment to the workgroup kernel
__global__ __launch_bounds__(256) void k_best_keys(bh_in R, int mode, u32 seg_cap, u64 *key, u32 *flags, u32 *rank, u32 *wave_segs, u32 *wg_segs,
                                                   unsigned long long *bad) {
#pragma clang fp contract(off)
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R.n_rows) return;
    const u32 q = R.qid[r], t = R.tid[r];
    u64 kx = 0;
    if ((R.q.off && q >= R.q.n) || (R.t.off && t >= R.t.n)) ks_first_bad(bad, BH_BAD_ID, r);
    else {
        bool bad_size;
        const double s = bh_row_score(R.rank_by, r, q, t, R.isect[r], R.q, R.t, R.score, &bad_size);
        if (bad_size) ks_first_bad(bad, BH_BAD_SIZE, r);
        kx = bh_sortable(s);
    }
    key[r] = kx;
    if (r != 0 && R.qid[r - 1] == q) return;
    // the first row of a segment: where it ends, and which kernel takes it
    const u32 len = ks_seg_len(R.qid, R.n_rows, r, q);
    if (mode == 1 || (mode == 0 && len <= BH_WAVE_MAX)) {
        if (mode == 0 && len == 1) { flags[r] = 1u; rank[r] = 0u; } // (k >= 1)
        else ks_seg_list_push(wave_segs, seg_cap, r, len);
    } else ks_seg_list_push(wg_segs, seg_cap, r, len);
}

// `o` at row index oi beats `s` at row index si
KS_DEV u32 bh_beats(u64 o, u32 oi, u64 s, u32 si) { return (o > s || (o == s && oi < si)) ? 1u : 0u; }

// A wave per listed segment.  64 rows ("subjects") sit one per lane; the segment's keys ("opponents") pass by 64 at a time, read
// lane by lane through v_readlane (a scalar broadcast: no LDS, no ds_bpermute).  A segment of the by-length split is one round
// of at most 64 steps; a longer one (KS_DEBUG_BEST_PATH = 1) takes ceil(len / 64)^2 rounds.
__global__ __launch_bounds__(256) void k_best_wave(const u64 *key, const u32 *segs, u32 seg_cap, u32 k, u32 *flags, u32 *rank) {
    const u32 lane = threadIdx.x & 63;
    for (ks_seg_walk seg = ks_seg_list_by_wave(segs, seg_cap); seg.next();) {
        const u32 b = seg.b, len = seg.len;
        for (u32 sc = 0; sc < len; sc += 64) {
            const u32 si = sc + lane;
            const u64 skey = si < len ? key[b + si] : 0;
            u32 cnt = 0;
            for (u32 oc = 0; oc < len; oc += 64) {
                const u64 okey = oc + lane < len ? key[b + oc + lane] : 0;
                const u32 nv = len - oc < 64u ? len - oc : 64u;
                for (u32 j = 0; j < nv; j++) {
                    const u64 o = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(okey >> 32), (int)j) << 32) |
                                  (u32)__builtin_amdgcn_readlane((int)(u32)okey, (int)j);
                    cnt += bh_beats(o, oc + j, skey, si);
                }
            }
            if (si < len) {
                const bool keep = cnt < k;
                flags[b + si] = keep ? 1u : 0u;
                rank[b + si] = keep ? cnt : BH_NONE;
            }
        }
    }
}

// A workgroup per listed segment; chunk <= BH_CHUNK.  kept_rows[b, b + kept): the segment's kept rows (relative), in row order.
__global__ __launch_bounds__(256) void k_best_wg(const u64 *key, const u32 *segs, u32 seg_cap, u32 k, u32 chunk, u32 *flags, u32 *rank,
                                                 u32 *kept_rows) {
    __shared__ u64 s_keys[BH_CHUNK];
    __shared__ u32 s_hist[256];
    __shared__ u32 s_scan[8];
    __shared__ u32 s_sel[3];
    const u32 t = threadIdx.x;
    for (ks_seg_walk seg = ks_seg_list_by_wg(segs, seg_cap); seg.next();) {
        const u32 b = seg.b, len = seg.len;
        const u32 kk = k < len ? k : len; // rows kept
        const bool staged = len <= chunk;
        __syncthreads(); // (the previous segment's last readers of s_keys)
        if (staged)
            for (u32 i = t; i < len; i += 256) s_keys[i] = key[b + i];
        // Radix select, most significant byte first.  Invariant: the rows whose key agrees with P above bit `shift + 8` form the
        // class that holds the kk-th best key, `quota` of the class are kept, every row above the class is kept.  A pass picks the
        // byte value d of the class's quota-th best key: bins above d are kept outright.  It ends early when the whole class is kept.
        u64 P = 0;
        u32 shift = 0, quota = kk;
        if (kk < len) {
            for (u32 pass = 0; pass < 8; pass++) {
                shift = 56 - 8 * pass;
                s_hist[t] = 0;
                __syncthreads();
                for (u32 i = t; i < len; i += 256) {
                    const u64 kx = staged ? s_keys[i] : key[b + i];
                    if (pass == 0 || (kx >> (shift + 8)) == (P >> (shift + 8))) atomicAdd(&s_hist[(u32)(kx >> shift) & 255u], 1u);
                }
                __syncthreads();
                const u32 h = s_hist[255 - t]; // thread t: bin 255 - t, so that the scan counts the bins above it
                u32 total;
                const u32 above = ks_block_excl_scan(h, s_scan, &total);
                if (above < quota && quota <= above + h) { s_sel[0] = 255 - t; s_sel[1] = above; s_sel[2] = h; }
                __syncthreads();
                P |= (u64)s_sel[0] << shift;
                quota -= s_sel[1];
                if (s_sel[2] == quota) break; // (uniform)
            }
        }
        // keep: above the class, or one of its first `quota` rows in row order (the smallest tids)
        const u64 ptop = P >> shift;
        u32 gt_base = 0, eq_base = 0;
        for (u32 base = 0; base < len; base += 256) {
            const u32 i = base + t;
            const bool live = i < len;
            const u64 top = (live ? (staged ? s_keys[i] : key[b + i]) : 0) >> shift;
            const bool gt = live && top > ptop, eq = live && top == ptop;
            u32 total;
            const u32 ex = ks_block_excl_scan((gt ? 0x10000u : 0u) | (eq ? 1u : 0u), s_scan, &total);
            const u32 gt_before = gt_base + (ex >> 16), eq_before = eq_base + (ex & 0xffffu);
            const bool keep = gt || (eq && eq_before < quota);
            if (live) {
                flags[b + i] = keep ? 1u : 0u;
                const u32 pos = gt_before + (eq_before < quota ? eq_before : quota);
                if (keep && pos < len) kept_rows[b + pos] = i; // (pos < kk: the guard costs nothing and keeps a broken invariant in bounds)
                else if (!keep) rank[b + i] = BH_NONE;
            }
            gt_base += total >> 16;
            eq_base += total & 0xffffu;
        }
        // rank of a kept row = the kept rows that beat it (position in kept_rows orders as the row index does)
        for (u32 oc = 0; oc < kk; oc += chunk) {
            const u32 nc = kk - oc < chunk ? kk - oc : chunk;
            __syncthreads(); // (kept_rows is written; the readers of s_keys are done)
            for (u32 j = t; j < nc; j += 256) { const u32 row = kept_rows[b + oc + j]; s_keys[j] = key[b + (row < len ? row : 0u)]; }
            __syncthreads();
            for (u32 si = t; si < kk; si += 256) {
                const u32 row_ = kept_rows[b + si], row = row_ < len ? row_ : 0u;
                const u64 skey = key[b + row];
                u32 cnt = 0;
                for (u32 j = 0; j < nc; j++) cnt += bh_beats(s_keys[j], oc + j, skey, si);
                rank[b + row] = oc ? rank[b + row] + cnt : cnt;
            }
        }
    }
}

static int best_run(ks_ctx *ctx, const ks_hits *H, const ks_sketches *Q, const ks_sketches *T, const double *d_score, const ks_best_opts *o,
                    ks_hits *B) {
    u32 n;
    u64 cap; // every query keeps at most k
    KS_TRY(ks_hits_select_plan(ctx, "best hits", H, Q, o->k, &n, &cap));
    KS_TRY(B->alloc(ctx, (size_t)cap, B->has_stats, KS_COLS_RANKED));
    if (n == 0) return KS_OK;

    bool small; // (tests: every segment one way; 3 = the workgroup path with a small chunk)
    const int mode = ks_seg_path_knob(ctx, KS_DBG_BEST_PATH, &small);
    const u32 chunk = small ? BH_CHUNK_SMALL : BH_CHUNK;
    const u32 seg_cap = Q && Q->n_seqs < n ? Q->n_seqs : n; // segments there can be
    ks_scratch sc(ctx);
    u64 *key = nullptr;
    u32 *flags = nullptr, *rank = nullptr, *kept_rows = nullptr, *wave_segs = nullptr, *wg_segs = nullptr;
    ks_ctl ctl; // [BH_BAD_ID], [BH_BAD_SIZE]: the first such row; [BH_KEPT]: the scan's total
    KS_TRY(sc.alloc(&key, (size_t)n)); KS_TRY(sc.alloc(&flags, (size_t)n)); KS_TRY(sc.alloc(&rank, (size_t)n));
    KS_TRY(sc.alloc(&kept_rows, (size_t)n));
    KS_TRY(ks_seg_list_alloc(ctx, sc, seg_cap, &wave_segs)); KS_TRY(ks_seg_list_alloc(ctx, sc, seg_cap, &wg_segs));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_BEST, 2, 1));

    const bh_in R = {H->d_qid, H->d_tid, H->d_isect, d_score, n, o->rank_by, o->k, bh_set_of(Q), bh_set_of(T)};
    const u32 g = (n + 255) / 256;
    KS_LAUNCH(ctx, "best_keys", k_best_keys, g, 256, R, mode, seg_cap, key, flags, rank, wave_segs, wg_segs, ctl.words());
    if (mode != 2)
        KS_LAUNCH(ctx, "best_wave", k_best_wave, BH_WAVE_GRID, 256, (const u64 *)key, (const u32 *)wave_segs, seg_cap, o->k, flags, rank);
    if (mode != 1)
        KS_LAUNCH(ctx, "best_wg", k_best_wg, BH_WG_GRID, 256, (const u64 *)key, (const u32 *)wg_segs, seg_cap, o->k, chunk, flags, rank, kept_rows);
    return ks_hits_select_tail(ctx, "best hits", H, n, flags, rank, cap, nullptr, ctl, BH_KEPT, [&]() -> int {
        if (ctl.bad(BH_BAD_ID))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "best hits: hit row %llu names a query or target beyond the sketch sets",
                           (unsigned long long)ctl[BH_BAD_ID]);
        if (ctl.bad(BH_BAD_SIZE))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "best hits: hit row %llu names an empty sketch: its score divides by 0",
                           (unsigned long long)ctl[BH_BAD_SIZE]);
        return KS_OK;
    }, B);
}

// the option words and what they ask of the other arguments; ctx may be NULL
static int best_opts_check(ks_ctx *ctx, const ks_best_opts *o, const ks_sketches *queries, const ks_sketches *targets, const double *d_score) {
    const auto bad = [&](const char *why) { return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "best hits options: %s", why) : KS_ERR_INVALID_ARG; };
    if (!o) return bad("NULL");
    KS_TRY(ks_opts_words_check(ctx, "best hits", o->flags, 0, o->reserved));
    if (o->k == 0) return bad("k must be >= 1");
    if (o->rank_by > KS_BEST_SCORE) return bad("unknown rank_by");
    if (o->rank_by == KS_BEST_SCORE && !d_score) return bad("KS_BEST_SCORE needs a score column");
    if (o->rank_by != KS_BEST_SCORE && d_score) return bad("a score column is only read with KS_BEST_SCORE");
    const bool need_t = o->rank_by == KS_BEST_TARGET_CONTAINMENT || o->rank_by == KS_BEST_MAX_CONTAINMENT || o->rank_by == KS_BEST_JACCARD;
    const bool need_q = o->rank_by == KS_BEST_MAX_CONTAINMENT || o->rank_by == KS_BEST_JACCARD;
    if (need_t && !targets) return bad("this rank key needs the target sketches");
    if (need_q && !queries) return bad("this rank key needs the query sketches");
    return KS_OK;
}

extern "C" int ks_hits_best(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *queries, const ks_sketches *targets, const double *d_score,
                            const ks_best_opts *opts, ks_hits **out) {
    return ks_guard(ctx, [&]() -> int {
    if (out) *out = nullptr;
    KS_TRY(best_opts_check(ctx, opts, queries, targets, d_score));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "best hits", hits, queries, targets));
    if (queries && targets) KS_TRY(ks_params_check_same(ctx, "best hits", "the sketch sets", queries->params, targets->params));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_hits> B(ctx, out, ks_hits_free);
    ks_hits_inherit(B, hits);
    KS_TRY(best_run(ctx, hits, queries, targets, d_score, opts, B));
    return B.commit();
    });
}
