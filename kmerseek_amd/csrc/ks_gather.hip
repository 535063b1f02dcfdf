// ks_gather.hip — ks_hits_gather: per query the shortest greedy list of targets that together explain its hashes (the `gather` /
// `fastmultigather` step of the sourmash / branchwater tools): round after round the row that covers the most still uncovered
// hashes of the query is kept and its hashes are taken out; ties go to the smaller tid.  Integers only.
//
// Hit rows are ordered by (qid, tid), so a query's rows are one contiguous segment (as in ks_best.hip).
//   incidence  an exclusive scan of the intersect column gives every row its slice of one u32 array; one pass over the rows (a lane
//              per short row, a wave per row with |q| + |t| above GA_CUT: ks_shared_walk_lane / _wave, as in ks_signif.hip)
//              writes the positions INSIDE q's sketch of the hashes the row shares with its target, ascending.  The
//              pass counts what it writes: another count than the row's intersect means hits and sketches do not belong together.
//              A row never writes outside its slice, and a row whose list is not whole starts dead (count 0): the rounds only
//              ever read lists that are complete.  The lane of a segment's first row lists the segment for one of:
//   wave       segments of up to GA_WAVE_MAX rows whose query has at most GA_WAVE_BITS hashes, a wave each: the live bitmap over
//              q's positions sits in the wave's share of LDS, a lane per row recounts its list against it, the argmax of the u64
//              key (count << 32) | ~row runs through DPP (ks_wave_max64), and the whole wave clears the winner's bits (one LDS
//              atomic per position: the bit it returns says whether the position was still live) and sums their abundances;
//   wg         every other segment, a workgroup each: the bitmap in LDS up to GA_LIVE_BITS positions, in global scratch above
//              (the streamed case: a proteome-sized union query).  A round reads the stale counts 256 at a time, recounts the
//              stale argmax first (a wave per row, 64 positions per load, popcount of a ballot), then only the rows whose stale
//              count reaches the best fresh count known — counts only fall, so a stale count is an upper bound and every
//              other row cannot win; a row whose count fell below min_unique is dead for good.  The winner is the same as with
//              every row recounted every round: the key holds the row, so the maximum is unique.
//   move       ks_hits_select_tail (ks_hits.hip): keep flags -> one-launch exclusive scan -> ks_hits_move_ranked with the three columns.
// No look-back, no spin, no dependency between workgroups: every loop is bounded by the segment's rows or a list's length.
// KS_DEBUG_GATHER_PATH = 1 every segment by a wave (where the bitmap fits GA_WAVE_BITS), 2 by a workgroup, 3 by a workgroup
// with GA_LIVE_BITS_SMALL LDS positions — the tests reach the streamed bitmap with a few hundred hashes.
#include "ks_device.h"

#define GA_CUT 128              // |q| + |t| above this: the row's incidence list is written by a wave
#define GA_ROWS_WAVE_GRID 1024  // workgroups of k_ga_rows_wave (4 waves each, striding over the listed rows)
#define GA_WAVE_MAX 64          // rows of the longest segment of the wave path
#define GA_WAVE_BITS 8192       // query hashes whose live bitmap one wave keeps in LDS (1 KB)
#define GA_LIVE_BITS 65536      // ... one workgroup keeps in LDS (8 KB); a longer query's bitmap lies in global scratch
#define GA_LIVE_BITS_SMALL 256  // ... under KS_DEBUG_GATHER_PATH = 3
#define GA_WAVE_GRID 1024       // workgroups of k_ga_wave (4 waves each, striding over the listed segments)
#define GA_WG_GRID 2048         // workgroups of k_ga_wg (striding likewise)
enum { GA_BAD_ID = 0, GA_BAD_COUNT = 1, GA_BAD_CAP = 2, GA_KEPT = 3 }; // words of the control block

struct ga_in {
    const u64 *q_off, *q_hash, *t_off, *t_hash;
    const u32 *q_abund;
    const u32 *qid, *tid, *isect;
    const u64 *off; // exclusive scan of isect: row r's list is inc[off[r], off[r] + isect[r])
    u32 *inc;
    u64 inc_cap;    // entries of inc
    u32 n_rows, n_q, n_t;
    u32 min_u, max_results; // max(min_unique, 1); 0 = no limit
    u32 *cnt;       // per row: the count of its last recount — an upper bound of its count now; 0: dead or picked
    u32 *flags, *rank, *unique, *remaining;
    u64 *weighted;
};

KS_DEV u64 ga_key(u32 count, u32 row) { return ((u64)count << 32) | (u32)~row; }
// the lanes of one wave have written LDS that its other lanes read next (the LDS operations of a wave execute in order)
KS_DEV void ga_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- incidence ---------------------------------------------------------------------------------------------------------------
// A lane per row.  mode: 0 segments by length, 1 every segment to the wave kernel (where the bitmap fits), 2 to the workgroup kernel.
__global__ __launch_bounds__(256) void k_ga_rows(ga_in G, int mode, u32 seg_cap, u32 *wave_rows, u32 *wave_segs, u32 *wg_segs,
                                                 unsigned long long *bad) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= G.n_rows) return;
    G.flags[r] = 0u; G.rank[r] = KS_RANK_NONE; G.cnt[r] = 0u;
    const u32 q = G.qid[r], t = G.tid[r];
    if (q >= G.n_q) { ks_first_bad(bad, GA_BAD_ID, r); return; }
    const u64 qb = G.q_off[q];
    const u32 nq = (u32)(G.q_off[q + 1] - qb);
    if (r == 0 || G.qid[r - 1] != q) { // the first row of a segment: where it ends, and which kernel takes it
        const u32 len = ks_seg_len(G.qid, G.n_rows, r, q);
        const bool wave = nq <= GA_WAVE_BITS && (mode == 1 || (mode == 0 && len <= GA_WAVE_MAX));
        ks_seg_list_push(wave ? wave_segs : wg_segs, seg_cap, r, len);
    }
    if (t >= G.n_t) { ks_first_bad(bad, GA_BAD_ID, r); return; }
    const u64 base = G.off[r];
    const u32 lim = G.isect[r];
    if (base > G.inc_cap || lim > G.inc_cap - base) { ks_first_bad(bad, GA_BAD_CAP, r); return; }
    const ks_run_pair P = ks_run_pair_of(G.q_off, G.q_hash, G.t_off, G.t_hash, q, t);
    if ((u64)P.nw + P.ns > GA_CUT) { ks_row_list_push(wave_rows, r); return; }
    const u32 c = ks_shared_walk_lane(P, [&](u32 pos, u32 before) { if (before < lim) G.inc[base + before] = pos; }); // (ascending)
    if (c != lim) ks_first_bad(bad, GA_BAD_COUNT, r);
    else G.cnt[r] = lim;
}

// The listed rows, a wave per row (ks_shared_walk_wave): a lane's place in the list is the shared hashes before its own.
__global__ __launch_bounds__(256) void k_ga_rows_wave(ga_in G, const u32 *wave_rows, unsigned long long *bad) {
    const u32 lane = threadIdx.x & 63;
    ks_row_list_walk(wave_rows, G.n_rows, [&](u32 r) {
        if (r >= G.n_rows) return; // (k_ga_rows lists rows below it, with ids in range and a slice inside inc)
        const ks_run_pair P = ks_run_pair_of(G.q_off, G.q_hash, G.t_off, G.t_hash, G.qid[r], G.tid[r]);
        const u64 base = G.off[r];
        const u32 lim = G.isect[r];
        const u32 c = ks_shared_walk_wave(P, lane, [&](bool found, u32 pos, u64 m, u32 before) {
            const u32 mine = before + ks_lane_lt_count(m);
            if (found && mine < lim) G.inc[base + mine] = pos;
        });
        if (lane == 0) {
            if (c != lim) ks_first_bad(bad, GA_BAD_COUNT, r);
            else G.cnt[r] = lim;
        }
    });
}

// ---- rounds: a wave per segment ------------------------------------------------------------------------------------------------
// words [0, (n + 31) / 32) of a bitmap with bits [0, n) set
KS_DEV u32 ga_full_word(u32 w, u32 n) { return (w + 1) * 32u <= n ? ~0u : ((1u << (n & 31u)) - 1u); }

// A lane per row, GA_WAVE_MAX rows per sweep (a segment of the by-length split is one sweep; KS_DEBUG_GATHER_PATH = 1 sends longer
// ones here too).  Every live row is recounted in every round: a lane's list is short, and the lanes wait for the longest anyway.
__global__ __launch_bounds__(256) void k_ga_wave(ga_in G, const u32 *segs, u32 seg_cap) {
    __shared__ u32 s_live[4][GA_WAVE_BITS / 32];
    const u32 lane = threadIdx.x & 63;
    u32 *live = s_live[threadIdx.x >> 6];
    for (ks_seg_walk seg = ks_seg_list_by_wave(segs, seg_cap); seg.next();) {
        const u32 b = seg.b, len = seg.len;
        const u32 q = ks_readfirst(G.qid[b]);
        const u64 qb = G.q_off[q];
        const u32 nq = ks_readfirst((u32)(G.q_off[q + 1] - qb)); // (<= GA_WAVE_BITS: k_ga_rows lists no other segment here)
        ga_wave_sync(); // (the previous segment's last readers)
        for (u32 i = lane; i < (nq + 31) / 32; i += 64) live[i] = ga_full_word(i, nq);
        ga_wave_sync();
        u32 rem = nq;
        for (u32 round = 0; round < len && rem != 0; round++) {
            if (G.max_results != 0 && round == G.max_results) break;
            u64 best = 0;
            for (u32 sc = 0; sc < len; sc += 64) {
                const u32 rr = sc + lane;
                u32 fresh = 0;
                if (rr < len && G.cnt[b + rr] >= G.min_u) {
                    const u32 *list = G.inc + G.off[b + rr];
                    const u32 n = G.isect[b + rr];
                    for (u32 j = 0; j < n; j++) {
                        const u32 p = list[j];
                        fresh += p < nq ? (live[p >> 5] >> (p & 31u)) & 1u : 0u;
                    }
                    G.cnt[b + rr] = fresh;
                }
                const u64 k = ks_wave_max64(fresh >= G.min_u ? ga_key(fresh, rr) : 0);
                best = k > best ? k : best;
            }
            if (best == 0) break; // (uniform) no row left that adds min_unique hashes
            const u32 win = ~(u32)best, fresh = (u32)(best >> 32);
            // the whole wave takes the winner's hashes out of the live set and sums their abundances
            const u32 *list = G.inc + G.off[b + win];
            const u32 n = G.isect[b + win];
            u64 part = 0;
            for (u32 j = lane; j < n; j += 64) {
                const u32 p = list[j];
                if (p < nq) {
                    const u32 bit = 1u << (p & 31u);
                    if (atomicAnd(&live[p >> 5], ~bit) & bit) part += G.q_abund[qb + p];
                }
            }
            const u64 weighted = ks_wave_sum64(part);
            ga_wave_sync();
            rem -= fresh < rem ? fresh : rem;
            if (lane == (win & 63u)) { // (the lane that reads this row's count in the next round writes it)
                G.cnt[b + win] = 0u;
                G.flags[b + win] = 1u; G.rank[b + win] = round; G.unique[b + win] = fresh; G.remaining[b + win] = rem;
                G.weighted[b + win] = weighted;
            }
        }
    }
}

// ---- rounds: a workgroup per segment -------------------------------------------------------------------------------------------
KS_DEV u32 ga_live_load(const u32 *live, u32 w) { return __hip_atomic_load(&live[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the largest key of the workgroup (uniform); two barriers, s_red is the caller's again on return
KS_DEV u64 ga_block_max64(u64 v, u64 *s_red) {
    const u64 m = ks_wave_max64(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    u64 best = s_red[0];
    for (u32 i = 1; i < (blockDim.x >> 6); i++) best = s_red[i] > best ? s_red[i] : best;
    __syncthreads();
    return best;
}
// one wave counts the live positions of a list: 64 positions per load (every lane returns the count)
KS_DEV u32 ga_recount_wave(const u32 *list, u32 n, const u32 *live, u32 nq, u32 lane) {
    u32 c = 0;
    for (u32 s = 0; s < n; s += 64) {
        bool on = false;
        if (s + lane < n) {
            const u32 p = list[s + lane];
            on = p < nq && ((ga_live_load(live, p >> 5) >> (p & 31u)) & 1u) != 0u;
        }
        c += (u32)__popcll((long long)__ballot(on));
    }
    return c;
}

// live_cap: positions of the LDS bitmap (<= GA_LIVE_BITS); gbits: the bitmaps of the longer queries, query q's at word
// (q_off[q] >> 5) + q (its own words: no two queries share one).
__global__ __launch_bounds__(256) void k_ga_wg(ga_in G, const u32 *segs, u32 seg_cap, u32 live_cap, u32 *gbits) {
    __shared__ u32 s_live[GA_LIVE_BITS / 32];
    __shared__ u64 s_red[4];
    __shared__ u32 s_f0;
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (ks_seg_walk seg = ks_seg_list_by_wg(segs, seg_cap); seg.next();) {
        const u32 b = seg.b, len = seg.len;
        const u32 q = G.qid[b];
        const u64 qb = G.q_off[q];
        const u32 nq = (u32)(G.q_off[q + 1] - qb);
        u32 *live = nq <= live_cap ? s_live : gbits + (qb >> 5) + q;
        __syncthreads(); // (the previous segment's last readers)
        for (u32 i = t; i < (nq + 31) / 32; i += 256) __hip_atomic_store(&live[i], ga_full_word(i, nq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        u32 rem = nq;
        for (u32 round = 0; round < len && rem != 0; round++) {
            if (G.max_results != 0 && round == G.max_results) break;
            // the row with the largest stale count
            u64 k = 0;
            for (u32 rr = t; rr < len; rr += 256) {
                const u32 c = G.cnt[b + rr];
                if (c >= G.min_u) { const u64 kx = ga_key(c, rr); k = kx > k ? kx : k; }
            }
            k = ga_block_max64(k, s_red);
            if (k == 0) break; // (uniform) every row is dead
            const u32 r0 = ~(u32)k;
            if (wave == 0) {
                const u32 f = ga_recount_wave(G.inc + G.off[b + r0], G.isect[b + r0], live, nq, lane);
                if (lane == 0) { G.cnt[b + r0] = f; s_f0 = f; }
            }
            __syncthreads();
            const u32 f0 = s_f0;
            // the rows that can still beat it: a wave per row, 64 stale counts per look.  `need` only rises, and never above the
            // best fresh count of this round: a row below it cannot win, a row at it can (a smaller row index breaks the tie).
            u32 need = f0 > G.min_u ? f0 : G.min_u;
            u64 best = wave == 0 && f0 >= G.min_u ? ga_key(f0, r0) : 0;
            for (u32 sc = wave * 64; sc < len; sc += 256) {
                const u32 rr = sc + lane;
                const u32 stale = rr < len && rr != r0 ? G.cnt[b + rr] : 0u;
                u64 m = __ballot(stale >= need);
                while (m) {
                    const u32 j = (u32)__ffsll((long long)m) - 1u, row = sc + j;
                    const u32 f = ga_recount_wave(G.inc + G.off[b + row], G.isect[b + row], live, nq, lane);
                    if (lane == j) G.cnt[b + row] = f;
                    if (f >= G.min_u) { const u64 kx = ga_key(f, row); best = kx > best ? kx : best; }
                    need = f > need ? f : need;
                    m = __ballot(stale >= need) & ~((2ULL << j) - 1ULL);
                }
            }
            best = ga_block_max64(best, s_red);
            if (best == 0) break; // (uniform) no row adds min_unique hashes any more
            const u32 win = ~(u32)best, fresh = (u32)(best >> 32);
            // the workgroup takes the winner's hashes out of the live set and sums their abundances
            const u32 *list = G.inc + G.off[b + win];
            const u32 n = G.isect[b + win];
            u64 part = 0;
            for (u32 j = t; j < n; j += 256) {
                const u32 p = list[j];
                if (p < nq) {
                    const u32 bit = 1u << (p & 31u);
                    if (__hip_atomic_fetch_and(&live[p >> 5], ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) part += G.q_abund[qb + p];
                }
            }
            part = ks_wave_sum64(part);
            if (lane == 0) s_red[wave] = part;
            __syncthreads();
            rem -= fresh < rem ? fresh : rem;
            if (t == 0) {
                G.cnt[b + win] = 0u;
                G.flags[b + win] = 1u; G.rank[b + win] = round; G.unique[b + win] = fresh; G.remaining[b + win] = rem;
                G.weighted[b + win] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
            }
            __syncthreads(); // (s_red is read; the count and the bitmap are written)
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int gather_run(ks_ctx *ctx, const ks_hits *H, const ks_sketches *Q, const ks_sketches *T, u32 min_u, u32 max_results, ks_hits *B) {
    u32 n;
    u64 cap;
    KS_TRY(ks_hits_select_plan(ctx, "gather", H, Q, max_results, &n, &cap));
    KS_TRY(B->alloc(ctx, (size_t)cap, B->has_stats, KS_COLS_RANKED | KS_COLS_GATHER));
    if (n == 0) return KS_OK;
    if (Q->n_hashes == 0 || T->n_hashes == 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "gather: %llu hit rows, but a sketch set is empty: the inputs do not belong together",
                       (unsigned long long)n);

    bool small; // (tests: every segment one way; 3 = the workgroup path with a small LDS bitmap)
    const int mode = ks_seg_path_knob(ctx, KS_DBG_GATHER_PATH, &small);
    const u32 live_cap = small ? GA_LIVE_BITS_SMALL : GA_LIVE_BITS;
    // A search's rows share n_pair_instances hashes in all (a thresholded or best-hits list fewer): the size of the incidence
    // array without a round trip for the scan's total.  A list whose counts sum to more is refused by the row pass (GA_BAD_CAP).
    const u64 inc_cap = H->n_pair_instances;
    const u32 seg_cap = Q->n_seqs < n ? Q->n_seqs : n; // segments there can be
    ks_scratch sc(ctx);
    u64 *off = nullptr, *weighted = nullptr;
    ks_ctl ctl; // [GA_BAD_ID], [GA_BAD_COUNT], [GA_BAD_CAP]: the first such row; [GA_KEPT]: the scan's total
    u32 *inc = nullptr, *cnt = nullptr, *flags = nullptr, *rank = nullptr, *unique = nullptr, *remaining = nullptr, *wave_rows = nullptr,
        *wave_segs = nullptr, *wg_segs = nullptr, *gbits = nullptr;
    KS_TRY(sc.alloc(&off, (size_t)n + 1)); KS_TRY(sc.alloc(&inc, (size_t)inc_cap));
    KS_TRY(sc.alloc(&cnt, (size_t)n)); KS_TRY(sc.alloc(&flags, (size_t)n)); KS_TRY(sc.alloc(&rank, (size_t)n));
    KS_TRY(sc.alloc(&unique, (size_t)n)); KS_TRY(sc.alloc(&remaining, (size_t)n)); KS_TRY(sc.alloc(&weighted, (size_t)n));
    KS_TRY(ks_row_list_alloc(ctx, sc, (size_t)n, &wave_rows));
    KS_TRY(ks_seg_list_alloc(ctx, sc, seg_cap, &wave_segs)); KS_TRY(ks_seg_list_alloc(ctx, sc, seg_cap, &wg_segs));
    KS_TRY(sc.alloc(&gbits, (size_t)(Q->n_hashes >> 5) + Q->n_seqs + 2));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_GATHER, 3, 1));

    KS_TRY(ks_scan_u32_to_u64(ctx, H->d_isect, off, n));
    const ga_in G = {Q->d_offsets, Q->d_hashes, T->d_offsets, T->d_hashes, Q->d_abunds, H->d_qid, H->d_tid, H->d_isect, off, inc, inc_cap,
                     n, Q->n_seqs, T->n_seqs, min_u, max_results, cnt, flags, rank, unique, remaining, weighted};
    KS_LAUNCH(ctx, "gather_rows", k_ga_rows, (n + 255) / 256, 256, G, mode, seg_cap, wave_rows, wave_segs, wg_segs, ctl.words());
    KS_LAUNCH(ctx, "gather_rows_wave", k_ga_rows_wave, GA_ROWS_WAVE_GRID, 256, G, (const u32 *)wave_rows, ctl.words());
    if (mode != 2) KS_LAUNCH(ctx, "gather_wave", k_ga_wave, GA_WAVE_GRID, 256, G, (const u32 *)wave_segs, seg_cap);
    KS_LAUNCH(ctx, "gather_wg", k_ga_wg, GA_WG_GRID, 256, G, (const u32 *)wg_segs, seg_cap, live_cap, gbits);
    const ks_gather_cols cols = {unique, remaining, weighted};
    return ks_hits_select_tail(ctx, "gather", H, n, flags, rank, cap, &cols, ctl, GA_KEPT, [&]() -> int {
        if (ctl.bad(GA_BAD_ID))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "gather: hit row %llu names a query or target beyond the sketch sets (%u queries, %u targets)",
                           (unsigned long long)ctl[GA_BAD_ID], Q->n_seqs, T->n_seqs);
        if (ctl.bad(GA_BAD_COUNT))
            return ks_fail(ctx, KS_ERR_INVALID_ARG,
                           "gather: hit row %llu does not share `intersect` hashes in these sketches: hits and sketches do not belong together",
                           (unsigned long long)ctl[GA_BAD_COUNT]);
        if (ctl.bad(GA_BAD_CAP))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "gather: the intersect column sums to more than the list's %llu matched pairs at hit row %llu",
                           (unsigned long long)inc_cap, (unsigned long long)ctl[GA_BAD_CAP]);
        return KS_OK;
    }, B);
}

extern "C" int ks_hits_gather(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *queries, const ks_sketches *targets,
                              const ks_gather_opts *opts, ks_hits **out) {
    return ks_guard(ctx, [&]() -> int {
    if (out) *out = nullptr;
    if (opts) KS_TRY(ks_opts_words_check(ctx, "gather", opts->flags, 0, opts->reserved));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!hits || !queries || !targets || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "gather", hits, queries, targets));
    KS_TRY(ks_params_check_same(ctx, "gather", "the sketch sets", queries->params, targets->params));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(queries))); // (the passes read both sets as plain CSRs)
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(targets)));
    ks_result<ks_hits> B(ctx, out, ks_hits_free);
    ks_hits_inherit(B, hits);
    const u32 min_u = opts && opts->min_unique ? opts->min_unique : 1u;
    KS_TRY(gather_run(ctx, hits, queries, targets, min_u, opts ? opts->max_results : 0u, B));
    if (hits->n_hits == 0) KS_TRY(ks_stream_wait(ctx)); // (a dense copy may be queued: the pass is synchronous on return)
    return B.commit();
    });
}
