// ks_rows.hip — from a sorted list to one record per run of equal keys: ks_sorted_runs (a sketch set's hashes: the union,
// ks_union.hip, and the corpus, ks_signif.hip, emit one record per distinct hash) and ks_search_rows / ks_search_rows_agg (a
// search's matches, sorted or by level-1 region -> rows, then per row the abundance statistics and the containment filter).
#include "ks_device.h"

// ---------------------------------------------------------------------------------------------
// run boundaries of a sorted key list (ks_sorted_runs): heads, then the first record of every run
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pair_heads(const u64 *keys, u64 n, u32 *heads) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    heads[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// hidx = exclusive scan of heads; row r starts where hidx steps from r to r+1
__global__ __launch_bounds__(256) void k_pair_rows(const u64 *keys, const u32 *hidx, u64 n, u32 n_rows, u64 *row_start) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool head = (i == 0) || keys[i] != keys[i - 1];
    if (head) row_start[hidx[i]] = i;
    if (i == 0) row_start[n_rows] = n;
}

// in: dense (ks_sketches_make_dense), n_hashes > 0.  Its postings sorted by hash and the start of every run, in the caller's scratch;
// one wait.  The count is used only after the scan that made it is known to have held, and only if it can be a run count.
int ks_sorted_runs(ks_ctx *ctx, const ks_sketches *in, ks_scratch &sc, ks_runs *out) {
    const u64 n = in->n_hashes;
    u64 *k0 = nullptr, *k1 = nullptr;
    u32 *v0 = nullptr, *v1 = nullptr, *heads = nullptr, *d_nrows = nullptr;
    KS_TRY(sc.alloc(&k0, (size_t)n)); KS_TRY(sc.alloc(&k1, (size_t)n));
    KS_TRY(sc.alloc(&v0, (size_t)n)); KS_TRY(sc.alloc(&v1, (size_t)n));
    const int shifts[8] = {0, 8, 16, 24, 32, 40, 48, 56};
    KS_TRY(ks_radix_sort_u32(ctx, KS_SORT_PAIRS, in->d_hashes, in->d_abunds, k0, v0, k1, v1, n, shifts, 8, &out->keys, &out->vals));
    KS_TRY(sc.alloc(&heads, (size_t)n));
    KS_TRY(sc.alloc(&d_nrows, 1));
    const u32 g = (u32)((n + 255) / 256);
    KS_LAUNCH(ctx, "run_heads", k_pair_heads, g, 256, (const u64 *)out->keys, n, heads);
    KS_TRY(ks_scan_u32_inplace(ctx, heads, n, d_nrows));
    u64 *const rb = ctx->h_pin + KS_PIN_READ;
    KS_HIP(ctx, hipMemcpyAsync(rb, d_nrows, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    KS_TRY(ks_scan_status_fetch(ctx));
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    KS_TRY(ks_scan_status_check(ctx));
    const u32 n_rows = *(u32 *)rb;
    if (n_rows == 0 || n_rows > n) return ks_fail(ctx, KS_ERR_HIP, "internal error: %u runs in %llu sorted postings", n_rows, (unsigned long long)n);
    out->n_rows = n_rows;
    KS_TRY(sc.alloc(&out->row_start, (size_t)n_rows + 1));
    KS_LAUNCH(ctx, "run_starts", k_pair_rows, g, 256, (const u64 *)out->keys, (const u32 *)heads, n, n_rows, out->row_start);
    return KS_OK;
}

// ---------------------------------------------------------------------------------------------
// Sorted match list -> COO rows in ONE pass: heads, their prefix over the whole list and the per-row sums used to be three
// passes (heads, a device-wide scan, a reduce) — 0.23 ms of the 1M x 1M step and a quarter of the all-vs-all one, where two
// records in three open a row.  Here a tile of PF_TILE records keeps its keys in registers: sweep 1 marks the heads (bit per
// round) and counts them per (round, wave); wave 0 turns the 32 counts into offsets and chains the tile's total through a
// decoupled look-back (ticket-ordered tiles, 8-byte {flag, value} words); sweep 2 gives every record its row and sums
// count / abundance per row with a segmented scan (rows span waves and tiles, so the partial sums are added atomically:
// ~2 atomics per wave and round).  Rows beyond `rows_cap` are dropped (the row arrays are sized from the previous search's
// row count; the host repeats this launch with exact arrays when the true count is larger).
// ---------------------------------------------------------------------------------------------
#define PF_THREADS 256
#define PF_IPT 8
#define PF_TILE (PF_THREADS * PF_IPT)
#define PF_WAVES (PF_THREADS / 64)

__global__ __launch_bounds__(PF_THREADS) void k_pair_rows_fused(const u64 *keys, u64 n, u32 *qid, u32 *tid, u32 *isect, unsigned long long *nw,
                                                                int tbits, int abits, u32 rows_cap, unsigned long long *status,
                                                                u32 *ticket /* [0] tile ids, [1] a look-back gave up */, u32 *n_rows_out,
                                                                int use_ticket) {
    __shared__ u32 tile_s;
    __shared__ u32 wcount[PF_IPT][PF_WAVES]; // heads per (round, wave), then exclusive offsets inside the tile
    __shared__ unsigned long long base_s;
    const u32 tid_ = threadIdx.x, lane = tid_ & 63, wave = tid_ >> 6;
    // Tile ids in dispatch order (blockIdx.x): workgroups start in that order on this hardware, so a tile's predecessors are
    // running or done when it looks back.  That is not a documented guarantee: the look-back spins for a bounded time, and a
    // launch in which one gave up is repeated with ids from an atomic ticket (order of arrival; ~12 ns per ticket on one
    // address — 10^4 tiles are 0.1 ms of queueing, most of this kernel's former run time).
    if (use_ticket) { // uniform
        if (tid_ == 0) tile_s = atomicAdd(&ticket[0], 1u);
        __syncthreads();
    }
    const u32 tile = use_ticket ? tile_s : blockIdx.x;
    const u64 b0 = (u64)tile * PF_TILE;
    u64 key[PF_IPT];
    u32 headbits = 0;
    // sweep 1: record i of round r is b0 + r * PF_THREADS + tid (coalesced); a head opens a row
#pragma unroll
    for (int r = 0; r < PF_IPT; r++) {
        const u64 i = b0 + (u64)r * PF_THREADS + tid_;
        key[r] = i < n ? keys[i] : 0;
    }
    // The previous record: the lane below's (two DPP moves, no LDS crossbar), except for lane 0, whose predecessor sits in the
    // previous wave / round / tile: lane r of the wave loads it for round r — one register pair and ONE memory latency for all
    // rounds (a load inside the loop was waited for in every round: eight dependent latencies per tile).
    u64 pp = 0;
    {
        const u64 iw = b0 + (u64)lane * PF_THREADS + (tid_ & ~63u); // lane r: where this wave's round r starts
        if (lane < PF_IPT && iw > 0 && iw < n) pp = keys[iw - 1];
    }
#pragma unroll
    for (int r = 0; r < PF_IPT; r++) {
        const u64 i = b0 + (u64)r * PF_THREADS + tid_;
        const u64 below = ((u64)ks_lane_below((u32)(key[r] >> 32)) << 32) | ks_lane_below((u32)key[r]);
        const u64 first = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(pp >> 32), r) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)pp, r);
        const u64 prev = lane ? below : first;
        const bool head = i < n && (i == 0 || (prev >> abits) != (key[r] >> abits));
        headbits |= head ? (1u << r) : 0u;
        const u64 m = __ballot(head);
        if (lane == 0) wcount[r][wave] = (u32)__popcll(m);
    }
    __syncthreads();
    // wave 0: exclusive offsets of the 32 (round, wave) groups in record order, tile total, look-back
    if (wave == 0) {
        const u32 c = lane < PF_IPT * PF_WAVES ? wcount[lane / PF_WAVES][lane % PF_WAVES] : 0u;
        const u32 incl = ks_wave_incl_scan(c);
        const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
        if (lane < PF_IPT * PF_WAVES) wcount[lane / PF_WAVES][lane % PF_WAVES] = incl - c;
        if (lane == 0)
            __hip_atomic_store(&status[tile], (tile == 0 ? KS_LB_PRE : KS_LB_AGG) | (u64)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u64 excl = 0;
        if (tile > 0) {
            excl = ks_lookback_walk(tile, lane, ks_lookback_words(status), &ticket[1]); // gave up: the host reports it
            if (lane == 0)
                __hip_atomic_store(&status[tile], KS_LB_PRE | (excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            base_s = excl;
            if (b0 + PF_TILE >= n) *n_rows_out = (u32)(excl + total); // the last tile knows the row count
        }
    }
    __syncthreads();
    const u64 base = base_s;
    // sweep 2: rows and per-row sums
#pragma unroll
    for (int r = 0; r < PF_IPT; r++) {
        const u64 i = b0 + (u64)r * PF_THREADS + tid_;
        const bool live = i < n;
        const bool head = (headbits >> r) & 1u;
        const u64 m = __ballot(head);
        // heads at or before this record, over the whole list, minus one = its row
        const u64 row64 = base + wcount[r][wave] + ks_lane_lt_count(m) + (head ? 1u : 0u) - 1u;
        const u32 row = live ? (u32)row64 : 0xffffffffu;
        u64 w = live ? (key[r] & ((1ULL << abits) - 1ULL)) : 0;
        u32 c = live ? 1u : 0u;
        if (head && row < rows_cap) {
            const u64 ids = key[r] >> abits;
            qid[row] = (u32)(ids >> tbits);
            tid[row] = (u32)(ids & ((1ULL << tbits) - 1ULL));
        }
        // Inclusive segmented scan (segments = equal row; rows ascend, so a lane whose source has my row continues my segment) with DPP
        // moves only: four row_shr steps inside the rows of 16, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 — the
        // __shfl_up form was 25 ds_bpermute per round, 213 per thread: the LDS crossbar was this kernel (19 M wave-level permutes
        // for the 49 M records of a 200k all-vs-all).  A lane without a source reads `rowx`, which is not its row: it adds nothing.
        {
            const u32 rowx = row ^ 1u;
            u32 wl = (u32)w, wh = (u32)(w >> 32);
#define PF_SEG_STEP(CTRL, RMASK) do { \
                const u32 orow = (u32)__builtin_amdgcn_update_dpp((int)rowx, (int)row, CTRL, RMASK, 0xf, false); \
                const u32 oc = (u32)__builtin_amdgcn_update_dpp(0, (int)c, CTRL, RMASK, 0xf, false); \
                const u32 ol = (u32)__builtin_amdgcn_update_dpp(0, (int)wl, CTRL, RMASK, 0xf, false); \
                const u32 oh = (u32)__builtin_amdgcn_update_dpp(0, (int)wh, CTRL, RMASK, 0xf, false); \
                const bool same = orow == row; \
                const u64 nw_ = (((u64)wh << 32) | wl) + (same ? (((u64)oh << 32) | ol) : 0ULL); \
                c += same ? oc : 0u; wl = (u32)nw_; wh = (u32)(nw_ >> 32); } while (0)
            PF_SEG_STEP(0x111, 0xf); // row_shr:1
            PF_SEG_STEP(0x112, 0xf); // row_shr:2
            PF_SEG_STEP(0x114, 0xf); // row_shr:4
            PF_SEG_STEP(0x118, 0xf); // row_shr:8
            PF_SEG_STEP(0x142, 0xa); // row_bcast:15 -> rows 1 and 3
            PF_SEG_STEP(0x143, 0xc); // row_bcast:31 -> rows 2 and 3
#undef PF_SEG_STEP
            w = ((u64)wh << 32) | wl;
        }
        const u32 nrow = (u32)__builtin_amdgcn_update_dpp((int)(row ^ 1u), (int)row, 0x130, 0xf, 0xf, false); // wave_shl:1 (lane 63: not its row)
        // (Measured dead end: STORING the rows whose records all sit inside one wave — most rows of an all-vs-all search are one or
        // two records — instead of adding them: 0.45 -> 0.83 ms at 200k x 200k hp.  Scattered 4- / 8-byte stores of a wave cost
        // more than the same no-return atomics, which the L2 merges line by line.  Handing the head lanes' ids to lanes 0 .. heads-1
        // through LDS so that qid[] / tid[] leave coalesced: no change, 0.453 ms either way.)
        if (live && (lane == 63 || nrow != row) && row < rows_cap) {
            atomicAdd(&isect[row], c);
            atomicAdd(&nw[row], (unsigned long long)w);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Level-1 regions of the match sort -> COO rows by HASH aggregation (k_pairs_aggregate).  The rows need the records grouped by
// (qid, tid) with a count and an abundance sum, and the groups in order — not a totally ordered list.  Where many records share
// a row (80 at 1M x 1M protein k = 10) grouping by hash and sorting only the groups is that many times the smaller sort: the
// two further moves of the list, the in-LDS radix sort and the run-length pass (0.39 ms of that step) become ONE read of the
// level-1 output.  Workgroup r owns region r (every (qid, tid) lies wholly inside one region, regions ascend in the ids):
//   1. every record goes into an open-addressing table in LDS, keyed by record >> abits: an LDS compare-and-swap claims the
//      slot, two LDS adds count the record and sum its abundance.  Linear probing with wrap-around, at most n_slots probes: a
//      record that finds no slot raises the overflow word, the workgroup stops inserting, and the host resumes the sort on the
//      untouched list.  No loop here is unbounded.  A thread's eight records of burst t + 1 are requested before burst t is
//      inserted, and the first probes of a burst's eight records are in flight together: with many records per row nearly
//      every record finds its key there and is two adds without a return value; only a miss walks the probe loop.
//   2. the region's group count is published for the decoupled look-back (ks_device.h) BEFORE the sort, so the successors'
//      walks find it early; the occupied slots are then compacted to the front of the table and sorted by key with a bitonic
//      network over the next power of two at or above the group count (a quarter of the slots at 1M x 1M: 55 steps of 512
//      pairs instead of 78 of 2,048)
//   3. wave 0 walks back for the rows of the regions before this one; the groups leave as rows base .. base + groups - 1
// The list is read once.  Rows beyond `rows_cap` are dropped and the host repeats the launch, as for k_pair_rows_fused.
// ---------------------------------------------------------------------------------------------
#define AG_THREADS 1024
#define AG_IPT 8
#define AG_SLOTS 4096 // 20 bytes per slot: 80 KB of the CU's 160 KB LDS
#define AG_EMPTY (~0ULL) // (a key has at most 63 bits: the records keep at least one abundance bit)
static_assert(AG_SLOTS % AG_THREADS == 0 && (AG_SLOTS & (AG_SLOTS - 1)) == 0, "the bitonic network walks a power of two");

// key k (abundance w) into the table, probing from `slot`: false = no slot within n_slots probes
KS_DEV bool ag_insert(unsigned long long *keys, unsigned long long *sums, u32 *cnts, u32 *n_used, unsigned long long k,
                      unsigned long long w, u32 slot, u32 n_slots) {
    for (u32 p = 0; p < n_slots; p++) {
        unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == AG_EMPTY) {
            cur = atomicCAS(&keys[slot], AG_EMPTY, k);
            if (cur == AG_EMPTY) { atomicAdd(n_used, 1u); cur = k; }
        }
        if (cur == k) {
            atomicAdd(&cnts[slot], 1u);
            atomicAdd(&sums[slot], w);
            return true;
        }
        slot = slot + 1 == n_slots ? 0 : slot + 1;
    }
    return false;
}

__global__ __launch_bounds__(AG_THREADS) void k_pairs_aggregate(const u64 *list, const u32 *ends, u32 n_slots, u32 *qid, u32 *tid, u32 *isect,
                                                                unsigned long long *nw, int tbits, int abits, u32 rows_cap,
                                                                unsigned long long *status,
                                                                u32 *ctl /* [0] a table overflowed, [1] a look-back gave up, [2] rows */) {
    __shared__ unsigned long long keys[AG_SLOTS];
    __shared__ unsigned long long sums[AG_SLOTS];
    __shared__ u32 cnts[AG_SLOTS];
    __shared__ u32 n_used, n_packed, oflow;
    __shared__ unsigned long long base_s;
    const u32 tid_ = threadIdx.x, lane = tid_ & 63, wave = tid_ >> 6, region = blockIdx.x;
    for (u32 i = tid_; i < AG_SLOTS; i += AG_THREADS) { keys[i] = AG_EMPTY; sums[i] = 0; cnts[i] = 0; }
    if (tid_ == 0) { n_used = 0; n_packed = 0; oflow = 0; }
    const u64 s = region ? ends[region - 1] : 0, e = ends[region];
    const u64 am = (1ULL << abits) - 1ULL;
    // (every load is issued, past the region's end at a clamped index: loads under a branch cannot be counted, and the wait for
    // burst t would then also wait for burst t + 1)
    const u64 last = e ? e - 1 : 0;
    u64 nxt[AG_IPT];
#pragma unroll
    for (int r = 0; r < AG_IPT; r++) {
        const u64 i = s + (u64)r * AG_THREADS + tid_;
        nxt[r] = list[i < e ? i : last];
    }
    __syncthreads();
    for (u64 t0 = s; t0 < e; t0 += AG_THREADS * AG_IPT) {
        u64 rec[AG_IPT];
#pragma unroll
        for (int r = 0; r < AG_IPT; r++) rec[r] = nxt[r];
#pragma unroll
        for (int r = 0; r < AG_IPT; r++) { // the next burst is on its way while this one is inserted
            const u64 i = t0 + (u64)(AG_IPT + r) * AG_THREADS + tid_;
            nxt[r] = list[i < e ? i : last];
        }
        if (*(volatile u32 *)&oflow) break; // (once per burst: a region that overflowed is not read to its end)
        u32 slot[AG_IPT];
        unsigned long long seen[AG_IPT];
#pragma unroll
        for (int r = 0; r < AG_IPT; r++) { // all first probes of the burst together: one LDS latency, not eight
            const unsigned long long k = rec[r] >> abits;
            slot[r] = __umulhi((u32)((k * 0x9E3779B97F4A7C15ULL) >> 32), n_slots); // (< n_slots)
            seen[r] = __hip_atomic_load(&keys[slot[r]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
#pragma unroll
        for (int r = 0; r < AG_IPT; r++) {
            const u64 i = t0 + (u64)r * AG_THREADS + tid_;
            if (i >= e) continue;
            const unsigned long long k = rec[r] >> abits, w = rec[r] & am;
            if (seen[r] == k) {
                atomicAdd(&cnts[slot[r]], 1u);
                atomicAdd(&sums[slot[r]], w);
            } else if (!ag_insert(keys, sums, cnts, &n_used, k, w, slot[r], n_slots)) {
                oflow = 1u;
            }
        }
    }
    __syncthreads();
    // an overflowed region publishes no groups: its successors must not wait for it, and the host drops every row anyway
    const u32 groups = oflow ? 0u : n_used;
    if (tid_ == 0) {
        if (oflow) atomicOr(&ctl[0], 1u);
        __hip_atomic_store(&status[region], (region == 0 ? KS_LB_PRE : KS_LB_AGG) | (u64)groups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (groups > 0) { // (uniform)
        // the occupied slots to [0, groups), in any order: every thread takes its slots into registers, then writes where they lay
        unsigned long long ck[AG_SLOTS / AG_THREADS], cs[AG_SLOTS / AG_THREADS];
        u32 cc[AG_SLOTS / AG_THREADS];
#pragma unroll
        for (int j = 0; j < AG_SLOTS / AG_THREADS; j++) {
            const u32 i = (u32)j * AG_THREADS + tid_;
            ck[j] = keys[i]; cs[j] = sums[i]; cc[j] = cnts[i];
        }
        u32 p2 = 1;
        while (p2 < groups) p2 <<= 1; // (groups <= n_slots <= AG_SLOTS)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < AG_SLOTS / AG_THREADS; j++) {
            const bool occ = ck[j] != AG_EMPTY;
            const u64 m = __ballot(occ);
            u32 b = 0;
            if (lane == 0 && m) b = atomicAdd(&n_packed, (u32)__popcll(m));
            b = (u32)__builtin_amdgcn_readfirstlane((int)b);
            if (occ) {
                const u32 d = b + ks_lane_lt_count(m); // (< groups: every occupied slot was counted in n_used)
                keys[d] = ck[j]; sums[d] = cs[j]; cnts[d] = cc[j];
            }
        }
        for (u32 i = groups + tid_; i < p2; i += AG_THREADS) keys[i] = AG_EMPTY; // (empty = the largest key: stays behind the groups)
        __syncthreads();
        // bitonic network over [0, p2), a pair per thread and step: ascending, the groups end up in [0, groups)
        for (u32 k2 = 2; k2 <= p2; k2 <<= 1) {
            for (u32 j = k2 >> 1; j > 0; j >>= 1) {
                for (u32 t = tid_; t < p2 / 2; t += AG_THREADS) {
                    const u32 i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
                    const unsigned long long a = keys[i], b = keys[o];
                    if ((a > b) == ((i & k2) == 0) && a != b) {
                        keys[i] = b; keys[o] = a;
                        const unsigned long long sa = sums[i]; sums[i] = sums[o]; sums[o] = sa;
                        const u32 ca = cnts[i]; cnts[i] = cnts[o]; cnts[o] = ca;
                    }
                }
                __syncthreads();
            }
        }
    }
    if (wave == 0) {
        u64 excl = 0;
        if (region > 0) {
            excl = ks_lookback_walk(region, lane, ks_lookback_words(status), &ctl[1]); // gave up: the host resumes the sort
            if (lane == 0)
                __hip_atomic_store(&status[region], KS_LB_PRE | (excl + groups), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            base_s = excl;
            if (region == gridDim.x - 1) ctl[2] = (u32)(excl + groups); // the last region knows the row count
        }
    }
    __syncthreads();
    const u64 base = base_s;
    for (u32 i = tid_; i < groups; i += AG_THREADS) {
        const u64 row = base + i;
        if (row < rows_cap) {
            const unsigned long long k = keys[i];
            qid[row] = (u32)(k >> tbits);
            tid[row] = (u32)(k & ((1ULL << tbits) - 1ULL));
            isect[row] = cnts[i];
            nw[row] = sums[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// KS_SEARCH_ABUND_STATS: per-row statistics of the shared target abundances.  The match sort then also orders the abundance
// bits, so the records of row r — [row_start[r], row_start[r] + isect[r]) of the sorted list — ascend in abundance, and the
// statistics replay a host loop over the sorted abundances operation for operation: sum += a, mean = sum / n, then
// ss += (a - mean) * (a - mean), in ascending order, rounded after every operation (no contraction into fma).  Most rows hold
// one or two records: a lane per row.  A row longer than RA_LONG is listed for k_row_abund_stats_long instead, where a wave
// loads it 64 records at a time and adds them in order from registers — a self-hit at scaled = 1 is as long as the sequence,
// and one lane walking it through memory would hold its workgroup's other 255 lanes for the whole walk.
// ---------------------------------------------------------------------------------------------
#define RA_LONG 64

__global__ __launch_bounds__(256) void k_row_abund_stats(const u64 *pk, const u64 *row_start, const u32 *isect, const u32 *n_rows_dev,
                                                         u32 rows_cap, int abits, u64 *median2, double *ss, u32 *long_rows) {
#pragma clang fp contract(off)
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 n_rows = *n_rows_dev < rows_cap ? *n_rows_dev : rows_cap; // (more rows than the arrays: the host repeats the pass)
    if (r >= n_rows) return;
    const u32 n = isect[r];
    const u64 *a = pk + row_start[r];
    const u64 am = (1ULL << abits) - 1ULL;
    if (n > RA_LONG) { ks_row_list_push(long_rows, r); return; }
    if (n == 0) { median2[r] = 0; ss[r] = 0.0; return; } // (no row: only after a look-back that gave up, which is repeated)
    double sum = 0.0;
    for (u32 j = 0; j < n; j++) sum += (double)(a[j] & am);
    const double mean = sum / (double)n;
    double acc = 0.0;
    for (u32 j = 0; j < n; j++) {
        const double d = (double)(a[j] & am) - mean;
        acc += d * d;
    }
    ss[r] = acc;
    median2[r] = (n & 1u) ? 2ULL * (a[n / 2] & am) : (a[n / 2 - 1] & am) + (a[n / 2] & am);
}

// the rows k_row_abund_stats listed (at most rows_cap), a wave per row (ks_row_list_walk): each chunk of 64 records is loaded
// coalesced, one per lane, and added in lane order
__global__ __launch_bounds__(256) void k_row_abund_stats_long(const u64 *pk, const u64 *row_start, const u32 *isect, const u32 *long_rows,
                                                              u32 rows_cap, int abits, u64 *median2, double *ss) {
    const u32 lane = threadIdx.x & 63;
    const u64 am = (1ULL << abits) - 1ULL;
    ks_row_list_walk(long_rows, rows_cap, [&](u32 r) {
#pragma clang fp contract(off)
        const u32 n = isect[r];
        const u64 *a = pk + row_start[r];
        double sum = 0.0;
        for (u32 c = 0; c < n; c += 64) {
            const double x = c + lane < n ? (double)(a[c + lane] & am) : 0.0;
            ks_wave_add_ordered(ks_lanes_below(n - c), sum, x);
        }
        const double mean = sum / (double)n;
        double acc = 0.0;
        for (u32 c = 0; c < n; c += 64) {
            const double d = c + lane < n ? (double)(a[c + lane] & am) - mean : 0.0;
            const double t = d * d;
            ks_wave_add_ordered(ks_lanes_below(n - c), acc, t);
        }
        if (lane == 0) {
            ss[r] = acc;
            median2[r] = (n & 1u) ? 2ULL * (a[n / 2] & am) : (a[n / 2 - 1] & am) + (a[n / 2] & am);
        }
    });
}

// ---------------------------------------------------------------------------------------------
// min_containment: a stable compaction of the row columns.  k_rows_keep writes the keep flag of every row (the host's f64
// test: (double)intersect / (double)|q| >= min_containment, |q| = the query's distinct hashes), an exclusive scan turns the
// flags into destinations (its total, the kept count, lands beside the row count: one read-back), k_rows_filter moves the kept
// rows (rf_cols / rf_move, ks_device.h), recomputing the same flag.
// ---------------------------------------------------------------------------------------------
KS_DEV bool rf_kept(const rf_cols &in, u32 r, const u64 *q_offsets, const u32 *q_counts, u32 n_queries, double min_c) {
    const u32 q = in.qid[r];
    if (q >= n_queries) return false; // (a row without a head: only after a look-back that gave up, which is repeated)
    const u64 nq = q_counts ? (u64)q_counts[q] : q_offsets[q + 1] - q_offsets[q];
    return (double)in.isect[r] / (double)nq >= min_c;
}

__global__ __launch_bounds__(256) void k_rows_keep(rf_cols in, const u32 *n_rows_dev, u32 rows_cap, const u64 *q_offsets, const u32 *q_counts,
                                                   u32 n_queries, double min_c, u32 *flags) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows_cap) return;
    const u32 n_rows = *n_rows_dev < rows_cap ? *n_rows_dev : rows_cap;
    flags[r] = (r < n_rows && rf_kept(in, r, q_offsets, q_counts, n_queries, min_c)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_rows_filter(rf_cols in, const u32 *n_rows_dev, u32 rows_cap, const u64 *q_offsets, const u32 *q_counts,
                                                     u32 n_queries, double min_c, const u32 *dst, u32 *qid, u32 *tid, u32 *isect, u64 *nw,
                                                     u64 *median2, double *ss) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 n_rows = *n_rows_dev < rows_cap ? *n_rows_dev : rows_cap;
    if (r >= n_rows || !rf_kept(in, r, q_offsets, q_counts, n_queries, min_c)) return;
    rf_move(in, r, dst[r], qid, tid, isect, nw, median2, ss);
}

// The wave grids of the two row splits stay two numbers: each is the launch shape its kernel was measured with.  The statistics
// list the few rows longer than RA_LONG (self-hits); the significance pass lists most rows of a scaled = 1 search (SG_WAVE_GRID).
#define RA_LONG_GRID 256 // workgroups of k_row_abund_stats_long (4 waves each, striding over the long rows)

// Behind the row pass of one attempt and before its wait: the statistics into H's columns (Q.stats) and the rows that pass
// the containment test into F (Q.min_c > 0).  The kernels take the row count from the device (ticket[2]; an attempt with more
// rows than rows_cap is repeated anyway) and the scan of the keep flags writes the kept count to ticket[3], which the row
// pass's read-back brings home with the row count: no wait of its own.
static int se_rows_post(ks_ctx *ctx, const ks_rows_in &Q, ks_hits *H, ks_hit_cols &F, const u64 *pk, u32 rows_cap, u32 *ticket, ks_scratch &sc) {
    const u32 *n_rows_dev = ticket + 2;
    const u32 g = (rows_cap + 255) / 256;
    if (Q.stats) {
        u64 *row_start = nullptr;
        u32 *long_rows = nullptr;
        KS_TRY(sc.alloc(&row_start, (size_t)rows_cap + 1));
        KS_TRY(ks_row_list_alloc(ctx, sc, rows_cap, &long_rows));
        KS_TRY(ks_alloc(ctx, &H->d_median2, rows_cap));
        KS_TRY(ks_alloc(ctx, &H->d_ss, rows_cap));
        KS_TRY(ks_scan_u32_to_u64(ctx, H->d_isect, row_start, rows_cap)); // (rows past the count have intersect 0)
        KS_LAUNCH(ctx, "row_abund_stats", k_row_abund_stats, g, 256, pk, (const u64 *)row_start, (const u32 *)H->d_isect, n_rows_dev,
                  rows_cap, Q.abits, H->d_median2, H->d_ss, long_rows);
        KS_LAUNCH(ctx, "row_abund_stats_long", k_row_abund_stats_long, RA_LONG_GRID, 256, pk, (const u64 *)row_start,
                  (const u32 *)H->d_isect, (const u32 *)long_rows, rows_cap, Q.abits, H->d_median2, H->d_ss);
    }
    if (Q.min_c > 0) {
        const ks_sketches *q = Q.q;
        const u32 *counts = q->gapped ? q->d_counts : nullptr; // (a gapped batch: distinct hashes per query; else the CSR's runs)
        const rf_cols in = H->rows();
        u32 *flags = nullptr;
        KS_TRY(sc.alloc(&flags, rows_cap));
        KS_LAUNCH(ctx, "rows_keep", k_rows_keep, g, 256, in, n_rows_dev, rows_cap, (const u64 *)q->d_offsets, counts, q->n_seqs, Q.min_c,
                  flags);
        KS_TRY(ks_scan_u32_inplace(ctx, flags, rows_cap, ticket + 3));
        KS_TRY(F.alloc(ctx, rows_cap, Q.stats, 0));
        KS_LAUNCH(ctx, "rows_filter", k_rows_filter, g, 256, in, n_rows_dev, rows_cap, (const u64 *)q->d_offsets, counts, q->n_seqs, Q.min_c,
                  (const u32 *)flags, F.d_qid, F.d_tid, F.d_isect, F.d_nw, F.d_median2, F.d_ss);
    }
    return KS_OK;
}

// Above how many records per row of the previous search the aggregate pass is taken.  DESIGN.md 3.2 [r6] has the measurements:
// the aggregate pass won at every multiplicity that fits the tables, down to 2.5, and nothing below was measured — 8 is that
// lowest winning point with a margin on the sort's side, not a crossover.  The rows per region it is trusted with: half of
// the slots, over the regions the batch can fill (the regions are the top 8 id bits: a batch just above a power of two
// reaches only half of them).  A search whose tables overflowed is remembered by its row count: the pass is not tried again
// on this context until a search expects under half as many rows (no wasted launch and wait on every search of a steady
// workload that is skewed beyond the average the capacity rule sees).
#define KS_AGG_MIN_MULT 8.0
#define KS_AGG_REGION_ROWS (AG_SLOTS / 2)

bool ks_rows_agg_wanted(const ks_ctx *ctx, const ks_rows_in &Q) {
    if (Q.stats || Q.n_pairs == 0) return false; // (the statistics read the sorted list)
    if (const char *f = ks_dbg(ctx, KS_DBG_ROWS_PATH)) return strcmp(f, "agg") == 0;
    // (a knob that forces a path of the sort's later levels or of its row pass asks for that pass)
    if (ks_dbg(ctx, KS_DBG_MSD_LDS_CAP) || ks_dbg(ctx, KS_DBG_ROWS_TICKET) || ks_dbg(ctx, KS_DBG_FORCE_ROWS_TICKET_RETRY)) return false;
    if (!(ctx->rows_mult > KS_AGG_MIN_MULT)) return false;
    const u32 n_q = Q.q->n_seqs;
    const int qbits = Q.qbits;
    const u64 regions = qbits >= 8 && n_q ? ((u64)(n_q - 1) >> (qbits - 8)) + 1 : (u64)KS_MSD_REGIONS;
    const double rows = (double)Q.n_pairs / ctx->rows_mult;
    if (ctx->agg_oflow_rows && rows * 2.0 > (double)ctx->agg_oflow_rows) return false;
    return rows <= (double)(regions * KS_AGG_REGION_ROWS);
}

void ks_rows_agg_overflowed(ks_ctx *ctx, u64 n_rows) {
    if (ks_dbg(ctx, KS_DBG_ROWS_PATH)) return; // (a forced path leaves no history)
    if (!ctx->agg_oflow_rows || n_rows < ctx->agg_oflow_rows) ctx->agg_oflow_rows = n_rows ? n_rows : 1;
}

// the matches into H's rows in one pass: the run-length reduce of the sorted list pk (k_pair_rows_fused), or — A != nullptr — the
// hash aggregation of the level-1 regions of the match sort (k_pairs_aggregate; *fell_back: see ks_search_rows_agg)
static int se_rows_run(ks_ctx *ctx, const ks_rows_in &Q, ks_hits *H, const u64 *pk, const ks_msd_plan *A, bool *fell_back) {
    const u64 n_pairs = Q.n_pairs;
    const int tbits = Q.tbits, abits = Q.abits;
    const u32 pf_tiles = A ? (u32)KS_MSD_REGIONS : (u32)((n_pairs + PF_TILE - 1) / PF_TILE);
    u32 agg_slots = AG_SLOTS;
    if (const char *f = ks_dbg(ctx, KS_DBG_AGG_CAP)) { // (tests: full tables, wrapping probe chains and the overflow on small inputs)
        const long v = atol(f);
        if (v >= 1 && v < AG_SLOTS) agg_slots = (u32)v;
    }
    // The row count is only known on the device here.  Instead of a round trip before the pass, the row arrays take
    // their size from the previous search of this context (+ 25 %) and the count is read with the final
    // synchronisation; a search that produced more rows than that repeats the (cheap) pass with exact arrays.
    u64 rows_cap = n_pairs;
    if (ctx->rows_hint && ctx->rows_hint < rows_cap && !ks_dbg(ctx, KS_DBG_NO_ROWS_HINT)) rows_cap = ctx->rows_hint;
    u32 n_rows = 0;
    bool settled = false;
    struct se_cols_scope : ks_hit_cols { // the filtered columns (Q.min_c > 0, se_rows_post) until they replace H's: released on every way out
        ks_ctx *ctx;
        explicit se_cols_scope(ks_ctx *c) : ks_hit_cols{}, ctx(c) {}
        ~se_cols_scope() { release(ctx); }
    } F(ctx);
    const u32 *pin = (const u32 *)(ctx->h_pin + KS_PIN_ROWS); // ticket pair | row count | kept rows (min_containment)
    const bool post = Q.stats || Q.min_c > 0;
    for (int attempt = 0; attempt < 3; attempt++) { // (repeats: more rows than the guess; a look-back that gave up)
        ks_scratch sc(ctx); // (the statistics' and the filter's scratch of this attempt)
        H->release(ctx); F.release(ctx); // (what the attempt before this one left)
        KS_TRY(ks_alloc(ctx, &H->d_qid, (size_t)rows_cap)); KS_TRY(ks_alloc(ctx, &H->d_tid, (size_t)rows_cap));
        // n_weighted (u64) | status words + ticket pair + row count + kept count (u64) | intersect (u32): one block, zeroed
        // together, per attempt (one memset, one read-back)
        const size_t st_words = (size_t)pf_tiles + 2, is_words = ((size_t)rows_cap + 1) / 2;
        KS_TRY(ks_alloc(ctx, &H->d_block, (size_t)rows_cap + st_words + is_words));
        H->d_nw = H->d_block;
        H->d_isect = (u32 *)(H->d_block + rows_cap + st_words);
        unsigned long long *const pf_status = (unsigned long long *)(H->d_block + rows_cap);
        u32 *const pf_ticket = (u32 *)(pf_status + pf_tiles);
        KS_HIP(ctx, hipMemsetAsync(H->d_block, 0, ((size_t)rows_cap + st_words + is_words) * sizeof(u64), ctx->stream));
        if (A)
            KS_LAUNCH(ctx, "pairs_aggregate", k_pairs_aggregate, pf_tiles, AG_THREADS, (const u64 *)A->kb, A->ends, agg_slots, H->d_qid,
                      H->d_tid, H->d_isect, (unsigned long long *)H->d_nw, tbits, abits, (u32)rows_cap, pf_status, pf_ticket);
        else
            KS_LAUNCH(ctx, "pair_rows", k_pair_rows_fused, pf_tiles, PF_THREADS, pk, n_pairs, H->d_qid, H->d_tid, H->d_isect,
                      (unsigned long long *)H->d_nw, tbits, abits, (u32)rows_cap, pf_status, pf_ticket, pf_ticket + 2,
                      (ctx->rows_use_ticket || ks_dbg(ctx, KS_DBG_ROWS_TICKET)) ? 1 : 0);
        if (post) KS_TRY(se_rows_post(ctx, Q, H, F, pk, (u32)rows_cap, pf_ticket, sc));
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ks_fetch_words(pf_ticket, ctx->h_pin + KS_PIN_ROWS, 4)})); // ticket pair + row count + kept count
        if (A && (pin[0] != 0 || pin[1] != 0)) { // a table overflowed / a region waited in vain: no rows from here
            H->release(ctx);
            *fell_back = true;
            return KS_OK;
        }
        bool gave_up = pin[1] != 0;
        if (!A && ks_dbg(ctx, KS_DBG_FORCE_ROWS_TICKET_RETRY) && !ctx->rows_use_ticket) gave_up = true; // (tests)
        if (gave_up) {
            if (ctx->rows_use_ticket || attempt == 2) return ks_fail(ctx, KS_ERR_HIP, "search: row look-back gave up waiting for a predecessor tile");
            ctx->rows_use_ticket = true; // dispatch order did not hold here: tickets from now on
            ctx->rows_ticket_fallbacks++;
        } else {
            n_rows = pin[2];
            if (n_rows <= rows_cap) { settled = true; break; }
            rows_cap = n_rows;
        }
    }
    if (!settled) return ks_fail(ctx, KS_ERR_HIP, "search: the row pass did not settle");
    H->n_hits = n_rows;
    const u64 want = (u64)n_rows + n_rows / 4 + 4096;
    ctx->rows_hint = want > ctx->rows_hint / 2 ? want : ctx->rows_hint / 2; // follows growth at once, decays slowly
    ctx->rows_mult = (double)n_pairs / (double)(n_rows ? n_rows : 1u); // (ks_rows_agg_wanted: the next search's path)
    if (A) ctx->agg_used++;
    if (Q.min_c > 0) { // the kept rows replace the row pass's columns
        H->take(ctx, F);
        H->n_hits = pin[3];
    }
    return KS_OK;
}

int ks_search_rows(ks_ctx *ctx, const ks_rows_in &Q, ks_hits *H, const u64 *pk) {
    if (Q.n_pairs == 0) return H->alloc(ctx, 0, H->has_stats, 0);
    return se_rows_run(ctx, Q, H, pk, nullptr, nullptr);
}

int ks_search_rows_agg(ks_ctx *ctx, const ks_rows_in &Q, ks_hits *H, const ks_msd_plan &P, bool *fell_back) {
    *fell_back = false;
    return se_rows_run(ctx, Q, H, nullptr, &P, fell_back);
}
