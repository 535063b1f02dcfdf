// ks_greedy.hip — ks_hits_cluster_greedy: greedy representative clustering of a hit list read as a graph (what CD-HIT's
// incremental clustering and the greedy set-cover modes of MMseqs2 / linclust compute).  Nodes, edges and scores are those of
// ks_hits_cluster (ks_score.h: one definition).  The nodes are taken in priority order — more distinct hashes first, ties and
// no node set: the smaller id first; a node none of whose neighbours of higher priority is a representative becomes one, every
// other node joins a representative it has a passing row with.  The set of representatives is the lexicographically first
// maximal independent set of the graph under the priority order: it is unique, so it cannot depend on the schedule.
//
//   rank      key (~distinct hashes << 32) | id, written in id order, sorted stably on the live bits of the size field
//             (ks_radix_sort_keys) -> order[rank] = node, rank[node]; without a node set rank[v] = v and nothing is sorted
//   edges     a lane per hit row over a fixed grid: ids and sizes checked, row scored, rows that passed counted in registers
//             (as k_cluster_hook does); a passing non-self row is appended as a (u32, u32) pair to the live list — one atomicAdd
//             per workgroup and 256 rows — and, every node being undecided, is round 1's row step at once: its end of lower
//             priority is stamped
//   rounds    state[v] = UNDECIDED | REP | MEMBER.  Round r, row step over the live edges: an UNDECIDED end beside a REP becomes
//             MEMBER; on an edge with both ends UNDECIDED the end of lower priority gets stamp[v] = r and the edge goes to the
//             other live list (ping-pong); every other edge is dead.  Node step: an UNDECIDED node whose stamp is not r becomes
//             REP; the others are counted.  GR_ROUNDS_PER_WAIT rounds are queued per host look at that count (a round after the
//             last one finds nothing to do).
//   tail      once at most GR_TAIL_EDGES edges are live, ONE workgroup runs all remaining rounds in one launch: row step,
//             __syncthreads(), node step driven by the edges it just read, __syncthreads().
//   assign    a lane per hit row again, with the final states (not over the live list: the edges to a representative that was
//             decided late are long dead): ASSIGN_FIRST atomicMin(best_rank[member], rank[rep]) over the passing rows with a
//             REP and a MEMBER end; ASSIGN_BEST first atomicMax of the order-preserving u64 image of the row's f64 score
//             (-0.0 as +0.0), then atomicMin of the rank among the rows whose image is that maximum
//   label     label[v] = v for a REP, order[best_rank[v]] for a MEMBER; root flags -> the tail ks_hits_cluster ends with
//             (ks_clusters_from_labels: cluster ids, CSR, sizes); the representative of a cluster is its root
//
// Why the rounds are right, whatever the schedule:
//   * state only ever moves UNDECIDED -> REP (node step) or UNDECIDED -> MEMBER (row step), never back.
//   * an edge leaves the live list only when one end was read as REP or MEMBER.  A REP beside an UNDECIDED end makes that end
//     MEMBER in the same step, so an edge that has died never ran between an UNDECIDED node and a REP that still had to act.
//   * a node is only ever made MEMBER beside a node that was read as REP, and REP is only written by a node step: a kernel
//     boundary (or, in the tail, a workgroup barrier) lies between that write and every read.
//   * a node v is promoted in round r only if it is UNDECIDED after the row step and stamp[v] != r.  Every edge (v, w) to a
//     neighbour w of higher priority is either dead — then w was read as MEMBER (had it been REP, v would be MEMBER) — or was
//     read in round r: w read as UNDECIDED stamps v, as REP makes v MEMBER, as MEMBER kills the edge.  So v is promoted only when
//     every neighbour of higher priority is MEMBER: the sequential rule.
//   * a read of `state` inside a row step may be stale or concurrent with another lane's write: the L2s of the XCDs are not
//     coherent with each other.  The only write of that step is UNDECIDED -> MEMBER, so such a read can only return UNDECIDED
//     for a node that is MEMBER already.  That keeps an edge alive and stamps a node that needed no stamp: a promotion is put
//     off by a round, never made wrongly.  Writes of one round are visible in the next: a kernel boundary lies between them.
//   * after any node step every UNDECIDED node carries that round's stamp, so it is an end of an edge of the new live list: the
//     tail can find every node still in play through the edges.
//   * the UNDECIDED node of highest priority has no UNDECIDED neighbour above it: the round decides it (REP, or MEMBER beside a
//     REP).  Every round decides a node, the loop ends after at most n rounds — a path in priority order is the worst case.
//   * no wave ever waits for another wave: no spin, no flag, no ticket.
// Everything after the scores is integers (counts, integer atomics on ranks and score images, scans, a key sort): the result
// depends on neither the path (KS_DEBUG_GREEDY_PATH = 1 grid rounds only, 2 the tail straight after the edge kernel and its
// node step), the launch geometry nor the schedule.  Only the round count (ks_clusters_n_rounds) may.
//
// Scratch, from the pool: 60 bytes per node (state, stamp, rank, order, best_rank u32; best_img u64; the tail's 32: two u32, a
// u64, two u64 key buffers that the rank sort uses first); the first live list is sized before the scores are known, 8 bytes
// per hit row, the second one after the edge kernel's wait, 8 bytes per passing non-self row — the two ping-pong lists are
// 16 bytes per passing row when every row passes.
#include "ks_score.h"

#define GR_TAIL_EDGES 8192u   // at most this many live edges: one workgroup finishes (measured crossover 4k - 16k: DESIGN.md §3.3h)
#define GR_ROUNDS_PER_WAIT 4  // grid rounds queued per host look at the undecided count
#define GR_WG_PER_CU 8        // workgroups of the row kernels per CU, as k_cluster_hook
#define GR_TAIL_THREADS 1024
enum { GR_LIVE = 5 /* and 6: the lengths of the two live lists */, GR_UNDECIDED = 7, GR_ROUNDS = 8, GR_ORPHANS = 9, GR_WORDS = 10 };
enum : u32 { GR_ST_UNDECIDED = 0u, GR_ST_REP = 1u, GR_ST_MEMBER = 2u };
enum { GR_MODE_FIRST = 0, GR_MODE_BEST_MAX = 1, GR_MODE_BEST_MIN = 2 };
#define GR_NONE 0xffffffffu

struct gr_in {
    const u32 *qid, *tid, *isect;
    const double *score;
    u32 n_rows, similarity, n;
    double threshold;
    bh_set sizes; // off == NULL: no node set
};

// monotone u64 image of a score that passed (never NaN); -0.0 and +0.0 share one image; 0 is below every image
KS_DEV u64 gr_score_image(double s) {
    u64 b = (u64)__double_as_longlong(s);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

template <int SCOPE> KS_DEV u32 gr_load(const u32 *state, u32 v) { return __hip_atomic_load(&state[v], __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE> KS_DEV void gr_store(u32 *state, u32 v, u32 x) { __hip_atomic_store(&state[v], x, __ATOMIC_RELAXED, SCOPE); }

// The row step on one live edge: true iff the edge stays alive (both ends read as UNDECIDED; its end of lower priority is stamped).
template <int SCOPE> KS_DEV bool gr_edge_step(u32 a, u32 b, u32 round, const u32 *rank, u32 *state, u32 *stamp) {
    const u32 sa = gr_load<SCOPE>(state, a), sb = gr_load<SCOPE>(state, b);
    if (sa == GR_ST_UNDECIDED && sb == GR_ST_UNDECIDED) {
        stamp[rank[a] > rank[b] ? a : b] = round;
        return true;
    }
    if (sa == GR_ST_UNDECIDED && sb == GR_ST_REP) gr_store<SCOPE>(state, a, GR_ST_MEMBER);
    else if (sb == GR_ST_UNDECIDED && sa == GR_ST_REP) gr_store<SCOPE>(state, b, GR_ST_MEMBER);
    return false;
}

// The kept pairs of the 256 lanes of a workgroup go to out[] behind ONE atomicAdd on *count.  Every lane of the workgroup calls.
KS_DEV void gr_append(bool keep, u32 a, u32 b, uint2 *out, u32 cap, unsigned long long *count, u32 *s_cnt, u32 *s_base) {
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 m = __ballot(keep);
    if (lane == 0) s_cnt[w] = (u32)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        *s_base = total ? (u32)atomicAdd(count, (unsigned long long)total) : 0u;
    }
    __syncthreads();
    if (keep) {
        u32 pos = *s_base + (u32)__popcll(m & ((1ULL << lane) - 1ULL));
        for (u32 i = 0; i < w; i++) pos += s_cnt[i];
        if (pos < cap) out[pos] = make_uint2(a, b);
    }
    __syncthreads(); // (s_cnt and s_base are written again by the next 256 rows)
}

__global__ __launch_bounds__(256) void k_greedy_init(u32 n, bh_set S, u32 *state, u32 *stamp, u32 *best_rank, u64 *best_img, u32 *sizes, u64 *rep,
                                                     u64 *key, u32 *rank, u32 *order) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    state[i] = GR_ST_UNDECIDED;
    stamp[i] = 0u;
    best_rank[i] = GR_NONE;
    best_img[i] = 0ULL;
    sizes[i] = 0u;
    rep[i] = 0ULL;
    if (S.off) {
        const u64 nh = bh_size(S, i);
        key[i] = ((u64)(u32)~(u32)(nh < 0xffffffffULL ? nh : 0xffffffffULL) << 32) | i;
    } else {
        rank[i] = i;
        order[i] = i;
    }
}

__global__ __launch_bounds__(256) void k_greedy_rank(u32 n, const u64 *sorted, u32 *rank, u32 *order) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 v = (u32)sorted[i];
    order[i] = v;
    if (v < n) rank[v] = i;
}

// Rows as in k_cluster_hook: a fixed grid, 256 consecutive rows per workgroup and trip (the trip count is uniform over a
// workgroup), the rows that passed counted in registers.  live has room for n_rows pairs: a row appends at most one.
__global__ __launch_bounds__(256) void k_greedy_edges(gr_in R, const u32 *rank, u32 *stamp, uint2 *live, unsigned long long *ctl) {
    __shared__ u32 s_passed[4], s_cnt[4], s_base;
    const u32 lane = threadIdx.x & 63;
    u32 n_passed = 0; // (wave-uniform)
    for (u64 base = (u64)blockIdx.x * 256; base < R.n_rows; base += (u64)gridDim.x * 256) {
        const u64 r64 = base + threadIdx.x;
        const u32 r = (u32)r64;
        u32 q = 0, t = 0;
        bool passed = false;
        if (r64 < R.n_rows) {
            q = R.qid[r]; t = R.tid[r];
            if (q >= R.n || t >= R.n) ks_first_bad(ctl, CL_BAD_ID, r);
            else {
                bool bad_size;
                const double s = bh_row_score(R.similarity, r, q, t, R.isect[r], R.sizes, R.sizes, R.score, &bad_size);
                if (bad_size) ks_first_bad(ctl, CL_BAD_SIZE, r);
                else passed = s >= R.threshold; // (a NaN score never passes)
            }
        }
        n_passed += (u32)__popcll(__ballot(passed));
        const bool edge = passed && q != t;
        if (edge) stamp[rank[q] > rank[t] ? q : t] = 1u; // round 1: every node is undecided
        gr_append(edge, q, t, live, R.n_rows, &ctl[GR_LIVE], s_cnt, &s_base);
    }
    if (lane == 0) s_passed[threadIdx.x >> 6] = n_passed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 sum = (u64)s_passed[0] + s_passed[1] + s_passed[2] + s_passed[3];
        if (sum) atomicAdd(&ctl[CL_EDGES], (unsigned long long)sum);
    }
}

// Round `round` >= 2, row step: the live edges of in[] (their count is ctl[w_in], at most cap_in) -> out[] (ctl[w_out], zero on entry).
__global__ __launch_bounds__(256) void k_greedy_round(const uint2 *in, u32 cap_in, u32 w_in, uint2 *out, u32 cap_out, u32 w_out, u32 round, const u32 *rank,
                                                      u32 *state, u32 *stamp, unsigned long long *ctl) {
    __shared__ u32 s_cnt[4], s_base;
    const u64 have = ctl[w_in];
    const u32 cnt = have < cap_in ? (u32)have : cap_in;
    for (u64 base = (u64)blockIdx.x * 256; base < cnt; base += (u64)gridDim.x * 256) {
        const u64 i = base + threadIdx.x;
        uint2 e = make_uint2(0u, 0u);
        bool keep = false;
        if (i < cnt) {
            e = in[i];
            keep = gr_edge_step<__HIP_MEMORY_SCOPE_AGENT>(e.x, e.y, round, rank, state, stamp);
        }
        gr_append(keep, e.x, e.y, out, cap_out, &ctl[w_out], s_cnt, &s_base);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { // (the node step of the round before counted; this round's counts anew)
        if (ctl[GR_UNDECIDED]) ctl[GR_ROUNDS] = round;
        ctl[GR_UNDECIDED] = 0ULL;
    }
}

// Node step of round `round`; w_zero: the count of the list the round read — the next round appends to it.
__global__ __launch_bounds__(256) void k_greedy_promote(u32 n, u32 round, u32 w_zero, u32 *state, const u32 *stamp, unsigned long long *ctl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool undecided = false;
    if (i < n && state[i] == GR_ST_UNDECIDED) {
        if (stamp[i] != round) state[i] = GR_ST_REP;
        else undecided = true;
    }
    const u64 m = __ballot(undecided);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[GR_UNDECIDED], (unsigned long long)__popcll(m));
    if (i == 0) ctl[w_zero] = 0ULL;
}

// One workgroup, all remaining rounds from `round` on.  A node step has run (every undecided node is an end of a live edge),
// and the live edges are list[cur][0, ctl[GR_LIVE + cur]).  A round: row step over the edges, barrier, node step over the ends
// of the same edges, barrier.  The barriers make the writes of one step visible to the next (workgroup scope: one CU, one L1).
__global__ __launch_bounds__(GR_TAIL_THREADS) void k_greedy_tail(uint2 *list0, u32 cap0, uint2 *list1, u32 cap1, u32 cur, u32 round, const u32 *rank,
                                                                  u32 *state, u32 *stamp, unsigned long long *ctl) {
    __shared__ u32 s_next;
    const u32 lane = threadIdx.x & 63, first = round;
    const u64 have = ctl[GR_LIVE + cur];
    u32 cnt = have < (cur ? cap1 : cap0) ? (u32)have : (cur ? cap1 : cap0);
    while (cnt) {
        const uint2 *in = cur ? list1 : list0;
        uint2 *out = cur ? list0 : list1;
        const u32 cap_out = cur ? cap0 : cap1;
        if (threadIdx.x == 0) s_next = 0u;
        __syncthreads();
        for (u32 base = 0; base < cnt; base += GR_TAIL_THREADS) { // (uniform trip count)
            const u32 i = base + threadIdx.x;
            uint2 e = make_uint2(0u, 0u);
            bool keep = false;
            if (i < cnt) {
                e = in[i];
                keep = gr_edge_step<__HIP_MEMORY_SCOPE_WORKGROUP>(e.x, e.y, round, rank, state, stamp);
            }
            const u64 m = __ballot(keep);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                u32 at = 0;
                if ((int)lane == leader) at = atomicAdd(&s_next, (u32)__popcll(m));
                at = (u32)__shfl((int)at, leader) + (u32)__popcll(m & ((1ULL << lane) - 1ULL));
                if (keep && at < cap_out) out[at] = e;
            }
        }
        __syncthreads();
        for (u32 i = threadIdx.x; i < cnt; i += GR_TAIL_THREADS) {
            const uint2 e = in[i];
            if (gr_load<__HIP_MEMORY_SCOPE_WORKGROUP>(state, e.x) == GR_ST_UNDECIDED && stamp[e.x] != round) gr_store<__HIP_MEMORY_SCOPE_WORKGROUP>(state, e.x, GR_ST_REP);
            if (gr_load<__HIP_MEMORY_SCOPE_WORKGROUP>(state, e.y) == GR_ST_UNDECIDED && stamp[e.y] != round) gr_store<__HIP_MEMORY_SCOPE_WORKGROUP>(state, e.y, GR_ST_REP);
        }
        __syncthreads();
        cnt = s_next < cap_out ? s_next : cap_out;
        cur ^= 1u;
        round++;
        __syncthreads(); // (s_next is zeroed again at the top)
    }
    if (threadIdx.x == 0) {
        ctl[GR_UNDECIDED] = 0ULL;
        if (round > first) ctl[GR_ROUNDS] = round - 1;
    }
}

// The hit rows once more, with the final states.  The edge kernel has refused what is wrong: ids and sizes are checked only to stay in bounds.
__global__ __launch_bounds__(256) void k_greedy_assign(gr_in R, int mode, const u32 *state, const u32 *rank, u32 *best_rank, u64 *best_img) {
    for (u64 base = (u64)blockIdx.x * 256; base < R.n_rows; base += (u64)gridDim.x * 256) {
        const u64 r64 = base + threadIdx.x;
        if (r64 >= R.n_rows) continue;
        const u32 r = (u32)r64, q = R.qid[r], t = R.tid[r];
        if (q >= R.n || t >= R.n || q == t) continue;
        const u32 sq = state[q], st = state[t];
        u32 member, rep;
        if (sq == GR_ST_REP && st == GR_ST_MEMBER) { rep = q; member = t; }
        else if (st == GR_ST_REP && sq == GR_ST_MEMBER) { rep = t; member = q; }
        else continue;
        bool bad_size;
        const double s = bh_row_score(R.similarity, r, q, t, R.isect[r], R.sizes, R.sizes, R.score, &bad_size);
        if (bad_size || !(s >= R.threshold)) continue;
        if (mode == GR_MODE_BEST_MAX) atomicMax((unsigned long long *)&best_img[member], (unsigned long long)gr_score_image(s));
        else if (mode == GR_MODE_FIRST || gr_score_image(s) == best_img[member]) atomicMin(&best_rank[member], rank[rep]);
    }
}

// label and root flag per node; a node that is neither a representative nor beside one cannot be (counted: an internal error)
__global__ __launch_bounds__(256) void k_greedy_label(u32 n, const u32 *state, const u32 *best_rank, const u32 *order, u32 *label, u32 *flag,
                                                      unsigned long long *ctl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 l = i;
    if (state[i] == GR_ST_MEMBER && best_rank[i] < n) l = order[best_rank[i]];
    else if (state[i] != GR_ST_REP) atomicAdd(&ctl[GR_ORPHANS], 1ULL);
    label[i] = l < n ? l : i;
    flag[i] = l == i ? 1u : 0u;
}

// the representative of a greedy cluster is its root
__global__ __launch_bounds__(256) void k_greedy_reps(u32 n, const u32 *label, const u32 *cluster_id, u32 *representative) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && label[i] == i && cluster_id[i] < n) representative[cluster_id[i]] = i;
}

static int greedy_run(ks_ctx *ctx, const ks_hits *H, const ks_sketches *N, const double *d_score, const ks_greedy_opts *o, ks_clusters *K) {
    const u64 n64 = H->n_hits;
    if (n64 >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "cluster_greedy: 2^32 - 2 or more hit rows");
    const u32 n_rows = (u32)n64, n = N ? N->n_seqs : o->n_nodes;
    KS_TRY(ks_clusters_alloc(ctx, K, n));
    if (n == 0) {
        if (n_rows) return ks_fail(ctx, KS_ERR_INVALID_ARG, "cluster_greedy: hit row 0 names a node beyond the 0 nodes of the set");
        KS_HIP(ctx, hipMemsetAsync(K->d_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    int path = 0; // 0: grid rounds until GR_TAIL_EDGES edges are live, then the tail
    if (const char *f = ks_dbg(ctx, KS_DBG_GREEDY_PATH)) { // (tests, tools/greedy_bench.py)
        const int v = atoi(f);
        if (v == 1 || v == 2) path = v;
    }

    ks_scratch sc(ctx);
    u32 *state = nullptr, *stamp = nullptr, *rank = nullptr, *order = nullptr, *best_rank = nullptr;
    u64 *best_img = nullptr;
    uint2 *list[2] = {nullptr, nullptr};
    ks_label_scratch W = {};
    ks_ctl ctl; // the five words of ks_hits_cluster, then GR_LIVE .. GR_ORPHANS
    KS_TRY(sc.alloc(&state, (size_t)n)); KS_TRY(sc.alloc(&stamp, (size_t)n)); KS_TRY(sc.alloc(&rank, (size_t)n));
    KS_TRY(sc.alloc(&order, (size_t)n)); KS_TRY(sc.alloc(&best_rank, (size_t)n)); KS_TRY(sc.alloc(&best_img, (size_t)n));
    KS_TRY(sc.alloc(&W.root_idx, (size_t)n)); KS_TRY(sc.alloc(&W.sizes, (size_t)n)); KS_TRY(sc.alloc(&W.rep, (size_t)n));
    KS_TRY(sc.alloc(&W.ka, (size_t)n)); KS_TRY(sc.alloc(&W.kb, (size_t)n));
    KS_TRY(sc.alloc(&list[0], (size_t)n_rows));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_GREEDY, 2, GR_WORDS - 2));

    const u32 g_n = (n + 255) / 256, g_max = (u32)ctx->n_cus * GR_WG_PER_CU;
    const auto grid_of = [&](u64 items) { const u64 g = (items + 255) / 256; return (u32)(g < 1 ? 1 : g < g_max ? g : g_max); };
    const bh_set S = bh_set_of(N);
    KS_LAUNCH(ctx, "greedy_init", k_greedy_init, g_n, 256, n, S, state, stamp, best_rank, best_img, W.sizes, W.rep, W.ka, rank, order);
    if (N) { // keys in id order, a stable sort on the size field alone: ties keep the smaller id first
        const u64 most = N->n_slots > N->n_hashes ? N->n_slots : N->n_hashes; // no sketch holds more
        const int bits = most < 0xffffffffULL ? ks_key_bits(most) : 32;
        int shifts[4], ns = 0;
        for (int sh = 0; sh < bits; sh += 8) shifts[ns++] = 32 + sh;
        u64 *sorted = nullptr;
        KS_TRY(ks_radix_sort_keys(ctx, KS_SORT_PAIRS, W.ka, W.ka, W.kb, n, shifts, ns, &sorted));
        KS_LAUNCH(ctx, "greedy_rank", k_greedy_rank, g_n, 256, n, (const u64 *)sorted, rank, order);
    }
    const gr_in R = {H->d_qid, H->d_tid, H->d_isect, d_score, n_rows, o->similarity, n, o->threshold, S};
    if (n_rows) KS_LAUNCH(ctx, "greedy_edges", k_greedy_edges, grid_of(n_rows), 256, R, (const u32 *)rank, stamp, list[0], ctl.words());
    KS_LAUNCH(ctx, "greedy_promote", k_greedy_promote, g_n, 256, n, 1u, (u32)(GR_LIVE + 1), state, (const u32 *)stamp, ctl.words());
    const ks_fetch_seg seg = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &seg, 1));
    if (ctl.bad(CL_BAD_ID) || ctl.bad(CL_BAD_SIZE)) return ks_clusters_finish(ctx, "cluster_greedy", K, ctl);
    u64 live = ctl[GR_LIVE], undecided = ctl[GR_UNDECIDED];
    if (live > n_rows) return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu live edges from %u hit rows", (unsigned long long)live, n_rows);
    const u32 cap[2] = {n_rows, (u32)live};
    KS_TRY(sc.alloc(&list[1], (size_t)live));

    // round r >= 2 reads list[r & 1] and appends to the other one
    u32 round = 1;
    while (undecided) {
        const u32 cur = (round + 1) & 1u;
        if (path == 2 || (path == 0 && live <= GR_TAIL_EDGES)) {
            KS_LAUNCH(ctx, "greedy_tail", k_greedy_tail, 1, GR_TAIL_THREADS, list[0], cap[0], list[1], cap[1], cur, round + 1, (const u32 *)rank, state, stamp,
                      ctl.words());
            break;
        }
        if (round > n) return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu nodes undecided after %u rounds on %u nodes", (unsigned long long)undecided, round, n);
        for (int k = 0; k < GR_ROUNDS_PER_WAIT; k++) {
            round++;
            const u32 in = round & 1u, out = in ^ 1u;
            KS_LAUNCH(ctx, "greedy_round", k_greedy_round, grid_of(live), 256, (const uint2 *)list[in], cap[in], (u32)(GR_LIVE + in), list[out], cap[out],
                      (u32)(GR_LIVE + out), round, (const u32 *)rank, state, stamp, ctl.words());
            KS_LAUNCH(ctx, "greedy_promote", k_greedy_promote, g_n, 256, n, round, (u32)(GR_LIVE + in), state, (const u32 *)stamp, ctl.words());
        }
        KS_TRY(ks_stream_wait_fetch(ctx, &seg, 1));
        live = ctl[GR_LIVE + ((round + 1) & 1u)];
        undecided = ctl[GR_UNDECIDED];
    }

    if (n_rows) {
        if (o->assign == KS_GREEDY_ASSIGN_BEST) {
            KS_LAUNCH(ctx, "greedy_assign", k_greedy_assign, grid_of(n_rows), 256, R, (int)GR_MODE_BEST_MAX, (const u32 *)state, (const u32 *)rank, best_rank, best_img);
            KS_LAUNCH(ctx, "greedy_assign", k_greedy_assign, grid_of(n_rows), 256, R, (int)GR_MODE_BEST_MIN, (const u32 *)state, (const u32 *)rank, best_rank, best_img);
        } else {
            KS_LAUNCH(ctx, "greedy_assign", k_greedy_assign, grid_of(n_rows), 256, R, (int)GR_MODE_FIRST, (const u32 *)state, (const u32 *)rank, best_rank, best_img);
        }
    }
    KS_LAUNCH(ctx, "greedy_label", k_greedy_label, g_n, 256, n, (const u32 *)state, (const u32 *)best_rank, (const u32 *)order, K->d_label, W.root_idx, ctl.words());
    KS_TRY(ks_clusters_from_labels(ctx, K, N, W, ctl));
    KS_LAUNCH(ctx, "greedy_reps", k_greedy_reps, g_n, 256, n, (const u32 *)K->d_label, (const u32 *)K->d_cluster_id, K->d_rep);
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    if (ctl[GR_ORPHANS] || ctl[GR_UNDECIDED])
        return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu nodes without a representative, %llu undecided", (unsigned long long)ctl[GR_ORPHANS],
                       (unsigned long long)ctl[GR_UNDECIDED]);
    KS_TRY(ks_clusters_finish(ctx, "cluster_greedy", K, ctl));
    K->n_rounds = ctl[GR_ROUNDS] > 1 ? (u32)ctl[GR_ROUNDS] : 1u;
    return KS_OK;
}

// the option words and what they ask of the other arguments; ctx may be NULL
static int greedy_opts_check(ks_ctx *ctx, const ks_greedy_opts *o, const ks_sketches *nodes, const double *d_score) {
    const auto bad = [&](const char *why) { return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "cluster_greedy options: %s", why) : KS_ERR_INVALID_ARG; };
    if (!o) return bad("NULL");
    KS_TRY(ks_opts_words_check(ctx, "cluster_greedy", o->flags, 0, 0));
    if (o->assign > KS_GREEDY_ASSIGN_BEST) return bad("unknown assign mode");
    return ks_cluster_words_check(ctx, "cluster_greedy", o->similarity, o->n_nodes, o->threshold, nodes, d_score);
}

extern "C" int ks_hits_cluster_greedy(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *nodes, const double *d_score, const ks_greedy_opts *opts,
                                      ks_clusters **out) {
    return ks_guard(ctx, [&]() -> int {
    if (out) *out = nullptr;
    KS_TRY(greedy_opts_check(ctx, opts, nodes, d_score));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "cluster_greedy", hits, nodes));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_clusters> K(ctx, out, ks_clusters_free);
    KS_TRY(greedy_run(ctx, hits, nodes, d_score, opts, K));
    return K.commit();
    });
}

extern "C" uint32_t ks_debug_greedy_tail_edges(void) { return GR_TAIL_EDGES; }
