// ks_cluster.hip — ks_hits_cluster: the connected components of a hit list read as a graph (the `pairwise` + `cluster` step of the
// sourmash / branchwater tool family).  Nodes 0 .. n-1 are the sequences of one set; row r = (q, t) is an undirected edge iff
// q != t and score(r) >= threshold, the score being ks_hits_best's (ks_score.h: one definition for both passes).
//
//   init      a lane per node: parent[i] = i, sizes and representative keys zeroed
//   hook      a lane per hit row: score, threshold, ids and sizes checked (atomicMin of the first bad row, as k_best_keys does);
//             an edge finds its two roots with path halving and links the larger root under the smaller by compare-and-swap
//   flatten   a lane per node, a launch of its own: follow parent to the root -> label
//   compact   root flags label[i] == i -> one-launch exclusive scan -> cluster_id; per node one integer atomicAdd on its
//             cluster's size, one atomicMax on its cluster's packed (distinct hashes << 32 | ~id), the key cluster_id << 32 | id;
//             (both once per wave and cluster); sizes scanned to offsets (ks_scan_u32_to_u64), keys sorted stably on the live
//             bits of the cluster id (ks_radix_sort_keys) -> members
//   finish    members and representatives unpacked, the largest size by atomicMax; the scalars come back with the one wait
// compact and finish are ks_clusters_from_labels (ks_common.h): the tail of ks_hits_cluster_greedy (ks_greedy.hip) too, whose
// labels mark their roots the same way (label[i] == i).
//
// The union-find is lock-free on parent u32[n] (0.8 MB at 200k nodes: cache-resident).  Its correctness argument:
//   * parent[x] <= x always.  parent starts as the identity, and
//   * every write to parent inside the hook launch is an agent-scope atomic that can only lower the entry: a compare-and-swap of
//     parent[hi] from hi to lo < hi (a link), or an atomicMin with an ancestor of x (path halving).
//   * every read of parent inside the hook launch is a relaxed agent-scope atomic load.
//   * correctness never rests on a load being fresh.  The L2s of the XCDs are not coherent with each other: a load may return an
//     older value.  Entries only ever move to ancestors and trees only ever grow upwards, so a stale value is an older ancestor
//     in the same component, and that is enough: a "root" that is none any more is either the larger of the pair — the
//     compare-and-swap fails and returns its parent — or the smaller, and linking under a non-root of the right component with a
//     smaller id is still a valid link.  Correctness rests only on the value the compare-and-swap returns.
//   * no wave ever waits for another wave: no spin, no flag, no ticket.  A walk towards the root moves to a strictly smaller id
//     every step, and a failed compare-and-swap returns a value < hi, so the larger root of the pair strictly decreases: a lane's
//     loop is bounded whatever the schedule.
//   * therefore every non-root has a parent with a smaller id: the root of every tree is its smallest id.  When a lane is done
//     with an edge, both ends are in one tree; nothing ever splits a tree.  The trees are the components and the final label —
//     the smallest id of the component — does not depend on the order in which rows, lanes or waves ran.
// Everything after the hook is integers: counts, scans, a key sort.  No f64 atomics, no score reductions: the result never
// depends on the path (KS_DEBUG_CLUSTER_PATH), the launch geometry or the schedule.
//
// Wave-uniform query path (gfx950, 64-lane waves): rows are ordered by (qid, tid), so the 64 rows of a wave usually share one
// qid.  The lanes with an edge ballot `qid == the first such lane's qid`; if all agree, one lane walks to the query's root and
// broadcasts it, and every lane links its tid to that root instead of repeating the same pointer chase 64 times.  Measured on
// the 200k all-vs-all (tools/cluster_bench.py; the table in DESIGN.md §3.3f) it does not beat the plain lane-per-row path by more than the box-to-box noise (64 lanes that load one
// address are one memory request already), so the plain path is the default and this one stays behind the knob:
// KS_DEBUG_CLUSTER_PATH = 1 the plain path for every wave, 2 the wave-uniform path wherever a wave's edges share the query.
#include "ks_score.h"

#define CL_WAVE_UNIFORM_DEFAULT 0 // the wave-uniform query path did not beat the plain one by more than the noise: behind the knob
#define CL_HOOK_WG_PER_CU 8 // workgroups of k_cluster_hook per CU: 32 waves, what a CU holds

struct cl_in {
    const u32 *qid, *tid, *isect;
    const double *score;
    u32 n_rows, similarity, n;
    double threshold;
    bh_set sizes; // off == NULL: no node set
};

KS_DEV u32 cl_load(const u32 *parent, u32 x) { return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// An ancestor of x that was a root when it was read.  Path halving: x's entry moves to its grandparent (atomicMin: the entry
// only goes down, a concurrent lower value stays).  p < x and g <= p: x strictly decreases.
KS_DEV u32 cl_find(u32 *parent, u32 x) {
    for (;;) {
        const u32 p = cl_load(parent, x);
        if (p == x) return x;
        const u32 g = cl_load(parent, p);
        if (g != p) (void)__hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// a and b into one tree.  max(a, b) strictly decreases over the iterations.
KS_DEV void cl_unite(u32 *parent, u32 a, u32 b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const u32 hi = a > b ? a : b, lo = a > b ? b : a;
        u32 seen = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = seen; // hi had a parent already (seen < hi): go on from there
        b = lo;
    }
}

__global__ __launch_bounds__(256) void k_cluster_init(u32 n, u32 *parent, u32 *sizes, u64 *rep) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    sizes[i] = 0u;
    rep[i] = 0ULL;
}

// A fixed grid strides over the rows, 256 consecutive rows per workgroup and round (the trip count is uniform over a
// workgroup).  The rows that passed are counted in registers and leave the workgroup as ONE atomicAdd: one add per wave of
// rows on the one counter cost 2.3 of this kernel's 2.4 ms on the 31.6 M rows of the 200k all-vs-all (first version).
__global__ __launch_bounds__(256) void k_cluster_hook(cl_in R, int wave_uniform, u32 *parent, unsigned long long *ctl) {
    __shared__ u32 s_passed[4];
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
        const u64 me = __ballot(edge);
        if (!me) continue;
        if (wave_uniform) {
            const int leader = __ffsll((long long)me) - 1;
            const u32 q0 = (u32)__shfl((int)q, leader);
            if (__ballot(edge && q == q0) == me && (me & (me - 1))) { // one query, more than one edge: its root once
                u32 rq = 0;
                if ((int)lane == leader) rq = cl_find(parent, q0);
                rq = (u32)__shfl((int)rq, leader);
                if (edge) cl_unite(parent, rq, t);
                continue;
            }
        }
        if (edge) cl_unite(parent, q, t);
    }
    if (lane == 0) s_passed[threadIdx.x >> 6] = n_passed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 sum = (u64)s_passed[0] + s_passed[1] + s_passed[2] + s_passed[3];
        if (sum) atomicAdd(&ctl[CL_EDGES], (unsigned long long)sum);
    }
}

// the kernel boundary made the table visible: plain loads
__global__ __launch_bounds__(256) void k_cluster_flatten(u32 n, const u32 *parent, u32 *label, u32 *flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 x = i, p = parent[x];
    while (p < x) { x = p; p = parent[x]; } // (a non-root's parent is smaller; a root's is itself)
    label[i] = x;
    flag[i] = x == i ? 1u : 0u;
}

// root_idx: the exclusive scan of the root flags.  The lanes of a wave that share a cluster add their count and their best
// representative key with ONE atomic each (a giant cluster is one address: an atomic per node on it cost 3.3 ms at 200k nodes: DESIGN.md §3.3f).
__global__ __launch_bounds__(256) void k_cluster_ids(u32 n, const u32 *label, const u32 *root_idx, bh_set S, u32 *cluster_id, u32 *sizes, u64 *rep,
                                                     u64 *key) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = i < n;
    u32 c = 0;
    u64 pk = 0;
    if (live) {
        const u32 root = label[i] < n ? label[i] : i;
        c = root_idx[root] < n ? root_idx[root] : 0u;
        cluster_id[i] = c;
        key[i] = ((u64)c << 32) | i;
        const u64 nh = S.off ? bh_size(S, i) : 0ULL; // without a node set every member ties: the smallest id wins
        pk = ((nh < 0xffffffffULL ? nh : 0xffffffffULL) << 32) | (u32)~i;
    }
    u64 todo = __ballot(live);
    while (todo) { // (wave-uniform: one round per distinct cluster among the wave's nodes)
        const int leader = __ffsll((long long)todo) - 1;
        const u32 c0 = (u32)__shfl((int)c, leader);
        const bool mine = live && c == c0;
        const u64 grp = __ballot(mine);
        u64 best = mine ? pk : 0ULL;
        if (grp & (grp - 1)) {
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                const u64 o = ((u64)(u32)__shfl_xor((int)(u32)(best >> 32), d) << 32) | (u32)__shfl_xor((int)(u32)best, d);
                best = o > best ? o : best;
            }
        }
        if ((int)lane == leader) {
            atomicAdd(&sizes[c0], (u32)__popcll(grp));
            atomicMax((unsigned long long *)&rep[c0], (unsigned long long)best);
        }
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(256) void k_cluster_finish(u32 n, const u64 *sorted, const u32 *sizes, const u64 *rep, u32 *members, u32 *representative,
                                                        unsigned long long *ctl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    u32 sz = 0;
    if (i < n) {
        members[i] = (u32)sorted[i];
        sz = sizes[i];
        representative[i] = sz ? ~(u32)rep[i] : 0u; // (entries past n_clusters: 0)
    }
    sz = ks_wave_max_u32(sz);
    if ((threadIdx.x & 63) == 0 && sz) atomicMax(&ctl[CL_LARGEST], (unsigned long long)sz);
}

int ks_clusters_alloc(ks_ctx *ctx, ks_clusters *K, u32 n) {
    K->n_nodes = n; K->n_clusters = 0; K->largest = 0; K->n_edges = 0;
    KS_TRY(ks_alloc(ctx, &K->d_label, (size_t)n)); KS_TRY(ks_alloc(ctx, &K->d_cluster_id, (size_t)n));
    KS_TRY(ks_alloc(ctx, &K->d_members, (size_t)n)); KS_TRY(ks_alloc(ctx, &K->d_rep, (size_t)n));
    return ks_alloc(ctx, &K->d_offsets, (size_t)n + 1);
}

int ks_clusters_from_labels(ks_ctx *ctx, ks_clusters *K, const ks_sketches *N, const ks_label_scratch &W, const ks_ctl &ctl) {
    const u32 n = K->n_nodes, g_n = (n + 255) / 256;
    KS_TRY(ks_scan_u32_inplace(ctx, W.root_idx, n, ctl.low32(CL_CLUSTERS)));
    KS_LAUNCH(ctx, "cluster_ids", k_cluster_ids, g_n, 256, n, (const u32 *)K->d_label, (const u32 *)W.root_idx, bh_set_of(N), K->d_cluster_id, W.sizes, W.rep,
              W.ka);
    KS_TRY(ks_scan_u32_to_u64(ctx, W.sizes, K->d_offsets, n));
    // members: the keys are written in id order, so a STABLE sort on the cluster id alone leaves them ordered by (cluster, id).
    // LSD passes on the live bits of the id field — not ks_sort_live_keys: its MSD variant partitions on the top bits, and a
    // giant cluster is one bucket that a single workgroup then sorts (2.2 ms at 200k nodes in one component; these passes
    // do not care how the ids are distributed).
    int shifts[4], ns = 0;
    for (int sh = 0; sh < ks_key_bits((u64)n - 1); sh += 8) shifts[ns++] = 32 + sh;
    u64 *sorted = nullptr;
    KS_TRY(ks_radix_sort_keys(ctx, KS_SORT_PAIRS, W.ka, W.ka, W.kb, n, shifts, ns, &sorted));
    KS_LAUNCH(ctx, "cluster_finish", k_cluster_finish, g_n, 256, n, (const u64 *)sorted, (const u32 *)W.sizes, (const u64 *)W.rep, K->d_members, K->d_rep,
              ctl.words());
    return KS_OK;
}

int ks_clusters_finish(ks_ctx *ctx, const char *what, ks_clusters *K, const ks_ctl &ctl) {
    const u32 n = K->n_nodes;
    if (ctl.bad(CL_BAD_ID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: hit row %llu names a node beyond the %u nodes of the set", what, (unsigned long long)ctl[CL_BAD_ID], n);
    if (ctl.bad(CL_BAD_SIZE))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: hit row %llu names an empty sketch: its score divides by 0", what, (unsigned long long)ctl[CL_BAD_SIZE]);
    if (ctl[CL_CLUSTERS] == 0 || ctl[CL_CLUSTERS] > n || ctl[CL_LARGEST] > n)
        return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu clusters, the largest of %llu, on %u nodes", (unsigned long long)ctl[CL_CLUSTERS],
                       (unsigned long long)ctl[CL_LARGEST], n);
    K->n_edges = ctl[CL_EDGES];
    K->n_clusters = (u32)ctl[CL_CLUSTERS];
    K->largest = (u32)ctl[CL_LARGEST];
    return KS_OK;
}

static int cluster_run(ks_ctx *ctx, const ks_hits *H, const ks_sketches *N, const double *d_score, const ks_cluster_opts *o, ks_clusters *K) {
    const u64 n64 = H->n_hits;
    if (n64 >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "cluster: 2^32 - 2 or more hit rows");
    const u32 n_rows = (u32)n64, n = N ? N->n_seqs : o->n_nodes;
    KS_TRY(ks_clusters_alloc(ctx, K, n));
    if (n == 0) {
        if (n_rows) return ks_fail(ctx, KS_ERR_INVALID_ARG, "cluster: hit row 0 names a node beyond the 0 nodes of the set");
        KS_HIP(ctx, hipMemsetAsync(K->d_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    int wave_uniform = CL_WAVE_UNIFORM_DEFAULT;
    if (const char *f = ks_dbg(ctx, KS_DBG_CLUSTER_PATH)) { // (tests, tools/cluster_bench.py: every wave one way)
        const int v = atoi(f);
        if (v == 1) wave_uniform = 0;
        else if (v == 2) wave_uniform = 1;
    }

    ks_scratch sc(ctx);
    u32 *parent = nullptr;
    ks_label_scratch W = {};
    ks_ctl ctl; // [CL_BAD_ID], [CL_BAD_SIZE]: the first such row; the three counts
    KS_TRY(sc.alloc(&parent, (size_t)n)); KS_TRY(sc.alloc(&W.root_idx, (size_t)n)); KS_TRY(sc.alloc(&W.sizes, (size_t)n));
    KS_TRY(sc.alloc(&W.rep, (size_t)n)); KS_TRY(sc.alloc(&W.ka, (size_t)n)); KS_TRY(sc.alloc(&W.kb, (size_t)n));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_CLUSTER, 2, 3));

    const u32 g_n = (n + 255) / 256;
    KS_LAUNCH(ctx, "cluster_init", k_cluster_init, g_n, 256, n, parent, W.sizes, W.rep);
    if (n_rows) {
        const cl_in R = {H->d_qid, H->d_tid, H->d_isect, d_score, n_rows, o->similarity, n, o->threshold, bh_set_of(N)};
        const u32 g_rows = (n_rows + 255) / 256, g_max = (u32)ctx->n_cus * CL_HOOK_WG_PER_CU;
        KS_LAUNCH(ctx, "cluster_hook", k_cluster_hook, g_rows < g_max ? g_rows : g_max, 256, R, wave_uniform, parent, ctl.words());
    }
    KS_LAUNCH(ctx, "cluster_flatten", k_cluster_flatten, g_n, 256, n, (const u32 *)parent, K->d_label, W.root_idx);
    KS_TRY(ks_clusters_from_labels(ctx, K, N, W, ctl));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    return ks_clusters_finish(ctx, "cluster", K, ctl);
}

int ks_cluster_words_check(ks_ctx *ctx, const char *what, u32 similarity, u32 n_nodes, double threshold, const ks_sketches *nodes,
                           const double *d_score) {
    const auto bad = [&](const char *why) { return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "%s options: %s", what, why) : KS_ERR_INVALID_ARG; };
    if (similarity > KS_BEST_SCORE) return bad("unknown similarity");
    if (threshold != threshold) return bad("the threshold is NaN");
    if (similarity == KS_BEST_SCORE && !d_score) return bad("KS_BEST_SCORE needs a score column");
    if (similarity != KS_BEST_SCORE && d_score) return bad("a score column is only read with KS_BEST_SCORE");
    const bool need_sizes = similarity == KS_BEST_TARGET_CONTAINMENT || similarity == KS_BEST_MAX_CONTAINMENT || similarity == KS_BEST_JACCARD;
    if (need_sizes && !nodes) return bad("this similarity needs the node sketches");
    if (nodes && n_nodes != 0 && n_nodes != nodes->n_seqs) return bad("n_nodes is not the node set's sequence count");
    return KS_OK;
}

// the option words and what they ask of the other arguments; ctx may be NULL
static int cluster_opts_check(ks_ctx *ctx, const ks_cluster_opts *o, const ks_sketches *nodes, const double *d_score) {
    if (!o) return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "cluster options: NULL") : KS_ERR_INVALID_ARG;
    KS_TRY(ks_opts_words_check(ctx, "cluster", o->flags, 0, o->reserved));
    return ks_cluster_words_check(ctx, "cluster", o->similarity, o->n_nodes, o->threshold, nodes, d_score);
}

extern "C" int ks_hits_cluster(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *nodes, const double *d_score, const ks_cluster_opts *opts,
                               ks_clusters **out) {
    return ks_guard(ctx, [&]() -> int {
    if (out) *out = nullptr;
    KS_TRY(cluster_opts_check(ctx, opts, nodes, d_score));
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (!hits || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "cluster", hits, nodes));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_result<ks_clusters> K(ctx, out, ks_clusters_free);
    KS_TRY(cluster_run(ctx, hits, nodes, d_score, opts, K));
    return K.commit();
    });
}

extern "C" uint32_t ks_clusters_n_nodes(const ks_clusters *c) { return c ? c->n_nodes : 0; }
extern "C" uint32_t ks_clusters_n_clusters(const ks_clusters *c) { return c ? c->n_clusters : 0; }
extern "C" uint64_t ks_clusters_n_edges(const ks_clusters *c) { return c ? c->n_edges : 0; }
extern "C" uint32_t ks_clusters_largest(const ks_clusters *c) { return c ? c->largest : 0; }
extern "C" uint32_t ks_clusters_n_rounds(const ks_clusters *c) { return c ? c->n_rounds : 0; }
extern "C" const uint32_t *ks_clusters_device_label(const ks_clusters *c) { return c ? c->d_label : nullptr; }
extern "C" const uint32_t *ks_clusters_device_cluster_id(const ks_clusters *c) { return c ? c->d_cluster_id : nullptr; }
extern "C" const uint64_t *ks_clusters_device_offsets(const ks_clusters *c) { return c ? c->d_offsets : nullptr; }
extern "C" const uint32_t *ks_clusters_device_members(const ks_clusters *c) { return c ? c->d_members : nullptr; }
extern "C" const uint32_t *ks_clusters_device_representative(const ks_clusters *c) { return c ? c->d_rep : nullptr; }

extern "C" int ks_clusters_copy_to_host(ks_ctx *ctx, const ks_clusters *c, uint32_t *label, uint32_t *cluster_id, uint64_t *offsets, uint32_t *members,
                                        uint32_t *representative) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, c, label, cluster_id, offsets, members, representative); });
}

extern "C" void ks_clusters_free(ks_clusters *c) { ks_obj_free(c); }
