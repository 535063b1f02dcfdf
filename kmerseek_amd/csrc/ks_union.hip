// ks_union.hip — the unions of sketches.  ks_sketches_union (at the end: one sort + run-length reduce of the whole set) and
// ks_sketches_union_groups: the union of consecutive runs of sketches.  Group g of the host array group_offsets is the
// sketches [group_offsets[g], group_offsets[g + 1]) of the input set; its output sketch holds their distinct hashes, ascending,
// with the abundances of equal hashes summed and saturating at 2^32 - 1 (as ks_sketches_union, which folds the whole set into one
// sketch).  The six frames of a translated record are one group (ks_translate.hip); the proteins of a genome are another use.
//
// The input is made dense first (ks_sketches_make_dense), so group g's hashes are the span [off[go[g]], off[go[g + 1]]) of the hash
// array, member after member, each member ascending.  Both paths bring every span into (hash, member) order in place — the
// span's bounds do not move — as two columns: the hash, and (group << 32) | abundance.
//   rank path   every group has at most UN_RANK_MAX members.  A lane per hash: its place in the span is its index in its own
//               member plus, for every other member of the group, a binary-search count: the hashes <= it in an earlier member,
//               the hashes < it in a later one, so equal hashes keep member order.  A bijection, since a member's hashes are
//               distinct.  One kernel, no sort.  Cost per hash: (members - 1) searches over short, cached runs.
//   sort path   any group size.  Two stable radix sorts (ks_radix_sort_u64): all 8 digits of the hash, carrying
//               (group << 32) | abundance; then that word as the key, on the digits of its group field only — as many passes as
//               n_groups has bytes — carrying the hash.
//   tail        shared: run heads (a new hash or a new group) -> exclusive scan -> where every run starts -> one record per run,
//               its abundances summed in u64 (ks_run_abund_sum) and saturated; per group the number of runs in its span, scanned
//               into the output offsets (ks_scan_u32_to_u64).
// Everything is integer counting on a total order, so the result does not depend on the path (KS_DEBUG_UNION_PATH = 1 / 2 force
// the rank / the sort path for the tests), the launch geometry or the schedule.
//
// One stream, one wait (the run count comes back with it), synchronous on return.  The output's hash and abundance arrays are sized
// by the input's hash count, which bounds the run count: no second wait just to size them.  Scratch from the pool, per input hash:
// 32 bytes on the rank path (two u64 columns, heads, abundances, run starts), 56 on the sort path (the tagged column and two
// ping-pong pairs instead of the two columns); 4 bytes per group twice.
#include "ks_device.h"

#define UN_RANK_MAX 8u // the largest group the rank path takes (a frame set is 6)

// the member (sketch) that holds element i of the dense hash array, and that member's group
KS_DEV void un_owner(const u64 *off, u32 n_seqs, const u32 *go, u32 n_groups, u64 i, u32 *m, u32 *g) {
    *m = ks_last_le_u64(off, 0, n_seqs - 1, i);
    *g = ks_last_le_u32(go, n_groups, *m);
}
// entries of the ascending a[0, n) that are <= x
KS_DEV u32 un_count_le(const u64 *a, u32 n, u64 x) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_union_rank(const u64 *off, const u64 *hashes, const u32 *abunds, u32 n_seqs, u64 n, const u32 *go, u32 n_groups,
                                                    u64 *out_hash, u64 *out_ga, unsigned long long *bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 m, g;
    un_owner(off, n_seqs, go, n_groups, i, &m, &g);
    const u64 h = hashes[i];
    const u32 mb = go[g], me = go[g + 1];
    u64 at = i - off[m];
    for (u32 o = mb; o < me; o++) {
        if (o == m) continue;
        const u64 b = off[o];
        const u32 len = (u32)(off[o + 1] - b);
        at += o < m ? un_count_le(hashes + b, len, h) : ks_lower_bound_u64(hashes + b, len, h);
    }
    const u64 slot = off[mb] + at;
    if (slot >= n) { ks_first_bad(bad, 0, (u32)i); return; } // (cannot be: the counts of a span sum to less than its length)
    out_hash[slot] = h;
    out_ga[slot] = ((u64)g << 32) | abunds[i];
}

// the column the first sort of the sort path carries
__global__ __launch_bounds__(256) void k_union_tag(const u64 *off, const u32 *abunds, u32 n_seqs, u64 n, const u32 *go, u32 n_groups, u64 *ga) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 m, g;
    un_owner(off, n_seqs, go, n_groups, i, &m, &g);
    ga[i] = ((u64)g << 32) | abunds[i];
}

KS_DEV bool un_head(const u64 *hash, const u64 *ga, u64 i) { return i == 0 || hash[i] != hash[i - 1] || (ga[i] >> 32) != (ga[i - 1] >> 32); }

__global__ __launch_bounds__(256) void k_union_heads(const u64 *hash, const u64 *ga, u64 n, u32 *heads, u32 *abund) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    heads[i] = un_head(hash, ga, i) ? 1u : 0u;
    abund[i] = (u32)ga[i];
}

// hidx: the scanned heads; *n_runs: their total
__global__ __launch_bounds__(256) void k_union_starts(const u64 *hash, const u64 *ga, const u32 *hidx, u64 n, const u32 *n_runs, u64 *run_start) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (un_head(hash, ga, i)) run_start[hidx[i]] = i;
    if (i == 0) run_start[*n_runs] = n;
}

__global__ __launch_bounds__(256) void k_union_groups_emit(const u64 *hash, const u32 *abund, const u64 *run_start, const u32 *n_runs, u64 *hashes, u32 *abunds) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *n_runs) return;
    const u64 b = run_start[r], w = ks_run_abund_sum(abund, b, run_start[r + 1]);
    hashes[r] = hash[b];
    abunds[r] = w > 0xffffffffULL ? 0xffffffffu : (u32)w;
}

// runs in every group's span: a span begins with a head, so the scanned heads at its two ends are the runs before them
__global__ __launch_bounds__(256) void k_union_group_counts(const u64 *off, const u32 *go, u32 n_groups, const u32 *hidx, u64 n, const u32 *n_runs, u32 *counts) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const u64 b = off[go[g]], e = off[go[g + 1]];
    counts[g] = (e < n ? hidx[e] : *n_runs) - (b < n ? hidx[b] : *n_runs);
}

static int union_groups_run(ks_ctx *ctx, const ks_sketches *in, const u32 *go, u32 n_groups, ks_sketches *U) {
    const u64 n = in->n_hashes;
    KS_TRY(ks_alloc(ctx, &U->d_offsets, (size_t)n_groups + 1));
    KS_TRY(ks_alloc(ctx, &U->d_hashes, (size_t)n));
    KS_TRY(ks_alloc(ctx, &U->d_abunds, (size_t)n));
    if (n == 0 || n_groups == 0) {
        KS_HIP(ctx, hipMemsetAsync(U->d_offsets, 0, ((size_t)n_groups + 1) * sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    if (n >= 0xfffffffeULL) return ks_fail(ctx, KS_ERR_CAPACITY, "union_groups: 2^32 - 2 or more hashes");
    u32 largest = 0;
    for (u32 g = 0; g < n_groups; g++) largest = go[g + 1] - go[g] > largest ? go[g + 1] - go[g] : largest;
    bool rank = largest <= UN_RANK_MAX;
    if (const char *f = ks_dbg(ctx, KS_DBG_UNION_PATH)) { // (tests, tools/translate_bench.py)
        const int v = atoi(f);
        if (v == 1 || v == 2) rank = v == 1;
    }

    ks_scratch sc(ctx);
    u32 *d_go = nullptr, *heads = nullptr, *abund = nullptr, *counts = nullptr;
    u64 *hash = nullptr, *ga = nullptr, *run_start = nullptr;
    ks_ctl ctl; // word 0: the first hash the rank path could not place (an internal error); word 1: the runs
    KS_TRY(sc.alloc(&d_go, (size_t)n_groups + 1));
    KS_TRY(sc.alloc(&counts, (size_t)n_groups));
    KS_TRY(sc.alloc(&heads, (size_t)n)); KS_TRY(sc.alloc(&abund, (size_t)n)); KS_TRY(sc.alloc(&run_start, (size_t)n + 1));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_UNION, 1, 1));
    KS_HIP(ctx, hipMemcpyAsync(d_go, go, ((size_t)n_groups + 1) * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
    const u32 g_n = (u32)((n + 255) / 256);
    if (rank) {
        KS_TRY(sc.alloc(&hash, (size_t)n)); KS_TRY(sc.alloc(&ga, (size_t)n));
        KS_LAUNCH(ctx, "union_rank", k_union_rank, g_n, 256, (const u64 *)in->d_offsets, (const u64 *)in->d_hashes, (const u32 *)in->d_abunds, in->n_seqs, n,
                  (const u32 *)d_go, n_groups, hash, ga, ctl.words());
    } else {
        u64 *tag = nullptr, *ka = nullptr, *va = nullptr, *kb = nullptr, *vb = nullptr, *k1 = nullptr, *v1 = nullptr;
        KS_TRY(sc.alloc(&tag, (size_t)n)); KS_TRY(sc.alloc(&ka, (size_t)n)); KS_TRY(sc.alloc(&va, (size_t)n));
        KS_TRY(sc.alloc(&kb, (size_t)n)); KS_TRY(sc.alloc(&vb, (size_t)n));
        KS_LAUNCH(ctx, "union_tag", k_union_tag, g_n, 256, (const u64 *)in->d_offsets, (const u32 *)in->d_abunds, in->n_seqs, n, (const u32 *)d_go, n_groups, tag);
        const int by_hash[8] = {0, 8, 16, 24, 32, 40, 48, 56};
        KS_TRY(ks_radix_sort_u64(ctx, KS_SORT_INDEX, in->d_hashes, tag, ka, va, kb, vb, n, by_hash, 8, &k1, &v1));
        // the tagged column is the key now, the hash rides along: the pairs swap roles, and whichever holds the input is read first
        int by_group[4], ns = 0;
        for (int b = 0; n_groups > 1 && b < ks_key_bits(n_groups - 1); b += 8) by_group[ns++] = 32 + b;
        KS_TRY(ks_radix_sort_u64(ctx, KS_SORT_INDEX, v1, k1, va, ka, vb, kb, n, by_group, ns, &ga, &hash));
    }
    KS_LAUNCH(ctx, "union_heads", k_union_heads, g_n, 256, (const u64 *)hash, (const u64 *)ga, n, heads, abund);
    KS_TRY(ks_scan_u32_inplace(ctx, heads, n, ctl.low32(1)));
    const u32 *n_runs = ctl.low32(1);
    KS_LAUNCH(ctx, "union_starts", k_union_starts, g_n, 256, (const u64 *)hash, (const u64 *)ga, (const u32 *)heads, n, n_runs, run_start);
    KS_LAUNCH(ctx, "union_groups_emit", k_union_groups_emit, g_n, 256, (const u64 *)hash, (const u32 *)abund, (const u64 *)run_start, n_runs, U->d_hashes,
              U->d_abunds);
    KS_LAUNCH(ctx, "union_group_counts", k_union_group_counts, (n_groups + 255) / 256, 256, (const u64 *)in->d_offsets, (const u32 *)d_go, n_groups,
              (const u32 *)heads, n, n_runs, counts);
    KS_TRY(ks_scan_u32_to_u64(ctx, counts, U->d_offsets, n_groups));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    const u64 runs = ctl[1] & 0xffffffffULL;
    if (ctl.bad(0)) return ks_fail(ctx, KS_ERR_HIP, "internal error: union_groups could not place hash %llu of its input", (unsigned long long)ctl[0]);
    if (runs == 0 || runs > n) return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu runs in %llu hashes", (unsigned long long)runs, (unsigned long long)n);
    U->n_hashes = U->n_slots = runs;
    return KS_OK;
}

int ks_union_groups_impl(ks_ctx *ctx, const ks_sketches *in, const u32 *group_offsets, u32 n_groups, ks_sketches **out) {
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(in)));
    ks_result<ks_sketches> U(ctx, out, ks_sketches_free);
    U->params = in->params; U->n_seqs = n_groups; U->n_windows = in->n_windows;
    KS_TRY(union_groups_run(ctx, in, group_offsets, n_groups, U));
    return U.commit();
}

extern "C" int ks_sketches_union_groups(ks_ctx *ctx, const ks_sketches *in, const uint32_t *group_offsets, uint32_t n_groups, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!in || !group_offsets || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "union_groups: NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "union_groups", in));
    if (group_offsets[0] != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "union_groups: group_offsets[0] must be 0");
    for (u32 g = 0; g < n_groups; g++)
        if (group_offsets[g + 1] < group_offsets[g]) return ks_fail(ctx, KS_ERR_INVALID_ARG, "union_groups: group_offsets must ascend (group %u)", g);
    if (group_offsets[n_groups] != in->n_seqs)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "union_groups: group_offsets must end at the set's %u sketches, not at %u", in->n_seqs, group_offsets[n_groups]);
    return ks_union_groups_impl(ctx, in, group_offsets, n_groups, out);
    });
}

// ---------------------------------------------------------------------------------------------
// union of all sketches with summed abundances: the "combined minhash" of ProteomeIndex::store_signatures
// (src/rust/index.rs:800-830, add_many_with_abund under a mutex there; here one sort + run-length reduce)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_union_emit(const u64 *keys, const u32 *vals, const u64 *row_start, u32 n_rows,
                                                    u64 *hashes, u32 *abunds) {
    u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u64 b = row_start[r], w = ks_run_abund_sum(vals, b, row_start[r + 1]);
    hashes[r] = keys[b];
    abunds[r] = w > 0xffffffffULL ? 0xffffffffu : (u32)w;
}

static int union_run(ks_ctx *ctx, const ks_sketches *in, ks_sketches *U) {
    const u64 n = in->n_hashes;
    KS_TRY(ks_alloc(ctx, &U->d_offsets, 2));
    if (n == 0) {
        KS_HIP(ctx, hipMemsetAsync(U->d_offsets, 0, 2 * sizeof(u64), ctx->stream));
        KS_TRY(ks_alloc(ctx, &U->d_hashes, 1)); KS_TRY(ks_alloc(ctx, &U->d_abunds, 1));
        KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return KS_OK;
    }
    ks_scratch sc(ctx);
    ks_runs R;
    KS_TRY(ks_sorted_runs(ctx, in, sc, &R));
    U->n_hashes = U->n_slots = R.n_rows;
    KS_TRY(ks_alloc(ctx, &U->d_hashes, (size_t)R.n_rows)); KS_TRY(ks_alloc(ctx, &U->d_abunds, (size_t)R.n_rows));
    KS_LAUNCH(ctx, "union_emit", k_union_emit, (R.n_rows + 255) / 256, 256, (const u64 *)R.keys, (const u32 *)R.vals,
              (const u64 *)R.row_start, R.n_rows, U->d_hashes, U->d_abunds);
    u64 *const rb = ctx->h_pin + KS_PIN_READ;
    rb[0] = 0; rb[1] = R.n_rows;
    KS_HIP(ctx, hipMemcpyAsync(U->d_offsets, rb, 2 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KS_OK;
}

int ks_union_impl(ks_ctx *ctx, const ks_sketches *in, ks_sketches **out) {
    if (!in || !out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    KS_TRY(ks_sketches_make_dense(ctx, const_cast<ks_sketches *>(in)));
    ks_result<ks_sketches> U(ctx, out, ks_sketches_free);
    U->params = in->params; U->n_seqs = 1; U->n_windows = in->n_windows;
    KS_TRY(union_run(ctx, in, U));
    return U.commit();
}

extern "C" uint32_t ks_debug_union_rank_max(void) { return UN_RANK_MAX; }
