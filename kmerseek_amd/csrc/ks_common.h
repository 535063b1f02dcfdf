// ks_common.h — internal definitions shared by the HIP translation units of libkmerseek_amd.
// gfx950 (MI355X) only: wave = 64 lanes, 160 KiB LDS per CU, 256 CUs in 8 XCDs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kmerseek_amd.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t i32;
typedef int64_t i64;

#define KS_WAVE 64

// ---- device memory pool: grow-only, size classes with exact-fit reuse (ks_ctx.hip), so steady-state batches never hipMalloc ----
struct ks_pool_block {
    void *ptr;
    size_t size;
    bool in_use;
};

struct ks_timer_slot {
    hipEvent_t a, b;
    int name_id;
};

struct ks_copy_engine; // ks_copy.hip: pinned staging + host copy threads for pageable host buffers

// Diagnostic knobs (the KS_DEBUG_* environment variables: they force the rarely taken paths in the tests; results never
// depend on them).  They are read ONCE, into the context, when it is created — never on the per-call path, so a stray
// variable cannot switch kernels under a running service — and again only on request (ks_ctx_reload_debug_env: the tests
// switch paths on one context).
#define KS_DBG_LIST(X)                                                                                                   \
    X(STAGED_H2D) X(PLAIN_COPIES) X(PAIRS_LSD) X(MSD_LDS_CAP) X(SCAN_3PASS) X(INDEX_LSD) X(JOIN_FP) X(FP_COARSEN)        \
    X(PAIR_LIMIT) X(PBITS_MAX) X(RECORD_BITS) X(ONE_CURSOR) X(JOIN_SEGS) X(JOIN_SEG_CAP) X(JOIN_SPARSE)                \
    X(NO_ROWS_HINT) X(ROWS_TICKET) X(FORCE_ROWS_TICKET_RETRY) X(FORCE_TICKET_RETRY) X(NO_PLAN) X(NO_COMPACT) X(SPAN)      \
    X(NO_PACK) X(PLAN_SYNC) X(TILE_R) X(OUT_CAP) X(POOL_CAP) X(THROW) X(QCAP) X(LOOKBACK_SKIP) X(TILE_LOOKBACK) X(SYNC_API) X(POSTINGS12) X(POSTINGS10) X(NO_DEFER) X(BUCKET) X(JOIN_SPLIT) X(SUBSHIFT) X(MATCHPOS_ROW_BITS) X(SIGNIF_WAVE_ROWS) X(BEST_PATH) X(REGIONS_ROW_BITS) X(QFILTER) X(QFILTER_OCC) X(CLUSTER_PATH) X(GATHER_PATH) X(GREEDY_PATH) X(UNION_PATH) X(AGG_CAP) X(ROWS_PATH) X(CULL_PATH) X(CHAIN_PATH) X(COMP_PATH) X(PILEUP_PATH) X(POOL_FILL)
enum ks_dbg_id {
#define KS_DBG_ENUM(n) KS_DBG_##n,
    KS_DBG_LIST(KS_DBG_ENUM)
#undef KS_DBG_ENUM
    KS_DBG_COUNT
};
struct ks_debug {
    bool set[KS_DBG_COUNT];
    char val[KS_DBG_COUNT][32];
};
void ks_debug_load(ks_debug *d); // ks_ctx.hip

struct ks_ctx {
    int device = 0;
    ks_copy_engine *copy = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cus = 256;
    ks_debug dbg;            // KS_DEBUG_* as they were when the context was created
    u64 pool_cap = 0;        // KS_DEBUG_POOL_CAP: the pool refuses to hold more device bytes than this (0 = no cap)
    int pool_fill = -1;      // KS_DEBUG_POOL_FILL: 0..255, the byte every block the pool hands out is filled with first (-1 = handed out as it is)
    std::string err;
    std::vector<ks_pool_block> pool;
    u64 pool_mallocs = 0; // hipMalloc calls made by the pool (0 in steady state)
    // timing
    int timing = 0; // 0 off, 1 every launch, 2 only the kernels that carry the bytes (lower event overhead)
    std::vector<std::string> t_names;
    std::vector<u64> t_launches;
    std::vector<double> t_ms;
    std::vector<ks_timer_slot> t_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> t_free;
    bool t_open = false; // the last ks_timer_begin recorded a start event
    // small pinned host scratch for counters read back from the device
    u64 *h_pin = nullptr; // KS_PIN_WORDS x u64, one slot per read-back (KS_PIN_*)
    // matched posting pairs of recent searches (+ slack): sizes the next search's match list so the join runs once
    u64 pair_cap_hint = 0;
    // hit rows of recent searches (+ slack): sizes the next search's row arrays so that the row count can be read with the
    // final synchronisation instead of a round trip of its own
    u64 rows_hint = 0;
    // the sketch tiles take their ids from blockIdx.x (dispatch order) until a look-back ever gives up on this context;
    // from then on from an atomic ticket (guaranteed order, one more memory round trip per tile)
    bool sketch_use_ticket = false;
    // how often a sketch batch had to be repeated: look-back gave up (-> ticket ids from then on), a compacting tile
    // overflowed its LDS lists (-> plain tiles for that batch), bounded outputs too small (-> window-count sized)
    u64 sketch_ticket_fallbacks = 0, sketch_compact_fallbacks = 0, sketch_cap_fallbacks = 0;
    u64 sketch_planned_slots = 0; // shared-tile launches whose tiles took their CSR base from the plan (no look-back): a path, not a repeat
    bool rows_use_ticket = false; u64 rows_ticket_fallbacks = 0; // k_pair_rows_fused: dispatch-order tile ids until a look-back gives up
    u64 fused_deferred = 0, fused_redos = 0; // ks_sketch_search_device: calls that folded the sketch wait into the first wait of the search / were repeated plainly
    u64 fused_aggregated = 0;                // ... whose rows the aggregate pass made (agg_used below rose)
    u64 join_retries = 0; // searches whose match list outgrew a segment and ran the join twice
    // The rows of a search come from the match list by sort aggregation (two more partition levels + the run-length pass) or by
    // hash aggregation of the level-1 regions (k_pairs_aggregate, ks_rows.hip), which pays while many records share a row:
    // rows_mult is the previous search's records per row (0: no search yet, the first one sorts).  KS_DEBUG_ROWS_PATH = agg /
    // sort forces either.  agg_used: searches whose rows the aggregate pass made; agg_overflows: searches in which a region's
    // table overflowed (or its look-back gave up) and the sort resumed on the level-1 output; agg_oflow_rows: the fewest rows
    // of such a search (0: none yet) — the pass is not tried again until a search expects under half of them.
    double rows_mult = 0.0;
    u64 agg_used = 0, agg_overflows = 0, agg_oflow_rows = 0;
    // The presence filter of the bucket scatter (ks_index::d_presence) pays while most query postings are foreign to the index.
    // false after a search whose scatter kept more than half of its postings (the probes then cost more than the dropped
    // bytes save); true again after an unfiltered search with fewer than a quarter as many matches as postings.
    // KS_DEBUG_QFILTER = 0 / 1 forces either.
    bool qfilter_pays = true;
    u64 qfilter_seen = 0, qfilter_dropped = 0; // query postings of the filtered scatters of this context / those they dropped
    // ... and of the latest of them alone (qf_last_seen 0: none yet): its kept / seen fraction is what the next filtered search
    // expects its join buckets to hold when it picks the join kernel (se_join).  join_table: searches that took the table kernel
    // (k_join_sparse); fused_table_joined: ks_sketch_search_device calls among them.
    u64 qf_last_seen = 0, qf_last_kept = 0;
    u64 join_table = 0, fused_table_joined = 0;
    // single-launch scans (ks_prims.hip): status ring + ticket counter in device memory, never reset: every entry is
    // tagged with the global tile number that wrote it
    unsigned long long *scan_ring = nullptr;
    u32 *scan_ticket = nullptr;
    u32 scan_ticket_base = 0; // value the device counter will have when the next scan starts
    // encode LUTs (3 x 256 bytes) in device memory
    u8 *d_lut = nullptr;
    // ks_stream_wait: a pinned host word the stream's last kernel stamps, polled by the host (see ks_ctx.hip)
    unsigned long long *h_flag = nullptr;
    unsigned long long wait_seq = 0;
};

// The host waits for everything queued on the context's stream (what hipStreamSynchronize does) by polling a pinned word
// that a one-thread kernel at the end of the queue stamps: the wake-up of a blocking synchronisation costs 10 - 25 us of idle
// queue on this runtime, and a sketch + search step waits three times.  KS_DEBUG_SYNC_API = the runtime's call instead.
int ks_stream_wait(ks_ctx *ctx);
// ... and the same with the words the host wants to read afterwards: the stamping kernel writes them to pinned memory itself
// (instead of one device -> host copy dispatch per block before it).  dst must lie in pinned host memory (ctx->h_pin).
#define KS_FETCH_MAX 4
struct ks_fetch_seg {
    const void *src; // device
    u32 *dst;        // pinned host
    u32 rows, row_words, src_stride; // 32-bit words
};
static inline ks_fetch_seg ks_fetch_words(const void *src, void *dst, u32 n_words32) { return ks_fetch_seg{src, (u32 *)dst, 1u, n_words32, n_words32}; }
int ks_stream_wait_fetch(ks_ctx *ctx, const ks_fetch_seg *segs, int n);

// returns nullptr and sets ctx->err on failure
void *ks_pool_alloc(ks_ctx *ctx, size_t bytes);
void ks_pool_free(ks_ctx *ctx, void *ptr);
void ks_pool_trim(ks_ctx *ctx);

int ks_fail(ks_ctx *ctx, int status, const char *fmt, ...);
// value of a diagnostic knob as the context holds it, or nullptr (drop-in for getenv("KS_DEBUG_" #name))
static inline const char *ks_dbg(const ks_ctx *ctx, int id) { return (ctx && ctx->dbg.set[id]) ? ctx->dbg.val[id] : nullptr; }

// Every extern "C" entry point that can allocate host memory (new, std::vector / std::string growth in the context, the
// pool's block list, timers) runs its body inside this guard: a C++ exception never unwinds into the caller's frames
// (Rust, ctypes: that is std::terminate).  bad_alloc -> KS_ERR_OOM, anything else -> KS_ERR_HIP "internal error".
// Reference convention: every failure is a value (src/rust/errors.rs:8-24).
int ks_guard_fail(ks_ctx *ctx, int status, const char *what) noexcept;
void ks_guard_enter(ks_ctx *ctx); // KS_DEBUG_THROW (tests): throws the named exception from inside the guard
template <typename F>
static inline int ks_guard(ks_ctx *ctx, F &&body) noexcept {
    try {
        ks_guard_enter(ctx);
        return body();
    } catch (const std::bad_alloc &) {
        return ks_guard_fail(ctx, KS_ERR_OOM, "out of host memory (std::bad_alloc)");
    } catch (const std::exception &e) {
        return ks_guard_fail(ctx, KS_ERR_HIP, e.what());
    } catch (...) {
        return ks_guard_fail(ctx, KS_ERR_HIP, "unknown exception");
    }
}

void ks_timer_begin(ks_ctx *ctx, const char *name);
void ks_timer_end(ks_ctx *ctx);

#define KS_HIP(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return ks_fail(ctx, KS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                                    \
    } while (0)

#define KS_TRY(expr)                        \
    do {                                    \
        int s__ = (expr);                   \
        if (s__ != KS_OK) return s__;       \
    } while (0)

// Launch on the context's stream, bracketed by HIP events when timing is enabled.
#define KS_LAUNCH(ctx, name, kernel, grid, block, ...)                                   \
    do {                                                                                 \
        ks_timer_begin(ctx, name);                                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (ctx)->stream, __VA_ARGS__); \
        ks_timer_end(ctx);                                                               \
        KS_HIP(ctx, hipGetLastError());                                                  \
    } while (0)

template <typename T>
static inline int ks_alloc(ks_ctx *ctx, T **out, size_t count) {
    void *p = ks_pool_alloc(ctx, (count ? count : 1) * sizeof(T));
    if (!p) return KS_ERR_OOM;
    *out = (T *)p;
    return KS_OK;
}

// Pool blocks a host driver borrows for one call: given back (ks_pool_free, stream-ordered like every pool free) when the
// owner goes out of scope, so that the drivers can return early through KS_TRY / KS_HIP.  A fixed table: no heap allocation.
struct ks_scratch {
    ks_ctx *ctx;
    void *blk[16];
    int n = 0;
    explicit ks_scratch(ks_ctx *c) : ctx(c) {}
    ks_scratch(const ks_scratch &) = delete;
    ~ks_scratch() { for (int i = 0; i < n; i++) ks_pool_free(ctx, blk[i]); }
    template <typename T> int alloc(T **out, size_t count) {
        if (n == 16) return ks_fail(ctx, KS_ERR_HIP, "internal error: scratch table full");
        KS_TRY(ks_alloc(ctx, out, count));
        blk[n++] = *out;
        return KS_OK;
    }
    void free(void *p) { if (forget(p)) ks_pool_free(ctx, p); } // early give-back (a retry sizes the block anew); nullptr: no-op
    template <typename T> T *keep(T *p) { forget(p); return p; } // the block outlives the call (part of a result object)
    bool forget(void *p) {
        for (int i = 0; p && i < n; i++)
            if (blk[i] == p) { blk[i] = blk[--n]; return true; }
        return false;
    }
};

// The control block of a pass over hit rows, u64 words in the pass's scratch: `n_bad` words "the first row that is wrong for
// reason i" (atomicMin; all ones: none), then `n_count` counters from 0.  fetch() names all of it for the pass's one wait, which
// brings it to the pass's pinned slot (KS_PIN_*, at least n_bad + n_count words); [] and bad() read that copy.
struct ks_ctl {
    u64 *dev = nullptr;
    u64 *host = nullptr;
    u32 n_words = 0;
    int init(ks_ctx *ctx, ks_scratch &sc, u32 pin_slot, u32 n_bad, u32 n_count) {
        n_words = n_bad + n_count;
        host = ctx->h_pin + pin_slot;
        KS_TRY(sc.alloc(&dev, n_words));
        KS_HIP(ctx, hipMemsetAsync(dev, 0xff, n_bad * sizeof(u64), ctx->stream));
        KS_HIP(ctx, hipMemsetAsync(dev + n_bad, 0, n_count * sizeof(u64), ctx->stream));
        return KS_OK;
    }
    unsigned long long *words() const { return (unsigned long long *)dev; } // what the kernels take
    u32 *low32(u32 i) const { return (u32 *)(dev + i); }                    // a counter a u32 scan total is written to
    ks_fetch_seg fetch() const { return ks_fetch_words(dev, host, 2 * n_words); }
    u64 operator[](u32 i) const { return host[i]; }
    bool bad(u32 i) const { return host[i] != ~0ULL; }
};

// One lifecycle for every opaque result object (ks_sketches, ks_index, ks_hits, ...).  The constructor clears *out and makes
// the object: value-initialised, ->ctx set.  The driver fills it through KS_TRY / KS_HIP and ends with `return R.commit();`,
// which hands the object to *out without a wait.  Every other way out of the scope — a failed status, an exception, a return
// with KS_OK and nothing produced (search_core's split, sketch_attempt's redo) — waits for the stream (launches already queued
// may still write the object's blocks) and gives the object to its free function; *out stays nullptr.
template <typename T>
struct ks_result {
    T *obj = nullptr;
    T **out;
    void (*free_fn)(T *);
    ks_result(ks_ctx *ctx, T **out_, void (*f)(T *)) : out(out_), free_fn(f) {
        *out = nullptr;
        obj = new T();
        obj->ctx = ctx;
    }
    ks_result(const ks_result &) = delete;
    ~ks_result() {
        if (!obj) return;
        (void)hipStreamSynchronize(obj->ctx->stream);
        free_fn(obj);
    }
    T *operator->() const { return obj; }
    operator T *() const { return obj; }
    int commit() { *out = obj; obj = nullptr; return KS_OK; }
};

// the body of every *_copy_to_host: each column with a destination and bytes to copy goes through ks_copy_d2h, then one wait
struct ks_column { void *dst; const void *src; size_t bytes; };
int ks_copy_d2h(ks_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
static inline int ks_columns_to_host(ks_ctx *ctx, const ks_column *cols, size_t n) {
    KS_HIP(ctx, hipSetDevice(ctx->device));
    for (const ks_column *c = cols; c < cols + n; c++)
        if (c->dst && c->bytes) KS_TRY(ks_copy_d2h(ctx, c->dst, c->src, c->bytes));
    KS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KS_OK;
}
int ks_columns_to_host(ks_ctx *ctx, std::initializer_list<ks_column> cols); // ks_copy.hip

// ---- the column list of a result object ----
// A result struct names its device columns ONCE, in its member `each`: f(column, element count) for every column, in the order
// of the object's copy_to_host parameters; a third argument `false` marks a column made on demand, which copy_to_host does not
// carry and ks_obj_alloc leaves alone.  The walks below are all that frees, copies out, allocates and (ks_obj_take, ks_api.hip)
// takes them.  Where the count is a member of the struct, `each` passes that member itself (s.n_regions, no copy of it): a walk
// over the columns of ONE count knows them by the member's address, so that two counts of equal value stay two.
// every column back to the pool (NULL: never allocated), then the object
template <class T>
static inline void ks_obj_free(T *o) {
    if (!o) return;
    T::each(*o, [&](auto *p, const u64 &, bool = true) { ks_pool_free(o->ctx, p); });
    delete o;
}
// the body of ks_<object>_copy_to_host, behind its ks_guard: dst are its destination parameters in their order (NULL: skip that column)
template <class T, class... D>
static inline int ks_obj_to_host(ks_ctx *ctx, const T *o, D *...dst) {
    if (!ctx || !o) return KS_ERR_INVALID_ARG;
    void *const to[] = {dst...};
    const size_t elem[] = {sizeof(D)...};
    ks_column cols[sizeof...(D)];
    size_t i = 0;
    bool same = true;
    T::each(*o, [&](auto *p, const u64 &n, bool copied = true) {
        if (!copied) return;
        if (i < sizeof...(D) && elem[i] == sizeof(*p)) cols[i] = ks_column{to[i], p, (size_t)n * sizeof(*p)};
        else same = false;
        i++;
    });
    if (!same || i != sizeof...(D)) return ks_fail(ctx, KS_ERR_HIP, "internal error: a column list and its copy_to_host differ");
    return ks_columns_to_host(ctx, cols, i);
}
// the columns of o listed with the member `count`, allocated at its value (set before the call)
template <class T>
static inline int ks_obj_alloc(ks_ctx *ctx, T *o, const u64 &count) {
    int st = KS_OK;
    bool any = false;
    T::each(*o, [&](auto *&p, const u64 &n, bool up_front = true) {
        if (&n != &count || !up_front || st != KS_OK) return;
        st = ks_alloc(ctx, &p, (size_t)n);
        any = true;
    });
    return any ? st : ks_fail(ctx, KS_ERR_HIP, "internal error: no column is listed with that count");
}

// ---- opaque objects ----
struct ks_sketches {
    ks_ctx *ctx;
    ks_params params;
    u32 n_seqs;
    u64 n_hashes;
    u64 n_windows;
    // CSR with slots: d_offsets[s] is where sequence s's SLOT starts — as long as the sequence's kept hashes, repeats included,
    // so that a tile knows its place as soon as it has hashed (ks_sketch.hip: the look-back runs on kept counts) — and the
    // sequence's sketch (ascending distinct hashes + abundances) is the first d_counts[s] entries of the slot.  gapped == false
    // (no sequence repeats a k-mer: every synthetic batch, most real ones at large k; or after ks_sketches_make_dense): slots and
    // runs coincide and d_offsets is the plain CSR of the C ABI.  Everything that reads the arrays as a plain CSR calls
    // ks_sketches_make_dense first (one gather pass, only when gapped); the fused postings of a query batch never do.
    u64 *d_offsets; // n_seqs + 1
    u64 *d_hashes;  // n_slots
    u32 *d_abunds;  // n_slots
    u32 *d_counts;  // n_seqs distinct hashes per sequence, or NULL (sketches from host arrays, unions: dense by construction)
    u64 n_slots;    // d_offsets[n_seqs]
    bool gapped;
    // optional, made by ks_sketch_queries_device: postings (hash, seq) already partitioned on hash bits
    // low 8 bits of the join prefix (ks_join_prefix) into part_regions fixed-capacity regions (region r holds part_len[r] records
    // starting at r * part_cap) — the first partition pass of a search against an index that joins on part_pbits bits
    u64 *part_keys;
    u32 *part_vals;
    u32 *part_len;  // device, [part_regions]
    u64 part_cap;
    u32 part_regions;
    int part_pbits;
    u32 part_K;     // ks_join_prefix multiplier the regions were cut with
    // each region is split into 2^part_sub_shift sub-regions, one per XCD of the sketch launch (segment r << shift | x
    // at (r << shift | x) * part_cap, part_len likewise): slices that are neighbours in memory were written through ONE L2
    u32 part_sub_shift;
    // part_s != 0: 10-byte postings.  Inside region r the 8 hash bits [part_s, part_s + 8) ARE r (scaled = 1: the join
    // prefix is a bit field of the hash), so the key column carries the low 8 bits of the sequence id there and part_vals is
    // a u16 column with the rest (sequence ids < 2^24): 10 instead of 12 bytes through the sketch write, the bucket scatter
    // (in and out) and the join's read.
    u32 part_s;
    // pending != 0 (ks_sketch_search_device): the launches are queued, the copy of the control block to
    // h_pin + KS_PIN_SKETCH too, but nobody has waited yet — n_hashes / n_windows are upper bounds until
    // ks_sketch_finish_pending has run behind a wait on the context's stream (the search's first wait)
    // the sketch call's control block (device): statistics | posting cursors (part_len points INTO it) | tile status words —
    // one allocation, one memset per call; freed with the object
    u64 *ctl_block;
    int pending;
    u64 *pend_stats; // the statistics words of ctl_block, read back by the caller's next wait
    u64 pend_out_cap;
    u32 pend_max_seq_len;
    int pend_planned;
};

// ---- the pinned host words (ctx->h_pin, KS_PIN_WORDS x u64): one slot per read-back, in u64 words.  No two slots overlap,
// so words that are fetched in the same wait (join + pending sketch; row pass + scan status) never clobber each other.
enum : u32 {
    KS_PIN_JOIN = 0, KS_PIN_JOIN_WORDS = 128, // join: per segment (count, flags) as u32 pairs, 2 words apart (ks_search.hip)
    KS_PIN_SKETCH = 128, KS_PIN_SKETCH_WORDS = 32, // the control block of a sketch whose read-back is pending ...
    KS_PIN_SKETCH_SYNC = 160, KS_PIN_SKETCH_SYNC_WORDS = 32, // ... and of a sketch that waits for itself
    KS_PIN_STAGE = 192,      // u32 uploaded by the sketch's ticket repeat (the status bits it keeps)
    KS_PIN_ROWS = 193,       // 2 words, row pass: u32 (ticket / an aggregate table overflowed, look-back flag) | u32 (row count, kept rows)
    KS_PIN_SCAN = 195,       // u32: a one-launch scan gave up a look-back (ks_scan_status_check)
    KS_PIN_SORT_OFLOW = 196, // u32: a fixed capacity of the partitioned index sort did not hold
    KS_PIN_READ = 197,       // 2 words, one-call read-backs: index build, union, merge, k-mer positions
    KS_PIN_DENSE = 199,      // u64: the scan total of ks_sketches_make_dense
    KS_PIN_SIGNIF = 200,     // 3 words, significance: first row with an id out of range | first row with another shared count | corpus flag
    KS_PIN_BEST = 203,       // 3 words, best hits: first row with an id out of range | first row with an empty sketch | kept rows
    KS_PIN_REGIONS = 206,    // u32: match regions kept (ks_regions.hip)
    KS_PIN_CLUSTER = 207,    // 5 words, clusters: first row with an id out of range | first row with an empty sketch | edges | clusters | largest
    KS_PIN_GATHER = 212,     // 4 words, gather: first row with an id out of range | first row with another shared count | first row past the incidence array | kept rows
    KS_PIN_GREEDY = 216,     // 10 words, greedy clusters: the five of KS_PIN_CLUSTER | the two live-edge counts | undecided nodes | rounds | members without a representative
    KS_PIN_TRANSLATE = 226,  // 4 words, six-frame translation: bad offsets | the frames' residue count (the last frame offset)
    KS_PIN_UNION = 230,      // 2 words, union by group: distinct (group, hash) runs
    KS_PIN_RSCORE = 232,     // 1 word, region scores: first row whose regions do not lie inside its sequences (ks_rscore.hip)
    KS_PIN_RALIGN = 233,     // 2 words, region alignments: first row whose regions do not lie inside its sequences | first row with a sequence too long (ks_ralign.hip)
    KS_PIN_RTRACE = 235,     // 8 words, region traceback: bad row | sequence too long | alignment outside its region's sequences | walk that does not close, then the scan totals (ks_rtrace.hip)
    KS_PIN_RCULL = 243,      // 3 words, region cull: first row that breaks the CSR | first region with a length of 0 | kept regions (ks_rcull.hip)
    KS_PIN_RCHAIN = 246,     // 5 words, region chain: first row that breaks the CSR | first region with a length of 0 | with an end beyond 0xffffffff | with a score beyond 2^30 | chained regions (ks_rchain.hip)
    KS_PIN_RCHAIN_COV = 251, // 2 words, chain coverage: first row with an id beyond the batches | first row whose chain is longer than its sequence (ks_rchain.hip)
    KS_PIN_RSTITCH = 253,    // 14 words, region stitch: the eleven first-offender words (ks_stitch_kit.h: ST_BAD_*), then the scan totals: direction rows | columns | ops
    KS_PIN_RCOMP = 267,      // 2 words, residue composition: first sequence whose offsets descend or pass the batch | first sequence of 2^32 residues or more (ks_astats.hip)
    KS_PIN_ASTATS = 269,     // 4 words, alignment statistics: first row that breaks the CSR | with an id beyond its composition | with a sequence too long | fallback rows (ks_astats.hip)
    KS_PIN_MASK = 273,       // 7 words, low-complexity mask and split: first record with bad offsets | masked residues | hot-window runs | raw segments | kept segments, then the segments' residue count (ks_mask.hip)
    KS_PIN_FFOLD = 280,      // 8 words, frame fold: first record with bad offsets | too long | first row with a qid beyond the frames | out of order | that breaks the CSR | first region beyond its frame | beyond the target bound, then the folded rows (ks_ffold.hip)
    KS_PIN_FSTITCH = 288,    // 14 words, frame stitch: the same eleven words, then the scan totals: direction rows | columns | ops
    KS_PIN_PILEUP = 302,     // 7 words, pileup: the seven first-offender words (ks_pileup.hip: PU_BAD_*)
    KS_PIN_PROFILE = 309,    // 1 word, profile build: the last offset of the query batch (ks_profile.hip)
    KS_PIN_PWEIGHTS = 310,   // 8 words, entry weights: the seven of KS_PIN_PILEUP | first entry with a column the counts do not hold (ks_pileup.hip)
    KS_PIN_END = 318,
};
#define KS_PIN_WORDS 320
static_assert(KS_PIN_JOIN + KS_PIN_JOIN_WORDS <= KS_PIN_SKETCH && KS_PIN_SKETCH + KS_PIN_SKETCH_WORDS <= KS_PIN_SKETCH_SYNC &&
                  KS_PIN_SKETCH_SYNC + KS_PIN_SKETCH_SYNC_WORDS <= KS_PIN_STAGE && KS_PIN_STAGE < KS_PIN_ROWS &&
                  KS_PIN_ROWS + 2 <= KS_PIN_SCAN && KS_PIN_SCAN < KS_PIN_SORT_OFLOW && KS_PIN_SORT_OFLOW < KS_PIN_READ &&
                  KS_PIN_READ + 2 <= KS_PIN_DENSE && KS_PIN_DENSE < KS_PIN_SIGNIF && KS_PIN_SIGNIF + 3 <= KS_PIN_BEST && KS_PIN_BEST + 3 <= KS_PIN_REGIONS && KS_PIN_REGIONS < KS_PIN_CLUSTER && KS_PIN_CLUSTER + 5 <= KS_PIN_GATHER && KS_PIN_GATHER + 4 <= KS_PIN_GREEDY && KS_PIN_GREEDY + 10 <= KS_PIN_TRANSLATE && KS_PIN_TRANSLATE + 4 <= KS_PIN_UNION && KS_PIN_UNION + 2 <= KS_PIN_RSCORE && KS_PIN_RSCORE < KS_PIN_RALIGN && KS_PIN_RALIGN + 2 <= KS_PIN_RTRACE && KS_PIN_RTRACE + 8 <= KS_PIN_RCULL && KS_PIN_RCULL + 3 <= KS_PIN_RCHAIN && KS_PIN_RCHAIN + 5 <= KS_PIN_RCHAIN_COV && KS_PIN_RCHAIN_COV + 2 <= KS_PIN_RSTITCH && KS_PIN_RSTITCH + 14 <= KS_PIN_RCOMP && KS_PIN_RCOMP + 2 <= KS_PIN_ASTATS && KS_PIN_ASTATS + 4 <= KS_PIN_MASK && KS_PIN_MASK + 7 <= KS_PIN_FFOLD && KS_PIN_FFOLD + 8 <= KS_PIN_FSTITCH && KS_PIN_FSTITCH + 14 <= KS_PIN_PILEUP && KS_PIN_PILEUP + 7 <= KS_PIN_PROFILE && KS_PIN_PROFILE < KS_PIN_PWEIGHTS && KS_PIN_PWEIGHTS + 8 <= KS_PIN_END &&
                  KS_PIN_END <= KS_PIN_WORDS,
              "pinned host slots overlap or do not fit KS_PIN_WORDS");

// one index posting as the join fetches it for a candidate match: one 16-byte load
struct __attribute__((aligned(16))) ks_post {
    u64 key;
    u32 tid;
    u32 abund;
};

// per join bucket: first key (the fingerprints count from it) and the multiplier of the in-LDS directory slot
// (floor(2^32 * JN_DIR / (largest fingerprint of the bucket + 1)), ks_search.hip)
struct __attribute__((aligned(16))) ks_bmeta {
    u64 base;
    u32 slot_mul;
    u32 pad;
};

struct ks_index {
    ks_ctx *ctx;
    ks_params params;
    u32 n_targets;
    u64 n_postings;
    u64 *d_keys;   // sorted hashes      } columns of the sort: what the join of a small / medium index reads;
    u32 *d_tids;   // target id          } released once d_fp / d_post are written when the index is big (fp_layout)
    u32 *d_abunds; // target abundance   }
    u32 *d_fp;     // per posting, in hash order: min((key - first key of its join bucket) >> (32 - pbits), 2^32 - 1) — the 4 bytes
                   // per posting the join streams; monotone inside a bucket
    ks_post *d_post; // per posting, in hash order: (key, tid, abundance)
    ks_bmeta *d_bmeta; // per join bucket (2^pbits entries)
    bool fp_layout;    // true: d_fp / d_post / d_bmeta are what the join reads; false: the sorted columns
    int fp_shift;      // 32 - pbits (KS_DEBUG_FP_COARSEN adds to it: coarser fingerprints, more false candidates — tests)
    u32 max_abund; // largest of them: how many low bits of a packed match record the abundance needs
    u64 *d_dir;    // join-bucket directory: d_dir[b] = first posting whose join prefix is >= b (2^pbits + 1 entries)
    int pbits;     // join prefix bits, a function of n_postings and the layout alone (ks_join_pbits)
    // fp_layout: presence filter over hash prefixes, for the query side's bucket scatter (k_bucket_scatter): 2^pres_bits bits in
    // 32-bit words (pres_bits >= pbits: every join bucket owns 2^(pres_bits - pbits) of them, ~KS_QF_OCC per posting; one word at
    // the least).  A posting with prefix p = ks_join_prefix(hash, pres_K) sets two bits of word p >> 5: bit p & 31 and bit
    // ks_presence_bit2(hash); a query hash whose two bits are not both set matches no posting.  nullptr: the index has none
    // (key-column join).
    u32 *d_presence;
    u32 pres_K;
    int pres_bits;
    // The same at ~KS_QF_OCC_BIG bits per posting, for batches big enough to earn back the fetch of a filter twice the size
    // (se_partition picks).  nullptr: the index has one size only (both widths round to the same power of two, or
    // KS_DEBUG_QFILTER_OCC named the one to build).
    u32 *d_presence_big;
    u32 pres_big_K;
    int pres_big_bits;
};

// the row columns of a hit list as the kernels read them (rf_move, ks_device.h)
struct rf_cols {
    const u32 *qid, *tid, *isect;
    const u64 *nw, *median2;
    const double *ss;
};

// The column set of a hit list: the one owner of the pointers.  Every column is a pool block of its own, or NULL (the list
// does not have it) — except that d_nw and d_isect point INTO d_block where that is not NULL (the row pass: one allocation and
// one memset with its status words).  The members (ks_hits.hip) are the only code that knows this.
enum : u32 { KS_COLS_RANKED = 1u, KS_COLS_GATHER = 2u }; // rank + src_row; the three gather columns
struct ks_hit_cols {
    u32 *d_qid, *d_tid, *d_isect;
    u64 *d_nw;
    u64 *d_block;
    // KS_SEARCH_ABUND_STATS: per row 2 x median and sum of squared deviations of the shared target abundances
    u64 *d_median2;
    double *d_ss;
    // ks_hits_best: per kept row its rank inside its query and its row in the input list; NULL for every other hit list
    u32 *d_rank, *d_src_row;
    // ks_hits_gather: per kept row the hashes it newly covered, the query's hashes still uncovered after it, and the query's
    // abundances over the newly covered ones; NULL for every other hit list
    u32 *d_ga_unique, *d_ga_remaining;
    u64 *d_ga_weighted;

    int alloc(ks_ctx *ctx, size_t n, bool with_stats, u32 extra); // n rows: the four columns every list has, the statistics, KS_COLS_*
    void release(ks_ctx *ctx);                                    // every column back to the pool and NULL (an empty set: no-op)
    void take(ks_ctx *ctx, ks_hit_cols &from) { release(ctx); *this = from; from = ks_hit_cols{}; } // `from`'s columns replace these
    // the device view of the row columns.  The statistics are NULL unless the list has them (ks_hits::has_stats): every alloc of a
    // list's columns is called with that flag, and the row pass (se_rows_post) makes them itself only under it
    rf_cols rows() const { return rf_cols{d_qid, d_tid, d_isect, d_nw, d_median2, d_ss}; }
    // the first n rows of `from` to rows [at, at + n) of this set, on the context's stream; stats: both sets have the statistics
    int append(ks_ctx *ctx, u64 at, const ks_hit_cols &from, u64 n, bool stats);
};

struct ks_hits : ks_hit_cols {
    ks_ctx *ctx;
    u64 n_hits;
    u64 n_pair_instances;
    int partition_path; // how the query postings reached their join buckets (see ks_hits_partition_path)
    int bucket_posting_bytes; // bytes per query posting inside the join buckets (12, 10 or 9; 0: no bucket scatter ran)
    bool has_stats; // KS_SEARCH_ABUND_STATS: the list has d_median2 and d_ss
};

struct ks_kmerpos {
    ks_ctx *ctx;
    ks_params params; // what the table was made with (ks_match_positions joins only tables of equal parameters)
    u32 n_seqs;       // sequences of the batch: d_seq values are below it
    u64 n;
    u32 *d_seq, *d_start;
    u64 *d_hash;
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_seq, s.n); f(s.d_start, s.n); f(s.d_hash, s.n); }
};

// pairs of window starts that share a hash, grouped by hit row (ks_matchpos.hip)
struct ks_matchpos {
    ks_ctx *ctx;
    ks_params params;            // of the tables the pairs were joined from (ks_match_regions chains with their ksize)
    u64 n_rows, n_pairs;
    u32 n_slices;
    u32 max_qs, max_ts;          // the longest query / target start of the tables: bounds of q_start / t_start
    u64 *d_row_offsets;          // n_rows + 1
    u32 *d_qstart, *d_tstart;    // n_pairs
    u32 *d_qlo, *d_qhi, *d_tlo, *d_thi; // n_rows
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_qstart, s.n_pairs); f(s.d_tstart, s.n_pairs);
        f(s.d_qlo, s.n_rows); f(s.d_qhi, s.n_rows); f(s.d_tlo, s.n_rows); f(s.d_thi, s.n_rows);
    }
};

// chained pairs of one hit row: maximal colinear runs of shared k-mers (ks_regions.hip)
struct ks_regions {
    ks_ctx *ctx;
    u64 n_rows, n_regions;
    u32 n_slices;
    u64 *d_row_offsets;                                 // n_rows + 1
    u32 *d_qstart, *d_tstart, *d_length, *d_nkmers, *d_covered; // n_regions
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_qstart, s.n_regions); f(s.d_tstart, s.n_regions); f(s.d_length, s.n_regions);
        f(s.d_nkmers, s.n_regions); f(s.d_covered, s.n_regions);
    }
    void take_from(const ks_regions &src) { n_slices = src.n_slices; } // what a take copies besides the columns
};

// the columns of a cull's input on the device; tl == ql for regions of one length
struct ks_rcull_cols { const u64 *row_offs; const u32 *qs, *ql, *ts, *tl; const i64 *score; };
// ... and of a chain's: the same and ident, alen: NULL or a column to sum
struct ks_rchain_cols : ks_rcull_cols { const u32 *ident, *alen; };

// one row of 28 scores per residue of a query batch (ks_profile.hip)
struct ks_profile {
    ks_ctx *ctx;
    u64 n_seqs, n_residues, n_scores;    // n_scores: 28 x n_residues
    int8_t *d_scores;                    // n_scores
    u8 *d_consensus;                     // n_residues
    u32 *d_n_obs;                        // n_residues
    int8_t matrix[KS_RSCORE_ALPHABET * KS_RSCORE_ALPHABET]; // the fallback the rows were built with
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_scores, s.n_scores); f(s.d_consensus, s.n_residues); f(s.d_n_obs, s.n_residues);
    }
};

// the regions of a ks_regions scored under a substitution matrix and extended without gaps (ks_rscore.hip)
struct ks_rscores {
    ks_ctx *ctx;
    u64 n_rows, n_regions;
    u64 *d_row_offsets;                                                              // n_rows + 1
    u32 *d_qstart, *d_tstart, *d_length, *d_identities, *d_positives, *d_core_ident; // n_regions
    i64 *d_score;                                                                    // n_regions
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_qstart, s.n_regions); f(s.d_tstart, s.n_regions); f(s.d_length, s.n_regions);
        f(s.d_score, s.n_regions); f(s.d_identities, s.n_regions); f(s.d_positives, s.n_regions); f(s.d_core_ident, s.n_regions);
    }
    void take_from(const ks_rscores &) {}
    // the view a cull / a chain reads: one length for both sides, which is also the alignment length
    ks_rchain_cols cols() const { return {{d_row_offsets, d_qstart, d_length, d_tstart, d_length, d_score}, d_identities, d_length}; }
};
// one residue batch on the device, as the C ABI passes it
struct ks_res_batch { const u8 *res; const u64 *offs; u32 n_seqs; u64 n_res; };
// ks_regions_score behind its argument checks (opts: validated; R, H: of ctx, equal row counts)
// what the passes against a profile refuse before any device work (ks_rscore.hip): no profile, one of another context or of another batch than Q
int rk_profile_check(ks_ctx *ctx, const char *pass, const ks_profile *prof, const ks_res_batch &Q);
// prof: NULL, or the profile of Q (of ctx, Q.n_res residues) that scores the pairs in the matrix's place
int ks_regions_score_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                          const ks_rscore_opts *opts, const ks_profile *prof, ks_rscores *S);

// the regions of a ks_regions aligned with gaps from the middle of their seeds (ks_ralign.hip)
struct ks_raligns {
    ks_ctx *ctx;
    u64 n_rows, n_regions;
    u64 *d_row_offsets;                                             // n_rows + 1
    u32 *d_qstart, *d_qlength, *d_tstart, *d_tlength;               // n_regions
    u32 *d_identities, *d_positives, *d_gap_opens, *d_gaps, *d_aln_length; // n_regions
    i64 *d_score;                                                   // n_regions
    // the options the alignments were made with: ks_regions_traceback walks the path of exactly this program
    u32 band, gap_open, gap_extend, x_drop;
    int8_t matrix[KS_RSCORE_ALPHABET * KS_RSCORE_ALPHABET];
    // made against a ks_profile (ks_regions_align_profile): `matrix` is the profile's fallback, and a pass that reads residues under
    // a matrix refuses the object (ks_refuse_by_profile)
    bool by_profile;
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_qstart, s.n_regions); f(s.d_qlength, s.n_regions); f(s.d_tstart, s.n_regions);
        f(s.d_tlength, s.n_regions); f(s.d_score, s.n_regions); f(s.d_identities, s.n_regions); f(s.d_positives, s.n_regions);
        f(s.d_gap_opens, s.n_regions); f(s.d_gaps, s.n_regions); f(s.d_aln_length, s.n_regions);
    }
    void take_from(const ks_raligns &src) {
        band = src.band; gap_open = src.gap_open; gap_extend = src.gap_extend; x_drop = src.x_drop;
        memcpy(matrix, src.matrix, sizeof matrix);
        by_profile = src.by_profile;
    }
    ks_rchain_cols cols() const { return {{d_row_offsets, d_qstart, d_qlength, d_tstart, d_tlength, d_score}, d_identities, d_aln_length}; }
};
// ks_regions_align behind its argument checks (opts: not NULL, validated; R, H: of ctx, equal row counts)
// prof: as ks_regions_score_impl
int ks_regions_align_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                          const ks_ralign_opts *opts, const ks_profile *prof, ks_raligns *S);
// what every pass that reads residues under the recorded matrix says to a profile-made ks_raligns, before any device work
int ks_refuse_by_profile(ks_ctx *ctx, const char *pass, const ks_raligns *S);

// the paths of the alignments of a ks_raligns, one CIGAR per region (ks_rtrace.hip)
struct ks_cigars {
    ks_ctx *ctx;
    u64 n_rows, n_regions, n_ops;
    u64 *d_op_offsets; // n_regions + 1
    u32 *d_ops;        // n_ops: len << 4 | op
    u64 dir_bytes;     // direction scratch the call allocated, the slices it ran in (diagnostic)
    u32 n_slices;
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_op_offsets, s.n_regions + 1); f(s.d_ops, s.n_ops); }
};
// ks_regions_traceback behind its argument checks (flags validated; R, H, S: of ctx, equal counts)
// prof: NULL where S was made under a matrix, the profile (as ks_regions_score_impl) where S is profile-made
int ks_regions_traceback_impl(ks_ctx *ctx, const ks_regions *R, const ks_hits *H, const ks_res_batch &Q, const ks_res_batch &T,
                              const ks_raligns *S, const ks_profile *prof, u32 flags, u64 max_scratch_bytes, ks_cigars *C);

// the regions of a hit row that no better region of the row covers (ks_rcull.hip)
struct ks_rcull {
    ks_ctx *ctx;
    u64 n_rows, n_regions, n_kept;
    u64 *d_row_offsets;                  // n_rows + 1: the CSR of the kept regions
    u32 *d_src_region, *d_rank, *d_n_merged; // n_kept (blocks of n_regions entries)
    u32 *d_keeper;                       // n_regions
    double *d_row_best;                  // n_rows
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_src_region, s.n_kept); f(s.d_rank, s.n_kept); f(s.d_n_merged, s.n_kept);
        f(s.d_keeper, s.n_regions); f(s.d_row_best, s.n_rows);
    }
};
// ks_regions_cull_device behind its argument checks (opts: validated, defaults filled in; n_regions == 0 where n_rows == 0)
int ks_regions_cull_impl(ks_ctx *ctx, const ks_rcull_cols &cols, u64 n_rows, u64 n_regions, const ks_rcull_opts *opts, ks_rcull *K);
// out[c][i] = in[c][src[i]] for i < n and every listed column (at most KS_TAKE_COLS of 32 bits, one of 64), enqueued
#define KS_TAKE_COLS 10
struct ks_take_cols { const u32 *in[KS_TAKE_COLS]; u32 *out[KS_TAKE_COLS]; u32 n32; const i64 *in64; i64 *out64; };
int ks_rcull_take_launch(ks_ctx *ctx, const ks_rcull *K, const ks_take_cols &cols);

// the best colinear chain of the regions of each hit row (ks_rchain.hip)
struct ks_rchain {
    ks_ctx *ctx;
    u64 n_rows, n_regions, n_chained;
    u64 *d_row_offsets;                  // n_rows + 1: the CSR of the chains' members
    u32 *d_src_region;                   // n_chained (a block of n_regions entries)
    i64 *d_best;                         // n_regions
    u32 *d_pred;                         // n_regions
    i64 *d_chain_score;                  // n_rows, as every column below
    u32 *d_q_start, *d_q_length, *d_t_start, *d_t_length, *d_q_aligned, *d_t_aligned;
    u64 *d_identities, *d_aln_length;
    double *d_row_score;
    double *d_row_cov;                   // NULL until ks_rchain_coverage has run: not a column of copy_to_host
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_row_offsets, s.n_rows + 1); f(s.d_src_region, s.n_chained); f(s.d_best, s.n_regions); f(s.d_pred, s.n_regions);
        f(s.d_chain_score, s.n_rows); f(s.d_q_start, s.n_rows); f(s.d_q_length, s.n_rows); f(s.d_t_start, s.n_rows);
        f(s.d_t_length, s.n_rows); f(s.d_q_aligned, s.n_rows); f(s.d_t_aligned, s.n_rows); f(s.d_identities, s.n_rows);
        f(s.d_aln_length, s.n_rows); f(s.d_row_score, s.n_rows); f(s.d_row_cov, s.n_rows, false);
    }
};
// ks_regions_chain_device behind its argument checks (opts: validated, not NULL; n_regions == 0 where n_rows == 0)
int ks_regions_chain_impl(ks_ctx *ctx, const ks_rchain_cols &cols, u64 n_rows, u64 n_regions, const ks_rchain_opts *opts, ks_rchain *K);
// ks_rchain_coverage behind its argument checks (H: of ctx, K's row count; mode <= 3)
int ks_rchain_coverage_impl(ks_ctx *ctx, ks_rchain *K, const ks_hits *H, const u64 *d_q_off, u32 n_q, const u64 *d_t_off, u32 n_t, u32 mode);

// the frame rows of a translated search folded per (record, strand, target), their regions on the strand's bases (ks_ffold.hip)
struct ks_ffold {
    ks_ctx *ctx;
    u64 n_rows, n_regions, n_src_rows;   // folded rows; regions (all of the input's); hit rows of the input
    u32 *d_src_row;                      // 3 * n_rows (a block of 3 * n_src_rows entries)
    u64 *d_row_offsets;                  // n_rows + 1 (a block of n_src_rows + 1)
    u32 *d_src_region;                   // n_regions, as every column below
    u8 *d_frame;
    u32 *d_nt_length, *d_s_start, *d_nt_start, *d_t_start3, *d_t_length3;
    i64 *d_score;                        // NULL where the input column was not passed, as the two below
    u32 *d_identities, *d_aln_length;
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_src_row, 3 * s.n_rows); f(s.d_row_offsets, s.n_rows + 1); f(s.d_src_region, s.n_regions); f(s.d_frame, s.n_regions);
        f(s.d_nt_length, s.n_regions); f(s.d_s_start, s.n_regions); f(s.d_nt_start, s.n_regions); f(s.d_t_start3, s.n_regions);
        f(s.d_t_length3, s.n_regions); f(s.d_score, (u64)(s.d_score ? s.n_regions : 0)); f(s.d_identities, (u64)(s.d_identities ? s.n_regions : 0));
        f(s.d_aln_length, (u64)(s.d_aln_length ? s.n_regions : 0));
    }
};
// ks_frames_fold_device behind its argument checks (H: of ctx; n_regions == 0 where H has no rows; cols.score may be NULL): F and D
// are filled
int ks_frames_fold_impl(ks_ctx *ctx, const ks_hits *H, const u64 *d_nt_offs, u32 n_records, const ks_rchain_cols &cols, u64 n_regions,
                        ks_hits *F, ks_ffold *D);

// the chain of each hit row stitched into one gapped alignment with one CIGAR (ks_rstitch.hip)
struct ks_hitalns {
    ks_ctx *ctx;
    u64 n_rows, n_ops;
    u64 *d_op_offsets;                   // n_rows + 1
    u32 *d_ops;                          // n_ops: len << 4 | op
    i64 *d_score;                        // n_rows, as every column below
    u32 *d_q_start, *d_q_length, *d_t_start, *d_t_length;
    u32 *d_identities, *d_positives, *d_gap_opens, *d_gaps, *d_aln_length;
    u32 *d_n_members, *d_n_filled, *d_n_open, *d_n_trimmed;
    double *d_row_score;
    u64 dir_bytes;                       // direction scratch the call allocated, the slices it ran in (diagnostic)
    u32 n_slices;
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_op_offsets, s.n_rows + 1); f(s.d_ops, s.n_ops); f(s.d_q_start, s.n_rows); f(s.d_q_length, s.n_rows);
        f(s.d_t_start, s.n_rows); f(s.d_t_length, s.n_rows); f(s.d_score, s.n_rows); f(s.d_identities, s.n_rows);
        f(s.d_positives, s.n_rows); f(s.d_gap_opens, s.n_rows); f(s.d_gaps, s.n_rows); f(s.d_aln_length, s.n_rows);
        f(s.d_n_members, s.n_rows); f(s.d_n_filled, s.n_rows); f(s.d_n_open, s.n_rows); f(s.d_n_trimmed, s.n_rows);
        f(s.d_row_score, s.n_rows);
    }
};
// ks_regions_stitch behind its argument checks (options validated, defaults filled in; K, S, G, H: of ctx, equal counts)
int ks_regions_stitch_impl(ks_ctx *ctx, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G, const ks_hits *H, const ks_res_batch &Q,
                           const ks_res_batch &T, u32 max_fill, u32 flags, u64 max_scratch_bytes, ks_hitalns *R);

// the chain of each folded row of a translated search stitched into one alignment of the strand's bases (ks_fstitch.hip)
struct ks_framealns {
    ks_ctx *ctx;
    u64 n_rows, n_ops;
    u64 *d_op_offsets;                   // n_rows + 1
    u32 *d_ops;                          // n_ops: len << 4 | op
    i64 *d_score;                        // n_rows, as every column below
    u32 *d_s_start, *d_nt_length, *d_nt_start, *d_t_start, *d_t_length;
    u32 *d_identities, *d_positives, *d_gap_opens, *d_gaps, *d_aln_length;
    u32 *d_n_members, *d_n_filled, *d_n_open, *d_n_trimmed, *d_n_frameshifts;
    double *d_row_score;
    u64 dir_bytes;                       // direction scratch the call allocated, the slices it ran in (diagnostic)
    u32 n_slices;
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_op_offsets, s.n_rows + 1); f(s.d_ops, s.n_ops); f(s.d_s_start, s.n_rows); f(s.d_nt_length, s.n_rows); f(s.d_nt_start, s.n_rows);
        f(s.d_t_start, s.n_rows); f(s.d_t_length, s.n_rows); f(s.d_score, s.n_rows); f(s.d_identities, s.n_rows);
        f(s.d_positives, s.n_rows); f(s.d_gap_opens, s.n_rows); f(s.d_gaps, s.n_rows); f(s.d_aln_length, s.n_rows);
        f(s.d_n_members, s.n_rows); f(s.d_n_filled, s.n_rows); f(s.d_n_open, s.n_rows); f(s.d_n_trimmed, s.n_rows);
        f(s.d_n_frameshifts, s.n_rows); f(s.d_row_score, s.n_rows);
    }
};
// ks_frames_stitch behind its argument checks (options validated, defaults filled in; F, H, K, S, G: of ctx, equal counts)
int ks_frames_stitch_impl(ks_ctx *ctx, const ks_ffold *F, const ks_hits *H, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G,
                          const ks_res_batch &Q, const ks_res_batch &T, u32 max_fill, u32 flags, u32 frameshift_cost, u64 max_scratch_bytes,
                          ks_framealns *R);

// the alignments of a hit list piled up on the residues of one batch: depth, profile, per-sequence coverage (ks_pileup.hip)
struct ks_pileup {
    ks_ctx *ctx;
    u64 n_seqs, n_residues, n_profile;   // n_profile: 28 x n_residues with KS_PILEUP_PROFILE, else 0
    u32 *d_depth;                        // n_residues
    u32 *d_counts;                       // n_profile
    u32 *d_length, *d_n_alignments, *d_covered, *d_max_depth; // n_seqs, as every column below
    u64 *d_depth_sum;
    double *d_breadth, *d_mean_depth;
    // a weighted pileup alone (ks_wpileup_device): the weights of the entries that place a residue, summed
    u64 n_weighted, n_wprofile;          // n_residues and n_profile of a weighted pileup, else 0
    u64 *d_wdepth;                       // n_weighted
    u64 *d_wcounts;                      // n_wprofile
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_depth, s.n_residues); f(s.d_counts, s.n_profile); f(s.d_length, s.n_seqs); f(s.d_n_alignments, s.n_seqs); f(s.d_covered, s.n_seqs);
        f(s.d_max_depth, s.n_seqs); f(s.d_depth_sum, s.n_seqs); f(s.d_breadth, s.n_seqs); f(s.d_mean_depth, s.n_seqs);
        f(s.d_wdepth, s.n_weighted, false); f(s.d_wcounts, s.n_wprofile, false); // (ks_wpileup_copy_to_host carries them)
    }
};
// one weight per entry of a pileup (ks_pileup.hip: ks_entry_weights_device)
struct ks_pweights {
    ks_ctx *ctx;
    u64 n_entries;
    u32 *d_weight, *d_n_cols;            // n_entries
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_weight, s.n_entries); f(s.d_n_cols, s.n_entries); }
};

// the residue classes of the sequences of a batch, counted (ks_astats.hip)
struct ks_rcomp {
    ks_ctx *ctx;
    u32 n_seqs;
    u64 n_res;
    u32 *d_counts;  // n_seqs x KS_RSCORE_ALPHABET
    u64 *d_totals;  // KS_RSCORE_ALPHABET
    u32 *d_length;  // n_seqs
    u64 h_totals[KS_RSCORE_ALPHABET]; // the totals again: the default background of ks_scores_stats_device
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_counts, (u64)s.n_seqs * KS_RSCORE_ALPHABET); f(s.d_totals, (u64)KS_RSCORE_ALPHABET); f(s.d_length, (u64)s.n_seqs);
    }
};
int ks_residue_composition_impl(ks_ctx *ctx, const ks_res_batch &B, ks_rcomp *C);
// bit scores and E-values of a column of scores (ks_astats.hip)
struct ks_astats {
    ks_ctx *ctx;
    u64 n_rows, n, n_fallback;
    double lambda_std, lambda_used, K_used;
    u32 params_source;
    u8 *d_status;                                                // n_rows
    double *d_x, *d_ratio, *d_row_bit, *d_row_evalue;            // n_rows
    double *d_bit, *d_evalue;                                    // n
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_status, s.n_rows); f(s.d_x, s.n_rows); f(s.d_ratio, s.n_rows); f(s.d_bit, s.n); f(s.d_evalue, s.n);
        f(s.d_row_bit, s.n_rows); f(s.d_row_evalue, s.n_rows);
    }
};
// ks_scores_stats_device behind its argument checks (o: validated, defaults filled in, its matrix the one to use; H, Q, T: of
// ctx; T may be NULL where the contract allows it)
int ks_scores_stats_impl(ks_ctx *ctx, const u64 *d_row_offs, const i64 *d_score, u64 n_rows, u64 n, const ks_hits *H, const ks_rcomp *Q,
                         const ks_rcomp *T, const ks_astats_opts &o, ks_astats *A);

// clusters of a hit list read as a graph: its connected components (ks_cluster.hip) or greedy representative clusters (ks_greedy.hip)
struct ks_clusters {
    ks_ctx *ctx;
    u32 n_nodes, n_clusters, largest;
    u64 n_edges;
    u32 n_rounds; // ks_greedy.hip: the rounds the pass took; 0 for connected components
    u32 *d_label, *d_cluster_id, *d_members, *d_rep; // n_nodes each (d_rep: the first n_clusters are meaningful)
    u64 *d_offsets;                                  // n_nodes + 1 (entries past n_clusters repeat n_nodes)
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_label, (u64)s.n_nodes); f(s.d_cluster_id, (u64)s.n_nodes); f(s.d_offsets, (u64)s.n_clusters + 1); f(s.d_members, (u64)s.n_nodes);
        f(s.d_rep, (u64)s.n_clusters);
    }
};
// ---- labels -> clusters (ks_cluster.hip; ks_hits_cluster and ks_hits_cluster_greedy) ----
// the first words of the control block of both passes: the first row with an id out of range / with an empty sketch, the rows
// that passed, and what the tail below counts
enum { CL_BAD_ID = 0, CL_BAD_SIZE = 1, CL_EDGES = 2, CL_CLUSTERS = 3, CL_LARGEST = 4 };
// the result arrays of a cluster pass over n nodes (label, cluster_id, members, representative, offsets), scalars zeroed
int ks_clusters_alloc(ks_ctx *ctx, ks_clusters *K, u32 n);
// per-node scratch of the tail, n entries each.  On entry sizes and rep are zero and root_idx[i] = (K->d_label[i] == i)
struct ks_label_scratch { u32 *root_idx, *sizes; u64 *rep, *ka, *kb; };
// The tail of a cluster pass: K->d_label holds per node the root of its cluster (a root labels itself) -> cluster_id (clusters
// numbered by ascending root), the CSR (offsets, members ascending), per cluster the member with the most distinct hashes of
// `nodes` (ties, and without `nodes`: the smallest id), ctl[CL_CLUSTERS] and ctl[CL_LARGEST].  Enqueued; the caller waits
// (ks_stream_wait_fetch_scans: the scans are one-launch ones).
int ks_clusters_from_labels(ks_ctx *ctx, ks_clusters *K, const ks_sketches *nodes, const ks_label_scratch &W, const ks_ctl &ctl);
// what both passes refuse after the wait (the first bad row named) and the scalars of the tail, from ctl's host copy into K
int ks_clusters_finish(ks_ctx *ctx, const char *what, ks_clusters *K, const ks_ctl &ctl);
// the option words both passes share and what they ask of the other arguments ("<what> options: ..."); ctx may be NULL
int ks_cluster_words_check(ks_ctx *ctx, const char *what, u32 similarity, u32 n_nodes, double threshold, const ks_sketches *nodes,
                           const double *d_score);

// ---- low-complexity masking (ks_mask.hip) ----
// one byte per residue (1: masked) and the masked residues of every record
struct ks_mask {
    ks_ctx *ctx;
    u32 n_seqs;
    u64 n_res, n_masked;
    u32 window, k1, k2; // the options the mask was made with, defaults filled in
    u8 *d_mask;         // n_res (the block is padded to whole words)
    u32 *d_counts;      // n_seqs
    template <class S, class F> static constexpr void each(S &s, F &&f) { f(s.d_mask, s.n_res); f(s.d_counts, (u64)s.n_seqs); }
};
// the unmasked stretches of a batch of at least min_len residues, in record order, as a residue batch of their own
struct ks_segments {
    ks_ctx *ctx;
    u32 n_records, min_len;
    u64 n_segs, n_res;
    u32 *d_seg_record, *d_seg_start; // n_segs: the record of a segment, its first residue counted from the record's
    u64 *d_seg_offsets;              // n_segs + 1: the batch layout of d_residues
    u8 *d_residues;                  // n_res (+ 16: the sketch tiles load whole 16-byte words)
    u32 *d_group_offsets;            // n_records + 1: record r owns the segments [d_group_offsets[r], d_group_offsets[r + 1])
    template <class S, class F> static constexpr void each(S &s, F &&f) {
        f(s.d_seg_record, s.n_segs); f(s.d_seg_start, s.n_segs); f(s.d_seg_offsets, s.n_segs + 1); f(s.d_residues, s.n_res);
        f(s.d_group_offsets, (u64)s.n_records + 1);
    }
};

// ---- passes whose sort key is `hit row | fields of the pair` (ks_matchpos.hip, ks_regions.hip) ----
// Row index and fields that do not fit 64 bits together: the hit rows are cut into slices, each sorted with a key of its own
// whose row field counts from the slice's first row.  A record of another slice carries the row value one past the slice:
// the sort takes it to the end.
struct ks_slice_fmt {
    int pt, pqt;          // bits of the lowest field, of all fields below the row
    u32 row0, slice_rows; // rows [row0, row0 + slice_rows) are this slice's
};
struct ks_row_slices {
    u64 per_slice, n_slices;
    int low_bits; // the key bits below the row field
    ks_slice_fmt fmt(u64 s, u64 n_rows, int pt) const {
        ks_slice_fmt F;
        F.pt = pt; F.pqt = low_bits;
        F.row0 = (u32)(s * per_slice);
        F.slice_rows = (u32)(n_rows - F.row0 < per_slice ? n_rows - F.row0 : per_slice);
        return F;
    }
};
int ks_key_bits(u64 v); // bits of v (at least 1)
// the slices of n_rows (>= 1) hit rows under a key with low_bits bits below the row; dbg_id: the knob that narrows the row
// field (tests: small inputs take the slice path).  KS_ERR_CAPACITY ("<what>: ...") when no key bit is left for a row.
int ks_row_slices_plan(ks_ctx *ctx, int dbg_id, const char *what, int low_bits, u64 n_rows, ks_row_slices *out);
// the sort of n keys in ka on their nbits live bits (ks_sort_pairs_msd, LSD passes for short lists); kb: scratch of the
// same size; *sorted = where they ended up (ka or kb)
int ks_sort_live_keys(ks_ctx *ctx, u64 *ka, u64 *kb, u64 n, int nbits, u64 **sorted);

// ---- hit lists (ks_hits.hip): what the passes that return one share (ks_search, ks_hits_best, ks_hits_gather) ----
// what a list made of H's rows says about the search that made them
void ks_hits_inherit(ks_hits *B, const ks_hits *H);
// Row r of H with rank[r] != KS_RANK_NONE goes to row dst[r] (< cap) of B: all columns of H that B holds, the rank and r itself
// (src_row).  ga != NULL: the three per-row gather columns go with it, into B's.
#define KS_RANK_NONE 0xffffffffu
struct ks_gather_cols { const u32 *unique, *remaining; const u64 *weighted; };
int ks_hits_move_ranked(ks_ctx *ctx, const ks_hits *H, u32 n_rows, const u32 *dst, const u32 *rank, u32 cap, ks_hits *B,
                        const ks_gather_cols *ga);
// the hit rows of such a pass: *n, their count as a u32, or "<what>: 2^32 - 2 or more hit rows" (KS_ERR_CAPACITY); *cap: the rows
// the output can hold, at most `per_query` (0: no limit) for each query of Q (NULL: not known)
int ks_hits_select_plan(ks_ctx *ctx, const char *what, const ks_hits *H, const ks_sketches *Q, u32 per_query, u32 *n, u64 *cap);
// The tail of such a pass (`what`, for its messages): the keep flags of H's n_rows rows are scanned in place, the total into
// ctl's counter `kept`; the kept rows move to B (room for `cap` rows); ONE wait brings ctl home; `checks` — what the pass's own
// control words refuse — runs before the kept count is held against cap and becomes B->n_hits.
int ks_hits_select_tail(ks_ctx *ctx, const char *what, const ks_hits *H, u32 n_rows, u32 *flags, const u32 *rank, u64 cap,
                        const ks_gather_cols *ga, const ks_ctl &ctl, u32 kept, const std::function<int()> &checks, ks_hits *B);
// the hit lists of the slices of one query batch (parts[i]: the queries from firsts[i] on) in one, query ids back to batch numbering
int ks_hits_concat(ks_ctx *ctx, const std::vector<ks_hits *> &parts, const std::vector<u32> &firsts, bool has_stats, ks_hits **out);
// a row list for ks_row_list_push (ks_device.h): room for n_rows rows behind its count, the count zeroed
int ks_row_list_alloc(ks_ctx *ctx, ks_scratch &sc, size_t n_rows, u32 **list);
// a segment list for ks_seg_list_push: room for `cap` segments behind its count, the count zeroed
int ks_seg_list_alloc(ks_ctx *ctx, ks_scratch &sc, size_t cap, u32 **list);
// the knob that sends every segment one way (tests): 0 by length (unset), 1 by a wave, 2 by a workgroup; 3: 2 with *small set
int ks_seg_path_knob(const ks_ctx *ctx, int dbg_id, bool *small);

// ---- device-wide primitives (ks_scan.hip, ks_sort.hip) ----
// exclusive scan of n u32 values into u64 (out[n] = total is also written: out has n+1 entries)
// BOUND: the SUM must stay below 2^38 whenever the one-launch path runs (2 or more tiles of 2048 values, at most 2^19 tiles,
// KS_DEBUG_SCAN_3PASS unset): a tile's status word carries its running sum in 38 bits under the 24-bit tile tag, and the path is
// picked by n (n < 2^38), not by the sum — a larger sum runs into the tag, predecessors stop matching and the look-back gives
// up (ks_scan_status_check reports it; nothing hangs).  A single tile and the 3-pass path have no such limit.  2^38 u32 counts
// of records that exist in device memory cannot be reached; a sum of sizes that are only COMPUTED (DESIGN.md §"primitives,
// tested directly" lists the callers) needs a host-side bound of its own.
int ks_scan_u32_to_u64(ks_ctx *ctx, const u32 *in, u64 *out, u64 n);
// ... without that bound (never the one-launch path: two more small launches), for sums of sizes that nothing has allocated yet
int ks_scan_u32_to_u64_wide(ks_ctx *ctx, const u32 *in, u64 *out, u64 n);
// the status ring + ticket words of the one-launch scans, made by the context's first such scan (or by a test hook before it)
int ks_scan_ring_make(ks_ctx *ctx);
// exclusive scan u32 -> u32 in place (n < 2^32 total); optionally writes the total to d_total
// The one-launch scans cannot report a look-back that gave up (bounded spin) by themselves: callers enqueue
// ks_scan_status_fetch before a stream synchronisation they do anyway and call ks_scan_status_check after it.
int ks_scan_status_fetch(ks_ctx *ctx);
int ks_scan_status_check(ks_ctx *ctx);
// ks_stream_wait_fetch of the segments (fewer than KS_FETCH_MAX) and of the scans' give-up word, then ks_scan_status_check: the
// one wait of a pass that ran one-launch scans
int ks_stream_wait_fetch_scans(ks_ctx *ctx, std::initializer_list<ks_fetch_seg> segs);
int ks_scan_u32_inplace(ks_ctx *ctx, u32 *data, u64 n, u32 *d_total);

// Stable LSD radix passes over (key u64, value V) records, one 8-bit digit at each listed shift.
// keys_in / vals_in are only read (they may be the caller's own data, or one of the scratch pairs);
// passes ping-pong between the scratch pairs (ka, va) and (kb, vb); *keys_out / *vals_out point at the
// result.  `tag` picks the kernel instantiation name ("radix_scatter.<tag>" in the timing table).
enum { KS_SORT_INDEX = 0, KS_SORT_QPART = 1, KS_SORT_PAIRS = 2 };
// optional segmented input of the FIRST pass: `regions` fixed-capacity regions, region r = len[r] records at r * cap
struct ks_rs_segments {
    const u32 *len; // device
    u64 cap;
    u32 regions;    // number of segments
    u32 sub_shift;  // partition digit of segment s = s >> sub_shift (sub-regions of one region share it)
};
int ks_radix_sort_u32(ks_ctx *ctx, int tag, const u64 *keys_in, const u32 *vals_in, u64 *ka, u32 *va, u64 *kb, u32 *vb,
                      u64 n, const int *shifts, int n_shifts, u64 **keys_out, u32 **vals_out,
                      const ks_rs_segments *seg = nullptr, u32 pfxK = 0);
// last partition pass of a search without a histogram: segmented input -> 2^pbits buckets of capacity bcap;
// bcur[bucket] ends as the bucket's record count, status[1] != 0 if some bucket overflowed
// keys only (the match list with the abundance packed under the ids)
int ks_radix_sort_keys(ks_ctx *ctx, int tag, const u64 *keys_in, u64 *ka, u64 *kb, u64 n, const int *shifts, int n_shifts,
                       u64 **keys_out);
// storage slot of join bucket (high digit d, region r): region-major, so the 2^(P-8) runs a scatter tile writes lie in
// one window of n_hi * bcap records (a handful of pages) instead of 256 * bcap records apart (one page each: 5 M
// UTCL1 translation misses per launch with the digit-major order, 0.02 M with this one — same run time, though)
#define KS_BSLOT(d, r, n_hi) ((r) * (n_hi) + (d))
// status[1] of the bucket scatter: bit 0 = a bucket overflowed; from bit KS_QF_KEPT up = postings that passed the presence filter
#define KS_QF_KEPT 1
// presence != nullptr: postings without both of their bits in the index's presence filter (ks_index::d_presence, multiplier presK)
// are dropped; fix_s: where the region's 8 prefix bits sit in the high word of a hash (vfmt != 0: the keys carry id bits there)
int ks_bucket_scatter_u32(ks_ctx *ctx, const u64 *keys_in, const u32 *vals_in, const ks_rs_segments *seg, int shift,
                          u32 pfxK, u64 *bkeys, u32 *bvals, u32 *bcur, u32 bcap, unsigned long long *status, u32 n_hi, int vfmt,
                          const u32 *presence, u32 presK, u32 fix_s);
// index build in three passes (two partition passes + in-LDS bucket sort); *overflowed = 1: use the LSD sort instead
int ks_index_sort_partitioned(ks_ctx *ctx, const u64 *keys_in, const u64 *vals_in, u64 n, u64 max_hash, u64 *okeys, u32 *otids,
                              u32 *oabunds, u32 *d_max_abund, int *overflowed);
// Match-list sort in three moves whatever the key width (ks_msd.hip): two exact MSD partition levels of 8 bits + in-LDS sort of the
// 65,536 buckets.  Sorts `ka` in place on key bits [lo_bit, lo_bit + nbits); kb = scratch.  *done = 0: not applicable (small list /
// narrow key / KS_DEBUG_PAIRS_LSD), the caller takes the LSD passes.
// segs != NULL: the list lies in ka in segs->n segments seg_cap records apart, count[s] of them filled (the join's segmented
// pair list): the first partition level reads it as it lies — no copy that makes it dense first
#define KS_MSD_MAX_SEGS 64
struct ks_msd_segs {
    u32 n;
    u32 tile_start[KS_MSD_MAX_SEGS + 1]; // first level-1 tile of every segment (the last entry: all tiles)
    u32 count[KS_MSD_MAX_SEGS];
    u64 seg_cap;
};
int ks_sort_pairs_msd(ks_ctx *ctx, u64 *ka, u64 *kb, u64 n, int lo_bit, int nbits, int *done, const ks_msd_segs *segs = nullptr);
// The same sort in two steps, for a caller that may not need the rest: ks_msd_level1 leaves the list in kb in KS_MSD_REGIONS exact
// regions on the top 8 key bits (region r ends at P->ends[r], the spent cursors; every key lies wholly inside one region) and
// ka untouched as scratch; ks_msd_finish runs levels 2 / 3 on those buffers (the sorted list: ka) and ks_msd_drop gives the
// plan's block back instead.  P->blk == nullptr behind ks_msd_level1: not applicable, nothing was launched.
#define KS_MSD_REGIONS 256
struct ks_msd_plan {
    u64 *ka, *kb, n;
    int lo_bit, nbits;
    u32 *blk;        // off1 | off2 | big-list counter | big list (ks_msd.hip)
    const u32 *ends; // [KS_MSD_REGIONS] inside blk
};
// what levels 2 / 3 need of a plan: how wide level 2 is (*bits2_out: a function of n and nbits alone) and where the words of the
// plan's block lie (n_zero words that start at zero: the histograms, then the big-list counter as the last of them)
struct ms_layout {
    int shift1, shift2;
    u32 mask2, n_buckets, n_sub, sub_stride;
    size_t off2_words, n_zero;
};
ms_layout ms_layout_of(u64 n, int lo_bit, int nbits, int *bits2_out);
int ks_msd_level1(ks_ctx *ctx, u64 *ka, u64 *kb, u64 n, int lo_bit, int nbits, const ks_msd_segs *segs, ks_msd_plan *P);
int ks_msd_finish(ks_ctx *ctx, ks_msd_plan *P);
void ks_msd_drop(ks_ctx *ctx, ks_msd_plan *P);
int ks_radix_sort_u64(ks_ctx *ctx, int tag, const u64 *keys_in, const u64 *vals_in, u64 *ka, u64 *va, u64 *kb, u64 *vb,
                      u64 n, const int *shifts, int n_shifts, u64 **keys_out, u64 **vals_out);

// ---- sorted list -> runs -> one record per run; a search's matches -> rows (ks_rows.hip) ----
// a dense sketch set sorted by hash: keys / vals (hashes, abundances) and row_start[n_rows + 1] in the caller's scratch
struct ks_runs { u64 *keys; u32 *vals; u64 *row_start; u32 n_rows; };
int ks_sorted_runs(ks_ctx *ctx, const ks_sketches *in, ks_scratch &sc, ks_runs *out);
// what the row half needs from one search; the sorted match list pk becomes H's rows (n_pairs == 0: none, pk is not read)
struct ks_rows_in { const ks_sketches *q; u64 n_pairs; int tbits, abits; bool stats; double min_c; int qbits; };
int ks_search_rows(ks_ctx *ctx, const ks_rows_in &R, ks_hits *H, const u64 *pk);
// ... and from the level-1 output of the match sort instead (hash aggregation per region, k_pairs_aggregate).  *fell_back: a
// region's table overflowed or a look-back gave up — H has no rows, the list is untouched: the caller finishes the sort and
// takes ks_search_rows.
int ks_search_rows_agg(ks_ctx *ctx, const ks_rows_in &R, ks_hits *H, const ks_msd_plan &P, bool *fell_back);
// whether the aggregate pass is expected to pay for a list of n_pairs records (the context's history, KS_DEBUG_ROWS_PATH)
bool ks_rows_agg_wanted(const ks_ctx *ctx, const ks_rows_in &R);
// a search of n_rows rows overflowed the aggregate pass's tables: remembered, ks_rows_agg_wanted holds back (agg_oflow_rows)
void ks_rows_agg_overflowed(ks_ctx *ctx, u64 n_rows);

// ---- pipelines (ks_sketch.hip, ks_search.hip) ----
// part_pbits > 0: also emit postings partitioned for a join on the top part_pbits hash bits
// allow_defer: the first attempt may return with ks_sketches::pending set (no wait at the end), see there
int ks_sketch_device_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res,
                          u32 max_seq_len, const ks_params *p, int part_pbits, int part_fmt10, int allow_defer, ks_sketches **out);
// After a wait on the stream: the exact counts of a pending sketch.  *redo != 0: the launch has to be repeated the plain way
// (1 compacting tile overflowed, 2 bounded outputs too small, 3 look-back gave up, 4 postings dropped) — the caller frees S.
int ks_sketch_finish_pending(ks_sketches *S, int *redo);
// the fetch segment (ks_stream_wait_fetch) that brings a pending sketch's control block to h_pin + KS_PIN_SKETCH
ks_fetch_seg ks_sketch_pending_seg(const ks_sketches *S);
// bits of hash prefix the join against an index of n_postings uses (buckets of ~3k index postings, <= 16)
int ks_join_pbits(const ks_ctx *ctx, u64 n_postings, u64 per_bucket);
// multiplier of ks_join_prefix (ks_device.h) for a join on pbits prefix bits of hashes kept below max_hash
u32 ks_join_prefix_mul(int pbits, u64 max_hash);
// ---- the deferred sequences of a sketch call (ks_sketch_long.hip) ----
struct sk_args; // the launch arguments of a sketch call (ks_tile.h)
// their lists (n_cls[0] medium, n_cls[1] long ones listed, on the device) and the side buffers their runs are produced in
struct ks_deferred { u32 *med_ids, *long_ids, *n_cls; u64 *lg_hash; u32 *lg_abund; };
// the listed long sequences (at most n_long, none longer than max_len) sketched into the side buffers; the slabs come from sc
int ks_sketch_long_launch(ks_ctx *ctx, const sk_args &A, const ks_deferred &D, u64 n_long, u32 max_len, ks_scratch &sc);
// after the shared tiles (A: their launch): the runs of the listed medium / long sequences into their CSR slots
int ks_sketch_place_launch(ks_ctx *ctx, const sk_args &A, const ks_deferred &D, u64 n_med, u64 n_long);
// ---- k-mer positions (ks_kmerpos.hip, ks_api.hip) ----
int ks_kmerpos_tiles_launch(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_params *p, u32 *d_seq,
                            u32 *d_start, u64 *d_hash, u64 *n_out);
int ks_kmerpos_device_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res,
                           const ks_params *p, ks_kmerpos **out);
int ks_index_build_impl(ks_ctx *ctx, const ks_sketches *t, ks_index **out);
// opts: NULL or validated (ks_search_opts_check); NULL and all-zero options run the same launches
int ks_search_impl(ks_ctx *ctx, const ks_index *ix, const ks_sketches *q, ks_hits **out, int *sketch_redo = nullptr,
                   const ks_search_opts *opts = nullptr);
int ks_search_opts_check(ks_ctx *ctx, const ks_search_opts *opts);
// ---- six-frame translation and the unions (ks_translate.hip, ks_union.hip) ----
int ks_union_impl(ks_ctx *ctx, const ks_sketches *in, ks_sketches **out);
// group_offsets: host, checked by the caller (0 first, in->n_seqs last, ascending); in: of ctx.  Synchronous on return.
int ks_union_groups_impl(ks_ctx *ctx, const ks_sketches *in, const u32 *group_offsets, u32 n_groups, ks_sketches **out);
// the checks of ks_sketch_translated* that need no device, then translate -> sketch the 6 * n_seqs frames -> union by record
int ks_sketch_translated_impl(ks_ctx *ctx, const u8 *d_nt, const u64 *d_offs, u32 n_seqs, u64 n_nt, u32 max_seq_len, const ks_params *p,
                              ks_sketches **out);

// ---- low-complexity masking (ks_mask.hip): mask -> split at min_len = ksize -> sketch the segments -> union by record ----
// behind the entry points' NULL checks; opts: NULL for the defaults
int ks_sketch_masked_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, u32 max_seq_len, const ks_params *p,
                          const ks_mask_opts *opts, ks_sketches **out);
int ks_kmerpos_masked_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_params *p,
                           const ks_mask_opts *opts, ks_kmerpos **out);
int ks_mask_device_impl(ks_ctx *ctx, const u8 *d_res, const u64 *d_offs, u32 n_seqs, u64 n_res, const ks_mask_opts *opts, ks_mask **out);
// what the options are refused for ("<what> options: ..."), for the entry points that upload before they call the above
int ks_mask_opts_check(ks_ctx *ctx, const char *what, const ks_mask_opts *opts);

int ks_check_params(ks_ctx *ctx, const ks_params *p);
// two objects were made with the same parameters: all five fields
bool ks_same_params(const ks_params &a, const ks_params &b);
// ... or KS_ERR_INVALID_ARG "<pass>: <the sketch sets / the tables> were made with different parameters (k, scaled, moltype)"
int ks_params_check_same(ks_ctx *ctx, const char *pass, const char *noun, const ks_params &a, const ks_params &b);
// every input that is not NULL belongs to ctx, or KS_ERR_INVALID_ARG "<pass>: an input of another context"
template <typename... In>
static inline int ks_inputs_check_ctx(ks_ctx *ctx, const char *pass, const In *...in) {
    if (((!in || in->ctx == ctx) && ...)) return KS_OK;
    return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: an input of another context", pass);
}
// the flags / reserved words of an options struct: "<what> options: reserved must be 0" / "... unknown flags"; ctx may be NULL
int ks_opts_words_check(ks_ctx *ctx, const char *what, u32 flags, u32 allowed, u32 reserved);
// gapped slots -> plain CSR (see ks_sketches); no-op for dense sketches.  Enqueued on ctx's stream.
int ks_sketches_make_dense(ks_ctx *ctx, ks_sketches *s);

// ---- boundary copies (ks_copy.hip): one DMA for pinned host memory, double-buffered pinned staging + copy threads otherwise
int ks_copy_h2d(ks_ctx *ctx, void *dst_device, const void *src_host, size_t bytes); // enqueued; complete for pageable sources
int ks_copy_d2h(ks_ctx *ctx, void *dst_host, const void *src_device, size_t bytes); // returns when dst holds the data
void ks_copy_engine_destroy(ks_ctx *ctx);
