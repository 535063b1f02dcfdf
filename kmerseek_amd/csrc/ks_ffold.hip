// ks_ffold.hip — ks_frames_fold_device: the hit rows of a translated search, whose queries are the 6 n frames of
// ks_translate6_device, folded into one row per (record, strand, target), and the regions of the member rows brought onto one
// nucleotide coordinate per strand, so that the chain (ks_rchain.hip) links across frames (include/kmerseek_amd.h has the
// contract).  Integer work on ids and extents only: no residues, bound by latency and bytes.
//
// The three frames of a strand are the consecutive queries 3 x, 3 x + 1, 3 x + 2 (x = 2 s + strand), each segment of the hit list
// sorted by target: a strand's rows are one contiguous run of the input, and the folded order (x, tid) is the stable 3-way
// merge of its segments, the lower frame first among equal targets.
//
//   plan     k_ff_plan, a thread per input row (and per record: the offsets are checked): the four segment bounds of its strand
//            (ks_query_row_begin); its place in the merge = the strand's first row + its index in its own segment + the rows
//            of the two other segments that come before it (ks_lower_bound_u32 of its target there; an equal target of a lower
//            frame comes before it too, and makes it no head).  A head also finds its members in the higher frames.  It writes,
//            at its merged position, the head flag and its region count; qid, order and row_offsets are checked.  Both arrays
//            are zeroed first: a refused row writes neither, and the scans must not read what the pool block held before.
//   scans    head flags -> folded row ids (ks_scan_u32_inplace, the total is the folded row count); region counts -> the region
//            offsets in merged order (ks_scan_u32_to_u64_wide: counts of a row_offsets that lies can add up to anything).
//   rows     k_ff_rows, a thread per input row: src_row[3 r + frame]; a head adds up intersect (saturating) and n_weighted of
//            its at most three members and writes the folded hit row and its row offset.  No atomics.
//   regions  k_ff_regions, a thread per input region: its row (the last row whose offset is <= it), the frame's length from the
//            record's, the two end checks, and the mapped columns at region offset of the row + index inside the row: reads
//            coalesced, writes contiguous per row.
// Every index that leads to a store is held against the capacity of its array: rows that are out of order or offsets that lie
// are named with the call's one wait and cannot make a kernel write outside its blocks.  The result does not depend on the
// launch geometry.
#include "ks_rkit.h"

#define FF_THREADS 256
#define FF_NONE KS_FFOLD_NONE
#define FF_MAX_LEN 0xfffffff0ULL // bases of a record, as ks_translate6_device takes them
enum : u32 { FF_BAD_OFFS = 0, FF_BAD_LONG = 1, FF_BAD_QID = 2, FF_BAD_ORDER = 3, FF_BAD_CSR = 4, FF_BAD_QEND = 5, FF_BAD_TEND = 6, FF_N_BAD = 7, FF_FOLDED = 7 };

struct ff_in {
    const u32 *qid, *tid, *isect; // n_rows
    const u64 *nw;
    const u64 *nt_offs;           // n_records + 1
    const u64 *row_offs;          // n_rows + 1
    const u32 *qs, *ql, *ts, *tl; // n
    const i64 *score;             // n or NULL, as ident and alen
    const u32 *ident, *alen;
    u32 n_records, n_rows, n;
};
// per input row: its merged position (FF_NONE: a row the plan refused), whether it is the first member of its folded row, and a
// head's members in the next two frames
struct ff_plan { u32 *mpos, *is_head, *mate; };
struct ff_out {
    u32 *qid, *tid, *isect; // the folded hit list
    u64 *nw;
    u32 *src_row;           // 3 per folded row
    u64 *row_offs;
    u32 *src_region;        // per folded region, as every column below
    u8 *frame;
    u32 *nt_length, *s_start, *nt_start, *t_start3, *t_length3;
    i64 *score;
    u32 *ident, *alen;
};

__global__ __launch_bounds__(FF_THREADS) void k_ff_plan(ff_in I, ff_plan P, u32 *heads, u32 *cnt, unsigned long long *bad) {
    const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
    if (i < I.n_records) {
        const u64 a = I.nt_offs[i], e = I.nt_offs[i + 1];
        if (e < a || (i == 0 && a != 0)) ks_first_bad(bad, FF_BAD_OFFS, (u32)i);
        else if (e - a > FF_MAX_LEN) ks_first_bad(bad, FF_BAD_LONG, (u32)i);
    }
    if (i >= I.n_rows) return;
    const u32 r = (u32)i, q = I.qid[r], t = I.tid[r];
    P.mpos[r] = FF_NONE; P.is_head[r] = 0u; P.mate[2 * (u64)r] = FF_NONE; P.mate[2 * (u64)r + 1] = FF_NONE;
    if (r > 0) {
        const u32 pq = I.qid[r - 1], pt = I.tid[r - 1];
        if (pq > q || (pq == q && pt >= t)) ks_first_bad(bad, FF_BAD_ORDER, r);
    }
    const u64 b = I.row_offs[r], e = I.row_offs[r + 1];
    u32 c = 0;
    if ((r == 0 && b != 0) || b > e || e > I.n || (r == I.n_rows - 1 && e != I.n)) ks_first_bad(bad, FF_BAD_CSR, r);
    else c = (u32)(e - b);
    if ((u64)q >= 6ULL * I.n_records) { ks_first_bad(bad, FF_BAD_QID, r); return; }
    const u32 f = q % 3u, s3 = q - f;
    u32 sb[4]; // the first rows of the strand's three frames, and of the next strand
#pragma unroll
    for (u32 g = 0; g < 4; g++) sb[g] = s3 + g < s3 ? I.n_rows : ks_query_row_begin(I.qid, I.n_rows, s3 + g);
    u32 pos = sb[0] + (r - sb[f]);
    bool head = true;
#pragma unroll
    for (u32 g = 0; g < 3; g++) {
        if (g == f) continue;
        const u32 len = sb[g + 1] >= sb[g] ? sb[g + 1] - sb[g] : 0u; // (rows out of order: named above, nothing is read past a bound)
        const u32 lb = ks_lower_bound_u32(I.tid + sb[g], len, t);
        const bool has = lb < len && I.tid[sb[g] + lb] == t;
        pos += lb + ((g < f && has) ? 1u : 0u);
        if (has && g < f) head = false;
        if (has && g > f) P.mate[2 * (u64)r + (g - f - 1u)] = sb[g] + lb;
    }
    if (pos < I.n_rows) { P.mpos[r] = pos; P.is_head[r] = head ? 1u : 0u; heads[pos] = head ? 1u : 0u; cnt[pos] = c; }
}

// fid_before: the exclusive scan of the head flags in merged order; m_offs: of the region counts (n_rows + 1 entries)
__global__ __launch_bounds__(FF_THREADS) void k_ff_rows(ff_in I, ff_plan P, const u32 *fid_before, const u64 *m_offs, ff_out O) {
    const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
    if (i >= I.n_rows) return;
    const u32 r = (u32)i, p = P.mpos[r];
    if (p >= I.n_rows) return;
    const bool head = P.is_head[r] != 0u;
    const u32 fid = head ? fid_before[p] : fid_before[p] - 1u; // (a member's head lies before it and is counted)
    if (fid >= I.n_rows) return;
    const u32 q = I.qid[r];
    O.src_row[3 * (u64)fid + q % 3u] = r;
    if (head) {
        u64 is = I.isect[r], nw = I.nw[r];
#pragma unroll
        for (u32 j = 0; j < 2; j++) {
            const u32 m = P.mate[2 * (u64)r + j];
            if (m < I.n_rows) { is += I.isect[m]; nw += I.nw[m]; }
        }
        O.qid[fid] = q / 3u; O.tid[fid] = I.tid[r]; O.isect[fid] = is > 0xffffffffULL ? 0xffffffffu : (u32)is; O.nw[fid] = nw;
        O.row_offs[fid] = m_offs[p];
    }
    if (p == I.n_rows - 1) O.row_offs[(u64)fid + 1] = m_offs[I.n_rows];
}

__global__ __launch_bounds__(FF_THREADS) void k_ff_regions(ff_in I, ff_plan P, const u64 *m_offs, ff_out O, unsigned long long *bad) {
    const u64 j = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
    if (j >= I.n) return;
    const u32 r = ks_last_le_u64(I.row_offs, 0, I.n_rows - 1, j);
    const u64 b = I.row_offs[r];
    const u32 q = I.qid[r];
    if ((u64)q >= 6ULL * I.n_records) return; // (named by the plan)
    const u32 s = q / 6u, f = q % 3u;
    const u64 a = I.nt_offs[s], e = I.nt_offs[s + 1];
    const u64 L = e >= a ? e - a : 0;
    const u64 flen = L >= f ? (L - f) / 3u : 0;
    const u64 qs = I.qs[j], ql = I.ql[j], ts = I.ts[j], tl = I.tl[j];
    bool ok = L <= FF_MAX_LEN;
    if (ok && qs + ql > flen) { ks_first_bad(bad, FF_BAD_QEND, (u32)j); ok = false; }
    if (3u * (ts + tl) > 0xffffffffULL) { ks_first_bad(bad, FF_BAD_TEND, (u32)j); ok = false; }
    const u32 p = P.mpos[r];
    if (!ok || p >= I.n_rows || j < b) return;
    const u64 o = m_offs[p] + (j - b);
    if (o >= I.n) return;
    const u32 s_start = f + 3u * (u32)qs; // (3 (qs + ql) <= L <= FF_MAX_LEN: nothing leaves 32 bits)
    O.src_region[o] = (u32)j; O.frame[o] = (u8)(q % 6u); O.nt_length[o] = 3u * (u32)ql; O.s_start[o] = s_start;
    O.nt_start[o] = q % 6u < 3u ? s_start : (u32)(L - f - 3u * (qs + ql));
    O.t_start3[o] = 3u * (u32)ts; O.t_length3[o] = 3u * (u32)tl;
    if (I.score) O.score[o] = I.score[j];
    if (I.ident) O.ident[o] = I.ident[j];
    if (I.alen) O.alen[o] = I.alen[j];
}

int ks_frames_fold_impl(ks_ctx *ctx, const ks_hits *H, const u64 *d_nt_offs, u32 n_records, const ks_rchain_cols &cols, u64 ng, ks_hits *F, ks_ffold *D) {
    const u64 n_rows = H->n_hits;
    KS_TRY(rk_counts_check(ctx, "frame fold", n_rows, ng));
    ks_hits_inherit(F, H);
    F->has_stats = false;
    F->n_hits = 0;
    D->n_rows = 0; D->n_regions = ng; D->n_src_rows = n_rows;
    KS_TRY(F->alloc(ctx, (size_t)n_rows, false, 0)); // (n_folded of them are filled, as of src_row and row_offsets)
    KS_TRY(ks_alloc(ctx, &D->d_src_row, 3 * (size_t)n_rows));
    KS_TRY(ks_alloc(ctx, &D->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, D, D->n_regions));
    if (cols.score) KS_TRY(ks_alloc(ctx, &D->d_score, (size_t)ng));
    if (cols.ident) KS_TRY(ks_alloc(ctx, &D->d_identities, (size_t)ng));
    if (cols.alen) KS_TRY(ks_alloc(ctx, &D->d_aln_length, (size_t)ng));
    if (n_rows == 0) KS_HIP(ctx, hipMemsetAsync(D->d_row_offsets, 0, sizeof(u64), ctx->stream));

    ks_scratch sc(ctx);
    ks_ctl ctl;
    ff_plan P = {nullptr, nullptr, nullptr};
    u32 *heads = nullptr, *cnt = nullptr;
    u64 *m_offs = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_FFOLD, FF_N_BAD, 1));
    KS_TRY(sc.alloc(&P.mpos, (size_t)n_rows)); KS_TRY(sc.alloc(&P.is_head, (size_t)n_rows)); KS_TRY(sc.alloc(&P.mate, 2 * (size_t)n_rows));
    KS_TRY(sc.alloc(&heads, (size_t)n_rows)); KS_TRY(sc.alloc(&cnt, (size_t)n_rows)); KS_TRY(sc.alloc(&m_offs, (size_t)n_rows + 1));

    const ff_in I = {H->d_qid, H->d_tid, H->d_isect, H->d_nw, d_nt_offs, cols.row_offs, cols.qs, cols.ql, cols.ts, cols.tl, cols.score,
                     cols.ident, cols.alen, n_records, (u32)n_rows, (u32)ng};
    const ff_out O = {F->d_qid, F->d_tid, F->d_isect, F->d_nw, D->d_src_row, D->d_row_offsets, D->d_src_region, D->d_frame, D->d_nt_length,
                      D->d_s_start, D->d_nt_start, D->d_t_start3, D->d_t_length3, D->d_score, D->d_identities, D->d_aln_length};
    const u64 n_plan = n_rows > n_records ? n_rows : n_records;
    // A row the plan refuses writes no merged position, and rows out of order collide: what the scans read there must not be
    // whatever the pool block held (words that add up beyond a look-back status word: the call would end as a scan that gave up,
    // not as the named refusal).  Zeroed, the head flags sum to at most n_rows.
    if (n_rows) {
        KS_HIP(ctx, hipMemsetAsync(heads, 0, (size_t)n_rows * sizeof(u32), ctx->stream));
        KS_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)n_rows * sizeof(u32), ctx->stream));
    }
    if (n_plan) KS_LAUNCH(ctx, "ffold_plan", k_ff_plan, (u32)((n_plan + FF_THREADS - 1) / FF_THREADS), FF_THREADS, I, P, heads, cnt, ctl.words());
    if (n_rows) {
        KS_TRY(ks_scan_u32_inplace(ctx, heads, n_rows, ctl.low32(FF_FOLDED)));
        KS_TRY(ks_scan_u32_to_u64_wide(ctx, cnt, m_offs, n_rows));
        KS_HIP(ctx, hipMemsetAsync(D->d_src_row, 0xff, 3 * (size_t)n_rows * sizeof(u32), ctx->stream));
        KS_LAUNCH(ctx, "ffold_rows", k_ff_rows, (u32)((n_rows + FF_THREADS - 1) / FF_THREADS), FF_THREADS, I, P, (const u32 *)heads, (const u64 *)m_offs, O);
        if (ng) KS_LAUNCH(ctx, "ffold_regions", k_ff_regions, (u32)((ng + FF_THREADS - 1) / FF_THREADS), FF_THREADS, I, P, (const u64 *)m_offs, O, ctl.words());
    }
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    if (ctl.bad(FF_BAD_OFFS))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: the record offsets do not start at 0 and ascend: record %llu breaks it", (unsigned long long)ctl[FF_BAD_OFFS]);
    if (ctl.bad(FF_BAD_LONG))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: record %llu is longer than 2^32 - 16 bases", (unsigned long long)ctl[FF_BAD_LONG]);
    if (ctl.bad(FF_BAD_QID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: hit row %llu names a query beyond the %llu frames of %u records", (unsigned long long)ctl[FF_BAD_QID],
                       6ULL * n_records, n_records);
    if (ctl.bad(FF_BAD_ORDER))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: the hit rows do not ascend strictly by (qid, tid): hit row %llu does not come after the row before it",
                       (unsigned long long)ctl[FF_BAD_ORDER]);
    if (ctl.bad(FF_BAD_CSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: row_offsets is not a CSR from 0 to %llu regions that never descends: hit row %llu breaks it",
                       (unsigned long long)ng, (unsigned long long)ctl[FF_BAD_CSR]);
    if (ctl.bad(FF_BAD_QEND))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: region %llu ends beyond the last residue of its frame", (unsigned long long)ctl[FF_BAD_QEND]);
    if (ctl.bad(FF_BAD_TEND))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame fold: region %llu ends beyond target position (2^32 - 1) / 3", (unsigned long long)ctl[FF_BAD_TEND]);
    F->n_hits = D->n_rows = n_rows ? (ctl[FF_FOLDED] & 0xffffffffULL) : 0;
    return KS_OK;
}
