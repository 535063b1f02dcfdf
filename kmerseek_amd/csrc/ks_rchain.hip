// ks_rchain.hip — ks_regions_chain_device: per hit row the best colinear chain of its regions (alignments, extended regions), and
// ks_rchain_coverage: how much of the two sequences that chain explains (include/kmerseek_amd.h has the contract).  Like the
// cull (ks_rcull.hip) a pass over extents and scores: no residues, all of it in signed 64-bit integers, bound by latency and
// lane use.  The program is the cull's greedy loop with another step: the regions of a row are visited in the order of
// (q_start, input index) — follows() needs a strictly smaller q_start, so every predecessor of a region comes before it — and
// the region visited has its final `best`; every later region relaxes its running (value, pred) against it.
//
//   plan    k_rh_plan, a thread per hit row and per region: row_offsets is checked — 0 first, n_regions last, never descending —
//           before anything is indexed by it (a row that breaks it is named and taken by no kernel), a region with a length of 0,
//           an end beyond 0xffffffff or |score| > 2^30 is named.  Rows of 0 and 1 regions are settled here; every other row goes
//           onto one of three segment lists as (row, regions), with one atomic per workgroup and list (ks_seg_list_push_block):
//   lanes   k_rh_lanes<8>: 2 .. 8 regions, a group of 8 lanes per row, 8 rows per wave; k_rh_lanes<64>: 9 .. 64 regions, a wave
//           per row.  One program: a lane holds a region; its rank is the number of lanes before it by (q_start, index); step p:
//           a ballot finds the lane of rank p, it broadcasts its extents and its best (an i64 as two 32-bit words), every lane
//           tests follows() and relaxes.  Then a butterfly argmax picks the end region, the group walks back along pred (every
//           lane keeps the same cursor, a member learns its distance from the end), and butterfly sums give the row's columns.
//   wg      k_rh_wg, a workgroup of 256 threads per row: rank by counting, order[rank] = region, then blocked: wave 0 finalises a
//           tile of 64 consecutive ranks among themselves (the lane program) and leaves it in LDS, then all threads relax their
//           regions (thread t owns regions t, t + 256, ... and is the only writer of their (value, pred) outside a tile's
//           finalising) against the finished tile: two barriers per 64 regions, not per region.  A row of up to RH_LDS_ROWS
//           regions is staged in LDS (40 bytes per region: 30 KiB, and 1.75 KiB of tile); a longer one runs the SAME function on
//           the input columns, the result's best and pred columns and one u32 per region of global scratch.  One thread walks the chain back; the members add their shares of
//           the row's sums with integer LDS atomics: any order gives the same sums.
//   emit    the member flags -> one-launch exclusive scan -> src_region in chain order (a member's place inside its row's
//           block is its distance from the chain's first member) and the result's row_offsets.
//   cover   k_rh_cover, a thread per row: one f64 division of two integers per side.
// The result does not depend on the path a row took (KS_DEBUG_CHAIN_PATH = 1 every row of <= 64 regions by a wave, 2 every row
// by a workgroup, 3 as 2 with RH_LDS_ROWS_SMALL so that small rows take the global path) or on the launch geometry.  One host wait.
#include "ks_rkit.h"

#define RH_THREADS 256
#define RH_PLAN_THREADS 1024 // k_rh_plan: one atomic per workgroup and list
#define RH_GROUP 8           // lanes of a group of k_rh_lanes<8>
#define RH_LDS_ROWS 768      // regions of a row k_rh_wg stages in LDS (40 bytes each: 30 KiB)
#define RH_LDS_ROWS_SMALL 32 // ... under KS_DEBUG_CHAIN_PATH = 3
#define RH_LANES_GRID 1024   // workgroups of k_rh_lanes (4 waves each, striding over the listed rows)
#define RH_WG_GRID 2048      // workgroups of k_rh_wg (striding likewise)
#define RH_NONE KS_RCHAIN_NONE
#define RH_SCORE_MAX (1LL << 30)
enum : u32 { RH_BAD_CSR = 0, RH_BAD_LEN = 1, RH_BAD_END = 2, RH_BAD_SCORE = 3, RH_N_BAD = 4 };
enum : u32 { RH_COV_BAD_ID = 0, RH_COV_BAD_LEN = 1, RH_COV_N_BAD = 2 };

struct rh_in {
    const u64 *row_offs;
    const u32 *qs, *ql, *ts, *tl;
    const i64 *score;
    const u32 *ident, *alen; // may be NULL
    u32 n_rows, n;
    i64 max_gap, max_ov, link, skew, ovc; // max_gap 0: no limit
};
struct rh_out {
    i64 *best;                 // per input region
    u32 *pred;
    u32 *flag, *place, *first; // per input region (scratch): a member; its place in the chain; its row's first region
    i64 *chain_score;          // per row
    u32 *q_start, *q_length, *t_start, *t_length, *q_aligned, *t_aligned;
    u64 *identities, *aln_length;
    double *row_score;
};
// the columns of one row
struct rh_row {
    i64 score;
    u64 qs, qe, ts, te, qa, ta, ident, alen; // (qe - qs, te - ts, qa, ta <= 0xffffffff: the plan admits no end beyond it)
};

KS_DEV void rh_row_store(const rh_out &O, u32 r, const rh_row &R, bool empty) {
    O.chain_score[r] = R.score; O.row_score[r] = empty ? ks_nan() : (double)R.score;
    O.q_start[r] = (u32)R.qs; O.q_length[r] = (u32)(R.qe - R.qs); O.t_start[r] = (u32)R.ts; O.t_length[r] = (u32)(R.te - R.ts);
    O.q_aligned[r] = (u32)R.qa; O.t_aligned[r] = (u32)R.ta; O.identities[r] = R.ident; O.aln_length[r] = R.alen;
}
// What linking a (ends aqe, ate; its starts lie in aqs, ats) in front of b costs, or -1 where b does not follow a.  Everything
// is below 2^33 before the products and the costs are at most 2^16: nothing leaves 64 bits.
KS_DEV i64 rh_link(const rh_in &I, i64 aqs, i64 aqe, i64 ats, i64 ate, i64 bqs, i64 bqe, i64 bts, i64 bte) {
    if (!(aqs < bqs && ats < bts && aqe < bqe && ate < bte)) return -1;
    const i64 dq = bqs - aqe, dt = bts - ate;
    const i64 lo = dq < dt ? dq : dt, hi = dq > dt ? dq : dt;
    const i64 ov = lo < 0 ? -lo : 0;
    if (ov > I.max_ov || (I.max_gap > 0 && hi > I.max_gap)) return -1;
    return I.link + I.skew * (hi - lo) + I.ovc * ov;
}
// candidate (value c through region j) beats the running (value v, pred p): a link is taken only where c > 0, and among equal
// values the smaller index wins (v starts at 0 with p = RH_NONE)
KS_DEV bool rh_better(i64 c, u32 j, i64 v, u32 p) { return c > v || (c == v && c > 0 && j < p); }
// (best a at index i) comes before (best b at index j) as the end of a chain
KS_DEV bool rh_end_before(i64 a, u32 i, i64 b, u32 j) { return a > b || (a == b && i < j); }

// mode: 0 by length, 1 every row of <= 64 regions to k_rh_lanes<64>, 2 every row to k_rh_wg.  (No thread leaves early: the
// pushes are the workgroup's.)
__global__ __launch_bounds__(RH_PLAN_THREADS) void k_rh_plan(rh_in I, int mode, u32 *seg8, u32 *seg64, u32 *segwg, rh_out O, unsigned long long *bad) {
    __shared__ u32 s_push[2];
    const u64 i = (u64)blockIdx.x * RH_PLAN_THREADS + threadIdx.x;
    if (i < I.n) {
        const u32 ql = I.ql[i], tl = I.tl[i];
        const i64 s = I.score[i];
        if (ql == 0 || tl == 0) ks_first_bad(bad, RH_BAD_LEN, (u32)i);
        if ((u64)I.qs[i] + ql > 0xffffffffULL || (u64)I.ts[i] + tl > 0xffffffffULL) ks_first_bad(bad, RH_BAD_END, (u32)i);
        if (s > RH_SCORE_MAX || s < -RH_SCORE_MAX) ks_first_bad(bad, RH_BAD_SCORE, (u32)i);
    }
    const u32 r = (u32)i;
    u32 len = 0, to = 0; // the list the row goes onto: 1 seg8, 2 seg64, 3 segwg, 0 none
    if (i < I.n_rows) {
        const u64 b = I.row_offs[r], e = I.row_offs[r + 1];
        if ((r == 0 && b != 0) || b > e || e > I.n || (r == I.n_rows - 1 && e != I.n)) ks_first_bad(bad, RH_BAD_CSR, r);
        else if (e == b) rh_row_store(O, r, rh_row{0, 0, 0, 0, 0, 0, 0, 0, 0}, true);
        else if (e - b == 1 && mode == 0) { // [b, e) lies inside [0, n)
            const u64 qs = I.qs[b], ts = I.ts[b], ql = I.ql[b], tl = I.tl[b];
            O.best[b] = I.score[b]; O.pred[b] = RH_NONE; O.flag[b] = 1u; O.place[b] = 0u; O.first[b] = (u32)b;
            rh_row_store(O, r, rh_row{I.score[b], qs, qs + ql, ts, ts + tl, ql, tl, I.ident ? I.ident[b] : 0u, I.alen ? I.alen[b] : 0u}, false);
        } else {
            len = (u32)(e - b);
            to = mode == 2 || len > 64 ? 3u : (mode == 1 || len > RH_GROUP) ? 2u : 1u;
        }
    }
    ks_seg_list_push_block(seg8, I.n_rows, to == 1u, r, len, s_push);
    ks_seg_list_push_block(seg64, I.n_rows, to == 2u, r, len, s_push);
    ks_seg_list_push_block(segwg, I.n_rows, to == 3u, r, len, s_push);
}

// lane j's value inside the group of W lanes; j is the same in every lane of the group (W == 64: v_readlane; else a width-W shuffle)
template <u32 W> KS_DEV u32 rh_from(u32 v, u32 j) {
    if constexpr (W == 64) return (u32)__builtin_amdgcn_readlane((int)v, (int)ks_readfirst(j));
    else return (u32)__shfl((int)v, (int)j, (int)W);
}
template <u32 W> KS_DEV i64 rh_from64(i64 v, u32 j) { return (i64)(((u64)rh_from<W>((u32)((u64)v >> 32), j) << 32) | rh_from<W>((u32)(u64)v, j)); }
KS_DEV u64 rh_xor64(u64 v, u32 m, u32 w) { return ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), (int)m, (int)w) << 32) | (u32)__shfl_xor((int)(u32)v, (int)m, (int)w); }
template <u32 W> KS_DEV u64 rh_group_sum(u64 v) {
    for (u32 m = 1; m < W; m <<= 1) v += rh_xor64(v, m, W);
    return v;
}

// A group of W lanes per listed row, 64 / W rows per wave (all 64 lanes run every step: the ballots and shuffles see whole
// waves; a group without a row, or past its row's ranks, relaxes nothing).
template <u32 W> __global__ __launch_bounds__(RH_THREADS) void k_rh_lanes(rh_in I, const u32 *segs, rh_out O) {
    constexpr u32 G = 64 / W;
    const u32 lane = threadIdx.x & 63, sub = lane % W, gsh = (lane / W) * W;
    const u64 gmask = W == 64 ? ~0ULL : (1ULL << (W & 63)) - 1ULL;
    const u32 n_list = segs[0] < I.n_rows ? segs[0] : I.n_rows;
    const u64 n_waves = (u64)gridDim.x * (RH_THREADS / 64);
    for (u64 w = (u64)blockIdx.x * (RH_THREADS / 64) + (threadIdx.x >> 6); w * G < n_list; w += n_waves) { // (wave-uniform)
        const u64 si = w * G + lane / W;
        u32 r = 0, len = 0;
        u64 b = 0;
        if (si < n_list) {
            r = segs[1 + 2 * si]; len = segs[2 + 2 * si];
            if (r < I.n_rows && len <= W) b = I.row_offs[r]; else len = 0; // (the plan lists nothing else)
        }
        const bool valid = sub < len;
        const u32 g = (u32)(b + sub);
        u32 qs = 0, ql = 1, ts = 0, tl = 1;
        i64 sc = 0;
        if (valid) { qs = I.qs[g]; ql = I.ql[g]; ts = I.ts[g]; tl = I.tl[g]; sc = I.score[g]; }
        const i64 qe = (i64)qs + ql, te = (i64)ts + tl;
        u32 rk = 0; // the lanes of the row that come before this one by (q_start, index)
        for (u32 j = 0; j < W; j++) {
            if (!__ballot(j < len)) break;
            const u32 qj = rh_from<W>(qs, j);
            rk += (j < len && (qj < qs || (qj == qs && j < sub))) ? 1u : 0u;
        }
        i64 val = 0, pqe = 0, pte = 0; // the best value to link from, and that predecessor's ends
        u32 pred = RH_NONE;            // (a lane of the group)
        for (u32 p = 0; p < W; p++) {
            if (!__ballot(p < len)) break;
            const u64 own = (__ballot(valid && rk == p) >> gsh) & gmask;
            const u32 src = own ? (u32)__ffsll((long long)own) - 1u : 0u; // the lane of rank p: its best is final
            const i64 aqs = rh_from<W>(qs, src), ats = rh_from<W>(ts, src);
            const i64 aqe = aqs + rh_from<W>(ql, src), ate = ats + rh_from<W>(tl, src);
            const i64 ab = rh_from64<W>(sc + val, src);
            const i64 cost = rh_link(I, aqs, aqe, ats, ate, qs, qe, ts, te);
            if (own && valid && cost >= 0 && rh_better(ab - cost, src, val, pred)) { val = ab - cost; pred = src; pqe = aqe; pte = ate; }
        }
        const i64 best = sc + val;
        // the end region: the largest best, the smaller index among equals
        i64 eb = valid ? best : INT64_MIN;
        u32 ei = valid ? sub : RH_NONE;
        for (u32 m = 1; m < W; m <<= 1) {
            const i64 ob = (i64)rh_xor64((u64)eb, m, W);
            const u32 oi = (u32)__shfl_xor((int)ei, (int)m, (int)W);
            if (rh_end_before(ob, oi, eb, ei)) { eb = ob; ei = oi; }
        }
        // back along pred: every lane of the group keeps the same cursor
        u32 cur = ei, firstl = 0, back = RH_NONE, nmem = 0;
        for (u32 s = 0; s < W; s++) {
            if (!__ballot(cur != RH_NONE)) break;
            const u32 nxt = rh_from<W>(pred, cur == RH_NONE ? 0u : cur);
            if (cur != RH_NONE) { if (sub == cur) back = s; firstl = cur; nmem = s + 1; cur = nxt; }
        }
        const bool member = back != RH_NONE;
        // the union of the members' intervals: starts and ends ascend along the chain
        const u64 qa = rh_group_sum<W>(!member ? 0 : pred == RH_NONE ? (u64)ql : (u64)(qe - ((i64)qs > pqe ? (i64)qs : pqe)));
        const u64 ta = rh_group_sum<W>(!member ? 0 : pred == RH_NONE ? (u64)tl : (u64)(te - ((i64)ts > pte ? (i64)ts : pte)));
        const u64 sid = rh_group_sum<W>(member && I.ident ? I.ident[g] : 0u), sal = rh_group_sum<W>(member && I.alen ? I.alen[g] : 0u);
        const u32 fe = ei == RH_NONE ? 0u : ei;
        const u64 fqs = rh_from<W>(qs, firstl), fts = rh_from<W>(ts, firstl);
        const u64 lqe = (u64)rh_from<W>(qs, fe) + rh_from<W>(ql, fe), lte = (u64)rh_from<W>(ts, fe) + rh_from<W>(tl, fe);
        if (valid) {
            O.best[g] = best; O.pred[g] = pred == RH_NONE ? RH_NONE : (u32)(b + pred);
            O.flag[g] = member ? 1u : 0u; O.place[g] = member ? nmem - 1u - back : 0u; O.first[g] = (u32)b;
            if (sub == 0) rh_row_store(O, r, rh_row{eb, fqs, lqe, fts, lte, qa, ta, sid, sal}, false);
        }
    }
}

// a finished tile of 64 consecutive ranks, in LDS: what every later region relaxes against
struct rh_tile { u32 qs[64], ql[64], ts[64], tl[64], idx[64]; i64 best[64]; };

// One row by the workgroup (all 256 threads enter; everything but the array contents is uniform).  The arrays hold the row's
// `len` regions — LDS copies, or the input columns, the result's best / pred columns and global scratch at the row's first
// region b.  val: the running value, pred: the predecessor inside the row; order: the rank order, later a member's distance
// from the chain's end.  T, s_red / s_ri (4 words each), s_sum (4 sums), s_walk (2 words): LDS.
KS_DEV void rh_wg_row(const rh_in &I, const rh_out &O, u32 r, u32 b, u32 len, const u32 *qs, const u32 *ql, const u32 *ts, const u32 *tl,
                      const i64 *sc, u32 *order, i64 *val, u32 *pred, rh_tile &T, i64 *s_red, u32 *s_ri, unsigned long long *s_sum, u32 *s_walk) {
    const u32 t = threadIdx.x;
    for (u32 j = t; j < len; j += RH_THREADS) {
        const u32 qj = qs[j];
        u32 cnt = 0;
        for (u32 i = 0; i < len; i++) { const u32 qi = qs[i]; cnt += (qi < qj || (qi == qj && i < j)) ? 1u : 0u; }
        if (cnt < len) order[cnt] = j; // (a permutation: the ranks are distinct)
        val[j] = 0; pred[j] = RH_NONE;
    }
    if (t < 4) s_sum[t] = 0;
    for (u32 p0 = 0; p0 < len; p0 += 64) { // a tile of 64 consecutive ranks
        __syncthreads(); // order is written; the tile's regions have been relaxed against every earlier tile by their owners
        const u32 nt = len - p0 < 64u ? len - p0 : 64u;
        if (t < 64) { // wave 0 finalises the tile among itself: the lane program, lane = rank inside the tile
            u32 i = t < nt ? order[p0 + t] : RH_NONE;
            const bool on = i < len; // (always where t < nt)
            if (!on) i = 0;
            const u32 mqs = qs[i], mql = ql[i], mts = ts[i], mtl = tl[i];
            const i64 msc = sc[i], mqe = (i64)mqs + mql, mte = (i64)mts + mtl;
            i64 v = val[i];
            u32 pr = pred[i];
            for (u32 s = 0; s + 1 < nt; s++) { // lane s is final
                const i64 aqs = rh_from<64>(mqs, s), ats = rh_from<64>(mts, s);
                const i64 aqe = aqs + rh_from<64>(mql, s), ate = ats + rh_from<64>(mtl, s), ab = rh_from64<64>(msc + v, s);
                const u32 ai = rh_from<64>(i, s);
                const i64 cost = rh_link(I, aqs, aqe, ats, ate, mqs, mqe, mts, mte);
                if (on && cost >= 0 && rh_better(ab - cost, ai, v, pr)) { v = ab - cost; pr = ai; }
            }
            if (on) {
                val[i] = v; pred[i] = pr;
                T.qs[t] = mqs; T.ql[t] = mql; T.ts[t] = mts; T.tl[t] = mtl; T.idx[t] = i; T.best[t] = msc + v;
            }
        }
        __syncthreads();
        // every region against the finished tile, from LDS.  (A region of this tile or of an earlier one gains nothing: it
        // follows no member it has not met, and rh_better is idempotent.)
        for (u32 j = t; j < len; j += RH_THREADS) {
            const i64 bqs = qs[j], bts = ts[j], bqe = bqs + ql[j], bte = bts + tl[j];
            i64 v = val[j];
            u32 pr = pred[j];
            for (u32 k = 0; k < nt; k++) {
                const i64 aqs = T.qs[k], ats = T.ts[k];
                const i64 cost = rh_link(I, aqs, aqs + T.ql[k], ats, ats + T.tl[k], bqs, bqe, bts, bte);
                if (cost >= 0 && rh_better(T.best[k] - cost, T.idx[k], v, pr)) { v = T.best[k] - cost; pr = T.idx[k]; }
            }
            val[j] = v; pred[j] = pr;
        }
    }
    __syncthreads();
    // the end region
    i64 eb = INT64_MIN;
    u32 ei = RH_NONE;
    for (u32 j = t; j < len; j += RH_THREADS) {
        const i64 bj = sc[j] + val[j];
        if (rh_end_before(bj, j, eb, ei)) { eb = bj; ei = j; }
    }
    for (u32 m = 1; m < 64; m <<= 1) {
        const i64 ob = (i64)rh_xor64((u64)eb, m, 64);
        const u32 oi = (u32)__shfl_xor((int)ei, (int)m, 64);
        if (rh_end_before(ob, oi, eb, ei)) { eb = ob; ei = oi; }
    }
    if ((t & 63) == 0) { s_red[t >> 6] = eb; s_ri[t >> 6] = ei; }
    for (u32 j = t; j < len; j += RH_THREADS) order[j] = RH_NONE; // (the ranks are used up)
    __syncthreads();
    for (u32 w = 0; w < RH_THREADS / 64; w++)
        if (rh_end_before(s_red[w], s_ri[w], eb, ei)) { eb = s_red[w]; ei = s_ri[w]; }
    if (t == 0) { // back along pred
        u32 s = 0, cur = ei, first = ei;
        while (cur < len && s < len) { order[cur] = s++; first = cur; cur = pred[cur]; }
        s_walk[0] = s; s_walk[1] = first;
    }
    __syncthreads();
    const u32 nmem = s_walk[0], first = s_walk[1];
    for (u32 j = t; j < len; j += RH_THREADS) {
        const u32 back = order[j], pj = pred[j];
        const bool member = back != RH_NONE;
        if (member) {
            const i64 q0 = qs[j], t0 = ts[j], q1 = q0 + ql[j], t1 = t0 + tl[j];
            i64 qa = ql[j], ta = tl[j];
            if (pj < len) {
                const i64 pqe = (i64)qs[pj] + ql[pj], pte = (i64)ts[pj] + tl[pj];
                qa = q1 - (q0 > pqe ? q0 : pqe); ta = t1 - (t0 > pte ? t0 : pte);
            }
            atomicAdd(&s_sum[0], (unsigned long long)qa); atomicAdd(&s_sum[1], (unsigned long long)ta);
            if (I.ident) atomicAdd(&s_sum[2], (unsigned long long)I.ident[b + j]);
            if (I.alen) atomicAdd(&s_sum[3], (unsigned long long)I.alen[b + j]);
        }
        O.flag[b + j] = member ? 1u : 0u; O.place[b + j] = member ? nmem - 1u - back : 0u; O.first[b + j] = b;
        O.best[b + j] = sc[j] + val[j]; // (val may BE this column: this thread's own element)
        O.pred[b + j] = pj < len ? b + pj : RH_NONE;
    }
    __syncthreads();
    if (t == 0 && ei < len && first < len)
        rh_row_store(O, r, rh_row{eb, qs[first], (u64)qs[ei] + ql[ei], ts[first], (u64)ts[ei] + tl[ei], s_sum[0], s_sum[1], s_sum[2], s_sum[3]}, false);
}

// chunk: the longest row that is staged (<= RH_LDS_ROWS); g_order: one u32 per input region, for the longer rows
__global__ __launch_bounds__(RH_THREADS) void k_rh_wg(rh_in I, const u32 *segs, u32 chunk, u32 *g_order, rh_out O) {
    __shared__ u32 s_qs[RH_LDS_ROWS], s_ql[RH_LDS_ROWS], s_ts[RH_LDS_ROWS], s_tl[RH_LDS_ROWS], s_order[RH_LDS_ROWS], s_pred[RH_LDS_ROWS];
    __shared__ i64 s_sc[RH_LDS_ROWS], s_val[RH_LDS_ROWS], s_red[RH_THREADS / 64];
    __shared__ unsigned long long s_sum[4];
    __shared__ u32 s_ri[RH_THREADS / 64], s_walk[2];
    __shared__ rh_tile s_tile;
    for (ks_seg_walk seg = ks_seg_list_by_wg(segs, I.n_rows); seg.next();) {
        const u32 r = seg.b, len = seg.len;
        if (r >= I.n_rows) continue;
        const u64 b64 = rk_readfirst64(I.row_offs[r]);
        if (b64 + len > I.n) continue; // (the plan lists nothing else)
        const u32 b = (u32)b64;
        __syncthreads(); // (the previous row's last readers of the staged arrays)
        if (len <= chunk) {
            for (u32 j = threadIdx.x; j < len; j += RH_THREADS) {
                s_qs[j] = I.qs[b + j]; s_ql[j] = I.ql[b + j]; s_ts[j] = I.ts[b + j]; s_tl[j] = I.tl[b + j]; s_sc[j] = I.score[b + j];
            }
            __syncthreads();
            rh_wg_row(I, O, r, b, len, s_qs, s_ql, s_ts, s_tl, s_sc, s_order, s_val, s_pred, s_tile, s_red, s_ri, s_sum, s_walk);
        } else
            rh_wg_row(I, O, r, b, len, I.qs + b, I.ql + b, I.ts + b, I.tl + b, I.score + b, g_order + b, O.best + b, O.pred + b, s_tile, s_red, s_ri, s_sum, s_walk);
    }
}

// the members to their places in chain order, and the result's row_offsets: the members before each row's first region
__global__ __launch_bounds__(RH_THREADS) void k_rh_emit(rh_in I, rh_out O, const u64 *pos, u32 *o_src, u64 *o_offs) {
    const u64 i = (u64)blockIdx.x * RH_THREADS + threadIdx.x;
    if (i < I.n && O.flag[i]) {
        const u32 f = O.first[i];
        const u64 o = (f < I.n ? pos[f] : I.n) + O.place[i];
        if (o < I.n) o_src[o] = (u32)i;
    }
    if (i <= I.n_rows) {
        const u64 b = I.row_offs[i];
        o_offs[i] = pos[b < I.n ? b : I.n];
    }
}

int ks_regions_chain_impl(ks_ctx *ctx, const ks_rchain_cols &cols, u64 n_rows, u64 ng, const ks_rchain_opts *o, ks_rchain *K) {
    K->n_rows = n_rows; K->n_regions = ng; K->n_chained = 0;
    KS_TRY(rk_counts_check(ctx, "region chain", n_rows, ng));
    KS_TRY(ks_alloc(ctx, &K->d_row_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_alloc(ctx, &K->d_src_region, (size_t)ng)); // (n_chained of them are filled)
    KS_TRY(ks_obj_alloc(ctx, K, K->n_regions));
    KS_TRY(ks_obj_alloc(ctx, K, K->n_rows));
    if (n_rows == 0 || ng == 0) KS_HIP(ctx, hipMemsetAsync(K->d_row_offsets, 0, ((size_t)n_rows + 1) * sizeof(u64), ctx->stream));
    if (n_rows == 0) return ks_stream_wait(ctx); // (ng == 0: the caller has checked)

    bool small; // (tests: every row one way; 3 = the workgroup path with a small LDS capacity)
    const int mode = ks_seg_path_knob(ctx, KS_DBG_CHAIN_PATH, &small);
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u32 *seg8 = nullptr, *seg64 = nullptr, *segwg = nullptr, *flag = nullptr, *place = nullptr, *first = nullptr, *g_order = nullptr;
    u64 *pos = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RCHAIN, RH_N_BAD, 0));
    KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &seg8)); KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &seg64));
    KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)n_rows, &segwg));
    KS_TRY(sc.alloc(&flag, (size_t)ng)); KS_TRY(sc.alloc(&place, (size_t)ng)); KS_TRY(sc.alloc(&first, (size_t)ng));
    KS_TRY(sc.alloc(&g_order, (size_t)ng)); KS_TRY(sc.alloc(&pos, (size_t)ng + 1));

    const rh_in I = {cols.row_offs, cols.qs, cols.ql, cols.ts, cols.tl, cols.score, cols.ident, cols.alen, (u32)n_rows, (u32)ng,
                     (i64)o->max_gap, (i64)o->max_overlap, (i64)o->link_cost, (i64)o->skew_cost, (i64)o->overlap_cost};
    const rh_out O = {K->d_best, K->d_pred, flag, place, first, K->d_chain_score, K->d_q_start, K->d_q_length, K->d_t_start, K->d_t_length,
                      K->d_q_aligned, K->d_t_aligned, K->d_identities, K->d_aln_length, K->d_row_score};
    const u64 n_plan = n_rows > ng ? n_rows : ng;
    KS_LAUNCH(ctx, "rchain_plan", k_rh_plan, (u32)((n_plan + RH_PLAN_THREADS - 1) / RH_PLAN_THREADS), RH_PLAN_THREADS, I, mode, seg8, seg64, segwg, O, ctl.words());
    u64 *const hk = ctx->h_pin + KS_PIN_RCHAIN + RH_N_BAD;
    *hk = 0;
    if (ng == 0) KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    else {
        if (mode == 0) KS_LAUNCH(ctx, "rchain_lanes8", k_rh_lanes<RH_GROUP>, RH_LANES_GRID, RH_THREADS, I, (const u32 *)seg8, O);
        if (mode != 2) KS_LAUNCH(ctx, "rchain_lanes64", k_rh_lanes<64>, RH_LANES_GRID, RH_THREADS, I, (const u32 *)seg64, O);
        KS_LAUNCH(ctx, "rchain_wg", k_rh_wg, RH_WG_GRID, RH_THREADS, I, (const u32 *)segwg, small ? RH_LDS_ROWS_SMALL : RH_LDS_ROWS, g_order, O);
        KS_TRY(ks_scan_u32_to_u64(ctx, flag, pos, ng));
        const u64 n_emit = n_rows + 1 > ng ? n_rows + 1 : ng;
        KS_LAUNCH(ctx, "rchain_emit", k_rh_emit, (u32)((n_emit + RH_THREADS - 1) / RH_THREADS), RH_THREADS, I, O, (const u64 *)pos, K->d_src_region, K->d_row_offsets);
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(pos + ng, hk, 2)}));
    }
    if (ctl.bad(RH_BAD_CSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain: row_offsets is not a CSR from 0 to %llu regions that never descends: hit row %llu breaks it",
                       (unsigned long long)ng, (unsigned long long)ctl[RH_BAD_CSR]);
    if (ctl.bad(RH_BAD_LEN))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain: region %llu has a length of 0: nothing follows it and it follows nothing",
                       (unsigned long long)ctl[RH_BAD_LEN]);
    if (ctl.bad(RH_BAD_END))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain: region %llu ends beyond position 0xffffffff", (unsigned long long)ctl[RH_BAD_END]);
    if (ctl.bad(RH_BAD_SCORE))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "region chain: region %llu has a score beyond +-2^30", (unsigned long long)ctl[RH_BAD_SCORE]);
    K->n_chained = *hk;
    return KS_OK;
}

// mode: 0 the query's share, 1 the target's, 2 the smaller, 3 the larger; NaN for a row without a chain or a sequence of length 0
__global__ __launch_bounds__(RH_THREADS) void k_rh_cover(const u64 *c_offs, const u32 *qa, const u32 *ta, const u32 *qid, const u32 *tid, const u64 *q_off,
                                                         u32 n_q, const u64 *t_off, u32 n_t, u32 n_rows, u32 mode, double *cov, unsigned long long *bad) {
    const u64 i = (u64)blockIdx.x * RH_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    const u32 r = (u32)i, q = qid[r], t = tid[r];
    double v = ks_nan();
    if (q >= n_q || t >= n_t) ks_first_bad(bad, RH_COV_BAD_ID, r);
    else {
        const u64 qb = q_off[q], qe = q_off[q + 1], tb = t_off[t], te = t_off[t + 1];
        const u64 Lq = qe >= qb ? qe - qb : 0, Lt = te >= tb ? te - tb : 0, a = qa[r], c = ta[r];
        if (a > Lq || c > Lt) ks_first_bad(bad, RH_COV_BAD_LEN, r);
        else if (c_offs[r + 1] != c_offs[r]) {
            const double cq = Lq ? (double)a / (double)Lq : ks_nan(), ct = Lt ? (double)c / (double)Lt : ks_nan();
            v = mode == 0 ? cq : mode == 1 ? ct : (cq != cq || ct != ct) ? ks_nan() : mode == 2 ? (cq < ct ? cq : ct) : (cq > ct ? cq : ct);
        }
    }
    cov[r] = v;
}

static int rh_cover_run(ks_ctx *ctx, ks_rchain *K, const ks_hits *H, const u64 *d_q_off, u32 n_q, const u64 *d_t_off, u32 n_t, u32 mode) {
    ks_scratch sc(ctx);
    ks_ctl ctl;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_RCHAIN_COV, RH_COV_N_BAD, 0));
    KS_LAUNCH(ctx, "rchain_cover", k_rh_cover, (u32)((K->n_rows + RH_THREADS - 1) / RH_THREADS), RH_THREADS, (const u64 *)K->d_row_offsets,
              (const u32 *)K->d_q_aligned, (const u32 *)K->d_t_aligned, (const u32 *)H->d_qid, (const u32 *)H->d_tid, d_q_off, n_q, d_t_off, n_t,
              (u32)K->n_rows, mode, K->d_row_cov, ctl.words());
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    if (ctl.bad(RH_COV_BAD_ID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "chain coverage: hit row %llu names a sequence beyond the %u queries or the %u targets",
                       (unsigned long long)ctl[RH_COV_BAD_ID], n_q, n_t);
    if (ctl.bad(RH_COV_BAD_LEN))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "chain coverage: the chain of hit row %llu covers more positions than its sequence has: these are not the sequences of the chained regions",
                       (unsigned long long)ctl[RH_COV_BAD_LEN]);
    return KS_OK;
}
int ks_rchain_coverage_impl(ks_ctx *ctx, ks_rchain *K, const ks_hits *H, const u64 *d_q_off, u32 n_q, const u64 *d_t_off, u32 n_t, u32 mode) {
    if (!K->d_row_cov) KS_TRY(ks_alloc(ctx, &K->d_row_cov, (size_t)K->n_rows));
    if (K->n_rows == 0) return KS_OK;
    const int st = rh_cover_run(ctx, K, H, d_q_off, n_q, d_t_off, n_t, mode);
    if (st != KS_OK) { ks_pool_free(ctx, K->d_row_cov); K->d_row_cov = nullptr; } // (a refused call leaves no column)
    return st;
}

extern "C" uint32_t ks_debug_rchain_lds_rows(uint32_t *small_rows) {
    if (small_rows) *small_rows = RH_LDS_ROWS_SMALL;
    return RH_LDS_ROWS;
}
