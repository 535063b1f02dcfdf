// ks_pileup.hip — coverage (include/kmerseek_amd.h has the contract): the alignments of a hit list reduced ACROSS the hit rows
// onto the residues of one batch — per residue the depth and, on request, the counts of the residue classes aligned to it, per
// sequence covered / max_depth / depth_sum and the two quotients.  Everything but the quotients is an integer; every add is an
// integer atomic or a scan, so the order entries are taken in never shows.
//
//   csr      k_pu_csr, a lane per offset: both CSRs ascend and end at their counts.
//   entries  k_pu_entries, a wave per entry (a run of CIGAR ops of one hit row).  Before anything is indexed by them: the row
//            that owns the entry, its mask byte, the ids, the sequences inside their batches, the op range.  Then the ops are
//            read twice.  Once to judge them: the codes, and what they consume on either side against what the sequences have
//            from the starts.  Only an entry that passed writes: lanes over the ops, 64 at a time, a DPP scan gives each op its
//            position; every maximal run of pair ops is one interval, +1 in `begins` at its first residue and +1 in `ends` one
//            past its last (two atomics per run, not per column: 1= 1X 1= ... is one run).  With the profile the pair ops of
//            the chunk are replayed one after the other, lanes over the columns: the residue of the other side is read and one
//            add goes to counts[p][class].  A weighted pileup (k_pu_entries<., PU_W_SUM>) replays the runs also without the
//            profile: the entry's weight goes to wdepth[p] and, with the profile, to wcounts[p][class], 64-bit integer atomics.
//   weights  ks_entry_weights_device.  k_pw_classes, 28 lanes a residue: k_p, the classes seen at the residue, one byte.  Then
//            k_pu_entries<true, PU_W_MAKE>: the same judgement, nothing piled up; the replay reads per column one byte k_p and
//            one count, each lane sums floor(2^30 / (k_p * cnt)) in 64 bits, the wave reduces, lane 0 stores the mean.
//   scans    two ks_scan_u32_inplace.  depth[p] = begins up to p - ends up to p.  Two unsigned arrays and not one of signed
//            marks: the one-launch scan carries a tile's running sum in 38 bits of its status word, a run of "negative" u32
//            tile sums passes that after 64 tiles.
//   seqs     k_pu_seq_wave, a wave per sequence: the offsets are checked, the length written, a sequence of at most
//            PU_WAVE_MAX residues reduced on the spot, a longer one listed for k_pu_seq_group (a workgroup per sequence).  Both
//            write depth[] as they read the two scans (KS_DEBUG_PILEUP_PATH = 1 / 2: every sequence by a wave / a workgroup).
// One host wait.  A refused call names the first offender of the first kind.
#include "ks_rkit.h"

#define PU_THREADS 256
#define PU_A RK_A
#define PU_WAVE_MAX 1024u  // the longest sequence a wave reduces (ks_debug_pileup_limits)
#define PU_GROUP_GRID 2048
enum : u32 { PU_M = 0, PU_I = 1, PU_D = 2, PU_N = KS_CIGAR_FSHIFT, PU_EQ = 7, PU_X = 8 }; // BAM op codes
enum : u32 { PU_BAD_ROWCSR = 0, PU_BAD_OPCSR = 1, PU_BAD_ID = 2, PU_BAD_OP = 3, PU_BAD_EXTENT = 4, PU_BAD_SEQ = 5, PU_BAD_OFFS = 6, PU_N_BAD = 7,
             PU_BAD_COUNTS = 7, PW_N_BAD = 8 }; // (the weights pass alone: a column the counts do not hold)
enum : int { PU_W_NONE = 0, PU_W_SUM = 1, PU_W_MAKE = 2 }; // k_pu_entries: no weights | the entries' weights summed | the weights made

struct pu_args {
    const u64 *row_offs;            // n_rows + 1, or NULL: entry e is row e
    const u64 *op_offs;             // n_entries + 1
    const u32 *ops;                 // n_ops
    const u32 *start, *other_start; // n_entries
    const u8 *row_mask;             // n_rows or NULL
    const u32 *qid, *tid;           // n_rows
    const u64 *s_offs;              // the side's batch
    const u8 *o_res;                // the other batch (profile)
    const u64 *o_offs;
    u64 n_ops, n_s_res, n_o_res;
    u32 n_rows, n_entries, n_s, n_o, side;
    u32 *begins, *ends;             // n_s_res + 2 each
    u32 *counts, *n_aln;
    unsigned long long *bad;
    // a weighted pileup: the entries' weights, and where they are summed
    const u32 *weight;              // n_entries
    unsigned long long *wdepth, *wcounts;
    // the weights pass: the side's residues (NULL: the sequence itself is no member of its columns), the classes seen per
    // residue (k_pw_classes), the counts they were made from, and the two columns made
    const u8 *s_res, *n_classes;
    const u32 *in_counts;
    u32 *out_weight, *out_cols;
};

KS_DEV bool pu_is_pair(u32 c) { return c == PU_M || c == PU_EQ || c == PU_X; }
KS_DEV bool pu_is_op(u32 c) { return c <= PU_N || c == PU_EQ || c == PU_X; }

__global__ __launch_bounds__(PU_THREADS) void k_pu_csr(pu_args A) {
    const u64 i = (u64)blockIdx.x * PU_THREADS + threadIdx.x;
    if (A.row_offs) {
        if (i < A.n_rows && A.row_offs[i] > A.row_offs[i + 1]) ks_first_bad(A.bad, PU_BAD_ROWCSR, (u32)i);
        if (i == A.n_rows && A.row_offs[i] != A.n_entries) ks_first_bad(A.bad, PU_BAD_ROWCSR, (u32)i);
    }
    if (i < A.n_entries && A.op_offs[i] > A.op_offs[i + 1]) ks_first_bad(A.bad, PU_BAD_OPCSR, (u32)i);
    if (i == A.n_entries && A.op_offs[i] != A.n_ops) ks_first_bad(A.bad, PU_BAD_OPCSR, (u32)i);
}

template <bool PROFILE, int W = PU_W_NONE>
__global__ __launch_bounds__(PU_THREADS) void k_pu_entries(pu_args A) {
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 e64 = (u64)blockIdx.x * (PU_THREADS / 64) + wave;
    if (e64 >= A.n_entries) return;
    const u32 e = (u32)e64;
    u32 row = e;
    if (A.row_offs) { // (a CSR that is none is named by k_pu_csr; the search stays inside [0, n_rows) whatever it holds)
        row = ks_readfirst(ks_last_le_u64(A.row_offs, 0, A.n_rows - 1, e));
        if (e < rk_readfirst64(A.row_offs[row]) || e >= rk_readfirst64(A.row_offs[row + 1])) return;
    }
    if (A.row_mask && !ks_readfirst(A.row_mask[row])) return;
    const bool on_q = A.side == KS_PILEUP_QUERY, reads_q = on_q || PROFILE;
    const u32 q = ks_readfirst(A.qid[row]), t = ks_readfirst(A.tid[row]);
    const u32 sid = on_q ? q : t, oid = on_q ? t : q;
    if (sid >= A.n_s || (PROFILE && oid >= A.n_o)) {
        if (lane == 0) ks_first_bad(A.bad, PU_BAD_ID, row);
        return;
    }
    const u64 sb = rk_readfirst64(A.s_offs[sid]), se = rk_readfirst64(A.s_offs[(u64)sid + 1]);
    u64 ob = 0, oe = 0;
    if (PROFILE) { ob = rk_readfirst64(A.o_offs[oid]); oe = rk_readfirst64(A.o_offs[(u64)oid + 1]); }
    if (sb > se || se > A.n_s_res || ob > oe || oe > A.n_o_res) {
        if (lane == 0) ks_first_bad(A.bad, PU_BAD_SEQ, e);
        return;
    }
    const u64 kb = rk_readfirst64(A.op_offs[e]), ke = rk_readfirst64(A.op_offs[e64 + 1]);
    if (kb > ke || ke > A.n_ops) return; // (k_pu_csr names it)
    const u32 c_side = on_q ? PU_I : PU_D, c_other = on_q ? PU_D : PU_I; // the gap op that consumes the side / the other side

    // the ops judged: nothing is written for an entry that fails
    u64 ns = 0, no = 0, np = 0;
    bool bad_op = false;
    for (u64 k = kb + lane; k < ke; k += 64) {
        const u32 op = A.ops[k], len = op >> 4, c = op & 15u;
        if (!pu_is_op(c) || (c == PU_N && reads_q)) bad_op = true;
        const bool pair = pu_is_pair(c);
        if (pair || c == c_side) ns += len;
        if (pair || c == c_other) no += len;
        if (pair) np += len;
    }
    if (__ballot(bad_op)) {
        if (lane == 0) ks_first_bad(A.bad, PU_BAD_OP, e);
        return;
    }
    ns = ks_wave_sum64(ns); no = ks_wave_sum64(no); np = ks_wave_sum64(np);
    const u32 s0 = ks_readfirst(A.start[e]), o0 = PROFILE ? ks_readfirst(A.other_start[e]) : 0u;
    if ((u64)s0 + ns > se - sb || (PROFILE && (u64)o0 + no > oe - ob)) {
        if (lane == 0) ks_first_bad(A.bad, PU_BAD_EXTENT, e);
        return;
    }
    if (np == 0) return;
    if (W != PU_W_MAKE && lane == 0) atomicAdd(&A.n_aln[sid], 1u);
    const u32 wt = W == PU_W_SUM ? ks_readfirst(A.weight[e]) : 0u;
    u64 term_sum = 0;     // PU_W_MAKE: this lane's column terms
    bool no_count = false; //            a column whose count is 0

    // (from here on every position lies inside [sb, se] and [ob, oe): 32 bits hold the offsets into the two sequences)
    u32 spos = s0, opos = o0;
    for (u64 k0 = kb; k0 < ke; k0 += 64) {
        const u64 k = k0 + lane;
        const bool have = k < ke;
        const u32 op = have ? A.ops[k] : 0u, len = op >> 4, c = have ? (op & 15u) : 15u;
        const bool pair = pu_is_pair(c);
        const u32 ds = (pair || c == c_side) ? len : 0u;
        const u32 is = ks_wave_incl_scan(ds), xs = spos + is - ds; // where the op begins on the side
        if (W != PU_W_MAKE && pair) {
            const bool prev = k > kb && pu_is_pair(A.ops[k - 1] & 15u), next = k + 1 < ke && pu_is_pair(A.ops[k + 1] & 15u);
            if (!prev) atomicAdd(&A.begins[sb + xs], 1u);
            if (!next) atomicAdd(&A.ends[sb + xs + len], 1u);
        }
        if (PROFILE || (W == PU_W_SUM && wt != 0)) {
            u32 io = 0, xo = 0;
            if (PROFILE) {
                const u32 dx = (pair || c == c_other) ? len : 0u;
                io = ks_wave_incl_scan(dx); xo = opos + io - dx;
            }
            u64 m = __ballot(pair && len != 0);
            m = ((u64)ks_readfirst((u32)(m >> 32)) << 32) | ks_readfirst((u32)m);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const u32 L = (u32)__builtin_amdgcn_readlane((int)len, j);
                const u64 ps = sb + (u32)__builtin_amdgcn_readlane((int)xs, j), po = ob + (u32)__builtin_amdgcn_readlane((int)xo, j);
                if (W == PU_W_NONE) {
                    for (u32 i = lane; i < L; i += 64) atomicAdd(&A.counts[(ps + i) * PU_A + rk_class(A.o_res[po + i])], 1u);
                } else if (W == PU_W_SUM) {
                    for (u32 i = lane; i < L; i += 64) {
                        if (PROFILE) {
                            const u64 at = (ps + i) * PU_A + rk_class(A.o_res[po + i]);
                            atomicAdd(&A.counts[at], 1u);
                            if (wt) atomicAdd(&A.wcounts[at], (unsigned long long)wt);
                        }
                        if (wt) atomicAdd(&A.wdepth[ps + i], (unsigned long long)wt);
                    }
                } else {
                    for (u32 i = lane; i < L; i += 64) {
                        const u32 cl = rk_class(A.o_res[po + i]);
                        const u32 cn = A.in_counts[(ps + i) * PU_A + cl] + ((A.s_res && rk_class(A.s_res[ps + i]) == cl) ? 1u : 0u);
                        const u32 kp = A.n_classes[ps + i]; // (cn != 0: the class is one of the kp seen, kp >= 1)
                        if (cn == 0) no_count = true;
                        else term_sum += (u64)KS_WEIGHT_ONE / ((u64)kp * cn);
                    }
                }
            }
            if (PROFILE) opos += (u32)__builtin_amdgcn_readlane((int)io, 63);
        }
        spos += (u32)__builtin_amdgcn_readlane((int)is, 63);
    }
    if (W == PU_W_MAKE) {
        if (__ballot(no_count)) {
            if (lane == 0) ks_first_bad(A.bad, PU_BAD_COUNTS, e);
            return;
        }
        term_sum = ks_wave_sum64(term_sum);
        if (lane == 0) { A.out_weight[e] = (u32)(term_sum / np); A.out_cols[e] = (u32)np; }
    }
}

// the weights pass: per residue of the side's batch the classes with a count, the residue's own class counted in with s_res
__global__ __launch_bounds__(PU_THREADS) void k_pw_classes(const u32 *counts, const u8 *s_res, u64 n_res, u8 *n_classes) {
    const u64 p = ((u64)blockIdx.x * PU_THREADS + threadIdx.x) >> 5;
    const u32 c = threadIdx.x & 31;
    bool seen = false;
    if (p < n_res && c < PU_A) seen = counts[p * PU_A + c] != 0 || (s_res && rk_class(s_res[p]) == c);
    const u64 b = __ballot(seen);
    if (c == 0 && p < n_res) n_classes[p] = (u8)__popc((u32)(b >> (threadIdx.x & 32)));
}
// ... and the offsets of the side's batch, which the pileup judges while it reduces the sequences
__global__ __launch_bounds__(PU_THREADS) void k_pw_offs(const u64 *offs, u32 n_seqs, u64 n_res, unsigned long long *bad) {
    const u64 s = (u64)blockIdx.x * PU_THREADS + threadIdx.x;
    if (s < n_seqs && (offs[s] > offs[s + 1] || offs[s + 1] > n_res)) ks_first_bad(bad, PU_BAD_OFFS, (u32)s);
}

// ---------------------------------------------------------------------------------------------
// per sequence
// ---------------------------------------------------------------------------------------------
struct pu_seq_args {
    const u64 *offs;
    u32 n_seqs;
    u64 n_res;
    const u32 *begins, *ends; // scanned: [p + 1] = the intervals that begin / end at or before p
    u32 *depth, *length, *covered, *max_depth;
    u64 *depth_sum;
    double *breadth, *mean_depth;
    u32 *list, list_cap;
    unsigned long long *bad;
};
KS_DEV void pu_seq_store(const pu_seq_args &A, u32 s, u32 len, u32 cov, u32 mx, u64 sum) {
    A.covered[s] = cov; A.max_depth[s] = mx; A.depth_sum[s] = sum;
    A.breadth[s] = (double)cov / (double)len; A.mean_depth[s] = (double)sum / (double)len; // (0 / 0: NaN for an empty sequence)
}

// mode: 0 by length, 1 every sequence by a wave, 2 every sequence by a workgroup
__global__ __launch_bounds__(PU_THREADS) void k_pu_seq_wave(pu_seq_args A, int mode) {
    const u32 lane = threadIdx.x & 63, w = ks_readfirst(threadIdx.x >> 6);
    const u64 s64 = (u64)blockIdx.x * (PU_THREADS / 64) + w;
    if (s64 >= A.n_seqs) return;
    const u32 s = (u32)s64;
    const u64 b = rk_readfirst64(A.offs[s]), e = rk_readfirst64(A.offs[s64 + 1]);
    if (b > e || e > A.n_res) {
        if (lane == 0) { ks_first_bad(A.bad, PU_BAD_OFFS, s); A.length[s] = 0; pu_seq_store(A, s, 0, 0, 0, 0); }
        return;
    }
    const u32 len = (u32)(e - b); // (n_res < 2^32)
    if (lane == 0) A.length[s] = len;
    if (mode == 2 || (mode == 0 && len > PU_WAVE_MAX)) {
        if (lane == 0) ks_seg_list_push(A.list, A.list_cap, s, len);
        return;
    }
    u32 cov = 0, mx = 0;
    u64 sum = 0;
    for (u32 i = lane; i < len; i += 64) {
        const u32 d = A.begins[b + i + 1] - A.ends[b + i + 1];
        A.depth[b + i] = d;
        cov += d ? 1u : 0u; mx = d > mx ? d : mx; sum += d;
    }
    cov = (u32)ks_wave_sum64(cov); mx = ks_wave_max_u32(mx); sum = ks_wave_sum64(sum);
    if (lane == 0) pu_seq_store(A, s, len, cov, mx, sum);
}

__global__ __launch_bounds__(PU_THREADS) void k_pu_seq_group(pu_seq_args A) {
    __shared__ u32 s_cov[PU_THREADS / 64], s_mx[PU_THREADS / 64];
    __shared__ u64 s_sum[PU_THREADS / 64];
    const u32 t = threadIdx.x, w = t >> 6;
    for (ks_seg_walk seg = ks_seg_list_by_wg(A.list, A.list_cap); seg.next();) {
        const u32 s = seg.b;
        if (s >= A.n_seqs) continue; // (the list holds nothing else; uniform, as every `continue` here)
        const u64 b = rk_readfirst64(A.offs[s]), e = rk_readfirst64(A.offs[(u64)s + 1]);
        if (b > e || e > A.n_res) continue;
        const u32 len = (u32)(e - b);
        u32 cov = 0, mx = 0;
        u64 sum = 0;
        for (u32 i = t; i < len; i += PU_THREADS) {
            const u32 d = A.begins[b + i + 1] - A.ends[b + i + 1];
            A.depth[b + i] = d;
            cov += d ? 1u : 0u; mx = d > mx ? d : mx; sum += d;
        }
        cov = (u32)ks_wave_sum64(cov); mx = ks_wave_max_u32(mx); sum = ks_wave_sum64(sum);
        __syncthreads(); // (the previous item's reader)
        if ((t & 63) == 0) { s_cov[w] = cov; s_mx[w] = mx; s_sum[w] = sum; }
        __syncthreads();
        if (t == 0) {
            for (u32 k = 1; k < PU_THREADS / 64; k++) { cov += s_cov[k]; mx = s_mx[k] > mx ? s_mx[k] : mx; sum += s_sum[k]; }
            pu_seq_store(A, s, len, cov, mx, sum);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// the entries of a call as the entry points hand them on (n_rows is the hit list's)
struct pu_entries {
    const u64 *row_offs, *op_offs;
    const u32 *ops;
    u64 n_rows, n_entries, n_ops;
    const u32 *start, *other_start;
};

// the first offender of the first kind, named: what the pileup and the weights pass refuse alike
static int pu_refuse(ks_ctx *ctx, const ks_ctl &ctl, const pu_entries &E, const ks_res_batch &S, bool profile);

// weighted: d_weight holds one weight per entry, and the pileup also sums them (wdepth, with the profile wcounts)
static int pu_run(ks_ctx *ctx, const pu_entries &E, const u8 *d_row_mask, const ks_hits *H, const ks_res_batch &S, const ks_res_batch &O, u32 side,
                  bool profile, bool weighted, const u32 *d_weight, ks_pileup *P) {
    const u64 ns = S.n_seqs, nr = S.n_res;
    P->n_seqs = ns; P->n_residues = nr; P->n_profile = profile ? nr * PU_A : 0;
    KS_TRY(ks_alloc(ctx, &P->d_depth, (size_t)nr));
    KS_TRY(ks_alloc(ctx, &P->d_counts, (size_t)P->n_profile));
    KS_TRY(ks_obj_alloc(ctx, P, P->n_seqs));
    if (weighted) {
        P->n_weighted = nr; P->n_wprofile = P->n_profile;
        KS_TRY(ks_alloc(ctx, &P->d_wdepth, (size_t)nr));
        KS_TRY(ks_alloc(ctx, &P->d_wcounts, (size_t)P->n_wprofile));
        if (nr) KS_HIP(ctx, hipMemsetAsync(P->d_wdepth, 0, (size_t)nr * sizeof(u64), ctx->stream));
        if (P->n_wprofile) KS_HIP(ctx, hipMemsetAsync(P->d_wcounts, 0, (size_t)P->n_wprofile * sizeof(u64), ctx->stream));
    }
    KS_HIP(ctx, hipMemsetAsync(P->d_n_alignments, 0, (ns ? ns : 1) * sizeof(u32), ctx->stream));
    if (profile && nr) KS_HIP(ctx, hipMemsetAsync(P->d_counts, 0, (size_t)P->n_profile * sizeof(u32), ctx->stream));

    ks_scratch sc(ctx);
    ks_ctl ctl;
    u32 *begins = nullptr, *ends = nullptr, *list = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_PILEUP, PU_N_BAD, 0));
    KS_TRY(sc.alloc(&begins, (size_t)nr + 2));
    KS_TRY(sc.alloc(&ends, (size_t)nr + 2));
    KS_HIP(ctx, hipMemsetAsync(begins, 0, ((size_t)nr + 2) * sizeof(u32), ctx->stream));
    KS_HIP(ctx, hipMemsetAsync(ends, 0, ((size_t)nr + 2) * sizeof(u32), ctx->stream));

    const pu_args A = {E.row_offs, E.op_offs, E.ops, E.start, E.other_start, d_row_mask, H->d_qid, H->d_tid, S.offs, O.res, O.offs,
                       E.n_ops, nr, O.n_res, (u32)E.n_rows, (u32)E.n_entries, S.n_seqs, O.n_seqs, side, begins, ends, P->d_counts,
                       P->d_n_alignments, ctl.words(), d_weight, (unsigned long long *)P->d_wdepth, (unsigned long long *)P->d_wcounts,
                       nullptr, nullptr, nullptr, nullptr, nullptr};
    const u64 n_off = (E.n_rows > E.n_entries ? E.n_rows : E.n_entries) + 1;
    KS_LAUNCH(ctx, "pileup_csr", k_pu_csr, (u32)((n_off + PU_THREADS - 1) / PU_THREADS), PU_THREADS, A);
    if (E.n_entries) {
        const u32 grid = (u32)((E.n_entries + PU_THREADS / 64 - 1) / (PU_THREADS / 64));
        if (weighted && profile) KS_LAUNCH(ctx, "pileup_profile_weighted", (k_pu_entries<true, PU_W_SUM>), grid, PU_THREADS, A);
        else if (weighted) KS_LAUNCH(ctx, "pileup_marks_weighted", (k_pu_entries<false, PU_W_SUM>), grid, PU_THREADS, A);
        else if (profile) KS_LAUNCH(ctx, "pileup_profile", k_pu_entries<true>, grid, PU_THREADS, A);
        else KS_LAUNCH(ctx, "pileup_marks", k_pu_entries<false>, grid, PU_THREADS, A);
    }
    KS_TRY(ks_scan_u32_inplace(ctx, begins, nr + 1, nullptr));
    KS_TRY(ks_scan_u32_inplace(ctx, ends, nr + 1, nullptr));
    if (ns) {
        bool unused;
        const int mode = ks_seg_path_knob(ctx, KS_DBG_PILEUP_PATH, &unused);
        KS_TRY(ks_seg_list_alloc(ctx, sc, (size_t)ns, &list));
        const pu_seq_args Q = {S.offs, S.n_seqs, nr, begins, ends, P->d_depth, P->d_length, P->d_covered, P->d_max_depth, P->d_depth_sum,
                               P->d_breadth, P->d_mean_depth, list, S.n_seqs, ctl.words()};
        KS_LAUNCH(ctx, "pileup_seq_wave", k_pu_seq_wave, (u32)((ns + PU_THREADS / 64 - 1) / (PU_THREADS / 64)), PU_THREADS, Q, mode);
        if (mode != 1) KS_LAUNCH(ctx, "pileup_seq_group", k_pu_seq_group, (u32)(ns < PU_GROUP_GRID ? ns : PU_GROUP_GRID), PU_THREADS, Q);
    }
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch()}));
    return pu_refuse(ctx, ctl, E, S, profile);
}

static int pu_refuse(ks_ctx *ctx, const ks_ctl &ctl, const pu_entries &E, const ks_res_batch &S, bool profile) {
    const u64 nr = S.n_res;
    const auto at = [&](u32 i) { return (unsigned long long)ctl[i]; };
    if (ctl.bad(PU_BAD_ROWCSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: row_offsets descends at hit row %llu or does not end at the %llu entries", at(PU_BAD_ROWCSR),
                       (unsigned long long)E.n_entries);
    if (ctl.bad(PU_BAD_OPCSR))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: op_offsets descends at entry %llu or does not end at the %llu ops", at(PU_BAD_OPCSR),
                       (unsigned long long)E.n_ops);
    if (ctl.bad(PU_BAD_ID))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: hit row %llu names a sequence beyond its batch (%u on the side%s)", at(PU_BAD_ID), S.n_seqs,
                       profile ? ", the other batch likewise" : "");
    if (ctl.bad(PU_BAD_OP))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: entry %llu holds an op that is none of M I D N = X, or an N where the query side is read",
                       at(PU_BAD_OP));
    if (ctl.bad(PU_BAD_EXTENT))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: the ops of entry %llu consume more of a sequence than it has from the entry's start",
                       at(PU_BAD_EXTENT));
    if (ctl.bad(PU_BAD_SEQ))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: entry %llu lies on a sequence whose offsets descend or pass its batch", at(PU_BAD_SEQ));
    if (ctl.bad(PU_BAD_OFFS))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: the offsets of sequence %llu descend or pass the batch's %llu residues", at(PU_BAD_OFFS),
                       (unsigned long long)nr);
    return KS_OK;
}

// what the options are refused for; ctx may be NULL.  has_other: the other batch and the entries' starts on it were given
static int pu_opts_check(ks_ctx *ctx, const ks_pileup_opts *opts, bool has_other, ks_pileup_opts *o) {
    *o = opts ? *opts : ks_pileup_opts{0u, KS_PILEUP_QUERY, 0ull};
    KS_TRY(ks_opts_words_check(ctx, "pileup", o->flags, KS_PILEUP_PROFILE, o->reserved ? 1u : 0u));
    const char *why = o->side > KS_PILEUP_TARGET ? "side is neither KS_PILEUP_QUERY nor KS_PILEUP_TARGET"
                      : ((o->flags & KS_PILEUP_PROFILE) && !has_other) ? "KS_PILEUP_PROFILE needs the other batch and the entries' starts on it"
                                                                       : nullptr;
    if (!why) return KS_OK;
    return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup options: %s", why) : KS_ERR_INVALID_ARG;
}

// the weights of the entries (include/kmerseek_amd.h has the rule).  S.res: the side's residues with KS_PWEIGHTS_INCLUDE_QUERY, else NULL
static int pw_run(ks_ctx *ctx, const pu_entries &E, const u8 *d_row_mask, const ks_hits *H, const ks_res_batch &S, const ks_res_batch &O, u32 side,
                  const u32 *d_counts, ks_pweights *Wt) {
    const u64 nr = S.n_res;
    Wt->n_entries = E.n_entries;
    KS_TRY(ks_obj_alloc(ctx, Wt, Wt->n_entries));
    if (E.n_entries) {
        KS_HIP(ctx, hipMemsetAsync(Wt->d_weight, 0, (size_t)E.n_entries * sizeof(u32), ctx->stream));
        KS_HIP(ctx, hipMemsetAsync(Wt->d_n_cols, 0, (size_t)E.n_entries * sizeof(u32), ctx->stream));
    }
    ks_scratch sc(ctx);
    ks_ctl ctl;
    u8 *n_classes = nullptr;
    KS_TRY(ctl.init(ctx, sc, KS_PIN_PWEIGHTS, PW_N_BAD, 0));
    KS_TRY(sc.alloc(&n_classes, (size_t)nr + 1));
    const pu_args A = {E.row_offs, E.op_offs, E.ops, E.start, E.other_start, d_row_mask, H->d_qid, H->d_tid, S.offs, O.res, O.offs,
                       E.n_ops, nr, O.n_res, (u32)E.n_rows, (u32)E.n_entries, S.n_seqs, O.n_seqs, side, nullptr, nullptr, nullptr,
                       nullptr, ctl.words(), nullptr, nullptr, nullptr, S.res, n_classes, d_counts, Wt->d_weight, Wt->d_n_cols};
    const u64 n_off = (E.n_rows > E.n_entries ? E.n_rows : E.n_entries) + 1;
    KS_LAUNCH(ctx, "pileup_csr", k_pu_csr, (u32)((n_off + PU_THREADS - 1) / PU_THREADS), PU_THREADS, A);
    if (S.n_seqs) KS_LAUNCH(ctx, "pweights_offsets", k_pw_offs, (u32)(((u64)S.n_seqs + PU_THREADS - 1) / PU_THREADS), PU_THREADS, S.offs, S.n_seqs, nr, ctl.words());
    if (nr) KS_LAUNCH(ctx, "pweights_classes", k_pw_classes, (u32)((nr * 32 + PU_THREADS - 1) / PU_THREADS), PU_THREADS, d_counts, S.res, nr, n_classes);
    if (E.n_entries)
        KS_LAUNCH(ctx, "pweights_entries", (k_pu_entries<true, PU_W_MAKE>), (u32)((E.n_entries + PU_THREADS / 64 - 1) / (PU_THREADS / 64)), PU_THREADS, A);
    const ks_fetch_seg f = ctl.fetch();
    KS_TRY(ks_stream_wait_fetch(ctx, &f, 1));
    KS_TRY(pu_refuse(ctx, ctl, E, S, true));
    if (ctl.bad(PU_BAD_COUNTS))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup weights: entry %llu holds a column that the counts do not: counts of other entries, another mask or "
                                                "another side", (unsigned long long)ctl[PU_BAD_COUNTS]);
    return KS_OK;
}

// what every call is refused for behind its options, before the device: NULL arguments, contexts, counts, capacity
static int pu_precheck(ks_ctx *ctx, const pu_entries &E, const ks_hits *H, const ks_res_batch &S, const void *out) {
    if (!out || !H || !S.offs || !E.op_offs || (E.n_ops && !E.ops) || (E.n_entries && !E.start))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(ks_inputs_check_ctx(ctx, "pileup", H));
    if (E.n_rows != H->n_hits)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: the entries lie in %llu hit rows, the hit list has %llu: alignments of another search",
                       (unsigned long long)E.n_rows, (unsigned long long)H->n_hits);
    if (!E.row_offs && E.n_entries != E.n_rows)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: %llu entries for %llu hit rows without row_offsets", (unsigned long long)E.n_entries,
                       (unsigned long long)E.n_rows);
    if (E.n_rows == 0 && E.n_entries != 0)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: %llu entries in no hit row: row_offsets is not a CSR from 0 to n", (unsigned long long)E.n_entries);
    if (S.n_res >= 0xffffffffULL)
        return ks_fail(ctx, KS_ERR_CAPACITY, "pileup: a batch of %llu residues: one 32-bit scan takes fewer than 2^32 - 1", (unsigned long long)S.n_res);
    KS_TRY(rk_counts_check(ctx, "pileup", E.n_rows, E.n_entries));
    if (E.n_entries >= 0xfffffffeULL || E.n_ops > 0xffffffffULL)
        return ks_fail(ctx, KS_ERR_CAPACITY, "pileup: 2^32 - 2 or more entries, or more than 2^32 - 1 ops");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    return KS_OK;
}
// behind the options: the checks above, then the device.  weighted: d_weight holds a weight per entry
static int pu_checked(ks_ctx *ctx, const pu_entries &E, const u8 *d_row_mask, const ks_hits *H, const ks_res_batch &S, const ks_res_batch &O,
                      const ks_pileup_opts &o, ks_pileup **out, bool weighted = false, const u32 *d_weight = nullptr) {
    const bool profile = (o.flags & KS_PILEUP_PROFILE) != 0;
    if (weighted && E.n_entries && !d_weight) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(pu_precheck(ctx, E, H, S, out));
    ks_result<ks_pileup> P(ctx, out, ks_pileup_free);
    KS_TRY(pu_run(ctx, E, d_row_mask, H, S, profile ? O : ks_res_batch{nullptr, nullptr, 0u, 0ull}, o.side, profile, weighted, d_weight, P));
    return P.commit();
}
// ... of the weights pass: the counts and, with the flag, the side's residues are arguments like the others
static int pw_checked(ks_ctx *ctx, const pu_entries &E, const u8 *d_row_mask, const ks_hits *H, const ks_res_batch &S, const ks_res_batch &O,
                      u32 side, u32 flags, const u32 *d_counts, ks_pweights **out) {
    if ((S.n_res && !d_counts) || ((flags & KS_PWEIGHTS_INCLUDE_QUERY) && S.n_res && !S.res)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    KS_TRY(pu_precheck(ctx, E, H, S, out));
    ks_result<ks_pweights> Wt(ctx, out, ks_pweights_free);
    KS_TRY(pw_run(ctx, E, d_row_mask, H, ks_res_batch{(flags & KS_PWEIGHTS_INCLUDE_QUERY) ? S.res : nullptr, S.offs, S.n_seqs, S.n_res}, O, side, d_counts, Wt));
    return Wt.commit();
}

// What the four entries do alike, in their order: the options (also without a context), the context, *out, the objects the
// entries come from (`in`: not NULL, of ctx), then `run`, which reads them.
template <typename Out, typename Refuse, typename Run, typename... In>
static int pu_entry(ks_ctx *ctx, const ks_pileup_opts *opts, bool has_other, Out **out, Refuse &&refuse, Run &&run, const In *...in) {
    return ks_guard(ctx, [&]() -> int {
    ks_pileup_opts o;
    KS_TRY(pu_opts_check(ctx, opts, has_other, &o));
    if (const char *why = refuse(o)) return ctx ? ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup options: %s", why) : KS_ERR_INVALID_ARG;
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if ((!in || ...)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "NULL argument");
    if constexpr (sizeof...(In) != 0) KS_TRY(ks_inputs_check_ctx(ctx, "pileup", in...));
    return run(o);
    });
}
static const char *pu_any(const ks_pileup_opts &) { return nullptr; }
static bool pu_has_batch(const u8 *d_res, const u64 *d_offs, u64 n_res) { return d_offs && (d_res || !n_res); }

extern "C" int ks_pileup_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops, uint64_t n_rows,
                                uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start,
                                const uint8_t *d_row_mask, const ks_hits *hits, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                                const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                                const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res) && (d_other_start || !n_entries), out, pu_any, [&](const ks_pileup_opts &o) {
        return pu_checked(ctx, pu_entries{d_row_offsets, d_op_offsets, d_ops, n_rows, n_entries, n_ops, d_start, d_other_start}, d_row_mask, hits,
                          ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o, out);
    });
}
extern "C" int ks_cigars_pileup(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_hits *hits, const uint8_t *d_row_mask,
                                const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets,
                                uint32_t n_o_seqs, uint64_t n_o_res, const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res), out, pu_any, [&](const ks_pileup_opts &o) {
        KS_TRY(ks_refuse_by_profile(ctx, "pileup", alignments));
        if (cigars->n_rows != alignments->n_rows || cigars->n_regions != alignments->n_regions)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: the cigars hold %llu regions in %llu hit rows, the alignments %llu in %llu: not traced from them",
                           (unsigned long long)cigars->n_regions, (unsigned long long)cigars->n_rows, (unsigned long long)alignments->n_regions,
                           (unsigned long long)alignments->n_rows);
        const bool on_q = o.side == KS_PILEUP_QUERY;
        return pu_checked(ctx, pu_entries{alignments->d_row_offsets, cigars->d_op_offsets, cigars->d_ops, cigars->n_rows, cigars->n_regions, cigars->n_ops,
                                          on_q ? alignments->d_qstart : alignments->d_tstart, on_q ? alignments->d_tstart : alignments->d_qstart},
                          d_row_mask, hits, ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o, out);
    }, cigars, alignments);
}
extern "C" int ks_hitalns_pileup(ks_ctx *ctx, const ks_hitalns *stitched, const ks_hits *hits, const uint8_t *d_row_mask, const uint64_t *d_offsets,
                                 uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs,
                                 uint64_t n_o_res, const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res), out, pu_any, [&](const ks_pileup_opts &o) {
        const bool on_q = o.side == KS_PILEUP_QUERY;
        return pu_checked(ctx, pu_entries{nullptr, stitched->d_op_offsets, stitched->d_ops, stitched->n_rows, stitched->n_rows, stitched->n_ops,
                                          on_q ? stitched->d_q_start : stitched->d_t_start, on_q ? stitched->d_t_start : stitched->d_q_start},
                          d_row_mask, hits, ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o, out);
    }, stitched);
}
extern "C" int ks_wpileup_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops,
                                        uint64_t n_rows, uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start,
                                        const uint8_t *d_row_mask, const ks_hits *hits, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                                        const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                                        const uint32_t *d_weight, const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res) && (d_other_start || !n_entries), out, pu_any, [&](const ks_pileup_opts &o) {
        return pu_checked(ctx, pu_entries{d_row_offsets, d_op_offsets, d_ops, n_rows, n_entries, n_ops, d_start, d_other_start}, d_row_mask, hits,
                          ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o, out, true, d_weight);
    });
}
// the entries of a ks_cigars with the ks_raligns they were traced from, as ks_cigars_pileup and its two siblings read them
static int pu_cigars_entries(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, u32 side, pu_entries *E) {
    KS_TRY(ks_refuse_by_profile(ctx, "pileup", alignments));
    if (cigars->n_rows != alignments->n_rows || cigars->n_regions != alignments->n_regions)
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup: the cigars hold %llu regions in %llu hit rows, the alignments %llu in %llu: not traced from them",
                       (unsigned long long)cigars->n_regions, (unsigned long long)cigars->n_rows, (unsigned long long)alignments->n_regions,
                       (unsigned long long)alignments->n_rows);
    const bool on_q = side == KS_PILEUP_QUERY;
    *E = pu_entries{alignments->d_row_offsets, cigars->d_op_offsets, cigars->d_ops, cigars->n_rows, cigars->n_regions, cigars->n_ops,
                    on_q ? alignments->d_qstart : alignments->d_tstart, on_q ? alignments->d_tstart : alignments->d_qstart};
    return KS_OK;
}
extern "C" int ks_cigars_pileup_weighted(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_hits *hits,
                                         const uint8_t *d_row_mask, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res,
                                         const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res, const uint32_t *d_weight,
                                         const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res), out, pu_any, [&](const ks_pileup_opts &o) {
        pu_entries E;
        KS_TRY(pu_cigars_entries(ctx, cigars, alignments, o.side, &E));
        return pu_checked(ctx, E, d_row_mask, hits, ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o,
                          out, true, d_weight);
    }, cigars, alignments);
}
extern "C" int ks_hitalns_pileup_weighted(ks_ctx *ctx, const ks_hitalns *stitched, const ks_hits *hits, const uint8_t *d_row_mask,
                                          const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets,
                                          uint32_t n_o_seqs, uint64_t n_o_res, const uint32_t *d_weight, const ks_pileup_opts *opts, ks_pileup **out) {
    return pu_entry(ctx, opts, pu_has_batch(d_o_res, d_o_offsets, n_o_res), out, pu_any, [&](const ks_pileup_opts &o) {
        const bool on_q = o.side == KS_PILEUP_QUERY;
        return pu_checked(ctx, pu_entries{nullptr, stitched->d_op_offsets, stitched->d_ops, stitched->n_rows, stitched->n_rows, stitched->n_ops,
                                          on_q ? stitched->d_q_start : stitched->d_t_start, on_q ? stitched->d_t_start : stitched->d_q_start},
                          d_row_mask, hits, ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o, out,
                          true, d_weight);
    }, stitched);
}

// The weights pass reads the other side like a pileup with the profile: its options are that pileup's, made from `side`.
static const char *pw_refuse(u32 flags) { return (flags & ~KS_PWEIGHTS_INCLUDE_QUERY) ? "unknown flags of the weights (KS_PWEIGHTS_INCLUDE_QUERY is the one there is)" : nullptr; }
extern "C" int ks_entry_weights_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops,
                                        uint64_t n_rows, uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start,
                                        const uint8_t *d_row_mask, const ks_hits *hits, const uint8_t *d_res, const uint64_t *d_offsets, uint32_t n_seqs,
                                        uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                                        const uint32_t *d_counts, uint32_t side, uint32_t flags, ks_pweights **out) {
    const ks_pileup_opts po = {KS_PILEUP_PROFILE, side, 0ull};
    return pu_entry(ctx, &po, pu_has_batch(d_o_res, d_o_offsets, n_o_res) && (d_other_start || !n_entries), out,
                    [&](const ks_pileup_opts &) { return pw_refuse(flags); }, [&](const ks_pileup_opts &o) {
        return pw_checked(ctx, pu_entries{d_row_offsets, d_op_offsets, d_ops, n_rows, n_entries, n_ops, d_start, d_other_start}, d_row_mask, hits,
                          ks_res_batch{d_res, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res}, o.side, flags, d_counts, out);
    });
}
extern "C" int ks_cigars_pileup_weights(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_pileup *pileup,
                                        const ks_hits *hits, const uint8_t *d_row_mask, const uint8_t *d_res, const uint64_t *d_offsets, uint32_t n_seqs,
                                        uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                                        uint32_t side, uint32_t flags, ks_pweights **out) {
    const ks_pileup_opts po = {KS_PILEUP_PROFILE, side, 0ull};
    return pu_entry(ctx, &po, pu_has_batch(d_o_res, d_o_offsets, n_o_res), out, [&](const ks_pileup_opts &) { return pw_refuse(flags); },
                    [&](const ks_pileup_opts &o) {
        pu_entries E;
        KS_TRY(pu_cigars_entries(ctx, cigars, alignments, o.side, &E));
        if (pileup->n_profile != pileup->n_residues * PU_A)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup weights: the pileup was made without KS_PILEUP_PROFILE: it holds no counts");
        if (pileup->n_seqs != n_seqs || pileup->n_residues != n_res)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "pileup weights: the pileup is of %llu sequences and %llu residues, the side's batch of %u and %llu: a "
                                                    "pileup of another batch or of the other side",
                           (unsigned long long)pileup->n_seqs, (unsigned long long)pileup->n_residues, n_seqs, (unsigned long long)n_res);
        return pw_checked(ctx, E, d_row_mask, hits, ks_res_batch{d_res, d_offsets, n_seqs, n_res}, ks_res_batch{d_o_res, d_o_offsets, n_o_seqs, n_o_res},
                          o.side, flags, pileup->d_counts, out);
    }, cigars, alignments, pileup);
}
extern "C" int ks_frames_pileup(ks_ctx *ctx, const ks_framealns *frame_alignments, const ks_hits *fold_hits, const uint8_t *d_row_mask,
                                   const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const ks_pileup_opts *opts, ks_pileup **out) {
    const auto refuse = [](const ks_pileup_opts &o) -> const char * {
        if (o.flags & KS_PILEUP_PROFILE) return "frame alignments have no profile (KS_PILEUP_PROFILE): their query side is a strand's bases";
        if (o.side != KS_PILEUP_TARGET) return "frame alignments pile up on KS_PILEUP_TARGET only: depth in bases on a strand is not built";
        return nullptr;
    };
    // (the profile is refused by name, not for its missing batch)
    return pu_entry(ctx, opts, true, out, refuse, [&](const ks_pileup_opts &o) {
        const ks_framealns *F = frame_alignments;
        return pu_checked(ctx, pu_entries{nullptr, F->d_op_offsets, F->d_ops, F->n_rows, F->n_rows, F->n_ops, F->d_t_start, nullptr}, d_row_mask,
                          fold_hits, ks_res_batch{nullptr, d_offsets, n_seqs, n_res}, ks_res_batch{nullptr, nullptr, 0u, 0ull}, o, out);
    }, frame_alignments);
}

extern "C" uint32_t ks_pileup_n_seqs(const ks_pileup *p) { return p ? (u32)p->n_seqs : 0; }
extern "C" uint64_t ks_pileup_n_residues(const ks_pileup *p) { return p ? p->n_residues : 0; }
extern "C" uint64_t ks_pileup_n_profile(const ks_pileup *p) { return p ? p->n_profile : 0; }
extern "C" const uint32_t *ks_pileup_device_depth(const ks_pileup *p) { return p ? p->d_depth : nullptr; }
extern "C" const uint32_t *ks_pileup_device_counts(const ks_pileup *p) { return p ? p->d_counts : nullptr; }
extern "C" const uint32_t *ks_pileup_device_length(const ks_pileup *p) { return p ? p->d_length : nullptr; }
extern "C" const uint32_t *ks_pileup_device_n_alignments(const ks_pileup *p) { return p ? p->d_n_alignments : nullptr; }
extern "C" const uint32_t *ks_pileup_device_covered(const ks_pileup *p) { return p ? p->d_covered : nullptr; }
extern "C" const uint32_t *ks_pileup_device_max_depth(const ks_pileup *p) { return p ? p->d_max_depth : nullptr; }
extern "C" const uint64_t *ks_pileup_device_depth_sum(const ks_pileup *p) { return p ? p->d_depth_sum : nullptr; }
extern "C" const double *ks_pileup_device_breadth(const ks_pileup *p) { return p ? p->d_breadth : nullptr; }
extern "C" const double *ks_pileup_device_mean_depth(const ks_pileup *p) { return p ? p->d_mean_depth : nullptr; }
extern "C" int ks_pileup_copy_to_host(ks_ctx *ctx, const ks_pileup *p, uint32_t *depth, uint32_t *counts, uint32_t *length, uint32_t *n_alignments,
                                      uint32_t *covered, uint32_t *max_depth, uint64_t *depth_sum, double *breadth, double *mean_depth) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, p, depth, counts, length, n_alignments, covered, max_depth, depth_sum, breadth, mean_depth); });
}
extern "C" uint64_t ks_wpileup_n_weighted(const ks_pileup *p) { return p ? p->n_weighted : 0; }
extern "C" const uint64_t *ks_wpileup_device_wdepth(const ks_pileup *p) { return p ? p->d_wdepth : nullptr; }
extern "C" const uint64_t *ks_wpileup_device_wcounts(const ks_pileup *p) { return p ? p->d_wcounts : nullptr; }
extern "C" int ks_wpileup_copy_to_host(ks_ctx *ctx, const ks_pileup *p, uint64_t *wdepth, uint64_t *wcounts) {
    return ks_guard(ctx, [&]() -> int {
        if (!ctx || !p) return KS_ERR_INVALID_ARG;
        return ks_columns_to_host(ctx, {{wdepth, p->d_wdepth, (size_t)p->n_weighted * sizeof(u64)}, {wcounts, p->d_wcounts, (size_t)p->n_wprofile * sizeof(u64)}});
    });
}
extern "C" void ks_pileup_free(ks_pileup *p) { ks_obj_free(p); }
extern "C" uint64_t ks_pweights_n_entries(const ks_pweights *w) { return w ? w->n_entries : 0; }
extern "C" const uint32_t *ks_pweights_device_weight(const ks_pweights *w) { return w ? w->d_weight : nullptr; }
extern "C" const uint32_t *ks_pweights_device_n_cols(const ks_pweights *w) { return w ? w->d_n_cols : nullptr; }
extern "C" int ks_pweights_copy_to_host(ks_ctx *ctx, const ks_pweights *w, uint32_t *weight, uint32_t *n_cols) {
    return ks_guard(ctx, [&]() -> int { return ks_obj_to_host(ctx, w, weight, n_cols); });
}
extern "C" void ks_pweights_free(ks_pweights *w) { ks_obj_free(w); }
extern "C" void ks_debug_pileup_limits(uint32_t *wave_max) {
    if (wave_max) *wave_max = PU_WAVE_MAX;
}
