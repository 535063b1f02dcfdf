// ks_fstitch.hip — ks_frames_stitch: the chain of every folded row of a translated search (ks_ffold.hip, ks_rchain.hip) made into
// ONE alignment of the strand's bases against the target protein: one CIGAR in codon columns with explicit frameshift ops,
// re-scored over the residues (include/kmerseek_amd.h has the contract).  All of it in integers.
//
// A strand base position p reads the codon that is residue p / 3 of frame sequence 6 record + 3 strand + p % 3: the fold's
// s_start = f + 3 q_start, f < 3, makes one rule address every frame.  M, = and X are a codon against a residue, I a codon without
// a residue, D a residue without a codon, N (KS_CIGAR_FSHIFT) r = 1 or 2 skipped bases.  The worked examples, a gene of n codons
// whose two parts are aligned in two frames:
//   one base inserted after codon m     X = 1, Y = 0          mM 1N (n - m)M
//   one base of codon m deleted         X = 2, Y = 1, c = 0   mM 1D 2N (n - m - 1)M
// The pass does not search for the place of the shift inside a link: the N op stands directly before the next member.
//
//   plan     k_fs_plan, a thread per chain member, as k_rs_plan: everything is checked before it is indexed — the member lies in
//            its folded row's regions, the fold's region names an alignment, the fold's columns are those of that alignment, the
//            frame is of the row's strand and inside the frame batch, the extents lie inside the sequences, the ops consume them
//            and carry the right pair codes, the ends do not lie before those of the member before it.  The same walk finds the
//            trim in bases (a query-consuming column moves the strand position by 3), then the link: X bases = 3 c + r, Y
//            residues, the class of the rectangle (c, Y) and the rows and columns a fill needs.  Two scans, one wait.
//   fill     k_fs_fill, a wave per filled link: rf_fill of ks_rfill_kit.h — the program of ks_rstitch.hip, not a copy — with the
//            query stretch taken from the PREVIOUS member's frame sequence directly after its end.
//   emit     k_fs_emit<false / true>, a thread per folded row: member ops from the first kept one, link runs or the link's
//            columns, and the N op, through one run merger that never merges N; a scan whose output IS op_offsets.
//   rescore  k_fs_rescore, a wave per folded row: the final ops replayed; each lane's column computes its own strand position
//            and from it the frame sequence and the residue; an N op moves the position by its length.
// No atomics but the first-offender words; the result does not depend on the launch geometry, the slices or the stage.
#include "ks_rfill_kit.h"

#define FS_THREADS 256
#define FS_N KS_CIGAR_FSHIFT
enum : u32 { FS_BAD_SRC = 0, FS_BAD_FSRC = 1, FS_BAD_FOLD = 2, FS_BAD_STRAND = 3, FS_BAD_ROW = 4, FS_BAD_LEN = 5, FS_BAD_EXT = 6, FS_BAD_OPS = 7,
              FS_BAD_CODE = 8, FS_BAD_ASC = 9, FS_BAD_WALK = 10, FS_N_BAD = 11 };
enum : u32 { FS_L_NONE = 0, FS_L_I = 1, FS_L_D = 2, FS_L_FILL = 3, FS_L_FILL_SWAP = 4, FS_L_OPEN = 5 };

// per chain member: its alignment, its trim and the link in front of it
struct fs_link {
    u32 g;         // the member's region in the alignments and the CIGARs
    u32 trim;      // leading columns removed
    u32 kop, krem; // the first op that is kept (inside the member's ops) and what is left of it
    u32 c, r, Y;   // the link: codons, skipped bases (X = 3 c + r) and target residues
    u32 cls;       // FS_L_* of the rectangle (c, Y)
    u32 ncol;      // filled: the columns of the path (k_fs_fill)
    u32 E, pte;    // the previous member's ends: strand bases, target residues
    u32 pad;
};

struct fs_args {
    const u64 *c_offs; const u32 *c_src;                                     // the chain: n_rows + 1, n_chained
    const u64 *f_offs; const u32 *f_src; const u8 *f_frame;                  // the fold: n_rows + 1, n_fregions
    const u32 *f_ntlen, *f_sstart, *f_ntstart, *f_ts3, *f_tl3;
    const u32 *a_qs, *a_ql, *a_ts, *a_tl;                                    // the alignments
    const u64 *g_offs; const u32 *g_ops;                                     // their CIGARs
    const u32 *qid, *tid;                                                    // the folded hits
    const u8 *q_res, *t_res;                                                 // the frame batch, the target batch
    const u64 *q_offs, *t_offs;
    const signed char *matrix;
    u64 n_q_res, n_t_res, n_gops;
    u32 n_rows, n_chained, n_fregions, n_regions, n_q, n_t;
    u32 o, e, max_fill, eqx, fcost;
    unsigned long long *bad;
};

KS_DEV bool fs_is_pair(u32 c) { return c == RP_M || c == RP_EQ || c == RP_X; }
KS_DEV u32 fs_even(u32 v) { return (v + 1u) & ~1u; }
KS_DEV double fs_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__global__ __launch_bounds__(FS_THREADS) void k_fs_plan(fs_args A, fs_link *links, u32 *rows, u32 *ncols) {
    const u64 j64 = (u64)blockIdx.x * FS_THREADS + threadIdx.x;
    if (j64 >= A.n_chained) return;
    const u32 j = (u32)j64;
    fs_link L{0u, 0u, 0u, 0u, 0u, 0u, 0u, FS_L_NONE, 0u, 0u, 0u, 0u};
    u32 nr = 0, nc = 0;
    [&]() {
        const u32 row = ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j); // (c_offs[0] == 0 <= j)
        const bool first = A.c_offs[row] == j;
        const u32 fg = A.c_src[j];
        if (fg >= A.n_fregions || fg < A.f_offs[row] || fg >= A.f_offs[row + 1]) { ks_first_bad(A.bad, FS_BAD_SRC, j); return; }
        const u32 g = A.f_src[fg];
        if (g >= A.n_regions) { ks_first_bad(A.bad, FS_BAD_FSRC, fg); return; }
        L.g = g;
        const u32 q = A.qid[row], t = A.tid[row], frame = A.f_frame[fg];
        if (frame >= 6u || frame / 3u != (q & 1u)) { ks_first_bad(A.bad, FS_BAD_STRAND, fg); return; }
        const u64 qs = A.a_qs[g], ql = A.a_ql[g], ts = A.a_ts[g], tl = A.a_tl[g];
        if ((u64)A.f_sstart[fg] != frame % 3u + 3u * qs || (u64)A.f_ntlen[fg] != 3u * ql || (u64)A.f_ts3[fg] != 3u * ts || (u64)A.f_tl3[fg] != 3u * tl) {
            ks_first_bad(A.bad, FS_BAD_FOLD, fg);
            return;
        }
        const u64 s6 = 6ULL * (q >> 1) + 3u * (q & 1u), fseq = s6 + frame % 3u;
        if (s6 + 3u > A.n_q || t >= A.n_t) { ks_first_bad(A.bad, FS_BAD_ROW, row); return; } // (all three frames of the strand exist)
        const rk_seqs S = rk_row_seqs<false>(A, (u32)fseq, t);
        if (!S.ok) { ks_first_bad(A.bad, FS_BAD_ROW, row); return; }
        if (S.Lq > RA_MAX_LEN || S.Lt > RA_MAX_LEN) { ks_first_bad(A.bad, FS_BAD_LEN, row); return; }
        if (ql == 0 || tl == 0 || qs + ql > S.Lq || ts + tl > S.Lt) { ks_first_bad(A.bad, FS_BAD_EXT, g); return; }
        const u64 s_start = frame % 3u + 3u * qs, s_end = s_start + 3u * ql; // (<= 3 * 2^20 + 2)
        u64 E = 0, pte = 0, Lqp = 0;
        if (!first) {
            const u32 fgp = A.c_src[j - 1];
            if (fgp >= A.n_fregions || fgp < A.f_offs[row] || fgp >= A.f_offs[row + 1]) return; // (its own thread names it, as below)
            const u32 gp = A.f_src[fgp], framep = A.f_frame[fgp];
            if (gp >= A.n_regions || framep >= 6u || framep / 3u != (q & 1u)) return;
            E = framep % 3u + 3u * ((u64)A.a_qs[gp] + A.a_ql[gp]); pte = (u64)A.a_ts[gp] + A.a_tl[gp];
            const rk_seqs P = rk_row_seqs<false>(A, (u32)(s6 + framep % 3u), t);
            if (!P.ok || P.Lq > RA_MAX_LEN) return;
            Lqp = P.Lq;
            if (E / 3u > Lqp) return;
            if (s_end < E || ts + tl < pte) { ks_first_bad(A.bad, FS_BAD_ASC, j); return; }
        }
        const u64 ob = A.g_offs[g], oe = A.g_offs[g + 1];
        if (ob > oe || oe > A.n_gops) { ks_first_bad(A.bad, FS_BAD_OPS, g); return; }
        const u32 nops = (u32)(oe - ob < 0xffffffffULL ? oe - ob : 0xffffffffULL);
        // one walk: what the ops consume, their codes, and the trim in bases
        u64 cq = 0, ct = 0, spos = s_start, tpos = ts;
        bool done = first, bad_code = false, bad_op = false;
        if (first) { L.kop = 0; L.krem = nops ? A.g_ops[ob] >> 4 : 0u; }
        for (u32 k = 0; k < nops; k++) {
            const u32 op = A.g_ops[ob + k], len = op >> 4, code = op & 15u;
            const bool pair = fs_is_pair(code);
            if (!pair && code != RP_I && code != RP_D) bad_op = true;
            if (pair && (A.eqx ? code == RP_M : code != RP_M)) bad_code = true;
            const u64 dq = pair || code == RP_I ? 1u : 0u, dt = pair || code == RP_D ? 1u : 0u;
            cq += len * dq; ct += len * dt;
            if (done) continue;
            const u64 needq = spos >= E ? 0 : (E - spos + 2u) / 3u, needt = tpos >= pte ? 0 : pte - tpos; // columns
            const u64 n = needq > needt ? needq : needt;
            if ((needq == 0 || dq) && (needt == 0 || dt) && n <= len) {
                done = true;
                L.kop = k; L.krem = len - (u32)n; L.trim += (u32)n;
                spos += 3u * n * dq; tpos += n * dt;
            } else { L.trim += len; spos += 3u * len * dq; tpos += len * dt; }
        }
        if (bad_op || cq != ql || ct != tl) { ks_first_bad(A.bad, FS_BAD_OPS, g); return; }
        if (bad_code) { ks_first_bad(A.bad, FS_BAD_CODE, g); return; }
        if (!done) { L.kop = nops; L.krem = 0; } // (no column is left: the position is the member's end)
        if (first) return;
        // (ends that do not descend and ops that consume the extents: spos >= E and tpos >= pte hold)
        const u64 X = spos - E, Y = tpos - pte, c = X / 3u;
        L.c = (u32)c; L.r = (u32)(X % 3u); L.Y = (u32)Y; L.E = (u32)E; L.pte = (u32)pte;
        if (E / 3u + c > Lqp) { ks_first_bad(A.bad, FS_BAD_EXT, g); return; } // (the link's codons lie inside the previous member's frame)
        const u64 lo = c < Y ? c : Y, hi = c < Y ? Y : c;
        if (hi == 0) L.cls = FS_L_NONE;
        else if (Y == 0) L.cls = FS_L_I;
        else if (c == 0) L.cls = FS_L_D;
        else if (lo <= RF_SHORT_MAX && hi <= A.max_fill) {
            L.cls = c < Y ? FS_L_FILL_SWAP : FS_L_FILL;
            nr = fs_even((u32)hi); nc = (u32)(c + Y);
        } else L.cls = FS_L_OPEN;
    }();
    links[j] = L; rows[j] = nr; ncols[j] = nc;
}

struct fs_slice {
    const u64 *dir_off, *col_off; // n_chained + 1: rows of directions / columns before member j
    u8 *dir, *cols;
    u64 dir_base;                 // dir_off[j0]
    u32 j0, j1;
};

__global__ __launch_bounds__(FS_THREADS) void k_fs_fill(fs_args A, fs_link *links, fs_slice Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    __shared__ uint4 s_stage[FS_THREADS / 64][RP_STAGE * RA_DIR_ROW / 16];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 j64 = (u64)Z.j0 + (u64)blockIdx.x * (FS_THREADS / 64) + wave;
    if (j64 >= Z.j1) return;
    const u32 j = (u32)j64;
    const u32 cls = ks_readfirst(links[j].cls);
    if (cls != FS_L_FILL && cls != FS_L_FILL_SWAP) return;
    // (behind the plan's wait: the member, the one before it and their row have passed every check)
    const u32 c = ks_readfirst(links[j].c), Y = ks_readfirst(links[j].Y), E = ks_readfirst(links[j].E), pte = ks_readfirst(links[j].pte);
    const u32 row = ks_readfirst(ks_last_le_u64(A.c_offs, 0, A.n_rows - 1, j));
    const u32 q = ks_readfirst(A.qid[row]), t = ks_readfirst(A.tid[row]);
    const u32 fseq = 6u * (q >> 1) + 3u * (q & 1u) + E % 3u; // the previous member's frame
    const u8 *const qst = A.q_res + rk_readfirst64(A.q_offs[fseq]) + E / 3u, *const tst = A.t_res + rk_readfirst64(A.t_offs[t]) + pte;
    u8 *const dir = Z.dir + (rk_readfirst64(Z.dir_off[j]) - Z.dir_base) * RA_DIR_ROW;
    u8 *const col = Z.cols + rk_readfirst64(Z.col_off[j]);
    rf_fill(rf_rect_of(c, Y, cls == FS_L_FILL_SWAP), qst, tst, A.o, A.e, A.eqx, dir, col, c + Y, s_cls, s_M, s_stage[wave], lane, [=](u32 n) {
        if (n == RP_BAD) {
            if (lane == 0) { ks_first_bad(A.bad, FS_BAD_WALK, j); links[j].ncol = 0; }
        } else if (lane == 0) links[j].ncol = n;
    });
}

struct fs_out {
    const u64 *col_off;
    const u8 *cols;
    u32 *n_ops;        // !WRITE: the ops of row r
    const u64 *op_off; // WRITE: their exclusive scan, and the ops
    u32 *ops;
    u32 *s_start, *nt_length, *nt_start, *t_start, *t_length, *n_members, *n_filled, *n_open, *n_trimmed, *n_frameshifts;
};

template <bool WRITE> __global__ __launch_bounds__(FS_THREADS) void k_fs_emit(fs_args A, const fs_link *links, fs_out Z) {
    const u64 r64 = (u64)blockIdx.x * FS_THREADS + threadIdx.x;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    const u64 b = A.c_offs[r], e = A.c_offs[r + 1];
    u64 o = 0, room = 0;
    if (WRITE) { o = Z.op_off[r]; room = Z.op_off[r + 1] - o; }
    u32 cur = 0xffu, len = 0, n = 0;
    auto flush = [&]() {
        if (cur == 0xffu) return;
        if (WRITE && n < room) Z.ops[o + n] = (len << 4) | cur;
        n++;
        cur = 0xffu;
    };
    auto push = [&](u32 code, u32 cnt) {
        if (cnt == 0) return;
        if (code == cur) { len += cnt; return; } // (a joint merges)
        flush();
        cur = code; len = cnt;
    };
    u32 n_filled = 0, n_open = 0, n_trim = 0, n_shift = 0;
    for (u64 j = b; j < e; j++) {
        const fs_link L = links[j];
        n_trim += L.trim;
        if (j > b) {
            if (L.cls == FS_L_I) push(RP_I, L.c);
            else if (L.cls == FS_L_D) push(RP_D, L.Y);
            else if (L.cls == FS_L_OPEN) { push(RP_I, L.c); push(RP_D, L.Y); n_open++; }
            else if (L.cls == FS_L_FILL || L.cls == FS_L_FILL_SWAP) {
                const u8 *path = Z.cols + Z.col_off[j] + (L.c + L.Y - L.ncol);
                for (u32 k = 0; k < L.ncol; k++) push(path[k], 1u);
                n_filled++;
            }
            if (L.r) { // the frameshift: an op of its own, merged with nothing
                flush();
                if (WRITE && n < room) Z.ops[o + n] = (L.r << 4) | FS_N;
                n++; n_shift++;
            }
        }
        const u64 ob = A.g_offs[L.g];
        const u32 nops = (u32)(A.g_offs[L.g + 1] - ob);
        for (u32 k = L.kop; k < nops; k++) {
            const u32 op = A.g_ops[ob + k];
            push(op & 15u, k == L.kop ? L.krem : op >> 4);
        }
    }
    flush();
    if (WRITE) return;
    Z.n_ops[r] = n;
    u32 ss = 0, se = 0, ns = 0, ts = 0, te = 0;
    if (e > b) {
        const u32 f0 = A.c_src[b], f1 = A.c_src[e - 1];
        ss = A.f_sstart[f0]; se = A.f_sstart[f1] + A.f_ntlen[f1];
        ns = (A.qid[r] & 1u) ? A.f_ntstart[f1] : A.f_ntstart[f0];
        const u32 g0 = links[b].g, g1 = links[e - 1].g;
        ts = A.a_ts[g0]; te = A.a_ts[g1] + A.a_tl[g1];
    }
    Z.s_start[r] = ss; Z.nt_length[r] = se - ss; Z.nt_start[r] = ns; Z.t_start[r] = ts; Z.t_length[r] = te - ts;
    Z.n_members[r] = (u32)(e - b); Z.n_filled[r] = n_filled; Z.n_open[r] = n_open; Z.n_trimmed[r] = n_trim; Z.n_frameshifts[r] = n_shift;
}

struct fs_cols {
    const u64 *op_off;
    const u32 *ops, *s_start, *t_start;
    i64 *score;
    u32 *identities, *positives, *gap_opens, *gaps, *aln_length;
    double *row_score;
};

KS_DEV u32 fs_wave_sum(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (u32)__shfl_xor((int)v, d);
    return v;
}

__global__ __launch_bounds__(FS_THREADS) void k_fs_rescore(fs_args A, fs_cols Z) {
    __shared__ u8 s_cls[256];
    __shared__ signed char s_M[RK_A * RK_A];
    rk_stage_tables(A.matrix, s_cls, s_M);
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = ks_readfirst(threadIdx.x >> 6);
    const u64 r64 = (u64)blockIdx.x * (FS_THREADS / 64) + wave;
    if (r64 >= A.n_rows) return;
    const u32 r = (u32)r64;
    const u64 ob = rk_readfirst64(Z.op_off[r]), oe = rk_readfirst64(Z.op_off[r + 1]);
    const bool empty = rk_readfirst64(A.c_offs[r]) == rk_readfirst64(A.c_offs[r + 1]);
    int sc = 0; // (at most 2^21 columns of |M| <= 128 over the lanes: 32 bits)
    u32 id = 0, po = 0, opens = 0, gaps = 0, alen = 0;
    i64 cost = 0;
    if (!empty) {
        // (a row with members has passed the plan: every pair of its ops lies inside a frame of the strand and inside the target)
        const u32 q = ks_readfirst(A.qid[r]), t = ks_readfirst(A.tid[r]);
        const u32 s6 = 6u * (q >> 1) + 3u * (q & 1u);
        const u8 *const f0 = A.q_res + rk_readfirst64(A.q_offs[s6]), *const f1 = A.q_res + rk_readfirst64(A.q_offs[s6 + 1]),
                 *const f2 = A.q_res + rk_readfirst64(A.q_offs[s6 + 2]);
        u32 p0 = ks_readfirst(Z.s_start[r]); // the strand position of the next column
        const u8 *tp = A.t_res + rk_readfirst64(A.t_offs[t]) + ks_readfirst(Z.t_start[r]);
        for (u64 k = ob; k < oe; k++) {
            const u32 op = ks_readfirst(Z.ops[k]), len = op >> 4, code = op & 15u;
            if (code == FS_N) { p0 += len; cost += (i64)A.fcost; continue; }
            alen += len;
            if (fs_is_pair(code)) {
                for (u32 c = lane; c < len; c += 64) {
                    const u32 p = p0 + 3u * c, f = p % 3u; // this column's codon: residue p / 3 of frame p % 3
                    const u32 a = (f == 0 ? f0 : f == 1 ? f1 : f2)[p / 3u], b = tp[c];
                    const int s = s_M[s_cls[a] * RK_A + s_cls[b]];
                    sc += s; id += rk_upper(a) == rk_upper(b) ? 1u : 0u; po += s > 0 ? 1u : 0u;
                }
                p0 += 3u * len; tp += len;
            } else {
                opens++; gaps += len; cost += (i64)A.o + (i64)len * A.e;
                if (code == RP_I) p0 += 3u * len; else tp += len;
            }
        }
    }
    const i64 total = (i64)(int)fs_wave_sum((u32)sc) - cost;
    id = fs_wave_sum(id); po = fs_wave_sum(po);
    if (lane == 0) {
        Z.score[r] = total; Z.identities[r] = id; Z.positives[r] = po; Z.gap_opens[r] = opens; Z.gaps[r] = gaps; Z.aln_length[r] = alen;
        Z.row_score[r] = empty ? fs_nan() : (double)total;
    }
}

int ks_frames_stitch_impl(ks_ctx *ctx, const ks_ffold *F, const ks_hits *H, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G,
                          const ks_res_batch &Q, const ks_res_batch &T, u32 max_fill, u32 flags, u32 frameshift_cost, u64 max_scratch_bytes,
                          ks_framealns *R) {
    const u64 n_rows = K->n_rows, nm = K->n_chained;
    R->n_rows = n_rows; R->n_ops = 0; R->dir_bytes = 0; R->n_slices = 0;
    KS_TRY(ks_alloc(ctx, &R->d_op_offsets, (size_t)n_rows + 1));
    KS_TRY(ks_obj_alloc(ctx, R, R->n_rows));
    if (n_rows == 0) {
        KS_HIP(ctx, hipMemsetAsync(R->d_op_offsets, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    KS_TRY(rk_counts_check(ctx, "frame stitch", n_rows, S->n_regions));

    ks_scratch sc(ctx);
    signed char *d_M = nullptr;
    ks_ctl ctl;
    fs_link *links = nullptr;
    u32 *rows = nullptr, *ncols = nullptr, *row_ops = nullptr;
    u64 *dir_off = nullptr, *col_off = nullptr;
    KS_TRY(rk_upload_matrix(ctx, sc, S->matrix, &d_M));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_FSTITCH, FS_N_BAD, 0));
    KS_TRY(sc.alloc(&links, (size_t)nm)); KS_TRY(sc.alloc(&rows, (size_t)nm)); KS_TRY(sc.alloc(&ncols, (size_t)nm));
    KS_TRY(sc.alloc(&dir_off, (size_t)nm + 1)); KS_TRY(sc.alloc(&col_off, (size_t)nm + 1));
    KS_TRY(sc.alloc(&row_ops, (size_t)n_rows));

    fs_args A;
    A.c_offs = K->d_row_offsets; A.c_src = K->d_src_region;
    A.f_offs = F->d_row_offsets; A.f_src = F->d_src_region; A.f_frame = F->d_frame;
    A.f_ntlen = F->d_nt_length; A.f_sstart = F->d_s_start; A.f_ntstart = F->d_nt_start; A.f_ts3 = F->d_t_start3; A.f_tl3 = F->d_t_length3;
    A.a_qs = S->d_qstart; A.a_ql = S->d_qlength; A.a_ts = S->d_tstart; A.a_tl = S->d_tlength;
    A.g_offs = G->d_op_offsets; A.g_ops = G->d_ops;
    A.qid = H->d_qid; A.tid = H->d_tid;
    A.q_res = Q.res; A.t_res = T.res; A.q_offs = Q.offs; A.t_offs = T.offs;
    A.matrix = d_M;
    A.n_q_res = Q.n_res; A.n_t_res = T.n_res; A.n_gops = G->n_ops;
    A.n_rows = (u32)n_rows; A.n_chained = (u32)nm; A.n_fregions = (u32)F->n_regions; A.n_regions = (u32)S->n_regions; A.n_q = Q.n_seqs; A.n_t = T.n_seqs;
    A.o = S->gap_open; A.e = S->gap_extend; A.max_fill = max_fill; A.eqx = (flags & KS_RSTITCH_EQX) ? 1u : 0u; A.fcost = frameshift_cost;
    A.bad = ctl.words();

    u64 *const rb = ctx->h_pin + KS_PIN_FSTITCH + FS_N_BAD; // direction rows | columns | ops
    rb[0] = rb[1] = rb[2] = 0;
    u8 *dir = nullptr, *cols = nullptr;
    if (nm) {
        KS_LAUNCH(ctx, "fstitch_plan", k_fs_plan, (u32)((nm + FS_THREADS - 1) / FS_THREADS), FS_THREADS, A, links, rows, ncols);
        KS_TRY(ks_scan_u32_to_u64_wide(ctx, rows, dir_off, nm)); // (the directions are made in slices: no allocation bounds their sum)
        KS_TRY(ks_scan_u32_to_u64(ctx, ncols, col_off, nm));
        KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(dir_off + nm, rb, 2), ks_fetch_words(col_off + nm, rb + 1, 2)}));
        if (ctl.bad(FS_BAD_SRC))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: chain member %llu names a region outside its folded row's regions: the chain was not made on this fold",
                           (unsigned long long)ctl[FS_BAD_SRC]);
        if (ctl.bad(FS_BAD_FSRC))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu names an alignment beyond the %llu of the alignments: the fold was not made of these alignments",
                           (unsigned long long)ctl[FS_BAD_FSRC], (unsigned long long)S->n_regions);
        if (ctl.bad(FS_BAD_FOLD))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu does not hold its alignment's extents (s_start = frame %% 3 + 3 q_start, nt_length = 3 q_length, t_start3 = 3 t_start, t_length3 = 3 t_length): the fold was not made of these alignments",
                           (unsigned long long)ctl[FS_BAD_FOLD]);
        if (ctl.bad(FS_BAD_STRAND))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu lies in a frame of the other strand than its folded row's: fold and folded hits do not belong together",
                           (unsigned long long)ctl[FS_BAD_STRAND]);
        if (ctl.bad(FS_BAD_ROW))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded row %llu names a frame sequence beyond the %u of the frame batch, a target beyond the %u of the target batch, or a sequence outside its batch",
                           (unsigned long long)ctl[FS_BAD_ROW], Q.n_seqs, T.n_seqs);
        if (ctl.bad(FS_BAD_LEN))
            return ks_fail(ctx, KS_ERR_CAPACITY, "frame stitch: folded row %llu has a frame or target sequence of more than 2^20 residues",
                           (unsigned long long)ctl[FS_BAD_LEN]);
        if (ctl.bad(FS_BAD_EXT))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: the alignment of region %llu does not lie inside its two sequences: alignments, hits and batches do not belong together",
                           (unsigned long long)ctl[FS_BAD_EXT]);
        if (ctl.bad(FS_BAD_OPS))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: the ops of region %llu do not consume exactly its q_length and t_length: the CIGARs were not traced from these alignments",
                           (unsigned long long)ctl[FS_BAD_OPS]);
        if (ctl.bad(FS_BAD_CODE))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, A.eqx ? "frame stitch: KS_RSTITCH_EQX is set and the ops of region %llu hold M: trace with KS_RTRACE_EQX"
                                                          : "frame stitch: the ops of region %llu hold = or X: set KS_RSTITCH_EQX",
                           (unsigned long long)ctl[FS_BAD_CODE]);
        if (ctl.bad(FS_BAD_ASC))
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: chain member %llu ends before the member in front of it on the strand or on the target: the chain was not made on this fold",
                           (unsigned long long)ctl[FS_BAD_ASC]);
        const u64 total_rows = rb[0], total_cols = rb[1];

        // slices of consecutive members whose directions fit the budget
        const u64 budget_rows = (max_scratch_bytes ? max_scratch_bytes : (u64)1 << 30) / RA_DIR_ROW;
        rp_slices Sl;
        KS_TRY(rp_slices_of(ctx, dir_off, nm, total_rows, budget_rows, &Sl));
        if (Sl.bad < nm)
            return ks_fail(ctx, KS_ERR_CAPACITY, "frame stitch: the link in front of chain member %llu needs %llu bytes of directions, max_scratch_bytes allows %llu",
                           (unsigned long long)Sl.bad, (unsigned long long)(Sl.bad_rows * RA_DIR_ROW), (unsigned long long)(budget_rows * RA_DIR_ROW));
        const std::vector<u64> &cut = Sl.cut, &first_row = Sl.first_row;
        const u64 slice_rows = Sl.max_rows;
        KS_TRY(sc.alloc(&dir, (size_t)(slice_rows * RA_DIR_ROW)));
        KS_TRY(sc.alloc(&cols, (size_t)total_cols));
        R->dir_bytes = slice_rows * RA_DIR_ROW; R->n_slices = (u32)(cut.size() - 1);
        if (total_rows)
            for (size_t i = 0; i + 1 < cut.size(); i++) { // (one block for all slices: the launches are ordered by the stream)
                const fs_slice Z{dir_off, col_off, dir, cols, first_row[i], (u32)cut[i], (u32)cut[i + 1]};
                KS_LAUNCH(ctx, "fstitch_fill", k_fs_fill, (u32)((cut[i + 1] - cut[i] + FS_THREADS / 64 - 1) / (FS_THREADS / 64)), FS_THREADS, A, links, Z);
            }
    }

    // the ops per row, their scan = op_offsets, the ops, the columns
    const u32 grid = (u32)((n_rows + FS_THREADS - 1) / FS_THREADS);
    fs_out E{col_off, cols, row_ops, R->d_op_offsets, nullptr, R->d_s_start, R->d_nt_length, R->d_nt_start, R->d_t_start, R->d_t_length,
             R->d_n_members, R->d_n_filled, R->d_n_open, R->d_n_trimmed, R->d_n_frameshifts};
    KS_LAUNCH(ctx, "fstitch_count", k_fs_emit<false>, grid, FS_THREADS, A, (const fs_link *)links, E);
    KS_TRY(ks_scan_u32_to_u64(ctx, row_ops, R->d_op_offsets, n_rows));
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(R->d_op_offsets + n_rows, rb + 2, 2)}));
    if (ctl.bad(FS_BAD_WALK))
        return ks_fail(ctx, KS_ERR_HIP, "frame stitch: internal error: the fill in front of chain member %llu did not walk back to its origin",
                       (unsigned long long)ctl[FS_BAD_WALK]);
    R->n_ops = rb[2];
    KS_TRY(ks_alloc(ctx, &R->d_ops, (size_t)R->n_ops));
    E.ops = R->d_ops;
    KS_LAUNCH(ctx, "fstitch_ops", k_fs_emit<true>, grid, FS_THREADS, A, (const fs_link *)links, E);
    const fs_cols C{R->d_op_offsets, R->d_ops, R->d_s_start, R->d_t_start, R->d_score, R->d_identities, R->d_positives, R->d_gap_opens,
                    R->d_gaps, R->d_aln_length, R->d_row_score};
    KS_LAUNCH(ctx, "fstitch_rescore", k_fs_rescore, (u32)((n_rows + FS_THREADS / 64 - 1) / (FS_THREADS / 64)), FS_THREADS, A, C);
    return ks_stream_wait(ctx);
}
