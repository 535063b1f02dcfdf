// ks_ralign_kit.h — the one extension of the banded affine-gap program (include/kmerseek_amd.h: region alignments) that
// ks_ralign.hip and ks_rtrace.hip share: a wave per region, lanes as diagonals.  Two instantiations of one row step, so the
// pass that reports an alignment and the pass that walks it back can never disagree on a tie.  The E step of that row step
// (ra_e_step) and the direction byte are also what the fill of ks_rstitch.hip, lanes as columns, takes and writes.
//   TR = false  ks_regions_align: every state carries the four counts of its path, the rows run to the X-drop rule's J and
//               the best cell comes back.
//   TR = true   ks_regions_traceback: the end cell is known (x_end <= J, y_end), so there is no X-drop rule, no best cell
//               and no counts — the selects and moves that carry them are not instantiated — and every row writes one
//               direction byte per lane (RA_DIR_*).
//
//   lanes      lane k is diagonal k - W of the band (W <= 31: 2W + 1 <= 63 lanes; the others hold the sentinel and only idle
//              along).  A step is one row x of the program: lane k holds the cell (x, y = x + k - W).
//   state      H and F of the previous row stay in registers, each with the four counts of the path that made it.
//              D reads the lane's own H (the same diagonal).  F reads the lane above: every lane first forms what it hands
//              down, G = max(H - o - e, F - e), and G with its counts moves one lane by DPP (wave_shl:1).
//              E of a row is one inclusive max scan (DPP, ks_wave_incl_max) of H~ + k * e, moved one lane up.  Only when some
//              lane takes its E are the source lane — the last lane below that attains the running maximum, from one ballot:
//              among equal values the largest lane, the tie rule of the contract — and its counts (ds_bpermute) fetched.
//   residues   RA_CHUNK rows at a time: lane i loads the query byte of row i of the chunk (the row's byte is then a readlane:
//              wave-uniform), and the chunk's target window — RA_CHUNK + 2W bytes — goes upper-cased and classified into the
//              wave's own LDS strip; a row reads strip[r + k].  No global load depends on a row.  The left side is the same
//              function with descending addresses.
//   scorer     what a pair scores is a policy (SC), as in ks_rkit.h: ra_by_matrix reads the matrix row of the row's query byte
//              in LDS.  ra_by_profile stages the chunk's RA_CHUNK rows of the profile — 64 x 28 bytes, 7 words a row, a row of
//              the program after the other, descending batch positions on the left side — into the wave's own LDS rows beside
//              the target window, and a cell reads rows[r][class(T_y)]: again no global load depends on a row.
//   result     every lane keeps its best cell, replaced by strictly larger values only (its smallest x); one 64-bit wave
//              maximum of (H, -x, -lane) at the end picks the largest H, then the smallest x, then the smallest y.  The row
//              maximum for the X-drop rule is one DPP max scan per row; the exit is wave-uniform.
//
// 32 bits are enough, and the sentinel is safe.  Sequences are at most RA_MAX_LEN = 2^20 residues (longer ones are refused),
// |M| <= 128, o, e <= 255, W <= 31.  Every existing cell (x, y) is reached by min(x, y) diagonal steps and one gap of at most W
// residues inside the band, so H >= -(2^20 * 128 + 255 + 31 * 255) > -2^27 - 2^14, and H <= 2^20 * 127 < 2^27.  RA_NEG = -2^30
// stands for "no such cell / state".  It is never carried along: a lane whose cell does not exist is SET to RA_NEG in every
// row, so what is derived from it in one row is at least RA_NEG - 128 - 2 * 255 - 62 * 255 > -2^31 (no wrap) and at most
// RA_NEG + 127 + 62 * 255 < -2^27 - 2^14 (below every real value: it never wins a maximum against one, and every existing
// cell of a row x >= 1 has a real D or a real F).  B - R < 2^28 + 2^14, x_drop <= 2^20: the X-drop test is an i32 compare.
// Counts: at most 2^21 + 31 steps on a path.
#pragma once
#include "ks_rkit.h"

#define RA_THREADS 256
#define RA_CHUNK 64           // rows whose residues are staged at once (ks_debug_ralign_chunk)
#define RA_WMAX 31
#define RA_STRIP (RA_CHUNK + 64) // >= RA_CHUNK + 2 * RA_WMAX, two entries per lane
#define RA_NEG (-(1 << 30))
#define RA_MAX_LEN (1u << 20)
static_assert(RA_CHUNK <= 64 && RA_CHUNK + 2 * RA_WMAX <= RA_STRIP && RA_STRIP == 128, "a chunk is a lane per row, its window two entries per lane");

// The direction byte of the cell (x, lane k), x >= 1, RA_DIR_ROW bytes per row.  One byte, two lane geometries (the walk that
// reads it is rp_walk of ks_rpath_kit.h):
//   RA_DIR_DIAG   H~(x, y) took D (else F)
//   RA_DIR_CONT   a gap F continued F of the row before (else it opened one from H of the row before).  Whose gap:
//                   lanes as diagonals (ra_extend<true>)  the G this lane HANDED DOWN in row x: it is the F of the cell one lane
//                                                         below, (x, lane k - 1).  A walk in state F at (x, lane j) reads this
//                                                         bit of lane j + 1 and goes to (x - 1, lane j + 1)
//                   lanes as columns (rf_fill)            the F of the lane's OWN cell.  A walk in state F at (x, lane j) reads
//                                                         this bit of lane j and goes to (x - 1, lane j)
//   >> RA_DIR_E   0: H(x, y) is H~; d >= 1: H took E from the H~ of lane k - d of the same row (d <= 63: 6 bits)
// The byte of a lane whose cell does not exist means nothing; a walk from an existing cell never reaches one.
#define RA_DIR_DIAG 1u
#define RA_DIR_CONT 2u
#define RA_DIR_E 2
#define RA_DIR_ROW 64u // bytes of a row of directions

struct ra_cnt { u32 id, po, go, ga; }; // identities, positives, gap opens, gap residues of the path into a state
struct ra_ext { u32 x, y; int score; ra_cnt c; };

// the value of the lane above (lane 63: `none`)
KS_DEV u32 ra_lane_above(u32 v, u32 none) { return (u32)__builtin_amdgcn_update_dpp((int)none, (int)v, 0x130, 0xf, 0xf, false); } // wave_shl:1
KS_DEV u32 ra_bias(int v) { return (u32)v ^ 0x80000000u; } // order-preserving i32 -> u32
KS_DEV int ra_unbias(u32 v) { return (int)(v ^ 0x80000000u); }

// The E step of a row, the one copy of its tie rules (all lanes enter; o is wave-uniform).  Ht: the lane's H~, RA_NEG where
// its cell does not exist (ex); ke = lane * e.  E is the best H~ of a lower lane, its gap paid by the lane distance: one
// inclusive max scan of H~ + ke, moved one lane up.  gap: the lane takes it (on a tie H~).  Where E came from is asked only in a
// row where some lane takes it, behind the wave-uniform guard `if (__ballot(S.gap))` of the caller (all lanes enter
// ra_e_src): the last lane below this one that attains the running maximum — a lane that equals it is a new record under >=:
// the largest lane wins a tie; lane 0 always is one.
struct ra_e { int E; bool gap; u32 key, inc; };
KS_DEV ra_e ra_e_step(int Ht, u32 lane, int ke, int o, bool ex) {
    ra_e S;
    S.key = ra_bias(Ht + ke); S.inc = ks_wave_incl_max(S.key);
    const u32 below = ks_lane_below(S.inc); // (a DPP move: outside every per-lane condition, all lanes take part)
    S.E = lane ? ra_unbias(below) - o - ke : RA_NEG;
    S.gap = ex && S.E > Ht;
    return S;
}
KS_DEV u32 ra_e_src(const ra_e &S, u32 lane) {
    const u64 rec = __ballot(S.key == S.inc) & ks_lanes_below(lane);
    return 63u - (u32)__clzll((long long)(rec | 1ULL));
}

struct ra_by_matrix {
    const signed char *s_M;
    KS_DEV void stage(i64, u32, u32, u32) const {}
    KS_DEV const signed char *row(u32, u32 cq) const { return s_M + rk_class(cq) * RK_A; }
};
#define RA_ROW_WORDS (RK_A / 4) // a profile row as u32 words
static_assert(RK_A % 4 == 0, "a profile row is whole words: rows are staged word by word");
struct ra_by_profile {
    const u32 *P; // the profile's scores as words (a pool block: aligned)
    i64 qx;       // the batch position of Q_0, the anchor's query residue
    u32 *s_rows;  // the wave's own RA_CHUNK x RA_ROW_WORDS words
    // rows base + 1 .. base + n_rows of the program: Q_x lies at batch position qx + sgn * x (inside its sequence: x <= X)
    KS_DEV void stage(i64 sgn, u32 base, u32 n_rows, u32 lane) const {
        for (u32 w = lane; w < n_rows * RA_ROW_WORDS; w += 64) {
            const u32 r = w / RA_ROW_WORDS;
            s_rows[w] = P[(u64)(qx + sgn * (i64)((u64)base + 1 + r)) * RA_ROW_WORDS + (w - r * RA_ROW_WORDS)];
        }
    }
    KS_DEV const signed char *row(u32 r, u32) const { return (const signed char *)(s_rows + r * RA_ROW_WORDS); }
};

// what k_ralign and k_rt_trace do alike around ra_extend: the scorer of a wave, and the anchor pair's score.  `table`: the
// kernel's rk_in.matrix (PROFILE: the profile's scores); qx: the batch position of the anchor's query residue
template <bool PROFILE> using ra_scorer = std::conditional_t<PROFILE, ra_by_profile, ra_by_matrix>;
template <bool PROFILE> KS_DEV ra_scorer<PROFILE> ra_scorer_of(const signed char *table, u64 qx, const signed char *s_M, u32 *s_rows) {
    if constexpr (PROFILE) return ra_by_profile{(const u32 *)table, (i64)qx, s_rows};
    else return ra_by_matrix{s_M};
}
template <bool PROFILE> KS_DEV int ra_anchor_score(const signed char *table, u64 qx, const u8 *s_cls, const signed char *s_M, u32 cq, u32 ct) {
    if constexpr (PROFILE) return rk_by_profile{s_cls, table}.pair(qx, cq, ct);
    else return rk_by_matrix{s_cls, s_M}.pair(qx, cq, ct);
}

// One side's extension (all 64 lanes enter; every argument but `lane` and `strip` is wave-uniform).  Q_x = qp[sgn * x] for
// x = 1 .. X and T_y = tp[sgn * y] for y = 1 .. Y: the caller points qp / tp at the anchor pair.  strip: the wave's own.
// A: W, o, e, x_drop.  TR: rows 1 .. x_end (the caller has checked x_end <= min(X, Y + W), y_end <= Y, |y_end - x_end| <= W)
// write their directions to dir[(x - 1) * RA_DIR_ROW + lane]; x, y, score = the end cell and its H, the counts are zero.
template <bool TR, class SC, class Args>
KS_DEV ra_ext ra_extend(const u8 *qp, const u8 *tp, i64 sgn, u32 X, u32 Y, const Args &A, const u8 *s_cls, const SC &sc,
                        unsigned short *strip, u32 lane, u8 *dir = nullptr, u32 x_end = 0, u32 y_end = 0) {
    const u32 W = A.W, ke = lane * A.e;
    const int oe = (int)(A.o + A.e), e = (int)A.e, o = (int)A.o;
    const bool inband = lane <= 2 * W;
    // row 0: H(0, 0) = 0, H(0, y) = E from it
    const int y0 = (int)lane - (int)W;
    bool ex = inband && y0 >= 0 && (u32)y0 <= Y;
    int H = ex ? (y0 ? -(o + y0 * e) : 0) : RA_NEG, F = RA_NEG;
    ra_cnt Hc = {0u, 0u, ex && y0 > 0 ? 1u : 0u, ex ? (u32)y0 : 0u}, Fc = {0u, 0u, 0u, 0u};
    int bH = H, B = 0; // the lane's best cell; the best row maximum so far (R_0 = H(0, 0) = 0)
    u32 bx = 0;
    ra_cnt bc = Hc;
    const u32 x_max = TR ? x_end : X < Y + W ? X : Y + W; // the last row that has a cell
    bool stop = false;
    for (u32 base = 0; base < x_max && !stop; base += RA_CHUNK) {
        const u32 left = x_max - base, n_rows = left < RA_CHUNK ? left : RA_CHUNK;
        u32 qbyte = 0;
        if (lane < n_rows) qbyte = qp[sgn * (i64)((u64)base + 1 + lane)];
        __builtin_amdgcn_wave_barrier(); // (the rows of the chunk before have read the strip; same wave: LDS operations execute in order)
#pragma unroll
        for (u32 h = 0; h < 2; h++) { // entry j of the strip is T_y, y = base + 1 - W + j
            const u32 j = lane + 64 * h;
            const i64 y = (i64)base + 1 - (i64)W + j;
            u32 v = 0;
            if (y >= 1 && y <= (i64)Y) {
                const u32 c = tp[sgn * y];
                v = rk_upper(c) | ((u32)s_cls[c] << 8);
            }
            strip[j] = (unsigned short)v;
        }
        sc.stage(sgn, base, n_rows, lane);
        __builtin_amdgcn_wave_barrier();
        for (u32 r = 0; r < n_rows; r++) {
            const u32 x = base + 1 + r;
            const u32 cq = (u32)__builtin_amdgcn_readlane((int)qbyte, (int)r);
            const u32 cq_up = rk_upper(cq);
            const signed char *const s_row = sc.row(r, cq);
            const i64 y = (i64)x + lane - W;
            ex = inband && y >= 0 && y <= (i64)Y;
            const u32 tv = strip[r + lane];
            const int s = s_row[tv >> 8];
            const bool idt = (tv & 0xffu) == cq_up;
            // F: what the lane above hands down from the row before (on a tie the continued gap)
            const int gH = H - oe, gF = F - e;
            const bool cont = gF >= gH;
            const int G = cont ? gF : gH;
            const ra_cnt Gc = {cont ? Fc.id : Hc.id, cont ? Fc.po : Hc.po, cont ? Fc.go : Hc.go + 1u, (cont ? Fc.ga : Hc.ga) + 1u};
            const int Fn = (int)ra_lane_above((u32)G, (u32)RA_NEG);
            ra_cnt Fnc = {0u, 0u, 0u, 0u};
            if (!TR) Fnc = {ra_lane_above(Gc.id, 0u), ra_lane_above(Gc.po, 0u), ra_lane_above(Gc.go, 0u), ra_lane_above(Gc.ga, 0u)};
            // D: the lane's own diagonal; H~ = max(D, F), on a tie D
            const int D = H + s;
            const bool diag = D >= Fn;
            int Ht = diag ? D : Fn;
            ra_cnt Htc = {diag ? Hc.id + (idt ? 1u : 0u) : Fnc.id, diag ? Hc.po + (s > 0 ? 1u : 0u) : Fnc.po, diag ? Hc.go : Fnc.go,
                          diag ? Hc.ga : Fnc.ga};
            if (!ex) Ht = RA_NEG;
            const ra_e S = ra_e_step(Ht, lane, (int)ke, o, ex);
            H = Ht; Hc = Htc;
            u32 code = (diag ? RA_DIR_DIAG : 0u) | (cont ? RA_DIR_CONT : 0u);
            if (__ballot(S.gap)) {
                const u32 src = ra_e_src(S, lane);
                if (TR) {
                    if (S.gap) { H = S.E; code |= (lane - src) << RA_DIR_E; }
                } else { // the counts of the path into the source
                    const u32 sid = (u32)__shfl((int)Htc.id, (int)src), spo = (u32)__shfl((int)Htc.po, (int)src);
                    const u32 sgo = (u32)__shfl((int)Htc.go, (int)src), sga = (u32)__shfl((int)Htc.ga, (int)src);
                    if (S.gap) { H = S.E; Hc = {sid, spo, sgo + 1u, sga + (lane - src)}; }
                }
            }
            F = Fn; Fc = Fnc;
            if (!ex) { H = RA_NEG; F = RA_NEG; }
            if (TR) {
                dir[(u64)(x - 1) * RA_DIR_ROW + lane] = (u8)code; // (a row is one 64-byte store of the wave)
                continue;
            }
            const int R = ra_unbias((u32)__builtin_amdgcn_readlane((int)ks_wave_incl_max(ra_bias(H)), 63)); // the row's maximum
            if (ex && H > bH) { bH = H; bx = x; bc = Hc; }
            B = R > B ? R : B;
            if (B - R > (int)A.x_drop) { stop = true; break; }
        }
    }
    ra_ext out;
    if (TR) { // H of the end cell: the lane of its diagonal, after row x_end (row 0 where x_end == 0)
        out.x = x_end; out.y = y_end;
        out.score = __shfl(H, (int)(y_end + W - x_end));
        out.c = {0u, 0u, 0u, 0u};
        return out;
    }
    // the largest H; then the smallest x; then the smallest y = the lowest lane (lane W holds H(0, 0) = 0: there is a real one)
    const u64 m = ks_wave_max64(((u64)ra_bias(bH) << 32) | ((u64)(0x3ffffffu - bx) << 6) | (63u - lane));
    const u32 wl = 63u - (u32)(m & 63u);
    out.x = 0x3ffffffu - (u32)((m >> 6) & 0x3ffffffu);
    out.y = out.x + wl - W;
    out.score = ra_unbias((u32)(m >> 32));
    out.c = {(u32)__builtin_amdgcn_readlane((int)bc.id, (int)wl), (u32)__builtin_amdgcn_readlane((int)bc.po, (int)wl),
             (u32)__builtin_amdgcn_readlane((int)bc.go, (int)wl), (u32)__builtin_amdgcn_readlane((int)bc.ga, (int)wl)};
    return out;
}
