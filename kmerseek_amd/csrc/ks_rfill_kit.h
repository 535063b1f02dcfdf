// ks_rfill_kit.h — the fill of a link's rectangle: the global affine program of a wave over the two stretches, its walk back
// and the = / X pass over the finished columns.  Its one caller is st_fill of ks_stitch_kit.h, the fill kernel of the two
// passes that stitch a chain into one alignment (ks_rstitch.hip: members of one protein pair; ks_fstitch.hip: members in the
// frames of one strand); that kit holds everything else of a stitch once.  One definition: the recurrence, the tie rules, the
// orientation and the fence cannot differ between the two passes.
#pragma once
#include "ks_rpath_kit.h"

#define RF_SHORT_MAX 63u // the shorter side of a filled rectangle: column 0 .. 63 are the lanes

// The rectangle of a link as the fill takes it: X query and Y target residues; swap: X < Y — the query stretch is T, the lanes;
// else the target stretch is.  nT <= RF_SHORT_MAX <, = nQ.
struct rf_rect { u32 X, Y, nQ, nT; bool swap; };
KS_DEV rf_rect rf_rect_of(u32 X, u32 Y, bool swap) { return rf_rect{X, Y, swap ? Y : X, swap ? X : Y, swap}; }

// One wave, all lanes enter; every argument but `lane` is wave-uniform.  qst: the X query residues of the link, tst: its Y target
// residues.  Lane y holds column y of T; a step is one row x of Q.  H and F stay in registers: F is the lane's own, D reads the H of
// the lane below (DPP), E is ra_e_step of ks_ralign_kit.h.  Q's residues are staged 64 rows at a time (a lane per row, a readlane
// per step), T's class is loaded once.  One direction byte per cell into `dir` (RA_DIR_ROW bytes per row of Q), rp_publish, then
// the wave walks back from (|Q|, |T|) — rp_walk<true> — writing one byte per column backward into col[0 .. cap), cap = X + Y the
// room of the slot.  `swap` exchanges the two gap codes and the matrix index.  walked(n): called by all lanes as soon as the walk
// is done, n the columns of the path, which are col[cap - n .. cap), or RP_BAD — the kernel records it.  eqx != 0: the pairs then
// become = / X in a pass over the finished columns (rp_places).  s_cls, s_M: the tables of rk_stage_tables in LDS; stage: the
// wave's own RP_STAGE rows.
// 32-bit scores: at most 4096 + 63 steps of |M| <= 128 and gaps of at most 255 + 255 per residue.
template <class Walked>
KS_DEV void rf_fill(const rf_rect R, const u8 *qst, const u8 *tst, u32 gap_open, u32 gap_extend, u32 eqx, u8 *dir, u8 *col, u32 cap,
                    const u8 *s_cls, const signed char *s_M, uint4 *stage, u32 lane, Walked &&walked) {
    const bool swap = R.swap;
    const u32 X = R.X, Y = R.Y, nQ = R.nQ, nT = R.nT;
    const u8 *const Qs = swap ? tst : qst, *const Ts = swap ? qst : tst;

    // forward: rows 1 .. nQ
    const int o = (int)gap_open, e = (int)gap_extend, oe = o + e, ke = (int)(lane * gap_extend);
    const bool ex = lane <= nT;
    u32 tcls = 0;
    if (lane >= 1 && lane <= nT) tcls = s_cls[Ts[lane - 1]];
    int H = ex ? (lane ? -(o + ke) : 0) : RA_NEG, F = RA_NEG;
    for (u32 base = 0; base < nQ; base += 64) {
        const u32 left = nQ - base, n_rows = left < 64u ? left : 64u;
        u32 qbyte = 0;
        if (lane < n_rows) qbyte = Qs[base + lane];
        for (u32 rr = 0; rr < n_rows; rr++) {
            const u32 x = base + 1 + rr;
            const u32 qcls = rk_class((u32)__builtin_amdgcn_readlane((int)qbyte, (int)rr));
            const int s = swap ? s_M[tcls * RK_A + qcls] : s_M[qcls * RK_A + tcls]; // M[class(query)][class(target)]
            const int gH = H - oe, gF = F - e;
            const bool cont = gF >= gH; // (on a tie the continued gap)
            const int Fn = cont ? gF : gH;
            const int Hb = (int)ks_lane_below((u32)H); // (a DPP move: all lanes take part)
            const int D = lane ? Hb + s : RA_NEG;
            const bool diag = D >= Fn; // (on a tie D)
            int Ht = diag ? D : Fn;
            if (!ex) Ht = RA_NEG;
            const ra_e S = ra_e_step(Ht, lane, ke, o, ex);
            u32 code = (diag ? RA_DIR_DIAG : 0u) | (cont ? RA_DIR_CONT : 0u);
            H = Ht;
            if (__ballot(S.gap)) {
                const u32 src = ra_e_src(S, lane);
                if (S.gap) { H = S.E; code |= (lane - src) << RA_DIR_E; }
            }
            F = Fn;
            if (!ex) { H = RA_NEG; F = RA_NEG; }
            dir[(u64)(x - 1) * RA_DIR_ROW + lane] = (u8)code;
        }
    }
    rp_publish();

    // back from (nQ, lane nT) to (0, lane 0); the columns go backward from col[cap - 1]
    const u32 n = rp_walk<true>(dir, nQ, nT, 0u, RF_SHORT_MAX, swap ? RP_I : RP_D, swap ? RP_D : RP_I, col, -1, cap, stage, lane);
    if (n == RP_BAD) { walked(RP_BAD); return; }
    walked(n);
    if (!eqx) return;
    rp_publish();
    u8 *const path = col + (cap - n);
    u32 nq = 0, nt = 0;
    for (u32 c = 0; c < n; c += 64) {
        const u32 i = c + lane;
        const bool valid = i < n;
        const u32 code = valid ? path[i] : 0xffu;
        const rp_place at = rp_places(valid, code, lane, nq, nt);
        if (code == RP_M && at.q < X && at.t < Y) path[i] = (u8)(rk_upper(qst[at.q]) == rk_upper(tst[at.t]) ? RP_EQ : RP_X);
    }
}
