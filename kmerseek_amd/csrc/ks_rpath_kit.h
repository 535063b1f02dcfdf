// ks_rpath_kit.h — what the two passes that walk a banded affine-gap program back share (ks_rtrace.hip, lanes as diagonals;
// ks_rstitch.hip, lanes as columns): the op codes, the fence between the direction stores and the walk, the stage loader, the
// walk, the places of a pair's two residues, and on the host the cut of a call into slices that fit the scratch budget.  The
// direction byte and the E step that writes its jump are one header down, in ks_ralign_kit.h: ra_extend<false> of
// ks_ralign.hip takes that same E step and includes nothing of the walk.  One definition each: a tie rule, a fence or a bounds
// check cannot be changed in one pass and not in the other.
#pragma once
#include <cstdint>
#include <vector>

// ---- host side: no device work, nothing of the project's: tests/hostsan/san_slices.cpp compiles it alone ----
// Items 0 .. n - 1 need off[i + 1] - off[i] rows (off: their exclusive scan, n + 1 values).  Greedy: a slice takes
// consecutive items while their rows fit budget_rows; an item of no rows always fits.  cut: the slices' bounds (0 .. n);
// first_row: off[] of each slice's first item; max_rows: the largest slice.  bad < n: the first item that does not fit alone
// (bad_rows: what it needs); the cut stops in front of it.
struct rp_slices {
    std::vector<uint64_t> cut{0}, first_row{0};
    uint64_t max_rows = 0, bad = ~(uint64_t)0, bad_rows = 0;
};
static inline rp_slices rp_cut_slices(const uint64_t *off, uint64_t n, uint64_t budget_rows) {
    rp_slices Z;
    for (uint64_t i0 = 0; i0 < n;) {
        uint64_t i1 = i0;
        while (i1 < n && off[i1 + 1] - off[i0] <= budget_rows) i1++;
        if (i1 == i0) { Z.bad = i0; Z.bad_rows = off[i0 + 1] - off[i0]; return Z; }
        if (off[i1] - off[i0] > Z.max_rows) Z.max_rows = off[i1] - off[i0];
        Z.cut.push_back(i1);
        if (i1 < n) Z.first_row.push_back(off[i1]);
        i0 = i1;
    }
    return Z;
}

#ifdef __HIPCC__
#include "ks_ralign_kit.h"

// The slices of a call whose n items need total_rows rows of directions, d_off their scan on the device.  Only a call that does
// not fit in one slice brings the offsets to the host to cut them.  The caller looks at Z->bad: the refusal's sentence is its own.
static inline int rp_slices_of(ks_ctx *ctx, const u64 *d_off, u64 n, u64 total_rows, u64 budget_rows, rp_slices *Z) {
    if (total_rows <= budget_rows) { Z->cut.push_back(n); Z->max_rows = total_rows; return KS_OK; }
    std::vector<u64> off((size_t)n + 1);
    KS_TRY(ks_copy_d2h(ctx, off.data(), d_off, off.size() * sizeof(u64)));
    *Z = rp_cut_slices(off.data(), n, budget_rows);
    return KS_OK;
}

enum : u32 { RP_M = 0, RP_I = 1, RP_D = 2, RP_EQ = 7, RP_X = 8 }; // BAM op codes
KS_DEV bool rp_is_pair(u32 c) { return c == RP_M || c == RP_EQ || c == RP_X; }
KS_DEV u32 rp_even(u32 v) { return (v + 1u) & ~1u; } // rows of a direction slot: it begins on a 128-byte line and shares none
#define RP_STAGE 64u // rows of directions a walk stages at once (ks_debug_rtrace_stage, ks_debug_rstitch_stage)
#define RP_BAD 0xffffffffu
static_assert(RP_STAGE * RA_DIR_ROW == 64 * 4 * 16, "a stage is four 16-byte loads per lane");

// Between the last direction store of a wave and the first load of its walk.  The directions a lane stores are read back by
// other lanes of the SAME wave and by nobody else.  Both go through the one vector-memory path of the wave's compute unit: its L1
// is write-through and keeps a line it holds consistent with a store from its own CU (program order of a single work-item
// needs no less).  This orders them: a workgroup-scope release, an explicit s_waitcnt vmcnt(0) — every direction store is
// acknowledged by L2 before the first load of the walk is issued — and a workgroup-scope acquire so that the compiler moves no
// load above it.  No agent-scope fence: no other CU reads these bytes in this launch, and the next launch starts with clean
// L1s.
KS_DEV void rp_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// rows cb + 1 .. x (at most RP_STAGE) of a direction slot into the wave's own stage: four 16-byte loads per lane
KS_DEV void rp_stage_rows(const u8 *dir, u32 cb, u32 x, uint4 *stage, u32 lane) {
    const uint4 *src = (const uint4 *)(dir + (u64)cb * RA_DIR_ROW);
    __builtin_amdgcn_wave_barrier(); // (the steps before have read the stage; same wave: LDS operations execute in order)
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        const u32 i = j * 64 + lane;
        if (i < (x - cb) * (RA_DIR_ROW / 16)) stage[i] = src[i];
    }
    __builtin_amdgcn_wave_barrier();
}

// The walk from the cell (x, lane k) back to (0, lane k0) through the direction bytes of ks_ralign_kit.h (all lanes enter;
// every argument but `lane` is wave-uniform and so is every step: the dependent chain is LDS reads only).  COL: the lanes are
// columns — a D step goes one lane down, an F step stays and reads the lane's own RA_DIR_CONT; else they are diagonals of a
// band, lanes 0 .. kmax — a D step stays, an F step goes one lane up and reads that lane's.  An E jump is op_e, an F step
// op_f.  At most `room` columns: diagonals write col[0], col[step], col[2 * step] ..., step = +-1; columns write backward from
// col[room - 1] (the slot is the room: a 32-bit index).  Every run is counted against the room left and every lane index
// against 0 and kmax, so no combination of inputs writes outside the slot.
// -> the columns written, or RP_BAD: a step that leaves the lanes or the room, a walk that does not close.
template <bool COL>
KS_DEV u32 rp_walk(const u8 *dir, u32 x, u32 k, u32 k0, u32 kmax, u32 op_e, u32 op_f, u8 *col, i64 step, u32 room, uint4 *stage, u32 lane) {
    u32 n = 0;
    bool inF = false, bad = false;
    auto put = [&](u32 op, u32 cnt) { // cnt <= 63 equal columns, a lane each
        if (cnt > room - n) { bad = true; return; }
        if (lane < cnt) {
            if (COL) col[room - 1u - (n + lane)] = (u8)op;
            else col[step * (i64)(n + lane)] = (u8)op;
        }
        n += cnt;
    };
    const u8 *const st = (const u8 *)stage;
    while (x > 0 && !bad) {
        const u32 cb = (x - 1) & ~(RP_STAGE - 1u);
        rp_stage_rows(dir, cb, x, stage, lane);
        while (x > cb && !bad) {
            const u8 *row = st + (x - 1 - cb) * RA_DIR_ROW;
            if (!inF) { // H(x, lane k)
                u32 b = row[k];
                const u32 d = b >> RA_DIR_E;
                if (d) { // E: a jump of d target residues from the H~ of lane k - d
                    if (d > k) { bad = true; break; }
                    put(op_e, d);
                    k -= d;
                    b = row[k];
                }
                if (b & RA_DIR_DIAG) { // D: (x - 1, y - 1)
                    if (COL && k == 0) { bad = true; break; }
                    put(RP_M, 1u);
                    x -= 1; k -= COL ? 1u : 0u;
                    continue;
                }
                inF = true;
            }
            // F(x, lane k): one query residue, from (x - 1, y) — its F again or its H
            if (!COL && k >= kmax) { bad = true; break; }
            k += COL ? 0u : 1u;
            inF = (row[k] & RA_DIR_CONT) != 0;
            put(op_f, 1u);
            x -= 1;
        }
    }
    if (bad || inF || k < k0) return RP_BAD; // (row 0 has no F, and no cell below y = 0)
    if (k > k0) put(op_e, k - k0);           // H(0, y) is an E of y residues from (0, 0)
    return bad ? RP_BAD : n;
}

// Lane i of a step of 64 alignment columns (valid: it has one, `code`): the places of its column's two residues — the query
// residues (columns that are no D) and the target residues (no I) before it — and nq / nt move on past the step.
struct rp_place { u32 q, t; };
KS_DEV rp_place rp_places(bool valid, u32 code, u32 lane, u32 &nq, u32 &nt) {
    const u64 mq = __ballot(valid && code != RP_D), mt = __ballot(valid && code != RP_I);
    const rp_place P{nq + (u32)__popcll(mq & ks_lanes_below(lane)), nt + (u32)__popcll(mt & ks_lanes_below(lane))};
    nq += (u32)__popcll(mq); nt += (u32)__popcll(mt);
    return P;
}
#endif
