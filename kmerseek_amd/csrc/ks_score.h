// ks_score.h — the similarity score of one hit row, shared by the passes that rank or threshold rows (ks_best.hip,
// ks_cluster.hip): one definition, so that two passes can never disagree on a row.  f64, one rounding per operation.
#pragma once
#include "ks_device.h"

// the distinct-hash counts of a sketch set: cnt of a gapped set, else the CSR run; off == NULL: no set
struct bh_set {
    const u64 *off;
    const u32 *cnt;
    u32 n;
};
KS_DEV u64 bh_size(const bh_set &S, u32 i) { return S.cnt ? (u64)S.cnt[i] : S.off[i + 1] - S.off[i]; }

static inline bh_set bh_set_of(const ks_sketches *s) {
    if (!s) return bh_set{nullptr, nullptr, 0};
    return bh_set{s->d_offsets, s->gapped ? s->d_counts : nullptr, s->n_seqs};
}

// Score of row r = (q, t, is) under key `by` (KS_BEST_*); Q / T: the sizes of the query / target side, score: the caller's
// column (KS_BEST_SCORE).  The ids are in range (the caller checked them against the sets that are not NULL).
// *bad_size: a size the key divides by is 0 — the score is then (double)is / 1.0 and the caller refuses the row.
KS_DEV double bh_row_score(u32 by, u32 r, u32 q, u32 t, u32 is, const bh_set &Q, const bh_set &T, const double *score, bool *bad_size) {
#pragma clang fp contract(off)
    *bad_size = false;
    if (by == KS_BEST_INTERSECT) return (double)is;
    if (by == KS_BEST_SCORE) return score[r];
    const u64 nt = bh_size(T, t), nq = by == KS_BEST_TARGET_CONTAINMENT ? 1ULL : bh_size(Q, q);
    u64 den = nt;
    if (by == KS_BEST_MAX_CONTAINMENT) den = nq < nt ? nq : nt;
    else if (by == KS_BEST_JACCARD) den = nq + nt - (u64)is;
    if (nq == 0 || nt == 0) { *bad_size = true; den = 1; }
    return (double)is / (double)den;
}
