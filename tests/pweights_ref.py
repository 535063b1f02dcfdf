"""The three weighting passes of include/kmerseek_amd.h restated in plain loops: ks_entry_weights_device (entry weights),
ks_wpileup_device (the pileup that sums them) and ks_profile_build_weighted_device (the rows made from it).  Integers are
Python integers; the f64 operations of the build are numpy.float64 operations, one at a time, in the header's order.  Shares no
code with the library.  Not a test module.

The arguments of the first two are those of pileup_ref.pileup (pileup_cases.ref_args): that function judges the call — a call the
device refuses raises its PileupError — and this module walks the entries once more for what the weights need."""
import numpy as np

import pileup_ref as PR
from profile_ref import class_letter
from ralign_ref import residue_class, upper

A = 28
ONE = 1 << 30
INCLUDE_QUERY = 1


class CountsError(ValueError):
    """a taken entry holds a column the counts do not: the lowest such entry"""
    def __init__(self, entry):
        super().__init__(f"counts at {entry}")
        self.entry = entry


def entry_columns(row_offsets, op_offsets, ops, start, other_start, row_mask, qid, tid, offsets, side="target", profile=False,
                  other_res=None, other_off=None):
    """Per entry None (not taken: a masked row, or no pair column) or its pair columns [(p, class of the other side's residue —
    None without the profile)], p in batch coordinates.  The call is one pileup_ref.pileup accepts."""
    n_rows, n_entries = len(qid), len(op_offsets) - 1
    on_q = side == "query"
    rows = list(range(n_rows + 1)) if row_offsets is None else [int(v) for v in row_offsets]
    out = [None] * n_entries
    for r in range(n_rows):
        if row_mask is not None and not row_mask[r]:
            continue
        sid, oid = (int(qid[r]), int(tid[r])) if on_q else (int(tid[r]), int(qid[r]))
        for e in range(rows[r], rows[r + 1]):
            p = int(offsets[sid]) + int(start[e])
            o = int(other_off[oid]) + int(other_start[e]) if profile else 0
            cols = []
            for v in ops[int(op_offsets[e]):int(op_offsets[e + 1])]:
                n, c = int(v) >> 4, int(v) & 15
                if c in PR.PAIR:
                    for _ in range(n):
                        cols.append((p, PR.res_class(int(other_res[o])) if profile else None))
                        p += 1; o += 1
                elif c == PR.N:
                    pass
                elif (c == PR.I) == on_q:
                    p += n
                else:
                    o += n
            out[e] = cols or None
    return out


def weights(args, counts, res=None, judged=False):
    """args: pileup_cases.ref_args(case, side, True); counts u32 [n_res * 28]; res: the side's residues for
    KS_PWEIGHTS_INCLUDE_QUERY, else None; judged: pileup_ref.pileup has taken these arguments already
    -> (weight u32[n_entries], n_cols u32[n_entries], S: the sums, None where not taken)"""
    if not judged:
        PR.pileup(**args)  # (the shared refusals)
    counts = [[int(v) for v in row] for row in np.asarray(counts).reshape(-1, A).tolist()]
    if res is not None:
        for p, row in enumerate(counts):
            row[PR.res_class(int(res[p]))] += 1
    k = [sum(1 for v in row if v > 0) for row in counts]
    weight, n_cols, sums = [], [], []
    bad = None
    for e, cols in enumerate(entry_columns(**args)):
        if cols is None:
            weight.append(0); n_cols.append(0); sums.append(None)
            continue
        if any(counts[p][c] == 0 for p, c in cols):
            bad = e if bad is None else bad
            weight.append(0); n_cols.append(0); sums.append(None)
            continue
        s = sum(ONE // (k[p] * counts[p][c]) for p, c in cols)
        weight.append(s // len(cols)); n_cols.append(len(cols)); sums.append(s)
    if bad is not None:
        raise CountsError(bad)
    return np.array(weight, np.uint32), np.array(n_cols, np.uint32), sums


def weighted_pileup(args, weight, base=None):
    """base: what pileup_ref.pileup gave for these arguments, if the caller has it
    -> (the nine arrays of pileup_ref.pileup, wdepth u64[n_res], wcounts u64[n_res * 28] — empty without the profile)"""
    if base is None:
        base, _ = PR.pileup(**args)
    n_res, profile = int(args["offsets"][-1]), args["profile"]
    wdepth = [0] * n_res
    wcounts = [[0] * A for _ in range(n_res)] if profile else []
    for e, cols in enumerate(entry_columns(**args)):
        for p, c in cols or ():
            wdepth[p] += int(weight[e])
            if profile:
                wcounts[p][c] += int(weight[e])
    assert all(sum(row) == d for row, d in zip(wcounts, wdepth))
    return base, np.array(wdepth, np.uint64), np.array([v for row in wcounts for v in row], np.uint64)


def build_row(byte, cnt, wcnt, depth, matrix, bg, ratio, beta, thresholds, base, flags):
    """One residue: its byte, 28 counts, 28 weighted counts and depth -> (28 scores, consensus byte, n_obs)"""
    f = np.float64
    a = residue_class(byte)
    cnt, wcnt = [int(v) for v in cnt], [int(v) for v in wcnt]
    J = [j for j in range(A) if bg[j] > 0]
    # the consensus: all 28 classes, the query's own column term whatever the flag
    if depth == 0:
        consensus = upper(byte)
    else:
        cq = list(cnt)
        cq[a] += 1
        kq = sum(1 for v in cq if v > 0)
        V = list(wcnt)
        V[a] += ONE // (kq * cq[a])
        top, top_j = 0, a
        for j in range(A):
            if V[j] > top:
                top, top_j = V[j], j
        consensus = class_letter(top_j)
    row = [int(matrix[a][c]) for c in range(A)]
    n0 = sum(cnt[j] for j in J)
    if n0 == 0:
        return row, consensus, 0
    inc = bool(flags & INCLUDE_QUERY) and a in J
    if inc:
        cnt[a] += 1
    n = sum(cnt[j] for j in J)
    k = sum(1 for j in J if cnt[j] > 0)
    W_j = list(wcnt)
    if inc:
        W_j[a] += ONE // (k * cnt[a])
    W = sum(W_j[j] for j in J)
    if W == 0:
        return row, consensus, 0
    with np.errstate(all="ignore"):
        x = {j: (f(W_j[j]) / f(W)) * f(k) for j in J}
        for c in J:
            g = f(0.0)
            for j in J:
                g = g + x[j] * f(ratio[j][c])
            t = g / f(k)
            t = f(bg[c]) * t
            t = f(beta) * t
            num = x[c] + t
            den = f(k) + f(beta)
            r = (num / den) / f(bg[c])
            row[c] = max(-127, min(127, base + sum(1 for th in thresholds if f(th) <= r)))
    return row, consensus, min(n, 2 ** 32 - 1)


def build(counts, wcounts, depth, q_res, params, flags=None):
    """counts u32 [n_res, 28], wcounts u64 [n_res, 28], depth u32 [n_res], q_res u8 [n_res]; params: a ProfileParams
    -> (scores int8 [n_res * 28], consensus u8 [n_res], n_obs u32 [n_res])"""
    m = params.matrix if params.matrix is not None else (2 * np.eye(A, dtype=np.int64) - 1)
    m = [[int(v) for v in r] for r in np.asarray(m).tolist()]
    bg, ratio, thr = np.asarray(params.bg, np.float64), np.asarray(params.ratio, np.float64), np.asarray(params.thresholds, np.float64)
    flags = (INCLUDE_QUERY if params.include_query else 0) if flags is None else flags
    counts, wcounts = np.asarray(counts).reshape(-1, A).tolist(), np.asarray(wcounts).reshape(-1, A).tolist()
    scores, cons, nobs = [], [], []
    memo = {}
    for p in range(len(q_res)):
        key = (int(q_res[p]), tuple(counts[p]), tuple(wcounts[p]), int(depth[p]))  # (a batch is mostly residues nobody was aligned to)
        if key not in memo:
            memo[key] = build_row(key[0], counts[p], wcounts[p], key[3], m, bg, ratio, params.beta, thr, params.base, flags)
        row, c, n = memo[key]
        scores += row; cons.append(c); nobs.append(n)
    return np.array(scores, np.int8), np.array(cons, np.uint8), np.array(nobs, np.uint32)


def build_columns(counts, wcounts, depth, q_res, params, flags=None):
    """build() a column of residues at a time: the same integer and f64 operations in the same order, each one numpy operation
    over all residues (numpy rounds every elementwise operation on its own) — for batches the loop above is too slow for.
    test_pweights_cpu.py holds the two against each other.  The weight sums of a residue must stay below 2^63."""
    f, u = np.float64, np.uint64
    m = np.asarray(params.matrix if params.matrix is not None else (2 * np.eye(A, dtype=np.int64) - 1), np.int64)
    bg, ratio, thr = np.asarray(params.bg, f), np.asarray(params.ratio, f), np.asarray(params.thresholds, f)
    flags = (INCLUDE_QUERY if params.include_query else 0) if flags is None else flags
    q = np.frombuffer(bytes(q_res), np.uint8).astype(np.int64)
    n_res = len(q)
    cnt = np.asarray(counts, u).reshape(n_res, A).astype(np.int64)
    w = np.asarray(wcounts, u).reshape(n_res, A).astype(np.int64)
    assert (w.sum(axis=1) >= 0).all() and (w >= 0).all()
    up = np.where((q >= 97) & (q <= 122), q - 32, q)
    a = np.where((up >= 65) & (up <= 90), up - 65, np.where(up == 42, 26, 27))
    own = np.zeros((n_res, A), np.int64)
    own[np.arange(n_res), a] = 1
    rows = np.arange(n_res)
    # the consensus
    cq = cnt + own
    term = ONE // ((cq > 0).sum(axis=1) * cq[rows, a])
    top_j = np.argmax(w + own * term[:, None], axis=1)  # (the first of equal maxima: the smaller class; V_a > 0 always)
    letters = np.array([class_letter(j) for j in range(A)], np.int64)
    consensus = np.where(np.asarray(depth, np.int64) == 0, up, letters[top_j]).astype(np.uint8)
    # the rows
    J = np.flatnonzero(bg > 0)
    n0 = cnt[:, J].sum(axis=1)
    inc = (n0 != 0) & (bg[a] > 0) if flags & INCLUDE_QUERY else np.zeros(n_res, bool)
    cnt = cnt + own * inc[:, None]
    n = cnt[:, J].sum(axis=1)
    k = (cnt[:, J] > 0).sum(axis=1)
    with np.errstate(all="ignore"):
        qterm = np.where(inc, ONE // np.maximum(k * cnt[rows, a], 1), 0)
    w = w + own * qterm[:, None]
    W = w[:, J].sum(axis=1)
    live = (n0 != 0) & (W != 0)
    scores = m[a].copy()
    with np.errstate(all="ignore"):
        x = {j: (w[:, j].astype(f) / W.astype(f)) * k.astype(f) for j in J}
        for c in J:
            g = np.zeros(n_res, f)
            for j in J:
                g = g + x[j] * f(ratio[j][c])
            t = g / k.astype(f)
            t = f(bg[c]) * t
            t = f(params.beta) * t
            num = x[c] + t
            den = k.astype(f) + f(params.beta)
            r = (num / den) / f(bg[c])
            kk = (thr[None, :] <= r[:, None]).sum(axis=1)
            scores[:, c] = np.where(live, np.clip(params.base + kk, -127, 127), scores[:, c])
    return scores.astype(np.int8).reshape(-1), consensus, np.where(live, np.minimum(n, 2 ** 32 - 1), 0).astype(np.uint32)
