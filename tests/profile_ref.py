"""CPU restatement of the profile passes for the tests (include/kmerseek_amd.h: position-specific scores): the build rule of
ks_profile_build_device and ks_regions_score_profile / _align_profile / _traceback_profile, in plain Python loops, one residue
and one cell at a time.  The loops are this module's own: those of rscore_ref / ralign_ref / rtrace_ref index a matrix by the
query residue's class and cannot take a score per position.  Shares no code with the library (only the byte helpers of
ralign_ref and the run-length helpers of rtrace_ref).  Not a test module.

A profile is `rows`: one list of 28 integers per residue of the query BATCH; the pair of the query residue at batch position p
and the target byte ct scores rows[p][class(ct)]."""
import numpy as np

from ralign_ref import residue_class, upper
from rtrace_ref import D, EQ, I, M, X, cigar_string, run_length  # noqa: F401

A = 28
INCLUDE_QUERY = 1


# ---- the build rule ------------------------------------------------------------------------------------------------------------
def class_letter(j):
    return 65 + j if j < 26 else 42 if j == 26 else 88  # 'A' .. 'Z', '*', 'X'


def build_row(byte, cnt, depth, matrix, bg, ratio, beta, thresholds, base, flags):
    """One residue: its byte, its 28 counts and its depth -> (28 scores, consensus byte, n_obs).  Every f64 operation is one
    numpy.float64 operation, in the order of the header."""
    f = np.float64
    a = residue_class(byte)
    cnt = [int(v) for v in cnt]
    J = [j for j in range(A) if bg[j] > 0]
    top, top_j = 0, 0
    for j in range(A):
        cc = cnt[j] + (1 if j == a else 0)
        if cc > top:
            top, top_j = cc, j
    consensus = upper(byte) if depth == 0 else class_letter(top_j)
    n0 = sum(cnt[j] for j in J)
    row = [int(matrix[a][c]) for c in range(A)]
    if n0 == 0:
        return row, consensus, 0
    if (flags & INCLUDE_QUERY) and a in J:
        cnt[a] += 1
    n = sum(cnt[j] for j in J)
    with np.errstate(all="ignore"):
        for c in J:
            g = f(0.0)
            for j in J:
                g = g + f(cnt[j]) * f(ratio[j][c])
            t = g / f(n)
            t = f(bg[c]) * t
            t = f(beta) * t
            num = f(cnt[c]) + t
            den = f(n) + f(beta)
            r = (num / den) / f(bg[c])
            k = sum(1 for th in thresholds if f(th) <= r)
            row[c] = max(-127, min(127, base + k))
    return row, consensus, min(n, 2 ** 32 - 1)


def build(counts, depth, q_res, params, flags=None):
    """counts u32 [n_res, 28], depth u32 [n_res], q_res u8 [n_res]; params: anything with matrix, bg, ratio, beta, thresholds, base,
    include_query (kmerseek_amd.ProfileParams).  -> (scores int8 [n_res * 28], consensus u8 [n_res], n_obs u32 [n_res])"""
    m = params.matrix if params.matrix is not None else (2 * np.eye(A, dtype=np.int64) - 1)
    m = [[int(v) for v in r] for r in np.asarray(m).tolist()]
    bg, ratio, thr = np.asarray(params.bg, np.float64), np.asarray(params.ratio, np.float64), np.asarray(params.thresholds, np.float64)
    flags = (INCLUDE_QUERY if params.include_query else 0) if flags is None else flags
    counts = np.asarray(counts).reshape(-1, A)
    scores, cons, nobs = [], [], []
    for p in range(len(q_res)):
        row, c, n = build_row(int(q_res[p]), counts[p], int(depth[p]), m, bg, ratio, params.beta, thr, params.base, flags)
        scores += row; cons.append(c); nobs.append(n)
    return np.array(scores, np.int8), np.array(cons, np.uint8), np.array(nobs, np.uint32)


def build_columns(counts, depth, q_res, params, flags=None):
    """build() a column of residues at a time: the same f64 operations in the same order, each one numpy operation over all
    residues (numpy rounds every elementwise operation on its own) — for batches the loop above is too slow for.
    test_profile_cpu.py holds the two against each other."""
    f = np.float64
    m = np.asarray(params.matrix if params.matrix is not None else (2 * np.eye(A, dtype=np.int64) - 1), np.int64)
    bg, ratio, thr = np.asarray(params.bg, f), np.asarray(params.ratio, f), np.asarray(params.thresholds, f)
    flags = (INCLUDE_QUERY if params.include_query else 0) if flags is None else flags
    q = np.frombuffer(bytes(q_res), np.uint8).astype(np.int64)
    n_res = len(q)
    cnt = np.asarray(counts, np.uint64).reshape(n_res, A).astype(np.int64)  # (sums of 28 u32 counts fit easily)
    up = np.where((q >= 97) & (q <= 122), q - 32, q)
    a = np.where((up >= 65) & (up <= 90), up - 65, np.where(up == 42, 26, 27))
    own = np.zeros((n_res, A), np.int64)
    own[np.arange(n_res), a] = 1
    top_j = np.argmax(cnt + own, axis=1)  # (the first of equal maxima: the smaller class)
    letters = np.array([class_letter(j) for j in range(A)], np.int64)
    consensus = np.where(np.asarray(depth, np.int64) == 0, up, letters[top_j]).astype(np.uint8)
    J = np.flatnonzero(bg > 0)
    n0 = cnt[:, J].sum(axis=1)
    scores = m[a].copy()
    live = n0 != 0
    if flags & INCLUDE_QUERY:
        cnt = cnt + own * (live & (bg[a] > 0))[:, None]
    n = cnt[:, J].sum(axis=1)
    with np.errstate(all="ignore"):
        for c in J:
            g = np.zeros(n_res, f)
            for j in J:
                g = g + cnt[:, j].astype(f) * f(ratio[j][c])
            t = g / n.astype(f)
            t = f(bg[c]) * t
            t = f(params.beta) * t
            num = cnt[:, c].astype(f) + t
            den = n.astype(f) + f(params.beta)
            r = (num / den) / f(bg[c])
            k = (thr[None, :] <= r[:, None]).sum(axis=1)
            scores[:, c] = np.where(live, np.clip(params.base + k, -127, 127), scores[:, c])
    return scores.astype(np.int8).reshape(-1), consensus, np.where(live, np.minimum(n, 2 ** 32 - 1), 0).astype(np.uint32)


def matrix_rows(q_res, matrix=None):
    """The profile that IS a matrix: row p = matrix[class(q_res[p])] -> int8 [n_res, 28]"""
    m = np.asarray(matrix, np.int8) if matrix is not None else (2 * np.eye(A, dtype=np.int8) - 1).astype(np.int8)
    return np.ascontiguousarray(m[[residue_class(int(b)) for b in q_res]].reshape(-1, A))


# ---- ks_regions_score_profile --------------------------------------------------------------------------------------------------
def ungapped_extend(pairs, x_drop):
    """pairs: (score, same bytes) of the pairs j = 1, 2, ... walking away from the core -> (ext, score, identities, positives)"""
    s_run, best, best_j = 0, 0, 0
    ident, pos, ident_best, pos_best = 0, 0, 0, 0
    for j, (s, same) in enumerate(pairs, 1):
        s_run += s
        ident += 1 if same else 0
        pos += 1 if s > 0 else 0
        if s_run > best:  # strictly: the shortest extension wins a tie
            best, best_j, ident_best, pos_best = s_run, j, ident, pos
        if best - s_run > x_drop:
            break
    return best_j, best, ident_best, pos_best


def score_region(qseq, tseq, rows, a, b, n, do_extend, x_drop):
    """rows: the profile rows of qseq's residues -> the seven values of a region"""
    pair = lambda i, j: (int(rows[i][residue_class(tseq[j])]), upper(qseq[i]) == upper(tseq[j]))
    core = [pair(a + i, b + i) for i in range(n)]
    left = right = (0, 0, 0, 0)
    if do_extend:
        e_r = min(len(qseq) - (a + n), len(tseq) - (b + n))
        right = ungapped_extend([pair(a + n + j - 1, b + n + j - 1) for j in range(1, e_r + 1)], x_drop)
        left = ungapped_extend([pair(a - j, b - j) for j in range(1, min(a, b) + 1)], x_drop)
    c_s, c_id, c_po = sum(s for s, _ in core), sum(1 for _, e in core if e), sum(1 for s, _ in core if s > 0)
    return (a - left[0], b - left[0], left[0] + n + right[0], left[1] + c_s + right[1], left[2] + c_id + right[2], left[3] + c_po + right[3], c_id)


def _per_region(regions, qid, tid, q_res, q_off, t_res, t_off, P, fn):
    offs = [int(v) for v in regions[0]]
    qs, ts, ln = [np.asarray(c).tolist() for c in regions[1:4]]
    q_bytes, t_bytes = bytes(np.asarray(q_res, np.uint8)), bytes(np.asarray(t_res, np.uint8))
    P = np.asarray(P).reshape(-1, A).tolist()
    out = []
    for r in range(len(offs) - 1):
        q, t = int(qid[r]), int(tid[r])
        qb, qe = int(q_off[q]), int(q_off[q + 1])
        qseq, tseq, rows = q_bytes[qb:qe], t_bytes[int(t_off[t]):int(t_off[t + 1])], P[qb:qe]
        for g in range(offs[r], offs[r + 1]):
            out.append(fn(g, qseq, tseq, rows, qs[g], ts[g], ln[g]))
    return out


def score(regions, qid, tid, q_res, q_off, t_res, t_off, P, extend=False, x_drop=0):
    """-> the eight columns of RegionScores.to_host(); P: the profile's scores [n_q_res * 28]"""
    rows = _per_region(regions, qid, tid, q_res, q_off, t_res, t_off, P,
                       lambda g, qseq, tseq, pr, a, b, n: score_region(qseq, tseq, pr, a, b, n, extend, x_drop))
    cols = list(zip(*rows)) if rows else [[] for _ in range(7)]
    dt = (np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32)
    return (np.asarray(regions[0], np.uint64).copy(), *[np.asarray(c, d) for c, d in zip(cols, dt)])


# ---- ks_regions_align_profile ----------------------------------------------------------------------------------------------------
def gapped_extend(Q, T, band, gap_open, gap_extend, x_drop):
    """One extension; Q = [(row of 28 scores, upper-cased byte)] for Q_1 .. Q_X, T = bytes T_1 .. T_Y, both walking away from the
    anchor -> (x, y, score, identities, positives, gap_opens, gaps) of the best cell.  The recurrence and every tie rule are those
    of ks_regions_align (rtrace_ref states them); a state is (score, ident, pos, opens, gaps)."""
    X_, Y, W, o, e = len(Q), len(T), band, gap_open, gap_extend

    def close_row(Ht):
        H, src = {}, None
        for y in sorted(Ht):
            h = Ht[y]
            if src is not None:
                s = Ht[src]
                E = (s[0] - o - (y - src) * e, s[1], s[2], s[3] + 1, s[4] + (y - src))
                if h is None or E[0] > h[0]:  # on a tie H-tilde
                    h = E
            H[y] = h
            if Ht[y] is not None and (src is None or Ht[y][0] + y * e >= Ht[src][0] + src * e):  # on a tie the largest y'
                src = y
        return H

    H = close_row({y: ((0, 0, 0, 0, 0) if y == 0 else None) for y in range(0, min(Y, W) + 1)})
    F = {}
    best_cell = (0, 0) + H[0]
    run_best = max(h[0] for h in H.values())
    for x in range(1, X_ + 1):
        ys = range(max(0, x - W), min(Y, x + W) + 1)
        if len(ys) == 0:
            break
        Ht, Fx = {}, {}
        row, cq_up = Q[x - 1]
        for y in ys:
            f = None
            if y in H:
                h_up, f_up = H[y], F.get(y)
                f = (h_up[0] - o - e, h_up[1], h_up[2], h_up[3] + 1, h_up[4] + 1)
                if f_up is not None and f_up[0] - e >= f[0]:  # on a tie the continued gap
                    f = (f_up[0] - e, f_up[1], f_up[2], f_up[3], f_up[4] + 1)
            Fx[y] = f
            d = None
            if y >= 1:
                ct = T[y - 1]
                s = int(row[residue_class(ct)])
                h_d = H[y - 1]
                d = (h_d[0] + s, h_d[1] + (1 if cq_up == upper(ct) else 0), h_d[2] + (1 if s > 0 else 0), h_d[3], h_d[4])
            Ht[y] = d if d is not None and (f is None or d[0] >= f[0]) else f  # on a tie D
        H, F = close_row(Ht), Fx
        r_x = max(h[0] for h in H.values())
        for y in ys:  # ascending y: the smallest x, then the smallest y wins a tie
            if H[y][0] > best_cell[2]:
                best_cell = (x, y) + H[y]
        run_best = max(run_best, r_x)
        if run_best - r_x > x_drop:
            break
    return best_cell


def _sides(qseq, tseq, rows, ai, bj):
    """the two extensions' inputs around the anchor (ai, bj): (Q right, T right, Q left, T left)"""
    qr = [(rows[i], upper(qseq[i])) for i in range(ai + 1, len(qseq))]
    ql = [(rows[i], upper(qseq[i])) for i in range(ai - 1, -1, -1)]
    return qr, tseq[bj + 1:], ql, tseq[:bj][::-1]


def align_region(qseq, tseq, rows, a, b, n, band, gap_open, gap_extend, x_drop):
    ai, bj = a + n // 2, b + n // 2
    s = int(rows[ai][residue_class(tseq[bj])])
    qr, tr, ql, tl = _sides(qseq, tseq, rows, ai, bj)
    right = gapped_extend(qr, tr, band, gap_open, gap_extend, x_drop)
    left = gapped_extend(ql, tl, band, gap_open, gap_extend, x_drop)
    gaps = left[6] + right[6]
    pairs2 = left[0] + left[1] + right[0] + right[1] - gaps
    return (ai - left[0], left[0] + 1 + right[0], bj - left[1], left[1] + 1 + right[1], s + left[2] + right[2],
            (1 if upper(qseq[ai]) == upper(tseq[bj]) else 0) + left[3] + right[3], (1 if s > 0 else 0) + left[4] + right[4],
            left[5] + right[5], gaps, 1 + pairs2 // 2 + gaps)


def align(regions, qid, tid, q_res, q_off, t_res, t_off, P, band=16, gap_open=11, gap_extend=1, x_drop=30):
    """-> the eleven columns of RegionAlignments.to_host()"""
    memo = {}

    def one(g, qseq, tseq, pr, a, b, n):
        key = (id(pr), id(tseq), a + n // 2, b + n // 2)  # (a function of the anchor alone)
        if key not in memo:
            memo[key] = (align_region(qseq, tseq, pr, a, b, n, band, gap_open, gap_extend, x_drop), pr, tseq)
        return memo[key][0]
    rows = _per_region(regions, qid, tid, q_res, q_off, t_res, t_off, P, one)
    cols = list(zip(*rows)) if rows else [[] for _ in range(10)]
    dt = (np.uint32, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32)
    return (np.asarray(regions[0], np.uint64).copy(), *[np.asarray(c, d) for c, d in zip(cols, dt)])


# ---- ks_regions_traceback_profile ------------------------------------------------------------------------------------------------
def trace_extension(Q, T, x_end, y_end, band, gap_open, gap_extend):
    """Tables of rows 0 .. x_end, then the walk from (x_end, y_end) back to (0, 0); Q, T as gapped_extend takes them.
    -> (steps in walk order: ("P", x, y) | ("I", x) | ("D", y), H(x_end, y_end))"""
    Y, W, o, e = len(T), band, gap_open, gap_extend
    assert 0 <= x_end <= len(Q) and 0 <= y_end <= Y and abs(y_end - x_end) <= W
    Ht, F, H = {}, {}, {}  # (x, y) -> (value, choice)
    for x in range(0, x_end + 1):
        ys = list(range(max(0, x - W), min(Y, x + W) + 1))
        for y in ys:
            f = None
            if x >= 1 and (x - 1, y) in H:
                f = (H[(x - 1, y)][0] - o - e, False)
                if (x - 1, y) in F and F[(x - 1, y)][0] - e >= f[0]:
                    f = (F[(x - 1, y)][0] - e, True)
                F[(x, y)] = f
            d = None
            if x >= 1 and y >= 1:
                d = H[(x - 1, y - 1)][0] + int(Q[x - 1][0][residue_class(T[y - 1])])
            if x == 0 and y == 0:
                Ht[(x, y)] = (0, "origin")
            elif d is not None and (f is None or d >= f[0]):
                Ht[(x, y)] = (d, "D")
            elif f is not None:
                Ht[(x, y)] = (f[0], "F")
        key, ksrc = None, None
        for y in ys:
            best, src = (None, None) if key is None else (key - o - y * e, ksrc)
            if (x, y) in Ht:
                v = Ht[(x, y)][0] + y * e
                if key is None or v >= key:
                    key, ksrc = v, y
            h = Ht.get((x, y))
            H[(x, y)] = (best, src) if h is None or (best is not None and best > h[0]) else (h[0], None)
    steps = []
    x, y, state = x_end, y_end, "H"
    while True:
        if state == "H":
            _, src = H[(x, y)]
            if src is not None:
                steps += [("D", yy) for yy in range(y, src, -1)]
                y = src
            if (x, y) == (0, 0):
                break
            state = "Ht"
        elif state == "Ht":
            if Ht[(x, y)][1] == "D":
                steps.append(("P", x, y))
                x, y, state = x - 1, y - 1, "H"
            else:
                state = "F"
        else:
            cont = F[(x, y)][1]
            steps.append(("I", x))
            x, state = x - 1, ("F" if cont else "H")
    return steps, H[(x_end, y_end)][0]


def trace_region(qseq, tseq, rows, a, b, n, aln, band, gap_open, gap_extend, eqx=False):
    """aln = (q_start, q_length, t_start, t_length) -> (cigar [(len, code)], score)"""
    qs, ql, ts, tl = [int(v) for v in aln]
    ai, bj = a + n // 2, b + n // 2
    xl, yl = ai - qs, bj - ts
    xr, yr = ql - 1 - xl, tl - 1 - yl
    qr, tr, qlft, tlft = _sides(qseq, tseq, rows, ai, bj)
    right, sr = trace_extension(qr, tr, xr, yr, band, gap_open, gap_extend)
    left, sl = trace_extension(qlft, tlft, xl, yl, band, gap_open, gap_extend)
    cols = []
    for sgn, steps in ((-1, left), (0, None), (1, right[::-1])):
        if steps is None:
            cols.append((M, ai, bj))
            continue
        for st in steps:
            cols.append((M, ai + sgn * st[1], bj + sgn * st[2]) if st[0] == "P" else (I, ai + sgn * st[1], None) if st[0] == "I" else
                        (D, None, bj + sgn * st[1]))
    if eqx:
        cols = [((EQ if upper(qseq[qi]) == upper(tseq[ti]) else X), qi, ti) if c == M else (c, qi, ti) for c, qi, ti in cols]
    return run_length([c for c, _, _ in cols]), int(rows[ai][residue_class(tseq[bj])]) + sl + sr


def trace(regions, alignments, qid, tid, q_res, q_off, t_res, t_off, P, band=16, gap_open=11, gap_extend=1, eqx=False):
    """alignments = RegionAlignments.to_host() -> per region its cigar [(len, code)]"""
    al = [np.asarray(c).tolist() for c in alignments[1:5]]
    sc = np.asarray(alignments[5]).tolist()

    def one(g, qseq, tseq, pr, a, b, n):
        cg, s = trace_region(qseq, tseq, pr, a, b, n, [c[g] for c in al], band, gap_open, gap_extend, eqx)
        assert s == sc[g], (g, s, sc[g])
        return cg
    return _per_region(regions, qid, tid, q_res, q_off, t_res, t_off, P, one)


def rescore(cigar, qseq, tseq, rows, q_start, t_start, gap_open, gap_extend):
    """The ops alone replayed under the profile rows of qseq -> (score, identities, positives, gap_opens, gaps, aln_length,
    q_length, t_length)"""
    qi, ti = q_start, t_start
    score = ident = pos = opens = gaps = length = 0
    for n, c in cigar:
        length += n
        if c in (M, EQ, X):
            for _ in range(n):
                s = int(rows[qi][residue_class(tseq[ti])])
                score += s; ident += 1 if upper(qseq[qi]) == upper(tseq[ti]) else 0; pos += 1 if s > 0 else 0
                qi += 1; ti += 1
        else:
            opens += 1; gaps += n
            score -= gap_open + n * gap_extend
            if c == I:
                qi += n
            else:
                ti += n
    return score, ident, pos, opens, gaps, length, qi - q_start, ti - t_start
