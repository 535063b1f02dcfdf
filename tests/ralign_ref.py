"""CPU restatement of ks_regions_align for the tests (include/kmerseek_amd.h: region alignments): plain Python loops over bytes
and integers, one cell at a time.  Shares no code with the library.  Not a test module."""
import numpy as np

ALPHABET = 28
COLUMNS = ("row_offsets", "q_start", "q_length", "t_start", "t_length", "score", "identities", "positives", "gap_opens", "gaps",
           "aln_length")
NONE = None  # a cell, or a state of a cell, that does not exist


def upper(x):
    """ASCII upper-casing of a byte value: only a-z change."""
    return x - 32 if 97 <= x <= 122 else x


def residue_class(x):
    """A..Z -> 0..25, * -> 26, every other byte -> 27 (after upper-casing)."""
    c = upper(x)
    if 65 <= c <= 90:
        return c - 65
    return 26 if c == 42 else 27


def default_matrix():
    m = [[-1] * ALPHABET for _ in range(ALPHABET)]
    for i in range(ALPHABET):
        m[i][i] = 1
    return m


def extend(Q, T, matrix, band, gap_open, gap_extend, x_drop):
    """One extension over Q = Q_1 .. Q_X and T = T_1 .. T_Y (bytes, walking away from the anchor).
    -> (x, y, score, identities, positives, gap_opens, gaps) of the best cell.  A state is (score, ident, pos, opens, gaps);
    the cells of a row are a dict y -> state."""
    X, Y, W, o, e = len(Q), len(T), band, gap_open, gap_extend

    def close_row(Ht):
        """H of a row from its H-tilde (E reads H-tilde only), ascending y"""
        H = {}
        src = NONE  # the y' < y with the largest H-tilde(y') + y' * e, on a tie the largest y': the source of E(y)
        for y in sorted(Ht):
            h = Ht[y]
            if src is not NONE:
                s = Ht[src]
                E = (s[0] - gap_open - (y - src) * e, s[1], s[2], s[3] + 1, s[4] + (y - src))
                if h is NONE or E[0] > h[0]:  # on a tie H-tilde
                    h = E
            assert h is not NONE
            H[y] = h
            if Ht[y] is not NONE and (src is NONE or Ht[y][0] + y * e >= Ht[src][0] + src * e):
                src = y
        return H

    H = close_row({y: ((0, 0, 0, 0, 0) if y == 0 else NONE) for y in range(0, min(Y, W) + 1)})
    F = {}
    best_cell = (0, 0) + H[0]
    run_best = max(h[0] for h in H.values())
    for x in range(1, X + 1):
        ys = range(max(0, x - W), min(Y, x + W) + 1)
        if len(ys) == 0:
            break  # (no later row has a cell either)
        Ht, Fx = {}, {}
        cq = Q[x - 1]
        for y in ys:
            f = NONE
            if y in H:  # the cell (x - 1, y) exists
                h_up, f_up = H[y], F.get(y, NONE)
                f = (h_up[0] - o - e, h_up[1], h_up[2], h_up[3] + 1, h_up[4] + 1)
                if f_up is not NONE and f_up[0] - e >= f[0]:  # on a tie the continued gap
                    f = (f_up[0] - e, f_up[1], f_up[2], f_up[3], f_up[4] + 1)
            Fx[y] = f
            d = NONE
            if y >= 1:  # (x - 1, y - 1) lies on the same diagonal: it exists
                ct = T[y - 1]
                s = int(matrix[residue_class(cq)][residue_class(ct)])
                h_d = H[y - 1]
                d = (h_d[0] + s, h_d[1] + (1 if upper(cq) == upper(ct) else 0), h_d[2] + (1 if s > 0 else 0), h_d[3], h_d[4])
            if d is NONE:
                Ht[y] = f
            elif f is NONE or d[0] >= f[0]:  # on a tie D
                Ht[y] = d
            else:
                Ht[y] = f
        H, F = close_row(Ht), Fx
        r_x = max(h[0] for h in H.values())
        for y in ys:  # ascending y: the smallest x, then the smallest y wins a tie
            if H[y][0] > best_cell[2]:
                best_cell = (x, y) + H[y]
        run_best = max(run_best, r_x)
        if run_best - r_x > x_drop:
            break
    return best_cell


def align_region(qseq, tseq, a, b, n, matrix, band, gap_open, gap_extend, x_drop):
    """One region with seed (a, b, n) of the sequences qseq / tseq (bytes) -> the ten output values."""
    assert n >= 1 and a + n <= len(qseq) and b + n <= len(tseq)
    ai, bj = a + n // 2, b + n // 2
    cq, ct = qseq[ai], tseq[bj]
    s = int(matrix[residue_class(cq)][residue_class(ct)])
    right = extend(qseq[ai + 1:], tseq[bj + 1:], matrix, band, gap_open, gap_extend, x_drop)
    left = extend(qseq[:ai][::-1], tseq[:bj][::-1], matrix, band, gap_open, gap_extend, x_drop)
    gaps = left[6] + right[6]
    pairs2 = left[0] + left[1] + right[0] + right[1] - gaps  # twice the aligned pairs of the two extensions
    assert pairs2 % 2 == 0
    return (ai - left[0], left[0] + 1 + right[0], bj - left[1], left[1] + 1 + right[1], s + left[2] + right[2],
            (1 if upper(cq) == upper(ct) else 0) + left[3] + right[3], (1 if s > 0 else 0) + left[4] + right[4],
            left[5] + right[5], gaps, 1 + pairs2 // 2 + gaps)


def align(regions, qid, tid, q_res, q_off, t_res, t_off, matrix=None, band=16, gap_open=11, gap_extend=1, x_drop=30):
    """regions: (row_offsets, q_start, t_start, length, ...) as Regions.to_host(); hit row r = (qid[r], tid[r]).
    -> the eleven columns of RegionAlignments.to_host()."""
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in np.asarray(matrix).tolist()]
    offs = [int(v) for v in regions[0]]
    qs, ts, ln = [np.asarray(c).tolist() for c in regions[1:4]]
    q_bytes, t_bytes = bytes(np.asarray(q_res, np.uint8)), bytes(np.asarray(t_res, np.uint8))
    rows, memo = [], {}
    for r in range(len(offs) - 1):
        q, t = int(qid[r]), int(tid[r])
        qseq = q_bytes[int(q_off[q]):int(q_off[q + 1])]
        tseq = t_bytes[int(t_off[t]):int(t_off[t + 1])]
        for g in range(offs[r], offs[r + 1]):
            key = (q, t, qs[g] + ln[g] // 2, ts[g] + ln[g] // 2)  # the result is a function of the anchor alone
            if key not in memo:
                memo[key] = align_region(qseq, tseq, qs[g], ts[g], ln[g], m, band, gap_open, gap_extend, x_drop)
            rows.append(memo[key])
    cols = list(zip(*rows)) if rows else [[] for _ in range(10)]
    dt = (np.uint32, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32)
    return (np.asarray(regions[0], np.uint64).copy(), *[np.asarray(c, d) for c, d in zip(cols, dt)])
