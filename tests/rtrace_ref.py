"""CPU restatement of ks_regions_traceback for the tests (include/kmerseek_amd.h: region traceback): plain Python loops that
fill the banded H-tilde / F / H tables of one extension cell by cell, remember every choice, and walk back from the end cell.
Shares no code with the library (only the byte helpers of ralign_ref).  Not a test module.

The recurrence, once more.  One extension over Q_1 .. Q_X and T_1 .. T_Y lives on the cells (x, y), 0 <= x <= X, 0 <= y <= Y,
|y - x| <= W; a cell outside does not exist and is never a source.
    H~(0, 0) = 0                                    (no other H~ in row 0)
    F(x, y)  = max(H(x - 1, y) - o - e, F(x - 1, y) - e)                  tie: the continued gap
    D(x, y)  = H(x - 1, y - 1) + M[class(Q_x)][class(T_y)]
    H~(x, y) = max(D, F)                                                  tie: D
    E(x, y)  = max over existing y' < y of H~(x, y') - o - (y - y') * e   tie: the largest y'
    H(x, y)  = max(H~, E)                                                 tie: H~
Columns, query as the read: a D step is an aligned pair (M; with eqx = where the upper-cased bytes are equal, X otherwise), an
F step is I (a query residue without a target residue), an E jump of L is D x L."""
from ralign_ref import default_matrix, residue_class, upper

M, I, D, EQ, X = 0, 1, 2, 7, 8  # BAM op codes
OP_CHARS = {M: "M", I: "I", D: "D", EQ: "=", X: "X"}


def trace_extension(Q, T, x_end, y_end, matrix, band, gap_open, gap_extend):
    """Tables of rows 0 .. x_end, then the walk from (x_end, y_end) back to (0, 0).
    -> (steps, score, events): steps in walk order, each ("P", x, y) an aligned pair of Q_x and T_y, ("I", x) or ("D", y);
    score = H(x_end, y_end); events: which ties and shapes lay ON the path (the tests' coverage)."""
    Y, W, o, e = len(T), band, gap_open, gap_extend
    assert 0 <= x_end <= len(Q) and 0 <= y_end <= Y and abs(y_end - x_end) <= W

    def exists(x, y):
        return 0 <= x and 0 <= y <= Y and abs(y - x) <= W

    Ht, F, H = {}, {}, {}  # (x, y) -> (value, choice, tie)
    for x in range(0, x_end + 1):
        ys = [y for y in range(max(0, x - W), min(Y, x + W) + 1)]
        for y in ys:
            f = None
            if x >= 1 and exists(x - 1, y):
                f = (H[(x - 1, y)][0] - o - e, False, False)
                if (x - 1, y) in F:
                    c = F[(x - 1, y)][0] - e
                    if c >= f[0]:
                        f = (c, True, c == f[0])
                F[(x, y)] = f
            d = None
            if x >= 1 and y >= 1:
                d = H[(x - 1, y - 1)][0] + int(matrix[residue_class(Q[x - 1])][residue_class(T[y - 1])])
            if x == 0 and y == 0:
                Ht[(x, y)] = (0, "origin", False)
            elif d is not None and (f is None or d >= f[0]):
                Ht[(x, y)] = (d, "D", f is not None and d == f[0])
            elif f is not None:
                Ht[(x, y)] = (f[0], "F", False)
        # E: over the y' < y of the row, the largest H~(x, y') + y' * e decides (the rest of the term is the same for all of
        # them); among equal ones the largest y'.  Ascending y: (key, src, tie) is the decision over the cells passed so far.
        key, ksrc, ktie = None, None, False
        for y in ys:
            best, src, tie = (None, None, False) if key is None else (key - o - y * e, ksrc, ktie)
            if (x, y) in Ht:
                v = Ht[(x, y)][0] + y * e
                if key is None or v > key:
                    key, ksrc, ktie = v, y, False
                elif v == key:
                    ksrc, ktie = y, True
            h = Ht.get((x, y))
            if h is None or (best is not None and best > h[0]):
                H[(x, y)] = (best, src, tie)
            else:
                H[(x, y)] = (h[0], None, best is not None and best == h[0])
    steps, events = [], set()
    x, y, state = x_end, y_end, "H"
    while True:
        if W >= 1 and abs(y - x) == W:
            events.add("band_edge")
        if state == "H":
            v, src, tie = H[(x, y)]
            if src is None:
                if tie:
                    events.add("tie_H")
                if (x, y) == (0, 0):
                    break
                state = "Ht"
            else:
                if tie:
                    events.add("tie_E")
                if y - src > 1:
                    events.add("E_jump_gt1")
                if x == 0:
                    events.add("row0_gap")
                for yy in range(y, src, -1):
                    steps.append(("D", yy))
                y, state = src, "Ht"
                if (x, y) == (0, 0):
                    break
        elif state == "Ht":
            v, choice, tie = Ht[(x, y)]
            if choice == "D":
                if tie:
                    events.add("tie_Ht")
                steps.append(("P", x, y))
                x, y, state = x - 1, y - 1, "H"
            else:
                assert choice == "F"
                state = "F"
        else:
            v, cont, tie = F[(x, y)]
            if tie:
                events.add("tie_F")
            steps.append(("I", x))
            x, state = x - 1, ("F" if cont else "H")
    return steps, H[(x_end, y_end)][0], events


def run_length(codes):
    out = []
    for c in codes:
        if out and out[-1][1] == c:
            out[-1][0] += 1
        else:
            out.append([1, c])
    return [(n, c) for n, c in out]


def trace_region(qseq, tseq, a, b, n, aln, matrix, band, gap_open, gap_extend, eqx=False):
    """One region with seed (a, b, n); aln = (q_start, q_length, t_start, t_length) of its alignment.
    -> (cigar [(len, code)], columns [(code, qi or None, ti or None)], score, events)."""
    qs, ql, ts, tl = [int(v) for v in aln]
    ai, bj = a + n // 2, b + n // 2
    xl, yl = ai - qs, bj - ts
    xr, yr = ql - 1 - xl, tl - 1 - yl
    assert xl >= 0 and yl >= 0 and xr >= 0 and yr >= 0
    right, sr, er = trace_extension(qseq[ai + 1:], tseq[bj + 1:], xr, yr, matrix, band, gap_open, gap_extend)
    left, sl, el = trace_extension(qseq[:ai][::-1], tseq[:bj][::-1], xl, yl, matrix, band, gap_open, gap_extend)
    cols = []
    for sgn, steps in ((-1, left), (0, None), (1, right[::-1])):
        if steps is None:
            cols.append((M, ai, bj))
            continue
        for st in steps:
            if st[0] == "P":
                cols.append((M, ai + sgn * st[1], bj + sgn * st[2]))
            elif st[0] == "I":
                cols.append((I, ai + sgn * st[1], None))
            else:
                cols.append((D, None, bj + sgn * st[1]))
    if eqx:
        cols = [((EQ if upper(qseq[qi]) == upper(tseq[ti]) else X), qi, ti) if c == M else (c, qi, ti) for c, qi, ti in cols]
    s_anchor = int(matrix[residue_class(qseq[ai])][residue_class(tseq[bj])])
    events = el | er
    codes = [c for c, _, _ in cols]
    for i in range(len(codes) - 1):
        if {codes[i], codes[i + 1]} == {I, D}:
            events.add("I_beside_D")
    return run_length(codes), cols, s_anchor + sl + sr, events


def rescore(cigar, qseq, tseq, q_start, t_start, matrix, gap_open, gap_extend):
    """The ops alone, replayed on the sequences -> (score, identities, positives, gap_opens, gaps, aln_length, q_length,
    t_length): what the alignment's columns must say."""
    qi, ti = q_start, t_start
    score = ident = pos = opens = gaps = length = 0
    for n, c in cigar:
        length += n
        if c in (M, EQ, X):
            for _ in range(n):
                s = int(matrix[residue_class(qseq[qi])][residue_class(tseq[ti])])
                same = upper(qseq[qi]) == upper(tseq[ti])
                assert c == M or (c == EQ) == same
                score += s; ident += 1 if same else 0; pos += 1 if s > 0 else 0
                qi += 1; ti += 1
        else:
            opens += 1; gaps += n
            score -= gap_open + n * gap_extend
            if c == I:
                qi += n
            else:
                ti += n
    return score, ident, pos, opens, gaps, length, qi - q_start, ti - t_start


def cigar_string(cigar):
    return "".join(f"{n}{OP_CHARS[c]}" for n, c in cigar)


def trace(regions, alignments, qid, tid, q_res, q_off, t_res, t_off, matrix=None, band=16, gap_open=11, gap_extend=1, eqx=False):
    """regions = Regions.to_host(), alignments = RegionAlignments.to_host() of them -> per region (cigar, events)."""
    import numpy as np
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in np.asarray(matrix).tolist()]
    offs = [int(v) for v in regions[0]]
    qs, ts, ln = [np.asarray(c).tolist() for c in regions[1:4]]
    al = [np.asarray(c).tolist() for c in alignments[1:5]]
    q_bytes, t_bytes = bytes(np.asarray(q_res, np.uint8)), bytes(np.asarray(t_res, np.uint8))
    out, memo = [], {}
    for r in range(len(offs) - 1):
        q, t = int(qid[r]), int(tid[r])
        qseq = q_bytes[int(q_off[q]):int(q_off[q + 1])]
        tseq = t_bytes[int(t_off[t]):int(t_off[t + 1])]
        for g in range(offs[r], offs[r + 1]):
            key = (q, t, qs[g] + ln[g] // 2, ts[g] + ln[g] // 2, al[0][g], al[1][g], al[2][g], al[3][g])
            if key not in memo:
                cg, _, _, ev = trace_region(qseq, tseq, qs[g], ts[g], ln[g], [c[g] for c in al], m, band, gap_open, gap_extend, eqx)
                memo[key] = (cg, ev)
            out.append(memo[key])
    return out
