"""CPU restatement of ks_regions_stitch for the tests (include/kmerseek_amd.h: region stitch): plain Python loops, column by
column.  Shares no code with the library; the fill is rtrace_ref.trace_extension — the same recurrence — with a band so wide that
every cell of the rectangle exists, the columns are rtrace_ref.rescore of the final ops.  Not a test module.

Per hit row the chain lists the members m_0 .. m_(k-1); an end is start + length.
    trim    member i >= 1 loses the fewest leading columns such that its position is >= the ORIGINAL ends of member i - 1 on
            both sequences; it then starts at (q', t')
    link    X = q' - q_end[i - 1], Y = t' - t_end[i - 1]: nothing / I x X / D x Y / a fill where min(X, Y) <= 63 and
            max(X, Y) <= max_fill / otherwise open: I x X then D x Y
    fill    T is the SHORTER stretch (X == Y: the target's).  Roles swapped (the query stretch is T): an F step is D, an E jump I
    splice  everything concatenated, adjacent equal ops merged
EVENTS names what a row can go through: the CPU tests ask the GPU tests' inputs to cover them."""
import math

import numpy as np

import rtrace_ref
from ralign_ref import default_matrix, upper

M, I, D, EQ, X = rtrace_ref.M, rtrace_ref.I, rtrace_ref.D, rtrace_ref.EQ, rtrace_ref.X
SHORT_MAX = 63
DEFAULT_MAX_FILL = 1024
EVENTS = ("trimmed", "trimmed_to_nothing", "pure_I", "pure_D", "filled", "filled_swapped", "open", "joint_merged", "tie_E", "tie_F")
NAMES = ("op_offsets", "ops", "q_start", "q_length", "t_start", "t_length", "score", "identities", "positives", "gap_opens", "gaps",
         "aln_length", "n_members", "n_filled", "n_open", "n_trimmed", "row_score")
DTYPES = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32, np.uint32,
          np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.float64)


def columns_of(cigar):
    out = []
    for n, c in cigar:
        out += [c] * n
    return out


def fill(qst, tst, matrix, gap_open, gap_extend, eqx):
    """The global alignment of the two stretches -> (column codes in forward order, score, events of the path, swapped)."""
    x, y = len(qst), len(tst)
    swapped = x < y
    if not swapped:
        steps, score, ev = rtrace_ref.trace_extension(qst, tst, x, y, matrix, x + y, gap_open, gap_extend)
        code = {"I": I, "D": D}
    else:  # Q is the target stretch, T the query stretch; a pair still scores M[class(query)][class(target)]
        mt = [[matrix[b][a] for b in range(len(matrix))] for a in range(len(matrix[0]))]
        steps, score, ev = rtrace_ref.trace_extension(tst, qst, y, x, mt, x + y, gap_open, gap_extend)
        code = {"I": D, "D": I}
    cols = []
    for st in steps[::-1]:
        if st[0] == "P":
            qi, ti = (st[2], st[1]) if swapped else (st[1], st[2])
            cols.append(M if not eqx else EQ if upper(qst[qi - 1]) == upper(tst[ti - 1]) else X)
        else:
            cols.append(code[st[0]])
    return cols, score, ev, swapped


def stitch_row(members, qseq, tseq, matrix, gap_open, gap_extend, max_fill=DEFAULT_MAX_FILL, eqx=False):
    """members: [(q_start, q_length, t_start, t_length, cigar [(len, code)])] in chain order.
    -> (cigar, n_filled, n_open, n_trimmed, events); ValueError for what the library refuses."""
    cols, events = [], set()
    n_filled = n_open = n_trim = 0
    for i, (qs, ql, ts, tl, cigar) in enumerate(members):
        mine = columns_of(cigar)
        if any(c not in (M, I, D, EQ, X) for c in mine) or sum(c != D for c in mine) != ql or sum(c != I for c in mine) != tl:
            raise ValueError(f"member {i}: the ops do not consume its extents")
        if any(c == (M if eqx else EQ) or (not eqx and c == X) for c in mine):
            raise ValueError(f"member {i}: M where = / X are expected or the other way round")
        if qs + ql > len(qseq) or ts + tl > len(tseq) or ql == 0 or tl == 0:
            raise ValueError(f"member {i}: an extent outside its sequence")
        link = []
        if i > 0:
            pqs, pql, pts, ptl, _ = members[i - 1]
            pqe, pte = pqs + pql, pts + ptl
            if qs + ql < pqe or ts + tl < pte:
                raise ValueError(f"member {i}: ends before the member in front of it")
            qp, tp, c = qs, ts, 0
            while not (qp >= pqe and tp >= pte):
                qp += mine[c] != D
                tp += mine[c] != I
                c += 1
            if c:
                events.add("trimmed")
                if c == len(mine):
                    events.add("trimmed_to_nothing")
            n_trim += c
            mine = mine[c:]
            x, y = qp - pqe, tp - pte
            if x == 0 and y == 0:
                pass
            elif y == 0:
                link = [I] * x
                events.add("pure_I")
            elif x == 0:
                link = [D] * y
                events.add("pure_D")
            elif min(x, y) <= SHORT_MAX and max(x, y) <= max_fill:
                link, _, ev, swapped = fill(qseq[pqe:qp], tseq[pte:tp], matrix, gap_open, gap_extend, eqx)
                n_filled += 1
                events.add("filled_swapped" if swapped else "filled")
                events |= {e for e in ("tie_E", "tie_F") if e in ev}
            else:
                link = [I] * x + [D] * y
                n_open += 1
                events.add("open")
        for piece in (link, mine):
            if piece and cols and cols[-1] == piece[0]:
                events.add("joint_merged")
            cols += piece
    return rtrace_ref.run_length(cols), n_filled, n_open, n_trim, events


def stitch(chain, alignments, cigars, qid, tid, q_res, q_off, t_res, t_off, matrix=None, gap_open=11, gap_extend=1, max_fill=0,
           eqx=False):
    """chain = RegionChain.to_host(), alignments = RegionAlignments.to_host() it was made of, cigars = RegionCigars.to_host() of
    those -> (the arrays of HitAlignments.to_host(), in that order; the union of the rows' events)."""
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in np.asarray(matrix).tolist()]
    max_fill = max_fill or DEFAULT_MAX_FILL
    c_offs, src = [int(v) for v in chain[0]], [int(v) for v in chain[1]]
    a_offs = [int(v) for v in alignments[0]]
    ext = [np.asarray(c).tolist() for c in alignments[1:5]]
    g_offs, g_ops = [int(v) for v in cigars[0]], [int(v) for v in cigars[1]]
    q_bytes, t_bytes = bytes(np.asarray(q_res, np.uint8)), bytes(np.asarray(t_res, np.uint8))
    out = {n: [] for n in NAMES}
    out["op_offsets"].append(0)
    events = set()
    for r in range(len(c_offs) - 1):
        q, t = int(qid[r]), int(tid[r])
        qseq, tseq = q_bytes[int(q_off[q]):int(q_off[q + 1])], t_bytes[int(t_off[t]):int(t_off[t + 1])]
        mem = src[c_offs[r]:c_offs[r + 1]]
        if any(not a_offs[r] <= g < a_offs[r + 1] for g in mem):
            raise ValueError(f"row {r}: a src_region outside the row's alignments")
        members = [(ext[0][g], ext[1][g], ext[2][g], ext[3][g], [(v >> 4, v & 15) for v in g_ops[g_offs[g]:g_offs[g + 1]]]) for g in mem]
        cigar, n_filled, n_open, n_trim, ev = stitch_row(members, qseq, tseq, m, gap_open, gap_extend, max_fill, eqx)
        events |= ev
        qs, ts = (members[0][0], members[0][2]) if members else (0, 0)
        qe, te = (members[-1][0] + members[-1][1], members[-1][2] + members[-1][3]) if members else (0, 0)
        score, ident, pos, opens, gaps, length, ql, tl = rtrace_ref.rescore(cigar, qseq, tseq, qs, ts, m, gap_open, gap_extend)
        assert (ql, tl) == (qe - qs, te - ts)  # the ops consume exactly the span
        out["ops"] += [(n << 4) | c for n, c in cigar]
        out["op_offsets"].append(len(out["ops"]))
        for n, v in (("q_start", qs), ("q_length", qe - qs), ("t_start", ts), ("t_length", te - ts), ("score", score), ("identities", ident),
                     ("positives", pos), ("gap_opens", opens), ("gaps", gaps), ("aln_length", length), ("n_members", len(members)),
                     ("n_filled", n_filled), ("n_open", n_open), ("n_trimmed", n_trim), ("row_score", float(score) if members else math.nan)):
            out[n].append(v)
    return tuple(np.array(out[n], d) for n, d in zip(NAMES, DTYPES)), events


def assert_same(got, want, what=""):
    assert len(got) == len(want) == len(NAMES)
    for n, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype, f"{what}: {n} is {g.dtype}, expected {w.dtype}"
        assert g.shape == w.shape, f"{what}: {n} has {g.shape}, expected {w.shape}"
        if not np.array_equal(g, w, equal_nan=(n == "row_score")):
            at = np.flatnonzero(~((g == w) | ((g != g) & (w != w))))[:8]
            raise AssertionError(f"{what}: {n} differs at {at.tolist()}: got {g[at].tolist()}, expected {w[at].tolist()}")


def strings(op_offsets, ops):
    offs, ops = [int(v) for v in op_offsets], [int(v) for v in ops]
    return ["".join(f"{v >> 4}{rtrace_ref.OP_CHARS[v & 15]}" for v in ops[offs[r]:offs[r + 1]]) for r in range(len(offs) - 1)]
