"""CPU restatement of ks_frames_stitch for the tests (include/kmerseek_amd.h: frame stitch): plain Python loops, column by column.
Shares no code with the library; a link's rectangle is rstitch_ref.fill — the recurrence of rtrace_ref — and the op codes are
rtrace_ref's.  Not a test module.

Per folded row the chain lists the members m_0 .. m_(k-1), each an alignment in one frame of the strand.  A strand base position
p reads the codon that is residue p // 3 of frame p % 3 of the strand.
    trim    member i >= 1 loses the fewest leading columns such that its strand position is >= the ORIGINAL strand end of member
            i - 1 and its target position >= that member's target end; a query-consuming column moves the strand position by 3
    link    X = p' - E bases, Y = t' - T_e residues, c = X // 3, r = X % 3: the protein link of rstitch_ref on (c, Y) with the c
            codons read in the previous member's frame directly after its end, then, if r, ONE N op of length r
    splice  everything concatenated, adjacent equal ops merged, N never
EVENTS names what a row can go through: the CPU test asks the fuzz inputs to cover them."""
import math

import numpy as np

import rstitch_ref
import rtrace_ref
from ralign_ref import default_matrix, residue_class, upper

M, I, D, EQ, X = rtrace_ref.M, rtrace_ref.I, rtrace_ref.D, rtrace_ref.EQ, rtrace_ref.X
N = 3  # BAM code of the frameshift op (KS_CIGAR_FSHIFT)
OP_CHARS = {**rtrace_ref.OP_CHARS, N: "N"}
SHORT_MAX = rstitch_ref.SHORT_MAX
DEFAULT_MAX_FILL = rstitch_ref.DEFAULT_MAX_FILL
DEFAULT_COST = 15
MAX_LEN = 2 ** 20
EVENTS = ("trimmed", "trimmed_to_nothing", "shift_1", "shift_2", "shift_with_codons", "same_frame_link", "pure_I", "pure_D", "filled",
          "filled_swapped", "open", "joint_merged")
NAMES = ("op_offsets", "ops", "s_start", "nt_length", "nt_start", "t_start", "t_length", "score", "identities", "positives", "gap_opens",
         "gaps", "aln_length", "n_members", "n_filled", "n_open", "n_trimmed", "n_frameshifts", "row_score")
DTYPES = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32, np.uint32,
          np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.float64)


class StitchError(ValueError):
    """what the library refuses: `kind` is one of src, fsrc, fold, strand, row, len, ext, ops, code, asc; `index` the offender"""

    def __init__(self, kind, index):
        super().__init__(f"{kind} at {index}")
        self.kind, self.index = kind, index


def stitch_row(members, frames3, tseq, matrix, gap_open, gap_extend, max_fill=DEFAULT_MAX_FILL, eqx=False):
    """members: [(s_start, nt_length, t_start, t_length, cigar [(len, code)])] in chain order, s_start in strand bases;
    frames3: the residues of the strand's three frames.  -> (ops [(len, code)] with N ops, n_filled, n_open, n_trimmed, events)"""
    ops, events = [], set()  # runs [len, code], merged as the columns come; an N run merges with nothing
    n_filled = n_open = n_trim = 0

    def splice(piece):
        if piece and ops and ops[-1][1] == piece[0] != N:
            events.add("joint_merged")
        for col in piece:
            if ops and ops[-1][1] == col != N:
                ops[-1][0] += 1
            else:
                ops.append([1, col])

    for i, (ss, nl, ts, tl, cigar) in enumerate(members):
        mine = rstitch_ref.columns_of(cigar)
        if i > 0:
            pss, pnl, pts, ptl, _ = members[i - 1]
            E, Te = pss + pnl, pts + ptl
            p, t, c = ss, ts, 0
            while not (p >= E and t >= Te):
                p += 3 * (mine[c] != D)
                t += mine[c] != I
                c += 1
            if c:
                events.add("trimmed")
                if c == len(mine):
                    events.add("trimmed_to_nothing")
            n_trim += c
            mine = mine[c:]
            Xb, Y = p - E, t - Te
            cod, r = Xb // 3, Xb % 3
            qst = frames3[E % 3][E // 3:E // 3 + cod]  # the link's codons, read in the previous member's frame
            assert len(qst) == cod
            link = []
            if cod == 0 and Y == 0:
                pass
            elif Y == 0:
                link = [I] * cod
                events.add("pure_I")
            elif cod == 0:
                link = [D] * Y
                events.add("pure_D")
            elif min(cod, Y) <= SHORT_MAX and max(cod, Y) <= max_fill:
                link, _, _, swapped = rstitch_ref.fill(qst, tseq[Te:t], matrix, gap_open, gap_extend, eqx)
                n_filled += 1
                events.add("filled_swapped" if swapped else "filled")
            else:
                link = [I] * cod + [D] * Y
                n_open += 1
                events.add("open")
            splice(link)
            if r:
                ops.append([r, N])
                events.add("shift_%d" % r)
                if cod:
                    events.add("shift_with_codons")
            else:
                events.add("same_frame_link")
        splice(mine)
    return [(n, c) for n, c in ops], n_filled, n_open, n_trim, events


def rescore(ops, frames3, tseq, s_start, t_start, matrix, gap_open, gap_extend, cost):
    """The ops alone, replayed -> (score, identities, positives, gap_opens, gaps, aln_length, nt_length, t_length, n_frameshifts)"""
    p, t = s_start, t_start
    score = ident = pos = opens = gaps = length = shifts = 0
    for n, c in ops:
        if c == N:
            p += n; shifts += 1; score -= cost
            continue
        length += n
        if c in (M, EQ, X):
            for _ in range(n):
                a, b = frames3[p % 3][p // 3], tseq[t]
                s = int(matrix[residue_class(a)][residue_class(b)])
                same = upper(a) == upper(b)
                assert c == M or (c == EQ) == same
                score += s; ident += same; pos += s > 0
                p += 3; t += 1
        else:
            opens += 1; gaps += n
            score -= gap_open + n * gap_extend
            if c == I:
                p += 3 * n
            else:
                t += n
    return score, ident, pos, opens, gaps, length, p - s_start, t - t_start, shifts


def stitch(fold, folded_hits, chain, alignments, cigars, f_res, f_off, t_res, t_off, matrix=None, gap_open=11, gap_extend=1, max_fill=0,
           eqx=False, frameshift_cost=DEFAULT_COST):
    """fold = FrameFold.to_host() (ffold_ref.NAMES), folded_hits = its Hits.to_host(), chain = RegionChain.to_host() of
    chain_frames, alignments = RegionAlignments.to_host() the fold was made of, cigars = RegionCigars.to_host() of those,
    f_res / f_off the frame batch of translate6 -> (the arrays of FrameAlignments.to_host(), in that order; the union of the
    rows' events).  StitchError for what the library refuses, the kinds in the order the library reports them."""
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in np.asarray(matrix).tolist()]
    max_fill = max_fill or DEFAULT_MAX_FILL
    ints = lambda a: [int(v) for v in np.asarray(a).tolist()]  # noqa: E731
    f_offs, f_src, f_frame, f_ntlen, f_sstart, f_ntstart, f_ts3, f_tl3 = (ints(fold[i]) for i in (1, 2, 3, 4, 5, 6, 7, 8))
    c_offs, c_src = ints(chain[0]), ints(chain[1])
    a_qs, a_ql, a_ts, a_tl = (ints(alignments[i]) for i in (1, 2, 3, 4))
    g_offs, g_ops = ints(cigars[0]), ints(cigars[1])
    qid, tid = ints(folded_hits[0]), ints(folded_hits[1])
    f_off, t_off = ints(f_off), ints(t_off)
    f_bytes, t_bytes = bytes(np.asarray(f_res, np.uint8)[:f_off[-1]]), bytes(np.asarray(t_res, np.uint8))
    n_f, n_t, n_rows = len(f_off) - 1, len(t_off) - 1, len(c_offs) - 1
    # the refusals, each kind over all members, in the library's order
    bad = {}

    def note(kind, index):
        bad[kind] = min(bad.get(kind, index), index)

    rows_members = []
    for r in range(n_rows):
        mem, prev = [], None
        for j in range(c_offs[r], c_offs[r + 1]):
            fg = c_src[j]
            cur = None
            if not (fg < len(f_src) and f_offs[r] <= fg < f_offs[r + 1]):
                note("src", j)
            elif f_src[fg] >= len(a_qs):
                note("fsrc", fg)
            else:
                g, fr, q, t = f_src[fg], f_frame[fg], qid[r], tid[r]
                qs, ql, ts, tl = a_qs[g], a_ql[g], a_ts[g], a_tl[g]
                s6 = 6 * (q >> 1) + 3 * (q & 1)
                if fr >= 6 or fr // 3 != (q & 1):
                    note("strand", fg)
                elif (f_sstart[fg], f_ntlen[fg], f_ts3[fg], f_tl3[fg]) != (fr % 3 + 3 * qs, 3 * ql, 3 * ts, 3 * tl):
                    note("fold", fg)
                elif s6 + 3 > n_f or t >= n_t:
                    note("row", r)
                else:
                    Lq, Lt = f_off[s6 + fr % 3 + 1] - f_off[s6 + fr % 3], t_off[t + 1] - t_off[t]
                    if Lq > MAX_LEN or Lt > MAX_LEN:
                        note("len", r)
                    elif ql == 0 or tl == 0 or qs + ql > Lq or ts + tl > Lt:
                        note("ext", g)
                    else:
                        cg = [(v >> 4, v & 15) for v in g_ops[g_offs[g]:g_offs[g + 1]]]
                        cols = rstitch_ref.columns_of(cg)
                        cur = (fr % 3 + 3 * qs, 3 * ql, ts, tl, cg)
                        if prev is not None and (cur[0] + cur[1] < prev[0] + prev[1] or ts + tl < prev[2] + prev[3]):
                            note("asc", j)
                        elif any(c not in (M, I, D, EQ, X) for c in cols) or sum(c != D for c in cols) != ql or sum(c != I for c in cols) != tl:
                            note("ops", g)
                        elif any(c == (M if eqx else EQ) or (not eqx and c == X) for c in cols):
                            note("code", g)
            mem.append(cur)
            prev = cur
        rows_members.append(mem)
    for kind in ("src", "fsrc", "fold", "strand", "row", "len", "ext", "ops", "code", "asc"):
        if kind in bad:
            raise StitchError(kind, bad[kind])
    out = {n: [] for n in NAMES}
    out["op_offsets"].append(0)
    events = set()
    for r in range(n_rows):
        members = rows_members[r]
        q, t = qid[r], tid[r]
        s6 = 6 * (q >> 1) + 3 * (q & 1)
        frames3 = [f_bytes[f_off[s6 + f]:f_off[s6 + f + 1]] for f in range(3)] if members else [b""] * 3
        tseq = t_bytes[t_off[t]:t_off[t + 1]] if members else b""
        ops, n_filled, n_open, n_trim, ev = stitch_row(members, frames3, tseq, m, gap_open, gap_extend, max_fill, eqx)
        events |= ev
        ss, ts = (members[0][0], members[0][2]) if members else (0, 0)
        se, te = (members[-1][0] + members[-1][1], members[-1][2] + members[-1][3]) if members else (0, 0)
        ns = 0
        if members:
            ns = f_ntstart[c_src[c_offs[r + 1] - 1]] if q & 1 else f_ntstart[c_src[c_offs[r]]]
        score, ident, pos, opens, gaps, length, nl, tl, shifts = rescore(ops, frames3, tseq, ss, ts, m, gap_open, gap_extend, frameshift_cost)
        # the two invariants: the ops consume exactly the span
        pairs = sum(n for n, c in ops if c in (M, EQ, X))
        assert 3 * (pairs + sum(n for n, c in ops if c == I)) + sum(n for n, c in ops if c == N) == se - ss == nl
        assert pairs + sum(n for n, c in ops if c == D) == te - ts == tl
        out["ops"] += [(n << 4) | c for n, c in ops]
        out["op_offsets"].append(len(out["ops"]))
        for n, v in (("s_start", ss), ("nt_length", se - ss), ("nt_start", ns), ("t_start", ts), ("t_length", te - ts), ("score", score),
                     ("identities", ident), ("positives", pos), ("gap_opens", opens), ("gaps", gaps), ("aln_length", length),
                     ("n_members", len(members)), ("n_filled", n_filled), ("n_open", n_open), ("n_trimmed", n_trim), ("n_frameshifts", shifts),
                     ("row_score", float(score) if members else math.nan)):
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
    return ["".join(f"{v >> 4}{OP_CHARS[v & 15]}" for v in ops[offs[r]:offs[r + 1]]) for r in range(len(offs) - 1)]
