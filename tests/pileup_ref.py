"""The contract of ks_pileup_device (include/kmerseek_amd.h) restated in plain loops over entries, ops and columns, and nothing
else: no interval marks, no scans, no numpy arithmetic but the two f64 divisions the contract names.  Not a test module.

pileup(...) -> (the arrays of Pileup.to_host(), in that order; the events met).  It asserts on every call that the 28 counts of a
residue sum to its depth and that depth sums to the pair columns taken.  A call the device refuses raises PileupError with the
kind and the index the device names: the first KIND in the order of KINDS, and of that kind the lowest index."""
import numpy as np

M, I, D, N, EQ, X = 0, 1, 2, 3, 7, 8  # BAM op codes; N: KS_CIGAR_FSHIFT
PAIR = (M, EQ, X)
OPS = (M, I, D, N, EQ, X)
OP_CHARS = {M: "M", I: "I", D: "D", N: "N", EQ: "=", X: "X"}
A = 28
NAMES = ("depth", "counts", "length", "n_alignments", "covered", "max_depth", "depth_sum", "breadth", "mean_depth")
DTYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.float64, np.float64)
EVENTS = ("run_merged", "I_on_query_side", "D_on_target_side", "N_op", "ends_at_sequence_end", "begins_at_next_sequence_start",
          "empty_sequence", "masked_row", "row_without_entries", "depth_over_255")
KINDS = ("row_csr", "op_csr", "id", "op", "extent", "seq", "offsets")  # the order the device reports in


class PileupError(ValueError):
    def __init__(self, kind, index):
        super().__init__(f"{kind} at {index}")
        self.kind, self.index = kind, index


def res_class(b):
    """the residue classes of ks_residue_composition_device: A..Z without case, '*', everything else"""
    if 97 <= b <= 122:
        b -= 32
    return b - 65 if 65 <= b <= 90 else 26 if b == 42 else 27


def parse(cigar):
    out, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append((n << 4) | {v: k for k, v in OP_CHARS.items()}[ch])
            n = 0
    return out


def _csr_offender(offs, count):
    for i in range(len(offs) - 1):
        if offs[i] > offs[i + 1]:
            return i
    return len(offs) - 1 if offs[-1] != count else None


def pileup(row_offsets, op_offsets, ops, start, other_start, row_mask, qid, tid, offsets, side="target", profile=False, other_res=None,
           other_off=None):
    """row_offsets: None for one entry per row.  start / other_start: the entries' starts on the side / on the other side (profile
    only).  offsets: the side's batch; other_res / other_off: the other batch (profile only)."""
    ints = lambda a: [int(v) for v in a]  # noqa: E731
    op_offsets, ops, start, qid, tid, offsets = ints(op_offsets), ints(ops), ints(start), ints(qid), ints(tid), ints(offsets)
    n_rows, n_entries, n_seqs, n_res = len(qid), len(op_offsets) - 1, len(offsets) - 1, int(offsets[-1])
    on_q, reads_q = side == "query", side == "query" or profile
    assert side in ("query", "target") and len(start) == n_entries
    if profile:
        other_start, other_off, other_res = ints(other_start), ints(other_off), bytes(np.asarray(other_res, np.uint8))
        n_other, n_other_res = len(other_off) - 1, len(other_res)
    if row_offsets is None:
        assert n_entries == n_rows
        row_offsets = list(range(n_rows + 1))
    else:
        row_offsets = ints(row_offsets)
        assert len(row_offsets) == n_rows + 1
    events = set()
    bad = {}

    def offend(kind, index):
        bad[kind] = min(bad.get(kind, index), index)

    at = _csr_offender(row_offsets, n_entries)
    if at is not None:
        raise PileupError("row_csr", at)
    at = _csr_offender(op_offsets, len(ops))
    if at is not None:
        raise PileupError("op_csr", at)

    depth = [0] * n_res
    counts = [[0] * A for _ in range(n_res)] if profile else []
    n_aln = [0] * n_seqs
    pair_total = 0
    for r in range(n_rows):
        if row_offsets[r] == row_offsets[r + 1]:
            events.add("row_without_entries")
        if row_mask is not None and not row_mask[r]:
            events.add("masked_row")
            continue
        for e in range(row_offsets[r], row_offsets[r + 1]):
            sid, oid = (qid[r], tid[r]) if on_q else (tid[r], qid[r])
            if sid >= n_seqs or (profile and oid >= n_other):
                offend("id", r)
                continue
            sb, se = offsets[sid], offsets[sid + 1]
            ob, oe = (other_off[oid], other_off[oid + 1]) if profile else (0, 0)
            if sb > se or se > n_res or ob > oe or (profile and oe > n_other_res):
                offend("seq", e)
                continue
            mine = [(v >> 4, v & 15) for v in ops[op_offsets[e]:op_offsets[e + 1]]]
            if any(c not in OPS or (c == N and reads_q) for _, c in mine):
                offend("op", e)
                continue
            takes_q = sum(n for n, c in mine if c in PAIR or c == I)
            takes_t = sum(n for n, c in mine if c in PAIR or c == D)
            takes_s, takes_o = (takes_q, takes_t) if on_q else (takes_t, takes_q)
            if start[e] + takes_s > se - sb or (profile and other_start[e] + takes_o > oe - ob):
                offend("extent", e)
                continue
            p, o = start[e], other_start[e] if profile else 0
            any_pair, in_run = False, False
            for n, c in mine:
                if c in PAIR:
                    if in_run:
                        events.add("run_merged")
                    if n and not in_run and p == 0 and sb > 0:
                        events.add("begins_at_next_sequence_start")
                    for _ in range(n):  # one pair column
                        depth[sb + p] += 1
                        if profile:
                            counts[sb + p][res_class(other_res[ob + o])] += 1
                        p += 1; o += 1
                        any_pair = True
                        pair_total += 1
                    if n and sb + p == se:
                        events.add("ends_at_sequence_end")
                    in_run = True
                    continue
                in_run = False
                if c == N:
                    events.add("N_op")  # (nothing on the target; the query side is not read)
                elif (c == I) == on_q:
                    events.add("I_on_query_side" if on_q else "D_on_target_side")
                    p += n
                else:
                    o += n
            n_aln[sid] += int(any_pair)
    for kind in KINDS:
        if kind in bad:
            raise PileupError(kind, bad[kind])

    length, covered, max_depth, depth_sum = [], [], [], []
    for s in range(n_seqs):
        b, e = offsets[s], offsets[s + 1]
        if b > e or e > n_res:
            raise PileupError("offsets", s)
        mine = depth[b:e]
        if not mine:
            events.add("empty_sequence")
        length.append(e - b); covered.append(sum(1 for d in mine if d)); max_depth.append(max(mine, default=0)); depth_sum.append(sum(mine))
    if any(d > 255 for d in depth):
        events.add("depth_over_255")
    assert sum(depth_sum) == pair_total == sum(depth)
    assert all(sum(c) == d for c, d in zip(counts, depth))
    with np.errstate(invalid="ignore", divide="ignore"):
        breadth = np.array(covered, np.uint32) / np.array(length, np.uint32)
        mean_depth = np.array(depth_sum, np.uint64) / np.array(length, np.uint32)
    flat = [v for c in counts for v in c]
    cols = (depth, flat, length, n_aln, covered, max_depth, depth_sum, breadth, mean_depth)
    return tuple(np.array(c, d) for c, d in zip(cols, DTYPES)), events


def assert_same(got, want, what=""):
    assert len(got) == len(want) == len(NAMES)
    for n, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype, f"{what}: {n} is {g.dtype}, expected {w.dtype}"
        assert g.shape == w.shape, f"{what}: {n} has {g.shape}, expected {w.shape}"
        if g.dtype == np.float64:  # bit for bit, but for which NaN it is
            same = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        else:
            same = g == w
        if not same.all():
            at = np.flatnonzero(~same)[:8]
            raise AssertionError(f"{what}: {n} differs at {at.tolist()}: got {g[at].tolist()}, expected {w[at].tolist()}")
