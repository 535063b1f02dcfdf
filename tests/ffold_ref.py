"""CPU restatement of ks_frames_fold_device (include/kmerseek_amd.h): the hit rows of a search whose queries are the six frames of
every nucleotide record, folded into one row per (record, strand, target), and their regions on the strand's bases.  Plain Python
loops, written from the header, with no code shared with the library: the GPU test holds every column against this."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_LEN = 2 ** 32 - 16
U32 = 2 ** 32 - 1
NAMES = ("src_row", "row_offsets", "src_region", "frame", "nt_length", "s_start", "nt_start", "t_start3", "t_length3", "score",
         "identities", "aln_length")
DTYPES = (np.uint32, np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32)


class FoldError(ValueError):
    """what the fold refuses: `kind` is one of offsets, long, qid, order, csr, qend, tend; `index` the first offending record,
    row or region"""

    def __init__(self, kind, index):
        super().__init__(f"{kind} at {index}")
        self.kind, self.index = kind, index


def frame_len(n_bases, f):
    return max(0, (n_bases - f) // 3)


def check(qid, tid, nt_offsets, row_offsets, q_start, q_length, t_start, t_length):
    """raises the FoldError the header promises, the kinds in the order the header lists them"""
    n_rec, n_rows, n = len(nt_offsets) - 1, len(qid), len(q_start)
    bad = [s for s in range(n_rec) if nt_offsets[s + 1] < nt_offsets[s] or (s == 0 and nt_offsets[0] != 0)]
    if bad:
        raise FoldError("offsets", bad[0])
    bad = [s for s in range(n_rec) if nt_offsets[s + 1] - nt_offsets[s] > MAX_LEN]
    if bad:
        raise FoldError("long", bad[0])
    bad = [r for r in range(n_rows) if qid[r] >= 6 * n_rec]
    if bad:
        raise FoldError("qid", bad[0])
    bad = [r for r in range(1, n_rows) if (qid[r - 1], tid[r - 1]) >= (qid[r], tid[r])]
    if bad:
        raise FoldError("order", bad[0])
    bad = [r for r in range(n_rows) if (r == 0 and row_offsets[0] != 0) or row_offsets[r] > row_offsets[r + 1] or row_offsets[r + 1] > n or
           (r == n_rows - 1 and row_offsets[r + 1] != n)]
    if bad:
        raise FoldError("csr", bad[0])
    qend, tend = [], []
    for r in range(n_rows):
        s, f = qid[r] // 6, qid[r] % 3
        flen = frame_len(nt_offsets[s + 1] - nt_offsets[s], f)
        for g in range(row_offsets[r], row_offsets[r + 1]):
            if q_start[g] + q_length[g] > flen:
                qend.append(g)
            if 3 * (t_start[g] + t_length[g]) > U32:
                tend.append(g)
    if qend:
        raise FoldError("qend", min(qend))
    if tend:
        raise FoldError("tend", min(tend))


def fold(qid, tid, intersect, n_weighted, nt_offsets, row_offsets, q_start, q_length, t_start, t_length=None, score=None, identities=None,
         aln_length=None):
    """-> (hits, cols): hits = (qid', tid, intersect, n_weighted) of the folded rows, cols = the twelve ks_ffold columns in the
    order of ks_ffold_copy_to_host (NAMES); a pass-through column that was not given comes back as None"""
    ints = lambda a: [int(x) for x in (a.tolist() if isinstance(a, np.ndarray) else a)]  # noqa: E731  (no detour through f64)
    qid, tid, intersect, n_weighted, nt_offsets, row_offsets = map(ints, (qid, tid, intersect, n_weighted, nt_offsets, row_offsets))
    q_start, q_length, t_start = map(ints, (q_start, q_length, t_start))
    t_length = q_length if t_length is None else ints(t_length)
    extra = [None if c is None else ints(c) for c in (score, identities, aln_length)]
    check(qid, tid, nt_offsets, row_offsets, q_start, q_length, t_start, t_length)
    groups = {}  # (2 s + strand, tid) -> {frame inside the strand: input row}
    for r in range(len(qid)):
        groups.setdefault((qid[r] // 3, tid[r]), {})[qid[r] % 3] = r
    hits = [[], [], [], []]
    out = {k: [] for k in NAMES}
    out["row_offsets"].append(0)
    for x, t in sorted(groups):
        members = groups[(x, t)]
        hits[0].append(x); hits[1].append(t)
        hits[2].append(min(U32, sum(intersect[r] for r in members.values())))
        hits[3].append(sum(n_weighted[r] for r in members.values()) % 2 ** 64)
        for j in range(3):
            r = members.get(j, NONE)
            out["src_row"].append(r)
            if r == NONE:
                continue
            s, f6, f = qid[r] // 6, qid[r] % 6, qid[r] % 3
            L = nt_offsets[s + 1] - nt_offsets[s]
            for g in range(row_offsets[r], row_offsets[r + 1]):
                s_start = f + 3 * q_start[g]
                out["src_region"].append(g); out["frame"].append(f6); out["nt_length"].append(3 * q_length[g]); out["s_start"].append(s_start)
                out["nt_start"].append(s_start if f6 < 3 else L - f - 3 * (q_start[g] + q_length[g]))
                out["t_start3"].append(3 * t_start[g]); out["t_length3"].append(3 * t_length[g])
                for name, col in zip(("score", "identities", "aln_length"), extra):
                    if col is not None:
                        out[name].append(col[g])
        out["row_offsets"].append(len(out["src_region"]))
    cols = tuple(None if (n in ("score", "identities", "aln_length") and extra[("score", "identities", "aln_length").index(n)] is None)
                 else np.array(out[n], d) for n, d in zip(NAMES, DTYPES))
    return (np.array(hits[0], np.uint32), np.array(hits[1], np.uint32), np.array(hits[2], np.uint32), np.array(hits[3], np.uint64)), cols


def assert_same(got_hits, got_cols, want_hits, want_cols, what=""):
    """exact equality of the folded hit list and of every column; a column the reference does not have is not compared"""
    for n, g, w in zip(("qid", "tid", "intersect", "n_weighted"), got_hits, want_hits):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: folded hits {n}: got {g[:16].tolist()}, expected {w[:16].tolist()}"
    assert len(got_cols) == len(want_cols) == len(NAMES)
    for n, g, w in zip(NAMES, got_cols, want_cols):
        if w is None:
            continue
        g = np.asarray(g)
        assert g.dtype == w.dtype, f"{what}: {n} is {g.dtype}, expected {w.dtype}"
        assert g.shape == w.shape, f"{what}: {n} has {g.shape}, expected {w.shape}"
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)[:8]
            raise AssertionError(f"{what}: {n} differs at {at.tolist()}: got {g[at].tolist()}, expected {w[at].tolist()}")
