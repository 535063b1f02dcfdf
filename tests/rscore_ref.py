"""CPU restatement of ks_regions_score for the tests (include/kmerseek_amd.h: region scores): plain Python loops over bytes
and integers, one position at a time.  Shares no code with the library.  Not a test module."""
import numpy as np

ALPHABET = 28
COLUMNS = ("row_offsets", "q_start", "t_start", "length", "score", "identities", "positives", "core_identities")


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


def extend(pairs, matrix, x_drop):
    """pairs: the (query byte, target byte) pairs j = 1, 2, ... walking away from the core.  -> (ext, score, identities, positives):
    the smallest j in [0, J] whose prefix sum is the largest seen up to J, that sum, and the counts over the first ext pairs.  J: the
    first j at which the sum lies more than x_drop below the best so far, or the last pair."""
    s_run, best, best_j = 0, 0, 0
    ident, pos, ident_best, pos_best = 0, 0, 0, 0
    for j, (cq, ct) in enumerate(pairs, 1):
        s = int(matrix[residue_class(cq)][residue_class(ct)])
        s_run += s
        ident += 1 if upper(cq) == upper(ct) else 0
        pos += 1 if s > 0 else 0
        if s_run > best:  # strictly: the shortest extension wins a tie
            best, best_j, ident_best, pos_best = s_run, j, ident, pos
        if best - s_run > x_drop:
            break
    return best_j, best, ident_best, pos_best


def score_region(qseq, tseq, a, b, n, matrix, do_extend, x_drop):
    """One region [a, a + n) x [b, b + n) of the sequences qseq / tseq (bytes) -> the seven output values."""
    assert a + n <= len(qseq) and b + n <= len(tseq)
    core = core_ident = core_pos = 0
    for i in range(n):
        cq, ct = qseq[a + i], tseq[b + i]
        s = int(matrix[residue_class(cq)][residue_class(ct)])
        core += s
        core_ident += 1 if upper(cq) == upper(ct) else 0
        core_pos += 1 if s > 0 else 0
    left = right = (0, 0, 0, 0)
    if do_extend:
        e_r = min(len(qseq) - (a + n), len(tseq) - (b + n))
        right = extend([(qseq[a + n + j - 1], tseq[b + n + j - 1]) for j in range(1, e_r + 1)], matrix, x_drop)
        left = extend([(qseq[a - j], tseq[b - j]) for j in range(1, min(a, b) + 1)], matrix, x_drop)
    return (a - left[0], b - left[0], left[0] + n + right[0], left[1] + core + right[1], left[2] + core_ident + right[2],
            left[3] + core_pos + right[3], core_ident)


def score(regions, qid, tid, q_res, q_off, t_res, t_off, matrix=None, extend=False, x_drop=0):
    """regions: (row_offsets, q_start, t_start, length, ...) as Regions.to_host() / regions_ref.chain; hit row r = (qid[r], tid[r]).
    -> the eight columns of RegionScores.to_host()."""
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in np.asarray(matrix).tolist()]
    offs = [int(v) for v in regions[0]]
    qs, ts, ln = [np.asarray(c).tolist() for c in regions[1:4]]
    q_bytes, t_bytes = bytes(np.asarray(q_res, np.uint8)), bytes(np.asarray(t_res, np.uint8))
    rows = []
    for r in range(len(offs) - 1):
        q, t = int(qid[r]), int(tid[r])
        qseq = q_bytes[int(q_off[q]):int(q_off[q + 1])]
        tseq = t_bytes[int(t_off[t]):int(t_off[t + 1])]
        for g in range(offs[r], offs[r + 1]):
            rows.append(score_region(qseq, tseq, qs[g], ts[g], ln[g], m, extend, x_drop))
    cols = list(zip(*rows)) if rows else [[] for _ in range(7)]
    dt = (np.uint32, np.uint32, np.uint32, np.int64, np.uint32, np.uint32, np.uint32)
    return (np.asarray(regions[0], np.uint64).copy(), *[np.asarray(c, d) for c, d in zip(cols, dt)])
