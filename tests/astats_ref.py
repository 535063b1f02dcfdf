"""Plain-loop reference of the alignment statistics (include/kmerseek_amd.h, "alignment statistics"): the residue classes and
their counts, the score histogram of a pair in Python integers, the regular-row tests, the Horner bisection in f64 exactly as the
contract states it, the ungapped Karlin-Altschul parameters with the K series, and the f64 formulas of the derived columns.
Nothing here imports the library."""
import math

import numpy as np

A = 28
STD_LETTERS = b"ACDEFGHIKLMNPQRSTVWY"
ROW_REGULAR, ROW_FALLBACK, ROW_SKIPPED = 0, 1, 2
MAX_SEQ_LEN = 1 << 20


def residue_class(byte: int) -> int:
    c = byte - 32 if 97 <= byte <= 122 else byte
    if 65 <= c <= 90:
        return c - 65
    return 26 if c == 42 else 27


CLASS_TABLE = np.array([residue_class(b) for b in range(256)], dtype=np.int64)
STD = [residue_class(b) for b in STD_LETTERS]


def pm1_matrix() -> np.ndarray:
    m = -np.ones((A, A), dtype=np.int8)
    np.fill_diagonal(m, 1)
    return m


def composition(res: np.ndarray, offs: np.ndarray):
    """(counts [n, 28], totals [28], length [n]) of a batch, by numpy.bincount of the class table."""
    n = len(offs) - 1
    counts = np.zeros((n, A), dtype=np.int64)
    for s in range(n):
        seq = np.asarray(res[int(offs[s]):int(offs[s + 1])], dtype=np.uint8)
        counts[s] = np.bincount(CLASS_TABLE[seq], minlength=A)
    length = np.diff(np.asarray(offs, dtype=np.int64))
    return counts, counts.sum(axis=0), length


def score_range(matrix):
    """(smin, smax) over the standard 20 x 20 block."""
    m = pm1_matrix() if matrix is None else np.asarray(matrix)
    vals = [int(m[i, j]) for i in STD for j in STD]
    return min(vals), max(vals)


def pair_histogram(matrix, cq, ct):
    """{score: h_s} in Python integers; cq, ct: the 28 class counts of the two sequences."""
    m = pm1_matrix() if matrix is None else np.asarray(matrix)
    h = {}
    for i in STD:
        a = int(cq[i])
        if a == 0:
            continue
        for j in STD:
            v = a * int(ct[j])
            if v:
                s = int(m[i, j])
                h[s] = h.get(s, 0) + v
    return h


def is_regular(h) -> bool:
    n = sum(h.values())
    return n > 0 and sum(s * v for s, v in h.items()) < 0 and any(s > 0 and v > 0 for s, v in h.items())


def coefficients(h, smin, smax):
    """Integer coefficients by power 0 .. d of f(x) = sum h_s x^(smax - s) - N x^smax, combined per power."""
    d = smax - smin
    c = [0] * (d + 1)
    for s, v in h.items():
        c[smax - s] += v
    c[smax] -= sum(h.values())
    return c


def horner(cf, x: float) -> float:
    """f at x from the highest power down, one f64 rounding per operation (Python floats: no contraction)."""
    v = cf[-1]
    for k in range(len(cf) - 2, -1, -1):
        v = v * x + cf[k]
    return v


def bisect_root(c) -> float:
    cf = [float(v) for v in c]
    lo, hi = 0.0, 1.0
    for _ in range(128):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if horner(cf, mid) > 0.0:
            lo = mid
        else:
            hi = mid
    return lo


def row_root(matrix, cq, ct, smin, smax):
    """(status, x) of one hit row."""
    h = pair_histogram(matrix, cq, ct)
    if not is_regular(h):
        return ROW_FALLBACK, 0.0
    return ROW_REGULAR, bisect_root(coefficients(h, smin, smax))


def std_freq(w):
    f = [float(w[i]) for i in STD]
    if any(not (v >= 0.0) or math.isinf(v) for v in f) or not sum(f) > 0.0:
        raise ValueError("weights")
    t = sum(f)
    return [v / t for v in f]


def score_probs(matrix, freq_q, freq_t):
    m = pm1_matrix() if matrix is None else np.asarray(matrix)
    fq, ft = std_freq(freq_q), std_freq(freq_t)
    p = {}
    for a, i in enumerate(STD):
        for b, j in enumerate(STD):
            s = int(m[i, j])
            p[s] = p.get(s, 0.0) + fq[a] * ft[b]
    return {s: v for s, v in p.items() if v > 0.0}


def karlin_ungapped(matrix, freq_q, freq_t, max_terms=400, want_K=True):
    """(lambda, K, H, terms) — the series of Karlin & Altschul 1990 as the header restates it.  ValueError where the library
    answers KS_ERR_INVALID_ARG.  want_K=False: no series is summed (K = 0.0, terms = 0), as where the library is given no K."""
    p = score_probs(matrix, freq_q, freq_t)
    if not p or max(p) <= 0:
        raise ValueError("no positive score has positive probability")
    if not sum(s * v for s, v in p.items()) < 0.0:
        raise ValueError("the expected score is not negative")

    def phi(lam):
        return sum(v * math.exp(lam * s) for s, v in p.items()) - 1.0

    up = 0.5
    while not phi(up) > 0.0:
        up *= 2.0
    a, b = 0.0, up
    for _ in range(200):
        mid = 0.5 * (a + b)
        if mid == a or mid == b:
            break
        if phi(mid) > 0.0:
            b = mid
        else:
            a = mid
    lam = b
    for _ in range(2):
        lam -= phi(lam) / sum(s * v * math.exp(lam * s) for s, v in p.items())
    hs = sum(s * v * math.exp(lam * s) for s, v in p.items())
    H = lam * hs
    if not want_K:
        return lam, 0.0, H, 0
    delta = 0
    for s in p:
        delta = math.gcd(delta, abs(s))
    q = {s // delta: v for s, v in p.items()}
    lp = lam * delta
    pk = dict(q)
    sigma, terms = 0.0, 0
    for k in range(1, max_terms + 1):
        if k > 1:
            nxt = {}
            for j, v in pk.items():
                for s, w in q.items():
                    nxt[j + s] = nxt.get(j + s, 0.0) + v * w
            pk = nxt
        term = (sum(v * math.exp(lp * j) for j, v in pk.items() if j < 0) + sum(v for j, v in pk.items() if j >= 0)) / k
        sigma += term
        terms = k
        if term < 2.0 ** -60:
            break
    else:
        raise ValueError("expected score too close to zero")
    K = -math.exp(-2.0 * sigma) / ((H / lp) * math.expm1(-lp))
    return lam, K, H, terms


def sat_n_eff(db_residues: int, db_seqs: int, length_adjust: int) -> int:
    off = min(db_seqs * length_adjust, 2 ** 64 - 1)
    return max(db_residues - off, 1)


def stats(scores, row_offsets, qid, tid, q_counts, q_len, t_counts, t_len, matrix=None, params=None, background=None,
          composition_based=True, pairwise=False, ratio=(0.5, 1.0), db_residues=0, db_seqs=0, length_adjust=0, x_of=None):
    """The whole pass.  scores: i64 [n]; row_offsets: [n_rows + 1] or None (one score per row).  x_of: the (status, x) per row
    to derive the f64 columns from (the library's own, so that the derived columns are compared on the same x); None: computed.
    Returns a dict of the result columns and scalars."""
    n_rows = len(qid)
    smin, smax = score_range(matrix)
    bg = background if background is not None else np.asarray(t_counts).sum(axis=0)
    lam_std = k_std = 0.0
    if composition_based or params is None:
        lam_std, k_std, _, _ = karlin_ungapped(matrix, bg, bg, want_K=params is None)
    lam_c, k_c = params if params is not None else (lam_std, k_std)
    dbr = db_residues or int(np.asarray(t_len, dtype=np.int64).sum())
    dbs = db_seqs or len(t_len)
    n_eff_db = sat_n_eff(dbr, dbs, length_adjust)
    status = np.zeros(n_rows, np.uint8)
    x = np.zeros(n_rows)
    rho = np.ones(n_rows)
    n = len(scores)
    bit = np.zeros(n)
    ev = np.zeros(n)
    row_bit = np.full(n_rows, np.nan)
    row_ev = np.full(n_rows, np.nan)
    ln_k, ln_2 = math.log(k_c), math.log(2.0)
    for r in range(n_rows):
        q, t = int(qid[r]), int(tid[r])
        if not composition_based:
            status[r], x[r] = ROW_SKIPPED, 0.0
        else:
            status[r], x[r] = x_of[r] if x_of is not None else row_root(matrix, q_counts[q], t_counts[t], smin, smax)
            if status[r] == ROW_REGULAR:
                lam_r = -math.log(x[r]) if x[r] > 0.0 else math.inf
                rho[r] = min(max(lam_r / lam_std, ratio[0]), ratio[1])
        m_eff = max(int(q_len[q]) - length_adjust, 1)
        n_eff = max(int(t_len[t]) - length_adjust, 1) if pairwise else n_eff_db
        b, e = (r, r + 1) if row_offsets is None else (int(row_offsets[r]), int(row_offsets[r + 1]))
        for i in range(b, e):
            sp = rho[r] * float(int(scores[i]))
            bit[i] = (lam_c * sp - ln_k) / ln_2
            arg = -(lam_c * sp)
            ev[i] = (k_c * float(n_eff)) * float(m_eff) * (math.exp(arg) if arg < 709.0 else math.inf)
        if e > b:
            row_bit[r] = bit[b:e].max()
            row_ev[r] = ev[b:e].min()
    return dict(status=status, x=x, lambda_ratio=rho, bit_score=bit, evalue=ev, row_bit_score=row_bit, row_evalue=row_ev,
                lambda_std=lam_std, lambda_used=lam_c, K_used=k_c, params_source=0 if params is None else 1,
                n_fallback=int((status == ROW_FALLBACK).sum()))
