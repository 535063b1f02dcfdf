"""The cases of the alignment-statistics tests, shared by tests/test_astats_cpu.py and tests/test_gpu_astats.py: matrices,
random hit rows of two small batches, the crafted fallback rows and the one row of two 2^20-residue sequences under a matrix
that spans -128 .. 127.  Everything is seeded; the reference results are computed once per process (rows_reference)."""
import functools

import numpy as np

import astats_ref as R

LETTERS = np.frombuffer(R.STD_LETTERS, dtype=np.uint8)


def matrix_pm(match: int, mismatch: int) -> np.ndarray:
    m = np.full((R.A, R.A), mismatch, dtype=np.int8)
    np.fill_diagonal(m, match)
    return m


def matrix_random(seed: int = 11, lo: int = -4, hi: int = 2) -> np.ndarray:
    """Symmetric, diagonal 4 .. 11, off-diagonal lo .. hi."""
    rng = np.random.default_rng(seed)
    m = rng.integers(lo, hi + 1, (R.A, R.A))
    m = np.triu(m, 1)
    m = m + m.T
    m[np.arange(R.A), np.arange(R.A)] = rng.integers(4, 12, R.A)
    return m.astype(np.int8)


def matrix_wide() -> np.ndarray:
    """Standard block from -128 to 127 with many distinct scores between: the degree-255 polynomial."""
    m = np.full((R.A, R.A), -100, dtype=np.int64)
    for a, i in enumerate(R.STD):
        for b, j in enumerate(R.STD):
            m[i, j] = 127 - 5 * (a % 4) if a == b else -128 + 6 * ((3 * a + 7 * b) % 20)
    return m.astype(np.int8)


MATRICES = {"pm1": None, "p5m4": matrix_pm(5, -4), "random": matrix_random()}


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    res = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if seqs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(res, dtype=np.uint8), offs


@functools.lru_cache(maxsize=None)
def random_batches(seed: int = 5, n_q: int = 12, n_t: int = 40, n_rows: int = 200):
    """(q_res, q_off, t_res, t_off, qid, tid): sequences of 30 .. 400 residues over the 20 letters, each with a composition of
    its own (a Dirichlet draw), and n_rows distinct (q, t) pairs in (q, t) order — the order of a hit list."""
    rng = np.random.default_rng(seed)

    def seqs(n):
        out = []
        for _ in range(n):
            p = rng.dirichlet(np.full(20, 3.0))
            out.append(LETTERS[rng.choice(20, size=int(rng.integers(30, 401)), p=p)])
        return out
    q, t = seqs(n_q), seqs(n_t)
    flat = np.sort(rng.choice(n_q * n_t, size=n_rows, replace=False))
    qid, tid = (flat // n_t).astype(np.uint32), (flat % n_t).astype(np.uint32)
    return (*pack(q), *pack(t), qid, tid)


def fallback_batches():
    """Rows that are not regular, each for a reason of its own (under every matrix of MATRICES and any positive-diagonal one):
    0 poly-W x poly-W: only a positive score occurs;  1 only X, * and B x a normal sequence: N = 0;  2 an empty sequence;
    3 expected score exactly 0 under +1 / -1: A x (A, C) halves — one match for every mismatch."""
    q = [np.full(50, ord("W"), np.uint8), np.frombuffer(b"XX**BBxb" * 5, np.uint8), np.zeros(0, np.uint8), np.full(40, ord("A"), np.uint8)]
    t = [np.full(70, ord("W"), np.uint8), LETTERS[np.arange(60) % 20], LETTERS[np.arange(45) % 20],
         np.frombuffer(b"AC" * 30, np.uint8)]
    qid = np.arange(4, dtype=np.uint32)
    tid = np.arange(4, dtype=np.uint32)
    return (*pack(q), *pack(t), qid, tid)


@functools.lru_cache(maxsize=None)
def wide_counts(seed: int = 9):
    """The 28 class counts of two sequences of 2^20 residues over the 20 letters (N = 2^40)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        c = np.zeros(R.A, dtype=np.int64)
        c[R.STD] = rng.multinomial(R.MAX_SEQ_LEN, rng.dirichlet(np.full(20, 5.0)))
        out.append(c)
    return out


def wide_sequence(counts) -> np.ndarray:
    """A sequence with exactly these class counts (the letters in runs)."""
    return np.repeat(np.arange(R.A, dtype=np.uint8) + 65, np.asarray(counts))


@functools.lru_cache(maxsize=None)
def rows_reference(name: str):
    """(status u8 [n_rows], x f64 [n_rows]) of the random rows under MATRICES[name], by the reference loop."""
    q_res, q_off, t_res, t_off, qid, tid = random_batches()
    cq, _, _ = R.composition(q_res, q_off)
    ct, _, _ = R.composition(t_res, t_off)
    smin, smax = R.score_range(MATRICES[name])
    got = [R.row_root(MATRICES[name], cq[int(q)], ct[int(t)], smin, smax) for q, t in zip(qid, tid)]
    return np.array([g[0] for g in got], np.uint8), np.array([g[1] for g in got], np.float64)
