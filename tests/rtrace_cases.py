"""The fixed inputs the traceback tests share: test_region_trace_cpu.py establishes on the reference alone that they exercise
every branch of the walk, test_gpu_region_trace.py runs the device on the same bytes.  Not a test module."""
import numpy as np

PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
CORE = b"ACDEFGHIKLPQ"
HUGE = 2 ** 20  # the largest x_drop: an extension never stops early


def two_letter_batch(seed, n_q, n_t, lo, hi):
    rng = np.random.default_rng(seed)
    seq = lambda: bytes(np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, int(rng.integers(lo, hi + 1)))])
    return [seq() for _ in range(n_q)], [seq() for _ in range(n_t)]


# +1 / -1 over {A, C}, k = 6: nearly every maximum is attained more than once
FUZZ_K = 6
FUZZ_OPTS = ({"band": 1, "x_drop": 1}, {"band": 5, "x_drop": HUGE}, {"band": 31, "x_drop": 4})


def fuzz_batch(gap_open, gap_extend):
    return two_letter_batch(11 + 2 * gap_open + gap_extend, 3, 3, 20, 60)


def indel_batch(W, seed):
    """One query; per (side, kind, L) a target that equals it but for L residues inserted into / deleted from the flank 20
    residues away from CORE.  Flanks of 90 random residues: bridging a gap pays.  -> (queries, targets, cases)."""
    rng = np.random.default_rng(seed)
    seq = lambda n: bytes(PROTEIN[rng.integers(0, 20, n)])
    left, right = seq(90), seq(90)
    cases, targets = [], []
    for side in (1, -1):
        for kind in ("ins", "del"):
            for L in sorted({1, W, W + 1}):
                if side > 0:
                    fl = right[:20] + (seq(L) + right[20:] if kind == "ins" else right[20 + L:])
                    targets.append(left + CORE + fl)
                else:
                    fl = (left[:70] + seq(L) if kind == "ins" else left[:70 - L]) + left[70:]
                    targets.append(fl + CORE + right)
                cases.append((side, kind, L))
    return [left + CORE + right], targets, cases


INDEL_K = 7
INDEL_BANDS = (1, 16, 31)
INDEL_OPTS = {"gap_open": 5, "gap_extend": 1, "x_drop": HUGE}


def k1_batch():
    """k = 1 over {A, C}: every maximal run of equal residue pairs on a diagonal is a seed — a quarter of them of length 1, whose
    anchor has no seed residue beside it — and 90 x 110 residues give thousands of them in one row; sequences of one residue."""
    rng = np.random.default_rng(5)
    two = lambda n: bytes(np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, n)])
    return [two(90), b"AC" * 3 + b"A", two(1)], [b"CACCA", two(110), b"A", b"C"]


K1_OPTS = ({"band": 2, "gap_open": 1, "gap_extend": 1, "x_drop": 2}, {"band": 5, "gap_open": 0, "gap_extend": 1, "x_drop": 0})
