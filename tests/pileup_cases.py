"""Inputs of the pileup tests, built from the CPU references alone.  Not a test module.

A CASE is a dict: q, t (each (res u8, off u64): the two batches), qid, tid (the hit rows), row_offsets (u64[n_rows + 1], or None:
one entry per row), op_offsets, ops, q_start, t_start (per entry) and row_mask (u8 per row, or None).  ref_args(case, side,
profile) are the arguments tests/pileup_ref.py takes for it.

build          hand-written rows [(qid, tid, [(q_start, t_start, "cigar"), ...])] -> a case
WORKED         the worked examples of the header with the depth written down
fuzz_batch     about 2,000 entries on 300 sequences of 0 .. 700 residues a side, by seed
gpu_cases      all of them by name, with the sides and profile settings each runs under
from_rstitch / from_fstitch   the CIGARs tests/rstitch_cases.py and tests/fstitch_cases.py produce on the CPU: the traced regions
               (entries through the alignments' CSR), the stitched rows and the frame alignments"""
import functools

import numpy as np

import pileup_ref as PR

ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdxBZUO*-X", np.uint8)  # every class kind: both cases, '*', bytes of class 27


def pack(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), off


def build(rows, q_seqs, t_seqs, one_per_row=False, row_mask=None):
    qid, tid, row_off, op_off, ops, qs, ts = [], [], [0], [0], [], [], []
    for q, t, entries in rows:
        qid.append(q); tid.append(t)
        assert not one_per_row or len(entries) == 1
        for a, b, cigar in entries:
            qs.append(a); ts.append(b)
            ops += PR.parse(cigar) if isinstance(cigar, str) else list(cigar)
            op_off.append(len(ops))
        row_off.append(len(qs))
    u32 = lambda a: np.array(a, np.uint32)  # noqa: E731
    return dict(q=pack(q_seqs), t=pack(t_seqs), qid=u32(qid), tid=u32(tid), row_offsets=None if one_per_row else np.array(row_off, np.uint64),
                op_offsets=np.array(op_off, np.uint64), ops=u32(ops), q_start=u32(qs), t_start=u32(ts),
                row_mask=None if row_mask is None else np.array(row_mask, np.uint8))


def ref_args(case, side, profile):
    on_q = side == "query"
    s, o = ("q", "t") if on_q else ("t", "q")
    return dict(row_offsets=case["row_offsets"], op_offsets=case["op_offsets"], ops=case["ops"], start=case[s + "_start"],
                other_start=case[o + "_start"] if profile else None, row_mask=case["row_mask"], qid=case["qid"], tid=case["tid"],
                offsets=case[s][1], side=side, profile=profile, other_res=case[o][0] if profile else None, other_off=case[o][1] if profile else None)


def reference(case, side, profile):
    return PR.pileup(**ref_args(case, side, profile))


# ---- the worked examples of the header: (name, cigar, query length, target length, depth on the query side, on the target side) ----
WORKED = [
    ("2M1I2M", "2M1I2M", 5, 4, [1, 1, 0, 1, 1], [1, 1, 1, 1]),
    ("2M1D2M", "2M1D2M", 4, 5, [1, 1, 1, 1], [1, 1, 0, 1, 1]),
    ("41M1N59M", "41M1N59M", None, 100, None, [1] * 100),  # (the query side of an N is not asked for)
    ("eqx_run", "2=1X1=1I1X", 6, 5, [1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1]),
    ("empty_op", "2M0M0D1M", 3, 3, [1, 1, 1], [1, 1, 1]),
]


def worked_case(name):
    _, cigar, nq, nt, _, _ = next(w for w in WORKED if w[0] == name)
    return build([(0, 0, [(0, 0, cigar)])], [b"ACDEFGHIKL"[:nq or 0] if (nq or 0) <= 10 else b"A" * nq], [(b"KLMNPQRSTV" * 10)[:nt]], one_per_row=True)


# ---- hand-written shapes the GPU test names ------------------------------------------------------------------------------------
def boundary_case(to_the_end=False):
    """three targets of 5, 0 and 7 residues and three queries alike: an entry 3M at position 0 of the first, one ending on the last
    residue of the first while another begins on the first of the third (the empty one lies between); the second sequence is empty
    and nothing touches the fourth."""
    seqs = [b"ACDEF", b"", b"GHIKLMN", b"PQRST"]
    rows = [(0, 0, [(0, 0, "3M"), (2, 2, "3M")]), (2, 2, [(0, 0, "2M"), (3, 3, "4M")]), (2, 0, [(5, 4, "1M")])]
    if to_the_end:  # ... and one ending on the last residue of the last sequence: its end lies at n_res
        rows.append((3, 3, [(1, 1, "4M")]))
    return build(rows, seqs, seqs)


def lane_tail_case():
    """pair ops of 1, 63, 64, 65, 129 and 700 columns, one entry each, with an I and a D between two of them"""
    lens = (1, 63, 64, 65, 129, 700)
    rng = np.random.default_rng(17)
    seq = lambda n: bytes(ALPHABET[rng.integers(0, len(ALPHABET), n)])  # noqa: E731
    qs, ts = [seq(n + 9) for n in lens], [seq(n + 11) for n in lens]
    rows = [(i, i, [(2, 3, f"{n}M")]) for i, n in enumerate(lens)]
    rows.append((5, 0, [(0, 0, "1M")]))
    rows.sort()
    rows[2][2].append((1, 2, "30=2I4D34X"))
    return build(rows, qs, ts)


def alternating_case(n=300):
    """one entry of n alternating 1= 1X ops (one run), one of 150 x (1M 1I 1M 1D): 300 runs"""
    rows = [(0, 0, [(3, 5, "1=1X" * (n // 2))]), (1, 1, [(0, 0, "1M1I1M1D" * 150)])]
    seqs = [bytes(ALPHABET[np.arange(700) % len(ALPHABET)])] * 2
    return build(rows, seqs, seqs)


def csr_rows(one_per_row):
    """rows of 0, 1, 2 and 9 entries through the CSR — or the same entries as one row each"""
    rng = np.random.default_rng(23)
    seq = lambda n: bytes(ALPHABET[rng.integers(0, len(ALPHABET), n)])  # noqa: E731
    qs, ts = [seq(60) for _ in range(4)], [seq(80) for _ in range(5)]
    per_row = [((0, 1), 0), ((1, 0), 1), ((1, 3), 2), ((2, 2), 9), ((3, 4), 0), ((3, 4), 1)]  # (a row without entries at either end of a query)
    rows = []
    for (q, t), n in per_row:
        entries = [(int(rng.integers(0, 20)), int(rng.integers(0, 30)), f"{int(rng.integers(1, 20))}M{int(rng.integers(1, 5))}I{int(rng.integers(1, 15))}M")
                   for _ in range(n)]
        if one_per_row:
            rows += [(q, t, [e]) for e in entries]
        else:
            rows.append((q, t, entries))
    return build(rows, qs, ts, one_per_row=one_per_row)


def contention_case(n=5000):
    """n entries over the same 40 residues of one target, from 50 queries: depth n"""
    rng = np.random.default_rng(31)
    qs = [bytes(ALPHABET[rng.integers(0, len(ALPHABET), 64)]) for _ in range(50)]
    ts = [b"A" * 10, bytes(ALPHABET[rng.integers(0, len(ALPHABET), 100)])]
    rows = [(q, 1, [(int(rng.integers(0, 20)), 30, "40M") for _ in range(n // 50)]) for q in range(50)]
    return build(rows, qs, ts)


# ---- the fuzz ------------------------------------------------------------------------------------------------------------------
def _random_ops(rng, room_q, room_t, with_n):
    """a CIGAR that fits room_q x room_t residues: -> (ops, query residues taken, target residues taken)"""
    ops, uq, ut = [], 0, 0
    for _ in range(int(rng.integers(1, 13))):
        kind = int(rng.integers(0, 12))
        n = int(rng.integers(1, 90)) if rng.random() < 0.3 else int(rng.integers(1, 9))
        if kind <= 6:
            n = min(n, room_q - uq, room_t - ut)
            code = (PR.M, PR.EQ, PR.X)[kind % 3]
            uq += n; ut += n
        elif kind <= 8:
            n = min(n, room_q - uq)
            code = PR.I
            uq += n
        elif kind <= 10:
            n = min(n, room_t - ut)
            code = PR.D
            ut += n
        elif with_n:
            n, code = int(rng.integers(1, 3)), PR.N
        else:
            continue
        if n > 0 or rng.random() < 0.05:  # (an op of length 0 now and then)
            ops.append((n << 4) | code)
    return ops, uq, ut


@functools.lru_cache(maxsize=None)
def fuzz_batch(seed=2024, n_seqs=300, n_rows=720, with_n=False):
    """n_seqs sequences of 0 .. 700 residues a side (every tenth empty), n_rows distinct hit rows in (qid, tid) order with 0 .. 9
    entries each (about 2,000 entries), a fifth of the rows masked out.  with_n: N ops too — a case for the target side alone."""
    rng = np.random.default_rng(seed)
    lens = lambda: [0 if i % 10 == 3 else int(rng.integers(1, 701)) for i in range(n_seqs)]  # noqa: E731
    mk = lambda L: [bytes(ALPHABET[rng.integers(0, len(ALPHABET), n)]) for n in L]  # noqa: E731
    qs, ts = mk(lens()), mk(lens())
    pairs = sorted({(int(a), int(b)) for a, b in rng.integers(0, n_seqs, (n_rows, 2))})
    rows = []
    for q, t in pairs:
        entries = []
        n = int(rng.choice([0, 1, 1, 2, 2, 3, 4, 9]))
        for _ in range(n):
            lq, lt = len(qs[q]), len(ts[t])
            a, b = int(rng.integers(0, lq + 1)), int(rng.integers(0, lt + 1))
            if rng.random() < 0.1:
                a, b = 0, 0
            ops, uq, ut = _random_ops(rng, lq - a, lt - b, with_n)
            if rng.random() < 0.2:  # flush with the ends of both sequences where the ops allow it
                a, b = lq - uq, lt - ut
            entries.append((a, b, ops))
        rows.append((q, t, entries))
    mask = (rng.random(len(rows)) >= 0.2).astype(np.uint8)
    return build(rows, qs, ts, row_mask=mask)


# ---- the CIGARs the stitch cases produce on the CPU ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def from_rstitch(eqx=False):
    """the pipe cases of tests/rstitch_cases.py as one batch -> (the traced regions as a case: entries through the alignments' CSR;
    the stitched rows as a case: one entry per row)"""
    import rstitch_cases as SC
    import rstitch_ref
    cases = SC.pipe_cases()
    opts = dict(band=16, gap_open=11, gap_extend=1, x_drop=30)
    P = SC.cpu_inputs([c[1] for c in cases], [c[2] for c in cases], eqx=eqx, **opts)
    al, cg, h = P["alignments"], P["cigars"], P["hits"]
    base = dict(q=P["q"], t=P["t"], qid=np.asarray(h[0], np.uint32), tid=np.asarray(h[1], np.uint32), row_mask=None)
    regions = dict(base, row_offsets=np.asarray(al[0], np.uint64), op_offsets=cg[0], ops=cg[1], q_start=np.asarray(al[1], np.uint32),
                   t_start=np.asarray(al[3], np.uint32))
    st, _ = rstitch_ref.stitch(P["chain"], al, cg, h[0], h[1], *P["q"], *P["t"], gap_open=11, gap_extend=1, eqx=eqx)
    stitched = dict(base, row_offsets=None, op_offsets=st[0], ops=st[1], q_start=st[2], t_start=st[4])
    return regions, stitched


@functools.lru_cache(maxsize=None)
def from_fstitch():
    """the worked examples of tests/fstitch_cases.py on the forward strand as one batch -> the frame alignments as a case for the
    target side (its query batch is empty: the strand's bases are not a residue batch)"""
    import fstitch_cases as FC
    import fstitch_ref as FR
    cases = [c for c in FC.worked_cases() if c[0].endswith("pad1+")]
    P = FC.cpu_inputs([c[1] for c in cases], [c[2] for c in cases], **FC.EXACT)
    got, _ = FR.stitch(P["fold"], P["fold_hits"], P["chain"], P["alignments"], P["cigars"], *P["frames"], *P["t"], gap_open=11, gap_extend=1)
    col = dict(zip(FR.NAMES, got))
    fh = P["fold_hits"]
    return dict(q=pack([]), t=P["t"], qid=np.asarray(fh[0], np.uint32), tid=np.asarray(fh[1], np.uint32), row_mask=None, row_offsets=None,
                op_offsets=col["op_offsets"], ops=col["ops"], q_start=np.zeros(len(fh[0]), np.uint32), t_start=col["t_start"])


def gpu_cases():
    """[(name, case, [(side, profile)])]: everything tests/test_gpu_pileup.py runs from this file, and what tests/test_pileup_cpu.py
    holds against the second formulation and counts the events of"""
    both = [(s, p) for s in ("query", "target") for p in (False, True)]
    regions, stitched = from_rstitch()
    regions_x, stitched_x = from_rstitch(eqx=True)
    return [("boundary", boundary_case(), both), ("boundary_to_the_end", boundary_case(True), both), ("lane_tails", lane_tail_case(), both), ("alternating", alternating_case(), both),
            ("csr", csr_rows(False), both), ("one_per_row", csr_rows(True), both), ("contention", contention_case(), [("target", False), ("target", True)]),
            ("fuzz", fuzz_batch(), both), ("fuzz_n", fuzz_batch(seed=7, with_n=True), [("target", False)]),
            ("rstitch_regions", regions, both), ("rstitch_stitched", stitched, both), ("rstitch_regions_eqx", regions_x, both),
            ("rstitch_stitched_eqx", stitched_x, both), ("fstitch", from_fstitch(), [("target", False)])]
