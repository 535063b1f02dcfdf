"""Inputs of the stitch tests with hand-written expectations, and the CPU pipeline that turns sequences into the stitch's inputs.
Not a test module.

MEMBER_CASES   chains written down member by member (extents and CIGAR): what the reference must make of them.  They need no
               pipeline, so they can state shapes a pipeline does not reach on demand (an overlap trimmed through an indel).
duplicate_pair a hit row that holds one alignment twice, and the doctored chain that links the two: a member trimmed to nothing.
PIPE_CASES     pairs of sequences whose stitched CIGAR is known by construction; they run through the CPU yardsticks
               (cpu_inputs) in the CPU test and through the device in the GPU test, with the same expected strings.
fuzz_batch     the GPU test's fuzz: relatives with planted insertions, deletions, replaced stretches and repeated boundaries."""
import numpy as np

import matchpos_join
import ralign_ref
import rchain_ref
import rcull_ref
import regions_ref
import rtrace_ref
from oracle import oracle

M, I, D, EQ, X = rtrace_ref.M, rtrace_ref.I, rtrace_ref.D, rtrace_ref.EQ, rtrace_ref.X
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
TWO = np.frombuffer(b"AC", np.uint8)
K = 7
INSERTION = 40


def _seq(rng, n, alphabet=PROTEIN):
    return bytes(alphabet[rng.integers(0, len(alphabet), n)])


def parse(cigar):
    out, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append((n, {"M": M, "I": I, "D": D, "=": EQ, "X": X}[ch]))
            n = 0
    return out


# ---- chains written down member by member ------------------------------------------------------------------------------------
# q and t are 'A' * 200 unless stated: under the +1 / -1 matrix every pair is a match.  members: (q_start, q_length, t_start,
# t_length, cigar).  expect: the stitched CIGAR, (n_filled, n_open, n_trimmed) and the events the row must show.
_A = b"A" * 200
MEMBER_CASES = [
    dict(name="touching", q=_A, t=_A, o=11, e=1, members=[(0, 10, 0, 10, "10M"), (10, 10, 10, 10, "10M")],
         expect="20M", counts=(0, 0, 0), events={"joint_merged"}),
    dict(name="one_member", q=_A, t=_A, o=11, e=1, members=[(3, 12, 5, 11, "6M1I5M")], expect="6M1I5M", counts=(0, 0, 0), events=set()),
    # X = Y = 1: one pair (a mismatch, -1) beats I + D (-24)
    dict(name="rect_1x1", q=b"AAAAACAAAAA", t=b"AAAAAGAAAAA", o=11, e=1, members=[(0, 5, 0, 5, "5M"), (6, 5, 6, 5, "5M")],
         expect="11M", counts=(1, 0, 0), events={"filled", "joint_merged"}),
    # X = 3, Y = 2, nothing matches: two pairs and one I; walking back prefers the diagonal, so the I comes first
    dict(name="rect_3x2", q=b"AAAAAKLMAAAAA", t=b"AAAAAWYAAAAA", o=11, e=1, members=[(0, 5, 0, 5, "5M"), (8, 5, 7, 5, "5M")],
         expect="5M1I7M", counts=(1, 0, 0), events={"filled", "joint_merged"}),
    # X = 3, Y = 2 with K and M shared: K = K, L alone, M = M
    dict(name="rect_3x2_match", q=b"AAAAAKLMAAAAA", t=b"AAAAAKMAAAAA", o=11, e=1, members=[(0, 5, 0, 5, "5M"), (8, 5, 7, 5, "5M")],
         expect="6M1I6M", counts=(1, 0, 0), events={"filled", "joint_merged"}),
    # the member behind starts 2 query and 3 target positions before the end of the one in front: M, D, M are trimmed — through
    # the D — and nothing lies between them
    dict(name="overlap_3_through_indel", q=_A, t=_A, o=11, e=1, members=[(0, 10, 0, 10, "10M"), (8, 11, 7, 12, "1M1D10M")],
         expect="19M", counts=(0, 0, 3), events={"trimmed", "joint_merged"}),
    # the trim ends inside an I run: after the M the target has reached the end in front, the query needs one I more
    dict(name="overlap_into_insertion", q=_A, t=_A, o=11, e=1, members=[(0, 10, 0, 10, "10M"), (8, 9, 9, 6, "1M3I5M")],
         expect="10M2I5M", counts=(0, 0, 2), events={"trimmed"}),
    # free gaps, a mismatch costs 1: every path without a pair scores 0.  H prefers H~ = F, so the walk's first step back is a
    # residue of Q — the target's here, roles swapped (X = 1 < Y = 2): ... I, then D D; the other orientation gives D, then I I
    dict(name="swapped_1x2", q=b"AAAAACAAAAA", t=b"AAAAAGGAAAAA", o=0, e=0, members=[(0, 5, 0, 5, "5M"), (6, 5, 7, 5, "5M")],
         expect="5M1I2D5M", counts=(1, 0, 0), events={"filled_swapped", "tie_F"}),
    dict(name="plain_2x1", q=b"AAAAACCAAAAA", t=b"AAAAAGAAAAA", o=0, e=0, members=[(0, 5, 0, 5, "5M"), (7, 5, 6, 5, "5M")],
         expect="5M1D2I5M", counts=(1, 0, 0), events={"filled", "tie_F"}),
    # both sides 64: open
    dict(name="rect_64x64", q=_A, t=_A, o=11, e=1, members=[(0, 5, 0, 5, "5M"), (69, 5, 69, 5, "5M")],
         expect="5M64I64D5M", counts=(0, 1, 0), events={"open"}),
    dict(name="pure_runs", q=_A, t=_A, o=11, e=1, members=[(0, 5, 0, 5, "5M"), (45, 5, 5, 5, "5M"), (50, 5, 30, 5, "5M")],
         expect="5M40I5M20D5M", counts=(0, 0, 0), events={"pure_I", "pure_D"}),
    # equal ends: every column of the second member goes, its end still stands; the third follows it
    dict(name="trimmed_to_nothing", q=_A, t=_A, o=11, e=1, members=[(0, 10, 0, 10, "10M"), (4, 6, 4, 6, "6M"), (12, 4, 10, 4, "4M")],
         expect="10M2I4M", counts=(0, 0, 6), events={"trimmed", "trimmed_to_nothing", "pure_I"}),
    # with max_fill 70: a long side of 70 is filled — the one pair goes last: H~ prefers D on the tie — 71 is open (short side 1)
    dict(name="long_side_at_max_fill", q=b"A" * 5 + b"C" * 70 + b"A" * 5, t=b"A" * 5 + b"G" + b"A" * 5, o=11, e=1, max_fill=70,
         members=[(0, 5, 0, 5, "5M"), (75, 5, 6, 5, "5M")], expect="5M69I6M", counts=(1, 0, 0), events={"filled", "joint_merged"}),
    dict(name="long_side_past_max_fill", q=b"A" * 5 + b"C" * 71 + b"A" * 5, t=b"A" * 5 + b"G" + b"A" * 5, o=11, e=1, max_fill=70,
         members=[(0, 5, 0, 5, "5M"), (76, 5, 6, 5, "5M")], expect="5M71I1D5M", counts=(0, 1, 0), events={"open"}),
]


# ---- pairs of sequences whose stitched CIGAR is known ------------------------------------------------------------------------
def insertion_pair():
    """Two proteins that are the same but for 40 residues inserted into the query: two alignments, one on each side."""
    rng = np.random.default_rng(2027)
    t = _seq(rng, 120)
    return t[:60] + _seq(rng, INSERTION) + t[60:], t


FLANK = np.frombuffer(b"ACDEFGHIKLMNPQRSTV", np.uint8)  # (no W, no Y: the middles are made of them)


def _flanked(rng, q_mid, t_mid, n=30):
    """A shared flank of n residues on both sides of two different middles."""
    a, b = _seq(rng, n, FLANK), _seq(rng, n, FLANK)
    return a + q_mid + b, a + t_mid + b


def pipe_cases():
    """[(name, q, t, options, expected CIGAR, expected CIGAR with eqx)]: band 0 and x_drop 0 keep an alignment on the exact
    matches around its seed, so what lies between two of them is exactly the two middles."""
    rng = np.random.default_rng(415)
    exact = dict(band=0, gap_open=11, gap_extend=1, x_drop=0)
    out = []
    q, t = insertion_pair()
    out.append(("insertion_pair", q, t, dict(band=16, gap_open=11, gap_extend=1, x_drop=30), "60M40I60M", "60=40I60="))
    # (the query's middle is W's, the target's Y's, the flanks hold neither: no pair of the middles matches, none extends a flank)
    q, t = _flanked(rng, b"W", b"Y")
    out.append(("rect_1x1", q, t, exact, "61M", "30=1X30="))
    q, t = _flanked(rng, b"WWW", b"YY")
    out.append(("rect_3x2", q, t, exact, "30M1I32M", "30=1I2X30="))
    q, t = _flanked(rng, b"W" * 64, b"Y" * 64)
    out.append(("rect_64x64", q, t, exact, "30M64I64D30M", "30=64I64D30="))
    q, t = _flanked(rng, b"", b"Y" * 9)
    out.append(("pure_D", q, t, exact, "30M9D30M", "30=9D30="))
    return out


def duplicate_pair():
    """A pair whose two seeds — the flanks on either side of one mismatch, on one diagonal — extend to the SAME alignment under an
    X-drop that tolerates the mismatch: without the cull the hit row holds it twice.  -> (q, t, alignment options)"""
    q, t = _flanked(np.random.default_rng(11), b"W", b"Y")
    return q, t, dict(band=0, gap_open=11, gap_extend=1, x_drop=5)


DOCTORED_CHAIN = dict(max_overlap=100)


def doctored_columns(al):
    """The chain's input columns for duplicate_pair's two alignments with the second moved one position down both sequences: a
    chain made of THESE links the two (starts and ends ascend strictly), and stitched with the real alignments its second
    member ends where the first does — every column of it is trimmed.  The one way to a member trimmed to nothing: a chain of
    the alignments themselves never links equal ends."""
    shift = np.arange(len(al[1]), dtype=np.uint32)
    return (al[0], al[1] + shift, al[2], al[3] + shift, al[4], al[5])


# ---- the CPU pipeline ---------------------------------------------------------------------------------------------------------
def cpu_inputs(qs, ts, k=K, matrix=None, band=16, gap_open=11, gap_extend=1, x_drop=30, eqx=False, cull=True, min_kmers=1, **chain_opts):
    """Sequences -> what ks_regions_stitch takes, through the CPU yardsticks alone: oracle sketches and join, regions, alignments,
    the cull's kept ones, their paths and their chain.  -> dict(hits, alignments, cigars, chain, q, t)."""
    q, t = oracle.pack(qs), oracle.pack(ts)
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], k, 1, "protein")
    rg = regions_ref.chain(join[0], join[1], join[2], k, min_kmers=min_kmers)
    kw = dict(matrix=matrix, band=band, gap_open=gap_open, gap_extend=gap_extend)
    al = ralign_ref.align(rg, hits[0], hits[1], q[0], q[1], t[0], t[1], x_drop=x_drop, **kw)
    if cull:
        cu = rcull_ref.cull(*al[:6])
        src = cu[1].astype(np.int64)
        al = (cu[0], *[np.asarray(c)[src] for c in al[1:]])
        rg = (cu[0], *[np.asarray(c)[src] for c in rg[1:]])
    tr = rtrace_ref.trace(rg, al, hits[0], hits[1], q[0], q[1], t[0], t[1], eqx=eqx, **kw)
    offs, ops = [0], []
    for cg, _ in tr:
        ops += [(n << 4) | c for n, c in cg]
        offs.append(len(ops))
    chain = rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **chain_opts)
    return dict(hits=hits, alignments=al, cigars=(np.array(offs, np.uint64), np.array(ops, np.uint32)), chain=chain, q=q, t=t)


# ---- the fuzz -------------------------------------------------------------------------------------------------------------------
FUZZ_ROWS = 300


def fuzz_batch(seed=99, n=FUZZ_ROWS):
    """n (query, target) pairs, query i a relative of target i: two or three shared blocks of 14 .. 50 residues, and between
    two of them one of: residues inserted into the query or the target alone (5 .. 60), a stretch replaced by another of
    another length (both sides 1 .. 70, or two short ones over two letters), a boundary repeated so that the neighbours overlap, or nothing but a few substitutions.
    Sequences of at most 200 residues; some pairs share nothing (no hit row) and some queries hit only through one block."""
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for i in range(n):
        n_blocks = int(rng.integers(1, 4))
        q, t = b"", b""
        for b in range(n_blocks):
            blk = _seq(rng, int(rng.integers(14, 51)))
            if b:
                kind = int(rng.integers(0, 7))
                if kind == 0:
                    q += _seq(rng, int(rng.integers(5, 61)))
                elif kind == 1:
                    t += _seq(rng, int(rng.integers(5, 61)))
                elif kind == 2:
                    q += _seq(rng, int(rng.integers(1, 71))); t += _seq(rng, int(rng.integers(1, 12)))
                elif kind == 3:
                    q += _seq(rng, int(rng.integers(1, 12))); t += _seq(rng, int(rng.integers(1, 71)))
                elif kind == 4:  # the insertion begins with the head of the block behind it, and ends with the tail of the one before
                    m = int(rng.integers(2, 7))
                    q += blk[:m] + _seq(rng, int(rng.integers(6, 30))) + q[-m:]
                elif kind == 5:
                    m = int(rng.integers(1, 4))
                    q += _seq(rng, m); t += _seq(rng, m)
                else:  # two stretches over two letters: a fill full of ties
                    q += _seq(rng, int(rng.integers(2, 25)), TWO); t += _seq(rng, int(rng.integers(2, 25)), TWO)
            q += blk; t += blk
        if i % 29 == 0:
            t = _seq(rng, 40)  # a pair that shares nothing
        qs.append(q[:200]); ts.append(t[:200])
    return qs, ts


def tie_batch(seed=7, n=200):
    """n pairs of two shared flanks around two different middles — the query's of 1 .. 12, the target's of 1 .. 6 residues (no
    k-mer: no hit through a middle) — over the two letters the flanks lack, whose
    first and last residues differ: aligned with band 0 and x_drop 0 the two alignments are the flanks, the link is the two
    middles, and with a free gap extension its fill is full of ties."""
    rng = np.random.default_rng(seed)
    wy = np.frombuffer(b"WY", np.uint8)
    qs, ts = [], []
    for _ in range(n):
        qm = bytearray(_seq(rng, int(rng.integers(1, 13)), wy)); tm = bytearray(_seq(rng, int(rng.integers(1, 7)), wy))
        tm[0] = ord("W") + ord("Y") - qm[0]
        if len(tm) > 1 or tm[0] == qm[-1]:
            tm[-1:] = bytes([ord("W") + ord("Y") - qm[-1]]) if len(tm) > 1 else tm[-1:]
        q, t = _flanked(rng, bytes(qm), bytes(tm), 12)
        qs.append(q); ts.append(t)
    return qs, ts


# the GPU test's fuzz inputs: the batch, the alignment and chain options it runs under, max_fill
FUZZ = (
    dict(name="relatives", batch=fuzz_batch, align=dict(band=4, gap_open=2, gap_extend=1, x_drop=6), chain=dict(max_overlap=12), max_fill=40),
    dict(name="ties", batch=tie_batch, align=dict(band=0, gap_open=1, gap_extend=0, x_drop=0), chain=dict(), max_fill=40),
)
