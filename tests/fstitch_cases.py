"""Inputs of the frame-stitch tests, built entirely from the CPU references, and hand-written expectations.  Not a test module.

cpu_inputs     nucleotide records x proteins -> what ks_frames_stitch takes, through the CPU yardsticks alone: translate_ref's six
               frames, the region / align / cull / trace references as rstitch_cases.cpu_inputs runs them, ffold_ref.fold and
               rchain_ref on the fold's columns.  Every claim about a case can be shown without a GPU.
WORKED         the two worked examples of the header (one base inserted, one base deleted), an overhang that must be trimmed and
               shifts with codons in the link, on both strands and in all three starting frames, with their CIGARs written down.
MEMBER_ROWS    chains written down member by member (frame, extents, CIGAR): shapes no pipeline reaches on demand — a member
               trimmed to nothing between two shifts.
fuzz_batch     genes of at most 120 codons with planted +-1 / +-2 base indels, planted codon insertions and replaced stretches.
planted        the 24 contigs of the kind tests/test_gpu_ffold.py plants, by seed."""
import functools

import numpy as np

import ffold_ref
import rchain_ref
import rstitch_cases as SC
import translate_ref

K = SC.K
EXACT = dict(band=0, gap_open=11, gap_extend=1, x_drop=0)  # an alignment is the exact matches around its seed
CHAIN = dict(max_overlap=15)                               # bases, as tests/test_gpu_ffold.py chains its planted contigs
AA = b"ACDEFGHIKLMNPQRSTVWY"


def cpu_inputs(contigs, proteins, chain=None, **opts):
    """-> dict: frames (f_res, f_off), t (t_res, t_off), nt_off, frame_hits, alignments, cigars, frame_chain (the per-frame
    chain of rstitch_cases.cpu_inputs), fold_hits, fold (ffold_ref.NAMES order), chain (of the fold's columns)"""
    frames = translate_ref.translate6(contigs)
    P = SC.cpu_inputs(frames, proteins, **opts)
    al, h = P["alignments"], P["hits"]
    nt_off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.uint64)
    fold_hits, fold = ffold_ref.fold(h[0], h[1], h[2], h[3], nt_off, al[0], al[1], al[2], al[3], al[4], score=al[5], identities=al[6], aln_length=al[10])
    c = dict(zip(ffold_ref.NAMES, fold))
    ch = rchain_ref.chain(c["row_offsets"], c["s_start"], c["nt_length"], c["t_start3"], c["t_length3"], c["score"], identities=c["identities"],
                          aln_length=c["aln_length"], **(CHAIN if chain is None else chain))
    return dict(frames=P["q"], t=P["t"], nt_off=nt_off, frame_hits=h, alignments=al, cigars=P["cigars"], frame_chain=P["chain"], fold_hits=fold_hits,
                fold=fold, chain=ch, opts=opts)


# ---- the worked examples -------------------------------------------------------------------------------------------------------
def _protein(rng, n, alphabet=SC.FLANK):
    return SC._seq(rng, n, alphabet)


def _contig(gene, pad, reverse, tail=b"TT"):
    """`pad` bases in front of the gene (the starting frame), on the strand asked for"""
    dna = b"G" * pad + gene + tail
    return translate_ref.reverse_complement(dna) if reverse else dna


def worked_cases(seed=5):
    """[(name, contig, protein, align options, max_fill, expected CIGAR, strand, n_frameshifts)] for pad 0, 1, 2 and both strands.
    The flanks hold neither W nor Y, so no pair of a W / Y middle matches and no flank extends into one; the seed is chosen so that
    no chance match exists beside a shift (the CPU test shows it: the reference reproduces the strings)."""
    out = []
    for pad in (0, 1, 2):
        for reverse in (False, True):
            rng = np.random.default_rng(seed + 10 * pad + int(reverse))
            tag = f"pad{pad}{'-' if reverse else '+'}"
            n, m = 40, 18
            prot = _protein(rng, n)
            gene = translate_ref.reverse_translate(prot, rng)
            mk = lambda g: _contig(g, pad, reverse)  # noqa: E731
            # one base inserted after codon m: X = 1, Y = 0
            out.append((f"inserted_{tag}", mk(gene[:3 * m] + b"C" + gene[3 * m:]), prot, EXACT, 0, f"{m}M1N{n - m}M", int(reverse), 1))
            # one base of codon m deleted: X = 2, Y = 1, c = 0
            out.append((f"deleted_{tag}", mk(gene[:3 * m] + gene[3 * m + 1:]), prot, EXACT, 0, f"{m}M1D2N{n - m - 1}M", int(reverse), 1))
            # an overhang: codon m is AAA (K) and the inserted base an A, so the old frame reads one more K; the member behind is
            # trimmed by that codon
            pk = prot[:m] + b"K" + prot[m + 1:]
            gk = gene[:3 * m] + b"AAA" + gene[3 * m + 3:]
            out.append((f"overhang_{tag}", mk(gk[:3 * m] + b"A" + gk[3 * m:]), pk, EXACT, 0, f"{m + 1}M1N{n - m - 1}M", int(reverse), 1))
            # codons in the link: two W codons against two Y residues, then the inserted base: a 2 x 2 fill of mismatches
            a, b = _protein(rng, 20), _protein(rng, 20)
            ga, gb = translate_ref.reverse_translate(a, rng), translate_ref.reverse_translate(b, rng)
            out.append((f"filled_{tag}", mk(ga + b"TGGTGG" + b"C" + gb), a + b"YY" + b, EXACT, 0, "22M1N20M", int(reverse), 1))
            # 64 x 64 codons: open, the shift behind it
            out.append((f"open_{tag}", mk(ga + b"TGG" * 64 + b"CC" + gb), a + b"Y" * 64 + b, EXACT, 0, "20M64I64D2N20M", int(reverse), 1))
            # no shift at all
            out.append((f"plain_{tag}", mk(gene), prot, EXACT, 0, f"{n}M", int(reverse), 0))
    return out


# ---- chains written down member by member ------------------------------------------------------------------------------------
# One record of 'A' bases: every frame of the forward strand is K's; the target is K's too: every pair matches.  members: (frame
# 0 .. 2, q_start, q_length, t_start, t_length, cigar) in chain order.
MEMBER_ROWS = [
    # the second member ends where the shift before it put it: every column goes, both N ops stay, side by side
    dict(name="nothing_between_two_shifts", members=[(0, 0, 10, 0, 10, "10M"), (1, 8, 2, 8, 2, "2M"), (2, 10, 5, 10, 5, "5M")],
         expect="10M1N1N5M", counts=(0, 0, 2, 2), events={"trimmed", "trimmed_to_nothing", "shift_1"}),
    dict(name="two_frames_back", members=[(2, 0, 10, 0, 10, "10M"), (0, 11, 5, 10, 5, "5M")],
         expect="10M1N5M", counts=(0, 0, 0, 1), events={"shift_1"}),
    dict(name="same_frame_I", members=[(1, 0, 10, 0, 10, "10M"), (1, 14, 5, 10, 5, "5M")],
         expect="10M4I5M", counts=(0, 0, 0, 0), events={"pure_I", "same_frame_link"}),
    dict(name="shift_2_after_fill", members=[(0, 0, 10, 0, 10, "10M"), (2, 12, 5, 12, 5, "5M")],
         expect="12M2N5M", counts=(1, 0, 0, 1), events={"filled", "shift_2", "shift_with_codons", "joint_merged"}),
    dict(name="one_member", members=[(1, 3, 12, 5, 11, "6M1I5M")], expect="6M1I5M", counts=(0, 0, 0, 0), events=set()),
]


def member_inputs(rows, n_bases=120, n_t=60, reverse=False):
    """Hand-written rows (each a list of members as in MEMBER_ROWS) -> the arrays ks_frames_stitch takes, one record of 'A' (or,
    reverse, of 'T': its reverse complement is 'A's) per row against one target of K's.  The frame rows are built in (qid, tid)
    order, folded by ffold_ref.fold, and the chain is written down: the folded regions in the members' order."""
    contigs = [(b"T" if reverse else b"A") * n_bases for _ in rows]
    frames = translate_ref.translate6(contigs)
    prot = [b"K" * n_t]
    strand = 3 if reverse else 0
    qid, tid, row_off, al, ops, op_off, where = [], [], [0], [[], [], [], []], [], [0], {}
    for s, members in enumerate(rows):
        for f in range(3):
            mine = [(i, m) for i, m in enumerate(members) if m[0] == f]
            if not mine:
                continue
            qid.append(6 * s + strand + f); tid.append(0)
            for i, m in mine:
                where[(s, i)] = len(al[0])
                for c, v in zip(al, m[1:5]):
                    c.append(v)
                ops += [(n << 4) | code for n, code in SC.parse(m[5])]
                op_off.append(len(ops))
            row_off.append(len(al[0]))
    u32 = lambda a: np.array(a, np.uint32)  # noqa: E731
    n = len(al[0])
    alignments = (np.array(row_off, np.uint64), u32(al[0]), u32(al[1]), u32(al[2]), u32(al[3]), np.array(al[1], np.int64), u32(al[1]), u32(al[1]),
                  np.zeros(n, np.uint32), np.zeros(n, np.uint32), u32(al[1]))
    nt_off = n_bases * np.arange(len(rows) + 1, dtype=np.uint64)
    hits = (u32(qid), u32(tid), np.ones(len(qid), np.uint32), np.ones(len(qid), np.uint64))
    fold_hits, fold = ffold_ref.fold(*hits, nt_off, *alignments[:5], score=alignments[5], identities=alignments[6], aln_length=alignments[10])
    src = fold[2].tolist()
    c_off, c_src = [0], []
    for s, members in enumerate(rows):
        c_src += [src.index(where[(s, i)]) for i in range(len(members))]
        c_off.append(len(c_src))
    z = np.zeros(len(rows), np.uint32)
    chain = (np.array(c_off, np.uint64), u32(c_src), np.zeros(n, np.int64), np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(len(rows), np.int64), z, z, z, z,
             z, z, np.zeros(len(rows), np.uint64), np.zeros(len(rows), np.uint64), np.zeros(len(rows), np.float64))
    assert fold_hits[0].tolist() == [2 * s + int(reverse) for s in range(len(rows))]
    return dict(frames=translate_ref.pack(frames), t=translate_ref.pack(prot), nt_off=nt_off, frame_hits=hits, alignments=alignments,
                cigars=(np.array(op_off, np.uint64), u32(ops)), fold_hits=fold_hits, fold=fold, chain=chain, opts=dict(gap_open=11, gap_extend=1))


# ---- the fuzz -------------------------------------------------------------------------------------------------------------------
def fuzz_batch(seed, n=110):
    """n genes of 40 .. 120 codons against their proteins.  A gene is two or three blocks of its protein; between two of them one
    of: one or two bases inserted or deleted (with or without a replaced stretch of 1 .. 6 codons beside them), 20 .. 60 codons
    inserted, a stretch of the protein replaced, a boundary codon repeated, a run of one base against a longer run of its residue, or nothing.  A third of the contigs are reverse
    complements; the starting frame varies.  -> (contigs, proteins)"""
    rng = np.random.default_rng(seed)
    base = lambda k: bytes(b"ACGT"[i] for i in rng.integers(0, 4, k))  # noqa: E731
    contigs, proteins = [], []
    for i in range(n):
        n_blocks = int(rng.integers(2, 4))
        prot, gene = b"", b""
        for b in range(n_blocks):
            blk = SC._seq(rng, int(rng.integers(14, 40)))
            if b:
                kind = int(rng.integers(0, 10))
                if kind in (0, 1):  # +1 / +2 bases
                    gene += base(kind + 1)
                elif kind in (2, 3):  # -1 / -2 bases: the tail of the codon before goes
                    gene = gene[:-(kind - 1)]
                elif kind == 4:  # a shift beside a replaced stretch
                    gene += translate_ref.reverse_translate(SC._seq(rng, int(rng.integers(1, 7))), rng) + base(int(rng.integers(1, 3)))
                    prot += SC._seq(rng, int(rng.integers(1, 7)))
                elif kind == 5:  # codons inserted, with or without a few residues of the target alone
                    gene += translate_ref.reverse_translate(SC._seq(rng, int(rng.integers(20, 61))), rng) + base(int(rng.integers(0, 3)))
                    prot += SC._seq(rng, int(rng.integers(0, 4)))
                elif kind == 6:  # a stretch of the target alone
                    prot += SC._seq(rng, int(rng.integers(1, 30)))
                    gene += base(int(rng.integers(0, 3)))
                elif kind == 7:  # the boundary repeated: the neighbours overlap
                    m = int(rng.integers(2, 6))
                    gene += gene[-3 * m:] + base(int(rng.integers(0, 3)))
                elif kind == 8:  # a run of one base, a frame more or less, against a longer run of its residue: every frame reads it
                    m, h = int(rng.integers(7, 11)), int(rng.integers(0, 4))
                    gene += b"ACGT"[h:h + 1] * (3 * m + int(rng.integers(1, 3))); prot += b"KPGF"[h:h + 1] * (m + int(rng.integers(1, 9)))
            prot += blk; gene += translate_ref.reverse_translate(blk, rng)
        prot, gene = prot[:120], gene[:360]
        dna = base(int(rng.integers(0, 5))) + gene + base(int(rng.integers(0, 5)))
        contigs.append(translate_ref.reverse_complement(dna) if i % 3 == 2 else dna)
        proteins.append(prot)
    return contigs, proteins


# the fuzz inputs: seeds chosen on the CPU so that the two batches together reach every event of fstitch_ref.EVENTS
FUZZ = (
    dict(name="indels", seed=3, align=dict(band=4, gap_open=2, gap_extend=1, x_drop=6), chain=dict(max_overlap=18), max_fill=40),
    dict(name="exact", seed=5, align=EXACT, chain=dict(max_overlap=30), max_fill=25),
)


@functools.lru_cache(maxsize=None)
def fuzz_inputs(i, eqx=False):
    F = FUZZ[i]
    contigs, proteins = fuzz_batch(F["seed"])
    return cpu_inputs(contigs, proteins, chain=F["chain"], eqx=eqx, **F["align"])


# ---- planted genes, half of them with a frameshift ------------------------------------------------------------------------------
N_CONTIGS = 24
PLANTED_SEED = 4242


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED):
    """24 contigs with one gene each, as tests/test_gpu_ffold.py plants them: half on the reverse strand, half with one base
    inserted m codons into the gene.  -> (proteins, contigs, truth)"""
    rng = np.random.default_rng(seed)
    proteins = [bytes(AA[i] for i in rng.integers(0, 20, int(rng.integers(60, 121)))) for _ in range(20)]
    flank = lambda n: bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    contigs, truth = [], []
    for c in range(N_CONTIGS):
        t = c % 20
        prot = proteins[t]
        reverse, shifted = c % 2 == 1, (c // 2) % 2 == 1
        gene = translate_ref.reverse_translate(prot, rng)
        m = 0
        if shifted:
            m = int(rng.integers(20, len(prot) - 20 + 1))
            gene = gene[:3 * m] + flank(1) + gene[3 * m:]
        left, right = (10, 11, 12)[c % 3], (10, 11, 12)[(c // 3) % 3]
        contigs.append(flank(left) + (translate_ref.reverse_complement(gene) if reverse else gene) + flank(right))
        truth.append(dict(record=c, target=t, reverse=reverse, shifted=shifted, start=left, end=left + len(gene), length=len(prot), m=m,
                          contig_length=len(contigs[-1])))
    return proteins, contigs, truth
