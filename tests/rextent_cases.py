"""Inputs of the extent tests (test_region_extents_cpu.py, test_gpu_region_extents.py): the region pipeline — align, trace,
cull, take, chain, stitch — at the extents its contracts allow and on real proteins.  Not a test module.

fills      section 1: flank pairs (rstitch_cases._flanked) whose link is a rectangle with a long side around the stitch's stage,
           its default max_fill (1024) and its limit (4096), all-mismatch and with a real path.
relative   section 2: one pair of relatives with every class of link between its stretches; the stitched CIGAR is written down
           from the construction alone.
capacity   section 3: pairs at 2^20 residues whose alignments can be stated on paper.
real       section 4: a subset of the golden human proteins, all against all.
FILLS      one memo of rstitch_ref.fill for a whole run: the tests stitch the same rectangles several times over (eqx on and off,
           max_fill 0 / 1024 / 4096, whole and sliced) and a 4096 x 63 table costs the reference a second."""
import os

import numpy as np

import rstitch_cases as SC
import rstitch_ref as SR

M, I, D, EQ, X = SR.M, SR.I, SR.D, SR.EQ, SR.X
K = SC.K
EXACT = dict(band=0, gap_open=11, gap_extend=1, x_drop=0)  # an alignment is the exact matches around its seed
FLANK = SC.FLANK  # the eighteen letters without W and Y
W, Y = ord("W") - 65, ord("Y") - 65
CHAIN = dict(max_overlap=12)
PROBE = dict(band=16, gap_open=11, gap_extend=1, x_drop=30)
HUGE = 2 ** 20


def random_matrix(seed):
    """The seeded int8 matrix of the align tests: not symmetric, holds both limits."""
    m = np.random.default_rng(seed).integers(-128, 128, (28, 28)).astype(np.int8)
    m[3, 7], m[7, 3] = -128, 127
    assert not np.array_equal(m, m.T)
    return m


class _Fills:
    """rstitch_ref.fill, remembered.  The table and the walk do not depend on eqx — it only names the pairs = / X instead of M
    (rstitch_ref.fill: the one line that reads it) — so a rectangle is filled once with eqx and the M version is that one with
    = and X renamed.  test_region_extents_cpu.py holds the renamed version to a direct call."""

    def __init__(self):
        self.memo, self.orig, self.depth = {}, SR.fill, 0

    def __call__(self, qst, tst, matrix, gap_open, gap_extend, eqx):
        key = (bytes(qst), bytes(tst), tuple(tuple(int(v) for v in row) for row in matrix), int(gap_open), int(gap_extend))
        if key not in self.memo:
            self.memo[key] = self.orig(qst, tst, matrix, gap_open, gap_extend, True)
        cols, score, ev, swapped = self.memo[key]
        return (list(cols) if eqx else [M if c in (EQ, X) else c for c in cols]), score, set(ev), swapped

    def __enter__(self):
        self.depth += 1
        SR.fill = self
        return self

    def __exit__(self, *exc):
        self.depth -= 1
        if self.depth == 0:
            SR.fill = self.orig


FILLS = _Fills()


def cpu_stages(qs, ts, k=K, matrix=None, band=16, gap_open=11, gap_extend=1, x_drop=30, eqx=False, chain=None):
    """rstitch_cases.cpu_inputs with every stage kept: sequences -> dict(hits, regions, all (every alignment), cull, alignments
    and kept_regions (what the cull kept), traced [(cigar, events)], cigars, chain, q, t), through the CPU yardsticks alone."""
    import matchpos_join
    import ralign_ref
    import rchain_ref
    import rcull_ref
    import regions_ref
    import rtrace_ref
    from oracle import oracle
    q, t = oracle.pack(qs), oracle.pack(ts)
    hits, join, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], k, 1, "protein")
    rg = regions_ref.chain(join[0], join[1], join[2], k, min_kmers=1)
    kw = dict(matrix=matrix, band=band, gap_open=gap_open, gap_extend=gap_extend)
    al_all = ralign_ref.align(rg, hits[0], hits[1], q[0], q[1], t[0], t[1], x_drop=x_drop, **kw)
    cu = rcull_ref.cull(*al_all[:6])
    src = cu[1].astype(np.int64)
    al = (cu[0], *[np.asarray(c)[src] for c in al_all[1:]])
    kept = (cu[0], *[np.asarray(c)[src] for c in rg[1:]])
    tr = rtrace_ref.trace(kept, al, hits[0], hits[1], q[0], q[1], t[0], t[1], eqx=eqx, **kw)
    return dict(hits=hits, regions=rg, all=al_all, cull=cu, alignments=al, kept_regions=kept, traced=tr, cigars=encode([c for c, _ in tr]),
                chain=rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **(chain or {})), q=q, t=t, opts=kw)


def cigars_of(P, eqx):
    """The kept alignments of cpu_stages traced once more, with or without eqx -> (op_offsets, ops)."""
    import rtrace_ref
    tr = rtrace_ref.trace(P["kept_regions"], P["alignments"], P["hits"][0], P["hits"][1], P["q"][0], P["q"][1], P["t"][0], P["t"][1],
                          eqx=eqx, **P["opts"])
    return encode([c for c, _ in tr])


def encode(cigars):
    """[(len, code)] per region -> (op_offsets u64, ops u32) as RegionCigars.to_host()."""
    offs, ops = [0], []
    for cg in cigars:
        ops += [(n << 4) | c for n, c in cg]
        offs.append(len(ops))
    return np.array(offs, np.uint64), np.array(ops, np.uint32)


def ref_stitch(P, matrix=None, gap_open=11, gap_extend=1, max_fill=0, eqx=False, cigars=None):
    """rstitch_ref.stitch on what cpu_stages (or the device, copied to the host in the same layout) made."""
    with FILLS:
        return SR.stitch(P["chain"], P["alignments"], cigars if cigars is not None else P["cigars"], P["hits"][0], P["hits"][1],
                         P["q"][0], P["q"][1], P["t"][0], P["t"][1], matrix=matrix, gap_open=gap_open, gap_extend=gap_extend,
                         max_fill=max_fill, eqx=eqx)


# ---- 1. long fills ---------------------------------------------------------------------------------------------------------------
SHORTS = (1, 2, 63, 64)
STAGE = 64  # ks_debug_rstitch_stage(): the GPU test asserts it


def long_sides(stage=STAGE):
    """The long sides by group: around two stages, around the default max_fill, around the limit — the last one side a group:
    eight rectangles each, a 4096 x 63 table costs the reference a second."""
    return {"stage": (2 * stage - 1, 2 * stage, 2 * stage + 1), "default": (1023, 1024, 1025), "4095": (4095,), "4096": (4096,),
            "4097": (4097,)}


SLICED = ((4095, 4096), (2, 63))  # the long and short sides of the batch that runs one link per slice: eight links, all filled


def mismatch_batch(longs, seed, shorts=SHORTS):
    """-> (shapes [(X, Y)], queries, targets): per long side and short side both orientations; the query's middle is X W's, the
    target's Y Y's, the flanks hold neither, so no pair of the middles matches and none extends a flank."""
    rng = np.random.default_rng(seed)
    shapes = [(a, b) for a in longs for b in shorts] + [(b, a) for a in longs for b in shorts]
    pairs = [SC._flanked(rng, b"W" * x, b"Y" * y) for x, y in shapes]
    return shapes, [q for q, _ in pairs], [t for _, t in pairs]


def link_class(x, y, max_fill):
    """What ks_regions_stitch makes of an X x Y link (both >= 1): the header's rule, 0 meaning 1024."""
    return "filled" if min(x, y) <= 63 and max(x, y) <= (max_fill or 1024) else "open"


def mismatch_row(x, y, max_fill, gap_open=11, gap_extend=1, flank=30):
    """An all-mismatch X x Y link between two flanks of `flank` matches -> (CIGAR or None, score, n_filled, n_open, gap_opens,
    aln_length).  Open: I x X then D x Y, literally.  Filled: min(X, Y) mismatched pairs and ONE run of the difference (any other
    path opens a second gap or pairs no more residues); where in the path the run lies is the tie rules' business, so the
    CIGAR of a filled link is left to the reference."""
    lo, hi = min(x, y), max(x, y)
    if link_class(x, y, max_fill) == "open":
        return (f"{flank}M{x}I{y}D{flank}M", 2 * flank - 2 * gap_open - (x + y) * gap_extend, 0, 1, 2, 2 * flank + x + y)
    return None, 2 * flank - lo - (gap_open + (hi - lo) * gap_extend), 1, 0, 1, 2 * flank + hi


PATH_GAPS = ((11, 1), (1, 0))  # (the second makes ties: a mismatch costs what a gap of any length does)
PLACES = ("start", "end", "middle", "split")


def path_matrix(seed):
    """random_matrix(seed) made to keep EXACT's alignments on the flanks: a flank letter scores > 0 against itself (the walk
    over a flank never drops), and W over Y is -128 (it stops at the middle's first and last pair).  Everything between two
    different letters stays random and asymmetric."""
    m = random_matrix(seed).astype(np.int16)
    for c in FLANK.tolist():
        m[c - 65, c - 65] = min(127, max(1, abs(int(m[c - 65, c - 65]))))
    m[W, Y] = -128
    return m.astype(np.int8)


def path_pair(rng, long_n, short_n, place, query_long):
    """Two middles with a real path: the long one is W / Y + random flank letters + W / Y; the short one a copy of a window of it
    (at its start, its end, its middle, or half at either end) with every fifth residue changed: at most four residues in a
    row agree, so no 7-mer is shared and the link stays a link.  The query's middle begins and ends with W, the target's with
    Y: the pair that would extend a flank is a mismatch under +1 / -1 and -128 under path_matrix.  -> (query, target)"""
    body = SC._seq(rng, long_n - 2, FLANK)
    n = short_n - 2
    at = {"start": [(0, n)], "end": [(len(body) - n, n)], "middle": [((len(body) - n) // 2, n)],
          "split": [(0, n // 2), (len(body) - (n - n // 2), n - n // 2)]}[place]
    window = bytearray(b"".join(body[a:a + k] for a, k in at))
    letters = FLANK.tolist()
    for i in range(2, len(window), 5):
        window[i] = letters[(letters.index(window[i]) + 1 + i % 7) % len(letters)]
    qb, tb = (body, bytes(window)) if query_long else (bytes(window), body)
    return SC._flanked(rng, b"W" + qb + b"W", b"Y" + tb + b"Y")


def path_batch(seed, stage=STAGE):
    """-> (shapes [(X, Y)], queries, targets): every placement at a long side of 2 * stage + 1 and of 4096, two of them at 1025;
    the orientation alternates."""
    rng = np.random.default_rng(seed)
    shapes, qs, ts = [], [], []
    for long_n, short_n, places in ((2 * stage + 1, 40, PLACES), (1025, 63, ("start", "split")), (4096, 63, PLACES)):
        for i, place in enumerate(places):
            query_long = (i + long_n) % 2 == 0
            q, t = path_pair(rng, long_n, short_n, place, query_long)
            shapes.append((long_n, short_n) if query_long else (short_n, long_n))
            qs.append(q); ts.append(t)
    return shapes, qs, ts


def middles(q, t, flank=30):
    return q[flank:len(q) - flank], t[flank:len(t) - flank]


def slices_of(rows_per_member, budget_rows):
    """The header's slicing, restated: consecutive chain members while the direction rows of their links fit the budget.
    -> the number of slices, or the first member whose link alone does not fit (as a negative number - 1)."""
    total = sum(rows_per_member)
    if total <= budget_rows:
        return 1
    n, j0 = 0, 0
    while j0 < len(rows_per_member):
        j1, have = j0, 0
        while j1 < len(rows_per_member) and have + rows_per_member[j1] <= budget_rows:
            have += rows_per_member[j1]
            j1 += 1
        if j1 == j0:
            return -1 - j0
        n, j0 = n + 1, j1
    return n


# ---- 2. one pair of relatives with every class of link ------------------------------------------------------------------------------
# The query and the target are the same stretches of random flank letters, the target's with a substitution at every sixth
# residue (positions 3, 9, 15, ... of a stretch: never its first or last residue), so that at most five residues in a row
# agree and no 7-mer is shared — but for the exact islands of 12 residues, the only seeds.  Between the stretches:
#   (10, 0)     ten W's in the query alone: band 16 and band 31 bridge them (a gap of 10 costs 21, x_drop is 30)
#   (40, 0)     forty W's in the query alone: beyond either band, two alignments and an I link
#   (50, 900)   W's over Y's: a filled link by default.  All-mismatch: 50 pairs and one run of 850; walked back from its end
#               the path takes a pair wherever a pair is among the best (H~ prefers D), so the pairs come LAST: 850D, 50 pairs
#   (50, 1100)  open by default (I x 50, D x 1100), filled at max_fill = 4096: 1050D, 50 pairs
#   (100, 100)  open at any max_fill: 100I 100D.  No alignment crosses it, not even without an X-drop: the stretches on either
#               side of it are worth less than the 100 it costs (120 residues: 100 matches - 20 substitutions = 80)
#   (0, 900)    nine hundred Y's in the target alone: a D link
# (stretch length, the starts of its islands)
STRETCHES = ((300, (100,)), (560, (200,)), (300, (60, 200)), (300, (140,)), (120, (50,)), (120, (50,)), (700, (140,)))
BETWEEN = ((10, 0), (40, 0), (50, 900), (50, 1100), (100, 100), (0, 900))
ISLAND = 12
RELATIVE_MEMBERS = 6          # stretches 0 and 1 are one alignment (the ten W's bridged), every other stretch is one
RELATIVE_MERGED = (2, 2, 1, 1, 1, 1)  # per kept alignment the seeds that gave it: the islands of its stretches
RELATIVE_CONFIGS = (dict(band=16, gap_open=11, gap_extend=1, x_drop=30), dict(band=31, gap_open=11, gap_extend=1, x_drop=HUGE))


def relative_pair(seed=2031):
    """-> (query, target, columns): columns is the alignment the construction means, one code per column (=, X, I, D) with the
    replaced stretches left out — they are written per max_fill in relative_cigar."""
    rng = np.random.default_rng(seed)
    letters = FLANK.tolist()
    q, t, cols = b"", b"", []
    for i, (n, islands) in enumerate(STRETCHES):
        s = SC._seq(rng, n, FLANK)
        u = bytearray(s)
        for p in range(3, n - 1, 6):
            if not any(a <= p < a + ISLAND for a in islands):
                u[p] = letters[(letters.index(u[p]) + 1 + p % 5) % len(letters)]
        q += s; t += bytes(u)
        cols.append([EQ if a == b else X for a, b in zip(s, u)])
        if i < len(BETWEEN):
            x, y = BETWEEN[i]
            q += b"W" * x; t += b"Y" * y
    return q, t, cols


def relative_cigar(cols, max_fill, eqx):
    """The stitched CIGAR of relative_pair, from the construction and the comments above alone."""
    out = []
    for i, c in enumerate(cols):
        out += c
        if i < len(BETWEEN):
            x, y = BETWEEN[i]
            if x == 0 or y == 0:
                out += [I] * x + [D] * y
            elif link_class(x, y, max_fill) == "open":
                out += [I] * x + [D] * y
            else:  # the run of the difference first, the mismatched pairs last
                out += ([D] * (y - x) if y > x else [I] * (x - y)) + [X] * min(x, y)
    if not eqx:
        out = [M if c in (EQ, X) else c for c in out]
    runs = []
    for c in out:
        if runs and runs[-1][1] == c:
            runs[-1][0] += 1
        else:
            runs.append([1, c])
    return "".join(f"{n}{'MID'[c] if c < 3 else '=' if c == EQ else 'X'}" for n, c in runs)


def relative_counts(max_fill):
    """-> (n_filled, n_open) of the one row."""
    cls = [link_class(x, y, max_fill) for x, y in BETWEEN if x and y]
    return cls.count("filled"), cls.count("open")


# ---- 3. pairs at the capacity limit -----------------------------------------------------------------------------------------------
CAPACITY = 2 ** 20
K_LONG = 10
CORE = b"WYWWYYWYWWYW"  # the one thing two unrelated sequences share: their random residues hold no W and no Y
Q_CORE_AT, T_CORE_AT = 1000, 1037
DELETED = 20


def unrelated_pair(n=CAPACITY, seed=5):
    """Two random sequences over the flank letters with CORE planted at different offsets."""
    rng = np.random.default_rng(seed)
    q, t = bytearray(SC._seq(rng, n, FLANK)), bytearray(SC._seq(rng, n, FLANK))
    q[Q_CORE_AT:Q_CORE_AT + len(CORE)] = CORE
    t[T_CORE_AT:T_CORE_AT + len(CORE)] = CORE
    return bytes(q), bytes(t)


def shared_kmers(q, t, k=K_LONG):
    """The k-mers two sequences over at most 32 letters share, by numpy: a yardstick for 'unrelated'."""
    def codes(s):
        a = np.frombuffer(s, np.uint8).astype(np.uint64) - 65
        assert a.max() < 32 and 5 * k <= 64
        c = np.zeros(len(a) - k + 1, np.uint64)
        for j in range(k):
            c = (c << np.uint64(5)) | a[j:len(a) - k + 1 + j]
        return c
    return np.intersect1d(codes(q), codes(t))


def all_127():
    return np.full((28, 28), 127, np.int8)


def core_only_matrix():
    """-128 everywhere but +127 for W over W and Y over Y: outside CORE no pair of unrelated_pair scores above -128."""
    m = np.full((28, 28), -128, np.int8)
    m[W, W] = m[Y, Y] = 127
    return m


def deleted_pair(n=CAPACITY, seed=8):
    """-> (full, the same without DELETED residues at the midpoint).  The 400 residues around the midpoint come from a stream of
    their own: they are the same at any n, so the CPU test can show at a small n that both seeds bridge the deletion under
    x_drop = 30.  The residues on either side of the deleted ones differ from those that would let the gap slide."""
    h = n // 2
    mid = bytearray(SC._seq(np.random.default_rng(seed), 400))
    rng = np.random.default_rng(seed + 1)
    full = bytearray(SC._seq(rng, h - 200) + bytes(mid) + SC._seq(rng, n - h - 200))
    for a, b in ((h - 1, h + DELETED - 1), (h, h + DELETED)):
        if full[a] == full[b]:
            full[b] = SC.PROTEIN[(SC.PROTEIN.tolist().index(full[b]) + 1) % 20]
    full = bytes(full)
    assert len(full) == n and full[h - 1] != full[h + DELETED - 1] and full[h] != full[h + DELETED]
    return full, full[:h] + full[h + DELETED:]


def trace_scratch(regions, alignments):
    """The direction scratch the header promises of a traceback: 64 bytes per row, each side's rows rounded up to an even number."""
    total = 0
    for a, n, qs, ql in zip(regions[1].tolist(), regions[3].tolist(), alignments[1].tolist(), alignments[2].tolist()):
        left = a + n // 2 - qs
        right = ql - 1 - left
        total += 64 * ((left + 1) // 2 * 2 + (right + 1) // 2 * 2)
    return total


# ---- 4. real proteins ---------------------------------------------------------------------------------------------------------------
REAL_FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz")
# BNIP3 / BNIP3L and the two protein kinases C (a filled link each way; the kinases chain three members with an open link as
# well), BNIP2 / BNIPL / ATCAY (an open link in each of their six rows), LRRK2 and DAPK1 (the longest self-hits: 2,527 and 1,430
# columns), five of the BCL2 family proper, and three fragments that hold an X.
REAL_ACCESSIONS = ("O60238", "Q12983", "P17252", "Q02156", "Q12982", "Q7Z465", "Q86WG3", "Q5S007", "P53355", "P10415", "Q07812",
                   "Q07817", "Q07820", "Q16611", "H0Y3R5", "H7C142", "H0YA56")


def real_records():
    from oracle import oracle
    by_acc = {n.split("|")[1]: (n, s) for n, s in oracle.read_fasta(REAL_FASTA)}
    return [by_acc[a] for a in REAL_ACCESSIONS]
