"""GPU: ks_frames_stitch — the chain of every folded row of a translated search as ONE alignment of the strand's bases, frameshifts
as N ops.  Every array is compared exactly with the plain-loop restatement of tests/fstitch_ref.py, run on the host copies of what
the device pipeline gave the pass (fold, chain, alignments, CIGARs, frames): the worked examples of the header with their CIGARs
written down, rows of 0, 1, 2 and 9 members, links of every class with r = 0, 1, 2 around the lanes and max_fill, whole and in
slices of one link, two fuzz batches whole and in slices, with and without eqx, three frameshift costs, single-frame rows against
Context.stitch_chains, row_score as a rank key, the wire on planted contigs, and every refusal."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffold_ref  # noqa: E402
import fstitch_cases as FC  # noqa: E402
import fstitch_ref as FR  # noqa: E402
import translate_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

K, MOL = FC.K, "protein"
INVALID, CAPACITY = _lib.KS_ERR_INVALID_ARG, _lib.KS_ERR_CAPACITY
M, I, D, EQ, X, N = FR.M, FR.I, FR.D, FR.EQ, FR.X, FR.N
COL = {n: i for i, n in enumerate(FR.NAMES)}
NONE = ffold_ref.NONE


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


class _Pipe:
    """contigs x proteins up to what the frame stitch takes, on the device: the six frames, the frame hits, the alignments the
    cull kept, their paths (with and without eqx, on demand), the fold and the chain over it."""

    def __init__(self, ctx, contigs, proteins, align, chain=None, min_kmers=1):
        self.ctx, self.align = ctx, align
        nt, self.nt_off = ks.pack(contigs)
        self.t = ks.pack(proteins)
        t_res, t_off = self.t
        self.n6, self.n_t = 6 * len(contigs), len(proteins)
        self.frames, self.foff, self.n_res = ctx.translate6(nt, self.nt_off)
        f = (self.frames.ptr, self.foff.ptr, self.n6, self.n_res)
        Q, T = ctx.sketch_batch_device(*f, K, 1, MOL), ctx.sketch_batch(t_res, t_off, K, 1, MOL)
        ix = ctx.index_build(T)
        self.hits = ctx.search(ix, Q)
        qp, tp = ctx.kmer_positions_table_device(*f, K, 1, MOL), ctx.kmer_positions_table(t_res, t_off, K, 1, MOL)
        mp = ctx.match_positions(qp, tp, self.hits)
        rg = ctx.match_regions(mp, min_kmers=min_kmers)
        self.d_t, self.d_to = ctx.to_device(t_res), ctx.to_device(t_off)
        self.batches = (*f, self.d_t.ptr, self.d_to.ptr, self.n_t, len(t_res))
        al = ctx.align_regions_device(rg, self.hits, *self.batches, **align)
        cu = ctx.cull_regions(al)
        self.rg, self.al = cu.take(rg), cu.take(al)
        for o in (cu, al, rg, mp, qp, tp, ix, Q, T):
            o.free()
        self.fold = ctx.fold_frames(self.hits, self.al, self.nt_off)
        self.ch = ctx.chain_frames(self.fold, **(FC.CHAIN if chain is None else chain))
        self.cg = {}
        self.host = dict(fold=self.fold.to_host(), fold_hits=self.fold.hits.to_host(), chain=self.ch.to_host(), al=self.al.to_host(),
                         frames=(self.frames.to_host(np.uint8, self.n_res), self.foff.to_host(np.uint64)))
        self.fq, self.ft = self.host["fold_hits"][:2]

    def cigars(self, eqx):
        if eqx not in self.cg:
            self.cg[eqx] = self.ctx.trace_regions_device(self.rg, self.hits, *self.batches, self.al, eqx=eqx)
        return self.cg[eqx]

    def stitch(self, eqx=False, batches=None, **kw):
        return self.ctx.stitch_frames_device(self.fold, self.ch, self.al, self.cigars(eqx), *(batches or self.batches), eqx=eqx, **kw)

    def ref(self, eqx=False, max_fill=0, cost=FR.DEFAULT_COST, **changed):
        h = {**self.host, "t": self.t, **changed}
        cg = changed.get("cigars") or self.cigars(eqx).to_host()
        return FR.stitch(h["fold"], h["fold_hits"], h["chain"], h["al"], cg, *h["frames"], *h["t"], matrix=self.align.get("matrix"),
                         gap_open=self.align["gap_open"], gap_extend=self.align["gap_extend"], max_fill=max_fill, eqx=eqx, frameshift_cost=cost)

    def check(self, what, eqx=(False, True), max_fill=0, cost=FR.DEFAULT_COST, **kw):
        """Stitched on the device and by the reference, for each eqx -> the device's arrays of the last one."""
        got = None
        for x in eqx:
            st = self.stitch(eqx=x, max_fill=max_fill, frameshift_cost=cost, **kw)
            got = st.to_host()
            assert st.n_rows == len(self.fq) and st.n_ops == len(got[1]) == int(got[0][-1]) and all(p != 0 for p in st.device_ptrs())
            assert st.row_score_ptr == st.device_ptrs()[COL["row_score"]] and st.strings() == FR.strings(got[0], got[1])
            assert all(np.array_equal(a, b) for a, b in zip(st.ops_to_host(), got[:2]))
            want, self.events = self.ref(x, max_fill, cost)
            FR.assert_same(got, want, f"{what} eqx={x}")
            self.last = st.n_slices, st.scratch_bytes
            st.free()
        return got

    def row(self, record, strand, target):
        return int(np.flatnonzero((self.fq == 2 * record + strand) & (self.ft == target))[0])

    def close(self):
        for o in (*self.cg.values(), self.ch, self.fold, self.al, self.rg, self.hits, self.d_t, self.d_to, self.frames, self.foff):
            o.free()


# ---- 1. the hand-written cases ------------------------------------------------------------------------------------------------------
def test_worked_examples(ctx):
    cases = FC.worked_cases()
    start = ctx.pool_stats()["bytes_in_use"]
    p = _Pipe(ctx, [c[1] for c in cases], [c[2] for c in cases], FC.EXACT)
    try:
        got = p.check("worked", eqx=(True, False))
        text = FR.strings(got[0], got[1])
        for i, (name, contig, prot, _, _, want, strand, n_shift) in enumerate(cases):
            r = p.row(i, strand, i)
            assert text[r] == want and got[COL["n_frameshifts"]][r] == n_shift, (name, text[r])
            assert (got[COL["t_start"]][r], got[COL["t_length"]][r], got[COL["s_start"]][r]) == (0, len(prot), int(name.split("pad")[1][0])), name
        # the cost is the caller's: 0 and 2^16 move the score of every row by its N ops and nothing else
        base = p.check("cost 0", eqx=(False,), cost=0)
        top = p.check("cost 2^16", eqx=(True,), cost=2 ** 16)
        assert np.array_equal(base[COL["score"]] - 2 ** 16 * top[COL["n_frameshifts"]].astype(np.int64), top[COL["score"]])
        assert np.array_equal(base[COL["score"]] - 15 * got[COL["n_frameshifts"]].astype(np.int64), got[COL["score"]]) and got[COL["n_frameshifts"]].sum() >= 30
    finally:
        p.close()
    assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 2. rows of 0, 1, 2 and 9 members -------------------------------------------------------------------------------------------------
def test_rows_of_0_1_2_and_9_members(ctx):
    rng = np.random.default_rng(78)
    rt = lambda s: translate_ref.reverse_translate(s, rng)  # noqa: E731
    blocks = [FC.SC._seq(rng, 20, FC.SC.FLANK) for _ in range(9)]
    nine = b"".join(rt(b) + b"C" for b in blocks[:-1]) + rt(blocks[-1])  # eight inserted bases: nine members, the frame moves on each time
    one = FC.SC._seq(rng, 50, FC.SC.FLANK)
    two = FC.SC._seq(rng, 40, FC.SC.FLANK)
    lone = FC.SC._seq(rng, 7, FC.SC.FLANK)  # one shared k-mer: a folded row whose one-k-mer region min_kmers = 2 drops
    none_q, none_t = FC.SC._seq(rng, 20, FC.SC.FLANK) + lone + FC.SC._seq(rng, 20, FC.SC.FLANK), FC.SC._seq(rng, 20, FC.SC.FLANK) + lone + FC.SC._seq(rng, 20, FC.SC.FLANK)
    g2 = rt(two)
    contigs = [nine + b"TT", b"G" + rt(one) + b"T", g2[:60] + b"GG" + g2[60:], rt(none_q)]
    p = _Pipe(ctx, contigs, [b"".join(blocks), one, two, none_t], FC.EXACT, min_kmers=2)
    try:
        got = p.check("member counts", eqx=(True, False))
        rows = [p.row(i, 0, i) for i in range(4)]
        assert [int(got[COL["n_members"]][r]) for r in rows] == [9, 1, 2, 0]
        text = FR.strings(got[0], got[1])
        # (a chance match beside a shift moves a codon from one member to the other: 180 pairs and eight single bases in any case)
        assert re.fullmatch(r"(\d+M1N){8}\d+M", text[rows[0]]) and got[COL["aln_length"]][rows[0]] == 180
        assert got[COL["n_frameshifts"]][rows[0]] == 8 and got[COL["score"]][rows[0]] == 180 - 8 * 15
        assert text[rows[1]] == "50M" and text[rows[2]] == "20M2N20M"
        r0 = rows[3]
        assert got[0][r0 + 1] == got[0][r0] and np.isnan(got[COL["row_score"]][r0]) and not any(int(got[i][r0]) for i in range(2, 18))
    finally:
        p.close()


# ---- 3. links of every class, r = 0, 1, 2 ------------------------------------------------------------------------------------------------
MAX_FILL = 70


def _shapes():
    longs, shorts = (63, 64, 65, MAX_FILL, MAX_FILL + 1), (0, 1, 62, 63, 64)
    shapes = {(a, b) for a in longs for b in shorts}
    shapes |= {(b, a) for a, b in shapes} | {(n, n) for n in (1, 62, 63, 64)}
    return sorted(shapes - {(0, 0)})


def test_links_around_the_lanes_and_max_fill(ctx):
    """Two flanks of 20 residues around x codons of W in the gene and y residues of Y in the protein, and r extra bases behind the
    W's: the link is exactly (c, Y) = (x, y) with a shift of r.  Aligned exactly, nothing of a flank extends into a middle."""
    rng = np.random.default_rng(124)
    shapes = [(x, y, r) for x, y in _shapes() for r in (0, 1, 2)]
    contigs, proteins = [], []
    for x, y, r in shapes:
        a, b = FC.SC._seq(rng, 20, FC.SC.FLANK), FC.SC._seq(rng, 20, FC.SC.FLANK)
        contigs.append(translate_ref.reverse_translate(a, rng) + b"TGG" * x + b"C" * r + translate_ref.reverse_translate(b, rng) + b"TT")
        proteins.append(a + b"Y" * y + b)
    p = _Pipe(ctx, contigs, proteins, FC.EXACT)
    try:
        got = p.check("links", eqx=(True, False), max_fill=MAX_FILL)
        assert set(FR.EVENTS) - {"trimmed", "trimmed_to_nothing"} <= p.events | {"joint_merged"}
        text = FR.strings(got[0], got[1])
        for i, (x, y, r) in enumerate(shapes):
            row = p.row(i, 0, i)
            lo, hi = min(x, y), max(x, y)
            filled = 1 <= lo <= 63 and hi <= MAX_FILL
            v = tuple(int(got[COL[k]][row]) for k in ("n_members", "n_filled", "n_open", "n_trimmed", "n_frameshifts"))
            assert v == (2, int(filled), int(lo >= 1 and not filled), 0, int(r != 0)), (x, y, r, text[row], v)
            shift = f"{r}N" if r else ""
            if not filled:
                assert text[row] == "20M" + (f"{x}I" if x else "") + (f"{y}D" if y else "") + shift + "20M", (x, y, r, text[row])
            else:  # min(x, y) mismatched pairs and one run of the difference
                assert (not r or text[row].endswith(shift + "20M")) and got[COL["aln_length"]][row] == 40 + hi
                assert got[COL["score"]][row] == 40 - lo - ((11 + hi - lo) if x != y else 0) - (15 if r else 0), (x, y, r, text[row])
        assert p.last[0] == 1 and p.last[1] >= 64 * MAX_FILL
        whole = p.check("links", eqx=(False,), max_fill=MAX_FILL)
        sliced = p.check("links sliced", eqx=(False,), max_fill=MAX_FILL, max_scratch_bytes=64 * (MAX_FILL + (MAX_FILL & 1)))
        assert p.last[0] >= 3 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, sliced))
        wide = p.check("links max_fill 0", eqx=(False,))
        assert wide[COL["n_filled"]].sum() > got[COL["n_filled"]].sum() and wide[COL["n_open"]].sum() < got[COL["n_open"]].sum()
    finally:
        p.close()


# ---- 4. the fuzz ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FC.FUZZ)), ids=[F["name"] for F in FC.FUZZ])
def test_fuzz_whole_and_in_slices(ctx, i):
    F = FC.FUZZ[i]
    contigs, proteins = FC.fuzz_batch(F["seed"])
    p = _Pipe(ctx, contigs, proteins, F["align"], chain=F["chain"])
    try:
        assert len(p.fq) <= 300
        whole = p.check(F["name"], max_fill=F["max_fill"])
        assert whole[COL["n_filled"]].sum() > 10 and whole[COL["n_frameshifts"]].sum() > 50 and p.last[0] == 1
        budget = max(64 * (F["max_fill"] + 1), p.last[1] // 4)
        sliced = p.check(F["name"] + " sliced", eqx=(True,), max_fill=F["max_fill"], max_scratch_bytes=budget)
        assert p.last[0] >= 3 and p.last[1] <= budget
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, sliced))
    finally:
        p.close()


# ---- 5. single-frame rows are what the protein stitch gives; row_score ranks ----------------------------------------------------------------
def test_single_frame_rows_equal_stitch_chains_and_row_score_ranks(ctx):
    F = FC.FUZZ[0]
    contigs, proteins = FC.fuzz_batch(F["seed"])
    p = _Pipe(ctx, contigs, proteins, F["align"], chain={})  # (no overlap, no cost: the same chain in bases and in residues)
    try:
        st = p.stitch(max_fill=F["max_fill"])
        got = st.to_host()
        per_frame = ctx.chain_regions(p.al)
        plain = ctx.stitch_chains_device(per_frame, p.al, p.cigars(False), p.hits, *p.batches, max_fill=F["max_fill"])
        pg, pc = plain.to_host(), per_frame.to_host()
        fold, ch = p.host["fold"], p.host["chain"]
        f_src = fold[2]
        n, multi = 0, 0
        for r in range(len(p.fq)):
            src = [int(s) for s in fold[0][3 * r:3 * r + 3] if s != NONE]
            if len(src) != 1:
                continue
            fr = src[0]
            mine = f_src[ch[1][int(ch[0][r]):int(ch[0][r + 1])]].tolist()
            if mine != pc[1][int(pc[0][fr]):int(pc[0][fr + 1])].tolist():
                continue
            a, b = got[1][int(got[0][r]):int(got[0][r + 1])], pg[1][int(pg[0][fr]):int(pg[0][fr + 1])]
            assert np.array_equal(a, b), r
            for mk, pk in (("score", 6), ("identities", 7), ("positives", 8), ("gap_opens", 9), ("gaps", 10), ("aln_length", 11), ("n_members", 12),
                           ("n_filled", 13), ("n_open", 14), ("n_trimmed", 15), ("t_start", 4), ("t_length", 5)):
                assert got[COL[mk]][r] == pg[pk][fr], (r, mk)
            assert got[COL["n_frameshifts"]][r] == 0 and got[COL["nt_length"]][r] == 3 * pg[3][fr]
            n += 1; multi += len(mine) > 1
        assert n >= 8 and multi >= 2, (n, multi)
        # row_score as the rank key of the folded hits
        best = ctx.best_hits(p.fold.hits, k=1, score=st.row_score_ptr)
        bq, bt, _, _ = best.to_host()
        score = got[COL["row_score"]]
        for q in np.unique(p.fq).tolist():
            rows = np.flatnonzero((p.fq == q) & ~np.isnan(score))
            if len(rows):
                top = rows[np.argmax(score[rows])]  # (the first among equals: the lower target)
                assert int(bt[np.flatnonzero(bq == q)[0]]) == int(p.ft[top]), q
        for o in (best, plain, per_frame, st):
            o.free()
    finally:
        p.close()


# ---- 6. the wire on planted contigs ------------------------------------------------------------------------------------------------------
def test_wire_on_planted_contigs(ctx, tmp_path):
    proteins, contigs, truth = FC.planted()
    nt_fa, t_fa = tmp_path / "contigs.fa", tmp_path / "proteins.fa"
    nt_fa.write_bytes(b"".join(b">contig%d\n%s\n" % (i, s) for i, s in enumerate(contigs)))
    t_fa.write_bytes(b"".join(b">prot%d\n%s\n" % (i, s) for i, s in enumerate(proteins)))
    start = ctx.pool_stats()["bytes_in_use"]
    kw = dict(ctx=ctx, gapped=True, gapped_x_drop=20, chain_max_overlap=15)
    rows = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, cigar=True, stitch=True, **kw)
    by = {(r["query_name"], r["strand"], r["match_name"]): r for r in rows}
    for t in truth:
        r = by[(f"contig{t['record']}", "-" if t["reverse"] else "+", f"prot{t['target']}")]
        shifts = [s for s in r["aln_frameshifts"].split(",") if s]
        assert len(shifts) == (1 if t["shifted"] else 0) == r["aln_cigar"].count("N"), (t, r)
        if t["shifted"]:
            pos, n = (int(v) for v in shifts[0].split(":"))
            planted_at = (t["end"] - 1 - 3 * t["m"]) if t["reverse"] else t["start"] + 3 * t["m"]
            assert n == 1 and abs(pos - planted_at) <= 15, (t, r)  # (the overhang bound of tests/test_gpu_ffold.py: 5 residues)
        assert r["aln_score"] >= t["length"] - 2 * K - 15
    plain = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, **kw)
    assert all("aln_cigar" not in r for r in plain) and [r["query_name"] for r in plain] == [r["query_name"] for r in rows]
    top = wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, cigar=True, eqx=True, stitch=True, top_k=1, **kw)
    assert {(r["query_name"], r["strand"]): r["match_name"] for r in top}.items() >= {
        (f"contig{t['record']}", "-" if t["reverse"] else "+"): f"prot{t['target']}" for t in truth}.items()
    assert all("M" not in r["aln_cigar"] for r in top)
    for bad, word in ((dict(stitch=True, cigar=True, gapped=False), "gapped=True"), (dict(stitch=True, gapped=True), "cigar=True")):
        with pytest.raises(ValueError, match=word):
            wire.search_translated_device(str(nt_fa), str(t_fa), K, 1, MOL, ctx=ctx, **bad)
    assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------------
WORDS = {"src": ("outside its folded row's regions", "chain member"), "fsrc": ("names an alignment beyond", "folded region"),
         "fold": ("does not hold its alignment's extents", "folded region"), "strand": ("other strand", "folded region"),
         "row": ("beyond the", "folded row"), "ext": ("does not lie inside its two sequences", "region"),
         "ops": ("do not consume exactly", "region"), "code": ("hold = or X", "region"), "asc": ("ends before the member in front", "chain member")}


def upload_into(ctx, d_ptr, a):
    a = np.ascontiguousarray(a)
    ctx._check(ctx._L.ks_dev_upload(ctx._h, C.c_void_p(int(d_ptr)), a.ctypes.data_as(C.c_void_p), a.nbytes))
    ctx.synchronize()


def test_refusals_name_the_first_offender(ctx):
    """One device column at a time is overwritten with a changed copy (and put back): the reference refuses the same arrays for the
    same reason and names the same index; the pool holds what it held.  Where two members offend in the same way the lower index is
    named.  A target of more than 2^20 residues and a frame batch of fewer frames come from the offsets and counts of the call."""
    cases = [c for c in FC.worked_cases() if c[0].endswith("pad1+")]
    p = _Pipe(ctx, [c[1] for c in cases], [c[2] for c in cases], FC.EXACT)
    try:
        cg = p.cigars(False)
        H = dict(p.host, cigars=cg.to_host())
        ptrs = dict(fold=p.fold.device_ptrs(), chain=p.ch.device_ptrs(), al=p.al.device_ptrs(), cigars=cg.device_ptrs(), fold_hits=p.fold.hits.device_ptrs())
        ch_off, ch_src, n_al = H["chain"][0], H["chain"][1], len(H["al"][1])
        two = int(np.flatnonzero(np.diff(ch_off.astype(np.int64)) == 2)[0])      # a folded row of two members
        j1 = int(ch_off[two]) + 1                                                  # its second chain member, its folded region, its alignment
        fg1, fg0 = int(ch_src[j1]), int(ch_src[j1 - 1])
        g1 = int(H["fold"][2][fg1])
        other = int(np.flatnonzero(np.arange(len(H["fold"][2])) >= H["fold"][1][two + 1])[0]) if H["fold"][1][two + 1] < len(H["fold"][2]) else 0
        op0 = int(H["cigars"][0][g1])
        # a second offender of the same kind behind the first: the last chain member, its folded row, region and alignment
        jL = len(ch_src) - 1
        rL = int(np.searchsorted(ch_off, jL, side="right")) - 1
        fgL = int(ch_src[jL])
        gL = int(H["fold"][2][fgL])
        opL = int(H["cigars"][0][gL])
        otherL = 0 if H["fold"][1][rL] > 0 else len(H["fold"][2]) - 1
        assert jL > j1 and rL > two and gL != g1 and not H["fold"][1][rL] <= otherL < H["fold"][1][rL + 1]
        f = H["fold"]
        changes = [("src", j1, [("chain", 1, j1, other)]), ("src", j1, [("chain", 1, jL, otherL), ("chain", 1, j1, other)]),
                   ("fsrc", fg1, [("fold", 2, fg1, n_al)]),
                   ("fold", fg1, [("fold", 5, fg1, int(f[5][fg1]) + 3)]), ("fold", fg1, [("fold", 4, fg1, int(f[4][fg1]) + 3)]),
                   ("fold", fg1, [("fold", 7, fg1, int(f[7][fg1]) + 3)]), ("fold", fg1, [("fold", 8, fg1, int(f[8][fg1]) + 3)]),
                   ("fold", min(fg1, fgL), [("fold", 5, fgL, int(f[5][fgL]) + 3), ("fold", 4, fg1, int(f[4][fg1]) + 3)]),
                   ("strand", fg0, [("fold", 3, fg0, int(f[3][fg0]) + 3)]),
                   ("row", two, [("fold_hits", 1, two, p.n_t)]), ("row", two, [("fold_hits", 1, rL, p.n_t + 7), ("fold_hits", 1, two, p.n_t)]),
                   ("ext", g1, [("al", 3, g1, 10 ** 6), ("fold", 7, fg1, 3 * 10 ** 6)]),
                   ("ops", g1, [("cigars", 1, op0, int(H["cigars"][1][op0]) + 16)]),
                   ("ops", min(g1, gL), [("cigars", 1, opL, int(H["cigars"][1][opL]) + 16), ("cigars", 1, op0, int(H["cigars"][1][op0]) + 16)]),
                   ("code", g1, [("cigars", 1, op0, (int(H["cigars"][1][op0]) & ~15) | EQ)]),
                   ("asc", j1, [("al", 3, g1, 0), ("fold", 7, fg1, 0), ("al", 4, g1, 1), ("fold", 8, fg1, 3)])]
        idle = ctx.pool_stats()["bytes_in_use"]
        for kind, index, edits in changes:
            changed = {}
            for key, col, at, v in edits:
                cols = list(changed.get(key, H[key]))
                cols[col] = cols[col].copy()
                cols[col][at] = v
                changed[key] = tuple(cols)
                upload_into(ctx, ptrs[key][col], cols[col])
            with pytest.raises(FR.StitchError) as ref:
                p.ref(**changed)
            assert (ref.value.kind, ref.value.index) == (kind, index), (kind, ref.value)
            with pytest.raises(ks.KmerseekError) as e:
                p.stitch()
            words, noun = WORDS[kind]
            assert e.value.status == INVALID and words in str(e.value) and re.search(r"\b%s %d\b" % (noun, index), str(e.value)), (kind, str(e.value))
            assert ctx.pool_stats()["bytes_in_use"] == idle, kind
            for key, col, _, _ in edits:
                upload_into(ctx, ptrs[key][col], H[key][col])
        # what the call's own offsets and counts say: a target of 2^20 + 1 residues (the plan reads offsets, never a residue, before
        # it refuses) and a frame batch that ends behind record 1
        t_res, t_off = p.t
        long_off = t_off.copy()
        long_off[-1] = long_off[-2] + 2 ** 20 + 1
        d_long = ctx.to_device(long_off)
        b = p.batches
        idle_now = ctx.pool_stats()["bytes_in_use"]
        for kind, status, word, batches, changed in (
                ("len", CAPACITY, "more than 2^20 residues", (*b[:5], d_long.ptr, b[6], int(long_off[-1])), dict(t=(t_res, long_off))),
                ("row", INVALID, "beyond the 12 of the frame batch", (b[0], b[1], 12, *b[3:]), dict(frames=(H["frames"][0], H["frames"][1][:13])))):
            with pytest.raises(FR.StitchError) as ref:
                p.ref(**changed)
            assert ref.value.kind == kind and ref.value.index > 0, ref.value
            with pytest.raises(ks.KmerseekError) as e:
                p.stitch(batches=batches)
            assert e.value.status == status and word in str(e.value) and re.search(r"\bfolded row %d\b" % ref.value.index, str(e.value)), str(e.value)
            assert ctx.pool_stats()["bytes_in_use"] == idle_now, kind
        d_long.free()
        got = p.check("after the refusals", eqx=(False,))  # everything is back: the context works
        # one filled link whose directions do not fit
        assert got[COL["n_filled"]].sum() >= 1
        with pytest.raises(ks.KmerseekError) as e:
            p.stitch(max_scratch_bytes=64)
        assert e.value.status == CAPACITY and "max_scratch_bytes allows 64" in str(e.value) and ctx.pool_stats()["bytes_in_use"] == idle
        # eqx on paths traced without it
        with pytest.raises(ks.KmerseekError) as e:
            ctx.stitch_frames_device(p.fold, p.ch, p.al, cg, *p.batches, eqx=True)
        assert e.value.status == INVALID and "trace with KS_RTRACE_EQX" in str(e.value)

        # before any device work
        L = ctx._L
        out = C.c_void_p()
        b = p.batches

        def call(c=ctx._h, fold=p.fold._h, hits=p.fold.hits._h, ch=p.ch._h, al=p.al._h, cigars=cg._h, opts=None, out_p=C.byref(out), f_off=b[1]):
            return L.ks_frames_stitch(c, fold, hits, ch, al, cigars, C.c_void_p(b[0]), C.c_void_p(f_off) if f_off else None, b[2], b[3], C.c_void_p(b[4]),
                                      C.c_void_p(b[5]), b[6], b[7], opts, out_p)
        for o in (_lib.ks_fstitch_opts(4097, 0, 15, 0, 0), _lib.ks_fstitch_opts(0, 2, 15, 0, 0), _lib.ks_fstitch_opts(0, 0, 2 ** 16 + 1, 0, 0),
                  _lib.ks_fstitch_opts(0, 0, 15, 1, 0)):
            assert call(opts=C.byref(o)) == INVALID and "frame stitch options" in L.ks_last_error(ctx._h).decode()
            assert call(c=None, opts=C.byref(o)) == INVALID and not out.value
        assert call(c=None) == INVALID
        for kw in (dict(fold=None), dict(hits=None), dict(ch=None), dict(al=None), dict(cigars=None), dict(out_p=None), dict(f_off=0)):
            assert call(**kw) == INVALID and "NULL" in L.ks_last_error(ctx._h).decode(), kw
        assert call(hits=p.hits._h) == INVALID and "objects of other regions" in L.ks_last_error(ctx._h).decode()  # the frame hits, not the folded
        per_frame = ctx.chain_regions(p.al)
        assert call(ch=per_frame._h) == INVALID and "objects of other regions" in L.ks_last_error(ctx._h).decode()
        per_frame.free()
        with ks.Context(0) as other_ctx:
            assert call(c=other_ctx._h) == INVALID and "another context" in L.ks_last_error(other_ctx._h).decode()
        ok = _lib.ks_fstitch_opts(0, 0, 2 ** 16, 0, 0)
        assert call(opts=C.byref(ok)) == _lib.KS_OK and out.value
        L.ks_framealns_free(out)
        assert ctx.pool_stats()["bytes_in_use"] == idle
    finally:
        p.close()
