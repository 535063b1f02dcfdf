"""CPU: the inputs of tests/test_gpu_region_extents.py are what tests/rextent_cases.py says they are, shown with the reference
restatements alone — and rstitch_ref.fill, which shares its recurrence with the library, is held to an independent global
affine-gap optimum (gotoh_global below) at the sizes ks_regions_stitch is built for, where brute force over every path (4 x 4 in
test_region_stitch_cpu.py) cannot go.  The GPU test imports gotoh_global and holds the device to it as well."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rextent_cases as EC  # noqa: E402
import rstitch_ref as SR  # noqa: E402
import rtrace_ref  # noqa: E402
from ralign_ref import default_matrix  # noqa: E402

M, I, D, EQ, X = SR.M, SR.I, SR.D, SR.EQ, SR.X
NEG = -(1 << 60)


def gotoh_global(qst, tst, matrix, o, e):
    """The best score of a global alignment of two byte strings, a gap of L costing o + L * e and a pair
    matrix[class(query byte)][class(target byte)]: the textbook three matrices, H = max(D, E, F) with E and F both opened from
    H, one row of the longer string at a time and the row vectorised over the shorter one.  Written apart from rtrace_ref on
    purpose: no shared code, no tie rules, only the score.  Within a row E[j] = max over j' < j of H[j'] - o - (j - j') * e is a
    running maximum of H[j'] + j' * e; H[j'] may be replaced by max(D, F)[j'] there, since an E opened from an E is the longer
    E with one more o >= 0 paid."""
    def classes(s):
        a = np.frombuffer(bytes(s), np.uint8).astype(np.int64)
        a = np.where((a >= 97) & (a <= 122), a - 32, a)
        return np.where((a >= 65) & (a <= 90), a - 65, np.where(a == 42, 26, 27))
    S = np.asarray(matrix, np.int64)[np.ix_(classes(qst), classes(tst))]
    if S.shape[0] < S.shape[1]:
        S = S.T  # (the gap costs are the same for both strings: the optimum does not care which one the rows walk)
    n, m = S.shape
    j = np.arange(m + 1, dtype=np.int64)
    H = np.where(j == 0, 0, -o - j * e)
    F = np.full(m + 1, NEG, np.int64)
    for i in range(n):
        F = np.maximum(H - o - e, F - e)
        G = F.copy()
        G[1:] = np.maximum(G[1:], H[:-1] + S[i])
        run = np.maximum.accumulate(G + j * e)
        H = G
        H[1:] = np.maximum(G[1:], run[:-1] - o - j[1:] * e)
    return int(H[m])


def test_gotoh_global_on_paper():
    m = default_matrix()
    assert gotoh_global(b"", b"", m, 11, 1) == 0 and gotoh_global(b"AAA", b"", m, 11, 1) == -14 == gotoh_global(b"", b"AAA", m, 11, 1)
    assert gotoh_global(b"ACD", b"ACD", m, 11, 1) == 3 and gotoh_global(b"KLM", b"WY", m, 11, 1) == -2 - 12
    assert gotoh_global(b"ACDEF", b"ACF", m, 1, 1) == 3 - 3 and gotoh_global(b"ACF", b"ACDEF", m, 1, 1) == 0
    assert gotoh_global(b"AWA", b"AA", m, 0, 0) == 2 and gotoh_global(b"WW", b"YYY", m, 1, 0) == -2  # I x 2 and D x 3, no pair
    a = np.array(m, np.int8)
    a[0, 2], a[2, 0] = 5, -7  # A over C is not C over A
    assert gotoh_global(b"A", b"C", a, 11, 1) == 5 and gotoh_global(b"C", b"A", a, 11, 1) == -7
    rng = np.random.default_rng(3)
    for _ in range(40):  # and against the reference's full table on small random rectangles, ties and all
        qst, tst = EC.SC._seq(rng, int(rng.integers(1, 9)), EC.SC.TWO), EC.SC._seq(rng, int(rng.integers(1, 9)), EC.SC.TWO)
        o, e = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        assert SR.fill(qst, tst, m, o, e, False)[1] == gotoh_global(qst, tst, m, o, e), (qst, tst, o, e)


def test_the_fill_memo_is_the_reference():
    rng = np.random.default_rng(4)
    m = [[int(v) for v in row] for row in EC.random_matrix(6).tolist()]
    for x, y in ((9, 4), (3, 11), (5, 5)):
        qst, tst = EC.SC._seq(rng, x, EC.SC.TWO), EC.SC._seq(rng, y, EC.SC.TWO)
        for eqx in (False, True, False):
            for mat, o, e in ((m, 3, 1), (default_matrix(), 1, 0)):
                got, want = EC.FILLS(qst, tst, mat, o, e, eqx), SR.fill(qst, tst, mat, o, e, eqx)
                assert (got[0], got[1], got[2], got[3]) == (want[0], want[1], want[2], want[3])
    with EC.FILLS:
        assert SR.fill is EC.FILLS
    assert SR.fill is EC.FILLS.orig


# ---- 1. long fills ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(EC.long_sides()))
def test_mismatch_fills(group):
    """Every shape has the class the header gives it at max_fill 0, 1024 and 4096; a filled one scores what the closed form
    and the independent optimum say; an open one is I x X then D x Y."""
    shapes, qs, ts = EC.mismatch_batch(EC.long_sides()[group], seed=11)
    P = EC.cpu_stages(qs, ts, **EC.EXACT)
    assert P["hits"][0].tolist() == P["hits"][1].tolist() == list(range(len(shapes)))  # pair i hits pair i alone
    assert P["alignments"][0].tolist() == list(range(0, 2 * len(shapes) + 1, 2))
    m = default_matrix()
    by_fill = {}
    for max_fill in (0, 1024, 4096):
        got, _ = EC.ref_stitch(P, max_fill=max_fill)
        text = SR.strings(got[0], got[1])
        for r, (x, y) in enumerate(shapes):
            cigar, score, n_filled, n_open, opens, length = EC.mismatch_row(x, y, max_fill)
            assert (got[12][r], got[13][r], got[14][r], got[15][r]) == (2, n_filled, n_open, 0), (x, y, max_fill)
            assert (got[6][r], got[9][r], got[11][r]) == (score, opens, length), (x, y, max_fill, text[r])
            assert cigar is None or text[r] == cigar
            if n_filled:
                qm, tm = EC.middles(qs[r], ts[r])
                assert EC.FILLS(qm, tm, m, 11, 1, False)[1] == gotoh_global(qm, tm, m, 11, 1) == score - 60
        by_fill[max_fill] = got
    SR.assert_same(by_fill[0], by_fill[1024], "max_fill 0 is 1024")
    # the header's rule at its three boundaries, literally
    want = {(1025, 0): "open", (1025, 4096): "filled", (4097, 0): "open", (4097, 4096): "open"}
    for (hi, mf), cls in want.items():
        assert all(EC.link_class(hi, lo, mf) == cls == EC.link_class(lo, hi, mf) for lo in (1, 2, 63))
    assert all(EC.link_class(hi, 64, mf) == "open" for hi in (127, 1024, 4096) for mf in (0, 4096))


def test_one_link_per_slice_by_the_header():
    """The batch the GPU test stitches under a budget of one 4096-row link: eight filled links, eight slices by the header's
    rule, and one row less refuses the link in front of chain member 1."""
    shapes, _, _ = EC.mismatch_batch(*EC.SLICED[:1], seed=13, shorts=EC.SLICED[1])
    rows = [r for x, y in shapes for r in (0, (max(x, y) + 1) // 2 * 2 if EC.link_class(x, y, 4096) == "filled" else 0)]
    assert len(shapes) == 8 and rows == [0, 4096] * 8 and EC.slices_of(rows, 4096) == 8 and EC.slices_of(rows, 4095) == -1 - 1
    assert EC.slices_of(rows, 2 * 4096) == 4 and EC.slices_of(rows, 1 << 24) == 1


@pytest.mark.parametrize("gaps", EC.PATH_GAPS, ids=lambda g: f"gap{g[0]}_{g[1]}")
@pytest.mark.parametrize("seeded", (False, True), ids=("plus_minus_1", "seeded_matrix"))
def test_path_fills(seeded, gaps):
    """Middles with a real path: the alignments are the flanks, the link is the two middles, filled at max_fill = 4096; the
    reference's fill scores the independent optimum, through gap runs of thousands of rows."""
    o, e = gaps
    matrix = EC.path_matrix(17) if seeded else None
    m = default_matrix() if matrix is None else [[int(v) for v in row] for row in matrix.tolist()]
    shapes, qs, ts = EC.path_batch(seed=23)
    P = EC.cpu_stages(qs, ts, **dict(EC.EXACT, gap_open=o, gap_extend=e, matrix=matrix))
    al = P["alignments"]
    assert P["hits"][0].tolist() == P["hits"][1].tolist() == list(range(len(shapes))) and len(al[1]) == 2 * len(shapes)
    got, ev = EC.ref_stitch(P, matrix=matrix, gap_open=o, gap_extend=e, max_fill=4096)
    assert {"filled", "filled_swapped"} <= ev and (got[13] == 1).all() and (got[14] == 0).all() and (got[15] == 0).all()
    longest = 0
    for r, (x, y) in enumerate(shapes):
        assert (al[1][2 * r], al[2][2 * r], al[3][2 * r], al[4][2 * r]) == (0, 30, 0, 30)            # the flank in front
        assert (al[1][2 * r + 1], al[2][2 * r + 1], al[3][2 * r + 1], al[4][2 * r + 1]) == (30 + x, 30, 30 + y, 30)  # and behind
        qm, tm = EC.middles(qs[r], ts[r])
        assert (len(qm), len(tm)) == (x, y)
        best = gotoh_global(qm, tm, m, o, e)
        assert EC.FILLS(qm, tm, m, o, e, False)[1] == best == int(got[6][r]) - int(al[5][2 * r]) - int(al[5][2 * r + 1]), (x, y)
        ops = got[1][int(got[0][r]):int(got[0][r + 1])]
        longest = max(longest, int((ops[(ops & 15) != M] >> 4).max()))
    # +1 / -1 with a gap open of 11: a run is never split (a pair inside it gains at most 1 and opens a second gap), so the
    # 4,033 rows without a partner are one run, or two where the copy lies in the middle: dozens of stages of 64 rows
    assert seeded or o != 11 or longest >= (4096 - 63) // 2
    assert o != 1 or "tie_F" in ev or "tie_E" in ev


# ---- 2. the pair of relatives ---------------------------------------------------------------------------------------------------------
def test_relative_pair_from_the_references_alone():
    q, t, cols = EC.relative_pair()
    assert 2500 < len(q) < 3000 and 5000 < len(t) < 6500
    t0 = time.perf_counter()
    P = EC.cpu_stages([q], [t], chain=EC.CHAIN, **EC.RELATIVE_CONFIGS[0])
    cg_eqx = EC.cigars_of(P, True)
    rows = {}
    for max_fill in (0, 4096):
        for eqx in (False, True):
            rows[(max_fill, eqx)] = EC.ref_stitch(P, max_fill=max_fill, eqx=eqx, cigars=cg_eqx if eqx else None)[0]
    took = time.perf_counter() - t0
    print(f"reference pipeline of the relative pair: {took:.1f} s")
    n_islands = sum(len(i) for _, i in EC.STRETCHES)
    assert len(P["regions"][1]) == n_islands and P["hits"][0].tolist() == [0]       # the islands are the only seeds
    assert P["cull"][3].tolist() == list(EC.RELATIVE_MERGED)                          # the islands of one stretch: one alignment
    assert len(P["chain"][1]) == EC.RELATIVE_MEMBERS and P["chain"][1].tolist() == list(range(EC.RELATIVE_MEMBERS))
    for (max_fill, eqx), got in rows.items():
        assert SR.strings(got[0], got[1]) == [EC.relative_cigar(cols, max_fill, eqx)], (max_fill, eqx)
        assert (got[12][0], got[13][0], got[14][0], got[15][0]) == (EC.RELATIVE_MEMBERS, *EC.relative_counts(max_fill), 0)
        assert (got[2][0], got[3][0], got[4][0], got[5][0]) == (0, len(q), 0, len(t))
    assert EC.relative_counts(0) == (1, 2) and EC.relative_counts(4096) == (2, 1)
    # the hand-written strings, spelled out where they are short enough to read: the links of the M version
    plain = EC.relative_cigar(cols, 0, False)
    assert plain == "300M10I560M40I300M850D350M50I1100D120M100I100D120M900D700M"
    assert EC.relative_cigar(cols, 4096, False) == "300M10I560M40I300M850D350M1050D170M100I100D120M900D700M"
    assert EC.relative_cigar(cols, 0, True).startswith("3=1X5=1X") and "850D50X3=1X" in EC.relative_cigar(cols, 0, True)
    # a traced side of more than eight stages of 64 rows: the seed of stretch 0 walks right through stretch 1
    sides = [(a + n // 2 - qs, ql - 1 - (a + n // 2 - qs)) for a, n, qs, ql in
             zip(P["kept_regions"][1].tolist(), P["kept_regions"][3].tolist(), P["alignments"][1].tolist(), P["alignments"][2].tolist())]
    assert max(max(s) for s in sides) > 8 * 64
    assert took < 10.0


# ---- 3. the pairs at the capacity limit ---------------------------------------------------------------------------------------------
def test_unrelated_pair_shares_the_core_alone():
    q, t = EC.unrelated_pair()
    assert len(q) == len(t) == 2 ** 20
    core = EC.shared_kmers(EC.CORE, EC.CORE)
    assert len(core) == len(EC.CORE) - EC.K_LONG + 1 and np.array_equal(EC.shared_kmers(q, t), core)
    assert q[EC.Q_CORE_AT - 1] != t[EC.T_CORE_AT - 1] and q[EC.Q_CORE_AT + 12] != t[EC.T_CORE_AT + 12]
    assert not (set(q) | set(t)) & set(b"WY") - set(EC.CORE) and q.count(b"W") == EC.CORE.count(b"W")


def test_deleted_pair_is_bridged_from_both_seeds():
    """At 2,048 residues, where the references can follow: the 400 residues around the deletion are those of the pair of 2^20,
    everything else is an exact match at any length.  Both seeds cross the deletion under x_drop = 30 and give the same
    alignment; the cull keeps one."""
    n = 2048
    full, cut = EC.deleted_pair(n)
    big, _ = EC.deleted_pair(4096)
    assert full[n // 2 - 200:n // 2 + 200] == big[2048 - 200:2048 + 200]
    P = EC.cpu_stages([full], [full, cut], k=EC.K_LONG, band=31, gap_open=11, gap_extend=1, x_drop=30)
    assert P["hits"][1].tolist() == [0, 1] and P["regions"][0].tolist() == [0, 1, 3] and P["cull"][3].tolist() == [1, 2]
    a, b = n // 2, n - n // 2 - EC.DELETED
    assert [rtrace_ref.cigar_string(c) for c, _ in P["traced"]] == [f"{n}M", f"{a}M{EC.DELETED}I{b}M"]
    assert P["alignments"][5].tolist() == [n, n - EC.DELETED - (11 + EC.DELETED)]
    full, cut = EC.deleted_pair()
    assert len(full) == 2 ** 20 and len(cut) == 2 ** 20 - EC.DELETED
    assert len(EC.shared_kmers(full, full)) == 2 ** 20 - EC.K_LONG + 1  # no 10-mer occurs twice: one seed per diagonal


# ---- 4. real proteins ---------------------------------------------------------------------------------------------------------------
def test_real_subset_meets_its_conditions():
    recs = EC.real_records()
    seqs = [s for _, s in recs]
    assert len(recs) == len(EC.REAL_ACCESSIONS) <= 40
    assert any(set(s.upper()) - set(b"ACDEFGHIKLMNPQRSTVWY") for s in seqs)  # a residue outside the twenty letters
    t0 = time.perf_counter()
    P = EC.cpu_stages(seqs, seqs, chain=EC.CHAIN, **EC.PROBE)
    got, ev = EC.ref_stitch(P)
    took = time.perf_counter() - t0
    print(f"reference pipeline of the real subset: {took:.1f} s; {len(P['hits'][0])} hit rows, {len(P['alignments'][1])} alignments, "
          f"{int(got[13].sum())} filled and {int(got[14].sum())} open links, longest alignment {int(P['alignments'][10].max())} columns")
    assert got[13].sum() >= 3 and got[14].sum() >= 3 and got[12].max() >= 3 and P["alignments"][10].max() >= 2000
    assert {"filled", "filled_swapped", "open"} <= ev
    odd = [i for i, s in enumerate(seqs) if b"X" in s.upper()]
    assert any(q != t and (q in odd or t in odd) for q, t in zip(P["hits"][0].tolist(), P["hits"][1].tolist()))  # and it is aligned
    assert took <= 10.0
