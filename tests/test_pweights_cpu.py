"""CPU: the weighting reference (tests/pweights_ref.py) against values written out by hand — the worked example of
include/kmerseek_amd.h with and without the query as a member, the conservation of a column's weight, the weighted build on three
residues — and the property the feature is for: the weighted build does not move when every entry is given d times, the unweighted
one does.  The refusals of the Python and wire layers that need no device; the _lib table names every new symbol.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_cases as PC  # noqa: E402
import pileup_ref as PR  # noqa: E402
import profile_ref  # noqa: E402
import pweights_ref as WR  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, ONE = 28, 1 << 30
cls = lambda ch: ord(ch) - 65  # noqa: E731


def worked_case():
    """the header's example: query ACDE, three entries 4M at start 0 against ACDE, ACDE, AGDK"""
    return PC.build([(0, t, [(0, 0, "4M")]) for t in range(3)], [b"ACDE"], [b"ACDE", b"ACDE", b"AGDK"])


def duplicate_case(d):
    """query AC, the entries 2M against AC and GC, each d times: per column k, the counts and d are powers of two"""
    return PC.build([(0, t, [(0, 0, "2M")] * d) for t in range(2)], [b"AC"], [b"AC", b"GC"])


def passes(case, side="query", include_query=False):
    """the three passes on a case -> (counts, depth, weight, n_cols, S, wdepth, wcounts)"""
    args = PC.ref_args(case, side, True)
    (depth, counts, *_), _ = PR.pileup(**args)
    res = case["q" if side == "query" else "t"][0] if include_query else None
    weight, n_cols, S = WR.weights(args, counts, res)
    base, wdepth, wcounts = WR.weighted_pileup(args, weight)
    PR.assert_same(base, PR.pileup(**args)[0], "the unweighted columns")
    return counts, depth, weight, n_cols, S, wdepth, wcounts


def test_worked_example_by_hand():
    assert ks.KS_WEIGHT_ONE == ONE == _lib.KS_WEIGHT_ONE and ONE // 3 == 357913941 and ONE // 4 == 268435456 and ONE // 2 == 536870912
    counts, depth, weight, n_cols, S, wdepth, wcounts = passes(worked_case())
    assert S == [1252698794, 1252698794, 1789569706] == [2 * 357913941 + 2 * 268435456] * 2 + [2 * 357913941 + 2 * 536870912]
    assert weight.tolist() == [313174698, 313174698, 447392426] and n_cols.tolist() == [4, 4, 4] and weight.dtype == n_cols.dtype == np.uint32
    assert wdepth.tolist() == [2 * 313174698 + 447392426] * 4 and wdepth.dtype == wcounts.dtype == np.uint64
    w = wcounts.reshape(4, A)
    assert w[1, cls("C")] == 2 * 313174698 and w[1, cls("G")] == 447392426 and w[3, cls("K")] == 447392426 and w[0, cls("A")] == wdepth[0]


def test_worked_example_with_the_query_as_a_member():
    """column 0 (and 2): k = 1, n = 4, every term 2^28.  Columns 1 and 3: the query agrees with the two: k = 2, n = 3 for them,
    floor(2^30 / 6) = 178956970 each; n = 1 for the odd one, 2^29."""
    _, _, weight, n_cols, S, _, _ = passes(worked_case(), include_query=True)
    assert ONE // 6 == 178956970
    assert S == [2 * (1 << 28) + 2 * 178956970] * 2 + [2 * (1 << 28) + 2 * (1 << 29)] == [894784852, 894784852, 1610612736]
    assert weight.tolist() == [223696213, 223696213, 402653184] and n_cols.tolist() == [4, 4, 4]


def test_alone_masked_and_without_a_pair_column():
    """an entry alone in each of its columns weighs exactly KS_WEIGHT_ONE; a masked row and an entry of gaps alone weigh 0"""
    case = PC.build([(0, 0, [(0, 0, "3M2I2M")]), (0, 1, [(0, 0, "4M")]), (1, 1, [(1, 0, "2I"), (0, 2, "2M")])], [b"ACDEFGH", b"KLM"], [b"ACDEF", b"WWYY"],
                    row_mask=[1, 0, 1])
    _, _, weight, n_cols, S, _, _ = passes(case)
    assert weight.tolist() == [ONE, 0, 0, ONE] and n_cols.tolist() == [5, 0, 0, 2] and S[1] is None and S[2] is None


def test_near_conservation():
    """entries that all span every column of one sequence: a column's terms sum to 2^30 but for the floors, at most one unit per
    entry: the sum of S lies in (cols * ONE - n_entries * cols, cols * ONE]"""
    rng = np.random.default_rng(5)
    cols, n = 37, 23
    ts = [bytes(rng.choice(np.frombuffer(b"ACDEFGH", np.uint8), cols)) for _ in range(n)]
    case = PC.build([(0, t, [(0, 0, f"{cols}M")]) for t in range(n)], [b"A" * cols], ts)
    for inc in (False, True):
        _, _, weight, n_cols, S, _, _ = passes(case, include_query=inc)
        if inc:  # the query is one more member: its own terms close the sum
            assert cols * ONE - (n + 1) * cols < sum(S) + sum(ONE // (k * c) for k, c in own_terms(case)) <= cols * ONE
        else:
            assert cols * ONE - n * cols < sum(S) <= cols * ONE
        assert (weight <= ONE).all() and (n_cols == cols).all()


def own_terms(case):
    """(k_p, cnt of the query's own class) per column of near_conservation's query, the query counted in"""
    (_, counts, *_), _ = PR.pileup(**PC.ref_args(case, "query", True))
    out = []
    for p, row in enumerate(counts.reshape(-1, A).tolist()):
        row[PR.res_class(int(case["q"][0][p]))] += 1
        out.append((sum(1 for v in row if v), row[PR.res_class(int(case["q"][0][p]))]))
    return out


def test_counts_of_other_entries_are_named():
    case = worked_case()
    args = PC.ref_args(case, "query", True)
    (_, counts, *_), _ = PR.pileup(**args)
    bad = counts.reshape(-1, A).copy()
    bad[1, cls("G")] = 0   # entry 2's column
    bad[3, cls("E")] = 0   # entries 0 and 1
    with pytest.raises(WR.CountsError) as e:
        WR.weights(args, bad)
    assert e.value.entry == 0
    with pytest.raises(WR.CountsError) as e:
        WR.weights(args, np.zeros_like(counts))
    assert e.value.entry == 0


def test_duplicates_do_not_move_the_weighted_build():
    """What the feature is for.  Every entry given d = 4 times: per column k stays, every count and every weight sum scale by
    powers of two that cancel exactly, so wcounts — and with them the scores and the consensus — are the original's bit for bit
    (n_obs, the number of sequences behind the row, is d times the original's by its definition).  The unweighted build moves."""
    m = np.full((A, A), -3, np.int8)
    np.fill_diagonal(m, 7)  # (scores fine enough for 2 against 8 observations under beta = 10 to show)
    params = ks.profile_params(m, beta=10.0, include_query=False)
    one, four = passes(duplicate_case(1)), passes(duplicate_case(4))
    assert one[2].tolist() == [ONE // 2] * 2 and four[2].tolist() == [ONE // 8] * 8
    assert np.array_equal(one[6], four[6]) and np.array_equal(one[5], four[5]) and np.array_equal(one[0] * 4, four[0])
    q = np.frombuffer(b"AC", np.uint8)
    w1, w4 = WR.build(one[0], one[6], one[1], q, params), WR.build(four[0], four[6], four[1], q, params)
    assert np.array_equal(w1[0], w4[0]) and np.array_equal(w1[1], w4[1]) and w1[2].tolist() == [2, 2] and w4[2].tolist() == [8, 8]
    u1, u4 = profile_ref.build(one[0], one[1], q, params), profile_ref.build(four[0], four[1], q, params)
    assert not np.array_equal(u1[0], u4[0])
    assert not np.array_equal(w1[0], profile_ref.matrix_rows(q, m).reshape(-1))  # (and the weighted rows are not the fallback's)


def test_weighted_build_by_hand():
    """bg = 1/2 for A and C, R = 1, beta = 0: r = 2 W_c / W exactly.  Residue 0: nothing observed.  Residue 1: counts but no
    weight (W == 0).  Residue 2: W_A = 3, W_C = 1 and an unmodelled class (G) with the largest weight: r = 3/2 and 1/2, G keeps the
    fallback and takes the consensus."""
    bg = np.zeros(A); bg[cls("A")] = bg[cls("C")] = 0.5
    params = ks.ProfileParams(None, bg, np.ones((A, A)), 0.0, [0.25, 1.0, 4.0], 0, False)
    counts, wcounts = np.zeros((3, A), np.uint32), np.zeros((3, A), np.uint64)
    counts[1, cls("A")] = 2
    counts[2, [cls("A"), cls("C"), cls("G")]] = (1, 1, 1)
    wcounts[2, [cls("A"), cls("C"), cls("G")]] = (3, 1, ONE)
    scores, cons, n_obs = WR.build(counts, wcounts, [0, 2, 3], np.frombuffer(b"wCC", np.uint8), params)
    s = scores.reshape(3, A)
    assert np.array_equal(s[0], profile_ref.matrix_rows(b"W")[0]) and np.array_equal(s[1], profile_ref.matrix_rows(b"C")[0])
    assert (int(s[2][cls("A")]), int(s[2][cls("C")]), int(s[2][cls("G")]), int(s[2][cls("W")])) == (2, 1, -1, -1)
    assert n_obs.tolist() == [0, 0, 2] and cons.tobytes() == b"WCG"  # (residue 1: no weight but the query's own term)
    # the flag: the query's own term floor(2^30 / (2 * 2)) joins W_C; the frequencies are then all but the query's
    params = ks.ProfileParams(None, bg, np.ones((A, A)), 0.0, [0.25, 1.0, 4.0], 0, True)
    s, _, n_obs = WR.build(counts, wcounts, [0, 2, 3], np.frombuffer(b"wCC", np.uint8), params)
    assert n_obs.tolist() == [0, 3, 3] and (int(s[28 + cls("C")]), int(s[28 + cls("A")])) == (2, 0) and int(s[56 + cls("C")]) == 2


def test_python_and_wire_refusals_without_a_device(tmp_path):
    def obj(kind):
        o = kind.__new__(kind)
        o._ctx = o._h = None
        return o
    fa, ha, cg = obj(engine.FrameAlignments), obj(engine.HitAlignments), obj(engine.RegionCigars)
    off = np.zeros(2, np.uint64)
    with pytest.raises(ValueError, match="weights= is not built"):
        engine.Context.pileup(None, fa, None, side="target", offsets=off, weights=np.zeros(1, np.uint32))
    with pytest.raises(ValueError, match="u32 values"):
        engine.Context.pileup(None, ha, None, offsets=off, weights=np.zeros(1, np.float64))
    with pytest.raises(ValueError, match="u32 values"):
        engine.Context.pileup(None, ha, None, offsets=off, weights=[-1])
    ew = engine.Context.entry_weights
    with pytest.raises(ValueError, match="neither"):
        ew(None, cg, None, None, side="both")
    with pytest.raises(TypeError, match="takes a RegionCigars"):
        ew(None, ha, None, None)
    with pytest.raises(TypeError, match="alignments="):
        ew(None, cg, None, None)
    with pytest.raises(TypeError, match="needs the Pileup"):
        ew(None, cg, None, (1, 2), alignments=obj(engine.RegionAlignments))
    with pytest.raises(TypeError, match="offsets=, other_res= and other_off="):
        ew(None, cg, None, obj(engine.Pileup), alignments=obj(engine.RegionAlignments), offsets=off)
    with pytest.raises(ValueError, match="needs res="):
        ew(None, cg, None, obj(engine.Pileup), alignments=obj(engine.RegionAlignments), offsets=off, other_res=b"", other_off=off, include_query=True)
    with pytest.raises(ValueError, match="neither"):
        engine.Context.entry_weights_device(None, None, 0, 0, 0, 0, 0, 0, 0, None, None, 0, 0, 0, 0, 0, 0, 0, 0, side="strand")
    with pytest.raises(ValueError, match="needs d_res"):
        engine.Context.entry_weights_device(None, None, 0, 0, 0, 0, 0, 0, 0, None, None, 0, 1, 5, 0, 0, 0, 0, 0, include_query=True)
    with pytest.raises(TypeError, match="ProfileParams"):
        engine.Context.build_profile(None, obj(engine.Pileup), b"", off, None, weighted=True)
    a = str(tmp_path / "none.fa")
    full = dict(regions=True, gapped=True, cigar=True, cull=True)
    with pytest.raises(ValueError, match="profile_weighting = 'henikoff' needs profile=True"):
        wire.search_extract_kmers_device(a, a, 7, 1, "protein", profile_weighting="henikoff", **full)
    with pytest.raises(ValueError, match="profile_weighting = 'blosum' is none of None, 'henikoff'"):
        wire.search_extract_kmers_device(a, a, 7, 1, "protein", profile=True, profile_weighting="blosum", **full)
    assert wire.PROFILE_WEIGHTINGS == (None, "henikoff")


def test_prototypes_and_table():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    names = ("ks_entry_weights_device", "ks_cigars_pileup_weights", "ks_pweights_n_entries", "ks_pweights_device_weight", "ks_pweights_device_n_cols",
             "ks_pweights_copy_to_host", "ks_pweights_free", "ks_wpileup_device", "ks_cigars_pileup_weighted", "ks_hitalns_pileup_weighted",
             "ks_wpileup_n_weighted", "ks_wpileup_device_wdepth", "ks_wpileup_device_wcounts", "ks_wpileup_copy_to_host",
             "ks_profile_build_weighted_device", "ks_profile_build_weighted_pileup")
    for n in names:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, header)
        assert m and n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    assert not re.search(r"\bks_frames_pileup_weight", header)
    for macro, value in (("KS_WEIGHT_ONE", r"\(1u << 30\)"), ("KS_PWEIGHTS_INCLUDE_QUERY", "1u")):
        assert re.search(r"#define\s+%s\s+%s" % (macro, value), header)
    assert _lib.KS_PWEIGHTS_INCLUDE_QUERY == 1
    # the weighted forms take their siblings' arguments and one pointer
    for sib, w in (("ks_pileup_device", "ks_wpileup_device"), ("ks_cigars_pileup", "ks_cigars_pileup_weighted"),
                   ("ks_hitalns_pileup", "ks_hitalns_pileup_weighted")):
        (res, args), (wres, wargs) = _lib.SIGNATURES[sib], _lib.SIGNATURES[w]
        assert wres is res and wargs[:-2] == args[:-2] + [C.c_void_p] and wargs[-2:] == args[-2:]
    assert _lib.SIGNATURES["ks_pileup_copy_to_host"] == (C.c_int, [C.c_void_p] * 11)
    assert engine.EntryWeights._PREFIX == "pweights" and engine.EntryWeights._COLUMNS == ("weight", "n_cols")
    for prop in ("weight_ptr",):
        assert isinstance(getattr(engine.EntryWeights, prop), property)
    for prop in ("wdepth_ptr", "wcounts_ptr", "n_weighted"):
        assert isinstance(getattr(engine.Pileup, prop), property)
    assert callable(engine.Pileup.weighted_to_host) and "EntryWeights" in ks.__all__ and "KS_WEIGHT_ONE" in ks.__all__


def blosum_like(rng):
    m = rng.integers(-4, 3, (A, A)).astype(np.int8)
    m = np.minimum(m, m.T)
    np.fill_diagonal(m, rng.integers(4, 12, A))
    return m


def wbuild_inputs(rng, lens, big=False):
    """sequences, counts, weighted counts (none for a third of the observed classes: W == 0 among them) and depth"""
    seqs = [bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdwyBXZ*-1", np.uint8), n)) for n in lens]
    n_res = sum(lens)
    counts = rng.integers(0, 4, (n_res, A)).astype(np.uint32) * (rng.random((n_res, A)) < 0.2)
    counts[rng.random(n_res) < 0.33] = 0
    if big and n_res:
        counts[rng.integers(0, n_res, 5), rng.integers(0, A, 5)] = rng.integers(256, 2 ** 32, 5)
    counts = counts.astype(np.uint32)
    wcounts = (counts != 0) * rng.integers(1, 1 << 40, (n_res, A)).astype(np.uint64) * (rng.random((n_res, A)) < 0.67)
    wcounts[rng.random(n_res) < 0.1] = 0
    return seqs, counts, wcounts.astype(np.uint64), np.minimum(counts.sum(axis=1, dtype=np.uint64), 2 ** 32 - 1).astype(np.uint32)


def test_the_column_form_is_the_loop():
    rng = np.random.default_rng(61)
    seqs, counts, wcounts, depth = wbuild_inputs(rng, [40, 0, 75, 1], big=True)
    depth[::7] = 0
    q = np.frombuffer(b"".join(seqs), np.uint8)
    m = blosum_like(rng)
    for inc, beta in ((True, 10.0), (False, 0.25)):
        params = ks.profile_params(m, freq=rng.random(A) + 0.05, beta=beta, include_query=inc)
        loop, cols = WR.build(counts, wcounts, depth, q, params), WR.build_columns(counts, wcounts, depth, q, params)
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(loop, cols))
        assert (loop[2] == 0).any() and (loop[2] > 0).any() and len(set(loop[0].tolist())) > 8
