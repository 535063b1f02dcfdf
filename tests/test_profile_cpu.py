"""CPU: the profile's yardstick and its Python layer, no device.

The build rule of tests/profile_ref.py against values worked out by hand; its three profile passes against the matrix references
(a profile that IS a matrix) and its gapped program against the enumeration of every path on small rectangles; profile_params; the
refusals Python makes before any device call; the ctypes table."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_ref as PR  # noqa: E402
import ralign_ref  # noqa: E402
import rscore_ref  # noqa: E402
import rtrace_cases as RC  # noqa: E402
import rtrace_ref  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

A = 28
cls = lambda ch: ord(ch) - 65


def hand_params(beta, include_query):
    """A and C modelled at 1/2 each; R = 2 on the diagonal, 1/2 off it; thresholds 1/2, 1, 2 above a base of -1"""
    bg = np.zeros(A); bg[cls("A")] = bg[cls("C")] = 0.5
    ratio = np.full((A, A), 0.5); np.fill_diagonal(ratio, 2.0)
    m = np.array(ralign_ref.default_matrix(), np.int8)
    m[cls("A"), cls("W")] = 7
    return ks.ProfileParams(m, bg, ratio, beta, [0.5, 1.0, 2.0], -1, include_query)


def test_the_build_rule_by_hand():
    q = np.frombuffer(b"aCA", np.uint8)
    counts = np.zeros((3, A), np.uint32)
    counts[1, cls("A")] = 1                      # one observation, of another class than the residue's own
    counts[2, cls("W")] = 3                      # an unmodelled class alone
    depth = [0, 1, 3]
    m = np.array(ralign_ref.default_matrix()); m[cls("A"), cls("W")] = 7
    # beta = 0, the query not counted: r = (cnt[c] / n) / bg[c]
    s, cons, nobs = PR.build(counts, depth, q, hand_params(0.0, False))
    s = s.reshape(3, A)
    assert s[0].tolist() == m[cls("A")].tolist() and cons[0] == ord("A") and nobs[0] == 0   # depth 0: the matrix row, own byte upper-cased
    want = m[cls("C")].copy(); want[cls("A")] = -1 + 3; want[cls("C")] = -1 + 0             # r = 2 passes all three thresholds, r = 0 none
    assert s[1].tolist() == want.tolist() and nobs[1] == 1
    assert cons[1] == ord("A")                                                              # A 1, C 0 + 1: a tie goes to the smaller class
    assert s[2].tolist() == m[cls("A")].tolist() and s[2][cls("W")] == 7 and nobs[2] == 0   # n0 == 0: nothing modelled was observed
    assert cons[2] == ord("W")                                                              # W 3 against A 0 + 1
    # the query counted once: n = 2, both r = (1 / 2) / (1 / 2) = 1: two thresholds
    s, cons, nobs = PR.build(counts, depth, q, hand_params(0.0, True))
    s = s.reshape(3, A)
    assert (s[1][cls("A")], s[1][cls("C")], nobs[1]) == (1, 1, 2) and nobs[2] == 0 and s[2].tolist() == m[cls("A")].tolist()
    # beta = 2, residue 1: A: g = 2, t = 2 -> 1 -> 2, num = 3, den = 3, r = 2;  C: g = 1/2, t = 1/2 -> 1/4 -> 1/2, r = (1/2 / 3) / (1/2) = 1/3
    s, _, _ = PR.build(counts, depth, q, hand_params(2.0, False))
    assert (s.reshape(3, A)[1][cls("A")], s.reshape(3, A)[1][cls("C")]) == (2, -1)
    # an unmodelled class observed beside a modelled one: its own entry stays the matrix's, the modelled ones move
    counts[2, cls("A")] = 1
    s, cons, nobs = PR.build(counts, [0, 1, 4], q, hand_params(0.0, False))
    s = s.reshape(3, A)
    assert (s[2][cls("W")], s[2][cls("A")], s[2][cls("C")], s[2][cls("D")], nobs[2], cons[2]) == (7, 2, -1, -1, 1, ord("W"))
    # the clamp and class 27's letter
    p = hand_params(0.0, False); p.base = 200
    assert PR.build(counts, [0, 1, 4], q, p)[0].reshape(3, A)[2][cls("A")] == 127
    p.base = -200
    assert PR.build(counts, [0, 1, 4], q, p)[0].reshape(3, A)[2][cls("C")] == -127
    counts[0, 27] = 5
    assert PR.build(counts, [5, 1, 4], q, hand_params(0.0, False))[1][0] == ord("X")
    assert PR.build(counts, [0, 1, 4], np.frombuffer(b"-CA", np.uint8), hand_params(0.0, False))[1][0] == ord("-")


def blosum_like(rng):
    """a symmetric int8 matrix with a negative expected score: 4 .. 11 on the diagonal, -4 .. 2 beside it"""
    m = rng.integers(-4, 3, (A, A)).astype(np.int8)
    m = np.minimum(m, m.T)
    np.fill_diagonal(m, rng.integers(4, 12, A))
    return m


def build_inputs(rng, n_res, big=False):
    """(q_res, counts, depth): a third of the residues unobserved, odd bytes among them, counts over all 28 classes"""
    q = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdwyBXZ*-1", np.uint8), n_res)
    counts = rng.integers(0, 4, (n_res, A)).astype(np.uint32) * (rng.random((n_res, A)) < 0.2)
    counts[rng.random(n_res) < 0.33] = 0
    if big and n_res:
        counts[rng.integers(0, n_res, 5), rng.integers(0, A, 5)] = rng.integers(256, 2 ** 32, 5)
    counts = counts.astype(np.uint32)
    return q, counts, np.minimum(counts.sum(axis=1, dtype=np.uint64), 2 ** 32 - 1).astype(np.uint32)


def test_the_column_form_of_the_build_rule_is_the_loop():
    rng = np.random.default_rng(11)
    m = blosum_like(rng)
    for beta, inc, freq in ((10.0, True, None), (0.0, False, rng.random(A)), (0.37, True, rng.random(A))):
        p = ks.profile_params(m, freq=freq, beta=beta, include_query=inc)
        q, counts, depth = build_inputs(rng, 160, big=True)
        want, got = PR.build(counts, depth, q, p), PR.build_columns(counts, depth, q, p)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        assert len(set(want[0].tolist())) > 8 and (want[2] == 0).any() and (want[2] > 255).any()
    assert [len(c) for c in PR.build_columns(np.zeros((0, A)), [], b"", p)] == [0, 0, 0]


def random_rows(rng, n, lo=-4, hi=6):
    return rng.integers(lo, hi, (n, A)).astype(np.int8)


def enumerate_paths(x, y):
    """every sequence of P (pair), I (query only), D (target only) from (0, 0) to (x, y)"""
    if x == 0 and y == 0:
        yield ()
        return
    if x and y:
        for p in enumerate_paths(x - 1, y - 1):
            yield p + ("P",)
    if x:
        for p in enumerate_paths(x - 1, y):
            yield p + ("I",)
    if y:
        for p in enumerate_paths(x, y - 1):
            yield p + ("D",)


def path_score(path, Q, T, o, e):
    x = y = s = 0
    for op, run in itertools.groupby(path):
        n = len(list(run))
        if op == "P":
            for _ in range(n):
                s += int(Q[x][0][ralign_ref.residue_class(T[y])]); x += 1; y += 1
        else:
            s -= o + n * e
            x, y = (x + n, y) if op == "I" else (x, y + n)
    return s


@pytest.mark.parametrize("o,e", [(0, 0), (0, 1), (2, 1), (11, 1)])
def test_the_profile_program_against_every_path(o, e):
    """Rectangles up to 5 x 5, the band wide enough to hold them: H of every end cell is the best score over all paths to it
    (position-specific rows: equal query residues score differently), the traced path re-scores to it, and without an X-drop
    the best cell is the largest of them, the smallest x, then the smallest y."""
    rng = np.random.default_rng(100 + 10 * o + e)
    for trial in range(6):
        X, Y = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        rows = random_rows(rng, X).tolist()
        Q = [(rows[i], ord("A")) for i in range(X)]  # one residue, X different rows
        T = bytes(RC.PROTEIN[rng.integers(0, 20, Y)])
        best = {}
        for x in range(X + 1):
            for y in range(Y + 1):
                best[(x, y)] = max(path_score(p, Q, T, o, e) for p in enumerate_paths(x, y))
                steps, h = PR.trace_extension(Q, T, x, y, 5, o, e)
                assert h == best[(x, y)], (trial, x, y)
                path = tuple({"P": "P", "I": "I", "D": "D"}[s[0]] for s in steps[::-1])
                assert path_score(path, Q, T, o, e) == h and (sum(c != "D" for c in path), sum(c != "I" for c in path)) == (x, y)
        top = max(best.values())
        cell = min(c for c, v in best.items() if v == top)
        got = PR.gapped_extend(Q, T, 5, o, e, 2 ** 20)
        assert (got[0], got[1], got[2]) == (cell[0], cell[1], top)


def _regions_of(queries, targets, rng, per_row=3):
    """hand-made hit rows and seeds (every (q, t) pair, seeds of 1 .. 4 residues anywhere): the references need no device"""
    q, t = ks.pack(queries), ks.pack(targets)
    offs, qs, ts, ln, qid, tid = [0], [], [], [], [], []
    for i, a in enumerate(queries):
        for j, b in enumerate(targets):
            qid.append(i); tid.append(j)
            for _ in range(per_row):
                n = int(rng.integers(1, min(4, len(a), len(b)) + 1))
                qs.append(int(rng.integers(0, len(a) - n + 1))); ts.append(int(rng.integers(0, len(b) - n + 1))); ln.append(n)
            offs.append(len(qs))
    regions = (np.array(offs, np.uint64), np.array(qs, np.uint32), np.array(ts, np.uint32), np.array(ln, np.uint32))
    return q, t, regions, np.array(qid, np.uint32), np.array(tid, np.uint32)


def test_a_profile_that_is_a_matrix_gives_the_matrix_references():
    rng = np.random.default_rng(7)
    qs, ts = RC.two_letter_batch(3, 2, 3, 8, 30)
    qs.append(b"acD*-xW"); ts.append(b"ACd*-XwW")
    q, t, regions, qid, tid = _regions_of(qs, ts, rng)
    m = rng.integers(-5, 6, (A, A)).astype(np.int8)
    P = PR.matrix_rows(q[0], m)
    for ext, xd in ((False, 0), (True, 0), (True, 3), (True, 2 ** 32 - 1)):
        want = rscore_ref.score(regions, qid, tid, q[0], q[1], t[0], t[1], matrix=m, extend=ext, x_drop=xd)
        got = PR.score(regions, qid, tid, q[0], q[1], t[0], t[1], P, extend=ext, x_drop=xd)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    for kw in ({"band": 0, "gap_open": 0, "gap_extend": 0, "x_drop": 2}, {"band": 3, "gap_open": 1, "gap_extend": 1, "x_drop": 4},
               {"band": 31, "gap_open": 0, "gap_extend": 1, "x_drop": 2 ** 20}):
        want = ralign_ref.align(regions, qid, tid, q[0], q[1], t[0], t[1], matrix=m, **kw)
        got = PR.align(regions, qid, tid, q[0], q[1], t[0], t[1], P, **kw)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        kw.pop("x_drop")
        for eqx in (False, True):
            wc = rtrace_ref.trace(regions, want, qid, tid, q[0], q[1], t[0], t[1], matrix=m, eqx=eqx, **kw)
            assert PR.trace(regions, got, qid, tid, q[0], q[1], t[0], t[1], P, eqx=eqx, **kw) == [c for c, _ in wc]


def test_profile_params():
    p = ks.profile_params(None)
    assert p.base == -9 and len(p.thresholds) == 18 and (np.diff(p.thresholds) > 0).all() and p.include_query and p.beta == 10.0
    assert sorted(np.flatnonzero(p.bg > 0).tolist()) == sorted(ks.engine.STANDARD_CLASSES) and abs(p.bg.sum() - 1) < 1e-12
    rng = np.random.default_rng(3)
    m = blosum_like(rng)
    freq = rng.random(A) + 0.1
    p = ks.profile_params(m, freq=freq, beta=1e300, include_query=False)
    assert p.base == int(m.min()) - 8 and p.base + len(p.thresholds) == int(m.max()) + 8 and (np.diff(p.thresholds) > 0).all()
    assert p.bg[cls("B")] == 0 and p.bg[26] == 0 and abs(p.bg[cls("A")] / p.bg[cls("C")] - freq[cls("A")] / freq[cls("C")]) < 1e-12
    # one observed residue and a prior that outweighs everything: r -> R[a][c] = exp(lambda M[a][c]), the row is the matrix's
    for a in ks.engine.STANDARD_CLASSES:
        counts = np.zeros((1, A), np.uint32); counts[0, a] = 1
        s, cons, nobs = PR.build(counts, [1], bytes([65 + a]), p)
        assert s.tolist() == m[a].tolist() and cons[0] == 65 + a and nobs[0] == 1
    # and with no prior at all an observed class scores high, an unobserved one hits the floor
    p0 = ks.profile_params(m, freq=freq, beta=0.0, include_query=False)
    s, _, _ = PR.build(counts, [1], b"Y", p0)
    assert s[cls("Y")] > m[cls("Y"), cls("Y")] and s[cls("A")] == p0.base and s[cls("B")] == m[cls("Y"), cls("B")]
    for bad in ({"freq": np.zeros(A)}, {"freq": np.ones(5)}, {"freq": -np.ones(A)}, {"beta": -1.0}, {"beta": float("nan")}):
        with pytest.raises(ValueError):
            ks.profile_params(m, **bad)


def test_python_refusals_without_a_device():
    ok = dict(matrix=None, bg=np.full(A, 1 / A), ratio=np.ones((A, A)), beta=1.0, thresholds=[1.0, 2.0], base=0)
    ks.ProfileParams(**ok)
    nan_ratio = np.ones((A, A)); nan_ratio[3, 4] = np.nan
    for bad in ({"thresholds": [1.0, 1.0]}, {"thresholds": [2.0, 1.0]}, {"thresholds": [1.0, float("nan")]}, {"thresholds": np.arange(255.0)},
                {"bg": -np.ones(A)}, {"bg": np.ones(5)}, {"ratio": np.ones((A, 5))}, {"ratio": nan_ratio}, {"beta": -0.5}, {"base": 2 ** 31},
                {"matrix": np.zeros((A, A), np.int32)}):
        with pytest.raises(ValueError):
            ks.ProfileParams(**{**ok, **bad})
    assert len(ks.ProfileParams(**{**ok, "thresholds": np.arange(254.0)}).thresholds) == 254
    # profile= is a Profile, and excludes matrix=: refused before the context is looked at
    fake = ks.Profile.__new__(ks.Profile)
    fake._h = None
    m = np.zeros((A, A), np.int8)
    for fn in (ks.Context.score_regions, ks.Context.align_regions, ks.Context.score_regions_device, ks.Context.align_regions_device):
        n_batch = 4 if fn.__name__.endswith("regions") else 8
        with pytest.raises(ValueError, match="exclusive"):
            fn(None, None, None, *[None] * n_batch, matrix=m, profile=fake)
        with pytest.raises(TypeError, match="Profile"):
            fn(None, None, None, *[None] * n_batch, profile=m)
    with pytest.raises(TypeError, match="Profile"):
        ks.Context.trace_regions(None, None, None, None, None, None, None, None, profile="no")
    for fn in (ks.Context.build_profile, ks.Context.build_profile_device):
        with pytest.raises(TypeError, match="ProfileParams"):
            fn(None, *[None] * (3 if fn is ks.Context.build_profile else 6), params={"beta": 1})
    with pytest.raises(ValueError, match="int8"):
        ks.Context.profile_from_host(None, np.zeros((3, A), np.int32), 1)


def test_the_wire_refuses_by_name_before_it_reads_a_file():
    base = dict(regions=True, gapped=True, cigar=True, cull=True)
    call = lambda **kw: wire.search_extract_kmers_device("no.fasta", "no.fasta", 7, 1, "protein", ctx=object(), profile=True, **kw)
    for missing in base:
        with pytest.raises(ValueError, match=f"profile=True needs {missing}=True"):
            call(**{**base, missing: False})
    for name, more in (("stitch", {"stitch": True, "chain": True, "hit_rows": True}), ("evalue", {"evalue": True, "stat_params": (0.3, 0.1)}),
                       ("coverage", {"coverage": "target"})):
        with pytest.raises(ValueError, match=f"profile=True with {name}"):
            call(**{**base, **more})
    with pytest.raises(ValueError, match="profile_beta"):
        call(profile_beta=-1.0, **base)
    with pytest.raises(ValueError, match="pssm needs cull"):
        wire.region_rows([], [], [], [], tuple(np.zeros(1 if i == 0 else 0, np.uint64) for i in range(6)), "protein", pssm=((), ()))


def test_the_lib_table():
    names = ["ks_profile_build_device", "ks_profile_build_pileup", "ks_profile_from_host", "ks_profile_n_seqs", "ks_profile_n_residues",
             "ks_profile_n_scores", "ks_profile_device_scores", "ks_profile_device_consensus", "ks_profile_device_n_obs", "ks_profile_copy_to_host",
             "ks_profile_free", "ks_regions_score_profile", "ks_regions_align_profile", "ks_regions_traceback_profile", "ks_raligns_by_profile"]
    for n in names:
        assert n in _lib.SIGNATURES, n
    # a profile pass takes its sibling's arguments and the profile in front of the options
    for sib in ("ks_regions_score", "ks_regions_align", "ks_regions_traceback"):
        res, args = _lib.SIGNATURES[sib]
        pres, pargs = _lib.SIGNATURES[sib + "_profile"]
        assert pres is res and len(pargs) == len(args) + 1 and pargs[:-3] + pargs[-2:] == args and pargs[-3] is C.c_void_p
    o = _lib.ks_profile_opts
    assert [f[0] for f in o._fields_] == ["matrix", "bg", "ratio", "beta", "thresholds", "n_thr", "base", "flags", "reserved"]
    assert C.sizeof(o) == 56 and o.beta.offset == 24 and o.n_thr.offset == 40 and o.reserved.offset == 52
    assert ks.Profile._COLUMNS == ("scores", "consensus", "n_obs") and ks.Profile._PREFIX == "profile"
    assert _lib.KS_PROFILE_INCLUDE_QUERY == 1 and _lib.KS_PROFILE_MAX_THRESHOLDS == 254
