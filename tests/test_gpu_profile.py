"""GPU: the profile — ks_profile_build_device and the three region passes against a profile of the query batch.

Everything is compared exactly.  The build against tests/profile_ref.py (the loop on small batches, its column form — which
test_profile_cpu.py holds against the loop — on the fuzz).  The passes: a profile that IS a matrix against the matrix entry
points, bit for bit, on the case sets of the align and traceback tests; position-specific rows, the staging chunk, the ungapped
step, both ends of the batch and the bands 0 and 31 against the reference's own loops; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_ref as PR  # noqa: E402
import ralign_ref  # noqa: E402
import rtrace_cases as RC  # noqa: E402
import test_gpu_region_align as TA  # noqa: E402  (its crafted batches around the staging chunk)
import test_gpu_region_trace as TT  # noqa: E402  (its _Case: the device objects up to the regions)

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib  # noqa: E402

A = 28
HUGE = RC.HUGE
DEFAULTS = {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30}
cls = lambda ch: ord(ch) - 65


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


# ---- 1. the build ---------------------------------------------------------------------------------------------------------------
def blosum_like(rng):
    m = rng.integers(-4, 3, (A, A)).astype(np.int8)
    m = np.minimum(m, m.T)
    np.fill_diagonal(m, rng.integers(4, 12, A))
    return m


def check_build(ctx, seqs, counts, depth, params, ref=PR.build):
    q_res, q_off = ks.pack(seqs)
    counts = np.asarray(counts, np.uint32).reshape(len(q_res), A)
    prof = ctx.build_profile((counts, depth), q_res, q_off, params)
    assert (prof.n_seqs, prof.n_residues, prof.n_scores) == (len(seqs), len(q_res), A * len(q_res))
    got, want = prof.to_host(), ref(counts, depth, q_res, params)
    for g, w, name in zip(got, want, ks.Profile._COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.flatnonzero(g != w)[:5].tolist(), g[:30].tolist(), w[:30].tolist())
    assert prof.consensus_strings(q_off) == [bytes(want[1][int(q_off[i]):int(q_off[i + 1])]).decode("latin-1") for i in range(len(seqs))]
    assert prof.scores_ptr == prof.device_ptrs()[0] and (prof.scores_ptr != 0 or len(q_res) == 0)
    prof.free()
    return want


def build_inputs(rng, lens, big=False):
    seqs = [bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdwyBXZ*-1", np.uint8), n)) for n in lens]
    n_res = sum(lens)
    counts = rng.integers(0, 4, (n_res, A)).astype(np.uint32) * (rng.random((n_res, A)) < 0.2)
    counts[rng.random(n_res) < 0.33] = 0
    if big and n_res:
        counts[rng.integers(0, n_res, 5), rng.integers(0, A, 5)] = rng.integers(256, 2 ** 32, 5)
    counts = counts.astype(np.uint32)
    return seqs, counts, np.minimum(counts.sum(axis=1, dtype=np.uint64), 2 ** 32 - 1).astype(np.uint32)


@pytest.mark.parametrize("include_query", [True, False])
def test_build_small_batches(ctx, include_query):
    """empty; 1, 2, 3 and 65 residues (a wave takes two); depth 0 and counts beyond a byte among them; both flags"""
    rng = np.random.default_rng(40 + include_query)
    m = blosum_like(rng)
    params = ks.profile_params(m, freq=rng.random(A) + 0.1, beta=3.5, include_query=include_query)
    check_build(ctx, [], np.zeros((0, A)), [], params)
    check_build(ctx, [b"", b""], np.zeros((0, A)), [], params)
    for lens in ((1,), (2,), (1, 0, 2), (65,), (33, 32)):
        seqs, counts, depth = build_inputs(rng, lens, big=True)
        counts[0, cls("L")] = 300
        depth[0] = counts[0].sum()
        want = check_build(ctx, seqs, counts, depth, params)
        assert want[2][0] >= 300


def test_build_every_class_and_unmodelled_observations(ctx):
    """all 28 classes as the residue, every one with a depth of 0, with modelled and with unmodelled classes observed"""
    rng = np.random.default_rng(43)
    seq = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*-"
    assert sorted(ralign_ref.residue_class(b) for b in seq) == list(range(A))
    m = rng.integers(-128, 128, (A, A)).astype(np.int8)  # (the fallback may hold any int8)
    p = ks.profile_params(blosum_like(rng), beta=10.0)
    params = ks.ProfileParams(m, p.bg, p.ratio, p.beta, p.thresholds, p.base, True)
    counts = np.zeros((3 * A, A), np.uint32)
    for i in range(A):
        np.add.at(counts[A + i], [cls("A"), cls("L"), i], np.array((2, 1, 3), np.uint32))  # modelled classes, and the residue's own
        counts[2 * A + i, [cls("B"), 26, 27]] = (1 + i % 2, 2, 1)    # unmodelled classes alone: n0 == 0 at a depth > 0
    want = check_build(ctx, [seq, seq + seq], counts, counts.sum(axis=1), params)
    s = want[0].reshape(3 * A, A)
    assert np.array_equal(s[:A], m[[ralign_ref.residue_class(b) for b in seq]]) and np.array_equal(s[2 * A:], s[:A]) and (want[2][2 * A:] == 0).all()
    assert not np.array_equal(s[A:2 * A], s[:A]) and want[1][:A].tobytes() == seq and chr(want[1][2 * A + 1]) in "B*"


def test_build_thresholds_edges_and_the_clamp(ctx):
    """beta = 0 and bg = 1/2: r = 2 cnt[c] / n is exact.  r == a threshold counts it; one ulp below the next one does not."""
    bg = np.zeros(A); bg[cls("A")] = bg[cls("C")] = 0.5
    ratio = np.ones((A, A))
    up = float(np.nextafter(1.0, 2.0))
    counts = np.zeros((2, A), np.uint32)
    counts[0, [cls("A"), cls("C")]] = (1, 1)     # r = 1 for both
    counts[1, [cls("A"), cls("C")]] = (3, 1)     # r = 3/2 and 1/2
    for thr, base, want_rows in (([0.25, 1.0, up, 4.0], 0, ((2, 2), (3, 1))), ([up], 5, ((5, 5), (6, 5))), ([1.0], -3, ((-2, -2), (-2, -3))),
                                 ([0.25, 0.5], 126, ((127, 127), (127, 127))), ([0.25, 0.5], -130, ((-127, -127), (-127, -127))),
                                 ([], 9, ((9, 9), (9, 9))), (list(np.linspace(0.01, 1.4, 254)), -100, None)):
        params = ks.ProfileParams(None, bg, ratio, 0.0, thr, base, False)
        want = check_build(ctx, [b"GG"], counts, [2, 4], params)
        s = want[0].reshape(2, A)
        if want_rows:
            assert tuple((int(s[i][cls("A")]), int(s[i][cls("C")])) for i in range(2)) == want_rows, (thr, base)
            assert s[0][cls("G")] == 1 and s[0][cls("W")] == -1  # unmodelled: the fallback, here +1 / -1


def test_build_fuzz(ctx):
    """300 sequences of 0 .. 700 residues, the flag on and off, against the column form of the reference"""
    rng = np.random.default_rng(44)
    lens = rng.integers(0, 701, 300).tolist()
    seqs, counts, depth = build_inputs(rng, lens, big=True)
    m = blosum_like(rng)
    for inc, beta in ((True, 10.0), (False, 0.25)):
        params = ks.profile_params(m, freq=rng.random(A) + 0.05, beta=beta, include_query=inc)
        want = check_build(ctx, seqs, counts, depth, params, ref=PR.build_columns)
        assert len(set(want[0].tolist())) > 12 and (want[2] == 0).any()


def test_build_from_a_pileup_and_its_refusals(ctx):
    """ks_profile_build_pileup on a real query-side pileup; options, NULLs, other batches: refused, nothing left in the pool"""
    rng = np.random.default_rng(45)
    qs, ts, _ = RC.indel_batch(1, 71)
    case = TT._Case(ctx, qs, ts, RC.INDEL_K)
    al = case.align(**DEFAULTS)
    cg = case.trace(al)
    pu = ctx.pileup(cg, case.hits, side="query", offsets=case.q[1], alignments=al, profile=True, other_res=case.t[0], other_off=case.t[1])
    params = ks.profile_params(blosum_like(rng), beta=2.0)
    prof = ctx.build_profile(pu, case.q[0], case.q[1], params)
    host = pu.to_host()
    want = PR.build(host[1], host[0], case.q[0], params)
    assert all(np.array_equal(g, w) for g, w in zip(prof.to_host(), want)) and (want[2] > 1).any()
    prof.free()
    before = ctx.pool_stats()["bytes_in_use"]
    plain = ctx.pileup(cg, case.hits, side="query", offsets=case.q[1], alignments=al)
    with pytest.raises(ks.KmerseekError, match="without KS_PILEUP_PROFILE"):
        ctx.build_profile(plain, case.q[0], case.q[1], params)
    plain.free()
    with pytest.raises(ks.KmerseekError, match="another batch"):
        ctx.build_profile(pu, case.t[0], case.t[1], params)
    n = len(case.q[0])
    with pytest.raises(ks.KmerseekError, match="end at"):
        ctx.build_profile((np.zeros((n + 1, A), np.uint32), np.zeros(n + 1, np.uint32)), np.append(case.q[0], 65), case.q[1], params)
    # the options come first, also with no context at all
    L = _lib.load()
    opts, keep = params._opts()
    out = C.c_void_p()
    bad = []
    for field, value in (("flags", 2), ("reserved", 1), ("n_thr", 255), ("beta", -1.0), ("beta", float("nan"))):
        o, _ = params._opts()
        setattr(o, field, value)
        bad.append(o)
    desc, _ = params._opts()
    two = (C.c_double * 2)(2.0, 1.0)
    desc.thresholds, desc.n_thr = C.cast(two, C.POINTER(C.c_double)), 2
    neg = (C.c_double * A)(*([0.1] * 27 + [-0.1]))
    nbg, _ = params._opts()
    nbg.bg = C.cast(neg, C.POINTER(C.c_double))
    for o in bad + [desc, nbg]:
        for c in (None, ctx._h):
            assert L.ks_profile_build_device(c, None, None, None, None, 0, 0, C.byref(o), C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_profile_build_device(ctx._h, None, None, None, None, 0, 0, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert L.ks_profile_build_device(ctx._h, None, None, None, None, 0, 5, C.byref(opts), C.byref(out)) == _lib.KS_ERR_INVALID_ARG  # NULL pointers
    assert ctx.pool_stats()["bytes_in_use"] == before
    for o in (pu, cg, al):
        o.free()
    case.close()


# ---- the passes -------------------------------------------------------------------------------------------------------------------
def profile_of(ctx, case, P, matrix=None):
    return ctx.profile_from_host(np.ascontiguousarray(P, np.int8).reshape(-1, A), len(case.q[1]) - 1, matrix=matrix)


def run_profile(case, prof, eqx=(False, True), **kw):
    """-> (alignment columns, {eqx: (op_offsets, ops)}) of the profile passes on the case's regions"""
    al = case.ctx.align_regions(case.rg, case.hits, *case.q, *case.t, profile=prof, **kw)
    assert al.by_profile and al.n_regions == case.rg.n_regions
    out = {}
    for x in eqx:
        cg = case.ctx.trace_regions(case.rg, case.hits, *case.q, *case.t, al, eqx=x, profile=prof)
        out[x] = cg.to_host()
        cg.free()
    host = al.to_host()
    al.free()
    return host, out


def check_against_ref(case, P, what="", eqx=(False, True), rescored=True, **kw):
    """align and trace against the profile rows P on the device == the reference's loops on the same regions; the device's ops,
    replayed under P, give the alignment's own score and counts"""
    prof = profile_of(case.ctx, case, P)
    got, cigars = run_profile(case, prof, eqx=eqx, **kw)
    prof.free()
    full = {**DEFAULTS, **kw}
    h = case.hits_host
    want = PR.align(case.regions, h[0], h[1], *case.q, *case.t, P, **full)
    for g, w, name in zip(got, want, ralign_ref.COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, kw, name, g.tolist()[:20], w.tolist()[:20])
    tkw = {k: v for k, v in full.items() if k != "x_drop"}
    for x in eqx:
        w_offs, w_ops = TT.encode(PR.trace(case.regions, got, h[0], h[1], *case.q, *case.t, P, eqx=x, **tkw))
        assert np.array_equal(cigars[x][0], w_offs) and np.array_equal(cigars[x][1], w_ops), (what, kw, x)
        TT.check_invariants(got, cigars[x][0], cigars[x][1], x)
    if rescored:
        rows = np.asarray(P).reshape(-1, A).tolist()
        offs, ops = cigars[eqx[0]]
        roffs = case.regions[0].tolist()
        qb, tb = bytes(case.q[0]), bytes(case.t[0])
        for r in range(len(roffs) - 1):
            q, t = int(h[0][r]), int(h[1][r])
            q0, q1, t0, t1 = int(case.q[1][q]), int(case.q[1][q + 1]), int(case.t[1][t]), int(case.t[1][t + 1])
            for g in range(roffs[r], roffs[r + 1]):
                cg = [(int(v) >> 4, int(v) & 15) for v in ops[int(offs[g]):int(offs[g + 1])]]
                rs = PR.rescore(cg, qb[q0:q1], tb[t0:t1], rows[q0:q1], int(got[1][g]), int(got[3][g]), full["gap_open"], full["gap_extend"])
                assert rs == (got[5][g], got[6][g], got[7][g], got[8][g], got[9][g], got[10][g], got[2][g], got[4][g]), (what, kw, g)
    return got, cigars


def positional_rows(q_res, matrix, rng, own_lo=2, own_hi=6, noise=0.3):
    """matrix rows made position-specific: the residue's own class scores own_lo .. own_hi - 1 by position, and a share of the
    other entries moves by -2 .. 2: two positions with the same residue hold different rows"""
    P = PR.matrix_rows(q_res, matrix).astype(np.int64)
    n = len(P)
    own = [ralign_ref.residue_class(int(b)) for b in q_res]
    P += rng.integers(-2, 3, P.shape) * (rng.random(P.shape) < noise)
    P[np.arange(n), own] = rng.integers(own_lo, own_hi, n)
    return np.clip(P, -128, 127).astype(np.int8)


# ---- 2. a profile that is a matrix gives the matrix entry points, bit for bit ----------------------------------------------------
def equivalence(ctx, case, m, score_opts, align_opts):
    P = PR.matrix_rows(case.q[0], m)
    prof = profile_of(ctx, case, P, matrix=m)
    for kw in score_opts:
        a = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, matrix=m, **kw)
        b = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, profile=prof, **kw)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a.to_host(), b.to_host())), kw
        a.free(); b.free()
    for kw in align_opts:
        a = ctx.align_regions(case.rg, case.hits, *case.q, *case.t, matrix=m, **kw)
        assert not a.by_profile
        want = a.to_host()
        got, cigars = run_profile(case, prof, **kw)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(got, want)), kw
        for x in (False, True):
            cg = ctx.trace_regions(case.rg, case.hits, *case.q, *case.t, a, eqx=x)
            assert all(np.array_equal(u, v) for u, v in zip(cg.to_host(), cigars[x])), (kw, x)
            cg.free()
        a.free()
    prof.free()


SCORE_OPTS = ({}, {"extend": True, "x_drop": 0}, {"extend": True, "x_drop": 3}, {"extend": True, "x_drop": 2 ** 32 - 1})


@pytest.mark.parametrize("side", [1, -1])
def test_equivalence_around_the_chunk(ctx, side):
    q, t, names = TA.crafted_batch(side)
    case = TT._Case(ctx, [bytes(q[0][int(q[1][i]):int(q[1][i + 1])]) for i in range(len(q[1]) - 1)],
                    [bytes(t[0][int(t[1][i]):int(t[1][i + 1])]) for i in range(len(t[1]) - 1)], 7)
    equivalence(ctx, case, TA.flank_matrix(), SCORE_OPTS,
                ({"band": 0, "gap_open": 0, "gap_extend": 0, "x_drop": 2}, {"band": 1, "gap_open": 1, "gap_extend": 1, "x_drop": 2}, DEFAULTS,
                 {"band": 31, "gap_open": 2, "gap_extend": 1, "x_drop": HUGE}, {"band": 31, "gap_open": 0, "gap_extend": 0, "x_drop": 3}))
    equivalence(ctx, case, None, SCORE_OPTS[:2], (DEFAULTS,))
    case.close()


def test_equivalence_on_indels_ties_and_an_asymmetric_matrix(ctx):
    for W in RC.INDEL_BANDS:
        qs, ts, _ = RC.indel_batch(W, 70 + W)
        case = TT._Case(ctx, qs, ts, RC.INDEL_K)
        equivalence(ctx, case, TT.random_matrix(W), SCORE_OPTS[2:], ({"band": W, **RC.INDEL_OPTS}, {"band": W, "gap_open": 20, "gap_extend": 3, "x_drop": 200}))
        equivalence(ctx, case, None, (), ({"band": W, **RC.INDEL_OPTS},))
        case.close()
    for o, e in ((0, 0), (0, 1), (1, 1)):
        qs, ts = RC.fuzz_batch(o, e)
        case = TT._Case(ctx, qs, ts, RC.FUZZ_K)
        equivalence(ctx, case, None, SCORE_OPTS, [{"gap_open": o, "gap_extend": e, **kw} for kw in RC.FUZZ_OPTS])
        case.close()
    qs, ts = RC.k1_batch()  # thousands of regions in one row, seeds of one residue, sequences of one residue
    case = TT._Case(ctx, qs, ts, 1)
    equivalence(ctx, case, TT.random_matrix(9), SCORE_OPTS[1:3], RC.K1_OPTS)
    case.close()


# ---- 3. position-specific rows change the path and the X-drop -------------------------------------------------------------------
def shifted_case():
    """-> (q0, t0, P for the queries [q0, q0], r0).  t0 is q0 with every fifth flank residue replaced: no seed but CORE, and an
    ungapped walk that gains 3 in 5 under +1 / -1.  Query 0: from residue 10 of the right flank on, the row of position i pays the
    target residue ONE FURTHER (+8) and fines the residue opposite (-8).  Query 1: rows 30 .. 35 of the right flank fine everything.
    The flanks repeat residues (60 positions over 20 letters): equal residues, different rows."""
    rng = np.random.default_rng(50)
    seq = lambda n: bytes(RC.PROTEIN[rng.integers(0, 20, n)])
    left, right = seq(40), seq(60)
    q0 = left + RC.CORE + right
    r0 = len(left) + len(RC.CORE)
    other = lambda b: int(RC.PROTEIN[(bytes(RC.PROTEIN).index(b) + 7) % 20])
    t0 = bytes(other(b) if (i < len(left) or i >= r0) and i % 5 == 2 else b for i, b in enumerate(q0))
    P = PR.matrix_rows(np.frombuffer(q0 + q0, np.uint8), None).copy()
    for i in range(r0 + 10, len(q0) - 1):
        P[i, :] = -2
        P[i, ralign_ref.residue_class(t0[i])] = -8
        P[i, ralign_ref.residue_class(t0[i + 1])] = 8
    P[len(q0) + r0 + 30:len(q0) + r0 + 36, :] = -9
    return q0, t0, P, r0


def test_position_specific_rows_move_the_diagonal_and_the_x_drop(ctx):
    """The gapped path of query 0 opens a gap of one and goes on along the next diagonal, where the matrix form has no gap; the
    ungapped extension of query 1 ends before its fined rows, that of query 0 where its rows turn."""
    q0, t0, P, r0 = shifted_case()
    case = TT._Case(ctx, [q0, q0], [t0], 7)
    assert case.rg.n_regions == 2 and case.hits_host[0].tolist() == [0, 1]  # (the seed: CORE and a residue or two beside it)
    kw = {"band": 4, "gap_open": 11, "gap_extend": 1, "x_drop": 40}
    got, cigars = check_against_ref(case, P, "diagonal", **kw)
    strings = ks.engine.cigar_strings(*cigars[False])
    assert strings[0].count("D") == 1 and "I" not in strings[0] and (got[8][0], got[9][0]) == (1, 1) and got[5][0] > 8 * 40
    assert got[4][0] == got[2][0] + 1 and "D" not in strings[1] and "I" not in strings[1]  # one target residue skipped; query 1 has no reason
    under_matrix = case.align(**kw)
    cg = case.trace(under_matrix)
    assert not any(c in text for text in cg.strings() for c in "DI") and under_matrix.to_host()[2][0] > got[2][0] - 8
    # the ungapped X-drop
    prof = profile_of(ctx, case, P)
    h = case.hits_host
    for xd in (20, 53, 2 ** 32 - 1):
        sc = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, profile=prof, extend=True, x_drop=xd)
        want = PR.score(case.regions, h[0], h[1], *case.q, *case.t, P, extend=True, x_drop=xd)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(sc.to_host(), want)), xd
        sc.free()
        ends = (want[1] + want[3]).tolist()  # (six rows of -9 are a dip of 54 that the 24 residues behind them never make good)
        assert r0 <= ends[0] <= r0 + 12 and r0 + 25 <= ends[1] <= r0 + 30, (xd, ends)
    plain = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, extend=True, x_drop=20)
    assert ((plain.to_host()[1] + plain.to_host()[3]) >= len(q0) - 3).all()
    for o in (plain, prof, cg, under_matrix):
        o.free()
    case.close()


# ---- 4. geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, -1])
def test_staged_rows_across_the_chunk_and_the_ungapped_step(ctx, side):
    """The batches of the traceback's end-cell test: extensions that end at row 63, 64, 65 and 129 on either side, with and
    without an indel in the flank.  W over M scores 1 + (position mod 3): a row staged from the wrong position changes a score."""
    c, step = int(_lib.load().ks_debug_ralign_chunk()), int(_lib.load().ks_debug_rscore_step())
    assert c == step == 64
    core_rows = 5 if side > 0 else 6  # the rest of CORE beyond the anchor CORE[6]
    flanks = sorted({T - core_rows for T in (c - 1, c, c + 1, 2 * c + 1)} | {step - 1, step, step + 1})  # gapped rows / ungapped pairs
    Ts = [f + core_rows for f in flanks]
    targets = [(b"NNN" + RC.CORE + b"M" * f) if side > 0 else (b"M" * f + RC.CORE + b"NNN") for f in flanks]
    targets += [(b"NNN" + RC.CORE + b"M" * 30 + b"N" * 2 + b"M" * f) if side > 0 else (b"M" * f + b"N" * 2 + b"M" * 30 + RC.CORE + b"NNN")
                for f in flanks[:4]]
    case = TT._Case(ctx, [b"W" * 150 + RC.CORE + b"W" * 150], targets, 7)
    assert case.regions[0].tolist() == list(range(len(targets) + 1))
    P = PR.matrix_rows(case.q[0], TA.flank_matrix()).copy()
    P[:, cls("M")] = np.where(case.q[0] == ord("W"), 1 + np.arange(len(P)) % 3, P[:, cls("M")])
    got, _ = check_against_ref(case, P, "band 0", band=0, gap_open=0, gap_extend=0, x_drop=HUGE)
    anchor = case.regions[1] + case.regions[3] // 2
    x_end = (got[1] + got[2] - 1 - anchor) if side > 0 else (anchor - got[1])
    assert x_end.tolist()[:len(Ts)] == Ts and {c - 1, c, c + 1, 2 * c + 1} <= set(Ts)
    for kw in ({"band": 1, "gap_open": 1, "gap_extend": 1, "x_drop": HUGE}, DEFAULTS, {"band": 31, "gap_open": 2, "gap_extend": 1, "x_drop": HUGE},
               {"band": 31, "gap_open": 0, "gap_extend": 0, "x_drop": 3}):
        check_against_ref(case, P, "gapped", eqx=(False,), **kw)
    # the ungapped walk: the flanks are its pairs beyond the core, 63, 64 and 65 among them
    prof = profile_of(ctx, case, P)
    h = case.hits_host
    for xd in (0, 2, 2 ** 32 - 1):
        sc = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, profile=prof, extend=True, x_drop=xd)
        want = PR.score(case.regions, h[0], h[1], *case.q, *case.t, P, extend=True, x_drop=xd)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(sc.to_host(), want)), xd
        sc.free()
    ext = (want[1] + want[3] - (case.regions[1] + case.regions[3])) if side > 0 else (case.regions[1] - want[1])
    assert ext.tolist()[:len(flanks)] == flanks and {step - 1, step, step + 1} <= set(flanks)
    prof.free()
    case.close()


def test_both_ends_of_the_batch_and_the_bands(ctx):
    """Identical queries and targets of 1 .. 400 residues, rows that pay the residue's own class by position: the alignment of
    (i, i) runs from the first residue to the last — the left extension of the first sequence down to row 0 of the profile, the
    right one of the last sequence to row n_res - 1 — under the bands 0 and 31."""
    rng = np.random.default_rng(51)
    seqs = [bytes(RC.PROTEIN[rng.integers(0, 20, n)]) for n in (70, 1, 7, 64, 65, 129, 400)]
    case = TT._Case(ctx, seqs, seqs, 7)
    P = positional_rows(case.q[0], None, rng)
    offs, n_res = case.q[1].tolist(), len(case.q[0])
    rows = {(q, t): r for r, (q, t) in enumerate(zip(case.hits_host[0].tolist(), case.hits_host[1].tolist()))}
    for kw in ({"band": 0, "gap_open": 0, "gap_extend": 0, "x_drop": HUGE}, {"band": 31, "gap_open": 11, "gap_extend": 1, "x_drop": HUGE}, DEFAULTS):
        got, _ = check_against_ref(case, P, "ends", **kw)
        g0, g6 = case.regions[0].tolist()[rows[(0, 0)]], case.regions[0].tolist()[rows[(6, 6)]]
        assert (got[1][g0], got[2][g0]) == (0, 70) and got[1][g6] + got[2][g6] == 400 and offs[6] + 400 == n_res
    case.close()


def test_position_specific_fuzz(ctx):
    """two letters, every maximum attained more than once, rows that differ by position"""
    rng = np.random.default_rng(52)
    qs, ts = RC.two_letter_batch(31, 3, 3, 20, 60)
    case = TT._Case(ctx, qs, ts, RC.FUZZ_K)
    assert 20 < case.rg.n_regions < 3000
    P = positional_rows(case.q[0], None, rng, own_lo=1, own_hi=3, noise=0.5)
    for kw in ({"band": 1, "gap_open": 0, "gap_extend": 1, "x_drop": 1}, {"band": 5, "gap_open": 1, "gap_extend": 0, "x_drop": HUGE},
               {"band": 31, "gap_open": 1, "gap_extend": 1, "x_drop": 4}):
        check_against_ref(case, P, "fuzz", **kw)
    prof = profile_of(ctx, case, P)
    h = case.hits_host
    for kw in ({}, {"extend": True, "x_drop": 1}, {"extend": True, "x_drop": 2 ** 32 - 1}):
        sc = ctx.score_regions(case.rg, case.hits, *case.q, *case.t, profile=prof, **kw)
        want = PR.score(case.regions, h[0], h[1], *case.q, *case.t, P, **kw)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(sc.to_host(), want)), kw
        sc.free()
    prof.free()
    case.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(ctx):
    """Every pass that reads residues under a matrix names a profile-made input — the object itself and the one a cull took
    from it; the traceback names the plain / profile mismatch and a profile of another batch."""
    import test_gpu_frame_stitch as TF
    import fstitch_cases as FC
    rng = np.random.default_rng(53)
    qs, ts, _ = RC.indel_batch(1, 71)
    case = TT._Case(ctx, qs, ts, RC.INDEL_K)
    q, t = case.q, case.t
    prof = profile_of(ctx, case, positional_rows(q[0], None, rng))
    other = ctx.profile_from_host(np.zeros((len(q[0]) + 1, A), np.int8), len(q[1]) - 1)
    al_p = ctx.align_regions(case.rg, case.hits, *q, *t, profile=prof)
    al_m = ctx.align_regions(case.rg, case.hits, *q, *t)
    cu = ctx.cull_regions(al_p)
    rg_k, al_k = cu.take(case.rg), cu.take(al_p)
    al_mk = cu.take(al_m)  # (a plain object the same cull took: the second offender of the plain / profile mismatch)
    assert al_k.by_profile and al_p.by_profile and not al_m.by_profile
    cg_p = ctx.trace_regions(case.rg, case.hits, *q, *t, al_p, profile=prof)
    cg_k = ctx.trace_regions(rg_k, case.hits, *q, *t, al_k, profile=prof)  # (a taken object keeps its mark and still traces)
    ch_p, ch_k = ctx.chain_regions(al_p), ctx.chain_regions(al_k)             # (the chain reads extents and scores only)
    comp_q, comp_t = ctx.residue_composition(*q), ctx.residue_composition(*t)
    # frame objects of the same context for ks_frames_stitch: the refusal comes before anything of them is compared
    name, contig, protein, align, max_fill, *_ = FC.worked_cases()[0]
    pipe = TF._Pipe(ctx, [contig], [protein], align)
    pipe_cg = pipe.cigars(False)
    before = ctx.pool_stats()["bytes_in_use"]
    BY = "made against a profile"
    for al, rg, cg, ch in ((al_p, case.rg, cg_p, ch_p), (al_k, rg_k, cg_k, ch_k)):
        with pytest.raises(ks.KmerseekError, match="region traceback: .*" + BY):
            ctx.trace_regions(rg, case.hits, *q, *t, al)
        with pytest.raises(ks.KmerseekError, match="region stitch: .*" + BY):
            ctx.stitch_chains(ch, al, cg, case.hits, *q, *t)
        with pytest.raises(ks.KmerseekError, match="frame stitch: .*" + BY):
            ctx.stitch_frames_device(pipe.fold, pipe.ch, al, pipe_cg, *pipe.batches)
        with pytest.raises(ks.KmerseekError, match="frame fold: .*" + BY):
            ctx.fold_frames(case.hits, al, np.array([0, 10], np.uint64))
        with pytest.raises(ks.KmerseekError, match="alignment statistics: .*" + BY):
            ctx.alignment_stats(al, case.hits, comp_q, comp_t, allow_ungapped=True)
        with pytest.raises(ks.KmerseekError, match="pileup: .*" + BY):
            ctx.pileup(cg, case.hits, side="query", offsets=q[1], alignments=al)
    # the traceback: plain alignments with a profile, profile-made ones with the profile of another batch; the other two passes likewise
    for al, rg in ((al_m, case.rg), (al_mk, rg_k)):
        with pytest.raises(ks.KmerseekError, match="made under a matrix"):
            ctx.trace_regions(rg, case.hits, *q, *t, al, profile=prof)
        with pytest.raises(ks.KmerseekError, match="made under a matrix"):
            ctx.trace_regions(rg, case.hits, *q, *t, al, profile=other)
    for fn, more in ((ctx.trace_regions, (al_p,)), (ctx.align_regions, ()), (ctx.score_regions, ())):
        with pytest.raises(ks.KmerseekError, match="profile of another batch"):
            fn(case.rg, case.hits, *q, *t, *more, profile=other)
        with pytest.raises(ks.KmerseekError, match="profile of another batch"):
            fn(case.rg, case.hits, q[0][:-1], np.minimum(q[1], len(q[0]) - 1), *t, *more, profile=prof)
    with ks.Context(0) as c2:  # a profile of another context
        foreign = c2.profile_from_host(np.zeros((len(q[0]), A), np.int8), len(q[1]) - 1)
        with pytest.raises(ks.KmerseekError):
            ctx.align_regions(case.rg, case.hits, *q, *t, profile=foreign)
        foreign.free()
    assert ctx.pool_stats()["bytes_in_use"] == before
    for o in (pipe.fold, pipe.ch, pipe.al, pipe.rg, pipe.hits, *pipe.cg.values(), comp_q, comp_t, ch_p, ch_k, cg_p, cg_k, rg_k, al_k, al_mk, cu, al_m, al_p, other, prof):
        o.free()
    case.close()


# ---- 6. the wire switch -----------------------------------------------------------------------------------------------------------
def test_wire_second_round_on_the_golden_pair(ctx, ced9_records, bcl2_records):
    """ced9 against the BCL2 set: the pssm_* columns are the reference's — pileup_ref, the build rule and the profile loops — run on
    the to_host() of the kept regions, alignments and CIGARs, which the same calls give again; the defaults return what they did."""
    import pileup_ref
    from kmerseek_amd import wire
    args = (os.path.join(TT.GOLDEN, "ced9.fasta"), os.path.join(TT.GOLDEN, TT.BCL2_25), 16, 5, "hp")
    opts = dict(regions=True, gapped=True, cigar=True, cull=True, eqx=True)
    plain = wire.search_extract_kmers_device(*args, ctx=ctx, **opts)
    rows = wire.search_extract_kmers_device(*args, ctx=ctx, profile=True, profile_beta=4.0, **opts)
    PSSM = ("pssm_score", "pssm_identities", "pssm_positives", "pssm_q_start", "pssm_q_end", "pssm_t_start", "pssm_t_end", "pssm_cigar")
    assert len(rows) == len(plain) >= 1 and [{k: v for k, v in r.items() if k not in PSSM} for r in rows] == plain
    assert all(set(PSSM) <= set(r) for r in rows) and not any(k.startswith("pssm") for r in plain for k in r)
    case = TT._Case(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], 16, 5, "hp")
    q, t, h = case.q, case.t, case.hits_host
    al = case.align(**DEFAULTS)
    cu = ctx.cull_regions(al)
    t_rg, t_al = cu.take(case.rg), cu.take(al)
    cg = ctx.trace_regions(t_rg, case.hits, *q, *t, t_al, eqx=True)
    rg_h, al_h, cg_h, cu_h = t_rg.to_host(), t_al.to_host(), cg.to_host(), cu.to_host()
    (depth, counts, *_), _ = pileup_ref.pileup(al_h[0], cg_h[0], cg_h[1], al_h[1], al_h[3], None, h[0], h[1], q[1], side="query", profile=True,
                                               other_res=t[0], other_off=t[1])
    assert depth.max() >= 1
    params = ks.profile_params(None, beta=4.0)
    P, _, n_obs = PR.build(counts, depth, q[0], params)
    assert (n_obs > 0).any() and not np.array_equal(P.reshape(-1, A), PR.matrix_rows(q[0], None))
    want_al = PR.align(rg_h, h[0], h[1], *q, *t, P, **DEFAULTS)
    want_cg = TT.encode(PR.trace(rg_h, want_al, h[0], h[1], *q, *t, P, band=16, gap_open=11, gap_extend=1, eqx=True))
    want = wire.region_rows(ced9_records, bcl2_records, h[0], h[1], case.regions, "hp", alignments=al.to_host(), cigars=cg_h, cull=cu_h,
                            pssm=(want_al, want_cg))
    assert [{k: r[k] for k in PSSM} for r in rows] == [{k: r[k] for k in PSSM} for r in want]
    for o in (cg, t_al, t_rg, cu, al):
        o.free()
    case.close()
    for bad in ({"stitch": True, "chain": True, "hit_rows": True}, {"evalue": True, "stat_params": (0.3, 0.1)}, {"coverage": "query"}, {"cull": False}):
        with pytest.raises(ValueError, match="profile=True"):
            wire.search_extract_kmers_device(*args, ctx=ctx, profile=True, **{**opts, **bad})
