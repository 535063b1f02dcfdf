"""GPU: alignment statistics — ks_residue_composition_device, ks_scores_stats_device and its three wrappers.

Composition: counts, totals and lengths exactly against numpy.bincount of the class table under KS_DEBUG_COMP_PATH unset, 1, 2
and 3.  Histogram and root: status and x bit for bit against the loop of tests/astats_ref.py (tests/test_astats_cpu.py holds
that loop against exact rational arithmetic) — 200 random rows under three matrices, the crafted fallback rows, one row of two
2^20-residue sequences under a matrix from -128 to 127, a lower-case copy.  Derived columns against the reference's f64 formulas
on the same x, with the tolerances of the contract: lambda_ratio 1e-13 relative (two logarithms of <= 1 ulp and a division),
bit_score 1e-12 |ref| + 1e-9, evalue 1e-9 relative where the reference is >= 1e-290 and below 1e-289 on both sides where it is
not.  Then the semantics of the options, the errors — a context still works after each — and the golden pair end to end."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import astats_cases as AC  # noqa: E402
import astats_ref as R  # noqa: E402
import crafted_sketches as cs  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
MODES = (None, "1", "2", "3")  # KS_DEBUG_COMP_PATH
PARAMS = (0.267, 0.041)        # a caller's (lambda, K): BLOSUM62 11 / 1, as an example of gapped values
UNIFORM = np.where(np.isin(np.arange(R.A), R.STD), 1.0, 0.0)


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


@pytest.fixture(params=MODES, ids=lambda m: f"path_{m}")
def mode_ctx(request, monkeypatch):
    """A context created after KS_DEBUG_COMP_PATH is set (the knobs are read when a context is made)."""
    if request.param is None:
        monkeypatch.delenv("KS_DEBUG_COMP_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_COMP_PATH", request.param)
    with ks.Context(0) as c:
        yield c


def limits():
    a, b = C.c_uint32(0), C.c_uint32(0)
    _lib.load().ks_debug_rcomp_limits(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def hits_of(ctx, qid, tid, n_q, n_t):
    """A hit list with exactly the rows (qid[r], tid[r]) — ascending, distinct: every pair shares one hash of its own."""
    h = (qid.astype(np.uint64) * np.uint64(n_t) + tid.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    ones = np.ones(len(h), np.uint32)
    Q, T = cs._csr(qid, h, ones, n_q), cs._csr(tid, h, ones, n_t)
    cs.check_valid(Q, 1); cs.check_valid(T, 1)
    Qd, Td = ctx.sketches_from_host(*Q, 10, 1, "protein"), ctx.sketches_from_host(*T, 10, 1, "protein")
    ix = ctx.index_build(Td)
    hits = ctx.search(ix, Qd)
    got = hits.to_host()
    assert np.array_equal(got[0], qid) and np.array_equal(got[1], tid)
    for o in (ix, Qd, Td):
        o.free()
    return hits


def run_stats(ctx, scores, row_offsets, hits, qc, tc, **kw):
    """alignment_stats_device on uploaded columns -> the host columns and the scalars, as astats_ref.stats names them."""
    scores = np.ascontiguousarray(scores, dtype=np.int64)
    bufs = [ctx.to_device(scores if len(scores) else np.zeros(1, np.int64))]
    if row_offsets is not None:
        bufs.append(ctx.to_device(np.ascontiguousarray(row_offsets, dtype=np.uint64)))
    try:
        st = ctx.alignment_stats_device(bufs[1].ptr if row_offsets is not None else None, bufs[0].ptr, hits.count, len(scores), hits, qc, tc, **kw)
        cols = st.to_host()
        assert [c.dtype for c in cols] == [np.uint8] + [np.float64] * 6 and all(p != 0 for p in st.device_ptrs())
        assert (st.row_bit_score_ptr, st.row_evalue_ptr) == st.device_ptrs()[5:] and (st.n_rows, st.n_entries) == (hits.count, len(scores))
        out = dict(zip(("status", "x", "lambda_ratio", "bit_score", "evalue", "row_bit_score", "row_evalue"), cols))
        out.update(lambda_std=st.lambda_std, lambda_used=st.lambda_used, K_used=st.K_used, params_source=st.params_source, n_fallback=st.n_fallback)
        st.free()
        return out
    finally:
        for b in bufs:
            b.free()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_derived(got, want, label=""):
    """The f64 columns against the reference computed on the library's own x; prints the largest deviations it saw."""
    def rel(a, b):
        return float(np.max(np.abs(a - b) / np.abs(b))) if len(a) else 0.0
    d_ratio = rel(got["lambda_ratio"], want["lambda_ratio"])
    d_bit = float(np.max(np.abs(got["bit_score"] - want["bit_score"]) - 1e-12 * np.abs(want["bit_score"]))) if len(want["bit_score"]) else 0.0
    big = want["evalue"] >= 1e-290
    d_ev = rel(got["evalue"][big], want["evalue"][big])
    a_bit = float(np.max(np.abs(got["bit_score"] - want["bit_score"]))) if len(want["bit_score"]) else 0.0
    print(f"astats deviations {label}: lambda_ratio {d_ratio:.3e} rel, bit_score {a_bit:.3e} abs, evalue {d_ev:.3e} rel")
    assert d_ratio <= 1e-13 and d_bit <= 1e-9 and d_ev <= 1e-9
    assert np.all(got["evalue"][~big] < 1e-289) and np.all(want["evalue"][~big] < 1e-289)
    for k in ("row_bit_score", "row_evalue"):
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k]), nan)
    n_rows = len(want["status"])
    offs = want.get("_offs")
    for r in range(n_rows):
        b, e = (r, r + 1) if offs is None else (int(offs[r]), int(offs[r + 1]))
        if e > b:  # the row columns are exactly the best of the row's own entries
            assert got["row_bit_score"][r] == got["bit_score"][b:e].max() and got["row_evalue"][r] == got["evalue"][b:e].min()
    for k in ("lambda_used", "K_used", "params_source", "n_fallback"):
        assert got[k] == want[k], k
    assert abs(got["lambda_std"] - want["lambda_std"]) <= 1e-12 * want["lambda_std"]


# ---- 1. composition -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def comp_batch():
    wave_max, group_max = limits()
    rng = np.random.default_rng(17)
    lens = [0, 1, 63, 64, 65, wave_max - 1, wave_max, wave_max + 1, group_max - 1, group_max, group_max + 1, 0]
    seqs = [np.arange(256, dtype=np.uint8)] + [rng.integers(0, 256, n).astype(np.uint8) for n in lens]
    seqs.append(np.full(70_000, ord("L"), np.uint8))                      # one counter passes 2^16
    seqs.append(AC.LETTERS[rng.integers(0, 20, 3 * group_max + 777)])     # split over four workgroups
    seqs.append(np.frombuffer(b"acdefghiklmnpqrstvwy*xbzjuo", np.uint8))
    res, offs = AC.pack(seqs)
    return res, offs, R.composition(res, offs)


def test_composition_every_path(mode_ctx):
    res, offs, (counts, totals, length) = comp_batch()
    comp = mode_ctx.residue_composition(res, offs)
    assert (comp.n_seqs, comp.n_residues) == (len(offs) - 1, len(res)) and all(p != 0 for p in comp.device_ptrs())
    got = comp.to_host()
    assert [a.dtype for a in got] == [np.uint32, np.uint64, np.uint32]
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], totals) and np.array_equal(got[2], length)
    assert got[0][13, 11] == 70_000 and got[0][0].sum() == 256 and got[0][0, 27] == 256 - 52 - 1
    comp.free()


def test_composition_empty_batch_and_errors(ctx):
    comp = ctx.residue_composition(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    got = comp.to_host()
    assert comp.n_seqs == 0 and got[0].shape == (0, 28) and not got[1].any() and len(got[2]) == 0
    comp.free()
    empty = ctx.residue_composition(np.zeros(0, np.uint8), np.zeros(4, np.uint64))
    assert empty.n_seqs == 3 and not empty.to_host()[0].any()
    empty.free()
    for offs, word in ((np.array([0, 5, 3, 8], np.uint64), "sequence 1"), (np.array([0, 5, 9], np.uint64), "sequence 1")):
        with pytest.raises(ks.KmerseekError) as e:
            ctx.residue_composition(np.full(8, 65, np.uint8), offs)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and word in str(e.value)
    with pytest.raises(ks.KmerseekError):
        ctx.residue_composition_device(0, 0, 1, 0)
    ok = ctx.residue_composition(np.full(8, 65, np.uint8), np.array([0, 8], np.uint64))
    assert ok.to_host()[0][0, 0] == 8
    ok.free()


# ---- 2. histogram and root, 3. derived columns ------------------------------------------------------------------------------------------
class Rows:
    """The random rows on the device: the compositions of both batches, the hit list, their host counts, and a CSR of scores
    with empty rows, negative scores and one score large enough for its E-value to underflow to 0."""

    def __init__(self, ctx, batches, lower=False):
        q_res, q_off, t_res, t_off, self.qid, self.tid = batches
        if lower:
            q_res, t_res = q_res | np.uint8(32), t_res | np.uint8(32)
        self.qc, self.tc = ctx.residue_composition(q_res, q_off), ctx.residue_composition(t_res, t_off)
        self.q_counts, _, self.q_len = R.composition(q_res, q_off)
        self.t_counts, _, self.t_len = R.composition(t_res, t_off)
        self.hits = hits_of(ctx, self.qid, self.tid, len(q_off) - 1, len(t_off) - 1)
        rng = np.random.default_rng(23)
        per = rng.integers(0, 4, len(self.qid))
        self.offs = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
        self.scores = rng.integers(-20, 400, int(per.sum())).astype(np.int64)
        self.scores[3] = 20_000

    def ref(self, got, scores, offs, **kw):
        want = R.stats(scores, offs, self.qid, self.tid, self.q_counts, self.q_len, self.t_counts, self.t_len,
                       x_of=list(zip(got["status"].tolist(), got["x"].tolist())), **kw)
        want["_offs"] = offs
        return want

    def close(self):
        for o in (self.qc, self.tc, self.hits):
            o.free()


@pytest.fixture(scope="module")
def rows(ctx):
    r = Rows(ctx, AC.random_batches())
    yield r
    r.close()


@pytest.mark.parametrize("name", sorted(AC.MATRICES))
def test_random_rows_bit_identical(ctx, rows, name):
    status, x = AC.rows_reference(name)
    assert not status.any()  # the condition of this set: no fallback row
    got = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, matrix=AC.MATRICES[name], params=PARAMS)
    assert np.array_equal(got["status"], status) and np.array_equal(bits(got["x"]), bits(x))
    check_derived(got, rows.ref(got, rows.scores, rows.offs, matrix=AC.MATRICES[name], params=PARAMS), f"{name}, CSR")
    assert got["evalue"][3] == 0.0 and np.isnan(got["row_bit_score"]).sum() == int((np.diff(rows.offs.astype(np.int64)) == 0).sum()) > 0
    # one score per hit row, without row_offsets
    one = np.arange(len(rows.qid), dtype=np.int64) * 3 - 50
    got1 = run_stats(ctx, one, None, rows.hits, rows.qc, rows.tc, matrix=AC.MATRICES[name], params=PARAMS)
    assert np.array_equal(bits(got1["x"]), bits(x))
    check_derived(got1, rows.ref(got1, one, None, matrix=AC.MATRICES[name], params=PARAMS), f"{name}, one per row")
    assert np.array_equal(bits(got1["row_bit_score"]), bits(got1["bit_score"])) and np.array_equal(bits(got1["row_evalue"]), bits(got1["evalue"]))


def test_lower_case_copy_is_identical(ctx, rows):
    low = Rows(ctx, AC.random_batches(), lower=True)
    try:
        a = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, matrix=AC.MATRICES["random"], params=PARAMS)
        b = run_stats(ctx, low.scores, low.offs, low.hits, low.qc, low.tc, matrix=AC.MATRICES["random"], params=PARAMS)
        for k in ("status", "x", "lambda_ratio", "bit_score", "evalue", "row_bit_score", "row_evalue"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert np.array_equal(low.qc.to_host()[0], rows.qc.to_host()[0])
    finally:
        low.close()


@pytest.mark.parametrize("name", sorted(AC.MATRICES))
def test_crafted_fallback_rows(ctx, name):
    q_res, q_off, t_res, t_off, qid, tid = AC.fallback_batches()
    qc, tc = ctx.residue_composition(q_res, q_off), ctx.residue_composition(t_res, t_off)
    hits = hits_of(ctx, qid, tid, 4, 4)
    try:
        got = run_stats(ctx, np.array([10, 20, 30, 40], np.int64), None, hits, qc, tc, matrix=AC.MATRICES[name], params=PARAMS, background=UNIFORM)
        assert got["status"].tolist() == [R.ROW_FALLBACK] * 4 and not got["x"].any() and got["lambda_ratio"].tolist() == [1.0] * 4
        assert got["n_fallback"] == 4
        want = R.stats(np.array([10, 20, 30, 40]), None, qid, tid, *R.composition(q_res, q_off)[::2], *R.composition(t_res, t_off)[::2],
                       matrix=AC.MATRICES[name], params=PARAMS, background=UNIFORM)
        check_derived(got, want, f"{name}, fallback rows")
    finally:
        for o in (qc, tc, hits):
            o.free()


def test_wide_row_of_two_2_20_sequences(ctx):
    """N = 2^40 and degree 255: the coefficients are still exact in f64, and the root is the reference's, bit for bit."""
    cq, ct = AC.wide_counts()
    m = AC.matrix_wide()
    q_res, q_off = AC.pack([AC.wide_sequence(cq)])
    t_res, t_off = AC.pack([AC.wide_sequence(ct)])
    qc, tc = ctx.residue_composition(q_res, q_off), ctx.residue_composition(t_res, t_off)
    one = np.zeros(1, np.uint32)
    hits = hits_of(ctx, one, one, 1, 1)
    try:
        assert np.array_equal(qc.to_host()[0][0], cq) and qc.to_host()[2][0] == R.MAX_SEQ_LEN
        got = run_stats(ctx, np.array([1000], np.int64), None, hits, qc, tc, matrix=m, params=PARAMS)
        status, x = R.row_root(m, cq, ct, *R.score_range(m))
        assert status == R.ROW_REGULAR and got["status"][0] == status and bits(got["x"])[0] == bits([x])[0]
        want = R.stats(np.array([1000]), None, one, one, cq[None], [R.MAX_SEQ_LEN], ct[None], [R.MAX_SEQ_LEN], matrix=m, params=PARAMS,
                       x_of=[(status, x)])
        check_derived(got, want, "wide row")
    finally:
        for o in (qc, tc, hits):
            o.free()


# ---- 4. semantics and errors --------------------------------------------------------------------------------------------------------------
def test_option_semantics(ctx, rows):
    m = AC.MATRICES["p5m4"]
    kw = dict(matrix=m, params=PARAMS)
    # the ratio is clamped at both bounds
    got = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, ratio=(0.97, 0.99), **kw)
    check_derived(got, rows.ref(got, rows.scores, rows.offs, ratio=(0.97, 0.99), **kw), "clamped")
    assert got["lambda_ratio"].min() == 0.97 and got["lambda_ratio"].max() == 0.99 and (got["lambda_ratio"] == 0.97).sum() > 3 < (got["lambda_ratio"] == 0.99).sum()
    # no composition: ratio 1, no histogram; the target composition may then be left out
    for tc, more in ((rows.tc, {}), (None, dict(db_residues=12345, db_seqs=40, background=UNIFORM))):
        got = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, tc, composition=False, **kw, **more)
        assert got["status"].tolist() == [R.ROW_SKIPPED] * len(rows.qid) and not got["x"].any() and (got["lambda_ratio"] == 1.0).all()
        check_derived(got, rows.ref(got, rows.scores, rows.offs, composition_based=False, **kw, **more), "no composition")
    with pytest.raises(ks.KmerseekError) as e:
        run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, None, composition=False, db_residues=12345, db_seqs=40, **kw)
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "NULL" in str(e.value)
    # pairwise: the search space is the target sequence; length_adjust floors both lengths at 1
    for more in (dict(pairwise=True), dict(length_adjust=7), dict(pairwise=True, length_adjust=100_000), dict(length_adjust=100_000),
                 dict(db_residues=10 ** 9, db_seqs=10 ** 6, length_adjust=31)):
        got = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, **kw, **more)
        check_derived(got, rows.ref(got, rows.scores, rows.offs, **kw, **more), str(more))
    floor = run_stats(ctx, np.zeros(len(rows.qid), np.int64), None, rows.hits, rows.qc, rows.tc, length_adjust=100_000, **kw)
    assert np.all(floor["evalue"] == PARAMS[1] * 1.0 * 1.0)
    # the library's own (ungapped) parameters against the caller's
    own = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, matrix=m)
    want = rows.ref(own, rows.scores, rows.offs, matrix=m)
    assert own["params_source"] == 0 and abs(own["lambda_used"] / want["lambda_used"] - 1) <= 1e-12 and abs(own["K_used"] / want["K_used"] - 1) <= 1e-9
    assert own["lambda_used"] == own["lambda_std"]
    want.update(lambda_used=own["lambda_used"], K_used=own["K_used"])
    check_derived(own, rows.ref(own, rows.scores, rows.offs, matrix=m, params=(own["lambda_used"], own["K_used"])) | dict(params_source=0), "own parameters")
    assert run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, **kw)["params_source"] == 1


def test_errors_leave_a_working_context(ctx, rows):
    kw = dict(matrix=AC.MATRICES["p5m4"], params=PARAMS)

    def refused(status, word, *a, **k):
        with pytest.raises(ks.KmerseekError) as e:
            run_stats(ctx, *a, **k)
        assert e.value.status == status and word in str(e.value), str(e.value)
        ok = run_stats(ctx, rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, **kw)  # the context still works
        assert ok["n_fallback"] == 0
    n = len(rows.qid)
    refused(_lib.KS_ERR_INVALID_ARG, "ratio_min", rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, ratio=(0.9, 0.5), **kw)
    refused(_lib.KS_ERR_INVALID_ARG, "come together", rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, params=(0.3, 0.0))
    refused(_lib.KS_ERR_INVALID_ARG, "negative and a positive", rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, matrix=AC.matrix_pm(3, 1), params=PARAMS)
    refused(_lib.KS_ERR_INVALID_ARG, "too close to zero", rows.scores, rows.offs, rows.hits, rows.qc, rows.tc, matrix=AC.MATRICES["random"])
    # row counts that disagree with the hit list; scores without a CSR; a CSR that is none
    bad = rows.offs.copy(); bad[5] = bad[-1] + 3
    refused(_lib.KS_ERR_INVALID_ARG, "hit row 4", rows.scores, bad, rows.hits, rows.qc, rows.tc, **kw)
    refused(_lib.KS_ERR_INVALID_ARG, "without row_offsets", rows.scores[: n - 1], None, rows.hits, rows.qc, rows.tc, **kw)
    with pytest.raises(ks.KmerseekError) as e:
        buf = ctx.to_device(rows.scores)
        try:
            ctx.alignment_stats_device(None, buf.ptr, n - 1, n - 1, rows.hits, rows.qc, rows.tc, **kw)
        finally:
            buf.free()
    assert e.value.status == _lib.KS_ERR_INVALID_ARG and "another search" in str(e.value)
    # an id beyond its composition: the first such row is named
    short_q = ctx.residue_composition(*AC.pack([AC.LETTERS] * int(rows.qid[150])))
    short_t = ctx.residue_composition(*AC.pack([AC.LETTERS] * 7))
    first_t = int(np.flatnonzero(rows.tid >= 7)[0])
    refused(_lib.KS_ERR_INVALID_ARG, f"hit row {int(np.flatnonzero(rows.qid >= rows.qid[150])[0])} ", rows.scores, rows.offs, rows.hits, short_q, rows.tc, **kw)
    refused(_lib.KS_ERR_INVALID_ARG, f"hit row {first_t} ", rows.scores, rows.offs, rows.hits, rows.qc, short_t, **kw)
    refused(_lib.KS_ERR_INVALID_ARG, f"hit row {first_t} ", rows.scores, rows.offs, rows.hits, rows.qc, short_t, composition=False, pairwise=True, **kw)
    short_q.free(); short_t.free()
    with ks.Context(0) as other:
        foreign = other.residue_composition(*AC.random_batches()[:2])
        refused(_lib.KS_ERR_INVALID_ARG, "another context", rows.scores, rows.offs, rows.hits, foreign, rows.tc, **kw)
        foreign.free()


def test_capacity_refusal_beyond_2_20(ctx):
    long_q = ctx.residue_composition(*AC.pack([np.full(R.MAX_SEQ_LEN + 1, ord("A"), np.uint8), AC.LETTERS]))
    tc = ctx.residue_composition(*AC.pack([AC.LETTERS]))
    qid, tid = np.array([0, 1], np.uint32), np.zeros(2, np.uint32)
    hits = hits_of(ctx, qid, tid, 2, 1)
    try:
        with pytest.raises(ks.KmerseekError) as e:
            run_stats(ctx, np.array([5, 6], np.int64), None, hits, long_q, tc, params=PARAMS)
        assert e.value.status == _lib.KS_ERR_CAPACITY and "hit row 0 " in str(e.value) and "2^20" in str(e.value)
        ok = run_stats(ctx, np.array([5, 6], np.int64), None, hits, long_q, tc, params=PARAMS, composition=False)  # no histogram: lengths only
        assert ok["status"].tolist() == [R.ROW_SKIPPED] * 2
    finally:
        for o in (long_q, tc, hits):
            o.free()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def test_golden_end_to_end(ctx, ced9_records, bcl2_records):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    q_res, q_off = ks.pack([s for _, s in ced9_records])
    t_res, t_off = ks.pack([s for _, s in bcl2_records])
    Q, T = ctx.sketch_batch(q_res, q_off, 16, 5, "hp"), ctx.sketch_batch(t_res, t_off, 16, 5, "hp")
    ix = ctx.index_build(T)
    hits = ctx.search(ix, Q)
    qp, tp = ctx.kmer_positions_table(q_res, q_off, 16, 5, "hp"), ctx.kmer_positions_table(t_res, t_off, 16, 5, "hp")
    mp = ctx.match_positions(qp, tp, hits)
    rg = ctx.match_regions(mp)
    sc = ctx.score_regions(rg, hits, q_res, q_off, t_res, t_off, extend=True, x_drop=10)
    al = ctx.align_regions(rg, hits, q_res, q_off, t_res, t_off)
    qc, tc = ctx.residue_composition(q_res, q_off), ctx.residue_composition(t_res, t_off)
    qid, tid = hits.to_host()[:2]
    objs = [Q, T, ix, hits, qp, tp, mp, rg, sc, al, qc, tc]
    try:
        assert hits.count > 0 and al.n_regions > 0
        # the refusals of the wrappers: gapped scores without gapped parameters; a matrix that is not the alignments'
        with pytest.raises(ks.KmerseekError) as e:
            ctx.alignment_stats(al, hits, qc, tc)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "gapped" in str(e.value)
        with pytest.raises(ks.KmerseekError) as e:
            ctx.alignment_stats(al, hits, qc, tc, params=PARAMS, matrix=AC.MATRICES["p5m4"])
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and "matrix differs" in str(e.value)
        with pytest.raises(TypeError):
            ctx.alignment_stats(rg, hits, qc, tc)
        # alignments: the object entry point is the column entry point on its columns
        st_al = ctx.alignment_stats(al, hits, qc, tc, params=PARAMS, matrix=R.pm1_matrix())
        al_host = al.to_host()
        by_cols = run_stats(ctx, al_host[5], al_host[0], hits, qc, tc, params=PARAMS)
        h_al = st_al.to_host()
        for a, k in zip(h_al, ("status", "x", "lambda_ratio", "bit_score", "evalue", "row_bit_score", "row_evalue")):
            assert np.array_equal(a.view(np.uint8), by_cols[k].view(np.uint8)), k
        want = R.stats(al_host[5], al_host[0], qid, tid, *R.composition(q_res, q_off)[::2], *R.composition(t_res, t_off)[::2], params=PARAMS)
        assert np.array_equal(h_al[0], want["status"]) and np.array_equal(bits(h_al[1]), bits(want["x"]))
        ung = ctx.alignment_stats(al, hits, qc, tc, allow_ungapped=True)
        assert ung.params_source == 0 and ung.lambda_used == ung.lambda_std > 0
        ung.free()
        rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, evalue=True, stat_params=PARAMS)
        plain = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True)
        assert rows == wire.region_rows(ced9_records, bcl2_records, qid, tid, rg.to_host(), "hp", alignments=al_host, stats=h_al)
        assert [{k: v for k, v in r.items() if k not in ("aln_bit_score", "aln_evalue", "lambda_ratio")} for r in rows] == plain
        # max_evalue removes exactly the rows above it
        ev = sorted({r["aln_evalue"] for r in rows})
        assert len(ev) >= 2
        cut = ev[-2]  # (everything but the rows of the largest E-value stays)
        kept = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, gapped=True, evalue=True, stat_params=PARAMS, max_evalue=cut)
        assert kept == [r for r in rows if r["aln_evalue"] <= cut] and 0 < len(kept) < len(rows)
        # scored regions: the ungapped parameters are the library's own
        st_sc = ctx.alignment_stats(sc, hits, qc, tc)
        s_rows = wire.search_extract_kmers_device(*args, ctx=ctx, regions=True, score=True, extend=True, x_drop=10, evalue=True)
        assert s_rows == wire.region_rows(ced9_records, bcl2_records, qid, tid, rg.to_host(), "hp", scores=sc.to_host(), stats=st_sc.to_host())
        assert st_sc.params_source == 0 and all("region_evalue" in r and "aln_evalue" not in r for r in s_rows)
        # stitched hits: one entry per hit row, and the row column ranks the hits
        on = dict(regions=True, gapped=True, cigar=True, cull=True, chain=True, hit_rows=True, stitch=True)
        h_rows = wire.search_extract_kmers_device(*args, ctx=ctx, evalue=True, stat_params=PARAMS, **on)
        base = wire.search_extract_kmers_device(*args, ctx=ctx, **on)
        assert [{k: v for k, v in r.items() if k not in ("aln_bit_score", "aln_evalue")} for r in h_rows] == base and h_rows
        lam, K = PARAMS
        cu = ctx.cull_regions(al)
        k_rg, k_al = cu.take(rg), cu.take(al)
        cg = ctx.trace_regions(k_rg, hits, q_res, q_off, t_res, t_off, k_al)
        ch = ctx.chain_regions(k_al)
        stt = ctx.stitch_chains(ch, k_al, cg, hits, q_res, q_off, t_res, t_off)
        st_hit = ctx.alignment_stats(stt, hits, qc, tc, params=PARAMS, alignments=k_al)
        objs += [cu, k_rg, k_al, cg, ch, stt, st_hit, st_al, st_sc]
        assert st_hit.n_entries == st_hit.n_rows == hits.count
        by_name = {(r["query_name"], r["match_name"]): r for r in h_rows}
        hb, he = st_hit.to_host()[3:5]
        assert len(by_name) == len(h_rows)
        for r in range(hits.count):  # (a hit row without a chain gives no row)
            row = by_name.get((ced9_records[qid[r]][0], bcl2_records[tid[r]][0]))
            assert row is None or (row["aln_bit_score"], row["aln_evalue"]) == (hb[r], he[r])
        top = ctx.best_hits(hits, 3, score=st_hit.row_bit_score_ptr)
        rank, src_row = top.best_to_host()
        per_q = {}
        for r in np.argsort(-hb, kind="stable"):
            per_q.setdefault(int(qid[r]), []).append(int(r))
        assert sorted(src_row.tolist()) == sorted(r for rs in per_q.values() for r in rs[:3]) and sorted(set(rank.tolist())) == [0, 1, 2]
        objs.append(top)
    finally:
        for o in objs:
            o.free()
