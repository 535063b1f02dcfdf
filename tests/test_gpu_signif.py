"""GPU: ks_corpus_build / ks_hits_significance — per hit row the two f64 sums behind multisearch's prob_overlap and tf_idf_score.

Everything is exact: the f64 columns are compared as uint64 views with the CPU restatement of tests/signif_ref.py, the corpus
tables as integers; no tolerance anywhere.  Cases: the reference's golden multisearch rows (ced9 vs BCL2-25), many real queries
(merged-query frequencies differ from a single query's) on both row paths, hand-made sketches on the edges of the arithmetic,
thresholded hits, the edges (no hits, one row) and inputs that do not belong together."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
import signif_ref  # noqa: E402
from conftest import load_golden  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
UNCHAR = "uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz"
COMPUTED = ("prob_overlap", "prob_overlap_adjusted", "containment_adjusted", "containment_adjusted_log10", "tf_idf_score")
SG_CUT = 128  # ks_signif.hip: a row with |q| + |t| above it takes the wave path
U32_MAX = (1 << 32) - 1
MODES = (None, "1", "0")  # KS_DEBUG_SIGNIF_WAVE_ROWS: by length, every row on the wave path, every row on the lane path


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def expected():
    return load_golden("multisearch_expected.json")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_f64(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


def _upload(ctx, S, k, scaled, mol):
    return ctx.sketches_from_host(S[0], S[1], S[2], k, scaled, mol)


def _device(ctx, Q, T, k, scaled, mol, min_containment=0.0):
    """host sketch sets -> (hits on the host, (prob_overlap, tf_idf)) through search + Context.significance"""
    dQ, dT = _upload(ctx, Q, k, scaled, mol), _upload(ctx, T, k, scaled, mol)
    ix = ctx.index_build(dT)
    hits = ctx.search(ix, dQ, min_containment=min_containment)
    sig = ctx.significance(dQ, dT, hits)
    assert sig.n_rows == hits.count and all(p != 0 for p in sig.device_ptrs())
    out = hits.to_host(), sig.to_host()
    for o in (sig, hits, ix, dQ, dT):
        o.free()
    return out


def _compare(ctx, Q, T, k, scaled, mol, min_containment=0.0, want_hits=None):
    hits, (po, tf) = _device(ctx, Q, T, k, scaled, mol, min_containment)
    if want_hits is not None:
        for g, w, name in zip(hits, want_hits, ("qid", "tid", "intersect")):
            assert np.array_equal(g, w), name
    w_po, w_tf, shared = signif_ref.significance(Q, T, hits[0], hits[1])
    assert np.array_equal(shared, hits[2])
    _same_f64(po, w_po, "prob_overlap")
    _same_f64(tf, w_tf, "tf_idf")
    return hits, po, tf


def _sketch(name, k, scaled, mol, n=None):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    recs = recs if n is None else recs[:n]
    res, off = oracle.pack([s.upper() for _, s in recs])
    return [nm for nm, _ in recs], oracle.sketch_batch(res, off, k, scaled, mol, n_threads=4)


# ---- golden ------------------------------------------------------------------------------------------------------------------
def test_golden_rows_through_context_significance(ctx, expected):
    qn, Q = _sketch("ced9.fasta", 16, 5, "hp")
    tn, T = _sketch(BCL2_25, 16, 5, "hp")
    hits, po, tf = _compare(ctx, Q, T, 16, 5, "hp")
    assert len(hits[0]) == 5
    by_name = {tn[t]: r for r, t in enumerate(hits[1].tolist())}
    for want in expected["rows"]:
        r = by_name[want["match_name"]]
        adj, c_adj, c_log = signif_ref.derived(float(po[r]), int(hits[2][r]), int(Q[0][1]), 1, 25)
        for col, got in zip(COMPUTED, (float(po[r]), adj, c_adj, c_log, float(tf[r]))):
            assert float(want[col]) == got, (want["match_name"], col, want[col], got)


def test_do_multisearch_writes_the_fixture(ctx, expected, tmp_path):
    paths = []
    for name in ("ced9.fasta", BCL2_25):
        dst = tmp_path / name
        dst.write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
        paths.append(wire.sketch(str(dst), "hp", 16, 5, ctx=ctx))
    out = str(tmp_path / "multisearch.csv")
    assert wire.do_multisearch(paths[0], paths[1], out, 16, 5, "hp", ctx=ctx) == 5
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == expected["columns"] == wire.MULTISEARCH_COLUMNS
    got = {r[2]: dict(zip(rows[0], r)) for r in rows[1:]}
    text = ("query_name", "query_md5", "match_name", "match_md5", "moltype")
    for want in expected["rows"]:
        g = got[want["match_name"]]
        for col in expected["columns"]:
            if col in text:
                assert g[col] == want[col], col
            else:
                assert float(g[col]) == float(want[col]), (want["match_name"], col, g[col], want[col])
        assert g["intersect_hashes"] == want["intersect_hashes"]


# ---- many real queries, both row paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scaled,mol", [(16, 5, "hp"), (7, 1, "protein")])
@pytest.mark.parametrize("targets", ["self", "uncharacterized"])
def test_real_proteins_on_both_row_paths(monkeypatch, k, scaled, mol, targets):
    _, Q = _sketch(BCL2_300, k, scaled, mol)
    T = Q if targets == "self" else _sketch(UNCHAR, k, scaled, mol)[1]
    want_hits = oracle.manysearch(Q[0], Q[1], T[0], T[1], T[2], n_threads=4)
    assert len(want_hits[0]) > 300
    # rows with a long sequence cross the natural cut; at hp scaled = 5 rows of short sketches stay below it (at protein k = 7
    # scaled = 1 nearly every sketch is longer than the cut: the forced modes below put those rows on the lane path)
    size = (np.diff(Q[0])[want_hits[0]] + np.diff(T[0])[want_hits[1]]).astype(np.int64)
    assert np.any(size > SG_CUT), int(size.max())
    if mol == "hp":
        assert np.any(size <= SG_CUT), int(size.min())
    # merged-query frequencies are not one query's: some hash sits in several queries
    assert signif_ref.corpus(Q)[2].max() > 1
    w_po, w_tf, shared = signif_ref.significance(Q, T, want_hits[0], want_hits[1])
    assert np.array_equal(shared, want_hits[2])
    with ks.Context(0, follow_debug_env=True) as c:
        for mode in MODES:
            if mode is None:
                monkeypatch.delenv("KS_DEBUG_SIGNIF_WAVE_ROWS", raising=False)
            else:
                monkeypatch.setenv("KS_DEBUG_SIGNIF_WAVE_ROWS", mode)
            hits, (po, tf) = _device(c, Q, T, k, scaled, mol)
            for g, w, name in zip(hits, want_hits, ("qid", "tid", "intersect", "n_weighted")):
                assert np.array_equal(g, w), (mode, name)
            _same_f64(po, w_po, ("prob_overlap", mode))
            _same_f64(tf, w_tf, ("tf_idf", mode))


# ---- hand-made sketches ------------------------------------------------------------------------------------------------------
def _crafted():
    """12 targets, 5 queries (the last one empty), protein k=10 scaled=1:
    H0 sits in every target (idf = 1.0 exactly) and in queries 0 - 2; H1 carries 2^32 - 1 in targets 1 - 5 and in queries 1 and 3
    (corpus sums beyond 2^32 on both sides; query 1's own abundances sum past 2^32); query 0 and target 0 share 5,000 of
    their 6,000 / 7,000 hashes, abundances drawn from the edge set, 0 included; query 2 shares H0 alone with every target."""
    rng = np.random.default_rng(2024)
    H0, H1 = 0x0123456789ABCDEF, 0x7FFFFFFF00000001
    pool = np.unique(rng.integers(1 << 20, 1 << 63, 9000, dtype=np.uint64))[:8000]
    n_t, n_q = 12, 5
    edges = np.array([0, 1, 2, 3, 7, 1 << 16, 1 << 31, U32_MAX], np.uint32)
    seq, h, a = [], [], []
    for t in range(n_t):
        seq.append(t); h.append(H0); a.append(t % 3)  # (abundance 0 in every third target)
    for t in range(1, 6):
        seq.append(t); h.append(H1); a.append(U32_MAX)
    big_t = pool[:7000]
    seq += [0] * len(big_t); h += big_t.tolist(); a += rng.choice(edges, len(big_t)).tolist()
    for t in range(6, n_t):
        own = pool[7000 + 10 * t:7000 + 10 * t + 10]
        seq += [t] * len(own); h += own.tolist(); a += [1] * len(own)
    T = cs._csr(seq, h, a, n_t)
    seq, h, a = [], [], []
    big_q = np.concatenate([pool[2000:7000], pool[7200:8000], rng.integers(1, 1 << 20, 200, dtype=np.uint64)])
    big_q = np.unique(big_q)
    seq += [0] * len(big_q); h += big_q.tolist(); a += rng.choice(edges, len(big_q)).tolist()
    seq += [0, 1, 2]; h += [H0] * 3; a += [5, 0, 9]
    seq += [1, 1, 1]; h += [H1, int(pool[0]), int(pool[1])]; a += [U32_MAX, U32_MAX, U32_MAX]
    seq += [3, 3]; h += [H1, 77]; a += [U32_MAX, 4]
    seq += [2]; h += [99]; a += [1]
    Q = cs._csr(seq, h, a, n_q)
    cs.check_valid(T, 1); cs.check_valid(Q, 1)
    return Q, T, H0, H1


def test_crafted_sketches_on_both_row_paths(monkeypatch):
    Q, T, H0, H1 = _crafted()
    want_hits = signif_ref.join(Q, T)
    ch, csum, cdf, ctot = signif_ref.corpus(T)
    at = {int(x): i for i, x in enumerate(ch.tolist())}
    assert int(cdf[at[H0]]) == 12 and signif_ref.idf_table(12, 12)[12] == 1.0  # a hash in every target: idf = 1.0 exactly
    assert int(csum[at[H1]]) == 5 * U32_MAX > 1 << 32                          # a u32 accumulator fails here
    qh, qsum, _, _ = signif_ref.corpus(Q)
    assert int(qsum[qh.tolist().index(H1)]) == 2 * U32_MAX > 1 << 32
    assert int(Q[2][int(Q[0][1]):int(Q[0][2])].astype(np.uint64).sum()) > 1 << 32  # query 1's abundances sum past 2^32
    assert np.any(T[2] == 0) and np.any(Q[2] == 0)
    rows = dict(zip(zip(want_hits[0].tolist(), want_hits[1].tolist()), want_hits[2].tolist()))
    assert rows[(0, 0)] >= 5000 and sum(1 for v in rows.values() if v == 1) >= 15 and (4, 0) not in rows
    w_po, w_tf, _ = signif_ref.significance(Q, T, want_hits[0], want_hits[1])
    assert np.all(np.isfinite(w_po)) and np.all(np.isfinite(w_tf))
    with ks.Context(0, follow_debug_env=True) as c:
        for mode in MODES:
            if mode is None:
                monkeypatch.delenv("KS_DEBUG_SIGNIF_WAVE_ROWS", raising=False)
            else:
                monkeypatch.setenv("KS_DEBUG_SIGNIF_WAVE_ROWS", mode)
            hits, po, tf = _compare(c, Q, T, 10, 1, "protein", want_hits=want_hits)
            r = list(rows).index((2, 5))  # query 2 shares H0 alone: tf_idf = (9 / 10) * 1.0
            assert hits[2][r] == 1 and tf[r] == 9.0 / 10.0


def test_row_lengths_family_on_both_row_paths(monkeypatch):
    """rows on both sides of SG_CUT and of the 64-hash chunk edges of the wave kernel (crafted_sketches.row_lengths)"""
    _, k, scaled, mol, T, Q = cs.family("row_lengths")
    assert cs.SG_CUT == SG_CUT
    want_hits = signif_ref.join(Q, T)
    assert want_hits[2].tolist() == list(cs.ROW_SHARED) + [40, 41]
    with ks.Context(0, follow_debug_env=True) as c:
        for mode in MODES:
            if mode is None:
                monkeypatch.delenv("KS_DEBUG_SIGNIF_WAVE_ROWS", raising=False)
            else:
                monkeypatch.setenv("KS_DEBUG_SIGNIF_WAVE_ROWS", mode)
            _compare(c, Q, T, k, scaled, mol, want_hits=want_hits)


# ---- corpus ----------------------------------------------------------------------------------------------------------------
def _corpus_case(ctx, S, k, scaled, mol):
    d = _upload(ctx, S, k, scaled, mol)
    c = d.corpus()
    want = signif_ref.corpus(S)
    got = c.to_host()
    assert (c.n_hashes, c.n_docs, c.total_abund) == (len(want[0]), len(S[0]) - 1, want[3])
    for g, w, name in zip(got, want[:3], ("hashes", "abund_sum", "doc_freq")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    u = d.union()
    _, uh, ua = u.to_host()
    assert np.array_equal(uh, got[0])
    plain = got[1] < np.uint64(U32_MAX)
    assert np.array_equal(ua[plain].astype(np.uint64), got[1][plain]) and np.all(ua[~plain] == U32_MAX)
    for o in (u, c, d):
        o.free()
    return got


def test_corpus_tables(ctx):
    _, Q = _sketch(BCL2_300, 16, 5, "hp")
    _corpus_case(ctx, Q, 16, 5, "hp")
    _, _, _, _, T, _ = cs.family("union_saturation")
    got = _corpus_case(ctx, T, 10, 1, "protein")
    assert int(got[1].max()) == cs.UNION_LONG_RUN * U32_MAX and int(got[2].max()) == cs.UNION_LONG_RUN
    empty = (np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    d = _upload(ctx, empty, 10, 1, "protein")
    c = d.corpus()
    assert (c.n_hashes, c.n_docs, c.total_abund) == (0, 3, 0) and all(len(x) == 0 for x in c.to_host())


def test_corpora_passed_in_give_the_same_columns(ctx):
    Q, T, _, _ = _crafted()
    dQ, dT = _upload(ctx, Q, 10, 1, "protein"), _upload(ctx, T, 10, 1, "protein")
    hits = ctx.search(ctx.index_build(dT), dQ)
    cq, ct = dQ.corpus(), dT.corpus()
    a = ctx.significance(dQ, dT, hits, q_corpus=cq, t_corpus=ct).to_host()
    b = ctx.significance(dQ, dT, hits).to_host()
    c = ctx.significance(dQ, dT, hits, t_corpus=ct).to_host()
    for x, y in ((a, b), (a, c)):
        _same_f64(x[0], y[0], "prob_overlap"); _same_f64(x[1], y[1], "tf_idf")
    assert ct.n_docs == 12 and cq.n_docs == 5  # (still alive: significance frees only what it built)


# ---- thresholded hits ----------------------------------------------------------------------------------------------------------
def test_thresholded_hits_keep_their_values(ctx):
    t_res, t_off = synth.proteome(300, stream=921)
    q_res, q_off = synth.queries(200, t_res, t_off, stream=922, frac_related=0.6)
    T = oracle.sketch_batch(t_res, t_off, 7, 1, "protein", n_threads=4)
    Q = oracle.sketch_batch(q_res, q_off, 7, 1, "protein", n_threads=4)
    all_hits, all_po, all_tf = _compare(ctx, Q, T, 7, 1, "protein")
    hits, po, tf = _compare(ctx, Q, T, 7, 1, "protein", min_containment=0.5)
    assert 0 < len(hits[0]) < len(all_hits[0])
    where = {(q, t): r for r, (q, t) in enumerate(zip(all_hits[0].tolist(), all_hits[1].tolist()))}
    pick = np.array([where[(q, t)] for q, t in zip(hits[0].tolist(), hits[1].tolist())])
    _same_f64(po, all_po[pick], "prob_overlap")
    _same_f64(tf, all_tf[pick], "tf_idf")


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    t_res, t_off = synth.proteome(50, stream=923)
    u_res, u_off = synth.proteome(20, stream=924)
    T = oracle.sketch_batch(t_res, t_off, 10, 1, "protein")
    U = oracle.sketch_batch(u_res, u_off, 10, 1, "protein")
    hits, po, tf = _compare(ctx, U, T, 10, 1, "protein")  # no hits
    assert len(hits[0]) == 0 and len(po) == 0 and len(tf) == 0
    one_t = tuple(x.copy() for x in (T[0][:2], T[1][:int(T[0][1])], T[2][:int(T[0][1])]))
    n = int(T[0][1])
    one_q = (np.array([0, n - 5], np.uint64), T[1][5:n].copy(), np.ones(n - 5, np.uint32))
    hits, po, tf = _compare(ctx, one_q, one_t, 10, 1, "protein")  # exactly one row
    assert hits[2].tolist() == [n - 5] and po[0] > 0 and abs(tf[0] - 1.0) < 1e-12  # (one target: idf = log(2 / 2) + 1; the tf sum to 1)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_inputs_that_do_not_belong_together_are_refused(ctx):
    t_res, t_off = synth.proteome(120, stream=925)
    q_res, q_off = synth.queries(80, t_res, t_off, stream=926, frac_related=0.6)
    o_res, o_off = synth.proteome(120, stream=927)  # as many sequences as the targets, none of their 10-mers
    T = ctx.sketch_batch(t_res, t_off, 10, 1, "protein")
    Q = ctx.sketch_batch(q_res, q_off, 10, 1, "protein")
    other = ctx.sketch_batch(o_res, o_off, 10, 1, "protein")
    fewer = ctx.sketch_batch(*synth.proteome(7, stream=928), 10, 1, "protein")
    hits = ctx.search(ctx.index_build(T), Q)
    assert hits.count > 0 and hits.to_host()[1].max() >= 7
    cq, ct = Q.corpus(), T.corpus()
    q11 = ctx.sketch_batch(q_res, q_off, 11, 1, "protein")
    t_dayhoff = ctx.sketch_batch(t_res, t_off, 10, 1, "dayhoff")
    c_other = other.corpus()
    cases = ((Q, other, cq, None, "belong"),      # targets that are not the searched ones: shared counts differ
             (Q, fewer, cq, None, "beyond"),      # ... a target id past the set
             (Q, T, cq, cq, "corpus"),            # a corpus of the wrong set (80 sketches, 120 targets)
             (Q, T, c_other, ct, "corpus"),
             (q11, T, None, ct, "parameters"),
             (Q, t_dayhoff, cq, None, "parameters"))
    for q, t, a, b, why in cases:
        before = ctx.pool_stats()["bytes_in_use"]
        with pytest.raises(ks.KmerseekError) as e:
            ctx.significance(q, t, hits, q_corpus=a, t_corpus=b)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and why in str(e.value), str(e.value)
        assert ctx.pool_stats()["bytes_in_use"] == before, why
    for opts in ((0, 7), (1, 0), (0x80000000, 0)):  # non-zero reserved, unknown flags: refused before any device work
        out = C.c_void_p()
        st = ctx._L.ks_hits_significance(ctx._h, Q._h, T._h, cq._h, ct._h, hits._h, C.byref(_lib.ks_signif_opts(*opts)), C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG and not out.value
        assert "options" in ctx._L.ks_last_error(ctx._h).decode()
    # the context stays usable
    sig = ctx.significance(Q, T, hits, q_corpus=cq, t_corpus=ct)
    h = hits.to_host()
    Qh, Th = Q.to_host(), T.to_host()
    w_po, w_tf, _ = signif_ref.significance(Qh, Th, h[0], h[1])
    po, tf = sig.to_host()
    _same_f64(po, w_po, "prob_overlap"); _same_f64(tf, w_tf, "tf_idf")
