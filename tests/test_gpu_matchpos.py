"""GPU: ks_match_positions — per hit row the (query start, target start) pairs of windows that share a kept hash.

Everything is compared exactly (integers) with the CPU restatement of tests/matchpos_join.py: the hit rows, row_offsets, the
pairs in order, and the four extents.  Cases: the reference's golden stitched rows (ced9 vs BCL2-25), real proteins, sequences
that are one residue repeated (m x n pairs in one row) and the max_pairs refusal, starts beyond 2^16, thresholded hits,
forced row slices, inputs that do not belong together, and the edges (no hits, no kept windows, one row)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, synth, wire  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
BCL2_300 = "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"
UNCHAR = "uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz"
COLUMNS = ("row_offsets", "q_start", "t_start", "q_lo", "q_hi", "t_lo", "t_hi")
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


def _device(ctx, q, t, k, scaled, mol, min_containment=0.0, max_pairs=0):
    """-> (hits on the host, MatchPositions.to_host(), MatchPositions.n_slices)"""
    T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
    Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
    hits = ctx.search(ctx.index_build(T), Q, min_containment=min_containment)
    qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
    tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
    mp = ctx.match_positions(qp, tp, hits, max_pairs=max_pairs)
    assert mp.n_rows == hits.count
    out = hits.to_host(), mp.to_host(), mp.n_slices
    assert mp.n_pairs == len(out[1][1]) == int(out[1][0][-1])
    assert all(p != 0 for p in mp.device_ptrs())
    for o in (mp, qp, tp, hits, Q, T):
        o.free()
    return out


def _compare(ctx, q, t, k, scaled, mol, min_containment=0.0):
    want_hits, want, q_sk, t_sk = matchpos_join.reference(q[0], q[1], t[0], t[1], k, scaled, mol, min_containment)
    got_hits, got, n_slices = _device(ctx, q, t, k, scaled, mol, min_containment)
    for g, w, name in zip(got_hits, want_hits, ("qid", "tid", "intersect", "n_weighted")):
        assert np.array_equal(g, w), name
    for g, w, name in zip(got, want, COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    per_row = (got[0][1:] - got[0][:-1]).astype(np.int64)
    assert np.all(per_row >= want_hits[2])
    # exactly `intersect` pairs where neither sequence repeats a k-mer (all abundances of both sketches are 1)
    plain_q = np.array([np.all(q_sk[2][int(q_sk[0][i]):int(q_sk[0][i + 1])] == 1) for i in range(len(q_sk[0]) - 1)])
    plain_t = np.array([np.all(t_sk[2][int(t_sk[0][i]):int(t_sk[0][i + 1])] == 1) for i in range(len(t_sk[0]) - 1)])
    plain = plain_q[want_hits[0]] & plain_t[want_hits[1]] if len(per_row) else np.zeros(0, bool)
    assert np.array_equal(per_row[plain], want_hits[2][plain].astype(np.int64))
    return want_hits, got, n_slices


def _records(name, n=None):
    recs = oracle.read_fasta(os.path.join(GOLDEN, name))
    return ks.pack([s.upper() for _, s in (recs if n is None else recs[:n])])


# ---- golden ---------------------------------------------------------------------------------------------------------------
def test_search_extract_kmers_device_equals_the_golden_rows(ctx, search_expected):
    args = (os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25), 16, 5, "hp")
    rows = wire.search_extract_kmers_device(*args, ctx=ctx)
    assert rows == wire.search_extract_kmers(*args, ctx=ctx)
    rows.sort(key=lambda r: r["match_name"])
    exp = sorted(search_expected["stitched_rows"], key=lambda r: r["match_name"])
    assert len(rows) == len(exp) == 5
    for g, w in zip(rows, exp):
        for col in search_expected["stitched_columns"]:
            assert str(g[col]) == str(w[col]), col


# ---- real proteins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scaled,mol", [(10, 1, "protein"), (16, 5, "dayhoff"), (24, 5, "hp")])
@pytest.mark.parametrize("targets", ["self", "uncharacterized500"])
def test_real_proteins(ctx, k, scaled, mol, targets):
    q = _records(BCL2_300)
    t = q if targets == "self" else _records(UNCHAR, 500)
    hits, got, _ = _compare(ctx, q, t, k, scaled, mol)
    assert len(hits[0]) > 0 and got[0][-1] > 0


# ---- repeats, blow-up and the refusal ------------------------------------------------------------------------------------------
def _repeat_case():
    """A few sequences that are ONE residue repeated (hp: one hash, thousands of windows on both sides -> m x n pairs in one
    row) next to ordinary, related ones.  hp k=24 scaled=1: the one hash is kept whatever it is."""
    t_res, t_off = synth.proteome(60, stream=901)
    q_res, q_off = synth.queries(40, t_res, t_off, stream=902, frac_related=0.5)
    q = ks.pack([b"A" * 1200, b"L" * 800] + matchpos_join.seqs_of(q_res, q_off) + [b"S" * 500])
    t = ks.pack(matchpos_join.seqs_of(t_res, t_off)[:30] + [b"G" * 1500, b"K" * 700] + matchpos_join.seqs_of(t_res, t_off)[30:])
    return q, t, 24, 1, "hp"


def test_repeats_give_m_times_n_pairs_in_one_row(ctx):
    q, t, k, scaled, mol = _repeat_case()
    hits, got, _ = _compare(ctx, q, t, k, scaled, mol)
    per_row = dict(zip(zip(hits[0].tolist(), hits[1].tolist()), (got[0][1:] - got[0][:-1]).tolist()))
    assert per_row[(0, 30)] == (1200 - 23) * (1500 - 23) and per_row[(1, 30)] == (800 - 23) * (1500 - 23)
    assert per_row[(len(q[1]) - 2, 31)] == (500 - 23) * (700 - 23)
    assert got[0][-1] > 3_000_000  # enough for the MSD match sort to take the list


def test_max_pairs_refuses_before_allocating(ctx):
    q, t, k, scaled, mol = _repeat_case()
    _, got, _ = _device(ctx, q, t, k, scaled, mol)
    n_pairs = int(got[0][-1])
    T = ctx.sketch_batch(t[0], t[1], k, scaled, mol)
    Q = ctx.sketch_batch(q[0], q[1], k, scaled, mol)
    hits = ctx.search(ctx.index_build(T), Q)
    qp = ctx.kmer_positions_table(q[0], q[1], k, scaled, mol)
    tp = ctx.kmer_positions_table(t[0], t[1], k, scaled, mol)
    before = ctx.pool_stats()["bytes_in_use"]
    with pytest.raises(ks.KmerseekError) as e:
        ctx.match_positions(qp, tp, hits, max_pairs=n_pairs - 1)
    assert e.value.status == _lib.KS_ERR_CAPACITY and str(n_pairs) in str(e.value)
    assert ctx.pool_stats()["bytes_in_use"] == before
    mp = ctx.match_positions(qp, tp, hits, max_pairs=n_pairs)  # the limit itself is fine, and the context still works
    for g, w, name in zip(mp.to_host(), got, COLUMNS):
        assert np.array_equal(g, w), name
    mp.free()
    assert ctx.pool_stats()["bytes_in_use"] == before


# ---- starts beyond 2^16 -----------------------------------------------------------------------------------------------------
def test_long_positions(ctx):
    rng = np.random.default_rng(70)
    big = rng.choice(PROTEIN, 70000).astype(np.uint8)
    mutated = big.copy()
    mutated[rng.integers(0, 70000, 900)] = rng.choice(PROTEIN, 900)
    t_res, t_off = synth.proteome(40, stream=903)
    q_res, q_off = synth.queries(30, t_res, t_off, stream=904, frac_related=0.5)
    t = ks.pack(matchpos_join.seqs_of(t_res, t_off)[:20] + [bytes(big)] + matchpos_join.seqs_of(t_res, t_off)[20:])
    q = ks.pack(matchpos_join.seqs_of(q_res, q_off) + [bytes(rng.choice(PROTEIN, 333).astype(np.uint8)) + bytes(mutated)])
    hits, got, _ = _compare(ctx, q, t, 10, 1, "protein")
    assert got[1].max() > 65536 + 300 and got[2].max() > 65536 and got[4].max() > 69000


# ---- thresholded hits -------------------------------------------------------------------------------------------------------
def test_filtered_hits_drop_their_pairs(ctx):
    t = synth.proteome(300, stream=905)
    q = synth.queries(200, t[0], t[1], stream=906, frac_related=0.6)
    all_hits, all_got, _ = _compare(ctx, q, t, 7, 1, "protein")
    hits, got, _ = _compare(ctx, q, t, 7, 1, "protein", min_containment=0.5)
    assert 0 < len(hits[0]) < len(all_hits[0]) and 0 < got[0][-1] < all_got[0][-1]


# ---- forced row slices --------------------------------------------------------------------------------------------------------
def test_forced_row_slices_give_the_same_result(monkeypatch):
    t = synth.proteome(200, stream=907)
    q = synth.queries(150, t[0], t[1], stream=908, frac_related=0.6)
    with ks.Context(0, follow_debug_env=True) as c:
        hits, plain, n1 = _compare(c, q, t, 7, 1, "protein")
        assert n1 == 1 and len(hits[0]) > 20
        for bits in ("3", "1"):
            monkeypatch.setenv("KS_DEBUG_MATCHPOS_ROW_BITS", bits)
            got_hits, sliced, n = _device(c, q, t, 7, 1, "protein")
            per = (1 << int(bits)) - 1
            assert n == (len(hits[0]) + per - 1) // per > 1
            for g, w, name in zip(sliced, plain, COLUMNS):
                assert np.array_equal(g, w), (bits, name)
        monkeypatch.delenv("KS_DEBUG_MATCHPOS_ROW_BITS")
        q2, t2, k, scaled, mol = _repeat_case()  # ... and with the MSD sort inside every slice
        _, plain2, _ = _device(c, q2, t2, k, scaled, mol)
        monkeypatch.setenv("KS_DEBUG_MATCHPOS_ROW_BITS", "3")
        _, sliced2, n = _device(c, q2, t2, k, scaled, mol)
        assert n > 1
        for g, w, name in zip(sliced2, plain2, COLUMNS):
            assert np.array_equal(g, w), name


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_inputs_that_do_not_belong_together_are_refused(ctx):
    t = synth.proteome(120, stream=909)
    q = synth.queries(80, t[0], t[1], stream=910, frac_related=0.6)
    other = synth.proteome(80, stream=911)  # unrelated to t: its windows share no 10-mer with the targets
    T = ctx.sketch_batch(t[0], t[1], 10, 1, "protein")
    Q = ctx.sketch_batch(q[0], q[1], 10, 1, "protein")
    hits = ctx.search(ctx.index_build(T), Q)
    assert hits.count > 0
    qp = ctx.kmer_positions_table(q[0], q[1], 10, 1, "protein")
    tp = ctx.kmer_positions_table(t[0], t[1], 10, 1, "protein")
    cases = ((lambda: (ctx.kmer_positions_table(q[0], q[1], 11, 1, "protein"), tp), "parameters"),
             (lambda: (qp, ctx.kmer_positions_table(t[0], t[1], 10, 2, "protein")), "parameters"),
             (lambda: (qp, ctx.kmer_positions_table(t[0], t[1], 10, 1, "dayhoff")), "parameters"),
             (lambda: (ctx.kmer_positions_table(other[0], other[1], 10, 1, "protein"), tp), "belong"),  # rows without pairs
             (lambda: (tp, qp), "belong"))
    for make, why in cases:
        bad_q, bad_t = make()
        before = ctx.pool_stats()["bytes_in_use"]
        with pytest.raises(ks.KmerseekError) as e:
            ctx.match_positions(bad_q, bad_t, hits)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG and why in str(e.value), str(e.value)
        assert ctx.pool_stats()["bytes_in_use"] == before
        for o in (bad_q, bad_t):
            if o is not qp and o is not tp:
                o.free()
    mp = ctx.match_positions(qp, tp, hits)  # the context stays usable
    want_hits, want, _, _ = matchpos_join.reference(q[0], q[1], t[0], t[1], 10, 1, "protein")
    for g, w, name in zip(mp.to_host(), want, COLUMNS):
        assert np.array_equal(g, w), name


# ---- edges ------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    t = synth.proteome(50, stream=912)
    unrelated = synth.proteome(20, stream=913)
    hits, got, n = _compare(ctx, unrelated, t, 10, 1, "protein")  # no hits
    assert len(hits[0]) == 0 and got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])
    short = ks.pack([b"ACDEFG", b"", b"KLMNP"])  # a query batch without a kept window (every record shorter than k)
    hits, got, _ = _compare(ctx, short, t, 10, 1, "protein")
    assert len(hits[0]) == 0 and got[0].tolist() == [0]
    longest = max(matchpos_join.seqs_of(*t), key=len)
    assert len(longest) > 250
    one_t = ks.pack([longest])
    one_q = ks.pack([longest[5:200]])
    hits, got, _ = _compare(ctx, one_q, one_t, 10, 1, "protein")  # exactly one row
    assert len(hits[0]) == 1 and got[0].tolist() == [0, 186] and got[3].tolist() == [0] and got[5].tolist() == [5]
    assert got[4].tolist() == [195] and got[6].tolist() == [200]


def test_table_objects_agree_with_the_fetching_calls(ctx):
    t = synth.proteome(40, stream=914)
    tab = ctx.kmer_positions_table(t[0], t[1], 16, 5, "dayhoff")
    want = ctx.kmer_positions(t[0], t[1], 16, 5, "dayhoff")
    assert tab.count == len(want[0])
    for g, w in zip(tab.to_host(), want):
        assert np.array_equal(g, w)
    d_res, d_off = ctx.to_device(np.concatenate([t[0], np.zeros(16, np.uint8)])), ctx.to_device(t[1])
    tab2 = ctx.kmer_positions_table_device(d_res.ptr, d_off.ptr, len(t[1]) - 1, int(t[1][-1]), 16, 5, "dayhoff")
    for g, w in zip(tab2.to_host(), want):
        assert np.array_equal(g, w)
