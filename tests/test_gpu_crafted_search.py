"""GPU: the search half on hand-made sketches (tests/crafted_sketches.py) — hashes on the edges of the join arithmetic and
abundances on the edges of the match record — uploaded with ks_sketches_from_host and held, exactly, against plain numpy /
Python references: every quantity here is an integer, and `ss` is bit-identical to the host loop by the header's contract.

- index_build + search equals the numpy join: rows, order, count, n_pair_instances;
- abund_stats leaves the four columns alone and gives the replica's median2 / ss (wide_records: on a fixed stride of rows, the
  first, the last and every row with n_weighted >= 2^32);
- min_containment keeps exactly the rows of the host's f64 test, with and without statistics;
- the union equals unique hashes with u64 sums clipped to 2^32 - 1;
- wide_records: 2^20 query sequences make 64-bit match records (the all-ones record among them), one sequence more makes
  slices of 2^20; the transport word escapes exactly the rows the reference predicts and round-trips;
- all of it under the search-side knob sets, the index rebuilt per set.

Sketches that come from the host carry no partitioned postings, so every search here groups its query postings with the dense
partition from the CSR (partition_path 3, no bucket scatter): asserted, so that a change of that cannot pass unnoticed.
Every input is valid by the ABI's own rules: a status code from the library is a failure to look into."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
from test_gpu_search_rows import THRESHOLDS  # noqa: E402

FP_KERNELS = {"staged": {"JOIN_FP": "1", "JOIN_SPARSE": "0"}, "sparse": {"JOIN_FP": "1", "JOIN_SPARSE": "1"}}
KNOB_SETS = {"default": {}, "key_columns": {"JOIN_FP": "0"}, "key_columns_split": {"JOIN_FP": "0", "JOIN_SPLIT": "3"}}
for _k, _v in FP_KERNELS.items():
    KNOB_SETS["fp_" + _k] = dict(_v)
for _k, _v in FP_KERNELS.items():
    KNOB_SETS["fp_" + _k + "_segs"] = dict(_v, JOIN_SEGS="1")
for _k, _v in FP_KERNELS.items():
    KNOB_SETS["fp_" + _k + "_coarse"] = dict(_v, FP_COARSEN="18")
for _k, _v in FP_KERNELS.items():
    KNOB_SETS["fp_" + _k + "_bucket64"] = dict(_v, BUCKET="64")
KNOB_SETS.update({"index_lsd": {"INDEX_LSD": "1"}, "pairs_lsd": {"PAIRS_LSD": "1"}, "rows_ticket": {"ROWS_TICKET": "1"}})
SMALL = [n for n in cs.NAMES if n != "wide_records"]
# The four big prefix_edges cases (1.6 - 2.8 M target postings each) run under nine of the sets: the ones whose paths depend on
# the size (segments need >= 64 buckets, the MSD match sort >= 65,536 matches, the index sorts) and one of each join kernel.
BIG = [n for n in SMALL if n.startswith("prefix_edges") and n != f"prefix_edges_s{cs.U32_MAX}"]
BIG_SKIPS = ("key_columns_split", "fp_staged_coarse", "fp_sparse_coarse", "fp_staged_bucket64", "rows_ticket")
# one_bucket under the query-table kernel with coarsened fingerprints is left out too: all 63,000 postings of the one bucket are
# then candidates of every query posting, and that one case took a quarter of this file's run time (10.6 s of 41 s); the staged
# kernel runs the same family with the same coarse fingerprints, and the query-table kernel runs it with exact ones.
FAMILY_KNOBS = [(n, k) for n in SMALL for k in KNOB_SETS
                if not (n in BIG and k in BIG_SKIPS) and (n, k) != ("one_bucket", "fp_sparse_coarse")]
WIDE_KNOBS = ("default", "pairs_lsd", "rows_ticket")  # the big family: the default set, the other match sort, ticket-ordered rows

_REF = {}


def _ref(name, batch=None):
    """the references of a family, computed once: rows, pairs, (rows whose statistics are checked, median2, ss)"""
    key = (name, batch)
    if key not in _REF:
        _, _, _, _, T, Q = cs.family(name)
        if name == "wide_records":
            Q = cs.wide_batches(Q)[batch]
        rows = cs.ref_join(T, Q)
        which = np.array(cs.wide_stat_rows(rows) if name == "wide_records" else np.arange(len(rows[0])), np.int64)
        _REF[key] = (T, Q, rows, int(rows[2].sum()), which, cs.ref_stats(rows, T, Q, which.tolist()))
    return _REF[key]


def _eq_rows(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (label, j, len(g), len(w))


def _bits_eq(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _upload(ctx, name, S):
    _, ksize, scaled, moltype, _, _ = cs.family(name)
    return ctx.sketches_from_host(S[0], S[1], S[2], ksize, scaled, moltype)


def _set(monkeypatch, knobs):
    for key, v in knobs.items():
        monkeypatch.setenv("KS_DEBUG_" + key, v)


def _expected_join(knobs, n_postings, n_q, moltype="protein"):
    """(segments of the match list, capacity of one) of a context's first search, replayed from ks_search.hip's host code"""
    per = 64 if "BUCKET" in knobs else 3072
    pbits = 0
    while pbits < 16 and (n_postings >> pbits) > per:
        pbits += 1
    n_buckets = 1 << pbits
    fp = (moltype != "hp") if "JOIN_FP" not in knobs else knobs["JOIN_FP"] != "0"
    per_bucket = n_q // n_buckets
    reservations = n_buckets * max(1, -(-per_bucket // 5120))
    n_segs = 64 if fp and n_buckets >= 64 and (reservations >= 8192 or "JOIN_SEGS" in knobs) else 1
    cap = max(1 << 20, n_q)
    return n_segs, (cap if n_segs == 1 else cap // n_segs + cap // n_segs // 8 + 4096)


def _check_search(ctx, name, knobs, label, batch=None):
    T, Q, rows, pairs, which, (want_m2, want_ss) = _ref(name, batch)
    dT, dQ = _upload(ctx, name, T), _upload(ctx, name, Q)
    assert dT.n_hashes == len(T[1]) and dQ.n_seqs == len(Q[0]) - 1
    ix = ctx.index_build(dT)  # (under the knob set: the layout is a property of the index)
    assert ix.n_postings == len(T[1]) and ix.n_targets == len(T[0]) - 1
    sliced = cs.bits_for(len(T[0]) - 1) + cs.bits_for(len(Q[0]) - 1) + cs.bits_for_value(int(T[2].max())) > 64
    H = ctx.search(ix, dQ)
    if not sliced:  # the first search of this context: did the join repeat exactly when its first list was too small?
        n_segs, seg_cap = _expected_join(knobs, len(T[1]), len(Q[1]))
        retries = ctx.search_stats()["join_retries"]
        if n_segs == 1:
            assert retries == (1 if pairs > seg_cap else 0), (label, retries, pairs, seg_cap)
        elif pairs > n_segs * seg_cap:  # (some segment has to overflow)
            assert retries == 1, (label, retries, pairs, seg_cap)
    assert H.count == len(rows[0]) and H.n_pair_instances == pairs, (label, H.count, len(rows[0]), H.n_pair_instances, pairs)
    _eq_rows(H.to_host(), rows, (label, "plain"))
    assert H.partition_path == 3 and H.bucket_posting_bytes == 0, label
    assert not H.has_abund_stats
    Hs = ctx.search(ix, dQ, abund_stats=True)
    _eq_rows(Hs.to_host(), rows, (label, "stats"))
    assert Hs.has_abund_stats and Hs.n_pair_instances == pairs
    m2, ss = Hs.abund_stats_to_host()
    assert len(m2) == len(ss) == len(rows[0])
    bad = np.nonzero(m2[which] != want_m2)[0]
    assert len(bad) == 0, (label, "median2", int(which[bad[0]]), int(m2[which][bad[0]]), int(want_m2[bad[0]]))
    bad = np.nonzero(ss[which].view(np.uint64) != want_ss.view(np.uint64))[0]
    assert len(bad) == 0, (label, "ss", int(which[bad[0]]), float(ss[which][bad[0]]), float(want_ss[bad[0]]))
    for thr in THRESHOLDS:
        sel = cs.keep(rows, Q, thr)
        for with_stats in (False, True):
            Hf = ctx.search(ix, dQ, min_containment=thr, abund_stats=with_stats)
            assert Hf.count == int(sel.sum())
            _eq_rows(Hf.to_host(), [a[sel] for a in rows], (label, thr, with_stats))
            if with_stats:
                f2, fs = Hf.abund_stats_to_host()
                assert np.array_equal(f2, m2[sel]) and _bits_eq(fs, ss[sel]), (label, thr)
            else:
                assert not Hf.has_abund_stats
            Hf.free()
        if thr == 0.0:
            assert sel.all()
        if thr == 1.5:
            assert not sel.any()
    return dT, dQ, ix, H, Hs


@pytest.mark.parametrize("name,knob", FAMILY_KNOBS)
def test_family_under_knob_set(monkeypatch, name, knob):
    knobs = KNOB_SETS[knob]
    _ref(name)
    _set(monkeypatch, knobs)
    ctx = ks.Context(0, follow_debug_env=True)  # (fresh: the size of the first match list depends on the context's history)
    try:
        _check_search(ctx, name, knobs, (name, knob))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", cs.NAMES)
def test_union_equals_the_reference(name):
    T = cs.family(name)[4]
    want = cs.ref_union(T)
    with ks.Context(0) as ctx:
        U = _upload(ctx, name, T).union()
        assert U.n_seqs == 1 and U.n_hashes == len(want[1])
        got = U.to_host()
        _eq_rows(got, want, (name, "union"))
        if name == "union_saturation":
            assert int(np.count_nonzero(got[2] == cs.U32_MAX)) >= 4 and cs.U32_MAX - 1 in got[2] and 0 in got[2]
        # the union of a union is itself (one sequence: every run has one posting)
        _eq_rows(U.union().to_host(), want, (name, "union of the union"))


@pytest.mark.parametrize("knob", WIDE_KNOBS)
def test_wide_records_full_width_and_natural_slices(monkeypatch, knob):
    knobs = KNOB_SETS[knob]
    rows20, rows21 = _ref("wide_records", 0)[2], _ref("wide_records", 1)[2]
    n20 = len(rows20[0])
    # the larger batch: the same rows, then the rows of the one sequence behind them
    assert len(rows21[0]) > n20 and all(np.array_equal(a[:n20], b) for a, b in zip(rows21, rows20))
    assert np.all(rows21[0][n20:] == cs.WIDE_N_Q) and int(rows20[0][-1]) == cs.WIDE_N_Q - 1 and int(rows20[1][-1]) == cs.WIDE_N_T - 1
    _set(monkeypatch, knobs)
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        # 12 + 20 + 32 bits: one list, the all-ones record in it (the last match of the last row)
        _, dQ, ix, _, _ = _check_search(ctx, "wide_records", knobs, ("wide 2^20", knob), batch=0)
        T = cs.family("wide_records")[4]
        assert int(rows20[3][-1]) >= cs.U32_MAX  # (that row holds the abundance 2^32 - 1 of the all-ones record)
        # one sequence more: 65 bits, slices of 2^20 sequences; the second slice is that sequence, and it has hits
        _check_search(ctx, "wide_records", knobs, ("wide 2^20 + 1", knob), batch=1)
        # and the context still works
        _eq_rows(ctx.search(ix, dQ).to_host(), rows20, ("wide again", knob))
        assert int(T[2].max()) == cs.U32_MAX
    finally:
        ctx.close()


def _dev_cols(ctx, n):
    return (ctx.to_device(np.zeros(max(n, 1), np.uint32)), ctx.to_device(np.zeros(max(n, 1), np.uint32)),
            ctx.to_device(np.zeros(max(n, 1), np.uint32)), ctx.to_device(np.zeros(max(n, 1), np.uint64)))


def _download(ctx, buf, n, dtype):
    return buf.to_host(dtype, n)  # (stream-ordered behind the asynchronous calls that filled the buffer)


def test_wide_records_transport_and_device_copies():
    T, Q, rows, _, _, _ = _ref("wide_records", 0)
    n = len(rows[0])
    qbits, tbits = cs.bits_for(cs.WIDE_N_Q), cs.bits_for(cs.WIDE_N_T)
    v = (64 - qbits - tbits) // 2
    assert v == 16
    vmax = (1 << v) - 1
    esc_want = np.nonzero((rows[2] >= vmax) | (rows[3] >= np.uint64(vmax)))[0]  # (all-ones is the marker: it escapes too)
    assert 0 < len(esc_want) < n
    assert np.any(rows[3] == np.uint64(vmax)) and np.any(rows[3] == np.uint64(vmax + 1)) and np.any(rows[3] >= np.uint64(1 << 32))
    with ks.Context(0) as ctx:
        H = ctx.search(ctx.index_build(_upload(ctx, "wide_records", T)), _upload(ctx, "wide_records", Q))
        assert H.count == n
        for esc_cap in (n, max(1, len(esc_want) // 3)):
            packed = ctx.to_device(np.zeros(n, np.uint64))
            e_row, e_is, e_nw = (ctx.to_device(np.zeros(esc_cap, np.uint32)), ctx.to_device(np.zeros(esc_cap, np.uint32)),
                                 ctx.to_device(np.zeros(esc_cap, np.uint64)))
            n_esc = ctx.to_device(np.zeros(1, np.uint32))
            H.pack64_to_device(packed.ptr, e_row.ptr, e_is.ptr, e_nw.ptr, n_esc.ptr, esc_cap, qbits, tbits)
            got_esc = int(_download(ctx, n_esc, 1, np.uint32)[0])
            assert got_esc == len(esc_want), (esc_cap, got_esc, len(esc_want))  # (the full count, also past esc_cap)
            if esc_cap < n:
                continue
            cols = _dev_cols(ctx, n)
            ctx.unpack_hits64_device(packed.ptr, n, qbits, tbits, *[c.ptr for c in cols])
            got = [_download(ctx, c, n, dt) for c, dt in zip(cols, (np.uint32, np.uint32, np.uint32, np.uint64))]
            er, ei, en = _download(ctx, e_row, got_esc, np.uint32), _download(ctx, e_is, got_esc, np.uint32), _download(ctx, e_nw, got_esc, np.uint64)
            assert np.array_equal(np.sort(er), esc_want)
            assert np.all(got[2][esc_want] == vmax) and np.all(got[3][esc_want] == np.uint64(vmax))  # the markers
            got[2][er] = ei
            got[3][er] = en
            _eq_rows(got, rows, "transport round trip")
        # ids shifted to a global numbering on the way into caller-owned buffers
        cols = _dev_cols(ctx, n)
        H.copy_to_device(*[c.ptr for c in cols], qid_base=3 << 20, tid_base=cs.U32_MAX - cs.WIDE_N_T + 1)
        got = [_download(ctx, c, n, dt) for c, dt in zip(cols, (np.uint32, np.uint32, np.uint32, np.uint64))]
        want = (rows[0] + np.uint32(3 << 20), rows[1] + np.uint32(cs.U32_MAX - cs.WIDE_N_T + 1), rows[2], rows[3])
        _eq_rows(got, want, "copy_to_device with bases")
        assert int(got[1].max()) == cs.U32_MAX


@pytest.mark.parametrize("name", ["one_bucket", "zero_abund", "union_saturation"])
def test_copy_to_device_round_trips(name):
    T, Q, rows, _, _, _ = _ref(name)
    n = len(rows[0])
    with ks.Context(0) as ctx:
        H = ctx.search(ctx.index_build(_upload(ctx, name, T)), _upload(ctx, name, Q))
        cols = _dev_cols(ctx, n)
        H.copy_to_device(*[c.ptr for c in cols], qid_base=1000, tid_base=7)
        got = [_download(ctx, c, n, dt) for c, dt in zip(cols, (np.uint32, np.uint32, np.uint32, np.uint64))]
        _eq_rows(got, (rows[0] + np.uint32(1000), rows[1] + np.uint32(7), rows[2], rows[3]), name)


def _fuzz():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
    spec = importlib.util.spec_from_file_location("fuzz_parity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("knob", ["default", "key_columns", "fp_sparse_coarse"])
def test_crafted_fuzz_under_knob_set(knob):
    assert _fuzz().run_crafted(40, 9000 + list(KNOB_SETS).index(knob), knobs=KNOB_SETS[knob]) == 0
