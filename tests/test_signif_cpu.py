"""CPU-side checks of the significance columns (ks_corpus_build / ks_hits_significance): the definitions, restated in
tests/signif_ref.py, reproduce the five computed columns of the reference's multisearch fixture bit for bit; the header,
_lib.py, engine and wire expose the new names; bad arguments are refused before any device work.  No GPU compute here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import signif_ref  # noqa: E402
from conftest import load_golden  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, engine, wire  # noqa: E402
from oracle import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTED = ("prob_overlap", "prob_overlap_adjusted", "containment_adjusted", "containment_adjusted_log10", "tf_idf_score")
NEW_SYMBOLS = ["ks_corpus_build", "ks_corpus_n_hashes", "ks_corpus_n_docs", "ks_corpus_total_abund", "ks_corpus_copy_to_host",
               "ks_corpus_free", "ks_hits_significance", "ks_signif_n_rows", "ks_signif_device_prob_overlap",
               "ks_signif_device_tf_idf", "ks_signif_copy_to_host", "ks_signif_free"]


@pytest.fixture(scope="module")
def expected():
    return load_golden("multisearch_expected.json")


@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def golden_sets(golden_sketches, ced9_records):
    """(query names, Q, target names, T): ced9 sketched by the oracle, the 25 golden hp.k16.scaled5 sketches as targets"""
    q_res, q_off = oracle.pack([s for _, s in ced9_records])
    Q = oracle.sketch_batch(q_res, q_off, 16, 5, "hp")
    sigs = golden_sketches["hp.k16.scaled5"]["signatures"]
    offs = np.zeros(len(sigs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s["mins"]) for s in sigs])
    T = (offs, np.array([h for s in sigs for h in s["mins"]], np.uint64), np.array([a for s in sigs for a in s["abundances"]], np.uint32))
    return [n for n, _ in ced9_records], Q, [s["name"] for s in sigs], T


def test_fixture_is_the_sixteen_column_file(expected):
    assert len(expected["columns"]) == 16 and expected["columns"][-5:] == list(COMPUTED)
    assert len(expected["rows"]) == 5 and all(list(r) == sorted(expected["columns"]) for r in expected["rows"])


def test_reference_reproduces_the_fixture_bit_for_bit(expected, golden_sketches, ced9_records):
    """float(text) == value for all 25 values of the five computed columns: the definitions, their order of operations included"""
    qn, Q, tn, T = golden_sets(golden_sketches, ced9_records)
    qid, tid, isect = signif_ref.join(Q, T)
    po, tf, shared = signif_ref.significance(Q, T, qid, tid)
    assert np.array_equal(shared, isect)
    by_name = {tn[t]: r for r, t in enumerate(tid.tolist())}
    assert sorted(by_name) == sorted(r["match_name"] for r in expected["rows"])
    q_size = int(Q[0][1] - Q[0][0])
    for want in expected["rows"]:
        r = by_name[want["match_name"]]
        assert float(want["intersect_hashes"]) == float(isect[r])
        adj, c_adj, c_log = signif_ref.derived(float(po[r]), int(isect[r]), q_size, len(qn), len(tn))
        got = dict(zip(COMPUTED, (float(po[r]), adj, c_adj, c_log, float(tf[r]))))
        for col in COMPUTED:
            print(want["match_name"][:20], col, want[col], repr(got[col]))
            assert float(want[col]) == got[col], (want["match_name"], col, want[col], got[col])


def test_multisearch_rows_print_the_fixture(expected, golden_sketches, ced9_records):
    """wire.multisearch_rows on the reference's sums: every column of the fixture, the numeric ones parsed as f64"""
    qn, Q, tn, T = golden_sets(golden_sketches, ced9_records)
    qid, tid, isect = signif_ref.join(Q, T)
    po, tf, _ = signif_ref.significance(Q, T, qid, tid)
    assert wire.MULTISEARCH_COLUMNS == expected["columns"]
    rows = wire.multisearch_rows(qn, Q[0], Q[1], tn, T[0], T[1], (qid, tid, isect, None), po, tf, 16, 5, "hp")
    got = {r["match_name"]: r for r in rows}
    text = ("query_name", "query_md5", "match_name", "match_md5", "moltype")
    for want in expected["rows"]:
        g = got[want["match_name"]]
        assert list(g) == expected["columns"]
        for col in expected["columns"]:
            if col in text:
                assert str(g[col]) == want[col], col
            else:
                assert float(g[col]) == float(want[col]), (col, g[col], want[col])
        assert g["intersect_hashes"] == want["intersect_hashes"]  # printed as the fixture prints it: 2.0
        assert "e" not in g["prob_overlap"]


def test_format_f64_reads_back_and_never_uses_an_exponent():
    for x in (2.0, 2.3191094619666044e-05, 70.4, 1e22, 1.5e300, 0.0, 5e-324, 1.8475726591421122, 123456789012345680.0):
        s = wire.format_f64(x)
        assert float(s) == x and "e" not in s.lower() and "." in s, s
    assert wire.format_f64(2.3191094619666044e-05) == "0.000023191094619666044" and wire.format_f64(2.0) == "2.0"
    assert wire.format_f64(float("nan")) == "NaN" and wire.format_f64(float("inf")) == "inf"


def test_reference_on_a_hand_made_case():
    """Two queries, three targets, done by hand: merged-query frequencies for prob_overlap, the single query's for tf_idf."""
    import math
    Q = (np.array([0, 2, 3], np.uint64), np.array([5, 9, 5], np.uint64), np.array([1, 3, 2], np.uint32))
    T = (np.array([0, 2, 3, 3], np.uint64), np.array([5, 7, 5], np.uint64), np.array([4, 1, 5], np.uint32))
    h, s, d, tot = signif_ref.corpus(Q)
    assert (h.tolist(), s.tolist(), d.tolist(), tot) == ([5, 9], [3, 3], [2, 1], 6)
    h, s, d, tot = signif_ref.corpus(T)
    assert (h.tolist(), s.tolist(), d.tolist(), tot) == ([5, 7], [9, 1], [2, 1], 10)
    qid, tid, isect = signif_ref.join(Q, T)
    assert (qid.tolist(), tid.tolist(), isect.tolist()) == ([0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1])
    po, tf, _ = signif_ref.significance(Q, T, qid, tid)
    idf2 = math.log((1.0 + 3.0) / (1.0 + 2.0)) + 1.0  # 3 targets (the empty one counts), hash 5 in two of them
    assert po.tolist() == [(3.0 / 6.0) * (9.0 / 10.0)] * 4
    assert tf.tolist() == [(1.0 / 4.0) * idf2, (1.0 / 4.0) * idf2, (2.0 / 2.0) * idf2, (2.0 / 2.0) * idf2]
    assert [len(signif_ref.join(Q, T, c)[0]) for c in (0.5, 0.51)] == [4, 2]


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return m.group(1).split()[-1], len([p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"])


def test_new_symbols_exported_with_declared_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        ret, n_params = _prototype(name)
        assert len(args) == n_params, (name, len(args), n_params)
        assert (res is C.c_int) == (ret == "int"), (name, ret)
    assert C.sizeof(_lib.ks_signif_opts) == 8 and _lib.ks_signif_opts.reserved.offset == 4


def test_engine_and_wire_expose_the_new_names():
    for name in ("corpus",):
        assert callable(getattr(engine.Sketches, name))
    assert callable(engine.Context.significance)
    for name in ("to_host", "n_hashes", "n_docs", "total_abund", "free"):
        assert hasattr(engine.Corpus, name), name
    for name in ("to_host", "device_ptrs", "n_rows", "free"):
        assert hasattr(engine.Significance, name), name
    assert callable(wire.multisearch_rows) and callable(wire.do_multisearch)
    assert len(wire.MULTISEARCH_COLUMNS) == 16


@pytest.mark.parametrize("opts", [None, (0, 0), (0, 7), (1, 0), (0x80000000, 3)])
def test_bad_or_null_arguments_are_invalid_arg_without_a_context(lib, opts):
    out = C.c_void_p()
    p = C.byref(_lib.ks_signif_opts(*opts)) if opts is not None else None
    assert lib.ks_hits_significance(None, None, None, None, None, None, p, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_corpus_build(None, None, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert not out.value


def test_accessors_accept_null(lib):
    assert lib.ks_corpus_n_hashes(None) == 0 and lib.ks_corpus_n_docs(None) == 0 and lib.ks_corpus_total_abund(None) == 0
    assert lib.ks_signif_n_rows(None) == 0
    assert not lib.ks_signif_device_prob_overlap(None) and not lib.ks_signif_device_tf_idf(None)
    assert lib.ks_corpus_copy_to_host(None, None, None, None, None) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_signif_copy_to_host(None, None, None, None) == _lib.KS_ERR_INVALID_ARG
    lib.ks_corpus_free(None)
    lib.ks_signif_free(None)


def test_every_entry_point_of_the_new_unit_is_guarded():
    src = open(os.path.join(ROOT, "kmerseek_amd", "csrc", "ks_signif.hip")).read()
    names = re.findall(r'^extern "C" int (\w+)\(', src, re.M)
    assert sorted(names) == ["ks_corpus_build", "ks_corpus_copy_to_host", "ks_hits_significance", "ks_signif_copy_to_host"]
    for m in re.finditer(r'^extern "C" int (\w+)\([^{]*\{', src, re.M):
        assert "ks_guard(" in src[m.end():m.end() + 120], m.group(1)
    assert "log(" not in re.sub(r"std::log\(", "", re.sub(r"//.*", "", src))  # the device never evaluates a logarithm
