"""CPU-side checks of ks_match_positions (where each hit's shared k-mers lie): the new symbols are exported with the prototypes
_lib.py declares, bad arguments are refused with KS_ERR_INVALID_ARG before any device work (no context needed), the engine
passes its options on, and the host half (wire.stitch_match_positions) turns the pairs of a CPU join of ced9 vs BCL2-25 into
exactly the reference's five stitched rows.  No GPU compute here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, engine, wire  # noqa: E402
from oracle import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ks_match_positions", "ks_matchpos_n_rows", "ks_matchpos_n_pairs", "ks_matchpos_n_slices",
               "ks_matchpos_device_row_offsets", "ks_matchpos_device_q_start", "ks_matchpos_device_t_start",
               "ks_matchpos_device_q_lo", "ks_matchpos_device_q_hi", "ks_matchpos_device_t_lo", "ks_matchpos_device_t_hi",
               "ks_matchpos_copy_to_host", "ks_matchpos_free", "ks_kmerpos_params"]


@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


def _prototype(name):
    """Parameter count and the return type word of `name` in include/kmerseek_amd.h."""
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
    assert C.sizeof(_lib.ks_matchpos_opts) == 16
    assert _lib.ks_matchpos_opts.max_pairs.offset == 8
    assert lib.ks_abi_version() == 1


def _opts(flags=0, reserved=0, max_pairs=0):
    return _lib.ks_matchpos_opts(flags, reserved, max_pairs)


@pytest.mark.parametrize("opts", [None, _opts(), _opts(0, 0, 5), _opts(0, 7, 0), _opts(1, 0, 0), _opts(0x80000000, 0, 9), _opts(2, 3, 1)])
def test_bad_or_null_arguments_are_invalid_arg_without_a_context(lib, opts):
    out = C.c_void_p()
    p = C.byref(opts) if opts is not None else None
    assert lib.ks_match_positions(None, None, None, None, p, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_match_positions(None, None, None, None, p, None) == _lib.KS_ERR_INVALID_ARG
    assert not out.value


def test_accessors_accept_null(lib):
    assert lib.ks_matchpos_n_rows(None) == 0 and lib.ks_matchpos_n_pairs(None) == 0 and lib.ks_matchpos_n_slices(None) == 0
    for col in engine.MatchPositions._COLUMNS:
        assert not getattr(lib, "ks_matchpos_device_" + col)(None)
    assert lib.ks_matchpos_copy_to_host(None, None, None, None, None, None, None, None, None) == _lib.KS_ERR_INVALID_ARG
    lib.ks_matchpos_free(None)
    p = _lib.ks_params(ksize=3, scaled=4, moltype=1, flags=0, seed=9)
    lib.ks_kmerpos_params(None, C.byref(p))
    assert (p.ksize, p.scaled, p.moltype, p.seed) == (3, 4, 1, 9)  # untouched


class _Recorder:
    """Stands in for the loaded library: records which entry point a Context method called, and with what options."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            opts = None
            for a in args:
                obj = getattr(a, "_obj", None)
                if isinstance(obj, _lib.ks_matchpos_opts):
                    opts = (obj.flags, obj.reserved, obj.max_pairs)
            self.calls.append((name, opts, len(args)))
            return _lib.KS_OK
        return call


def test_engine_passes_its_options_on(monkeypatch):
    for cls in (engine.Hits, engine.KmerPositions, engine.MatchPositions):
        monkeypatch.setattr(cls, "__del__", lambda self: None, raising=False)
    ctx = engine.Context.__new__(engine.Context)
    ctx._L = _Recorder()
    ctx._h = C.c_void_p(1)
    ctx._pinned, ctx._close_pending = 0, True  # (never destroys anything)
    qp, tp, hits = (cls.__new__(cls) for cls in (engine.KmerPositions, engine.KmerPositions, engine.Hits))
    qp._h = tp._h = hits._h = C.c_void_p(2)
    m = ctx.match_positions(qp, tp, hits)
    assert isinstance(m, engine.MatchPositions)
    ctx.match_positions(qp, tp, hits, max_pairs=12345678901)
    assert ctx._L.calls == [("ks_match_positions", (0, 0, 0), 6), ("ks_match_positions", (0, 0, 12345678901), 6)]
    ctx._L.calls.clear()
    res, offs = np.zeros(4, np.uint8), np.array([0, 4], np.uint64)
    assert isinstance(ctx.kmer_positions_table(res, offs, 3, 1, "protein"), engine.KmerPositions)
    assert isinstance(ctx.kmer_positions_table_device(16, 32, 1, 4, 3, 1, "protein"), engine.KmerPositions)
    assert [c[0] for c in ctx._L.calls] == ["ks_kmer_positions", "ks_kmer_positions_device"]


def test_join_restatement_on_a_hand_made_case():
    """The CPU join itself, on tables small enough to do by hand: a repeated hash gives m x n pairs, pairs outside the hits drop."""
    q_tab = (np.array([0, 0, 0, 1], np.uint32), np.array([0, 2, 5, 1], np.uint32), np.array([7, 9, 7, 7], np.uint64))
    t_tab = (np.array([0, 0, 1, 2], np.uint32), np.array([3, 4, 0, 8], np.uint32), np.array([7, 7, 9, 7], np.uint64))
    offs, a, b, qlo, qhi, tlo, thi = matchpos_join.join(q_tab, t_tab, np.array([0, 0, 1], np.uint32), np.array([0, 1, 2], np.uint32), 3)
    assert offs.tolist() == [0, 4, 5, 6]
    assert list(zip(a.tolist(), b.tolist())) == [(0, 3), (0, 4), (5, 3), (5, 4), (2, 0), (1, 8)]  # (q0, t2) and (q1, t0) are no hits
    assert (qlo.tolist(), qhi.tolist(), tlo.tolist(), thi.tolist()) == ([0, 2, 1], [8, 5, 4], [3, 0, 8], [7, 3, 11])


def test_stitch_match_positions_gives_the_golden_rows(search_expected, ced9_records, bcl2_records):
    """ced9 vs BCL2-25, hp k=16 scaled=5: the pairs of the CPU join, stitched, are the reference's five rows in every column."""
    k, sc, mol = 16, 5, "hp"
    q_res, q_off = oracle.pack([s for _, s in ced9_records])
    t_res, t_off = oracle.pack([s for _, s in bcl2_records])
    hits, (offs, a, b, *_), _, _ = matchpos_join.reference(q_res, q_off, t_res, t_off, k, sc, mol)
    assert len(hits[0]) == 5 and np.all(offs[1:] - offs[:-1] >= hits[2])
    got = wire.stitch_match_positions(ced9_records, bcl2_records, hits[0], hits[1], offs, a, b, k, mol)
    assert [(r["query_start"], r["query_end"]) for r in got] == sorted((r["query_start"], r["query_end"]) for r in got)
    got.sort(key=lambda r: r["match_name"])
    exp = sorted(search_expected["stitched_rows"], key=lambda r: r["match_name"])
    assert len(got) == 5
    for g, w in zip(got, exp):
        for col in search_expected["stitched_columns"]:
            assert str(g[col]) == str(w[col]), col


def test_stitch_match_positions_groups_by_query_and_match_for_several_queries(ced9_records, bcl2_records):
    """Two copies of the query: one row per (query, match) — not the reference's mix of both queries' k-mers per match."""
    k, sc, mol = 16, 5, "hp"
    q_recs = [ced9_records[0], ("second copy", ced9_records[0][1])]
    q_res, q_off = oracle.pack([s for _, s in q_recs])
    t_res, t_off = oracle.pack([s for _, s in bcl2_records])
    hits, (offs, a, b, *_), _, _ = matchpos_join.reference(q_res, q_off, t_res, t_off, k, sc, mol)
    got = wire.stitch_match_positions(q_recs, bcl2_records, hits[0], hits[1], offs, a, b, k, mol)
    assert len(got) == 10
    first = {r["match_name"]: r for r in got if r["query_name"] == q_recs[0][0]}
    second = {r["match_name"]: r for r in got if r["query_name"] == "second copy"}
    assert len(first) == len(second) == 5
    for name, r in first.items():
        assert {c: v for c, v in r.items() if c not in ("query_name", "to_print")} == \
               {c: v for c, v in second[name].items() if c not in ("query_name", "to_print")}
