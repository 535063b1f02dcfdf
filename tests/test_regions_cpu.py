"""CPU-side checks of ks_match_regions (each hit's pairs chained by diagonal): the numpy reference of tests/regions_ref.py on the
golden case ced9 vs BCL2-25 — seven regions where the reference's stitcher reports five, two of them wrong —, the host half
(wire.region_rows) against the golden stitched rows where a match IS one colinear run, the min_kmers filter, and the ctypes
layer.  No GPU compute here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchpos_join  # noqa: E402
import regions_ref  # noqa: E402

from kmerseek_amd import _lib, build as ks_build, engine, wire  # noqa: E402
from oracle import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ks_match_regions", "ks_regions_n_rows", "ks_regions_n_regions", "ks_regions_n_slices", "ks_regions_device_row_offsets",
               "ks_regions_device_q_start", "ks_regions_device_t_start", "ks_regions_device_length", "ks_regions_device_n_kmers",
               "ks_regions_device_covered", "ks_regions_copy_to_host", "ks_regions_free"]

# (q_start, t_start, length, n_kmers, covered) per match of ced9 vs BCL2-25, hp k=16 scaled=5
GOLDEN_REGIONS = {"BNIP2_HUMAN": [(76, 23, 16, 1, 16), (197, 255, 16, 1, 16)],
                  "ASPP2_HUMAN": [(241, 1084, 16, 1, 16)],
                  "BAK_HUMAN": [(245, 42, 16, 1, 16)],
                  "BBC3_HUMAN": [(170, 46, 17, 2, 17)],
                  "FBX10_HUMAN": [(59, 57, 17, 2, 17), (264, 555, 16, 1, 16)]}


def _short(name):
    return next(s for s in GOLDEN_REGIONS if s in name)


@pytest.fixture(scope="module")
def golden_join(ced9_records, bcl2_records):
    k, sc, mol = 16, 5, "hp"
    q_res, q_off = oracle.pack([s for _, s in ced9_records])
    t_res, t_off = oracle.pack([s for _, s in bcl2_records])
    hits, (offs, a, b, *_), _, _ = matchpos_join.reference(q_res, q_off, t_res, t_off, k, sc, mol)
    return hits, offs, a, b


def test_reference_gives_the_seven_golden_regions(golden_join, bcl2_records):
    hits, offs, a, b = golden_join
    got = regions_ref.chain(offs, a, b, 16)
    assert len(hits[0]) == 5 and int(got[0][-1]) == 7 and all(len(c) == 7 and c.dtype == np.uint32 for c in got[1:])
    per_match = {_short(bcl2_records[t][0]): regions_ref.as_tuples(got, r) for r, t in enumerate(hits[1].tolist())}
    assert per_match == GOLDEN_REGIONS
    assert np.array_equal(got[3], got[5])  # max_gap = 0: covered is the length
    # a gap wide enough joins nothing here (the extra k-mers lie on other diagonals), and changes no column
    for g, w in zip(regions_ref.chain(offs, a, b, 16, max_gap=1000), got):
        assert np.array_equal(g, w)


def test_reference_on_a_hand_made_row():
    """One row, k = 4: diagonal 0 holds starts 0, 2, 6, 11 — steps 2 (overlap), 4 (abut), 5 (a gap of one) — diagonal -3 holds 7."""
    offs = np.array([0, 5], np.uint64)
    a = np.array([0, 2, 6, 7, 11], np.uint32)
    b = np.array([0, 2, 6, 4, 11], np.uint32)
    assert regions_ref.as_tuples(regions_ref.chain(offs, a, b, 4), 0) == [(0, 0, 10, 3, 10), (7, 4, 4, 1, 4), (11, 11, 4, 1, 4)]
    assert regions_ref.as_tuples(regions_ref.chain(offs, a, b, 4, max_gap=1), 0) == [(0, 0, 15, 4, 14), (7, 4, 4, 1, 4)]
    assert regions_ref.as_tuples(regions_ref.chain(offs, a, b, 4, max_gap=1, min_kmers=2), 0) == [(0, 0, 15, 4, 14)]
    assert regions_ref.as_tuples(regions_ref.chain(offs, a, b, 4, max_gap=2 ** 32 - 1), 0) == [(0, 0, 15, 4, 14), (7, 4, 4, 1, 4)]


def test_region_rows_equal_the_golden_stitched_rows_where_a_match_is_one_run(golden_join, search_expected, ced9_records, bcl2_records):
    hits, offs, a, b = golden_join
    rows = wire.region_rows(ced9_records, bcl2_records, hits[0], hits[1], regions_ref.chain(offs, a, b, 16), "hp")
    assert len(rows) == 7
    assert [(r["query_start"], r["query_end"]) for r in rows] == sorted((r["query_start"], r["query_end"]) for r in rows)
    exp = {r["match_name"]: r for r in search_expected["stitched_rows"]}
    single = [r for r in rows if len(GOLDEN_REGIONS[_short(r["match_name"])]) == 1]
    assert sorted(_short(r["match_name"]) for r in single) == ["ASPP2_HUMAN", "BAK_HUMAN", "BBC3_HUMAN"]
    for g in single:
        for col in search_expected["stitched_columns"]:
            assert str(g[col]) == str(exp[g["match_name"]][col]), col
    for r in rows:
        want = GOLDEN_REGIONS[_short(r["match_name"])]
        assert (r["query_start"], r["match_start"], r["length"], r["n_kmers"], r["covered"]) in want
        assert len(r["query"]) == len(r["match"]) == len(r["encoded"]) == r["length"] == r["query_end"] - r["query_start"]
        assert r["encoded"] == wire.encode_kmer(r["match"], "hp")  # the two sides agree in the alphabet the hash was taken in


def test_min_kmers_two_leaves_two_regions_and_three_empty_rows(golden_join):
    hits, offs, a, b = golden_join
    got = regions_ref.chain(offs, a, b, 16, min_kmers=2)
    per_row = (got[0][1:] - got[0][:-1]).tolist()
    assert int(got[0][-1]) == 2 and sorted(per_row) == [0, 0, 0, 1, 1]
    assert sorted(zip(*[c.tolist() for c in got[1:]])) == [(59, 57, 17, 2, 17), (170, 46, 17, 2, 17)]
    assert all(np.array_equal(g, w) for g, w in zip(regions_ref.chain(offs, a, b, 16, min_kmers=0), regions_ref.chain(offs, a, b, 16)))


# ---- the ctypes layer ----------------------------------------------------------------------------------------------------------
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
    assert C.sizeof(_lib.ks_regions_opts) == 16
    assert [(f, getattr(_lib.ks_regions_opts, f).offset) for f, _ in _lib.ks_regions_opts._fields_] == \
           [("flags", 0), ("min_kmers", 4), ("max_gap", 8), ("reserved", 12)]
    assert lib.ks_abi_version() == 1


@pytest.mark.parametrize("opts", [None, (0, 0, 0, 0), (0, 3, 16, 0), (1, 0, 0, 0), (0, 0, 0, 7), (0x80000000, 2, 2, 1)])
def test_bad_or_null_arguments_are_invalid_arg_without_a_context(lib, opts):
    out = C.c_void_p()
    p = C.byref(_lib.ks_regions_opts(*opts)) if opts is not None else None
    assert lib.ks_match_regions(None, None, p, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_match_regions(None, None, p, None) == _lib.KS_ERR_INVALID_ARG
    assert not out.value


def test_accessors_accept_null(lib):
    assert lib.ks_regions_n_rows(None) == 0 and lib.ks_regions_n_regions(None) == 0 and lib.ks_regions_n_slices(None) == 0
    for col in engine.Regions._COLUMNS:
        assert not getattr(lib, "ks_regions_device_" + col)(None)
    assert lib.ks_regions_copy_to_host(None, None, None, None, None, None, None, None) == _lib.KS_ERR_INVALID_ARG
    lib.ks_regions_free(None)


class _Recorder:
    """Stands in for the loaded library: records which entry point a Context method called, and with what options."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            opts = None
            for a in args:
                obj = getattr(a, "_obj", None)
                if isinstance(obj, _lib.ks_regions_opts):
                    opts = (obj.flags, obj.min_kmers, obj.max_gap, obj.reserved)
            self.calls.append((name, opts, len(args)))
            return _lib.KS_OK
        return call


def test_engine_passes_its_options_on(monkeypatch):
    for cls in (engine.MatchPositions, engine.Regions):
        monkeypatch.setattr(cls, "__del__", lambda self: None, raising=False)
    ctx = engine.Context.__new__(engine.Context)
    ctx._L = _Recorder()
    ctx._h = C.c_void_p(1)
    ctx._pinned, ctx._close_pending = 0, True  # (never destroys anything)
    mp = engine.MatchPositions.__new__(engine.MatchPositions)
    mp._h = C.c_void_p(2)
    assert isinstance(ctx.match_regions(mp), engine.Regions)
    ctx.match_regions(mp, max_gap=2 ** 32 - 1, min_kmers=3)
    assert ctx._L.calls == [("ks_match_regions", (0, 1, 0, 0), 4), ("ks_match_regions", (0, 3, 2 ** 32 - 1, 0), 4)]
    for bad in ({"max_gap": -1}, {"max_gap": 2 ** 32}, {"min_kmers": -1}, {"min_kmers": 2 ** 32}):
        with pytest.raises(ValueError):
            ctx.match_regions(mp, **bad)
