"""CPU-side checks of the search options (ks_search_ex and friends): the new symbols are exported with the prototypes
_lib.py declares, bad options are refused with KS_ERR_INVALID_ARG before any device work (no context needed), and the
engine's keyword defaults call the plain entry points.  No GPU compute here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from kmerseek_amd import _lib, build as ks_build, engine, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ks_search_ex", "ks_sketch_search_device_ex", "ks_sketch_search_ex", "ks_hits_has_abund_stats",
               "ks_hits_device_median2", "ks_hits_device_abund_ss", "ks_hits_copy_abund_stats_to_host"]


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
    assert C.sizeof(_lib.ks_search_opts) == 16
    assert _lib.ks_search_opts.min_containment.offset == 8
    assert _lib.KS_SEARCH_ABUND_STATS == 1
    for name in ("ksh_index_search_ex", "ksh_index_search_fasta_ex"):
        assert hasattr(lib, name) and name in host.HOST_SIGNATURES


def _opts(flags=0, reserved=0, min_c=0.0):
    return _lib.ks_search_opts(flags, reserved, min_c)


@pytest.mark.parametrize("opts", [None, _opts(), _opts(1), _opts(0, 0, -0.5), _opts(0, 0, math.nan), _opts(1, 0, -1e-300),
                                  _opts(0, 7, 0.5), _opts(4, 0, 0.5), _opts(0, 0, math.inf)])
def test_bad_or_null_arguments_are_invalid_arg_without_a_context(lib, opts):
    out = C.c_void_p()
    p = C.byref(opts) if opts is not None else None
    assert lib.ks_search_ex(None, None, None, p, C.byref(out)) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_search_ex(None, None, None, p, None) == _lib.KS_ERR_INVALID_ARG
    assert not out.value
    sk, hits = C.c_void_p(), C.c_void_p()
    assert lib.ks_sketch_search_ex(None, None, None, None, 0, p, C.byref(sk), C.byref(hits)) == _lib.KS_ERR_INVALID_ARG
    assert lib.ks_sketch_search_device_ex(None, None, None, None, 0, 0, 0, p, C.byref(sk), C.byref(hits)) == _lib.KS_ERR_INVALID_ARG
    assert not sk.value and not hits.value


def test_hits_accessors_accept_null(lib):
    assert lib.ks_hits_has_abund_stats(None) == 0
    assert not lib.ks_hits_device_median2(None) and not lib.ks_hits_device_abund_ss(None)
    assert lib.ks_hits_copy_abund_stats_to_host(None, None, None, None) == _lib.KS_ERR_INVALID_ARG


class _Recorder:
    """Stands in for the loaded library: records which entry point a Context method called, and with what options."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            opts = None
            for a in args:
                obj = getattr(a, "_obj", None)
                if isinstance(obj, _lib.ks_search_opts):
                    opts = (obj.flags, obj.reserved, obj.min_containment)
            self.calls.append((name, opts))
            return _lib.KS_OK
        return call


def _fake_context():
    ctx = engine.Context.__new__(engine.Context)
    ctx._L = _Recorder()
    ctx._h = C.c_void_p(1)
    ctx._pinned, ctx._close_pending = 0, True  # (never destroys anything)
    return ctx


def test_engine_keyword_defaults_map_to_the_old_entries(monkeypatch):
    monkeypatch.setattr(engine.Hits, "__del__", lambda self: None, raising=False)
    monkeypatch.setattr(engine.Sketches, "__del__", lambda self: None, raising=False)
    ctx = _fake_context()
    ix, q = engine.Index.__new__(engine.Index), engine.Sketches.__new__(engine.Sketches)
    ix._h = q._h = C.c_void_p(2)
    res, offs = np.zeros(4, np.uint8), np.array([0, 4], np.uint64)

    ctx.search(ix, q)
    ctx.sketch_search(ix, res, offs)
    ctx.sketch_search_device(ix, 16, 32, 1, 4)
    assert [c[0] for c in ctx._L.calls] == ["ks_search", "ks_sketch_search", "ks_sketch_search_device"]

    ctx._L.calls.clear()
    ctx.search(ix, q, abund_stats=True)
    ctx.search(ix, q, min_containment=0.25)
    ctx.sketch_search(ix, res, offs, abund_stats=True, min_containment=0.5)
    ctx.sketch_search_device(ix, 16, 32, 1, 4, min_containment=1e-300)
    assert ctx._L.calls == [("ks_search_ex", (1, 0, 0.0)), ("ks_search_ex", (0, 0, 0.25)), ("ks_sketch_search_ex", (1, 0, 0.5)),
                            ("ks_sketch_search_device_ex", (0, 0, 1e-300))]
    assert engine.search_opts() is None and engine.search_opts(0.0, False) is None
