"""CPU-side checks of the column tables of kmerseek_amd/engine.py (every subclass of engine._Columns) against the C ABI as
include/kmerseek_amd.h declares it: the parameters of ks_<prefix>_copy_to_host are the table's columns, in order and of the
table's element types; every column has its ks_<prefix>_device_<column> accessor of that type; accessors, copy_to_host and free
take NULL.  The classes are found by walking the subclasses, so a new result object is covered when it is written.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kmerseek_amd import _lib, build as ks_build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"u1": "uint8_t", "u4": "uint32_t", "u8": "uint64_t", "i8": "int64_t", "f8": "double"}


def _subclasses(cls):
    for sub in cls.__subclasses__():
        yield sub
        yield from _subclasses(sub)


CLASSES = sorted(_subclasses(engine._Columns), key=lambda c: c.__name__)


@pytest.fixture(scope="module")
def lib():
    ks_build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)


def _prototype(text, name):
    """(return type, [(type, name) per parameter]) of `name` in the header; a pointer's type ends in '*'."""
    m = re.search(r"([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    params = []
    for p in m.group(2).split(","):
        words = p.replace("*", " * ").split()
        params.append(("".join(w for w in words[:-1] if w != "const"), words[-1]))
    return "".join(w for w in m.group(1).replace("*", " * ").split() if w != "const"), params


def test_there_are_column_classes():
    print(f"{len(CLASSES)} column classes: {', '.join(c.__name__ for c in CLASSES)}")
    assert len(CLASSES) >= 10
    prefixes = [c._PREFIX for c in CLASSES]
    assert len(set(prefixes)) == len(prefixes) and all(prefixes)
    for want in ("matchpos", "regions", "rscores", "raligns", "cigars", "rcull", "rchain", "hitalns", "rcomp", "astats"):
        assert want in prefixes, want


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_table_is_the_copy_to_host_of_the_header(cls, header):
    ret, params = _prototype(header, f"ks_{cls._PREFIX}_copy_to_host")
    assert ret == "int" and params[0] == ("ks_ctx*", "ctx") and params[1][0] == f"ks_{cls._PREFIX}*"
    assert [n for _, n in params[2:]] == [name for name, _, _ in cls._TABLE] == list(cls._COLUMNS)
    assert [t for t, _ in params[2:]] == [C_TYPES[dt] + "*" for _, dt, _ in cls._TABLE]
    for name, dt, _ in cls._TABLE:
        ret, acc = _prototype(header, f"ks_{cls._PREFIX}_device_{name}")
        assert ret == C_TYPES[dt] + "*" and [t for t, _ in acc] == [f"ks_{cls._PREFIX}*"], name
    for count in cls._COUNTS:
        ret, acc = _prototype(header, f"ks_{cls._PREFIX}_{count}")
        assert ret in ("uint32_t", "uint64_t") and len(acc) == 1, count


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_counts_and_shapes_evaluate(cls):
    """Every count expression is one over the declared counts, and the listing in help() names every column with its type."""
    counts = {c: 3 for c in cls._COUNTS}
    for name, dt, n in cls._TABLE:
        shape = eval(n, {"__builtins__": {}}, counts)
        assert np.zeros(shape, dt).size >= 3 and np.dtype(dt).itemsize == C.sizeof(getattr(C, "c_" + C_TYPES[dt].replace("_t", "")))
        for doc in (cls.device_ptrs.__doc__, cls.to_host.__doc__):
            assert f"{name} {engine._DTYPE_NAMES[dt]}[{n}]" in doc
    assert all(isinstance(getattr(cls, c), property) for c in cls._COUNTS)


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_null_objects(cls, lib):
    for name in cls._COLUMNS:
        assert not getattr(lib, f"ks_{cls._PREFIX}_device_{name}")(None), name
    for count in cls._COUNTS:
        assert getattr(lib, f"ks_{cls._PREFIX}_{count}")(None) == 0, count
    assert getattr(lib, f"ks_{cls._PREFIX}_copy_to_host")(None, None, *[None] * len(cls._TABLE)) == _lib.KS_ERR_INVALID_ARG
    getattr(lib, cls._free)(None)
