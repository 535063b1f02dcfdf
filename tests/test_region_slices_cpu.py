"""The slice cutter of ks_regions_traceback and ks_regions_stitch (rp_cut_slices, the host half of ks_rpath_kit.h) as a
stand-alone program under AddressSanitizer + UBSan (tests/hostsan/san_slices.cpp), against a restatement in Python, against
cuts written down by hand, and against what a cut is: slices that cover the items in order, each within the budget, none
that could have taken the next item.  No GPU, nothing sanitized loaded into this interpreter.
"""
import importlib.util
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module")
def san_slices(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("hostsan_build", os.path.join(HERE, "hostsan", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_alone(str(tmp_path_factory.mktemp("hostsan_slices")), "san_slices")


def cut_ref(off, budget):
    n, cut, first, largest, i0 = len(off) - 1, [0], [0], 0, 0
    while i0 < n:
        i1 = i0
        while i1 < n and off[i1 + 1] - off[i0] <= budget:
            i1 += 1
        if i1 == i0:
            return dict(bad=i0, bad_rows=off[i0 + 1] - off[i0], max_rows=largest, cut=cut, first_row=first)
        largest = max(largest, off[i1] - off[i0])
        cut.append(i1)
        if i1 < n:
            first.append(off[i1])
        i0 = i1
    return dict(bad=-1, bad_rows=0, max_rows=largest, cut=cut, first_row=first)


def run(exe, rows, budget):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    env = dict(os.environ)
    env.update(SAN_ENV)
    p = subprocess.run([exe, str(budget)] + [str(o) for o in off], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=60)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, f"exit {p.returncode}\n{p.stdout}\n{p.stderr[-4000:]}"
    got = dict(kv.split("=") for kv in p.stdout.split())
    got = {k: [int(x) for x in v.split(",")] if k in ("cut", "first_row") else int(v) for k, v in got.items()}
    return off, got


# rows per item, budget, and the cut by hand: (bad, slices as [first item, end item) pairs, the largest slice)
CASES = {
    "everything fits": ([3, 1, 4], 100, -1, [(0, 3)], 8),
    "everything fits exactly": ([3, 1, 4], 8, -1, [(0, 3)], 8),
    "exact fit at a cut": ([2, 3, 5, 1], 5, -1, [(0, 2), (2, 3), (3, 4)], 5),
    "one row short of the cut": ([2, 3, 5, 1], 6, -1, [(0, 2), (2, 4)], 6),
    "no rows at the start, between cuts and at the end": ([0, 0, 4, 0, 4, 0, 0], 4, -1, [(0, 4), (4, 7)], 4),
    "no rows between two full slices": ([4, 0, 0, 3, 2, 0], 4, -1, [(0, 3), (3, 4), (4, 6)], 4),
    "only items without rows": ([0, 0, 0], 7, -1, [(0, 3)], 0),
    "eight items, one each": ([5] * 8, 5, -1, [(i, i + 1) for i in range(8)], 5),
    "no items": ([], 5, -1, [], 0),
    "over budget first": ([9, 1], 5, 0, [], 0),
    "over budget in the middle": ([1, 2, 9, 1], 5, 2, [(0, 2)], 3),
    "over budget last, behind items without rows": ([5, 0, 0, 6], 5, 3, [(0, 3)], 5),
    "budget 0": ([1, 0], 0, 0, [], 0),
    "budget 0, items without rows first": ([0, 0, 1, 0], 0, 2, [(0, 2)], 0),
    "budget 0, nothing needs a row": ([0, 0], 0, -1, [(0, 2)], 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_slice_cutter(san_slices, name):
    rows, budget, bad, slices, largest = CASES[name]
    assert len(rows) <= 8
    off, got = run(san_slices, rows, budget)
    assert got == cut_ref(off, budget)
    # by hand
    assert got["bad"] == bad and got["max_rows"] == largest
    assert got["cut"] == [0] + [e for _, e in slices]
    assert got["bad_rows"] == (rows[bad] if bad >= 0 else 0)
    # what a cut is
    cut = got["cut"]
    done = cut[-1]
    assert done == (bad if bad >= 0 else len(rows))
    assert got["first_row"][0] == 0
    for i in range(len(cut) - 1):  # a launch per slice reads first_row[i], cut[i] and cut[i + 1]
        assert got["first_row"][i] == off[cut[i]]
    for a, b in zip(cut, cut[1:]):
        assert a < b and off[b] - off[a] <= budget
        assert b == len(rows) or off[b + 1] - off[a] > budget  # greedy: the next item did not fit
    if bad >= 0:
        assert rows[bad] > budget
