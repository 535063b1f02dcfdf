"""CPU: the table of tests/pool_fill_cases.py (what tests/test_gpu_poisoned_pool.py runs under KS_DEBUG_POOL_FILL) against the
functions it names, and its exemption list against the header and the sources.  No device."""
import glob
import os
import re

import pytest

import pool_fill_cases as PF

ROOT = PF.ROOT
TABLE = PF.expand()


def test_every_module_and_function_of_the_table_exists():
    assert len(TABLE) >= 100
    for module, function, psets in PF.CASES:
        fn = getattr(PF.load(module), function, None)
        assert callable(fn) and function.startswith("test_"), f"{module}.{function}"
        assert psets, f"{module}.{function}: no parameter set"


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_parameter_set_matches_the_signature(case):
    """Every value is one of the function's own parametrisation (nothing the suite does not run on a fresh pool), every mark has a
    value, and every other argument has a known source."""
    _, module, function, pset = case
    mod = PF.load(module)
    src = PF.sources(mod, getattr(mod, function), pset)
    assert "unknown" not in src.values(), src


def test_fill_values_and_ids():
    assert PF.FILLS == (0, 255)
    assert len({c[0] for c in TABLE}) == len(TABLE)


def test_no_prototype_is_unaccounted_for():
    """Header = exemption list + what the table has to reach: the list names no prototype that is gone, gives each a one-line reason,
    and what is left is what the last test of the GPU file asks the recorded calls for."""
    names, exempt = PF.declared(), PF.exempt()
    assert len(names) >= 400
    assert not sorted(set(exempt) - set(names)), "exempted, but not in the header"
    for n, why in exempt.items():
        assert why and "\n" not in why, n
    required = sorted(set(names) - set(exempt))
    assert 60 <= len(required) <= len(names) - 300, required
    assert "ks_sketches_copy_to_host" in required  # (it makes a gapped set dense: a kernel into new pool blocks)


def _extern_c_bodies():
    """{function: body} of every extern "C" definition under kmerseek_amd/csrc."""
    out = {}
    for path in glob.glob(os.path.join(ROOT, "kmerseek_amd", "csrc", "*")):
        s = open(path).read()
        for m in re.finditer(r'extern "C"[^;{}()]*?\b(ks_[a-z0-9_]+)\s*\(', s):
            i = s.find("{", m.end())
            if i < 0 or ";" in s[m.end():i]:
                continue  # a declaration
            depth, j = 0, i
            while True:
                depth += {"{": 1, "}": -1}.get(s[j], 0)
                if depth == 0:
                    break
                j += 1
            out[m.group(1)] = s[i:j + 1]
    return out


def test_no_exempted_entry_point_launches_a_kernel():
    bodies, exempt = _extern_c_bodies(), PF.exempt()
    assert len(bodies) >= 400 and set(PF.declared()) <= set(bodies)
    launching = sorted(n for n in exempt if "KS_LAUNCH" in bodies[n])
    assert not launching, launching
    # ... nor takes a block from the pool: the two micro-benchmarks are the exception the list names
    pooled = sorted(n for n in exempt if re.search(r"\bks_alloc\b|\bks_pool_alloc\b|\.alloc\(|\bks_obj_alloc\b", bodies[n]))
    assert pooled == ["ks_bench_device_rates", "ks_bench_gather_rates"], pooled
