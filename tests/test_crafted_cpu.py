"""CPU: the hand-made sketch families of tests/crafted_sketches.py are what they claim to be, and the references the GPU file
holds the library against agree with the oracle.

- every family is deterministic, valid for ks_sketches_from_host and passes its own property assertions (they run when the
  case is built);
- the numpy join equals oracle.manysearch on every family (wide_records: on its non-empty queries, renumbered — the oracle
  is pairwise);
- the union reference equals a dict-based accumulation;
- replica() agrees with oracle.manysearch_row's mean, median and std to rel 1e-12 on the wide_records rows."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as cs  # noqa: E402
from oracle import oracle  # noqa: E402


def _eq_case(a, b):
    return a[:4] == b[:4] and all(np.array_equal(x, y) and x.dtype == y.dtype for S, R in zip(a[4:], b[4:]) for x, y in zip(S, R))


@pytest.mark.parametrize("name", cs.NAMES)
def test_family_is_deterministic_and_valid(name):
    a, b = cs.family(name), cs.family(name, fresh=True)  # (building runs the property assertions and check_valid)
    assert a[0] == name and _eq_case(a, b)
    _, ksize, scaled, moltype, T, Q = a
    assert cs.max_hash(scaled) == oracle.max_hash(scaled)
    cs.check_valid(T, scaled); cs.check_valid(Q, scaled)
    assert cs.ref_pairs(T, Q) < cs.PAIR_BOUND


def test_the_checks_refuse_what_the_library_refuses():
    offs = np.array([0, 2], np.uint64)
    ab = np.ones(2, np.uint32)
    for mins, scaled in (([0, 5], 1), ([5, 5], 1), ([7, 5], 1), ([1, cs.max_hash(5) + 1], 5)):
        with pytest.raises(AssertionError):
            cs.check_valid((offs, np.array(mins, np.uint64), ab), scaled)
    cs.check_valid((np.array([0, 1, 2], np.uint64), np.array([7, 5], np.uint64), ab), 1)  # (descending across sequences is fine)
    cs.check_valid((offs, np.array([1, cs.max_hash(5)], np.uint64), ab), 5)


def test_bit_counts_and_prefix_formula():
    assert [cs.bits_for(n) for n in (0, 1, 2, 3, 4096, 4097, 1 << 20, (1 << 20) + 1)] == [1, 1, 1, 2, 12, 13, 20, 21]
    assert [cs.bits_for_value(v) for v in (0, 1, 2, 255, 256, cs.U32_MAX)] == [1, 1, 2, 8, 9, 32]
    for pbits in cs.PBITS_EDGES:  # scaled = 1: the prefix is the top pbits bits of the hash
        K = cs.prefix_mul(pbits, cs.U64_MAX)
        for h in (1, 1 << 63, cs.U64_MAX, 0x123456789ABCDEF0):
            assert cs.join_prefix(h, K) == h >> (64 - pbits)
    assert cs.max_hash(cs.U32_MAX) == (1 << 32) + 1


def _nonempty(Q):
    """the non-empty sequences of a batch as a batch of their own, and their ids"""
    offs, mins, ab = Q
    ids = np.nonzero(np.diff(offs))[0]
    o = np.zeros(len(ids) + 1, np.uint64)
    o[1:] = np.cumsum((offs[ids + 1] - offs[ids]))
    return (o, mins, ab), ids


@pytest.mark.parametrize("name", cs.NAMES)
def test_numpy_join_equals_the_oracle(name):
    _, ksize, scaled, moltype, T, Q = cs.family(name)
    got = cs.ref_join(T, Q)
    assert len(got[0]) > 0 and int(got[2].sum()) == cs.ref_pairs(T, Q)
    ids = None
    if name == "wide_records":
        Q, ids = _nonempty(Q)
    want = list(oracle.manysearch(Q[0], Q[1], T[0], T[1], T[2], n_threads=8))
    if ids is not None:
        want[0] = ids[want[0].astype(np.int64)].astype(np.uint32)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, j)


@pytest.mark.parametrize("name", cs.NAMES)
def test_union_reference_equals_a_dict(name):
    T = cs.family(name)[4]
    sums = {}
    for h, a in zip(T[1].tolist(), T[2].tolist()):
        sums[h] = sums.get(h, 0) + a
    offs, hashes, ab = cs.ref_union(T)
    assert offs.tolist() == [0, len(sums)] and hashes.tolist() == sorted(sums)
    assert ab.tolist() == [min(sums[h], cs.U32_MAX) for h in sorted(sums)]
    if name == "union_saturation":
        assert sum(v > cs.U32_MAX for v in sums.values()) >= 2 and cs.U32_MAX in sums.values() and cs.U32_MAX - 1 in sums.values()
        assert int(np.count_nonzero(ab == cs.U32_MAX)) >= 4  # 2^32 - 1 itself (twice), 2^32, far above


def test_replica_agrees_with_the_oracle_row_on_wide_records():
    _, ksize, scaled, moltype, T, Q = cs.family("wide_records")
    rows = cs.ref_join(T, Q)
    which = cs.wide_stat_rows(rows)
    assert which[0] == 0 and which[-1] == len(rows[0]) - 1
    m2, ss = cs.ref_stats(rows, T, Q, which)
    assert np.any(m2 >= np.uint64(1 << 32)) and np.any(rows[3][which] >= np.uint64(1 << 32))
    to, tm, ta = T
    qo, qm, _ = Q
    for j, r in enumerate(which):
        q, t, n = int(rows[0][r]), int(rows[1][r]), int(rows[2][r])
        w = oracle.manysearch_row("q", qm[int(qo[q]):int(qo[q + 1])], "t", tm[int(to[t]):int(to[t + 1])], ta[int(to[t]):int(to[t + 1])],
                                  ksize, scaled, moltype)
        assert w["intersect_hashes"] == n and w["n_weighted_found"] == int(rows[3][r])
        assert math.isclose(float(m2[j]) / 2.0, w["median_abund"], rel_tol=1e-12), r
        assert math.isclose(math.sqrt(ss[j] / n), w["std_abund"], rel_tol=1e-12, abs_tol=1e-300), r
        assert math.isclose(float(int(rows[3][r])) / n, w["average_abund"], rel_tol=1e-12), r


def test_thresholds_cut_somewhere():
    """the keep test is not all or nothing on these families: some threshold of the GPU file keeps some rows and drops others"""
    cut = []
    for name in cs.NAMES:
        _, _, _, _, T, Q = cs.family(name)
        rows = cs.ref_join(T, Q)
        cut.append(any(0 < cs.keep(rows, Q, thr).sum() < len(rows[0]) for thr in (0.0, 1e-300, 0.05, 0.5, 1.0, 1.5)))
    assert sum(cut) >= 8 and cut[cs.NAMES.index("wide_records")]


def test_keep_mask_is_the_f64_containment_test():
    _, _, _, _, T, Q = cs.family("one_bucket")
    rows = cs.ref_join(T, Q)
    sizes = np.diff(Q[0]).astype(np.int64)
    for thr in (0.0, 1e-300, 0.05, 0.5, 1.0, 1.5):
        want = [float(int(i)) / float(int(sizes[int(q)])) >= thr for q, i in zip(rows[0], rows[2])]
        assert cs.keep(rows, Q, thr).tolist() == want
