"""No GPU: the region cull's yardstick (tests/rcull_ref.py) against the hand-written expectations of tests/rcull_cases.py, the
contract's invariants on a seeded fuzz, wire.region_rows(cull=...) on host arrays, and the premise of the GPU test of the
deletion pair: its two fragment alignments coincide (tests/ralign_ref.py), so a cull must keep one of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rcull_cases as RC  # noqa: E402
import rcull_ref  # noqa: E402

from kmerseek_amd import wire  # noqa: E402


@pytest.mark.parametrize("c", RC.CASES, ids=[c["name"] for c in RC.CASES])
def test_reference_gives_the_hand_written_expectations(c):
    o = c["opts"]
    got = rcull_ref.cull(*RC.columns(c), P=o["P"], N=o["N"], min_score=o["min_score"])
    RC.assert_same(got, RC.expected(c), c["name"])


def test_overlap_pct_0_means_100():
    c = next(c for c in RC.CASES if c["name"] == "boundary_p100")
    RC.assert_same(rcull_ref.cull(*RC.columns(c), P=0), RC.expected(c))


@pytest.mark.parametrize("P,N,min_score", [(100, 0, None), (50, 0, None), (1, 0, 3), (80, 2, None), (100, 1, 10)])
def test_invariants_on_a_fuzz(P, N, min_score):
    cols = rcull_ref.fuzz_rows(7, 300, 24)
    offs, qs, ql, ts, tl, sc = [c.tolist() for c in cols]
    n = len(qs)
    o_offs, src, rank, nm, keeper, best = [a.tolist() for a in rcull_ref.cull(*cols, P=P, N=N, min_score=min_score)]
    ext = lambda g: (qs[g], ql[g], ts[g], tl[g])
    before = lambda g, h: sc[g] > sc[h] or (sc[g] == sc[h] and g < h)
    kept = set(src)
    n_removed = 0
    assert sum(nm) + sum(1 for k in keeper if k == rcull_ref.NONE) == n  # every region is counted once
    for r in range(len(offs) - 1):
        row = range(offs[r], offs[r + 1])
        mine = src[o_offs[r]:o_offs[r + 1]]
        assert mine == sorted(mine) and all(g in row for g in mine)  # input order survives
        assert sorted(rank[o_offs[r]:o_offs[r + 1]]) == list(range(len(mine)))
        by_rank = sorted(mine, key=lambda g: rank[src.index(g)])
        assert all(before(a, b) for a, b in zip(by_rank, by_rank[1:]))  # rank is priority order among the kept
        assert (best[r] == sc[by_rank[0]]) if mine else np.isnan(best[r])
        assert not N or len(mine) <= N
        for g in row:
            k = keeper[g]
            if g in kept:
                assert k == g
                # no kept region is covered by a kept region of higher priority
                assert not any(before(h, g) and rcull_ref.covers(P, ext(h), ext(g)) for h in mine if h != g)
            elif k != rcull_ref.NONE:
                n_removed += 1
                assert k in mine and before(k, g) and rcull_ref.covers(P, ext(k), ext(g))  # every removed region is covered by its keeper
                assert not any(before(h, k) and rcull_ref.covers(P, ext(h), ext(g)) for h in mine)  # ... the first that does
            else:
                assert (min_score is not None and sc[g] < min_score) or (N and len(mine) == N)
        for i, g in enumerate(mine):
            assert nm[o_offs[r] + i] == sum(1 for h in row if keeper[h] == g)
    if N == 0 and min_score is None:
        assert n_removed > n // 10  # coverage is frequent in this fuzz (a limit or a threshold drops most regions instead)
    # culling the kept again changes nothing
    again = rcull_ref.cull(np.array(o_offs, np.uint64), *[np.asarray(c)[src] for c in cols[1:]], P=P)
    assert again[0].tolist() == o_offs and again[1].tolist() == list(range(len(src))) and set(again[3].tolist()) <= {1}
    assert again[4].tolist() == list(range(len(src)))


# ---- wire.region_rows(cull=...) ------------------------------------------------------------------------------------------------
Q_RECS = [("q0", b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY"), ("q1", b"MKTAYIAKQRQISFVKSHFSRQ")]
T_RECS = [("t0", b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY"), ("t1", b"MKTAYIAKQRQISFVKSHFSRQ")]
QID, TID = [0, 1], [0, 1]
REGIONS = (np.array([0, 3, 4], np.uint64), np.array([0, 2, 20, 1], np.uint32), np.array([0, 2, 20, 1], np.uint32),
           np.array([10, 5, 12, 8], np.uint32), np.array([4, 1, 6, 2], np.uint32), np.array([10, 5, 12, 8], np.uint32))
SCORES = (REGIONS[0], REGIONS[1], REGIONS[2], REGIONS[3], np.array([10, 5, 12, 8], np.int64), REGIONS[3], REGIONS[3], REGIONS[3])
ALIGNS = (REGIONS[0], np.array([0, 0, 20, 0], np.uint32), np.array([12, 12, 14, 22], np.uint32), np.array([0, 0, 20, 0], np.uint32),
          np.array([12, 12, 14, 22], np.uint32), np.array([12, 12, 14, 22], np.int64), np.array([12, 12, 14, 22], np.uint32),
          np.array([12, 12, 14, 22], np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.array([12, 12, 14, 22], np.uint32))
CIGARS = (np.array([0, 1, 2, 3, 4], np.uint64), np.array([12 << 4, 12 << 4, 14 << 4, 22 << 4], np.uint32))


def test_region_rows_with_a_cull():
    base = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, cigars=CIGARS)
    assert len(base) == 4
    cull = rcull_ref.cull(*ALIGNS[:6])  # the two coinciding alignments of row 0: region 1 names region 0
    assert cull[1].tolist() == [0, 2, 3] and cull[3].tolist() == [2, 1, 1] and cull[2].tolist() == [1, 0, 0]
    rows = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, cigars=CIGARS, cull=cull)
    assert len(rows) == 3
    strip = lambda r: {k: v for k, v in r.items() if k not in ("aln_rank", "aln_n_merged")}
    assert [strip(r) for r in rows] == [b for b in base if not (b["query_name"] == "q0" and b["seed_start"] == 2)]
    assert [(r["aln_rank"], r["aln_n_merged"]) for r in rows] == [(1, 2), (0, 1), (0, 1)]
    assert list(rows[0])[-2:] == ["aln_rank", "aln_n_merged"]
    # the cigars of the kept alignments alone (traced from the taken objects) give the same rows
    kept_cigars = (np.array([0, 1, 2, 3], np.uint64), CIGARS[1][[0, 2, 3]])
    assert wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, cigars=kept_cigars, cull=cull) == rows
    # a cull of the scores: the other pair of columns
    s_cull = rcull_ref.cull(SCORES[0], SCORES[1], SCORES[3], SCORES[2], None, SCORES[4])
    s_rows = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, cull=s_cull)
    s_base = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES)
    assert [r["seed_start"] for r in s_rows] == [0, 20, 1]  # (2, 5) lies inside (0, 10) on both sequences
    assert all("region_rank" in r and "region_n_merged" in r and "aln_rank" not in r for r in s_rows)
    assert [{k: v for k, v in r.items() if not k.startswith("region_")} for r in s_rows] == [b for b in s_base if b["seed_start"] != 2]
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", cull=cull)  # a cull of nothing
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, cull=tuple(c[:-1] for c in cull))


def test_region_rows_without_a_cull_is_unchanged():
    """cull=None: byte for byte the rows of a call without the argument, in every combination of the other inputs."""
    for kw in ({}, {"scores": SCORES}, {"scores": SCORES, "alignments": ALIGNS}, {"alignments": ALIGNS, "cigars": CIGARS}):
        a = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", **kw)
        b = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", cull=None, **kw)
        assert repr(a) == repr(b) and len(a) == 4
        assert not any(k.endswith(("_rank", "_n_merged")) for r in a for k in r)


# ---- the premise of the deletion pair ------------------------------------------------------------------------------------------
def test_deletion_pair_fragments_coincide():
    q, t, seeds = RC.deletion_pair()
    assert t == q[:60] + q[63:] and len(seeds) == 2
    # the shared 7-mers lie on exactly the two seeds' diagonals
    shared = {(a, b) for a in range(len(q) - 6) for b in range(len(t) - 6) if q[a:a + 7] == t[b:b + 7]}
    assert shared == {(a, a) for a in range(0, 54)} | {(a, a - 3) for a in range(63, 114)}
    regions = (np.array([0, 2], np.uint64), np.array([s[0] for s in seeds], np.uint32), np.array([s[1] for s in seeds], np.uint32),
               np.array([s[2] for s in seeds], np.uint32))
    q_res, q_off = np.frombuffer(q, np.uint8), np.array([0, len(q)], np.uint64)
    t_res, t_off = np.frombuffer(t, np.uint8), np.array([0, len(t)], np.uint64)
    al = ralign_ref.align(regions, [0], [0], q_res, q_off, t_res, t_off)  # the defaults
    for col in al[1:]:
        assert col[0] == col[1]  # one alignment, reported twice
    assert (al[1][0], al[2][0], al[3][0], al[4][0]) == (0, 120, 0, 117) and al[9][0] == 3 and al[8][0] == 1
    cull = rcull_ref.cull(*al[:6])
    assert cull[1].tolist() == [0] and cull[3].tolist() == [2] and cull[4].tolist() == [0, 0]
