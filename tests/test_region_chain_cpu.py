"""No GPU: the region chain's yardstick (tests/rchain_ref.py) against the hand-written expectations of tests/rchain_cases.py and
against exhaustive enumeration of every ordered subset of small rows, the contract's invariants on a seeded fuzz, the condition
the GPU test's long rows rest on (their chains are long), wire.hit_chain_rows and wire.region_rows(chain=...) on host arrays, and
the premise of the GPU test of the insertion pair: two alignments that end and begin at the insertion (tests/ralign_ref.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rchain_cases as RH  # noqa: E402
import rchain_ref  # noqa: E402
import rcull_ref  # noqa: E402

from kmerseek_amd import wire  # noqa: E402
from kmerseek_amd.wire import format_f64  # noqa: E402


@pytest.mark.parametrize("c", RH.CASES, ids=[c["name"] for c in RH.CASES])
def test_reference_gives_the_hand_written_expectations(c):
    RH.assert_same(rchain_ref.chain(*RH.columns(c), **c["opts"]), RH.expected(c), c["name"])


GRID = [dict(max_gap=g, max_overlap=o, link_cost=l, skew_cost=s, overlap_cost=c)
        for g in (0, 15) for o in (0, 3) for l in (0, 7) for s in (0, 1) for c in (0, 2)]


def _rows(cols):
    offs = cols[0].tolist()
    for r in range(len(offs) - 1):
        b, e = offs[r], offs[r + 1]
        yield r, b, [tuple(int(cols[c][g]) for c in (1, 2, 3, 4)) for g in range(b, e)], [int(cols[5][g]) for g in range(b, e)]


def test_reference_against_exhaustive_enumeration():
    """300 random rows of up to 6 regions under 32 option sets: the recurrence finds the value of the best of ALL ordered
    subsets in which every region follows the one before it."""
    cols = rchain_ref.chain_rows(5, 300, 6, n_tracks=1, top_end=False)
    rows = [x for x in _rows(cols) if x[2]]
    assert sum(len(x[2]) >= 5 for x in rows) > 50
    linked = 0
    for opts in GRID:
        for _, _, ext, sc in rows:
            best, pred, mem = rchain_ref.chain_row(ext, sc, **opts)
            assert best[mem[-1]] == max(best) == rchain_ref.enumerate_row(ext, sc, **opts), (opts, ext, sc)
            linked += len(mem) > 1
    assert linked > len(rows) * len(GRID) // 4  # chains of several regions are common here


@pytest.mark.parametrize("opts", [{}, {"max_overlap": 4}, {"max_gap": 30, "max_overlap": 4, "link_cost": 2, "skew_cost": 1, "overlap_cost": 1},
                                  {"max_overlap": 2 ** 32 - 1, "overlap_cost": 3, "link_cost": 11}, {"max_gap": 8, "skew_cost": 2 ** 16}],
                         ids=lambda o: "_".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_invariants_on_a_fuzz(opts):
    cols = rchain_ref.chain_rows(7, 300, 24)
    assert int((cols[3].astype(np.int64) + cols[4]).max()) == 0xFFFFFFFF  # a region ends exactly at the top
    got = rchain_ref.chain(*cols[:6], identities=cols[6], aln_length=cols[7], **opts)
    offs, src, best, pred, score, qs, ql, ts, tl, qa, ta, ident, alen = [a.tolist() for a in got[:13]]
    gate = {k: opts.get(k, 0) for k in ("max_gap", "max_overlap")}
    price = {k: opts.get(k, 0) for k in ("link_cost", "skew_cost", "overlap_cost")}
    several = 0
    for r, b, ext, sc in _rows(cols):
        mem = src[offs[r]:offs[r + 1]]
        if not ext:
            assert not mem and score[r] == 0 and math.isnan(got[13][r]) and (qs[r], ql[r], ts[r], tl[r], qa[r], ta[r], ident[r], alen[r]) == (0,) * 8
            continue
        several += len(mem) > 1
        assert all(b <= g < b + len(ext) for g in mem) and len(set(mem)) == len(mem)
        e = lambda g: ext[g - b]
        # chain order: starts and ends ascend strictly on both sequences, every member follows the one before it and names it
        assert pred[mem[0]] == rchain_ref.NONE
        for a, c in zip(mem, mem[1:]):
            assert rchain_ref.follows(e(a), e(c), **gate) and pred[c] == a
            assert best[c] == sc[c - b] + best[a] - rchain_ref.cost(e(a), e(c), **price) and best[a] - rchain_ref.cost(e(a), e(c), **price) > 0
        # the score is the members' scores minus the links, the best of the row, at the smallest index that has it
        links = sum(rchain_ref.cost(e(a), e(c), **price) for a, c in zip(mem, mem[1:]))
        assert score[r] == best[mem[-1]] == sum(sc[g - b] for g in mem) - links == max(best[b:b + len(ext)]) and got[13][r] == float(score[r])
        assert mem[-1] == b + best[b:b + len(ext)].index(score[r])
        # no region could have done better through any predecessor, and ties went to the smaller index
        for i in range(len(ext)):
            cands = [(best[b + j] - rchain_ref.cost(ext[j], ext[i], **price), j) for j in range(len(ext)) if rchain_ref.follows(ext[j], ext[i], **gate)]
            top = max([v for v, _ in cands], default=0)
            assert best[b + i] == sc[i] + max(0, top)
            assert pred[b + i] == (b + min(j for v, j in cands if v == top) if top > 0 else rchain_ref.NONE)
        # the span and the union: a set of positions counted one by one
        f, l = e(mem[0]), e(mem[-1])
        assert (qs[r], qs[r] + ql[r], ts[r], ts[r] + tl[r]) == (f[0], l[0] + l[1], f[2], l[2] + l[3])
        if l[2] + l[3] < 2 ** 31:
            assert qa[r] == len(set().union(*[range(e(g)[0], e(g)[0] + e(g)[1]) for g in mem]))
            assert ta[r] == len(set().union(*[range(e(g)[2], e(g)[2] + e(g)[3]) for g in mem]))
        assert ident[r] == sum(int(cols[6][g]) for g in mem) and alen[r] == sum(int(cols[7][g]) for g in mem)
    assert several > 20  # rows that chain several regions exist under every option set
    assert offs[-1] == len(src)


def test_the_ladder_rows_have_long_chains():
    """A condition on the generator, not a measurement: the GPU test's rows of 700 and 3,000 regions exercise long dependent
    chains and a long walk back only if the reference chains them so."""
    cols = rchain_ref.chain_rows(21, 0, 0, lengths=[8, 9, 0, 64, 65, 31, 32, 33, 0, 1, 2, 700, 3000, 0, 3])
    n_mem = np.diff(rchain_ref.chain(*cols[:6])[0].astype(np.int64))
    assert n_mem[11] >= 50 and n_mem[12] >= 200, n_mem.tolist()
    assert (n_mem[np.diff(cols[0].astype(np.int64)) > 0] >= 1).all()


def test_coverage_reference():
    chain = rchain_ref.chain(np.array([0, 2, 2, 3], np.uint64), np.array([0, 20, 5], np.uint32), np.array([10, 10, 5], np.uint32),
                             np.array([0, 25, 0], np.uint32), np.array([10, 15, 5], np.uint32), np.array([5, 7, 3], np.int64))
    q_off, t_off = np.array([0, 40, 40], np.uint64), np.array([0, 50, 60], np.uint64)
    qid, tid = [0, 0, 1], [0, 1, 1]  # row 1 has no chain, row 2's query has no residues
    want = ([20 / 40, math.nan, math.nan], [25 / 50, math.nan, 5 / 10], [20 / 40, math.nan, math.nan], [25 / 50, math.nan, math.nan])
    for mode in range(4):
        assert np.array_equal(rchain_ref.coverage(chain, qid, tid, q_off, t_off, mode), np.array(want[mode]), equal_nan=True)


# ---- wire.region_rows(chain=...) and wire.hit_chain_rows ------------------------------------------------------------------------
Q_RECS = [("q0", b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY"), ("q1", b"MKTAYIAKQRQISFVKSHFSRQ")]
T_RECS = [("t0", b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY"), ("t1", b"MKTAYIAKQRQISFVKSHFSRQ")]
QID, TID = [0, 1], [0, 1]
REGIONS = (np.array([0, 3, 4], np.uint64), np.array([0, 2, 20, 1], np.uint32), np.array([0, 2, 20, 1], np.uint32),
           np.array([10, 5, 12, 8], np.uint32), np.array([4, 1, 6, 2], np.uint32), np.array([10, 5, 12, 8], np.uint32))
SCORES = (REGIONS[0], REGIONS[1], REGIONS[2], REGIONS[3], np.array([10, 5, 12, 8], np.int64), REGIONS[3], REGIONS[3], REGIONS[3])
ALIGNS = (REGIONS[0], np.array([0, 0, 20, 0], np.uint32), np.array([12, 12, 14, 22], np.uint32), np.array([0, 0, 20, 0], np.uint32),
          np.array([12, 12, 14, 22], np.uint32), np.array([12, 12, 14, 22], np.int64), np.array([12, 12, 13, 11], np.uint32),
          np.array([12, 12, 14, 22], np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.array([12, 12, 14, 22], np.uint32))


def _al_chain(al, **opts):
    return rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10], **opts)


def test_region_rows_with_a_chain():
    base = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS)
    chain = _al_chain(ALIGNS)  # row 0: [0,12) then [20,34) on both sequences; the copy of the first (region 1) stays outside
    assert chain[1].tolist() == [0, 2, 3] and chain[4].tolist() == [26, 22]
    rows = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, chain=chain)
    assert [{k: v for k, v in r.items() if k != "chain_pos"} for r in rows] == base and list(rows[0])[-1] == "chain_pos"
    assert [(r["query_name"], r["seed_start"], r["chain_pos"]) for r in rows] == [("q0", 0, 0), ("q0", 2, -1), ("q0", 20, 1), ("q1", 1, 0)]
    # with a cull the chain is that of the kept regions: its src_region indexes them
    cull = rcull_ref.cull(*ALIGNS[:6])
    assert cull[1].tolist() == [0, 2, 3]
    kept = (cull[0], *[c[cull[1]] for c in ALIGNS[1:]])
    k_chain = _al_chain(kept)
    assert k_chain[1].tolist() == [0, 1, 2]
    rows = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, cull=cull, chain=k_chain)
    assert [(r["seed_start"], r["chain_pos"], r["aln_rank"]) for r in rows] == [(0, 0, 1), (20, 1, 0), (1, 0, 0)]
    # a chain of the scores
    s_chain = rchain_ref.chain(SCORES[0], SCORES[1], SCORES[3], SCORES[2], None, SCORES[4])
    s_rows = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, chain=s_chain)
    assert [r["chain_pos"] for r in s_rows] == [0, -1, 1, 0]
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", chain=chain)  # a chain of nothing
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, chain=k_chain)  # of other regions
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, alignments=ALIGNS, cull=cull, chain=chain)
    with pytest.raises(ValueError):
        wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", scores=SCORES, chain=tuple(c[:-1] for c in s_chain))


def test_region_rows_without_a_chain_is_unchanged():
    for kw in ({}, {"scores": SCORES}, {"scores": SCORES, "alignments": ALIGNS}, {"alignments": ALIGNS, "cull": rcull_ref.cull(*ALIGNS[:6])}):
        a = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", **kw)
        b = wire.region_rows(Q_RECS, T_RECS, QID, TID, REGIONS, "protein", chain=None, **kw)
        assert repr(a) == repr(b) and not any("chain_pos" in r for r in a)


def test_hit_chain_rows():
    # three hit rows of query 0 and one of query 1: the order is (query's place, -chain_score, target's place); row 2 has no chain
    al = (np.array([0, 3, 4, 4, 5], np.uint64), np.array([0, 0, 20, 0, 5], np.uint32), np.array([12, 12, 14, 22, 10], np.uint32),
          np.array([0, 0, 20, 0, 5], np.uint32), np.array([12, 12, 14, 22, 10], np.uint32), np.array([12, 12, 14, 30, 8], np.int64),
          np.array([12, 12, 13, 11, 0], np.uint32), None, None, None, np.array([12, 12, 14, 22, 0], np.uint32))
    chain = _al_chain(al)
    rows = wire.hit_chain_rows(Q_RECS, T_RECS, [0, 0, 0, 1], [0, 1, 0, 1], chain)
    assert [(r["query_name"], r["match_name"], r["chain_score"], r["n_alns"]) for r in rows] == [("q0", "t1", 30, 1), ("q0", "t0", 26, 2), ("q1", "t1", 8, 1)]
    r = rows[1]
    assert list(r) == ["query_name", "match_name", "chain_score", "n_alns", "query_start", "query_end", "match_start", "match_end",
                       "q_aligned", "t_aligned", "qcov", "tcov", "pident"]
    assert (r["query_start"], r["query_end"], r["match_start"], r["match_end"], r["q_aligned"], r["t_aligned"]) == (0, 34, 0, 34, 26, 26)
    assert r["qcov"] == r["tcov"] == format_f64(26 / 40) and r["pident"] == format_f64(100.0 * 25 / 26)
    assert rows[0]["tcov"] == format_f64(22 / 22) and rows[0]["pident"] == format_f64(100.0 * 11 / 22)
    assert rows[2]["pident"] == format_f64(math.nan)  # an aln_length of 0
    with pytest.raises(ValueError):
        wire.hit_chain_rows(Q_RECS, T_RECS, [0, 0, 0], [0, 1, 0], chain)  # other hit rows
    empty = rchain_ref.chain(np.zeros(1, np.uint64), *[np.zeros(0, np.uint32)] * 4, np.zeros(0, np.int64))
    assert wire.hit_chain_rows(Q_RECS, T_RECS, [], [], empty) == []


# ---- the premise of the insertion pair -----------------------------------------------------------------------------------------
def test_insertion_pair_gives_two_alignments_a_chain_joins():
    q, t, seeds = RH.insertion_pair()
    assert q[:60] == t[:60] and q[100:] == t[60:] and len(q) == len(t) + RH.INSERTION and len(seeds) == 2
    shared = {(a, b) for a in range(len(q) - 6) for b in range(len(t) - 6) if q[a:a + 7] == t[b:b + 7]}
    assert shared == {(a, a) for a in range(0, 54)} | {(a, a - 40) for a in range(100, 154)}  # exactly the two seeds' diagonals
    regions = (np.array([0, 2], np.uint64), np.array([s[0] for s in seeds], np.uint32), np.array([s[1] for s in seeds], np.uint32),
               np.array([s[2] for s in seeds], np.uint32))
    q_res, q_off = np.frombuffer(q, np.uint8), np.array([0, len(q)], np.uint64)
    t_res, t_off = np.frombuffer(t, np.uint8), np.array([0, len(t)], np.uint64)
    al = ralign_ref.align(regions, [0], [0], q_res, q_off, t_res, t_off)  # the defaults: band 16 cannot bridge 40
    assert [(al[1][i], al[2][i], al[3][i], al[4][i]) for i in range(2)] == [(0, 60, 0, 60), (100, 60, 60, 60)]
    assert rcull_ref.cull(*al[:6])[1].tolist() == [0, 1]  # neither covers the other
    s0, s1 = int(al[5][0]), int(al[5][1])
    chain = _al_chain(al, skew_cost=1)
    assert chain[1].tolist() == [0, 1] and chain[4].tolist() == [s0 + s1 - 40] and chain[9].tolist() == [120] and chain[10].tolist() == [120]
    assert rchain_ref.coverage(chain, [0], [0], q_off, t_off, 2).tolist() == [120 / 160] and rchain_ref.coverage(chain, [0], [0], q_off, t_off, 3).tolist() == [1.0]
    alone = _al_chain(al, skew_cost=2 ** 16)
    assert alone[1].tolist() == [0] and alone[4].tolist() == [max(s0, s1)]
