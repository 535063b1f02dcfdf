"""No GPU: the stitch's yardstick (tests/rstitch_ref.py) against hand-written expectations and against exhaustive enumeration,
what the GPU test's fuzz inputs exercise, the row builder of the wire, and the option refusals of the C entry point.

1. The reference against tests/rstitch_cases.py: chains written down member by member, and pairs of sequences through the CPU
   pipeline (oracle join, regions, alignments, cull, paths, chain), each with its expected CIGAR.
2. Every global path over every rectangle up to 4 x 4 on a three-letter alphabet, enumerated: the fill's score is the maximum,
   both orientations give it, and re-scoring the fill's columns gives it.
3. The inputs of tests/test_gpu_region_stitch.py, on the CPU: the union of the events of its fuzz batches and of its doctored
   chain covers every class of link, trim and tie the reference names — so none is silently absent on the device.  The fuzz
   alone cannot reach `trimmed_to_nothing`: it needs a member that ends where the member in front of it ends, and a chain made
   of the alignments themselves links only regions whose ends ascend STRICTLY on both sequences (follows(),
   include/kmerseek_amd.h).  The GPU test therefore stitches one chain made from doctored columns (rstitch_cases.duplicate_pair),
   and this test shows that it is that case.
4. Every option, flag and reserved-field refusal of ks_regions_stitch with ctx == NULL (skipped only where the library is not
   built: the symbol does not exist before this feature).
5. hit_chain_rows(..., stitched=...) on hand-made arrays, and the prerequisites of search_extract_kmers_device(stitch=True)."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ralign_ref  # noqa: E402
import rchain_ref  # noqa: E402
import rstitch_cases as SC  # noqa: E402
import rstitch_ref as SR  # noqa: E402
import rtrace_ref  # noqa: E402

from kmerseek_amd import _lib, wire  # noqa: E402
from kmerseek_amd.wire import format_f64  # noqa: E402

M, I, D, EQ, X = SR.M, SR.I, SR.D, SR.EQ, SR.X
FUZZ_UNREACHABLE = {"trimmed_to_nothing"}  # (see 3. above)


def _stitch(P, align, max_fill=0, eqx=False):
    return SR.stitch(P["chain"], P["alignments"], P["cigars"], P["hits"][0], P["hits"][1], P["q"][0], P["q"][1], P["t"][0], P["t"][1],
                     gap_open=align["gap_open"], gap_extend=align["gap_extend"], max_fill=max_fill, eqx=eqx)


# ---- 1. the hand-written cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.MEMBER_CASES, ids=lambda c: c["name"])
def test_reference_on_chains_written_down(c):
    m = ralign_ref.default_matrix()
    members = [(qs, ql, ts, tl, SC.parse(cg)) for qs, ql, ts, tl, cg in c["members"]]
    cigar, n_filled, n_open, n_trim, events = SR.stitch_row(members, c["q"], c["t"], m, c["o"], c["e"], c.get("max_fill", SR.DEFAULT_MAX_FILL))
    assert rtrace_ref.cigar_string(cigar) == c["expect"]
    assert (n_filled, n_open, n_trim) == c["counts"] and events >= c["events"]
    # the ops consume exactly the span from the first member's start to the last member's end
    qs, ts = members[0][0], members[0][2]
    res = rtrace_ref.rescore(cigar, c["q"], c["t"], qs, ts, m, c["o"], c["e"])
    assert res[6:] == (members[-1][0] + members[-1][1] - qs, members[-1][2] + members[-1][3] - ts)
    if len(members) == 1:  # a row of one member is that member
        assert cigar == members[0][4]


def test_reference_refuses_what_the_library_refuses():
    m, a = ralign_ref.default_matrix(), b"A" * 50
    for members, eqx in (([(0, 10, 0, 10, "9M")], False), ([(0, 10, 0, 10, "10M")], True), ([(0, 10, 0, 10, "10=")], False),
                         ([(45, 10, 0, 10, "10M")], False), ([(0, 10, 0, 10, "10M"), (2, 7, 12, 5, "5M2I")], False)):
        with pytest.raises(ValueError):
            SR.stitch_row([(qs, ql, ts, tl, SC.parse(cg)) for qs, ql, ts, tl, cg in members], a, a, m, 11, 1, eqx=eqx)


@pytest.mark.parametrize("case", SC.pipe_cases(), ids=lambda c: c[0])
def test_reference_on_pairs_through_the_cpu_pipeline(case):
    name, q, t, opts, want, want_eqx = case
    for eqx, w in ((False, want), (True, want_eqx)):
        P = SC.cpu_inputs([q], [t], eqx=eqx, **opts)
        got, _ = _stitch(P, opts, eqx=eqx)
        assert SR.strings(got[0], got[1]) == [w]
        assert (got[2][0], got[3][0], got[4][0], got[5][0]) == (0, len(q), 0, len(t)) and got[12][0] == 2
        assert got[11][0] == sum(n for n, _ in SC.parse(w))
    if name == "insertion_pair":  # one alignment where the chain had two and a heuristic sum
        s0, s1 = (int(v) for v in P["alignments"][5])
        assert got[6][0] == s0 + s1 - (11 + SC.INSERTION) and got[9][0] == 1 and got[10][0] == SC.INSERTION and got[7][0] == 120


# ---- 2. exhaustive enumeration --------------------------------------------------------------------------------------------------
def _best_global(q, t, m, o, e):
    """The best score over every global path, by brute force: every interleaving of pairs, I and D columns."""
    best = None

    def rec(i, j, last, score):
        nonlocal best
        if i == len(q) and j == len(t):
            best = score if best is None or score > best else best
            return
        if i < len(q) and j < len(t):
            rec(i + 1, j + 1, M, score + m[ralign_ref.residue_class(q[i])][ralign_ref.residue_class(t[j])])
        if i < len(q):
            rec(i + 1, j, I, score - e - (0 if last == I else o))
        if j < len(t):
            rec(i, j + 1, D, score - e - (0 if last == D else o))
    rec(0, 0, None, 0)
    return best


def test_fill_against_every_global_path():
    rng = np.random.default_rng(31)
    m = [[int(v) for v in row] for row in rng.integers(-3, 4, (28, 28)).tolist()]  # not symmetric: the orientation must not matter
    n = 0
    for o, e in ((0, 0), (1, 1), (3, 2)):
        for x in range(1, 5):
            for y in range(1, 5):
                for q in itertools.product(b"ACD", repeat=x):
                    for t in itertools.product(b"ACD", repeat=y):
                        q_, t_ = bytes(q), bytes(t)
                        cols, score, _, swapped = SR.fill(q_, t_, m, o, e, False)
                        assert swapped == (x < y)
                        assert score == _best_global(q_, t_, m, o, e), (q_, t_, o, e)
                        res = rtrace_ref.rescore(rtrace_ref.run_length(cols), q_, t_, 0, 0, m, o, e)
                        assert res[0] == score and res[6:] == (x, y), (q_, t_, o, e, cols)
                        n += 1
    assert n == 3 * sum(3 ** x * 3 ** y for x in range(1, 5) for y in range(1, 5))


# ---- 3. what the GPU test's fuzz inputs exercise ---------------------------------------------------------------------------------
def test_the_gpu_tests_fuzz_inputs_cover_every_event():
    seen = set()
    for F in SC.FUZZ:
        qs, ts = F["batch"]()
        assert max(len(s) for s in qs + ts) <= 200
        for eqx in (False, True):
            P = SC.cpu_inputs(qs, ts, eqx=eqx, **F["align"], **F["chain"])
            got, events = _stitch(P, F["align"], max_fill=F["max_fill"], eqx=eqx)
            seen |= events
            # the invariants of the header, on the reference's own output
            offs, ops = got[0].tolist(), got[1].tolist()
            for r in range(len(offs) - 1):
                mine = [(v >> 4, v & 15) for v in ops[offs[r]:offs[r + 1]]]
                pairs = sum(k for k, c in mine if c in (M, EQ, X))
                assert all(a[1] != b[1] for a, b in zip(mine, mine[1:])) and all(k >= 1 for k, _ in mine)
                assert sum(k for k, _ in mine) == got[11][r] and pairs + sum(k for k, c in mine if c == I) == got[3][r]
                assert pairs + sum(k for k, c in mine if c == D) == got[5][r]
                assert sum(1 for _, c in mine if c in (I, D)) == got[9][r] and sum(k for k, c in mine if c in (I, D)) == got[10][r]
            assert all(np.array_equal(got[i], P["chain"][j]) for i, j in ((2, 5), (3, 6), (4, 7), (5, 8)))  # the chain's span
    assert set(SR.EVENTS) - seen == FUZZ_UNREACHABLE, sorted(set(SR.EVENTS) - seen)
    # the doctored chain: one alignment twice in a row without the cull, linked by a chain of shifted columns
    q, t, opts = SC.duplicate_pair()
    P = SC.cpu_inputs([q], [t], cull=False, **opts)
    al = P["alignments"]
    assert [c.tolist() for c in al[1:5]] == [[0, 0], [61, 61], [0, 0], [61, 61]]
    assert P["chain"][1].tolist() == [0]  # the chain of the alignments themselves does not link them
    P["chain"] = rchain_ref.chain(*SC.doctored_columns(al), **SC.DOCTORED_CHAIN)
    assert P["chain"][1].tolist() == [0, 1]
    got, events = _stitch(P, opts)
    assert SR.strings(got[0], got[1]) == ["61M"] and (got[12][0], got[15][0]) == (2, 61) and events == {"trimmed", "trimmed_to_nothing"}
    assert set(SR.EVENTS) <= seen | events


# ---- 4. the option refusals of the C entry point ------------------------------------------------------------------------------------
def test_option_refusals_with_a_null_context():
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    L = _lib.load()

    def call(max_fill=0, flags=0, scratch=0, reserved=(0, 0), null_opts=False):
        opts = _lib.ks_rstitch_opts(max_fill, flags, scratch, (C.c_uint32 * 2)(*reserved))
        out = C.c_void_p(1)
        st = L.ks_regions_stitch(None, None, None, None, None, None, None, 0, 0, None, None, 0, 0, None if null_opts else C.byref(opts), C.byref(out))
        assert out.value == 1  # nothing is written without a context
        return st
    bad = 4  # KS_ERR_INVALID_ARG
    assert L.ks_status_string(bad) is not None
    for kw in (dict(max_fill=_lib.KS_RSTITCH_MAX_FILL + 1), dict(max_fill=2 ** 32 - 1), dict(flags=2), dict(flags=_lib.KS_RSTITCH_EQX | 4),
               dict(flags=2 ** 31), dict(reserved=(1, 0)), dict(reserved=(0, 7)), dict(), dict(max_fill=_lib.KS_RSTITCH_MAX_FILL, flags=1), dict(null_opts=True)):
        assert call(**kw) == bad, kw  # (valid options too: a NULL context is refused after them)
    assert int(L.ks_debug_rstitch_stage()) == 64
    assert C.sizeof(_lib.ks_rstitch_opts) == 24
    assert all(L.ks_hitalns_n_rows(None) == 0 and getattr(L, "ks_hitalns_device_" + c)(None) is None for c in ("ops", "row_score"))
    L.ks_hitalns_free(None)


# ---- 5. the wire ---------------------------------------------------------------------------------------------------------------------
Q_RECS = [("q0", b"A" * 40), ("q1", b"C" * 30)]
T_RECS = [("t0", b"A" * 40), ("t1", b"C" * 22)]


def test_hit_chain_rows_with_stitched_alignments():
    al = (np.array([0, 3, 4, 4, 5], np.uint64), np.array([0, 0, 20, 0, 5], np.uint32), np.array([12, 12, 14, 22, 10], np.uint32),
          np.array([0, 0, 20, 0, 5], np.uint32), np.array([12, 12, 14, 22, 10], np.uint32), np.array([12, 12, 14, 30, 8], np.int64),
          np.array([12, 12, 13, 11, 0], np.uint32), None, None, None, np.array([12, 12, 14, 22, 0], np.uint32))
    chain = rchain_ref.chain(*al[:6], identities=al[6], aln_length=al[10])
    qid, tid = [0, 0, 0, 1], [0, 1, 0, 1]
    base = wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain)
    assert repr(wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stitched=None)) == repr(base)
    enc = lambda s: [(n << 4) | c for n, c in SC.parse(s)]
    rows_ops = [enc("12M8I8D14M"), enc("22M"), [], enc("10M")]
    ops = [v for r in rows_ops for v in r]
    offs = np.cumsum([0] + [len(r) for r in rows_ops]).astype(np.uint64)
    u = lambda *v: np.array(v, np.uint32)
    st = (offs, np.array(ops, np.uint32), u(0, 0, 0, 5), u(34, 22, 0, 10), u(0, 0, 0, 5), u(34, 22, 0, 10), np.array([0, 30, 0, 8], np.int64),
          u(25, 11, 0, 0), u(25, 11, 0, 4), u(2, 0, 0, 0), u(16, 0, 0, 0), u(42, 22, 0, 10), u(2, 1, 0, 1), u(0, 0, 0, 0), u(1, 0, 0, 0),
          u(0, 0, 0, 0), np.array([0.0, 30.0, math.nan, 8.0]))
    rows = wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stitched=st)
    added = ["aln_cigar", "aln_score", "aln_identities", "aln_positives", "aln_gap_opens", "aln_gaps", "aln_length", "aln_pident", "n_filled", "n_open"]
    assert [list(r) for r in rows] == [list(b) + added for b in base]
    assert [{k: v for k, v in r.items() if k not in added} for r in rows] == base
    r = rows[1]  # (q0, t0): the chain of two
    assert (r["match_name"], r["aln_cigar"], r["aln_score"], r["aln_gap_opens"], r["aln_gaps"], r["aln_length"], r["n_open"]) == ("t0", "12M8I8D14M", 0, 2, 16, 42, 1)
    assert r["aln_pident"] == format_f64(100.0 * 25 / 42) and r["pident"] == format_f64(100.0 * 25 / 26)
    assert rows[0]["aln_cigar"] == "22M" and rows[2]["aln_pident"] == format_f64(0.0)
    with pytest.raises(ValueError):
        wire.hit_chain_rows(Q_RECS, T_RECS, qid, tid, chain, stitched=tuple(c[:-1] for c in st))


def test_stitch_needs_its_prerequisites():
    on = dict(regions=True, gapped=True, cigar=True, chain=True, hit_rows=True)
    for missing in ("gapped", "cigar", "chain", "hit_rows"):
        kw = dict(on, **{missing: False})
        with pytest.raises(ValueError, match=f"stitch=True needs {missing}=True"):
            wire.search_extract_kmers_device("q.fa", "t.fa", 7, 1, "protein", stitch=True, **kw)
