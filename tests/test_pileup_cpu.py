"""CPU: the pileup reference (tests/pileup_ref.py) against the worked examples of include/kmerseek_amd.h written out by hand and
against a second, independent numpy formulation (np.add.at over expanded columns); every event of the reference is reached by the
case files the GPU test runs; wire.coverage_rows; the refusals of the Python layer that need no device; the _lib table names every
new symbol.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_cases as PC  # noqa: E402
import pileup_ref as PR  # noqa: E402

from kmerseek_amd import _lib, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {n: i for i, n in enumerate(PR.NAMES)}


def by_numpy(case, side, profile):
    """The same contract, formulated a second time: every pair column of every entry taken becomes one (position, class) record by
    array arithmetic, and np.add.at counts them.  Shares nothing with the reference but the op codes."""
    on_q = side == "query"
    s, o = ("q", "t") if on_q else ("t", "q")
    off, o_res, o_off = case[s][1].astype(np.int64), case[o][0], case[o][1].astype(np.int64)
    n_seqs, n_res = len(off) - 1, int(off[-1])
    n_rows = len(case["qid"])
    row_off = np.arange(n_rows + 1) if case["row_offsets"] is None else case["row_offsets"].astype(np.int64)
    row_of = np.repeat(np.arange(n_rows), np.diff(row_off))
    taken = np.ones(len(row_of), bool) if case["row_mask"] is None else case["row_mask"][row_of] != 0
    sid = (case["qid"] if on_q else case["tid"]).astype(np.int64)[row_of]
    oid = (case["tid"] if on_q else case["qid"]).astype(np.int64)[row_of]
    ops, op_off = case["ops"].astype(np.int64), case["op_offsets"].astype(np.int64)
    entry_of = np.repeat(np.arange(len(op_off) - 1), np.diff(op_off))
    n, c = ops >> 4, ops & 15
    pair = np.isin(c, PR.PAIR)
    moves_s = np.where(pair | (c == (PR.I if on_q else PR.D)), n, 0)
    moves_o = np.where(pair | (c == (PR.D if on_q else PR.I)), n, 0)

    def op_begin(moves, start):  # where every op begins inside its sequence
        before = np.cumsum(moves) - moves
        return before - before[np.minimum(op_off[entry_of], len(ops) - 1)] + start.astype(np.int64)[entry_of]
    use = pair & taken[entry_of] & (n > 0)
    reps = n[use]
    within = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
    pos = np.repeat(off[sid[entry_of[use]]] + op_begin(moves_s, case[s + "_start"])[use], reps) + within
    depth = np.zeros(n_res, np.int64)
    np.add.at(depth, pos, 1)
    counts = np.zeros(0, np.int64)
    if profile:
        o_pos = np.repeat(o_off[oid[entry_of[use]]] + op_begin(moves_o, case[o + "_start"])[use], reps) + within
        up = np.where((o_res >= 97) & (o_res <= 122), o_res - 32, o_res).astype(np.int64)
        cls = np.where((up >= 65) & (up <= 90), up - 65, np.where(up == 42, 26, 27))
        counts = np.zeros(n_res * PR.A, np.int64)
        np.add.at(counts, pos * PR.A + cls[o_pos], 1)
    n_aln = np.zeros(n_seqs, np.int64)
    has_pair = np.zeros(len(op_off) - 1, bool)
    has_pair[entry_of[use]] = True
    np.add.at(n_aln, sid[has_pair], 1)
    seq_of = np.repeat(np.arange(n_seqs), np.diff(off))
    length = np.diff(off)
    covered = np.bincount(seq_of[depth > 0], minlength=n_seqs)
    depth_sum = np.bincount(seq_of, weights=depth, minlength=n_seqs).astype(np.uint64)
    max_depth = np.zeros(n_seqs, np.int64)
    np.maximum.at(max_depth, seq_of, depth)
    with np.errstate(invalid="ignore", divide="ignore"):
        cols = (depth, counts, length, n_aln, covered, max_depth, depth_sum, covered.astype(np.uint32) / length.astype(np.uint32),
                depth_sum / length.astype(np.uint32))
    return tuple(np.asarray(a).astype(d) for a, d in zip(cols, PR.DTYPES))


# ---- 1. the worked examples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", PC.WORKED, ids=[w[0] for w in PC.WORKED])
def test_worked_examples_by_hand(w):
    name, cigar, nq, nt, want_q, want_t = w
    case = PC.worked_case(name)
    for side, want, n in (("query", want_q, nq), ("target", want_t, nt)):
        if want is None:
            with pytest.raises(PR.PileupError) as e:  # an N where the query side is read
                PC.reference(case, side, False)
            assert (e.value.kind, e.value.index) == ("op", 0)
            continue
        got, _ = PC.reference(case, side, False)
        assert got[COL["depth"]].tolist() == want and got[COL["length"]].tolist() == [n] and got[COL["n_alignments"]].tolist() == [1]
        assert got[COL["covered"]].tolist() == [sum(1 for d in want if d)] and got[COL["depth_sum"]].tolist() == [sum(want)]
        assert got[COL["max_depth"]].tolist() == [1] and got[COL["counts"]].size == 0
        assert got[COL["breadth"]].tolist() == [sum(1 for d in want if d) / n] and got[COL["mean_depth"]].tolist() == [sum(want) / n]
    if "N" in cigar:
        with pytest.raises(PR.PileupError):
            PC.reference(case, "target", True)  # the profile reads the query side
        return
    # the profile of 2M1I2M seen from the target: residue 2 of the target is aligned to query residue 3, behind the insertion
    got, _ = PC.reference(case, "target", True)
    q_res, counts = case["q"][0], got[COL["counts"]].reshape(-1, PR.A)
    assert np.array_equal(counts.sum(axis=1), got[COL["depth"]])
    if name == "2M1I2M":
        assert [int(np.argmax(counts[p])) for p in range(4)] == [PR.res_class(int(q_res[i])) for i in (0, 1, 3, 4)]
    if name == "2M1D2M":
        got_q, _ = PC.reference(case, "query", True)
        cq = got_q[COL["counts"]].reshape(-1, PR.A)
        assert [int(np.argmax(cq[p])) for p in range(4)] == [PR.res_class(int(case["t"][0][i])) for i in (0, 1, 3, 4)]


def test_overlapping_entries_of_one_row_each_count_and_an_entry_counts_once():
    case = PC.build([(0, 0, [(0, 0, "4M"), (2, 2, "4M"), (2, 2, "4M")]), (1, 0, [(0, 1, "2M")])], [b"ACDEFG", b"KL"], [b"ACDEFGH"])
    got, _ = PC.reference(case, "target", True)
    assert got[COL["depth"]].tolist() == [1, 2, 4, 3, 2, 2, 0] and got[COL["n_alignments"]].tolist() == [4]
    assert got[COL["covered"]].tolist() == [6] and got[COL["max_depth"]].tolist() == [4] and got[COL["depth_sum"]].tolist() == [14]
    counts = got[COL["counts"]].reshape(-1, PR.A)
    assert counts[1][PR.res_class(ord("C"))] == 1 and counts[1][PR.res_class(ord("K"))] == 1 and counts[2][PR.res_class(ord("D"))] == 3
    got_q, _ = PC.reference(case, "query", False)
    assert got_q[COL["depth"]].tolist() == [1, 1, 3, 3, 2, 2, 1, 1] and got_q[COL["n_alignments"]].tolist() == [3, 1]


def test_empty_inputs_and_nan():
    case = PC.build([], [b"", b""], [b""])
    got, ev = PC.reference(case, "query", True)
    assert got[COL["depth"]].size == 0 and got[COL["length"]].tolist() == [0, 0] and np.isnan(got[COL["breadth"]]).all() and np.isnan(got[COL["mean_depth"]]).all()
    assert "empty_sequence" in ev
    none = PC.build([], [], [])
    got, _ = PC.reference(none, "target", False)
    assert all(c.size == 0 for c in got)


# ---- 2. the reference against the second formulation -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in PC.gpu_cases()])
def test_reference_equals_the_numpy_formulation(name):
    _, case, modes = next(c for c in PC.gpu_cases() if c[0] == name)
    for side, profile in modes:
        want, _ = PC.reference(case, side, profile)
        PR.assert_same(by_numpy(case, side, profile), want, f"{name} {side} profile={profile}")


# ---- 3. every event is reached -------------------------------------------------------------------------------------------------
def test_every_event_is_reached_by_the_case_files():
    seen, by_case = set(), {}
    for name, case, modes in PC.gpu_cases():
        for side, profile in modes:
            _, ev = PC.reference(case, side, profile)
            assert ev <= set(PR.EVENTS)
            seen |= ev
            by_case.setdefault(name, set()).update(ev)
    assert seen == set(PR.EVENTS), set(PR.EVENTS) - seen
    assert {"ends_at_sequence_end", "begins_at_next_sequence_start", "empty_sequence"} <= by_case["boundary"]
    assert "depth_over_255" in by_case["contention"] and "run_merged" in by_case["alternating"] and "N_op" in by_case["fstitch"]
    assert {"masked_row", "row_without_entries", "I_on_query_side", "D_on_target_side"} <= by_case["fuzz"]
    fz = PC.fuzz_batch()
    assert 1500 <= len(fz["q_start"]) <= 2500 and len(fz["q"][1]) - 1 == 300 and int(np.diff(fz["t"][1]).max()) <= 700 and int(np.diff(fz["t"][1]).min()) == 0
    got, _ = PC.reference(PC.contention_case(), "target", False)
    assert int(got[COL["max_depth"]].max()) == 5000


# ---- 4. the reference's refusals: first kind, lowest index ------------------------------------------------------------------------
def test_reference_refusals():
    base = PC.csr_rows(False)

    def changed(**kw):
        c = dict(base)
        for k, (i, v) in kw.items():
            a = c[k].copy()
            a[i] = v
            c[k] = a
        return c
    e0 = int(base["row_offsets"][3])  # the first entry of the row of nine
    ops0 = int(base["op_offsets"][e0])
    for kind, index, case, side, profile in (
            ("row_csr", 2, changed(row_offsets=(3, 0)), "target", False),
            ("row_csr", len(base["qid"]), changed(row_offsets=(-1, 99)), "target", False),
            ("op_csr", e0 - 1, changed(op_offsets=(e0, 0)), "target", False),
            ("id", 3, changed(tid=(3, 5)), "target", False),
            ("id", 1, changed(tid=([1, 3], 99)), "target", False),
            ("id", 3, changed(qid=(3, 4)), "target", True),
            ("op", e0, changed(ops=(ops0, (3 << 4) | 4)), "target", False),
            ("op", e0, changed(ops=(ops0, (3 << 4) | PR.N)), "query", False),
            ("op", e0, changed(ops=(ops0, (3 << 4) | PR.N)), "target", True),
            ("op", e0, changed(ops=([ops0, int(base["op_offsets"][e0 + 3])], 15)), "query", False),
            ("extent", e0, changed(t_start=(e0, 79)), "target", False),
            ("extent", e0, changed(q_start=(e0, 59)), "target", True),
            ("extent", e0 + 1, changed(q_start=([e0 + 1, e0 + 5], 59)), "query", False)):
        with pytest.raises(PR.PileupError) as e:
            PC.reference(case, side, profile)
        assert (e.value.kind, e.value.index) == (kind, index), (kind, index, e.value)
    PC.reference(changed(q_start=(e0, 59)), "target", False)  # the other side is not read without the profile
    PC.reference(changed(ops=(ops0, (3 << 4) | PR.N)), "target", False)
    # an op before an id in the order of kinds, whatever their indices
    with pytest.raises(PR.PileupError) as e:
        PC.reference(changed(tid=(5, 99), ops=(ops0, 15)), "target", False)
    assert e.value.kind == "id"
    t_off = base["t"][1].copy()
    t_off[1] = t_off[2] + 1
    with pytest.raises(PR.PileupError) as e:
        PC.reference(dict(base, t=(base["t"][0], t_off)), "target", False)
    assert e.value.kind in ("seq", "offsets")


# ---- 5. wire.coverage_rows and the Python layer ---------------------------------------------------------------------------------
def test_coverage_rows():
    case = PC.boundary_case()
    got, _ = PC.reference(case, "target", False)
    recs = [(f"prot{i}", b"") for i in range(4)]
    rows = wire.coverage_rows(recs, got)
    assert [r["name"] for r in rows] == [n for n, _ in recs]
    assert list(rows[0]) == ["name", "length", "n_alignments", "covered", "breadth", "depth_sum", "mean_depth", "max_depth"]
    assert rows[0] == dict(name="prot0", length=5, n_alignments=3, covered=5, breadth="1.0", depth_sum=7, mean_depth="1.4", max_depth=2)
    assert rows[1]["breadth"] == "NaN" and rows[1]["mean_depth"] == "NaN" and rows[1]["length"] == 0
    assert rows[3] == dict(name="prot3", length=5, n_alignments=0, covered=0, breadth="0.0", depth_sum=0, mean_depth="0.0", max_depth=0)
    with pytest.raises(ValueError, match="4 sequences"):
        wire.coverage_rows(recs[:3], got)


def test_python_refusals_without_a_device(tmp_path):
    def obj(cls):
        o = cls.__new__(cls)
        o._ctx = o._h = None
        return o
    fa, ha, cg = obj(engine.FrameAlignments), obj(engine.HitAlignments), obj(engine.RegionCigars)
    off = np.zeros(2, np.uint64)
    pileup = engine.Context.pileup
    with pytest.raises(ValueError, match="side=\"query\" is not built"):
        pileup(None, fa, None, side="query", offsets=off)
    with pytest.raises(ValueError, match="profile=True is not built"):
        pileup(None, fa, None, side="target", offsets=off, profile=True)
    with pytest.raises(ValueError, match="neither"):
        pileup(None, ha, None, side="both", offsets=off)
    with pytest.raises(TypeError, match="alignments="):
        pileup(None, cg, None, offsets=off)
    with pytest.raises(TypeError, match="RegionCigars, a HitAlignments or a FrameAlignments"):
        pileup(None, object(), None, offsets=off)
    with pytest.raises(TypeError, match="offsets="):
        pileup(None, ha, None)
    with pytest.raises(ValueError, match="other_res and other_off"):
        pileup(None, ha, None, offsets=off, profile=True)
    with pytest.raises(ValueError, match="neither"):
        engine.Context.pileup_device(None, None, 0, 0, 0, 0, 0, 0, None, None, None, 0, 0, 0, side="strand")
    a = str(tmp_path / "none.fa")
    with pytest.raises(ValueError, match="cigar=True"):
        wire.search_extract_kmers_device(a, a, 7, 1, "protein", coverage="target")
    with pytest.raises(ValueError, match="none of"):
        wire.search_extract_kmers_device(a, a, 7, 1, "protein", cigar=True, gapped=True, regions=True, coverage="both")
    with pytest.raises(ValueError, match="stitch=True"):
        wire.search_translated_device(a, a, 7, 1, "protein", gapped=True, cigar=True, coverage=True)


def test_prototypes_and_table():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ks_pileup_[a-z0-9_]+|ks_[a-z]+_pileup|ks_debug_pileup_limits)\s*\(", header)))
    assert len(names) == 1 + 3 + 3 + 9 + 2 + 1 and all(n in _lib.SIGNATURES for n in names), names
    assert C.sizeof(_lib.ks_pileup_opts) == 16 and _lib.ks_pileup_opts.reserved.offset == 8
    for macro, value in (("KS_PILEUP_QUERY", 0), ("KS_PILEUP_TARGET", 1), ("KS_PILEUP_PROFILE", 1)):
        assert re.search(r"#define\s+%s\s+%du\b" % (macro, value), header) and getattr(_lib, macro) == value
    assert engine.Pileup._PREFIX == "pileup" and list(engine.Pileup._COLUMNS) == list(PR.NAMES) and list(engine.Pileup._COUNTS) == ["n_seqs", "n_residues", "n_profile"]
    assert [np.dtype(dt) for _, dt, _ in engine.Pileup._TABLE] == [np.dtype(d) for d in PR.DTYPES]
    assert isinstance(engine.Pileup.depth_ptr, property)
    assert len(_lib.SIGNATURES["ks_pileup_device"][1]) == 20 and len(_lib.SIGNATURES["ks_pileup_copy_to_host"][1]) == 11
