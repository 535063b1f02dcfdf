"""GPU: ks_pileup_device and its three wrappers — per-residue depth and profile, per-sequence coverage.  Every array is compared
exactly with the plain-loop reference of tests/pileup_ref.py (the two quotients bit for bit), never with the code under test:
empty inputs, the boundary marks, the lane tails of the profile pass, 300 alternating ops, the row CSR and its one-entry-per-row
form, row masks, 5,000 entries on 40 residues, the fuzz on both sides with and without the profile, the CIGARs of the stitch
cases, every forced path of the per-sequence reduction around its limit, the two wires end to end, and every refusal with two
offenders."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_sketches as crafted  # noqa: E402
import pileup_cases as PC  # noqa: E402
import pileup_ref as PR  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, engine, wire  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCL2_25 = "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz"
INVALID, CAPACITY = _lib.KS_ERR_INVALID_ARG, _lib.KS_ERR_CAPACITY
COL = {n: i for i, n in enumerate(PR.NAMES)}
MODES = (None, "1", "2")  # KS_DEBUG_PILEUP_PATH
BOTH = [(s, p) for s in ("query", "target") for p in (False, True)]


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


@pytest.fixture(params=MODES, ids=lambda m: f"path_{m}")
def mode_ctx(request, monkeypatch):
    """A context created after KS_DEBUG_PILEUP_PATH is set (the knobs are read when a context is made)."""
    if request.param is None:
        monkeypatch.delenv("KS_DEBUG_PILEUP_PATH", raising=False)
    else:
        monkeypatch.setenv("KS_DEBUG_PILEUP_PATH", request.param)
    with ks.Context(0) as c:
        yield c


def upload_into(ctx, d_ptr, a):
    a = np.ascontiguousarray(a)
    ctx._check(ctx._L.ks_dev_upload(ctx._h, C.c_void_p(int(d_ptr)), a.ctypes.data_as(C.c_void_p), a.nbytes))
    ctx.synchronize()


def hits_with(ctx, qid, tid):
    """A Hits of len(qid) rows whose qid and tid columns hold exactly these values (the pass reads nothing else of a hit list):
    row i of a crafted search is (i, 0) through a hash of its own; the two columns are then overwritten on the device."""
    n = len(qid)
    h = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    one = np.ones(n, np.uint32)
    if n:
        Q, T = crafted._csr(np.arange(n), h, one, n), crafted._csr(np.zeros(n, np.int64), h, one, 1)
    else:  # no row: two sketches that share nothing
        Q, T = crafted._csr([0], [2], [1], 1), crafted._csr([0], [4], [1], 1)
    sq, st = ctx.sketches_from_host(*Q, 10, 1, "protein"), ctx.sketches_from_host(*T, 10, 1, "protein")
    ix = ctx.index_build(st)
    hits = ctx.search(ix, sq)
    for o in (ix, sq, st):
        o.free()
    assert hits.count == n
    if n:
        p = hits.device_ptrs()
        upload_into(ctx, p[0], np.asarray(qid, np.uint32)); upload_into(ctx, p[1], np.asarray(tid, np.uint32))
    return hits


class Dev:
    """A case of tests/pileup_cases.py on the device: every array uploaded once, Context.pileup_device on raw pointers."""
    KEYS = ("row_offsets", "op_offsets", "ops", "q_start", "t_start", "row_mask")

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.host = {k: case[k] for k in self.KEYS if case[k] is not None}
        self.host.update(q_res=case["q"][0], q_off=case["q"][1], t_res=case["t"][0], t_off=case["t"][1])
        self.buf = {k: ctx.to_device(v if v.size else np.zeros(2, v.dtype)) for k, v in self.host.items()}
        self.hits = hits_with(ctx, case["qid"], case["tid"])

    def ptr(self, k):
        return self.buf[k].ptr if k in self.buf else None

    def put(self, k, a):
        """overwrite a device array (same size) with `a`"""
        upload_into(self.ctx, self.buf[k].ptr, a)

    def run(self, side, profile, mask="own", **kw):
        c = self.case
        s, o = ("q", "t") if side == "query" else ("t", "q")
        args = dict(d_row_offsets=self.ptr("row_offsets"), d_op_offsets=self.ptr("op_offsets"), d_ops=self.ptr("ops"), n_rows=len(c["qid"]),
                    n_entries=len(c["op_offsets"]) - 1, n_ops=len(c["ops"]), d_start=self.ptr(s + "_start"),
                    d_other_start=self.ptr(o + "_start") if profile else None, d_row_mask=self.ptr("row_mask") if mask == "own" else mask,
                    hits=self.hits, d_offsets=self.ptr(s + "_off"), n_seqs=len(c[s][1]) - 1, n_res=len(c[s][0]), side=side, profile=profile)
        if profile:
            args.update(d_other_res=self.ptr(o + "_res"), d_other_off=self.ptr(o + "_off"), n_other=len(c[o][1]) - 1, n_other_res=len(c[o][0]))
        args.update(kw)
        return self.ctx.pileup_device(**args)

    def check(self, side, profile, what, case=None, **kw):
        pu = self.run(side, profile, **kw)
        got = pu.to_host()
        c = case or self.case
        n_seqs, n_res = len(c["q" if side == "query" else "t"][1]) - 1, len(c["q" if side == "query" else "t"][0])
        assert (pu.n_seqs, pu.n_residues, pu.n_profile) == (n_seqs, n_res, PR.A * n_res if profile else 0)
        assert pu.depth_ptr == pu.device_ptrs()[0] != 0 and len(pu.device_ptrs()) == 9
        pu.free()
        want, events = PC.reference(c, side, profile)
        PR.assert_same(got, want, f"{what} {side} profile={profile}")
        return got, events

    def close(self):
        for b in self.buf.values():
            b.free()
        self.hits.free()


# ---- 1. empty inputs ---------------------------------------------------------------------------------------------------------------
def test_empty_inputs(ctx):
    start = ctx.pool_stats()["bytes_in_use"]
    seqs = [b"ACDEF", b"", b"GHIKLMN"]
    for name, case in (("zero rows", PC.build([], seqs, seqs)), ("rows without entries", PC.build([(0, 0, []), (2, 1, [])], seqs, seqs)),
                       ("every sequence empty", PC.build([(0, 1, [(0, 0, "0M")])], [b"", b""], [b"", b"", b""])),
                       ("no sequence", PC.build([], [], []))):
        d = Dev(ctx, case)
        try:
            for side, profile in BOTH:
                got, _ = d.check(side, profile, name)
                assert not got[COL["depth"]].any() and not got[COL["n_alignments"]].any()
                assert np.array_equal(np.isnan(got[COL["breadth"]]), got[COL["length"]] == 0)
                assert got[COL["counts"]].shape == ((PR.A * len(got[COL["depth"]]),) if profile else (0,))
        finally:
            d.close()
    assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 2. the case files -------------------------------------------------------------------------------------------------------------
CASES = {name: (case, modes) for name, case, modes in PC.gpu_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_equal_the_reference(ctx, name):
    case, modes = CASES[name]
    start = ctx.pool_stats()["bytes_in_use"]
    d = Dev(ctx, case)
    try:
        for side, profile in modes:
            got, events = d.check(side, profile, name)
            if name == "boundary" and side == "target":
                # 3M at 0, an end on the last residue of sequence 0, a begin on the first of sequence 2, nothing on sequence 3
                assert got[COL["depth"]].tolist() == [1, 1, 2, 1, 2] + [1, 1, 0, 1, 1, 1, 1] + [0] * 5
                assert {"ends_at_sequence_end", "begins_at_next_sequence_start", "empty_sequence"} <= events
            if name == "boundary_to_the_end":
                assert got[COL["depth"]][-4:].tolist() == [1, 1, 1, 1] and got[COL["covered"]].tolist()[3] == 4
            if name == "contention":
                assert int(got[COL["max_depth"]][1]) == 5000 and int(got[COL["n_alignments"]][1]) == 5000 and int(got[COL["covered"]][1]) == 40
            if name == "lane_tails" and side == "target":
                assert got[COL["covered"]].tolist()[:6] == [2, 63, 68, 65, 129, 700]
            if profile:
                assert np.array_equal(got[COL["counts"]].reshape(-1, PR.A).sum(axis=1), got[COL["depth"]])
    finally:
        d.close()
    assert ctx.pool_stats()["bytes_in_use"] == start


def test_csr_and_one_entry_per_row_agree(ctx):
    a, b = Dev(ctx, PC.csr_rows(False)), Dev(ctx, PC.csr_rows(True))
    try:
        assert a.case["row_offsets"] is not None and b.case["row_offsets"] is None and np.array_equal(a.case["ops"], b.case["ops"])
        assert sorted(np.diff(a.case["row_offsets"].astype(np.int64)).tolist()) == [0, 0, 1, 1, 2, 9]
        for side, profile in BOTH:
            x, _ = a.check(side, profile, "csr")
            y, _ = b.check(side, profile, "one per row")
            PR.assert_same(x, y, "csr against one per row")
    finally:
        a.close(); b.close()


# ---- 3. row masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "last", "every_second", "none", "all"])
def test_row_masks(ctx, which):
    base = PC.fuzz_batch(seed=11, n_seqs=40, n_rows=60)
    n = len(base["qid"])
    mask = np.ones(n, np.uint8)
    if which == "first":
        mask[0] = 0
    elif which == "last":
        mask[-1] = 0
    elif which == "every_second":
        mask[1::2] = 0
    elif which == "all":
        mask[:] = 0
    case = dict(base, row_mask=None if which == "none" else mask)
    d = Dev(ctx, dict(base, row_mask=mask))
    try:
        for side, profile in (("target", True), ("query", False)):
            got, _ = d.check(side, profile, which, case=case, mask=None if which == "none" else "own")
            assert which != "all" or not got[COL["depth"]].any()
    finally:
        d.close()


# ---- 4. every path of the per-sequence reduction -----------------------------------------------------------------------------------
def limit():
    a = C.c_uint32(0)
    _lib.load().ks_debug_pileup_limits(C.byref(a))
    return int(a.value)


def test_forced_paths_around_the_limit(mode_ctx):
    w = limit()
    assert 64 <= w <= 4096
    lens = [w - 1, w, w + 1, 0, 1, 63, 64, 65, 3 * w + 7]
    rng = np.random.default_rng(5)
    ts = [bytes(PC.ALPHABET[rng.integers(0, len(PC.ALPHABET), n)]) for n in lens]
    qs = [bytes(PC.ALPHABET[rng.integers(0, len(PC.ALPHABET), 200)]) for _ in range(3)]
    rows = []
    for q in range(3):
        for t, n in enumerate(lens):
            if n == 0:
                continue
            entries = []
            for _ in range(3):
                m = int(rng.integers(1, min(n, 200) + 1))
                entries.append((int(rng.integers(0, 200 - m + 1)), int(rng.integers(0, n - m + 1)), f"{m}M"))
            entries.append((0, n - 1, "1M"))  # the last residue
            rows.append((q, t, entries))
    d = Dev(mode_ctx, PC.build(rows, qs, ts))
    try:
        got, _ = d.check("target", False, "paths")
        assert got[COL["length"]].tolist() == lens and int(got[COL["covered"]].min()) == 0 and np.isnan(got[COL["breadth"]][3])
        ends = [int(e) - 1 for e, n in zip(d.case["t"][1][1:], lens) if n]
        assert all(int(got[COL["depth"]][p]) >= 3 for p in ends)  # the last residue of every sequence, by three rows
        d.check("target", True, "paths")
    finally:
        d.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
class Recorder:
    """Context.pileup, wrapped: what it was given — the to_host() of the alignments, the hits, the mask — is kept, the call goes on."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = engine.Context.pileup

        def pileup(ctx, aligned, hits, side="target", offsets=None, alignments=None, row_mask=None, **kw):
            self.calls.append(dict(kind=type(aligned).__name__, aligned=aligned.to_host(), hits=hits.to_host(), side=side, offsets=np.array(offsets),
                                   alignments=None if alignments is None else alignments.to_host(),
                                   row_mask=None if row_mask is None else np.array(row_mask), kw=kw))
            return inner(ctx, aligned, hits, side=side, offsets=offsets, alignments=alignments, row_mask=row_mask, **kw)
        monkeypatch.setattr(engine.Context, "pileup", pileup)

    def reference(self, i=-1):
        """the reference on the recorded arrays of call i (depth only) -> the arrays of Pileup.to_host()"""
        c = self.calls[i]
        a = c["aligned"]
        if c["kind"] == "RegionCigars":
            al = c["alignments"]
            row_off, op_off, ops, start = al[0], a[0], a[1], al[1] if c["side"] == "query" else al[3]
        elif c["kind"] == "HitAlignments":
            row_off, op_off, ops, start = None, a[0], a[1], a[2] if c["side"] == "query" else a[4]
        else:
            assert c["kind"] == "FrameAlignments" and c["side"] == "target"
            row_off, op_off, ops, start = None, a[0], a[1], a[5]
        assert not c["kw"].get("profile")
        return PR.pileup(row_off, op_off, ops, start, None, c["row_mask"], c["hits"][0], c["hits"][1], c["offsets"], side=c["side"])[0]


def test_golden_pair_through_the_wire(ctx, monkeypatch):
    rec = Recorder(monkeypatch)
    q_fa, t_fa = os.path.join(GOLDEN, "ced9.fasta"), os.path.join(GOLDEN, BCL2_25)
    t_recs, q_recs = wire.read_fasta(t_fa), wire.read_fasta(q_fa)
    start = ctx.pool_stats()["bytes_in_use"]
    on = dict(ctx=ctx, regions=True, gapped=True, cigar=True, cull=True, chain=True, hit_rows=True, chain_max_overlap=5, chain_skew_cost=1)
    plain = wire.search_extract_kmers_device(q_fa, t_fa, 16, 5, "hp", stitch=True, **on)
    rows, cov = wire.search_extract_kmers_device(q_fa, t_fa, 16, 5, "hp", stitch=True, coverage="target", **on)
    assert rows == plain and len(rec.calls) == 1 and rec.calls[0]["kind"] == "HitAlignments"
    assert cov == wire.coverage_rows(t_recs, rec.reference())
    assert [r["name"] for r in cov] == [n for n, _ in t_recs] and sum(r["n_alignments"] for r in cov) == len(rows) > 0
    assert all(r["covered"] <= r["length"] and r["max_depth"] <= 1 for r in cov)  # one query: a residue is placed once per hit
    # the traced alignments of the kept regions, query side: ced9 covered by all its relatives
    rows2, cov_q = wire.search_extract_kmers_device(q_fa, t_fa, 16, 5, "hp", coverage="query", **{**on, "chain": False, "hit_rows": False})
    assert rec.calls[-1]["kind"] == "RegionCigars" and cov_q == wire.coverage_rows(q_recs, rec.reference())
    assert len(cov_q) == 1 and cov_q[0]["max_depth"] >= 1 and cov_q[0]["n_alignments"] == len(rows2)
    assert ctx.pool_stats()["bytes_in_use"] == start


def test_planted_contigs_through_the_wire(ctx, monkeypatch, tmp_path):
    import fstitch_cases as FC
    rec = Recorder(monkeypatch)
    proteins, contigs, truth = FC.planted()
    # relatives of the first four proteins, every twelfth residue replaced: their contigs hit two proteins, top_k = 1 drops one
    proteins = list(proteins) + [bytes((87 if c != 87 else 89) if i % 12 == 5 else c for i, c in enumerate(p)) for p in proteins[:4]]
    nt_fa, t_fa = tmp_path / "contigs.fa", tmp_path / "proteins.fa"
    nt_fa.write_bytes(b"".join(b">contig%d\n%s\n" % (i, s) for i, s in enumerate(contigs)))
    t_fa.write_bytes(b"".join(b">prot%d\n%s\n" % (i, s) for i, s in enumerate(proteins)))
    t_recs = wire.read_fasta(str(t_fa))
    start = ctx.pool_stats()["bytes_in_use"]
    kw = dict(ctx=ctx, gapped=True, gapped_x_drop=20, chain_max_overlap=15, cigar=True, stitch=True)
    plain = wire.search_translated_device(str(nt_fa), str(t_fa), FC.K, 1, "protein", **kw)
    for top_k in (0, 1):
        rows, cov = wire.search_translated_device(str(nt_fa), str(t_fa), FC.K, 1, "protein", coverage=True, top_k=top_k, **kw)
        call = rec.calls[-1]
        assert call["kind"] == "FrameAlignments" and (call["row_mask"] is None) == (top_k == 0)
        assert cov == wire.coverage_rows(t_recs, rec.reference())
        if top_k == 0:
            assert rows == plain
        else:
            assert 0 < int(call["row_mask"].sum()) < len(call["row_mask"])
        by = {r["name"]: r for r in cov}
        for t in truth:  # every planted gene covers its protein (the bound tests/test_gpu_frame_stitch.py sets for the score)
            r = by[f"prot{t['target']}"]
            assert r["n_alignments"] >= 1 and r["covered"] >= t["length"] - 2 * FC.K - 15, (t, r)
    assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------
WORDS = {"row_csr": ("row_offsets descends", "hit row"), "op_csr": ("op_offsets descends", "entry"), "id": ("beyond its batch", "hit row"),
         "op": ("none of M I D N = X", "entry"), "extent": ("consume more of a sequence", "entry"), "seq": ("lies on a sequence whose offsets", "entry"),
         "offsets": ("descend or pass the batch", "sequence")}


def test_refusals_name_the_first_offender(ctx):
    """One device array at a time is overwritten with a changed copy (and put back): the reference refuses the same arrays for the
    same kind and names the same index — with two offenders the lower one — and the pool holds what it held."""
    base = PC.csr_rows(False)
    d = Dev(ctx, base)
    try:
        e0 = int(base["row_offsets"][3])  # the first entry of the row of nine
        o = base["op_offsets"]
        ops0, ops3 = int(o[e0]), int(o[e0 + 3])
        n_rows = len(base["qid"])
        hp = d.hits.device_ptrs()
        t_off_bad = base["t"][1].copy()
        t_off_bad[2] = t_off_bad[3] + 1  # sequence 2, the row of nine's, descends
        t_off_two = t_off_bad.copy()
        t_off_two[4] = t_off_two[5] + 1  # sequence 3, of the row before it, passes the batch; sequence 4 descends
        changes = [
            ("row_csr", 2, "target", False, [("row_offsets", 3, 0)]), ("row_csr", 1, "target", False, [("row_offsets", 4, 1), ("row_offsets", 1, 2)]),
            ("row_csr", n_rows, "query", True, [("row_offsets", n_rows, 99)]),
            ("op_csr", e0 - 1, "target", False, [("op_offsets", e0, 0)]), ("op_csr", 1, "target", False, [("op_offsets", e0 + 2, 1), ("op_offsets", 1, 100)]),
            ("op_csr", len(o) - 1, "query", False, [("op_offsets", len(o) - 1, int(o[-1]) - 1)]),
            ("id", 3, "target", False, [("tid", 3, 5)]), ("id", 1, "target", False, [("tid", 3, 99), ("tid", 1, 5)]),
            ("id", 3, "target", True, [("qid", 3, 4)]), ("id", 2, "query", False, [("qid", 5, 2 ** 32 - 1), ("qid", 2, 4)]),
            ("op", e0, "target", False, [("ops", ops0, (3 << 4) | 4)]), ("op", e0, "query", False, [("ops", ops0, (3 << 4) | PR.N)]),
            ("op", e0, "target", True, [("ops", ops0, (3 << 4) | PR.N)]), ("op", e0, "query", True, [("ops", ops3, 15), ("ops", ops0, (9 << 4) | 6)]),
            ("extent", e0, "target", False, [("t_start", e0, 79)]), ("extent", e0, "target", True, [("q_start", e0, 59)]),
            ("extent", e0 + 1, "query", False, [("q_start", e0 + 5, 2 ** 32 - 1), ("q_start", e0 + 1, 59)]),
            ("extent", e0, "query", False, [("ops", ops0, (2 ** 28 - 1) << 4)]),
        ]
        idle = ctx.pool_stats()["bytes_in_use"]
        for kind, index, side, profile, edits in changes:
            case = dict(base)
            for key, at, v in edits:
                a = case[key].copy()
                a[at] = v
                case[key] = a
            for key in {k for k, _, _ in edits}:
                if key in ("qid", "tid"):
                    upload_into(ctx, hp[0 if key == "qid" else 1], case[key])
                else:
                    d.put(key, case[key])
            with pytest.raises(PR.PileupError) as ref:
                PC.reference(case, side, profile)
            assert (ref.value.kind, ref.value.index) == (kind, index), (kind, index, ref.value)
            with pytest.raises(ks.KmerseekError) as e:
                d.run(side, profile)
            words, noun = WORDS[kind]
            assert e.value.status == INVALID and words in str(e.value) and re.search(r"\b%s %d\b" % (noun, index), str(e.value)), (kind, str(e.value))
            assert ctx.pool_stats()["bytes_in_use"] == idle, kind
            for key in {k for k, _, _ in edits}:
                if key in ("qid", "tid"):
                    upload_into(ctx, hp[0 if key == "qid" else 1], base[key])
                else:
                    d.put(key, base[key])
        # the offsets of the side's batch: an entry on such a sequence, then (no entry taken) the sequence itself
        for offs, mask_all, kind, noun in ((t_off_bad, False, "seq", "entry"), (t_off_two, False, "seq", "entry"), (t_off_bad, True, "offsets", "sequence"),
                                           (t_off_two, True, "offsets", "sequence")):
            d.put("t_off", offs)
            case = dict(base, t=(base["t"][0], offs), row_mask=np.zeros(n_rows, np.uint8) if mask_all else None)
            with pytest.raises(PR.PileupError) as ref:
                PC.reference(case, "target", False)
            assert ref.value.kind == kind
            zeros = ctx.to_device(np.zeros(n_rows, np.uint8))
            with pytest.raises(ks.KmerseekError) as e:
                d.run("target", False, mask=zeros.ptr if mask_all else None)
            zeros.free()
            assert e.value.status == INVALID and WORDS[kind][0] in str(e.value) and re.search(r"\b%s %d\b" % (noun, ref.value.index), str(e.value)), str(e.value)
            assert ctx.pool_stats()["bytes_in_use"] == idle
            d.put("t_off", base["t"][1])
        # the other batch's offsets with the profile
        q_off_bad = base["q"][1].copy()
        q_off_bad[3] = q_off_bad[2] - 1
        d.put("q_off", q_off_bad)
        with pytest.raises(PR.PileupError) as ref:
            PC.reference(dict(base, q=(base["q"][0], q_off_bad)), "target", True)
        with pytest.raises(ks.KmerseekError) as e:
            d.run("target", True)
        assert ref.value.kind == "seq" and re.search(r"\bentry %d\b" % ref.value.index, str(e.value)) and ctx.pool_stats()["bytes_in_use"] == idle
        d.put("q_off", base["q"][1])
        d.check("target", True, "after the refusals")  # everything is back: the context works

        # before any device work
        L = ctx._L
        out = C.c_void_p()
        P = d.ptr
        vp = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        n_e, n_ops = len(o) - 1, len(base["ops"])
        nt, nq = len(base["t"][1]) - 1, len(base["q"][1]) - 1

        def call(c=ctx._h, row_off=P("row_offsets"), op_off=P("op_offsets"), ops=P("ops"), n_rows_=n_rows, n_e_=n_e, start=P("t_start"),
                 other_start=P("q_start"), hits=d.hits._h, offs=P("t_off"), n_res=len(base["t"][0]), o_res=P("q_res"), o_off=P("q_off"), opts=None,
                 out_p=C.byref(out)):
            return L.ks_pileup_device(c, vp(row_off), vp(op_off), vp(ops), n_rows_, n_e_, n_ops, vp(start), vp(other_start), None, hits, vp(offs), nt, n_res,
                                      vp(o_res), vp(o_off), nq, len(base["q"][0]), opts, out_p)
        prof_t = _lib.ks_pileup_opts(_lib.KS_PILEUP_PROFILE, _lib.KS_PILEUP_TARGET, 0)
        for opts, kw in ((_lib.ks_pileup_opts(2, 0, 0), {}), (_lib.ks_pileup_opts(0, 2, 0), {}), (_lib.ks_pileup_opts(0, 1, 1), {}),
                         (prof_t, dict(o_off=0)), (prof_t, dict(o_res=0)), (prof_t, dict(other_start=0))):
            assert call(opts=C.byref(opts), **kw) == INVALID and "pileup options" in L.ks_last_error(ctx._h).decode(), (opts.flags, opts.side, kw)
            assert call(c=None, opts=C.byref(opts), **kw) == INVALID and not out.value
        assert call(c=None) == INVALID
        for kw in (dict(op_off=0), dict(ops=0), dict(start=0), dict(hits=None), dict(offs=0), dict(out_p=None)):
            assert call(**kw) == INVALID and "NULL" in L.ks_last_error(ctx._h).decode(), kw
        assert call(n_rows_=n_rows - 1) == INVALID and "alignments of another search" in L.ks_last_error(ctx._h).decode()
        assert call(row_off=0) == INVALID and "without row_offsets" in L.ks_last_error(ctx._h).decode()
        with ks.Context(0) as other_ctx:
            assert call(c=other_ctx._h) == INVALID and "another context" in L.ks_last_error(other_ctx._h).decode()
        assert call(n_res=2 ** 32 - 1) == CAPACITY and "32-bit scan" in L.ks_last_error(ctx._h).decode()
        assert call(opts=C.byref(prof_t)) == _lib.KS_OK and out.value
        L.ks_pileup_free(out)
        assert call() == _lib.KS_OK and L.ks_pileup_n_profile(out) == 0  # opts NULL: the depth of the query side
        L.ks_pileup_free(out)
        assert ctx.pool_stats()["bytes_in_use"] == idle
    finally:
        d.close()


def test_frame_alignments_refuse_the_query_side_and_the_profile_by_name(ctx):
    L = ctx._L
    out = C.c_void_p()
    for opts, word in ((_lib.ks_pileup_opts(0, _lib.KS_PILEUP_QUERY, 0), "KS_PILEUP_TARGET only"),
                       (_lib.ks_pileup_opts(_lib.KS_PILEUP_PROFILE, _lib.KS_PILEUP_TARGET, 0), "no profile"),
                       (None, "KS_PILEUP_TARGET only")):  # (the default side is the query's)
        o = C.byref(opts) if opts is not None else None
        assert L.ks_frames_pileup(ctx._h, None, None, None, None, 0, 0, o, C.byref(out)) == INVALID
        msg = L.ks_last_error(ctx._h).decode()
        assert "frame alignments" in msg and word in msg, msg
        assert L.ks_frames_pileup(None, None, None, None, None, 0, 0, o, C.byref(out)) == INVALID
    ok = _lib.ks_pileup_opts(0, _lib.KS_PILEUP_TARGET, 0)
    assert L.ks_frames_pileup(ctx._h, None, None, None, None, 0, 0, C.byref(ok), C.byref(out)) == INVALID and "NULL" in L.ks_last_error(ctx._h).decode()
    fa = engine.FrameAlignments.__new__(engine.FrameAlignments)
    fa._ctx, fa._h = ctx, None
    off = np.zeros(2, np.uint64)
    with pytest.raises(ValueError, match="side=\"query\" is not built"):
        ctx.pileup(fa, None, side="query", offsets=off)
    with pytest.raises(ValueError, match="profile=True is not built"):
        ctx.pileup(fa, None, side="target", offsets=off, profile=True)
