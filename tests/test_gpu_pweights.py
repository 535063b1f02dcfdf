"""GPU: sequence weighting — ks_entry_weights_device (one Henikoff weight per entry), ks_wpileup_device and its two
wrappers (the pileup that sums weights) and ks_profile_build_weighted_device (the rows made from it).  Every array is compared
exactly with the plain loops of tests/pweights_ref.py, never with the code under test: the worked examples, the lane tails of the
column replay, both sides, the row CSR, 5,000 entries on 40 residues, the fuzz; sums beyond 2^32; the refusal of counts that are
not the entries'; the weighted build on its edges and on the fuzz; duplicates that do not move it; the wire end to end."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_cases as PC  # noqa: E402
import pileup_ref as PR  # noqa: E402
import profile_ref  # noqa: E402
import pweights_ref as WR  # noqa: E402
import test_gpu_pileup as TP  # noqa: E402  (its Dev: a case on the device, Context.pileup_device on raw pointers)
import test_pweights_cpu as WC  # noqa: E402  (the hand-written cases and the build's inputs)

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib  # noqa: E402

A, ONE = 28, 1 << 30
cls = lambda ch: ord(ch) - 65  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    with ks.Context(0) as c:
        yield c


class Dev(TP.Dev):
    def weights(self, side, include_query, d_counts, mask="own"):
        c = self.case
        s, o = ("q", "t") if side == "query" else ("t", "q")
        return self.ctx.entry_weights_device(
            self.ptr("row_offsets"), self.ptr("op_offsets"), self.ptr("ops"), len(c["qid"]), len(c["op_offsets"]) - 1, len(c["ops"]),
            self.ptr(s + "_start"), self.ptr(o + "_start"), self.ptr("row_mask") if mask == "own" else mask, self.hits, self.ptr(s + "_off"),
            len(c[s][1]) - 1, len(c[s][0]), self.ptr(o + "_res"), self.ptr(o + "_off"), len(c[o][1]) - 1, len(c[o][0]), d_counts, side=side,
            include_query=include_query, d_res=self.ptr(s + "_res") if include_query else None)

    def three(self, side, include_query, what):
        """the unweighted pileup, the weights from its counts and the pileup under them, each against the reference
        -> (counts, depth, weight, wdepth, wcounts) of the device"""
        args = PC.ref_args(self.case, side, True)
        pu = self.run(side, True)
        base = pu.to_host()
        want_base = reference_pileup(self.case, side)
        PR.assert_same(base, want_base, what)
        assert pu.n_weighted == 0 and pu.wdepth_ptr == 0 and pu.wcounts_ptr == 0 and [a.size for a in pu.weighted_to_host()] == [0, 0]
        ew = self.weights(side, include_query, pu.device_ptrs()[1])
        weight, n_cols = ew.to_host()
        want_w, want_n, _ = WR.weights(args, want_base[1], self.case["q" if side == "query" else "t"][0] if include_query else None, judged=True)
        assert ew.n_entries == len(want_w) and ew.weight_ptr == ew.device_ptrs()[0]
        for name, g, w in (("weight", weight, want_w), ("n_cols", n_cols, want_n)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:5].tolist(), g[:8].tolist(), w[:8].tolist())
        wp = self.run(side, True, d_weight=ew.weight_ptr)
        PR.assert_same(wp.to_host(), base, what + ": the unweighted columns of the weighted pileup")
        wdepth, wcounts = wp.weighted_to_host()
        _, want_d, want_c = WR.weighted_pileup(args, want_w, base=want_base)
        n_res = len(base[0])
        assert wp.n_weighted == n_res and (wp.wdepth_ptr != 0 and wp.wcounts_ptr != 0 or n_res == 0)
        assert wdepth.dtype == want_d.dtype and np.array_equal(wdepth, want_d) and np.array_equal(wcounts, want_c), what
        for o in (wp, ew, pu):
            o.free()
        return base[1], base[0], weight, wdepth, wcounts


_BASE = {}


def reference_pileup(case, side):
    """pileup_ref.pileup with the profile: computed once per (case, side), shared by the flags"""
    key = (id(case), side)
    if key not in _BASE:
        _BASE[key] = (case, PR.pileup(**PC.ref_args(case, side, True))[0])
    return _BASE[key][1]


def on_device(ctx, case, side="query", include_query=False, what=""):
    start = ctx.pool_stats()["bytes_in_use"]
    d = Dev(ctx, case)
    try:
        return d.three(side, include_query, what)
    finally:
        d.close()
        assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 1. the weights ----------------------------------------------------------------------------------------------------------------
def test_worked_examples(ctx):
    _, _, weight, wdepth, _ = on_device(ctx, WC.worked_case(), what="worked")
    assert weight.tolist() == [313174698, 313174698, 447392426] and wdepth.tolist() == [2 * 313174698 + 447392426] * 4
    _, _, weight, _, _ = on_device(ctx, WC.worked_case(), include_query=True, what="worked with the query")
    assert weight.tolist() == [223696213, 223696213, 402653184]
    # an entry alone weighs exactly KS_WEIGHT_ONE, a masked row and an entry without a pair column 0
    case = PC.build([(0, 0, [(0, 0, "3M2I2M")]), (0, 1, [(0, 0, "4M")]), (1, 1, [(1, 0, "2I"), (0, 2, "2M")])], [b"ACDEFGH", b"KLM"], [b"ACDEF", b"WWYY"],
                    row_mask=[1, 0, 1])
    _, _, weight, _, _ = on_device(ctx, case, what="alone")
    assert weight.tolist() == [ONE, 0, 0, ONE]


def many_ops_case():
    """entries of 63, 64 and 65 ops (1M1I ...), and all of them over the same residues of one target"""
    t = bytes(PC.ALPHABET[np.arange(40) % len(PC.ALPHABET)])
    qs = [bytes(PC.ALPHABET[(np.arange(80) * (i + 2)) % len(PC.ALPHABET)]) for i in range(3)]
    cig = lambda n: "1M1I" * (n // 2) + ("1M" if n % 2 else "")  # noqa: E731
    return PC.build([(i, 0, [(0, 0, cig(n))]) for i, n in enumerate((63, 64, 65))], qs, [t])


def classes_case():
    """all 28 classes in one column; and k = 3, n = 5: 2^30 / 15 leaves a remainder"""
    letters = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*-"
    ts = [bytes([b]) + b"W" for b in letters] + [b"GA", b"GA", b"GA", b"GA", b"GA", b"GC", b"GD"]
    rows = [(0, t, [(0, 0, "1M")]) for t in range(28)] + [(1, t, [(1, 1, "1M")]) for t in range(28, 35)]
    return PC.build(rows, [b"AC", b"KLM"], ts)


WEIGHT_CASES = {
    "lane_tails": (PC.lane_tail_case, ("query", "target")),      # pair runs of 1, 63, 64, 65, 129, 700 columns; I and D between runs
    "many_ops": (many_ops_case, ("query", "target")),
    "alternating": (PC.alternating_case, ("query",)),
    "csr": (lambda: PC.csr_rows(False), ("query", "target")),
    "one_per_row": (lambda: PC.csr_rows(True), ("query", "target")),
    "classes": (classes_case, ("query",)),
    "contention": (PC.contention_case, ("target",)),             # 5,000 entries on 40 residues
    "boundary": (lambda: PC.boundary_case(True), ("query", "target")),  # the first and the last sequence of the batch
    "fuzz": (PC.fuzz_batch, ("query",)),                          # (the target side of the fuzz: test_fuzz_under_random_weights)
}


@pytest.mark.parametrize("name", list(WEIGHT_CASES))
def test_weights_and_weighted_pileup_equal_the_reference(ctx, name):
    make, sides = WEIGHT_CASES[name]
    case = make()
    for side in sides:
        for inc in (False, True):
            counts, depth, weight, wdepth, wcounts = on_device(ctx, case, side, inc, f"{name} {side} include_query={inc}")
            assert (weight <= ONE).all()
            if name == "classes" and not inc:
                assert weight[:28].tolist() == [ONE // 28] * 28 and weight[28:33].tolist() == [ONE // 15] * 5 and weight[33:].tolist() == [ONE // 3] * 2
            if name == "contention":
                assert int(depth.max()) == 5000 and (weight > 0).all()


# ---- 2. the refusal of counts that are not the entries' ------------------------------------------------------------------------------
def test_counts_of_other_entries_are_refused(ctx):
    start = ctx.pool_stats()["bytes_in_use"]
    case = PC.csr_rows(False)
    d = Dev(ctx, case)
    pu = d.run("query", True)
    counts = pu.to_host()[1].reshape(-1, A)
    cols = WR.entry_columns(**PC.ref_args(case, "query", True))
    buf = ctx.to_device(counts)
    before = ctx.pool_stats()["bytes_in_use"]
    try:
        for offenders in ((7, 3), (len(cols) - 1,)):  # two offenders: the lowest is named
            bad = counts.copy()
            for e in offenders:
                p, c = cols[e][0]
                bad[p, c] = 0
            want = min(e for e, cs in enumerate(cols) if cs and any(bad[p, c] == 0 for p, c in cs))
            TP.upload_into(ctx, buf.ptr, bad)
            with pytest.raises(ks.KmerseekError, match=r"pileup weights: entry \d+ holds a column that the counts do not") as e:
                d.weights("query", False, buf.ptr)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG and int(re.search(r"entry (\d+)", str(e.value)).group(1)) == want <= min(offenders)
            assert ctx.pool_stats()["bytes_in_use"] == before
        TP.upload_into(ctx, buf.ptr, np.zeros_like(counts))
        with pytest.raises(ks.KmerseekError, match="entry 0 holds a column"):
            d.weights("query", False, buf.ptr)
        # with the query as a member its own class is never 0, every other is
        with pytest.raises(ks.KmerseekError, match=r"entry \d+ holds a column"):
            d.weights("query", True, buf.ptr)
        assert ctx.pool_stats()["bytes_in_use"] == before
        # the shared refusals come first, named as the pileup names them
        with pytest.raises(ks.KmerseekError, match="pileup options: side is neither"):
            ctx._check(ctx._L.ks_entry_weights_device(ctx._h, None, None, None, 0, 0, 0, None, None, None, None, None, None, 0, 0, None, None, 0, 0,
                                                       None, 2, 0, None))
        with pytest.raises(ks.KmerseekError, match="unknown flags of the weights"):
            ctx._check(ctx._L.ks_entry_weights_device(ctx._h, None, None, None, 0, 0, 0, None, None, None, None, None, d.ptr("q_off"), 0, 0,
                                                       d.ptr("t_res"), d.ptr("t_off"), 0, 0, None, 0, 2, None))
        ops = case["ops"].copy()
        ops[0] = (1 << 4) | 5  # an op that is none
        d.put("ops", ops)
        with pytest.raises(ks.KmerseekError, match=r"pileup: entry 0 holds an op that is none of"):
            d.weights("query", False, pu.device_ptrs()[1])
        assert ctx.pool_stats()["bytes_in_use"] == before
    finally:
        buf.free(); pu.free(); d.close()
    assert ctx.pool_stats()["bytes_in_use"] == start


# ---- 3. the weighted pileup under any weights -------------------------------------------------------------------------------------------
def weighted(d, side, profile, weight):
    buf = d.ctx.to_device(np.ascontiguousarray(weight, np.uint32))
    try:
        pu = d.run(side, profile, d_weight=buf.ptr)
        got, w = pu.to_host(), pu.weighted_to_host()
        assert pu.n_weighted == len(got[0]) and w[1].size == (A * len(got[0]) if profile else 0)
        pu.free()
        return got, w
    finally:
        buf.free()


def test_weights_of_one_zero_and_all_ones_bits(ctx):
    """weights all 1: wdepth == depth and wcounts == counts; 0xFFFFFFFF on 5,000 entries: the sums pass 2^32 and are exact;
    weight 0 adds to the unweighted columns alone"""
    case = PC.contention_case()
    n = len(case["op_offsets"]) - 1
    d = Dev(ctx, case)
    try:
        plain = d.run("target", True)
        base = plain.to_host()
        plain.free()
        for w in (1, 0xFFFFFFFF, 0):
            got, (wdepth, wcounts) = weighted(d, "target", True, np.full(n, w, np.uint32))
            PR.assert_same(got, base, f"weights all {w}")
            assert np.array_equal(wdepth, base[0].astype(np.uint64) * np.uint64(w)) and np.array_equal(wcounts, base[1].astype(np.uint64) * np.uint64(w))
        assert int(wdepth.max()) == 0 and int(base[0].max()) * 0xFFFFFFFF > 1 << 44
        mixed = np.where(np.arange(n) % 3 == 0, 0, np.arange(n) + 1).astype(np.uint32)
        for profile in (True, False):  # (without the profile: wdepth alone)
            got, (wdepth, wcounts) = weighted(d, "target", profile, mixed)
            args = PC.ref_args(case, "target", profile)
            want, want_d, want_c = WR.weighted_pileup(args, mixed)
            PR.assert_same(got, want, "mixed weights")
            assert np.array_equal(wdepth, want_d) and np.array_equal(wcounts, want_c)
    finally:
        d.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_fuzz_under_random_weights_on_every_path(mode, monkeypatch):
    """the fuzz batch under random weights against the reference, the per-sequence reduction sent to a wave / to a workgroup"""
    monkeypatch.setenv("KS_DEBUG_PILEUP_PATH", mode)
    case = PC.fuzz_batch()
    weight = np.random.default_rng(71).integers(0, 1 << 32, len(case["op_offsets"]) - 1, dtype=np.uint64).astype(np.uint32)
    weight[::11] = 0
    with ks.Context(0) as c:
        d = Dev(c, case)
        try:
            for side, profile in (("query", True), ("target", False)):
                got, (wdepth, wcounts) = weighted(d, side, profile, weight)
                want, want_d, want_c = fuzz_reference(side, profile, weight.tobytes())
                PR.assert_same(got, want, f"fuzz {side} path {mode}")
                assert np.array_equal(wdepth, want_d) and np.array_equal(wcounts, want_c)
        finally:
            d.close()


_FUZZ = {}


def fuzz_reference(side, profile, weight_bytes):
    key = (side, profile, weight_bytes)
    if key not in _FUZZ:  # computed once, shared by the paths
        _FUZZ[key] = WR.weighted_pileup(PC.ref_args(PC.fuzz_batch(), side, profile), np.frombuffer(weight_bytes, np.uint32))
    return _FUZZ[key]


def test_the_wrappers_on_the_stitch_cases(ctx):
    """ks_cigars_pileup_weights / ks_cigars_pileup_weighted on traced regions and ks_hitalns_pileup_weighted on stitched rows,
    through Context, against the reference run on what the objects hold"""
    import rstitch_cases as SC
    import test_gpu_region_stitch as TS
    cases = SC.pipe_cases()
    p = TS._Pipe(ctx, [c[1] for c in cases], [c[2] for c in cases], dict(band=16, gap_open=11, gap_extend=1, x_drop=30))
    q, t = p.q, p.t
    cg = p.cigars(False)
    st = p.stitch()
    cg_h, st_h, al_h = cg.to_host(), st.to_host(), p.al_host
    both = dict(q=q, t=t, qid=np.asarray(p.qid, np.uint32), tid=np.asarray(p.tid, np.uint32), row_mask=None)
    regions = dict(both, row_offsets=np.asarray(al_h[0], np.uint64), op_offsets=cg_h[0], ops=cg_h[1], q_start=al_h[1], t_start=al_h[3])
    stitched = dict(both, row_offsets=None, op_offsets=st_h[0], ops=st_h[1], q_start=st_h[2], t_start=st_h[4])
    kw = dict(side="query", offsets=q[1], other_res=t[0], other_off=t[1])
    pu = ctx.pileup(cg, p.hits, alignments=p.al, profile=True, **kw)
    args = PC.ref_args(regions, "query", True)
    for inc in (False, True):
        ew = ctx.entry_weights(cg, p.hits, pu, alignments=p.al, include_query=inc, res=q[0] if inc else None, **kw)
        want_w, want_n, _ = WR.weights(args, pu.to_host()[1], q[0] if inc else None)
        got = ew.to_host()
        assert np.array_equal(got[0], want_w) and np.array_equal(got[1], want_n) and (want_w > 0).any()
        for weights in (ew, want_w):  # the object, and a host array uploaded for the call
            wp = ctx.pileup(cg, p.hits, alignments=p.al, profile=True, weights=weights, **kw)
            want, want_d, want_c = WR.weighted_pileup(args, want_w)
            PR.assert_same(wp.to_host(), want, "cigars wrapper")
            assert all(np.array_equal(g, w) for g, w in zip(wp.weighted_to_host(), (want_d, want_c)))
            wp.free()
        ew.free()
    w = (np.arange(len(p.qid)) * 2654435761 % (1 << 32)).astype(np.uint32)
    hp = ctx.pileup(st, p.hits, profile=True, weights=w, **kw)
    want, want_d, want_c = WR.weighted_pileup(PC.ref_args(stitched, "query", True), w)
    PR.assert_same(hp.to_host(), want, "hitalns wrapper")
    assert all(np.array_equal(g, x) for g, x in zip(hp.weighted_to_host(), (want_d, want_c))) and int(want_d.max()) > 0
    hp.free()
    plain = ctx.pileup(cg, p.hits, alignments=p.al, **kw)
    with pytest.raises(ks.KmerseekError, match="pileup weights: the pileup was made without KS_PILEUP_PROFILE"):
        ctx.entry_weights(cg, p.hits, plain, alignments=p.al, **kw)
    with pytest.raises(ValueError, match="values for"):
        ctx.pileup(st, p.hits, profile=True, weights=w[:-1], **kw)
    for o in (plain, pu, st, p.ch, p.al, p.rg, p.hits, *p.cg.values()):
        o.free()


# ---- 4. the weighted build ----------------------------------------------------------------------------------------------------------
def check_wbuild(ctx, seqs, counts, wcounts, depth, params, ref=WR.build):
    q_res, q_off = ks.pack(seqs)
    counts, wcounts = np.asarray(counts, np.uint32).reshape(len(q_res), A), np.asarray(wcounts, np.uint64).reshape(len(q_res), A)
    prof = ctx.build_profile((counts, wcounts, depth), q_res, q_off, params, weighted=True)
    assert (prof.n_seqs, prof.n_residues, prof.n_scores) == (len(seqs), len(q_res), A * len(q_res))
    got, want = prof.to_host(), ref(counts, wcounts, depth, q_res, params)
    for g, w, name in zip(got, want, ks.Profile._COLUMNS):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.flatnonzero(g != w)[:5].tolist(), g[:30].tolist(), w[:30].tolist())
    prof.free()
    return want


@pytest.mark.parametrize("include_query", [True, False])
def test_wbuild_small_batches(ctx, include_query):
    """empty; 1, 2, 3 and 65 residues (a wave takes two); depth 0, W == 0 with n0 > 0 and counts beyond a byte among them"""
    rng = np.random.default_rng(80 + include_query)
    params = ks.profile_params(WC.blosum_like(rng), freq=rng.random(A) + 0.1, beta=3.5, include_query=include_query)
    check_wbuild(ctx, [], np.zeros((0, A)), np.zeros((0, A)), [], params)
    check_wbuild(ctx, [b"", b""], np.zeros((0, A)), np.zeros((0, A)), [], params)
    for lens in ((1,), (2,), (1, 0, 2), (65,), (33, 32)):
        seqs, counts, wcounts, depth = WC.wbuild_inputs(rng, lens, big=True)
        counts[0, cls("L")] = 300; wcounts[0] = 0  # W == 0 (but for the query's own term) at n0 > 0
        depth[0] = counts[0].sum()
        depth[-1] = 0
        want = check_wbuild(ctx, seqs, counts, wcounts, depth, params)
        assert include_query or want[2][0] == 0


def test_wbuild_every_class_and_unmodelled_observations(ctx):
    """all 28 classes as the residue: depth 0; modelled and unmodelled classes observed; unmodelled classes alone (n0 == 0)"""
    rng = np.random.default_rng(83)
    seq = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*-"
    m = rng.integers(-128, 128, (A, A)).astype(np.int8)
    p = ks.profile_params(WC.blosum_like(rng), beta=10.0)
    counts, wcounts = np.zeros((3 * A, A), np.uint32), np.zeros((3 * A, A), np.uint64)
    for i in range(A):
        np.add.at(counts[A + i], [cls("A"), cls("L"), i], np.array((2, 1, 3), np.uint32))
        np.add.at(wcounts[A + i], [cls("A"), cls("L"), i], np.array((ONE // 3, ONE // 5, 7), np.uint64))
        counts[2 * A + i, [cls("B"), 26, 27]] = (1 + i % 2, 2, 1)
        wcounts[2 * A + i, [cls("B"), 26, 27]] = (ONE, 2 * ONE, 5)
    for inc in (True, False):
        params = ks.ProfileParams(m, p.bg, p.ratio, p.beta, p.thresholds, p.base, inc)
        want = check_wbuild(ctx, [seq, seq + seq], counts, wcounts, counts.sum(axis=1), params)
        s = want[0].reshape(3 * A, A)
        assert np.array_equal(s[2 * A:], s[:A]) and (want[2][2 * A:] == 0).all() and not np.array_equal(s[A:2 * A], s[:A])
        assert want[1][:A].tobytes() == seq and chr(want[1][2 * A + 1]) == "*"
    by_hand = WR.build  # the three residues of test_pweights_cpu.py, on the card
    bg = np.zeros(A); bg[cls("A")] = bg[cls("C")] = 0.5
    c3, w3 = np.zeros((3, A), np.uint32), np.zeros((3, A), np.uint64)
    c3[1, cls("A")] = 2
    c3[2, [cls("A"), cls("C"), cls("G")]] = (1, 1, 1)
    w3[2, [cls("A"), cls("C"), cls("G")]] = (3, 1, ONE)
    want = check_wbuild(ctx, [b"wCC"], c3, w3, [0, 2, 3], ks.ProfileParams(None, bg, np.ones((A, A)), 0.0, [0.25, 1.0, 4.0], 0, False), ref=by_hand)
    assert want[2].tolist() == [0, 0, 2] and want[1].tobytes() == b"WCG" and int(want[0][2 * A + cls("A")]) == 2


def test_wbuild_fuzz(ctx):
    """300 sequences of 0 .. 700 residues, the flag on and off, against the column form of the reference"""
    rng = np.random.default_rng(84)
    seqs, counts, wcounts, depth = WC.wbuild_inputs(rng, rng.integers(0, 701, 300).tolist(), big=True)
    depth[::9] = 0
    m = WC.blosum_like(rng)
    for inc, beta in ((True, 10.0), (False, 0.25)):
        params = ks.profile_params(m, freq=rng.random(A) + 0.05, beta=beta, include_query=inc)
        want = check_wbuild(ctx, seqs, counts, wcounts, depth, params, ref=WR.build_columns)
        assert len(set(want[0].tolist())) > 12 and (want[2] == 0).any() and (want[2] > 0).any()


def test_duplicates_do_not_move_the_weighted_build_on_the_card(ctx):
    """every entry given 4 times: weights, weighted pileup and weighted build on the device; scores and consensus are the
    original's bit for bit, the unweighted build's are not"""
    m = np.full((A, A), -3, np.int8)
    np.fill_diagonal(m, 7)
    params = ks.profile_params(m, beta=10.0, include_query=False)
    q_res, q_off = ks.pack([b"AC"])
    made = []
    for dup in (1, 4):
        counts, depth, weight, wdepth, wcounts = on_device(ctx, WC.duplicate_case(dup), what=f"duplicates x{dup}")
        assert weight.tolist() == [ONE // (2 * dup)] * (2 * dup)
        w = ctx.build_profile((counts, wcounts, depth), q_res, q_off, params, weighted=True)
        u = ctx.build_profile((counts, depth), q_res, q_off, params)
        made.append((w.to_host(), u.to_host()))
        w.free(); u.free()
    (w1, u1), (w4, u4) = made
    assert np.array_equal(w1[0], w4[0]) and np.array_equal(w1[1], w4[1]) and w1[2].tolist() == [2, 2] and w4[2].tolist() == [8, 8]
    assert not np.array_equal(u1[0], u4[0]) and not np.array_equal(w1[0], profile_ref.matrix_rows(q_res, m).reshape(-1))


def test_wbuild_from_a_pileup_and_its_refusals(ctx):
    case = WC.worked_case()
    d = Dev(ctx, case)
    q = case["q"]
    params = ks.profile_params(None, beta=2.0)
    before = ctx.pool_stats()["bytes_in_use"]
    plain = d.run("query", True)
    with pytest.raises(ValueError, match="needs a Pileup made with weights="):
        ctx.build_profile(plain, q[0], q[1], params, weighted=True)
    opts, keep = params._opts()
    import ctypes as C
    out = C.c_void_p()
    with ctx._uploaded(q[0], q[1]) as (d_q, d_qo):
        st = ctx._L.ks_profile_build_weighted_pileup(ctx._h, plain._h, C.c_void_p(d_q), C.c_void_p(d_qo), 1, 4, C.byref(opts), C.byref(out))
    assert st == _lib.KS_ERR_INVALID_ARG and not out.value and b"made without weights" in ctx._L.ks_last_error(ctx._h)
    ew = d.weights("query", True, plain.device_ptrs()[1])
    wp = d.run("query", True, d_weight=ew.weight_ptr)
    prof = ctx.build_profile(wp, q[0], q[1], params, weighted=True)
    host, (wdepth, wcounts) = wp.to_host(), wp.weighted_to_host()
    want = WR.build(host[1], wcounts, host[0], q[0], params)
    assert all(np.array_equal(g, w) for g, w in zip(prof.to_host(), want)) and (want[2] == 4).all()
    with pytest.raises(ks.KmerseekError, match="another batch"):
        ctx.build_profile(wp, case["t"][0], case["t"][1], params, weighted=True)
    for o in (prof, wp, ew, plain):
        o.free()
    assert ctx.pool_stats()["bytes_in_use"] == before
    d.close()


# ---- 5. the wire switch -------------------------------------------------------------------------------------------------------------
def test_wire_henikoff_on_the_golden_pair(ctx, ced9_records, bcl2_records):
    """ced9 against the BCL2 set with profile_weighting="henikoff": the pssm_* columns are those of the same four calls composed
    by hand through Context; without the option, and with None, the rows are what they were"""
    import test_gpu_region_trace as TT
    from kmerseek_amd import wire
    args = (os.path.join(TT.GOLDEN, "ced9.fasta"), os.path.join(TT.GOLDEN, TT.BCL2_25), 16, 5, "hp")
    opts = dict(regions=True, gapped=True, cigar=True, cull=True, eqx=True, profile=True, profile_beta=4.0)
    unweighted = wire.search_extract_kmers_device(*args, ctx=ctx, **opts)
    assert wire.search_extract_kmers_device(*args, ctx=ctx, profile_weighting=None, **opts) == unweighted
    rows = wire.search_extract_kmers_device(*args, ctx=ctx, profile_weighting="henikoff", **opts)
    PSSM = ("pssm_score", "pssm_identities", "pssm_positives", "pssm_q_start", "pssm_q_end", "pssm_t_start", "pssm_t_end", "pssm_cigar")
    strip = lambda rs: [{k: v for k, v in r.items() if k not in PSSM} for r in rs]  # noqa: E731
    assert len(rows) == len(unweighted) >= 1 and strip(rows) == strip(unweighted) and all(set(PSSM) <= set(r) for r in rows)
    case = TT._Case(ctx, [s for _, s in ced9_records], [s for _, s in bcl2_records], 16, 5, "hp")
    q, t, h = case.q, case.t, case.hits_host
    al = case.align(band=16, gap_open=11, gap_extend=1, x_drop=30)
    cu = ctx.cull_regions(al)
    t_rg, t_al = cu.take(case.rg), cu.take(al)
    cg = ctx.trace_regions(t_rg, case.hits, *q, *t, t_al, eqx=True)
    kw = dict(side="query", offsets=q[1], alignments=t_al, other_res=t[0], other_off=t[1])
    pu = ctx.pileup(cg, case.hits, profile=True, **kw)                                    # 1
    ew = ctx.entry_weights(cg, case.hits, pu, include_query=True, res=q[0], **kw)         # 2
    wp = ctx.pileup(cg, case.hits, profile=True, weights=ew, **kw)                        # 3
    pf = ctx.build_profile(wp, q[0], q[1], ks.profile_params(None, beta=4.0), weighted=True)  # 4
    weight = ew.to_host()[0]
    assert (weight > 0).any() and (weight <= ONE).all() and wp.n_weighted == len(q[0])
    p_al = ctx.align_regions(t_rg, case.hits, *q, *t, profile=pf, band=16, gap_open=11, gap_extend=1, x_drop=30)
    p_cg = ctx.trace_regions(t_rg, case.hits, *q, *t, p_al, eqx=True, profile=pf)
    want = wire.region_rows(ced9_records, bcl2_records, h[0], h[1], case.regions, "hp", alignments=al.to_host(), cigars=cg.to_host(), cull=cu.to_host(),
                            pssm=(p_al.to_host(), p_cg.to_host()))
    assert [{k: r[k] for k in PSSM} for r in rows] == [{k: r[k] for k in PSSM} for r in want]
    for o in (p_cg, p_al, pf, wp, ew, pu, cg, t_al, t_rg, cu, al):
        o.free()
    case.close()
