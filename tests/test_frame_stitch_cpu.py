"""CPU: the contract of ks_frames_stitch as tests/fstitch_ref.py restates it, on inputs made by the CPU yardsticks alone
(tests/fstitch_cases.py): the worked examples of the header, the invariants of every row, an independent re-scoring, the
single-frame rows against rstitch_ref, and the coverage of the fuzz batches the GPU test runs.  Plus the prototypes and the Python
table of the new object.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffold_ref  # noqa: E402
import fstitch_cases as FC  # noqa: E402
import fstitch_ref as FR  # noqa: E402
import rstitch_ref  # noqa: E402
from ralign_ref import default_matrix, residue_class  # noqa: E402

from kmerseek_amd import _lib, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, EQ, X, N = FR.M, FR.I, FR.D, FR.EQ, FR.X, FR.N
COL = {n: i for i, n in enumerate(FR.NAMES)}


def ref(P, max_fill=0, eqx=False, cost=FR.DEFAULT_COST):
    o = P["opts"]
    return FR.stitch(P["fold"], P["fold_hits"], P["chain"], P["alignments"], P["cigars"], *P["frames"], *P["t"], matrix=o.get("matrix"),
                     gap_open=o["gap_open"], gap_extend=o["gap_extend"], max_fill=max_fill, eqx=eqx, frameshift_cost=cost)


def rows_of(got):
    offs, ops = got[0].tolist(), got[1].tolist()
    return [[(v >> 4, v & 15) for v in ops[offs[r]:offs[r + 1]]] for r in range(len(offs) - 1)]


def check_invariants(P, got, eqx=False, cost=FR.DEFAULT_COST):
    """The two invariants, the counts, and `score` by a re-scoring written here: codon by codon from the strand's bases."""
    o = P["opts"]
    m = default_matrix() if o.get("matrix") is None else o["matrix"]
    f_res, f_off = P["frames"]
    t_res, t_off = P["t"]
    fq, ft = P["fold_hits"][0].tolist(), P["fold_hits"][1].tolist()
    for r, ops in enumerate(rows_of(got)):
        v = {n: got[i][r] for n, i in COL.items() if i >= 2}
        assert all(k >= 1 for k, _ in ops) and all(a[1] != b[1] or a[1] == N for a, b in zip(ops, ops[1:]))  # merged runs; N never
        assert {c for _, c in ops} <= ({EQ, X, I, D, N} if eqx else {M, I, D, N}) and all(k in (1, 2) for k, c in ops if c == N)
        pairs = sum(k for k, c in ops if c in (M, EQ, X))
        n_i, n_d, n_n = (sum(k for k, c in ops if c == code) for code in (I, D, N))
        assert 3 * (pairs + n_i) + n_n == v["nt_length"] and pairs + n_d == v["t_length"]
        assert pairs + n_i + n_d == v["aln_length"] and n_i + n_d == v["gaps"]
        assert sum(1 for _, c in ops if c in (I, D)) == v["gap_opens"] and sum(1 for _, c in ops if c == N) == v["n_frameshifts"]
        assert np.isnan(v["row_score"]) == (v["n_members"] == 0) and (v["n_members"] == 0 or v["row_score"] == float(v["score"]))
        if not ops:
            assert v["score"] == 0
            continue
        # the score again: every pair's codon looked up by its own strand position
        s6 = 6 * (fq[r] >> 1) + 3 * (fq[r] & 1)
        p, t, score, ident = int(v["s_start"]), int(t_off[ft[r]]) + int(v["t_start"]), 0, 0
        for k, c in ops:
            if c == N:
                p, score = p + k, score - cost
            elif c == I:
                p, score = p + 3 * k, score - (o["gap_open"] + k * o["gap_extend"])
            elif c == D:
                t, score = t + k, score - (o["gap_open"] + k * o["gap_extend"])
            else:
                for _ in range(k):
                    a, b = int(f_res[int(f_off[s6 + p % 3]) + p // 3]), int(t_res[t])
                    score += int(m[residue_class(a)][residue_class(b)]); ident += a == b
                    p += 3; t += 1
        assert score == v["score"] and ident == v["identities"], r


# ---- the worked examples ---------------------------------------------------------------------------------------------------------
WORKED = FC.worked_cases()


@pytest.mark.parametrize("case", WORKED, ids=[c[0] for c in WORKED])
def test_worked_examples(case):
    name, contig, prot, opts, max_fill, want, strand, n_shift = case
    P = FC.cpu_inputs([contig], [prot], **opts)
    got, _ = ref(P, max_fill)
    rows = [r for r in range(len(P["fold_hits"][0])) if P["fold_hits"][0][r] == strand]
    assert len(rows) == 1, (name, P["fold_hits"])
    r = rows[0]
    assert FR.strings(got[0], got[1])[r] == want, name
    assert got[COL["n_frameshifts"]][r] == n_shift and got[COL["t_start"]][r] == 0 and got[COL["t_length"]][r] == len(prot)
    pad = int(name.split("pad")[1][0])
    assert got[COL["s_start"]][r] == pad  # (in the strand's own orientation: behind the pad on either strand)
    nt_start = got[COL["nt_start"]][r]
    assert nt_start == (2 if strand else pad) and nt_start + got[COL["nt_length"]][r] == len(contig) - (pad if strand else 2)
    check_invariants(P, got)
    if n_shift:
        assert got[COL["score"]][r] == ref(P, max_fill, cost=0)[0][COL["score"]][r] - FR.DEFAULT_COST


@pytest.mark.parametrize("reverse", [False, True])
def test_member_rows(reverse):
    P = FC.member_inputs([c["members"] for c in FC.MEMBER_ROWS], reverse=reverse)
    got, _ = ref(P)
    text = FR.strings(got[0], got[1])
    f_res, f_off = P["frames"]
    for r, c in enumerate(FC.MEMBER_ROWS):
        assert text[r] == c["expect"], c["name"]
        assert tuple(int(got[COL[n]][r]) for n in ("n_filled", "n_open", "n_trimmed", "n_frameshifts")) == c["counts"], c["name"]
        frames3 = [bytes(f_res[int(f_off[6 * r + 3 * reverse + f]):int(f_off[6 * r + 3 * reverse + f + 1])]) for f in range(3)]
        members = [(f + 3 * qs, 3 * ql, ts, tl, FC.SC.parse(cg)) for f, qs, ql, ts, tl, cg in c["members"]]
        _, _, _, _, ev = FR.stitch_row(members, frames3, b"K" * 60, default_matrix(), 11, 1)
        assert ev == c["events"], (c["name"], ev)
    check_invariants(P, got)
    # nt_start on the record as given: the first member's forward, the last member's reverse
    first, last = FC.MEMBER_ROWS[1]["members"][0], FC.MEMBER_ROWS[1]["members"][-1]
    want = 120 - last[0] - 3 * (last[1] + last[2]) if reverse else first[0] + 3 * first[1]
    assert got[COL["nt_start"]][1] == want


def test_reference_refusals():
    P = FC.member_inputs([c["members"] for c in FC.MEMBER_ROWS])

    def changed(key, i, j, v):
        Q = dict(P)
        cols = [np.array(c) for c in P[key]]
        cols[i][j] = v
        Q[key] = tuple(cols)
        return Q
    n = len(P["alignments"][1])
    for kind, index, Q in (("src", 2, changed("chain", 1, 2, 5)), ("fsrc", 1, changed("fold", 2, 1, n)), ("fold", 3, changed("fold", 5, 3, 7)),
                           ("strand", 0, changed("fold", 3, 0, 4)), ("row", 1, changed("fold_hits", 1, 1, 1)), ("ext", 4, changed("alignments", 3, 4, 55)),
                           ("ops", 0, changed("cigars", 1, 0, (9 << 4) | M)), ("code", 0, changed("cigars", 1, 0, (10 << 4) | EQ)),
                           ("asc", 4, changed("alignments", 3, 3, 2))):
        with pytest.raises(FR.StitchError) as e:
            if kind in ("ext", "asc"):  # (the fold must still be of the alignments: refold, the chain stays)
                al = Q["alignments"]
                Q["fold"] = ffold_ref.fold(*Q["frame_hits"], Q["nt_off"], *al[:5], score=al[5], identities=al[6], aln_length=al[10])[1]
            ref(Q)
        assert (e.value.kind, e.value.index) == (kind, index), (kind, e.value)


# ---- the fuzz: coverage, invariants, single-frame rows --------------------------------------------------------------------------
def single_frame_rows(P):
    """folded rows whose chain members all lie in one frame -> [(row, frame 0 .. 5)]"""
    c_offs, c_src, frame = P["chain"][0].tolist(), P["chain"][1].tolist(), P["fold"][3].tolist()
    out = []
    for r in range(len(c_offs) - 1):
        fr = {frame[g] for g in c_src[c_offs[r]:c_offs[r + 1]]}
        if len(fr) == 1:
            out.append((r, fr.pop()))
    return out


def check_single_frame_rows(P, got, max_fill, eqx):
    """a row in one frame is rstitch_ref.stitch_row on that frame's residues, positions mapped by p = f + 3 q, and no N"""
    o = P["opts"]
    m = default_matrix() if o.get("matrix") is None else o["matrix"]
    f_res, f_off = P["frames"]
    t_res, t_off = P["t"]
    c_offs, c_src, f_src = P["chain"][0].tolist(), P["chain"][1].tolist(), P["fold"][2].tolist()
    al, (g_offs, g_ops) = P["alignments"], P["cigars"]
    rows, n = rows_of(got), 0
    for r, fr in single_frame_rows(P):
        q, t = int(P["fold_hits"][0][r]), int(P["fold_hits"][1][r])
        fs = 6 * (q >> 1) + fr
        qseq, tseq = bytes(f_res[int(f_off[fs]):int(f_off[fs + 1])]), bytes(t_res[int(t_off[t]):int(t_off[t + 1])])
        gs = [f_src[g] for g in c_src[c_offs[r]:c_offs[r + 1]]]
        members = [(int(al[1][g]), int(al[2][g]), int(al[3][g]), int(al[4][g]), [(int(v) >> 4, int(v) & 15) for v in g_ops[int(g_offs[g]):int(g_offs[g + 1])]])
                   for g in gs]
        cigar, n_filled, n_open, n_trim, _ = rstitch_ref.stitch_row(members, qseq, tseq, m, o["gap_open"], o["gap_extend"], max_fill or 1024, eqx)
        assert rows[r] == cigar and N not in {c for _, c in cigar}
        assert tuple(int(got[COL[k]][r]) for k in ("n_filled", "n_open", "n_trimmed", "n_frameshifts")) == (n_filled, n_open, n_trim, 0)
        assert got[COL["s_start"]][r] == fr % 3 + 3 * members[0][0] and got[COL["nt_length"]][r] == 3 * (members[-1][0] + members[-1][1] - members[0][0])
        n += len(members) > 1
    return n


def test_fuzz_rows():
    """the runs the GPU test makes — both batches, with and without eqx — reach every event together"""
    events, multi = set(), 0
    for i, eqx in ((0, False), (0, True), (1, False), (1, True)):
        F = FC.FUZZ[i]
        P = FC.fuzz_inputs(i, eqx)
        assert len(P["fold_hits"][0]) <= 300
        got, ev = ref(P, F["max_fill"], eqx)
        events |= ev
        check_invariants(P, got, eqx)
        multi += check_single_frame_rows(P, got, F["max_fill"], eqx)
        print(F["name"], "rows", len(got[2]), "members", int(got[COL["n_members"]].sum()), "shifts", int(got[COL["n_frameshifts"]].sum()), sorted(ev))
    assert events == set(FR.EVENTS), set(FR.EVENTS) - events
    assert multi >= 3  # single-frame rows of more than one member exist


def test_planted_contigs_by_the_cpu_pipeline():
    """What the GPU test asserts of the wire's stitched rows holds for the reference pipeline, for all 24 contigs: a shifted
    contig's row has exactly one N op, within the overhang bound of tests/test_gpu_ffold.py (5 residues = 15 bases) of the planted
    base; an unshifted contig's row has none."""
    proteins, contigs, truth = FC.planted()
    P = FC.cpu_inputs(contigs, proteins, band=16, gap_open=11, gap_extend=1, x_drop=20)
    got, _ = ref(P)
    by = {(int(q), int(t)): r for r, (q, t) in enumerate(zip(P["fold_hits"][0], P["fold_hits"][1]))}
    rows = rows_of(got)
    for t in truth:
        r = by[(2 * t["record"] + int(t["reverse"]), t["target"])]
        shifts = [(k, c) for k, c in rows[r] if c == N]
        assert len(shifts) == (1 if t["shifted"] else 0), (t, FR.strings(got[0], got[1])[r])
        if t["shifted"]:
            p = int(got[COL["s_start"]][r])
            for k, c in rows[r]:
                if c == N:
                    break
                p += 3 * k if c in (M, EQ, X, I) else 0
            nt_pos = t["contig_length"] - p - 1 if t["reverse"] else p  # the skipped base on the record as given
            planted_at = (t["end"] - 1 - 3 * t["m"]) if t["reverse"] else t["start"] + 3 * t["m"]
            assert abs(nt_pos - planted_at) <= 15, (t, nt_pos, planted_at)
    check_invariants(P, got)


# ---- above the ABI -------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_table():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ks_framealns_[a-z0-9_]+|ks_frames_stitch)\s*\(", header)))
    assert len(names) == 1 + 4 + 19 + 2 and all(n in _lib.SIGNATURES for n in names)
    assert C.sizeof(_lib.ks_fstitch_opts) == 24 and _lib.ks_fstitch_opts.max_scratch_bytes.offset == 16
    assert _lib.KS_CIGAR_FSHIFT == N == engine.CIGAR_OPS.index("N") and _lib.KS_FSTITCH_MAX_COST == 2 ** 16
    assert re.search(r"#define\s+KS_CIGAR_FSHIFT\s+3u", header)
    assert engine.FrameAlignments._COLUMNS == FR.NAMES
    assert [np.dtype(dt) for _, dt, _ in engine.FrameAlignments._TABLE] == [np.dtype(d) for d in FR.DTYPES]
    assert engine.cigar_strings([0, 3], [(10 << 4) | M, (1 << 4) | N, (5 << 4) | M]) == ["10M1N5M"]
    for bad in (dict(max_fill=4097), dict(frameshift_cost=2 ** 16 + 1), dict(frameshift_cost=-1)):
        with pytest.raises(ValueError):
            engine.Context._fstitch_opts(**{**dict(max_fill=0, eqx=False, frameshift_cost=15, max_scratch_bytes=0), **bad})
    csrc = lambda name: open(os.path.join(ROOT, "kmerseek_amd", "csrc", name)).read()  # noqa: E731
    src, kit = csrc("ks_fstitch.hip") + csrc("ks_rstitch.hip"), csrc("ks_stitch_kit.h")
    # one recurrence, in the fill kit, called by the one fill kernel of the stitch kit that both passes instantiate
    assert "rf_fill(" not in src and kit.count("rf_fill(") == 1 and "ra_e_step" not in src + kit


def test_frame_chain_rows_with_stitched_columns():
    P = FC.member_inputs([c["members"] for c in FC.MEMBER_ROWS], reverse=True)
    got, _ = ref(P)
    nt = [(f"rec{i}", b"T" * 120) for i in range(len(FC.MEMBER_ROWS))]
    plain = wire.frame_chain_rows(nt, [("prot", b"K" * 60)], P["fold_hits"], P["fold"], P["chain"])
    rows = wire.frame_chain_rows(nt, [("prot", b"K" * 60)], P["fold_hits"], P["fold"], P["chain"], stitched=got)
    # nothing of today's rows changes but aln_length, which becomes the one alignment's
    old = lambda row, like: {k: v for k, v in row.items() if k in like and k != "aln_length"}  # noqa: E731
    assert [old(r, p) for r, p in zip(rows, plain)] == [old(p, p) for p in plain]
    extra = set(rows[0]) - set(plain[0])
    assert extra == {"aln_cigar", "aln_score", "aln_identities", "aln_positives", "aln_gap_opens", "aln_gaps", "aln_pident", "n_filled", "n_open",
                     "aln_frameshifts"} and "aln_length" in plain[0]
    r0 = rows[0]  # 10M1N1N5M on the reverse strand of a record of 120 bases: the skipped bases are strand positions 30 and 31
    assert r0["aln_cigar"] == "10M1N1N5M" and r0["aln_frameshifts"] == "89:1,88:1" and r0["aln_length"] == 15 and r0["aln_pident"] == wire.format_f64(100.0)
    assert rows[3]["aln_frameshifts"] == "%d:2" % (120 - 36 - 2) and rows[4]["aln_frameshifts"] == ""
