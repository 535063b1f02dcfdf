"""No GPU: the frame fold's yardstick (tests/ffold_ref.py) against hand-written expectations, its two coordinate formulas against
the six-frame translation of tests/translate_ref.py on genes planted on both strands, wire.frame_chain_rows on hand-made arrays,
and the ctypes prototypes of the new entry points against the header."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffold_ref  # noqa: E402
import translate_ref  # noqa: E402

from kmerseek_amd import _lib, engine, wire  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = ffold_ref.NONE

# Four records of 30, 31, 32 and 31 bases (L = 0, 1, 2, 1 mod 3); record 1 has no rows.  Hit rows (qid, tid) and their regions
# (q_start, q_length, t_start, t_length); frame lengths: L = 30: 10, 9, 9; L = 31: 10, 10, 9; L = 32: 10, 10, 10.
LENGTHS = (30, 31, 32, 31)
ROWS = [
    ((0, 5), [(0, 4, 1, 4), (6, 4, 8, 5)]),   # 0: record 0 +, frame 0; tid 5 is in frames 0 and 2 but not 1; first and last residue
    ((0, 7), [(2, 3, 0, 3)]),                 # 1: tid 7 is in all three frames
    ((1, 3), []),                             # 2: one frame only, and a row without regions
    ((1, 7), [(0, 9, 3, 9)]),                 # 3: the whole frame
    ((2, 5), [(5, 4, 20, 4)]),                # 4: the last residue of frame 2
    ((2, 7), [(1, 2, 10, 2)]),                # 5
    ((3, 5), [(0, 10, 0, 10)]),               # 6: record 0 -, frame 0: both strands of one record; the whole frame
    ((4, 5), [(8, 1, 2, 1)]),                 # 7: the last residue of reverse frame 1
    ((13, 2), [(9, 1, 0, 1)]),                # 8: record 2 +, frame 1: the last residue
    ((17, 0), []),                            # 9: record 2 -, frame 2, no regions
    ((22, 1), [(7, 3, 0, 3)]),                # 10: record 3 -, frame 1: the last residue is base 0 of the record
]
WANT_HITS = ([0, 0, 0, 1, 4, 5, 7], [3, 5, 7, 5, 2, 0, 1], [3, 6, 12, 15, 9, 10, 11], [30, 60, 120, 150, 90, 100, 110])
WANT = {
    "src_row": [X, 2, X, 0, X, 4, 1, 3, 5, 6, 7, X, X, 8, X, X, X, 9, X, 10, X],
    "row_offsets": [0, 0, 3, 6, 8, 9, 9, 10],
    "src_region": [0, 1, 4, 2, 3, 5, 6, 7, 8, 9],
    "frame": [0, 0, 2, 0, 1, 2, 3, 4, 1, 4],
    "nt_length": [12, 12, 12, 9, 27, 6, 30, 3, 3, 9],
    "s_start": [0, 18, 17, 6, 1, 5, 0, 25, 28, 22],
    "nt_start": [0, 18, 17, 6, 1, 5, 0, 2, 28, 0],
    "t_start3": [3, 24, 60, 0, 9, 30, 0, 6, 0, 0],
    "t_length3": [12, 15, 12, 9, 27, 6, 30, 3, 3, 9],
}


def hand_case():
    qid = [q for (q, _), _ in ROWS]
    tid = [t for (_, t), _ in ROWS]
    isect = [i + 1 for i in range(len(ROWS))]
    nw = [10 * (i + 1) for i in range(len(ROWS))]
    offs = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.uint64)
    row_offs = np.concatenate([[0], np.cumsum([len(r) for _, r in ROWS])]).astype(np.uint64)
    regs = [g for _, r in ROWS for g in r]
    cols = [np.array([g[i] for g in regs], np.uint32) for i in range(4)]
    return qid, tid, isect, nw, offs, row_offs, cols


def test_hand_written_fold():
    qid, tid, isect, nw, offs, row_offs, cols = hand_case()
    n = len(cols[0])
    score = np.arange(100, 100 + n, dtype=np.int64)
    ident = np.arange(n, dtype=np.uint32)
    hits, got = ffold_ref.fold(qid, tid, isect, nw, offs, row_offs, *cols, score=score, identities=ident)
    assert [h.tolist() for h in hits] == [list(c) for c in WANT_HITS]
    named = dict(zip(ffold_ref.NAMES, got))
    for name, want in WANT.items():
        assert named[name].tolist() == want, name
        assert named[name].dtype == dict(zip(ffold_ref.NAMES, ffold_ref.DTYPES))[name]
    assert named["score"].tolist() == [100 + g for g in WANT["src_region"]] and named["identities"].tolist() == WANT["src_region"]
    assert named["aln_length"] is None
    # t_length None: the target lengths are the query lengths
    _, same = ffold_ref.fold(qid, tid, isect, nw, offs, row_offs, cols[0], cols[1], cols[2])
    assert dict(zip(ffold_ref.NAMES, same))["t_length3"].tolist() == named["nt_length"].tolist() and same[9] is None


def test_empty_inputs_and_saturation():
    z32, z64 = np.zeros(0, np.uint32), np.zeros(1, np.uint64)
    hits, cols = ffold_ref.fold([], [], [], [], [0, 9], z64, z32, z32, z32)
    assert all(len(h) == 0 for h in hits) and cols[1].tolist() == [0] and len(cols[0]) == 0 and len(cols[2]) == 0
    hits, cols = ffold_ref.fold([0, 1, 2], [4, 4, 4], [2 ** 32 - 1, 5, 1], [2 ** 64 - 1, 3, 0], [0, 9], [0, 0, 0, 0], z32, z32, z32)
    assert [h.tolist() for h in hits] == [[0], [4], [2 ** 32 - 1], [2]] and cols[0].tolist() == [0, 1, 2] and cols[1].tolist() == [0, 0]


@pytest.mark.parametrize("kind,index,change", [
    ("offsets", 0, dict(offs=[1, 30, 61, 93, 124])), ("offsets", 2, dict(offs=[0, 30, 61, 60, 124])),
    ("long", 1, dict(offs=[0, 30, 30 + 2 ** 32 - 15, 2 ** 32 + 100, 2 ** 32 + 200])),
    ("qid", 10, dict(offs=[0, 30, 61, 93])), ("order", 4, dict(swap=(3, 4))), ("order", 6, dict(dup=6)),
    ("csr", 0, dict(row_offs={0: 1})), ("csr", 3, dict(row_offs={4: 2})), ("csr", 10, dict(row_offs={11: 9})),
    ("qend", 7, dict(reg=(7, 1, 2))), ("qend", 3, dict(reg=(3, 0, 1))), ("tend", 5, dict(reg=(5, 2, (2 ** 32 - 1) // 3 - 1))),
])
def test_reference_refusals(kind, index, change):
    qid, tid, isect, nw, offs, row_offs, cols = hand_case()
    if "offs" in change:
        offs = np.array(change["offs"], np.uint64)
    if "swap" in change:
        a, b = change["swap"]
        qid[a], qid[b], tid[a], tid[b] = qid[b], qid[a], tid[b], tid[a]
    if "dup" in change:
        qid[change["dup"]], tid[change["dup"]] = qid[change["dup"] - 1], tid[change["dup"] - 1]
    for i, v in change.get("row_offs", {}).items():
        row_offs[i] = v
    if "reg" in change:
        g, c, v = change["reg"]
        cols[c][g] = v
    with pytest.raises(ffold_ref.FoldError) as e:
        ffold_ref.fold(qid, tid, isect, nw, offs, row_offs, *cols)
    assert (e.value.kind, e.value.index) == (kind, index)


@pytest.mark.parametrize("pad", [10, 11, 12])
@pytest.mark.parametrize("reverse", [False, True])
def test_coordinate_formulas_on_planted_genes(pad, reverse):
    """A gene between flanks of `pad` bases on the left and pad + 1, pad + 2, pad + 3 on the right, on either strand: the frame
    that holds the protein is found by search, and the fold's nt_start / s_start must be exactly where the gene's bases lie."""
    rng = np.random.default_rng([7, pad, int(reverse)])
    aa = b"ACDEFGHIKLMNPQRSTVWY"
    for right in (pad + 1, pad + 2, pad + 3):
        protein = bytes(aa[i] for i in rng.integers(0, 20, 40))
        gene = translate_ref.reverse_translate(protein, rng)
        flank = lambda n: bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
        planted = translate_ref.reverse_complement(gene) if reverse else gene
        contig = flank(pad) + planted + flank(right)
        L = len(contig)
        frames = translate_ref.translate6([contig])
        found = [(f, frames[f].find(protein)) for f in range(6) if frames[f].find(protein) >= 0]
        assert len(found) == 1 and (found[0][0] >= 3) == reverse, found
        f6, i = found[0]
        offs = np.array([0, L], np.uint64)
        one = np.array([0, 1], np.uint64)
        hits, cols = ffold_ref.fold([f6], [0], [1], [1], offs, one, [i], [len(protein)], [0])
        c = dict(zip(ffold_ref.NAMES, cols))
        nt_start, s_start, nt_len = int(c["nt_start"][0]), int(c["s_start"][0]), int(c["nt_length"][0])
        assert nt_len == len(gene) and hits[0].tolist() == [1 if reverse else 0] and c["frame"].tolist() == [f6]
        assert nt_start == pad and contig[nt_start:nt_start + nt_len] == planted
        strand = translate_ref.reverse_complement(contig) if reverse else contig
        assert strand[s_start:s_start + nt_len] == gene and s_start == (right if reverse else pad)
        # a region of the frame's first and of its last residue stays inside the record
        flen = ffold_ref.frame_len(L, f6 % 3)
        _, ends = ffold_ref.fold([f6], [0], [1], [1], offs, np.array([0, 2], np.uint64), [0, flen - 1], [1, 1], [0, 0])
        e = dict(zip(ffold_ref.NAMES, ends))
        for g in range(2):
            a = int(e["nt_start"][g])
            assert 0 <= a and a + 3 <= L
            codon = contig[a:a + 3]
            res = translate_ref.frame(translate_ref.reverse_complement(codon) if reverse else codon, 0)
            assert res == frames[f6][(0, flen - 1)[g]:(0, flen - 1)[g] + 1]


def test_frame_chain_rows_on_hand_made_arrays():
    qid, tid, isect, nw, offs, row_offs, cols = hand_case()
    n = len(cols[0])
    hits, fold = ffold_ref.fold(qid, tid, isect, nw, offs, row_offs, *cols, score=np.ones(n, np.int64), identities=np.zeros(n, np.uint32),
                                aln_length=np.zeros(n, np.uint32))
    n_rows = len(hits[0])
    # a hand-made chain over the 7 folded rows: row 1 (record 0 +, tid 5) chains its regions 0 and 2 (frames 0 and 2), row 3
    # (record 0 -, tid 5) its regions 6 and 7 (frames 3 and 4), row 6 (record 3 -, tid 1) its region 9; the others have none
    z = lambda dt: np.zeros(n_rows, dt)  # noqa: E731
    chain = [np.array([0, 0, 2, 2, 4, 4, 4, 5], np.uint64), np.array([0, 2, 6, 7, 9], np.uint32), np.zeros(n, np.int64), np.zeros(n, np.uint32),
             z(np.int64)] + [z(np.uint32) for _ in range(6)] + [z(np.uint64), z(np.uint64), z(np.float64)]
    for r, (score, qs, ql, ts, tl, ident, alen) in {1: (50, 0, 29, 3, 69, 18, 20), 3: (70, 0, 28, 0, 30, 0, 0), 6: (9, 22, 9, 0, 9, 3, 3)}.items():
        chain[4][r], chain[5][r], chain[6][r], chain[7][r], chain[8][r], chain[11][r], chain[12][r] = score, qs, ql, ts, tl, ident, alen
    nt_recs = [(f"contig{i}", b"A" * L) for i, L in enumerate(LENGTHS)]
    t_recs = [(f"prot{i}", b"M") for i in range(8)]
    rows = wire.frame_chain_rows(nt_recs, t_recs, hits, fold, chain)
    assert [(r["query_name"], r["strand"], r["match_name"]) for r in rows] == [("contig0", "+", "prot5"), ("contig0", "-", "prot5"), ("contig3", "-", "prot1")]
    plus, minus, last = rows
    assert (plus["nt_start"], plus["nt_end"], plus["t_start"], plus["t_end"]) == (0, 29, 1, 24)
    assert (plus["frames"], plus["n_frameshifts"], plus["n_alns"], plus["chain_score"]) == ("+1,+3", 1, 2, 50)
    assert (plus["identities"], plus["aln_length"], plus["pident"], plus["intersect_hashes"]) == (18, 20, "90.0", 6)
    assert (minus["nt_start"], minus["nt_end"], minus["t_start"], minus["t_end"]) == (2, 30, 0, 10)  # L - (0 + 28), L - 0
    assert (minus["frames"], minus["n_frameshifts"], minus["pident"], minus["intersect_hashes"]) == ("-1,-2", 1, "NaN", 15)
    assert (last["nt_start"], last["nt_end"], last["frames"], last["n_frameshifts"], last["n_alns"]) == (0, 9, "-2", 0, 1)  # 31 - (22 + 9), 31 - 22
    assert list(plus) == ["query_name", "strand", "match_name", "nt_start", "nt_end", "t_start", "t_end", "chain_score", "n_alns", "frames",
                          "n_frameshifts", "identities", "aln_length", "pident", "intersect_hashes"]
    assert wire.frame_chain_rows(nt_recs, t_recs, hits, fold, chain, keep_rows=[3, 5]) == [minus]
    with pytest.raises(ValueError):
        wire.frame_chain_rows(nt_recs, t_recs, [h[:-1] for h in hits], fold, chain)


def test_prototypes_match_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ks_ffold_[a-z0-9_]+|ks_frames_fold_device|ks_r(?:scores|aligns)_fold_frames)\s*\(", header)))
    assert len(names) == 3 + 3 + 12 + 2, names
    for name in names:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    import ctypes as C
    assert C.sizeof(_lib.ks_ffold_opts) == 16 and _lib.KS_FFOLD_NONE == 0xFFFFFFFF
    assert _lib.SIGNATURES["ks_frames_fold_device"][1][3] is C.c_uint32 and _lib.SIGNATURES["ks_frames_fold_device"][1][12] is C.c_uint64


def test_the_python_object_is_a_column_table():
    """FrameFold is found by the walk of tests/test_columns_cpu.py, which then holds its table against the header."""
    assert issubclass(engine.FrameFold, engine._Columns) and engine.FrameFold._PREFIX == "ffold"
    assert engine.FrameFold._COLUMNS == ffold_ref.NAMES
    assert [np.dtype(dt) for _, dt, _ in engine.FrameFold._TABLE] == [np.dtype(d) for d in ffold_ref.DTYPES]
    for fn in ("fold_frames", "fold_frames_device", "chain_frames"):
        assert callable(getattr(engine.Context, fn))
