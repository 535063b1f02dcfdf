"""No GPU: the host restatement of the translated sketch (tests/translate_ref.py) on answers written out by hand, its union by
group against a dict-based union, the round trip through reverse_translate on the 25 BCL2 proteins, and its composition with the
oracle's protein sketch: the frames of a gene, unioned, hold the sketch of the protein the gene encodes."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import translate_ref as tr  # noqa: E402

from oracle import oracle  # noqa: E402


def test_table():
    assert len(tr.TABLE) == 64 and tr.TABLE.count("*") == 3
    assert sorted(set(tr.TABLE) - {"*"}) == sorted("ACDEFGHIKLMNPQRSTVWY")
    assert sum(len(tr.codons_of(r)) for r in set(tr.TABLE)) == 64


def test_known_codons():
    one = lambda nt: tr.translate6([nt])[0]  # noqa: E731  forward frame 0
    assert one(b"ATG") == b"M" and one(b"TGG") == b"W"
    assert one(b"TAA") == one(b"TAG") == one(b"TGA") == b"*"
    assert tr.translate6([b"atg"]) == tr.translate6([b"ATG"])
    assert one(b"ANG") == b"X" and one(b"AUG") == b"X"
    assert one(b"A-G") == b"X" and one(bytes([0x41, 0xd4, 0x47])) == b"X"  # 0xd4 is not 'T' with a bit set


def test_six_frames_of_a_hexamer():
    # ATGGCC; its reverse complement is GGCCAT
    assert tr.reverse_complement(b"ATGGCC") == b"GGCCAT"
    assert tr.translate6([b"ATGGCC"]) == [b"MA", b"W", b"G", b"GH", b"A", b"P"]
    # stops and invalid codons are residues: nothing is skipped, nothing cuts the frame
    assert tr.translate6([b"ATGTAAGCCNNNATG"])[0] == b"M*AXM"
    # the complement of a byte that is no base is the byte itself, and its codon is X on both strands
    assert tr.translate6([b"ATNGCC"])[3] == b"GX"


def test_frame_lengths():
    want = {0: (0, 0, 0), 1: (0, 0, 0), 2: (0, 0, 0), 3: (1, 0, 0), 4: (1, 1, 0), 5: (1, 1, 1), 6: (2, 1, 1), 7: (2, 2, 1), 8: (2, 2, 2)}
    for n, lens in want.items():
        fr = tr.translate6([b"A" * n])
        assert tuple(len(x) for x in fr[:3]) == lens == tuple(len(x) for x in fr[3:])
        assert lens == tuple(tr.frame_len(n, f) for f in range(3))
    assert tr.translate6([]) == [] and tr.translate6([b"", b"AC"]) == [b""] * 12


def test_round_trip(bcl2_records):
    rng = np.random.default_rng(5)
    assert len(bcl2_records) == 25
    for _, p in bcl2_records:
        nt = tr.reverse_translate(p, rng)
        assert len(nt) == 3 * len(p)
        fr = tr.translate6([nt])
        assert fr[0] == p
        # the reverse complement of the gene carries the protein in reverse frame 0, and its own reverse frames are the gene's forward ones
        rc = tr.translate6([tr.reverse_complement(nt)])
        assert rc[3:] == fr[:3] and rc[:3] == fr[3:]


def _dict_union(offsets, hashes, abunds, go):
    out = []
    for g in range(len(go) - 1):
        d = collections.defaultdict(int)
        for s in range(go[g], go[g + 1]):
            for j in range(int(offsets[s]), int(offsets[s + 1])):
                d[int(hashes[j])] += int(abunds[j])
        out.append(sorted((h, min(a, 2 ** 32 - 1)) for h, a in d.items()))
    return out


def test_union_groups_against_a_dict():
    rng = np.random.default_rng(8)
    for trial in range(40):
        n = int(rng.integers(0, 12))
        sk = [np.unique(rng.integers(1, 30, size=int(rng.integers(0, 9))).astype(np.uint64)) for _ in range(n)]
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in sk])]).astype(np.uint64)
        hashes = np.concatenate(sk).astype(np.uint64) if n else np.zeros(0, np.uint64)
        big = trial % 4 == 0
        abunds = rng.integers(1, 2 ** 32 if big else 5, size=len(hashes)).astype(np.uint32)
        n_groups = int(rng.integers(0 if n == 0 else 1, 6))
        go = np.sort(np.concatenate([[0, n], rng.integers(0, n + 1, size=max(n_groups - 1, 0))])).tolist() if n_groups else [0]
        if n_groups == 0 and n:
            continue
        o, h, a = tr.union_groups(offsets, hashes, abunds, go)
        want = _dict_union(offsets, hashes, abunds, go)
        assert o.dtype == np.uint64 and h.dtype == np.uint64 and a.dtype == np.uint32 and len(o) == len(go)
        for g, w in enumerate(want):
            got = list(zip(h[int(o[g]):int(o[g + 1])].tolist(), a[int(o[g]):int(o[g + 1])].tolist()))
            assert got == w
    # saturation, written out: 2^31 + 2^31 does not fit
    o, h, a = tr.union_groups([0, 1, 2, 3], [7, 7, 9], [2 ** 31, 2 ** 31, 3], [0, 2, 3])
    assert o.tolist() == [0, 1, 2] and h.tolist() == [7, 9] and a.tolist() == [2 ** 32 - 1, 3]
    o, h, a = tr.union_groups([0], [], [], [0])
    assert o.tolist() == [0] and len(h) == 0 and len(a) == 0


def test_frames_of_a_gene_hold_the_sketch_of_its_protein(bcl2_records):
    """hp k=24 scaled=5: the oracle-sketched frames of reverse-translated BCL2, unioned per record, hold every hash of the oracle
    sketch of the protein itself, with at least its abundance (frame 0 IS the protein; the other five only add)."""
    k, scaled, mol = 24, 5, "hp"
    rng = np.random.default_rng(6)
    prots = [p for _, p in bcl2_records]
    genes = [tr.reverse_translate(p, rng) for p in prots]
    fo, fh, fa = oracle.sketch_batch(*tr.pack(tr.translate6(genes)), k, scaled, mol)
    uo, uh, ua = tr.union_groups(fo, fh, fa, 6 * np.arange(len(genes) + 1))
    po, ph, pa = oracle.sketch_batch(*oracle.pack(prots), k, scaled, mol)
    assert len(ph) > 0
    for i in range(len(prots)):
        have = dict(zip(uh[int(uo[i]):int(uo[i + 1])].tolist(), ua[int(uo[i]):int(uo[i + 1])].tolist()))
        for h, a in zip(ph[int(po[i]):int(po[i + 1])].tolist(), pa[int(po[i]):int(po[i + 1])].tolist()):
            assert have.get(h, 0) >= a
