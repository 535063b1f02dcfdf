"""No GPU: the host restatement of the low-complexity mask (tests/mask_ref.py) on the known answers of the rule, against a brute-force
second reading of the definition, the committed table against its formula, and on the BCL2 / model-organism golden file the
conditions the GPU test relies on (they were measured for the rule, so they hold for the reference alone)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as mr  # noqa: E402

from oracle import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_committed_table_is_the_formula():
    assert list(mr.T_COMMITTED) == mr.table(mr.W_MAX) and len(mr.T_COMMITTED) == mr.W_MAX + 1 >= 33
    assert list(mr.T_COMMITTED[:13]) == [0, 0, 131072, 311616, 524288, 760849, 1016449, 1287880, 1572864, 1869698, 2177059, 2493890, 2819329]
    # ... and the library's literal is the same list of numbers
    src = open(os.path.join(ROOT, "kmerseek_amd", "csrc", "ks_mask.hip")).read()
    m = re.search(r"mk_T\[KS_MASK_MAX_WINDOW \+ 1\] = \{([^}]*)\}", src)
    assert m and [int(x) for x in m.group(1).replace("\n", " ").split(",")] == list(mr.T_COMMITTED)
    hdr = open(os.path.join(ROOT, "include", "kmerseek_amd.h")).read()
    assert re.search(r"#define KS_MASK_MAX_WINDOW (\d+)", hdr).group(1) == str(mr.W_MAX)


def test_default_thresholds():
    W, k1, k2 = mr.DEFAULTS
    assert (mr.threshold(k1, W), mr.threshold(k2, W)) == (1730150, 1966080)
    assert mr.complexity(b"AAACCCDDEEGG", 0, 12) == 2819329 - 2 * 311616 - 3 * 131072  # 2.24 bits: between k1 and k2
    assert mr.threshold(k1, W) < mr.complexity(b"AAACCCDDEEGG", 0, 12) <= mr.threshold(k2, W)
    assert mr.complexity(b"AAACCCDDDEEE", 0, 12) == 2819329 - 4 * 311616 <= mr.threshold(k1, W)  # 2 bits
    assert mr.complexity(b"aAaAaAaAaAaA", 0, 12) == 0 and mr.cls(ord("*")) == 26 and mr.cls(ord("-")) == mr.cls(0x80) == mr.cls(ord("1")) == 27


KNOWN = [
    (b"AAAAAAAAAAAA", "x" * 12),
    (b"AAAAAAAAAAA", "." * 11),
    (b"AAACCCDDEEGG", "." * 12),
    (b"AAACCCDDDEEE", "x" * 12),
    (b"MKTLWVHNAAACCCDDEEGGAAACCCDDDEEEQRSTVWYFHIKLMN", "......xxxxxxxxxxxxxxxxxxxxxxxxxxxxx..........."),
    (b"MKTLWVHNQRSAAACCCDDEEGGPFYWHIKLMNQRSTV", "." * 38),
]


@pytest.mark.parametrize("seq,want", KNOWN)
def test_known_answers(seq, want):
    assert len(seq) == len(want)
    assert mr.show(mr.mask_record(seq)) == want == mr.show(mr.mask_record_brute(seq))


def test_known_segments():
    m = mr.mask_record(KNOWN[4][0])
    assert mr.segments_of(m, 1) == [(0, 6), (35, 46)]
    assert mr.segments_of(m, 7) == [(35, 46)] and mr.segments_of(m, 11) == [(35, 46)] and mr.segments_of(m, 12) == []
    assert mr.segments_of(mr.mask_record(KNOWN[0][0]), 1) == [] and mr.segments_of([], 1) == []
    # the k2 stretch of the last known answer is there, it just has no trigger
    lo1, lo2 = mr.flags(KNOWN[5][0], 12, 2200, 2500)
    assert any(lo2) and not any(lo1)


def test_mask_does_not_cross_records():
    a, b = b"MKTLWVHNQRSTAAAAAA", b"AAAAAAMKTLWVHNQRST"
    m, counts = mr.mask_batch([a, b])
    assert counts.tolist() == [0, 0] and not m.any()
    assert mr.mask_record(a + b)[12:24] == [1] * 12  # joined they would be masked


def test_reference_agrees_with_brute_force():
    rng = np.random.default_rng(5)
    for t in range(120):
        n = int(rng.integers(0, 70))
        alpha = list(b"ACDE") if t % 3 else list(b"ACDEFGHIKLMNPQRSTVWY")
        seq = bytes(rng.choice(alpha, size=n).tolist()) if n else b""
        if t % 4 == 0 and n > 20:
            seq = seq[:8] + bytes([seq[8]]) * 14 + seq[22:]
        for W, k1, k2 in ((12, 2200, 2500), (2, 0, 0), (2, 0, 1000), (5, 1000, 1800), (31, 3000, 3400), (32, 2900, 2900)):
            assert mr.mask_record(seq, W, k1, k2) == mr.mask_record_brute(seq, W, k1, k2), (seq, W, k1, k2)


def test_split_layout():
    recs = [KNOWN[4][0], b"", KNOWN[0][0], b"mktlwvhn"]
    rec_of, start_of, offs, res, groups, pieces = mr.split_batch(recs, 1)
    assert rec_of.tolist() == [0, 0, 3] and start_of.tolist() == [0, 35, 0] and groups.tolist() == [0, 2, 2, 2, 3]
    assert offs.tolist() == [0, 6, 17, 25] and bytes(res) == b"MKTLWV" + b"QRSTVWYFHIKLMN"[3:] + b"mktlwvhn" and len(pieces) == 3


def test_golden_file_has_what_the_gpu_test_relies_on():
    recs = [r for _, r in oracle.read_fasta(os.path.join(GOLDEN, "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"))]
    k = 10
    masks = [mr.mask_record(r) for r in recs]
    n_seg = [len(mr.segments_of(m, k)) for m in masks]
    share = sum(sum(m) for m in masks) / sum(len(m) for m in masks)
    print(f"{len(recs)} records, masked share {share:.4f}, most segments {max(n_seg)}, records without a segment {n_seg.count(0)}")
    assert max(n_seg) > 8 and n_seg.count(0) > 0 and 0 < share < 1
