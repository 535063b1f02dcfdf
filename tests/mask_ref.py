"""CPU restatement of the low-complexity mask, the split into segments and the masked sketch (include/kmerseek_amd.h): plain loops
over the definition, written from the header with no code shared with the library.  The GPU tests hold the library against this
plus the oracle's sketch.  The rule is the project's own (the first stage of SEG, in integers); no parity with NCBI seg is claimed."""
import math
from typing import List, Sequence, Tuple

import numpy as np

import translate_ref as tr

W_MAX = 32
# the table the library commits as a literal (kmerseek_amd/csrc/ks_mask.hip: mk_T); table() recomputes it
T_COMMITTED = (0, 0, 131072, 311616, 524288, 760849, 1016449, 1287880, 1572864, 1869698, 2177059, 2493890, 2819329, 3152656, 3493263, 3840630,
               4194304, 4553891, 4919044, 5289451, 5664838, 6044953, 6429573, 6818492, 7211522, 7608494, 8009248, 8413640, 8821535, 9232807,
               9647339, 10065024, 10485760)
DEFAULTS = (12, 2200, 2500)


def table(n: int = W_MAX) -> List[int]:
    """T[c] = floor(c log2(c) 65536 + 0.5), T[0] = 0"""
    return [0] + [int(math.floor(c * math.log2(c) * 65536 + 0.5)) for c in range(1, n + 1)]


def cls(b: int) -> int:
    """28 classes: the letters without case, '*', everything else"""
    if 97 <= b <= 122:
        b -= 32
    if 65 <= b <= 90:
        return b - 65
    return 26 if b == 42 else 27


def threshold(k_millibits: int, W: int) -> int:
    return k_millibits * W * 65536 // 1000


def complexity(rec: bytes, p: int, W: int, T=T_COMMITTED) -> int:
    """e(p) of the window rec[p : p + W] (valid: p + W <= len(rec))"""
    counts = {}
    for b in rec[p:p + W]:
        counts[cls(b)] = counts.get(cls(b), 0) + 1
    return T[W] - sum(T[c] for c in counts.values())


def flags(rec: bytes, W: int, k1: int, k2: int) -> Tuple[List[bool], List[bool]]:
    """(lo1, lo2) per window start of one record; the last W - 1 starts are invalid, so neither"""
    n = len(rec)
    lo1, lo2 = [False] * n, [False] * n
    for p in range(0, n - W + 1):
        e = complexity(rec, p, W)
        lo1[p], lo2[p] = e <= threshold(k1, W), e <= threshold(k2, W)
    return lo1, lo2


def runs(lo2: Sequence[bool]) -> List[Tuple[int, int]]:
    """the maximal stretches [i, j) of consecutive starts with lo2"""
    out, p, n = [], 0, len(lo2)
    while p < n:
        if lo2[p]:
            q = p
            while q < n and lo2[q]:
                q += 1
            out.append((p, q))
            p = q
        else:
            p += 1
    return out


def mask_record(rec: bytes, W: int = 12, k1: int = 2200, k2: int = 2500) -> List[int]:
    assert 2 <= W <= W_MAX and k2 >= k1
    lo1, lo2 = flags(rec, W, k1, k2)
    m = [0] * len(rec)
    for i, j in runs(lo2):
        if any(lo1[i:j]):  # hot
            for p in range(i, j - 1 + W):
                m[p] = 1
    return m


def mask_record_brute(rec: bytes, W: int = 12, k1: int = 2200, k2: int = 2500) -> List[int]:
    """the same a second way: residue p is masked iff some lo2 window that covers it is joined, through lo2 windows only, to a lo1 one"""
    n = len(rec)
    T = table(W)
    valid = lambda q: 0 <= q and q + W <= n  # noqa: E731
    e = {q: complexity(rec, q, W, T) for q in range(n) if valid(q)}
    is2 = lambda q: valid(q) and e[q] <= threshold(k2, W)  # noqa: E731
    is1 = lambda q: valid(q) and e[q] <= threshold(k1, W)  # noqa: E731
    m = []
    for p in range(n):
        hit = 0
        for q in range(p - W + 1, p + 1):
            if not is2(q):
                continue
            a = q
            while is2(a - 1):
                a -= 1
            b = q
            while is2(b + 1):
                b += 1
            if any(is1(x) for x in range(a, b + 1)):
                hit = 1
        m.append(hit)
    return m


def mask_batch(records: Sequence[bytes], W: int = 12, k1: int = 2200, k2: int = 2500) -> Tuple[np.ndarray, np.ndarray]:
    """(mask u8 over the concatenated residues, masked residues u32 per record)"""
    ms = [mask_record(bytes(r), W, k1, k2) for r in records]
    flat = [x for m in ms for x in m]
    return np.array(flat, np.uint8), np.array([sum(m) for m in ms], np.uint32)


def segments_of(m: Sequence[int], min_len: int = 1) -> List[Tuple[int, int]]:
    """the maximal stretches [a, b) of unmasked residues of one record with b - a >= min_len, in order"""
    min_len = max(min_len, 1)
    out, p, n = [], 0, len(m)
    while p < n:
        if not m[p]:
            q = p
            while q < n and not m[q]:
                q += 1
            if q - p >= min_len:
                out.append((p, q))
            p = q
        else:
            p += 1
    return out


def split_batch(records: Sequence[bytes], min_len: int, W: int = 12, k1: int = 2200, k2: int = 2500):
    """-> (seg_record u32, seg_start u32, seg_offsets u64[n_segs + 1], residues u8, group_offsets u32[n_records + 1], pieces)"""
    rec_of, start_of, pieces, groups = [], [], [], [0]
    for r, rec in enumerate(records):
        rec = bytes(rec)
        for a, b in segments_of(mask_record(rec, W, k1, k2), min_len):
            rec_of.append(r); start_of.append(a); pieces.append(rec[a:b])
        groups.append(len(pieces))
    res, offs = tr.pack(pieces)
    return (np.array(rec_of, np.uint32), np.array(start_of, np.uint32), offs, res, np.array(groups, np.uint32), pieces)


def masked_sketch(records: Sequence[bytes], k: int, scaled: int, mol: str, W: int = 12, k1: int = 2200, k2: int = 2500):
    """-> (offsets u64[n + 1], hashes u64, abunds u32, n_windows): the oracle's sketch of the segments at min_len = k, folded by record"""
    from oracle import oracle
    _, _, offs, res, groups, pieces = split_batch(records, k, W, k1, k2)
    so, sh, sa = oracle.sketch_batch(res, offs, k, scaled, mol)
    return tr.union_groups(so, sh, sa, groups) + (sum(len(p) - k + 1 for p in pieces),)


def masked_positions(records: Sequence[bytes], k: int, scaled: int, mol: str, W: int = 12, k1: int = 2200, k2: int = 2500):
    """-> (seq u32, start u32, hash u64) of every kept window without a masked residue, ordered by (seq, start): the oracle's
    k-mer positions of every segment, carried back to the record"""
    from oracle import oracle
    rec_of, start_of, _, _, _, pieces = split_batch(records, k, W, k1, k2)
    seq, start, h = [], [], []
    for r, a, piece in zip(rec_of.tolist(), start_of.tolist(), pieces):
        mins, _ = oracle.sketch_protein(piece, k, scaled, mol)
        st, hs = oracle.kmer_positions(piece, k, mol, mins)
        seq.extend([r] * len(st)); start.extend((st.astype(np.int64) + a).tolist()); h.extend(hs.tolist())
    return np.array(seq, np.uint32), np.array(start, np.uint32), np.array(h, np.uint64)


def show(m: Sequence[int]) -> str:
    return "".join("x" if v else "." for v in m)
