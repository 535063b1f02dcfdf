"""CPU restatement of the translated sketch (include/kmerseek_amd.h): six-frame translation, the union of sketches by group and
a reverse translation that makes test DNA from proteins.  Pure Python / numpy, written from the semantics in the header, with no
code shared with the library: the GPU tests hold the library against this plus the oracle's protein sketch."""
from typing import List, Sequence, Tuple

import numpy as np

TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"  # the standard code, NCBI table 1; bases in TCAG order
BASES = b"TCAG"
CODE = {b: i for i, b in enumerate(BASES)}
COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


def upper(nt: bytes) -> bytes:
    """ASCII upper-casing: only a-z change (bytes.upper would do the same; spelled out because bytes >= 0x80 must stay)"""
    return bytes(b - 32 if 97 <= b <= 122 else b for b in nt)


def codon(b1: int, b2: int, b3: int) -> int:
    if b1 in CODE and b2 in CODE and b3 in CODE:
        return ord(TABLE[16 * CODE[b1] + 4 * CODE[b2] + CODE[b3]])
    return ord("X")


def reverse_complement(nt: bytes) -> bytes:
    return bytes(COMPLEMENT.get(b, b) for b in reversed(nt))


def frame(nt: bytes, f: int) -> bytes:
    """the codons of nt[f:], a trailing partial codon dropped; nt already upper-cased"""
    return bytes(codon(nt[i], nt[i + 1], nt[i + 2]) for i in range(f, len(nt) - 2, 3))


def frame_len(n_bases: int, f: int) -> int:
    return max(0, (n_bases - f) // 3)


def translate6(records: Sequence[bytes]) -> List[bytes]:
    """6 sequences per record: 6s + f the forward frames, 6s + 3 + f the frames of the reverse complement"""
    out = []
    for rec in records:
        nt = upper(bytes(rec))
        rc = reverse_complement(nt)
        out.extend(frame(nt, f) for f in range(3))
        out.extend(frame(rc, f) for f in range(3))
    return out


def pack(seqs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    offs = np.zeros(len(seqs) + 1, np.uint64)
    if len(seqs):
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


def union_groups(offsets, hashes, abunds, group_offsets) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """sketch g = the ascending distinct hashes of the sketches [group_offsets[g], group_offsets[g + 1]), abundances summed per
    hash and saturating at 2^32 - 1 -> (offsets u64[n_groups + 1], hashes u64, abunds u32)"""
    offsets = np.asarray(offsets, np.uint64)
    hashes = np.asarray(hashes, np.uint64)
    abunds = np.asarray(abunds, np.uint32)
    go = [int(x) for x in group_offsets]
    assert go[0] == 0 and go[-1] == len(offsets) - 1 and all(a <= b for a, b in zip(go, go[1:]))
    out_off, out_h, out_a = [0], [], []
    for g in range(len(go) - 1):
        b, e = int(offsets[go[g]]), int(offsets[go[g + 1]])
        h, inv = np.unique(hashes[b:e], return_inverse=True)
        a = np.zeros(len(h), np.uint64)
        np.add.at(a, inv.reshape(-1), abunds[b:e].astype(np.uint64))  # (exact: fewer than 2^32 addends below 2^32)
        out_h.append(h)
        out_a.append(np.minimum(a, np.uint64(0xffffffff)).astype(np.uint32))
        out_off.append(out_off[-1] + len(h))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    return np.array(out_off, np.uint64), cat(out_h, np.uint64), cat(out_a, np.uint32)


def codons_of(residue: str) -> List[bytes]:
    return [bytes((BASES[i >> 4], BASES[(i >> 2) & 3], BASES[i & 3])) for i, r in enumerate(TABLE) if r == residue]


def reverse_translate(protein: bytes, rng) -> bytes:
    """DNA whose forward frame 0 is `protein`: for every residue any of its codons, picked by `rng` (numpy Generator).  A residue
    the table does not make (X, B, Z, U, ...) has no codon: ValueError."""
    out = []
    for r in bytes(protein):
        cs = codons_of(chr(r))
        if not cs:
            raise ValueError(f"residue {chr(r)!r} has no codon in the standard code")
        out.append(cs[int(rng.integers(len(cs)))])
    return b"".join(out)
