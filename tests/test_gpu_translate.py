"""GPU: the translated sketch — ks_translate6_device, ks_sketch_translated*, ks_sketches_union_groups.

Everything is bytes and integers, every check is exact equality, and every comparison is against tests/translate_ref.py plus the
oracle's protein sketch, never against the library itself.  The batch is the smallest that can still go wrong: records shorter
than a codon, hundreds of short records in one chunk of the translate kernel, record ends on either side of the first three
chunk boundaries, a record that spans chunks with the codon phase shifting at each boundary, lower case and bytes that are no
base, a palindrome, and for the sketch frames on either side of the sketch kernel's one-tile limit, a long record and a poly-A
one whose windows all share a hash.  The union runs with KS_DEBUG_UNION_PATH unset, 1 (rank) and 2 (sort): same result."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import translate_ref as tr  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402
from oracle import oracle  # noqa: E402

KNOB = "KS_DEBUG_UNION_PATH"
PATHS = (None, "1", "2")
PARAMS = (("protein", 7, 1), ("dayhoff", 16, 5), ("hp", 24, 5))


def _set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, path)


def _dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist()) if n else b""


@functools.lru_cache(maxsize=None)
def _records(for_sketch=False):
    """the batch of the module docstring; built once"""
    chunk = int(_lib.load().ks_debug_translate_chunk())
    assert chunk >= 256
    rng = np.random.default_rng(31)
    recs, total = [], 0

    def add(r):
        nonlocal total
        recs.append(r)
        total += len(r)

    for k in (1, 2, 3):  # ends at k * chunk - 1, k * chunk and k * chunk + 1; the next record begins right behind
        add(_dna(rng, k * chunk - 1 - 37 - total))
        add(_dna(rng, 37))
        assert total == k * chunk - 1
        add(_dna(rng, 1))
        add(_dna(rng, 1))
        assert total == k * chunk + 1
    for n in (0, 1, 2, 3, 4, 5, 20, 21, 22, 23):
        add(_dna(rng, n))
    for n in rng.integers(1, 41, size=300).tolist():  # many records in one chunk
        add(_dna(rng, n))
    add(_dna(rng, 3 * chunk + 7))  # spans chunks; chunk is no multiple of 3, or the + 7 shifts the phase at the record's end
    add(b"acgtacgtnnacgtAcGt" + _dna(rng, 30).lower())
    add(b"ACGTNACGTUACGT-ACGT" + bytes([0x41, 0xd4, 0x47, 0x80, 0xff, 0x43]) + b"RYKMSWBDHVN" + _dna(rng, 25))
    half = _dna(rng, 33)
    add(half + tr.reverse_complement(half))  # a palindrome: equal to its reverse complement
    assert recs[-1] == tr.reverse_complement(recs[-1])
    if for_sketch:
        add(_dna(rng, 12243))  # frames of 4,081 / 4,080 / 4,080 residues: either side of the sketch kernel's one-tile limit
        add(_dna(rng, 40000))
        add(b"A" * 3000)       # every window of a strand has the same hash
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def _frames(for_sketch=False):
    return tuple(tr.translate6(_records(for_sketch)))


@functools.lru_cache(maxsize=None)
def _want_sketch(mol, k, scaled):
    frames = _frames(True)
    fo, fh, fa = oracle.sketch_batch(*tr.pack(frames), k, scaled, mol)
    n = len(frames) // 6
    return tr.union_groups(fo, fh, fa, 6 * np.arange(n + 1)) + (sum(max(0, len(f) - k + 1) for f in frames),)


def _check_sketches(sk, want):
    o, h, a = sk.to_host()
    assert sk.n_seqs == len(want[0]) - 1 and sk.n_hashes == len(want[1])
    assert np.array_equal(o, want[0]) and np.array_equal(h, want[1]) and np.array_equal(a, want[2])
    assert o.dtype == np.uint64 and h.dtype == np.uint64 and a.dtype == np.uint32


# ---- translate6 -----------------------------------------------------------------------------------------------------------------
def _translate_and_check(c, records):
    nt, offs = tr.pack(records)
    want_res, want_off = tr.pack(tr.translate6(records))
    frames, foff, n_res = c.translate6(nt, offs)
    assert n_res == len(want_res) <= 2 * len(nt)
    assert np.array_equal(foff.to_host(np.uint64, 6 * len(records) + 1), want_off)
    assert np.array_equal(frames.to_host(np.uint8, n_res), want_res)
    frames.free(); foff.free()


def test_translate6_bytes_and_offsets():
    with ks.Context(0) as c:
        recs = _records()
        lens = [len(r) for r in recs]
        assert {0, 1, 2, 3, 4, 5, 20, 21, 22, 23} <= set(lens) and sum(1 for n in lens if 1 <= n <= 40) >= 300
        _translate_and_check(c, recs)
        _translate_and_check(c, [])               # an empty batch
        _translate_and_check(c, [b"", b"", b""])  # an all-empty batch
        _translate_and_check(c, [b"ATGGCC"])
        assert int(_lib.load().ks_translate6_bound(1000)) == 2000


def test_translate6_output_feeds_the_device_sketch():
    """the frames are an ordinary residue batch: ks_sketch_batch_device takes the two buffers as they are"""
    with ks.Context(0) as c:
        recs = _records()
        frames, foff, n_res = c.translate6(*tr.pack(recs))
        sk = c.sketch_batch_device(frames.ptr, foff.ptr, 6 * len(recs), n_res, 7, 1, "protein")
        _check_sketches(sk, oracle.sketch_batch(*tr.pack(_frames()), 7, 1, "protein"))


# ---- sketch_translated against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mol,k,scaled", PARAMS)
def test_sketch_translated_matches_the_oracle(monkeypatch, mol, k, scaled, path):
    want = _want_sketch(mol, k, scaled)
    if (mol, k, scaled) == ("protein", 7, 1):  # the poly-A record: one hash per strand, abundances in the thousands
        lo, hi = int(want[0][-2]), int(want[0][-1])
        assert hi - lo == 2 and sorted(want[2][lo:hi].tolist()) == [2980, 2980]
    with ks.Context(0, follow_debug_env=True) as c:
        _set_path(monkeypatch, path)
        nt, offs = tr.pack(_records(True))
        sk = c.sketch_translated(nt, offs, k, scaled, mol)
        _check_sketches(sk, want[:3])
        assert sk.n_windows == want[3] and not sk.has_postings
        # the device-pointer form: measured, and with an exact bound on the longest record
        d_nt, d_off = c.to_device(nt), c.to_device(offs)
        for hint in (0, max(len(r) for r in _records(True))):
            sk = c.sketch_translated_device(d_nt.ptr, d_off.ptr, len(offs) - 1, len(nt), k, scaled, mol, max_seq_len=hint)
            _check_sketches(sk, want[:3])
            assert sk.n_windows == want[3]


# ---- union_groups on crafted sets ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crafted():
    """-> (offsets, hashes, abunds, group_offsets): group sizes [0, 1, 2, 6, 0, 7, R, R + 1, 300]"""
    R = int(_lib.load().ks_debug_union_rank_max())
    rng = np.random.default_rng(41)
    rand = lambda n, hi: np.unique(rng.integers(1, hi, size=n).astype(np.uint64))  # noqa: E731
    A = rand(40, 200)
    members = [[(A, None)]]
    sat = np.array([7, 11, 500], np.uint64)
    members.append([(sat, np.array([2 ** 31, 5, 1], np.uint32)), (sat, np.array([2 ** 31, 6, 2 ** 32 - 1], np.uint32))])  # identical; 7 and 500 saturate
    members.append([(np.zeros(0, np.uint64), None), (A, None), (A, None), (A + np.uint64(1000), None), (A + np.uint64(1), None),
                    (np.zeros(0, np.uint64), None)])  # empty, identical, disjoint, interleaved, empty
    members.append([(rand(30, 60), None) for _ in range(7)])
    members.append([(rand(50, 300), None) for _ in range(R)])
    members.append([(rand(50, 300), None) for _ in range(R + 1)])
    members.append([(rand(int(rng.integers(0, 20)), 400), None) for _ in range(300)])
    sizes = [0, 1, 2, 6, 0, 7, R, R + 1, 300]
    it = iter(members)
    sk = []
    for s in sizes:
        if s:
            grp = next(it)
            assert len(grp) == s
            sk.extend(grp)
    offsets = np.concatenate([[0], np.cumsum([len(h) for h, _ in sk])]).astype(np.uint64)
    hashes = np.concatenate([h for h, _ in sk]).astype(np.uint64)
    abunds = np.concatenate([a if a is not None else rng.integers(1, 9, size=len(h)).astype(np.uint32) for h, a in sk]).astype(np.uint32)
    go = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return offsets, hashes, abunds, go


@pytest.mark.parametrize("path", PATHS)
def test_union_groups_crafted(monkeypatch, path):
    offsets, hashes, abunds, go = _crafted()
    want = tr.union_groups(offsets, hashes, abunds, go)
    lo = int(want[0][2])
    assert want[1][lo:lo + 3].tolist() == [7, 11, 500] and want[2][lo:lo + 3].tolist() == [2 ** 32 - 1, 11, 2 ** 32 - 1]
    with ks.Context(0, follow_debug_env=True) as c:
        S = c.sketches_from_host(offsets, hashes, abunds, 10, 1, "protein")
        _set_path(monkeypatch, path)
        U = S.union_groups(go)
        _check_sketches(U, want)
        assert U.n_windows == S.n_windows
        # every sketch a group of its own is a copy; one group of everything is what ks_sketches_union computes
        _check_sketches(S.union_groups(np.arange(len(offsets))), (offsets, hashes, abunds))
        _check_sketches(S.union_groups([0, len(offsets) - 1]), tr.union_groups(offsets, hashes, abunds, [0, len(offsets) - 1]))
        # n_groups = 0 on an empty set, and groups over a set without hashes
        E = c.sketches_from_host(np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), 10, 1, "protein")
        _check_sketches(E.union_groups([0]), (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32)))
        E3 = c.sketches_from_host(np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), 10, 1, "protein")
        _check_sketches(E3.union_groups([0, 1, 1, 3]), (np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32)))


@pytest.mark.parametrize("path", PATHS)
def test_union_groups_of_a_device_sketch_with_repeats(monkeypatch, path):
    """a set sketched by the device whose sequences repeat k-mers: its slots have gaps until the union makes it dense"""
    rng = np.random.default_rng(43)
    unit = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), size=23).tolist())
    seqs = [unit * int(n) + unit[:int(m)] for n, m in zip(rng.integers(1, 6, size=40), rng.integers(0, 23, size=40))] + [b"", b"AC"]
    res, offs = oracle.pack(seqs)
    go = [0, 0, 3, 4, 17, 17, 30, len(seqs)]
    so, sh, sa = oracle.sketch_batch(res, offs, 5, 1, "protein")
    assert sa.max() > 1
    with ks.Context(0, follow_debug_env=True) as c:
        _set_path(monkeypatch, path)
        _check_sketches(c.sketch_batch(res, offs, 5, 1, "protein").union_groups(go), tr.union_groups(so, sh, sa, go))


# ---- end to end: genes searched against their proteins ----------------------------------------------------------------------------
def test_translated_search_finds_the_proteins(bcl2_records, tmp_path):
    k, scaled, mol = 24, 5, "hp"
    rng = np.random.default_rng(6)
    prots = [p for _, p in bcl2_records]
    genes = [tr.reverse_translate(p, rng) for p in prots]
    genes = [tr.reverse_complement(g) if i % 2 else g for i, g in enumerate(genes)]
    to, tm, ta = oracle.sketch_batch(*oracle.pack(prots), k, scaled, mol)
    fo, fh, fa = oracle.sketch_batch(*tr.pack(tr.translate6(genes)), k, scaled, mol)
    qo, qm, qa = tr.union_groups(fo, fh, fa, 6 * np.arange(len(genes) + 1))
    with ks.Context(0) as c:
        Q = c.sketch_translated(*tr.pack(genes), k, scaled, mol)
        _check_sketches(Q, (qo, qm, qa))
        T = c.sketch_batch(*oracle.pack(prots), k, scaled, mol)
        hits = c.search(c.index_build(T), Q)
        got = hits.to_host()
        rows = {(int(q), int(t)): int(n) for q, t, n in zip(got[0], got[1], got[2])}
        sizes = (to[1:] - to[:-1]).astype(np.int64)
        assert (sizes > 0).sum() >= 20
        for i in range(len(prots)):
            if sizes[i]:
                assert rows.get((i, i)) == sizes[i]
        for g, w in zip(got, oracle.manysearch(qo, qm, to, tm, ta)):
            assert np.array_equal(g, w)
        # the same records through wire.sketch(translate=True): the .sig.zip reads back to the same arrays, under the same names
        fasta = tmp_path / "genes.fasta"
        fasta.write_text("".join(f">{n}\n{g.decode()}\n" for (n, _), g in zip(bcl2_records, genes)))
        names, o, m, a, kk, ss, mm = wire.read_sig_zip(wire.sketch(str(fasta), mol, k, scaled, ctx=c, translate=True))
        assert names == [n for n, _ in bcl2_records] and (kk, ss, mm) == (k, scaled, mol)
        assert np.array_equal(o, qo) and np.array_equal(m, qm) and np.array_equal(a, qa)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working():
    L = _lib.load()
    rng = np.random.default_rng(47)
    recs = [_dna(rng, 1000), _dna(rng, 90)]
    nt, offs = tr.pack(recs)
    with ks.Context(0) as c, ks.Context(0) as other:
        in_use = c.pool_stats()["bytes_in_use"]
        d_nt, d_off = c.to_device(nt), c.to_device(offs)
        frames, foff = c.to_device(np.zeros(2 * len(nt) + 32, np.uint8)), c.to_device(np.zeros(13, np.uint64))
        n_res = C.c_uint64(0)
        # a misaligned d_frames
        st = L.ks_translate6_device(c._h, d_nt._p, d_off._p, 2, len(nt), C.c_void_p(frames.ptr + 1), foff._p, C.byref(n_res))
        assert st == _lib.KS_ERR_INVALID_ARG and b"aligned" in L.ks_last_error(c._h)
        # the six frames of too many records for 32-bit sequence ids: refused before anything is read
        out = C.c_void_p()
        p = ks.make_params(7, 1, "protein")
        st = L.ks_sketch_translated_device(c._h, d_nt._p, d_off._p, 2 ** 32 // 6 + 1, len(nt), 0, C.byref(p), C.byref(out))
        assert st == _lib.KS_ERR_CAPACITY and not out.value
        # a max_seq_len hint of 10 against a 1,000-base record
        with pytest.raises(ks.KmerseekError) as e:
            c.sketch_translated_device(d_nt.ptr, d_off.ptr, 2, len(nt), 7, 1, "protein", max_seq_len=10)
        assert e.value.status == _lib.KS_ERR_INVALID_ARG
        # group offsets that do not start at 0, descend, or end before n_seqs
        S = c.sketch_translated(nt, offs, 7, 1, "protein")
        assert S.n_seqs == 2
        for bad in ([1, 2], [0, 2, 1, 2], [0, 1], [0, 3]):
            with pytest.raises(ks.KmerseekError) as e:
                S.union_groups(bad)
            assert e.value.status == _lib.KS_ERR_INVALID_ARG
        # an input of another context
        So = other.sketch_translated(nt, offs, 7, 1, "protein")
        go = (C.c_uint32 * 2)(0, 2)
        st = L.ks_sketches_union_groups(c._h, So._h, go, 1, C.byref(out))
        assert st == _lib.KS_ERR_INVALID_ARG and not out.value and b"another context" in L.ks_last_error(c._h)
        # the context still works, and gives back what it borrowed
        want = _ref_sketch(recs, 7, 1, "protein")
        _check_sketches(S, want)
        U = S.union_groups([0, 2])
        _check_sketches(U, tr.union_groups(*want, [0, 2]))
        T = c.sketch_translated_device(d_nt.ptr, d_off.ptr, 2, len(nt), 7, 1, "protein", max_seq_len=1000)
        _check_sketches(T, want)
        for x in (S, U, T, So, d_nt, d_off, frames, foff):
            x.free()
        assert c.pool_stats()["bytes_in_use"] == in_use


def _ref_sketch(records, k, scaled, mol):
    fo, fh, fa = oracle.sketch_batch(*tr.pack(tr.translate6(records)), k, scaled, mol)
    return tr.union_groups(fo, fh, fa, 6 * np.arange(len(records) + 1))
