"""GPU: low-complexity masking — ks_mask_*, ks_mask_split_device, ks_sketch_masked*, ks_kmer_positions_masked_device.

Everything is bytes and integers, every check is exact equality, and every comparison is against tests/mask_ref.py plus the
oracle's sketch, never against the library itself.  The batch is the smallest that can still go wrong: records of 0, 1, W - 1, W
and W + 1 residues for every window length tested, hundreds of short records in one chunk of the mask kernels, a low-complexity
run that ends at, one before and one after each of the first three chunk boundaries (three batches, shifted by one residue), a
run whose trigger window lies in another chunk than its far end, a homopolymer record over three chunks, a record that ends in a
low-complexity tail followed by one that begins with the same residues, a k2 stretch with no trigger, lower case and bytes that
are no letter, segments of k - 1, k and k + 1 residues for every k sketched, a record with more segments than the union's rank
path takes, and the 25 BCL2 proteins.  The union runs with KS_DEBUG_UNION_PATH unset, 1 (rank) and 2 (sort): same result."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as mr  # noqa: E402
import translate_ref as tr  # noqa: E402

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import _lib, wire  # noqa: E402
from oracle import oracle  # noqa: E402

KNOB = "KS_DEBUG_UNION_PATH"
PATHS = (None, "1", "2")
PARAMS = (("protein", 7, 1), ("dayhoff", 16, 5), ("hp", 24, 5))
KS = (7, 10, 16, 24)
WINDOWS = (2, 12, 32)
MASK_CASES = [(W, k1, k2) for W in WINDOWS for k1, k2 in ((2200, 2500), (0, 1000))]
AA = list(b"ACDEFGHIKLMNPQRSTVWY")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _prot(rng, n):
    return bytes(rng.choice(AA, size=n).tolist()) if n else b""


@functools.lru_cache(maxsize=None)
def _bcl2():
    return tuple(r for _, r in oracle.read_fasta(os.path.join(GOLDEN, "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz")))


@functools.lru_cache(maxsize=None)
def _records(shift=0):
    """the batch of the module docstring; the runs at the chunk boundaries end at k * chunk + shift"""
    L = _lib.load()
    chunk, R = int(L.ks_debug_mask_chunk()), int(L.ks_debug_union_rank_max())
    assert chunk >= 512 and R >= 1
    rng = np.random.default_rng(53)
    recs, total = [], 0

    def add(r):
        nonlocal total
        recs.append(bytes(r))
        total += len(r)

    for k in (1, 2, 3):  # a run of Q inside a record; what it masks (the reference says how far it reaches) ends at k * chunk + shift
        rec = _prot(rng, 40) + b"Q" * 20 + _prot(rng, 25)
        m = mr.mask_record(rec)
        end = max(i for i, v in enumerate(m) if v) + 1
        assert 60 <= end < len(rec) and not m[end]
        add(_prot(rng, k * chunk + shift - end - total))
        add(rec)
    # the trigger in chunk 3, the far end of its run in chunk 4: windows of (3, 3, 2, 2, 2) extend, (3, 3, 3, 3) triggers
    add(_prot(rng, 4 * chunk - 30 - 12 - total))
    add(b"AAACCCDDDEEE" + b"AAACCCDDEEGG" * 5 + _prot(rng, 20))
    far = recs[-1]
    assert total - len(far) + 12 < 4 * chunk < total - 20
    assert all(mr.mask_record(far)[:72]), "the run must reach from the trigger over the chunk boundary"
    add(b"A" * (2 * chunk + 100))  # a homopolymer over three chunks
    assert (total - len(recs[-1])) // chunk + 2 == (total - 1) // chunk
    for n in sorted({0, 1} | {W + d for W in WINDOWS for d in (-1, 0, 1)}):
        add(b"G" * n)
        add(_prot(rng, n))
    for i, n in enumerate(rng.integers(1, 41, size=300).tolist()):  # many records in one chunk, one in five a homopolymer
        add(b"S" * n if i % 5 == 0 else _prot(rng, n))
    add(_prot(rng, 30) + b"S" * 8)   # a low-complexity tail ...
    add(b"S" * 8 + _prot(rng, 30))   # ... and a head of the same residues: 16 together, 8 each
    add(_prot(rng, 30) + b"T" * 13)
    add(b"T" * 13 + _prot(rng, 30))
    add(b"MKTLWVHNQRSAAACCCDDEEGGPFYWHIKLMNQRSTV")  # a k2 stretch with no trigger
    add(b"mktlwvhnaaaaaaaaaaaaaaqrstvwyfhiklmn" + _prot(rng, 30).lower())
    add(b"MKT************LWVHN--------------QRSTXXXXXXXXXXXXXX" + bytes([0x80] * 14) + b"1234567890123" + bytes([0xff, 0x00, 0x41, 0xc1] * 4) + _prot(rng, 30))
    add(b"AaAaAaAaAaAaAa" + _prot(rng, 26) + b"a" * 6 + b"A" * 6)
    # segments of every length from 4 to 27 between two masked runs (the mask reaches into the filler: the lengths come out of
    # the reference, test_batch_holds_what_it_should looks for k - 1, k and k + 1)
    for n in range(12, 60, 2):
        add(b"W" * 14 + _prot(rng, n) + b"W" * 14 + _prot(rng, n + 1) + b"W" * 14)
    add((_prot(rng, 45) + b"P" * 14) * (R + 4))  # more segments than the union's rank path takes
    for r in _bcl2():
        add(r)
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def _want_mask(shift, W, k1, k2):
    m, counts = mr.mask_batch(_records(shift), W, k1, k2)
    m.setflags(write=False); counts.setflags(write=False)
    return m, counts


@functools.lru_cache(maxsize=None)
def _want_split(min_len):
    return mr.split_batch(_records(), min_len)


@functools.lru_cache(maxsize=None)
def _want_sketch(mol, k, scaled):
    return mr.masked_sketch(_records(), k, scaled, mol)


def _set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, path)


def _check_sketches(sk, want):
    o, h, a = sk.to_host()
    assert sk.n_seqs == len(want[0]) - 1 and sk.n_hashes == len(want[1])
    assert np.array_equal(o, want[0]) and np.array_equal(h, want[1]) and np.array_equal(a, want[2])
    assert o.dtype == np.uint64 and h.dtype == np.uint64 and a.dtype == np.uint32


def test_batch_holds_what_it_should():
    """the reference alone: the batch has the cases the other tests rely on"""
    L = _lib.load()
    chunk, R = int(L.ks_debug_mask_chunk()), int(L.ks_debug_union_rank_max())
    recs = _records()
    lens = [len(r) for r in recs]
    assert {0, 1, 2, 3, 11, 12, 13, 31, 32, 33} <= set(lens) and sum(1 for n in lens if 1 <= n <= 40) >= 300
    m, counts = _want_mask(0, *mr.DEFAULTS)
    assert 0 < int(m.sum()) < len(m) and int(counts.sum()) == int(m.sum())
    for shift in (-1, 0, 1):
        ms, _ = _want_mask(shift, *mr.DEFAULTS)
        for k in (1, 2, 3):
            e = k * chunk + shift
            assert ms[e - 20:e].all() and not ms[e], (shift, k)
    for k in KS:
        seg_lens = np.diff(_want_split(k)[2].astype(np.int64))
        assert len(seg_lens) and seg_lens.min() == k and k + 1 in seg_lens
        assert k - 1 in np.diff(_want_split(1)[2].astype(np.int64))
        assert np.diff(_want_split(k)[4].astype(np.int64)).max() > R
        assert 0 in np.diff(_want_split(k)[4].astype(np.int64))[[i for i, n in enumerate(lens) if n >= k]]


# ---- the mask ---------------------------------------------------------------------------------------------------------------------
def _mask_and_check(c, recs, want, W, k1, k2):
    res, offs = tr.pack(recs)
    M = c.mask_low_complexity(res, offs, window=W, k1=k1 / 1000, k2=k2 / 1000)
    m, counts = M.to_host()
    assert M.n_seqs == len(recs) and M.n_residues == len(res) and M.n_masked == int(want[0].sum())
    assert m.dtype == np.uint8 and counts.dtype == np.uint32
    assert np.array_equal(counts, want[1])
    assert np.array_equal(m, want[0]), np.flatnonzero(m != want[0])[:10]
    return M


@pytest.mark.parametrize("W,k1,k2", MASK_CASES)
def test_mask_bytes_and_counts(W, k1, k2):
    with ks.Context(0) as c:
        recs = _records()
        _mask_and_check(c, recs, _want_mask(0, W, k1, k2), W, k1, k2)
        res, offs = tr.pack(recs)
        d_res, d_off = c.to_device(res), c.to_device(offs)
        M = c.mask_low_complexity_device(d_res.ptr, d_off.ptr, len(recs), len(res), window=W, k1=k1 / 1000, k2=k2 / 1000)
        m, counts = M.to_host()
        assert np.array_equal(m, _want_mask(0, W, k1, k2)[0]) and np.array_equal(counts, _want_mask(0, W, k1, k2)[1])


@pytest.mark.parametrize("shift", (-1, 1))
def test_mask_runs_around_the_chunk_boundaries(shift):
    with ks.Context(0) as c:
        _mask_and_check(c, _records(shift), _want_mask(shift, *mr.DEFAULTS), *mr.DEFAULTS)


def test_mask_small_batches_and_defaults():
    with ks.Context(0) as c:
        for recs in ([], [b"", b"", b""], [b"A" * 12], [b"A" * 11], [b"AAACCCDDDEEE", b"AAACCCDDEEGG"], [b"a"], [b"", b"K" * 40, b""]):
            for W, k1, k2 in ((12, 2200, 2500), (2, 0, 0), (31, 2200, 2500)):
                _mask_and_check(c, recs, mr.mask_batch(recs, W, k1, k2), W, k1, k2)
        # an all-zero options struct and NULL mean the defaults; an unaligned residue pointer is read by bytes
        recs = _records()
        res, offs = tr.pack(recs)
        want = _want_mask(0, *mr.DEFAULTS)
        d_res, d_off = c.to_device(np.concatenate([np.zeros(1, np.uint8), res])), c.to_device(offs)
        for opts in (None, C.byref(_lib.ks_mask_opts(0, 0, 0)), C.byref(_lib.ks_mask_opts(0, 2200, 2500))):
            out = C.c_void_p()
            c._check(c._L.ks_mask_device(c._h, C.c_void_p(d_res.ptr + 1), d_off._p, len(recs), len(res), opts, C.byref(out)))
            m, counts = ks.Mask(c, out).to_host()
            assert np.array_equal(m, want[0]) and np.array_equal(counts, want[1])


# ---- the split --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", (1, 7, 24, 0))
def test_split_arrays(min_len):
    want = _want_split(max(min_len, 1))
    with ks.Context(0) as c:
        res, offs = tr.pack(_records())
        M = c.mask_low_complexity(res, offs)
        S = c.split_masked(M, res, offs, min_len)
        assert (S.n_segs, S.n_residues, S.n_records) == (len(want[0]), len(want[3]), len(offs) - 1)
        got = S.to_host()
        for g, w, name in zip(got, want, ks.Segments._COLUMNS):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
        assert S.device_ptrs()[3] % 16 == 0


def test_split_small_batches():
    with ks.Context(0) as c:
        for recs in ([], [b"", b""], [b"A" * 30], [b"MKTLWVHN"], [b"MKTLWVHN", b"", b"A" * 12, b"QRS"]):
            for min_len in (1, 4, 9):
                res, offs = tr.pack(recs)
                want = mr.split_batch(recs, min_len)
                S = c.split_masked(c.mask_low_complexity(res, offs), res, offs, min_len)
                assert (S.n_segs, S.n_residues, S.n_records) == (len(want[0]), len(want[3]), len(recs))
                for g, w in zip(S.to_host(), want):
                    assert np.array_equal(g, w)


# ---- the masked sketch against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mol,k,scaled", PARAMS)
def test_sketch_masked_matches_the_oracle(monkeypatch, mol, k, scaled, path):
    want = _want_sketch(mol, k, scaled)
    plain = oracle.sketch_batch(*tr.pack(_records()), k, scaled, mol)
    assert len(want[1]) < len(plain[1])  # masking takes something away
    with ks.Context(0, follow_debug_env=True) as c:
        _set_path(monkeypatch, path)
        res, offs = tr.pack(_records())
        sk = c.sketch_masked(res, offs, k, scaled, mol)
        _check_sketches(sk, want[:3])
        assert sk.n_windows == want[3] and not sk.has_postings
        d_res, d_off = c.to_device(res), c.to_device(offs)
        for hint in (0, max(len(r) for r in _records())):
            sk = c.sketch_masked_device(d_res.ptr, d_off.ptr, len(offs) - 1, len(res), k, scaled, mol, max_seq_len=hint)
            _check_sketches(sk, want[:3])
            assert sk.n_windows == want[3]
        before = c.pool_stats()["bytes_in_use"]
        c.sketch_masked_device(d_res.ptr, d_off.ptr, len(offs) - 1, len(res), k, scaled, mol).free()
        assert c.pool_stats()["bytes_in_use"] == before  # scratch went back to the pool


def test_sketch_masked_other_options_and_empty_records():
    with ks.Context(0) as c:
        recs = list(_records()[-40:]) + [b"", b"A" * 50, b"MKT"]
        res, offs = tr.pack(recs)
        for W, k1, k2 in ((2, 0, 1000), (32, 2200, 2500)):
            want = mr.masked_sketch(recs, 10, 1, "protein", W, k1, k2)
            sk = c.sketch_masked(res, offs, 10, 1, "protein", window=W, k1=k1 / 1000, k2=k2 / 1000)
            _check_sketches(sk, want[:3])
            assert sk.n_windows == want[3]
        for batch in ([], [b"", b""], [b"A" * 40, b"G" * 13]):  # nothing to sketch: empty sketches, one per record
            sk = c.sketch_masked(*tr.pack(batch), 7, 1, "protein")
            o, h, a = sk.to_host()
            assert sk.n_seqs == len(batch) and sk.n_hashes == 0 and sk.n_windows == 0 and not o.any() and len(o) == len(batch) + 1


def test_masking_that_masks_nothing_is_the_plain_sketch():
    rng = np.random.default_rng(59)
    recs = [_prot(rng, int(n)) for n in rng.integers(0, 400, size=120)] + [b"", b"MKTLWVH", b"MKTLWV"]
    assert not mr.mask_batch(recs, 12, 0, 0)[0].any()  # no window of one class: k1 = k2 = 0 masks nothing
    res, offs = tr.pack(recs)
    with ks.Context(0) as c:
        for mol, k, scaled in PARAMS:
            want = oracle.sketch_batch(res, offs, k, scaled, mol)
            sk = c.sketch_masked(res, offs, k, scaled, mol, k1=0.0, k2=0.0)
            _check_sketches(sk, want)
            assert sk.n_windows == sum(max(0, len(r) - k + 1) for r in recs)


# ---- masked positions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol,k,scaled", (("protein", 7, 1), ("hp", 24, 5)))
def test_masked_positions(mol, k, scaled):
    recs = [r for r in _records() if r == r.upper()]  # (the oracle's position walk hashes the bytes as given)
    assert len(recs) > len(_records()) - 8
    want = mr.masked_positions(recs, k, scaled, mol)
    assert 0 < len(want[0]) and np.all(np.diff(want[0].astype(np.int64)) >= 0)
    res, offs = tr.pack(recs)
    with ks.Context(0) as c:
        P = c.kmer_positions_table_masked(res, offs, k, scaled, mol)
        got = P.to_host()
        assert P.count == len(want[0])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        # the table agrees with the masked sketch: its distinct hashes per record are the record's sketch
        so, sh, _, _ = mr.masked_sketch(recs, k, scaled, mol)
        for r in (0, len(recs) // 2, len(recs) - 1):
            assert np.array_equal(np.unique(got[2][got[0] == r]), sh[int(so[r]):int(so[r + 1])])


def test_wire_sketch_with_mask(tmp_path):
    recs = list(_records()[-30:])
    fasta = tmp_path / "m.fasta"
    fasta.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(recs) if r))
    recs = [r for r in recs if r]
    want = mr.masked_sketch(recs, 10, 1, "protein")
    with ks.Context(0) as c:
        names, o, m, a, kk, ss, mm = wire.read_sig_zip(wire.sketch(str(fasta), "protein", 10, 1, ctx=c, mask=True))
        assert names == [f"r{i}" for i in range(len(recs))] and (kk, ss, mm) == (10, 1, "protein")
        assert np.array_equal(o, want[0]) and np.array_equal(m, want[1]) and np.array_equal(a, want[2])
        w2 = mr.masked_sketch(recs, 10, 1, "protein", 2, 0, 1000)
        _, o, m, a, _, _, _ = wire.read_sig_zip(wire.sketch(str(fasta), "protein", 10, 1, ctx=c, mask=True, mask_opts=dict(window=2, k1=0.0, k2=1.0)))
        assert np.array_equal(o, w2[0]) and np.array_equal(m, w2[1]) and np.array_equal(a, w2[2])
        with pytest.raises(ValueError):
            wire.sketch(str(fasta), "protein", 10, 1, ctx=c, mask=True, translate=True)


# ---- what is refused ----------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable():
    INV = _lib.KS_ERR_INVALID_ARG
    recs = [b"MKTLWVHNQRSTAAAAAAAAAAAAAAMKTLWVHNQRST", b"ACDEFGHIKLMNPQRSTVWY" * 2]
    res, offs = tr.pack(recs)
    want = mr.mask_batch(recs)
    with ks.Context(0) as c:
        L = c._L
        d_res, d_off = c.to_device(res), c.to_device(offs)
        p = ks.make_params(7, 1, "protein")
        out = C.c_void_p()

        def refused(st, *words):
            assert st == INV and not out.value
            msg = L.ks_last_error(c._h).decode()
            assert all(w in msg for w in words), msg
            _mask_and_check(c, recs, want, *mr.DEFAULTS)  # the context still works

        for o in (_lib.ks_mask_opts(1, 2200, 2500), _lib.ks_mask_opts(33, 2200, 2500), _lib.ks_mask_opts(12, 2500, 2200)):
            word = "k2" if o.window == 12 else "window"
            refused(L.ks_mask_device(c._h, d_res._p, d_off._p, 2, len(res), C.byref(o), C.byref(out)), "options", word)
            refused(L.ks_mask_batch(c._h, res.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), 2, C.byref(o), C.byref(out)), "options", word)
            refused(L.ks_sketch_masked_device(c._h, d_res._p, d_off._p, 2, len(res), 0, C.byref(p), C.byref(o), C.byref(out)), "options", word)
            refused(L.ks_sketch_masked(c._h, res.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), 2, C.byref(p), C.byref(o), C.byref(out)), "options", word)
            refused(L.ks_kmer_positions_masked_device(c._h, d_res._p, d_off._p, 2, len(res), C.byref(p), C.byref(o), C.byref(out)), "options", word)
        with pytest.raises(ValueError):
            c.mask_low_complexity(res, offs, window=33)
        # offsets that do not start at 0, descend, overrun: found on the device, the record named
        n = len(res)
        for bad, rec in (([1, 38, n], 0), ([0, 60, 50, n], 1), ([0, 38, n + 5], 1), ([0, 38, n - 1], 1)):
            d_bad = c.to_device(np.array(bad, np.uint64))
            for call in (lambda: L.ks_mask_device(c._h, d_res._p, d_bad._p, len(bad) - 1, n, None, C.byref(out)),
                         lambda: L.ks_sketch_masked_device(c._h, d_res._p, d_bad._p, len(bad) - 1, n, 0, C.byref(p), None, C.byref(out)),
                         lambda: L.ks_kmer_positions_masked_device(c._h, d_res._p, d_bad._p, len(bad) - 1, n, C.byref(p), None, C.byref(out))):
                refused(call(), "offsets", f"record {rec}")
        M = c.mask_low_complexity(res, offs)
        seg = C.c_void_p()
        d_bad = c.to_device(np.array([0, 60, 50, n], np.uint64))
        assert L.ks_mask_split_device(c._h, M._h, d_res._p, d_bad._p, 2, n, 1, C.byref(seg)) == INV and not seg.value  # another record count
        M3 = c.mask_low_complexity(*tr.pack([res.tobytes()[:38], res.tobytes()[38:60], res.tobytes()[60:]]))
        assert L.ks_mask_split_device(c._h, M3._h, d_res._p, d_bad._p, 3, n, 1, C.byref(seg)) == INV and not seg.value
        assert "record 1" in L.ks_last_error(c._h).decode()
        # NULL arguments
        assert L.ks_mask_device(c._h, None, d_off._p, 2, n, None, C.byref(out)) == INV
        assert L.ks_mask_device(c._h, d_res._p, None, 2, n, None, C.byref(out)) == INV
        assert L.ks_mask_device(c._h, d_res._p, d_off._p, 2, n, None, None) == INV
        assert L.ks_mask_device(None, d_res._p, d_off._p, 2, n, None, C.byref(out)) == INV
        assert L.ks_mask_split_device(c._h, None, d_res._p, d_off._p, 2, n, 1, C.byref(seg)) == INV
        assert L.ks_mask_split_device(c._h, M._h, d_res._p, d_off._p, 2, n, 1, None) == INV
        assert L.ks_sketch_masked_device(c._h, d_res._p, d_off._p, 2, n, 0, None, None, C.byref(out)) != _lib.KS_OK
        assert L.ks_sketch_masked_device(c._h, d_res._p, d_off._p, 2, n, 0, C.byref(p), None, None) == INV
        assert L.ks_kmer_positions_masked_device(c._h, d_res._p, d_off._p, 2, n, C.byref(p), None, None) == INV
        assert L.ks_mask_device(c._h, d_res._p, d_off._p, 0, n, None, C.byref(out)) == INV  # residues without records
        with ks.Context(0) as other:
            Mo = other.mask_low_complexity(res, offs)
            assert L.ks_mask_split_device(c._h, Mo._h, d_res._p, d_off._p, 2, n, 1, C.byref(seg)) == INV and "another context" in L.ks_last_error(c._h).decode()
        with pytest.raises(ks.KmerseekError) as e:
            c.sketch_masked_device(d_res.ptr, d_off.ptr, 2, n, 7, 1, "protein", max_seq_len=10)
        assert e.value.status == INV
        _mask_and_check(c, recs, want, *mr.DEFAULTS)
        _check_sketches(c.sketch_masked(res, offs, 7, 1, "protein"), mr.masked_sketch(recs, 7, 1, "protein")[:3])


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{r.decode()}\n" for n, r in recs))
    return str(path)


def test_wire_search_extract_kmers_with_mask(tmp_path):
    """search_extract_kmers_device(mask=True): masked sketches on both sides, masked position tables, the join.  The rows are those
    the host stitcher makes of the reference's masked sketches, the oracle's search of them and the reference's masked positions."""
    import matchpos_join as mj
    k, scaled, mol = 7, 1, "protein"
    t_recs = [(f"t{i}", r) for i, r in enumerate(r for r in _records()[-75:] if r.isalpha() and r.isupper())]  # (a FASTA of letters)
    q_recs = [(f"q{i}", r) for i, (_, r) in enumerate(t_recs[::6])] + [("q_mix", b"MKTLWVHN" + b"W" * 14 + t_recs[30][1][:60] + b"P" * 13 + t_recs[2][1][5:50])]
    qs, ts = [r for _, r in q_recs], [r for _, r in t_recs]
    assert mr.mask_batch(qs)[0].any() and mr.mask_batch(ts)[0].any()
    q_sk, t_sk = mr.masked_sketch(qs, k, scaled, mol), mr.masked_sketch(ts, k, scaled, mol)
    hits = oracle.manysearch(q_sk[0], q_sk[1], t_sk[0], t_sk[1], t_sk[2])
    J = mj.join(mr.masked_positions(qs, k, scaled, mol), mr.masked_positions(ts, k, scaled, mol), hits[0], hits[1], k)
    want = wire.stitch_match_positions(q_recs, t_recs, hits[0], hits[1], J[0], J[1], J[2], k, mol)
    assert len(hits[0]) >= 10 and len(want) >= 10 and int(J[0][-1]) > 500
    qf, tf = _fasta(tmp_path / "q.fasta", q_recs), _fasta(tmp_path / "t.fasta", t_recs)
    with ks.Context(0) as c:
        got = wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c, mask=True)
        assert got == want
        # other options reach both sides
        w2 = (12, 1800, 2200)
        q2, t2 = mr.masked_sketch(qs, k, scaled, mol, *w2), mr.masked_sketch(ts, k, scaled, mol, *w2)
        h2 = oracle.manysearch(q2[0], q2[1], t2[0], t2[1], t2[2])
        assert len(h2[0]) >= 10 and not np.array_equal(q2[1], q_sk[1])  # another mask than the default's
        J2 = mj.join(mr.masked_positions(qs, k, scaled, mol, *w2), mr.masked_positions(ts, k, scaled, mol, *w2), h2[0], h2[1], k)
        assert wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c, mask=True, mask_opts=dict(k1=1.8, k2=2.2)) == \
            wire.stitch_match_positions(q_recs, t_recs, h2[0], h2[1], J2[0], J2[1], J2[2], k, mol)
        # a mask that masks nothing gives the rows of mask=False
        rng = np.random.default_rng(61)
        t_plain = [(f"t{i}", _prot(rng, int(n))) for i, n in enumerate(rng.integers(20, 300, size=30))]
        q_plain = [(f"q{i}", r[3:]) for i, (_, r) in enumerate(t_plain[::5])]
        assert not mr.mask_batch([r for _, r in t_plain + q_plain], 12, 0, 0)[0].any()
        qf, tf = _fasta(tmp_path / "qp.fasta", q_plain), _fasta(tmp_path / "tp.fasta", t_plain)
        rows = wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c)
        assert len(rows) >= len(q_plain)
        assert wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c, mask=True, mask_opts=dict(k1=0.0, k2=0.0)) == rows
        with pytest.raises(ValueError):
            wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c, mask_opts=dict(window=12))
        with pytest.raises(ValueError):
            wire.search_extract_kmers_device(qf, tf, k, scaled, mol, ctx=c, mask=True, mask_opts=dict(window=0, k1=0.0, k2=0.0))


def test_python_refuses_a_window_of_zero():
    """window = 0 would make the all-zero struct with k1 = k2 = 0, which the library reads as the defaults"""
    from kmerseek_amd import engine
    for w in (0, 1, 33, 2.5):
        with pytest.raises(ValueError):
            engine.mask_opts(w, 0.0, 0.0)
    o = engine.mask_opts(2, 0.0, 0.0)
    assert (o.window, o.k1_millibits, o.k2_millibits) == (2, 0, 0)
