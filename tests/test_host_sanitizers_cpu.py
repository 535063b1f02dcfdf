"""The host layer (ks_ingest.cpp, ks_host.cpp, ks_input.cpp, ks_hostfn.cpp) under AddressSanitizer + UBSan and under
ThreadSanitizer, against the CPU stand-in of the ABI in tests/hostsan/ ("Host layer under sanitizers").

Stand-alone programs only: they are built once per session into a temporary directory and every case runs as a
subprocess with its own time limit (a deadlock of the ingest pipeline shows as that limit).  Nothing sanitized is loaded
into this interpreter, and nothing here needs a GPU.  Expected values come from the oracle over records parsed by
oracle.read_fasta: they never pass through the stand-in.

Timeouts are hang detectors, about ten times the wall time measured for the case (written beside each), no performance bound.
"""
import bz2
import gzip
import importlib.util
import json
import lzma
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BCL2 = os.path.join(GOLDEN, "bcl2_first25_uniprotkb_accession_O43236_OR_accession_2025_02_06.fasta.gz")
CED9 = os.path.join(GOLDEN, "ced9.fasta")
CHUNK = 4 << 20  # the reader's chunk (ks_ingest.cpp)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
K, SCALED, MOL = 16, 5, "hp"

SAN_ENV = {
    "TSAN_OPTIONS": "halt_on_error=1:exitcode=66",
    "ASAN_OPTIONS": "detect_leaks=1:exitcode=67",
    "UBSAN_OPTIONS": "print_stacktrace=1",
}
BOTH = ["asan", "tsan"]


@pytest.fixture(scope="session")
def progs(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("hostsan_build", os.path.join(HERE, "hostsan", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(str(tmp_path_factory.mktemp("hostsan_bin")))


def run(exe, args, timeout):
    env = dict(os.environ)
    env.update(SAN_ENV)
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                       timeout=timeout)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, f"{os.path.basename(exe)} {args}\nexit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    return p.stdout


def stats(out):
    line = [l for l in out.splitlines() if l.startswith("n_records=")][0]
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def parse_sketches(path):
    b = open(path, "rb").read()
    n, nh = np.frombuffer(b, np.uint64, 2).tolist()
    p = 16
    offs = np.frombuffer(b, np.uint64, n + 1, p); p += 8 * (n + 1)
    mins = np.frombuffer(b, np.uint64, nh, p); p += 8 * nh
    abunds = np.frombuffer(b, np.uint32, nh, p); p += 4 * nh
    ln = int(np.frombuffer(b, np.uint64, 1, p)[0]); p += 8
    blob = b[p:p + ln]
    assert p + ln == len(b)
    names = blob.decode().split("\n") if n else []
    return names, offs, mins, abunds


def expected(records, k=K, scaled=SCALED, mol=MOL):
    res, offs = oracle.pack([s for _, s in records])
    return [n for n, _ in records], oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=4)


def assert_sketches(path, want):
    names, offs, mins, abunds = parse_sketches(path)
    wn, (wo, wm, wa) = want
    assert names == wn
    assert np.array_equal(offs, wo) and np.array_equal(mins, wm) and np.array_equal(abunds, wa)


def write_fasta(path, records, width=60):
    with open(path, "wb") as f:
        for n, s in records:
            f.write(b">" + n.encode() + b"\n")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + b"\n")
    return str(path)


def random_seq(rng, n):
    return AA[rng.integers(0, 20, n)].tobytes()


# ---- san_ingest ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def small_files(tmp_path_factory):
    """BCL2-25 (gzip, as committed), ced9 and both in one plain file, with the oracle's sketches of each."""
    d = tmp_path_factory.mktemp("hostsan_small")
    both = oracle.read_fasta(BCL2) + oracle.read_fasta(CED9)
    files = {"bcl2": BCL2, "ced9": CED9, "both": write_fasta(d / "both.fasta", both)}
    return {k: (p, expected(oracle.read_fasta(p))) for k, p in files.items()}


@pytest.mark.parametrize("san", BOTH)
def test_ingest_small_batches_equal_oracle(progs, small_files, tmp_path, san):
    """Small batches: the three slots are reused several times and the queues fill; 8 jitter seeds, pipelined and serial."""
    for name, (path, want) in small_files.items():
        outs = []
        for pipeline in (1, 0):
            out = tmp_path / f"{name}.{pipeline}.bin"
            # measured: 0.2 s (asan), 0.5 s (tsan) per run
            st = stats(run(progs[san]["san_ingest"], ["sketch", path, K, SCALED, MOL, 0, 500, pipeline, out, 8, 200], timeout=10))
            if name != "ced9":  # (one record: one batch)
                assert st["n_batches"] >= 10, st
            assert st["n_records"] == len(want[0])
            assert_sketches(out, want)
            outs.append(open(out, "rb").read())
        assert outs[0] == outs[1]


@pytest.fixture(scope="session")
def framing_file(tmp_path_factory):
    """Two chunks and a bit: '>' is the first byte of the second chunk, a CRLF is split across the second chunk boundary;
    blank lines, CRLF records, a record without sequence, an unterminated last line."""
    rng = np.random.default_rng(11)
    parts, size, i = [], 0, 0

    def add(b):
        nonlocal size
        parts.append(b)
        size += len(b)

    def record(eol=b"\n"):
        nonlocal i
        i += 1
        s = random_seq(rng, int(rng.integers(40, 1200)))
        add(b">r%d some description %d" % (i, i) + eol)
        for j in range(0, len(s), 60):
            add(s[j:j + 60] + eol)
        if i % 7 == 0:
            add(eol)  # blank line
        if i % 97 == 0:
            add(b">empty%d" % i + eol)  # a record with no sequence

    def fill_to(target):  # records until `target` is near, then one line that ends exactly there
        while size < target - 4000:
            record(b"\r\n" if i % 5 == 0 else b"\n")
        add(b">pad%d\n" % size)
        return target - size

    left = fill_to(CHUNK)
    add(random_seq(rng, left - 1) + b"\n")  # the next byte, the first of the second chunk, is a '>'
    assert size == CHUNK
    record()
    left = fill_to(2 * CHUNK)
    add(random_seq(rng, left - 1) + b"\r")  # '\r' is the last byte of the second chunk, '\n' the first of the third
    assert size == 2 * CHUNK - 0 and parts[-1][-1:] == b"\r"
    add(b"\n")
    for _ in range(200):
        record(b"\r\n" if i % 5 == 0 else b"\n")
    add(b">last\n" + random_seq(rng, 333))  # no terminator
    blob = b"".join(parts)
    assert blob[CHUNK:CHUNK + 1] == b">" and blob[2 * CHUNK - 1:2 * CHUNK + 1] == b"\r\n" and not blob.endswith(b"\n")
    d = tmp_path_factory.mktemp("hostsan_framing")
    path = d / "framing.fasta"
    path.write_bytes(blob)
    records = oracle.read_fasta(str(path))
    assert any(len(s) == 0 for _, s in records) and records[-1][0] == "last"
    return str(path), expected(records), sum(len(s) for _, s in records)


@pytest.mark.parametrize("san", BOTH)
def test_ingest_framing_across_chunks(progs, framing_file, tmp_path, san):
    path, want, n_res = framing_file
    # (the serial path starts no thread: ThreadSanitizer runs the pipelined one only — 8.4 M windows are hashed per run)
    for pipeline in (1, 0) if san == "asan" else (1,):
        out = tmp_path / f"framing.{pipeline}.bin"
        # measured: 3 s (asan), 15 s (tsan) per run
        st = stats(run(progs[san]["san_ingest"], ["sketch", path, K, SCALED, MOL, 0, 1 << 20, pipeline, out, 1, 300], timeout=150))
        assert st["n_residues"] == n_res and st["n_batches"] >= 8
        assert_sketches(out, want)
    # a header-only file (one record without sequence, no terminator) and an empty file
    hdr, empty = tmp_path / "hdr.fasta", tmp_path / "empty.fasta"
    hdr.write_bytes(b">only a header")
    empty.write_bytes(b"")
    for path, recs in ((hdr, [("only a header", b"")]), (empty, [])):
        assert oracle.read_fasta(str(path)) == recs
        for pipeline in (1, 0):
            out = tmp_path / f"edge.{pipeline}.bin"
            run(progs[san]["san_ingest"], ["sketch", path, K, SCALED, MOL, 1, 1000, pipeline, out, 2, 100], timeout=10)  # measured: 0.1 s
            names, offs, mins, abunds = parse_sketches(out)
            assert names == [n for n, _ in recs] and offs.tolist() == [0] * (len(recs) + 1) and len(mins) == 0


@pytest.fixture(scope="session")
def one_batch_file(tmp_path_factory):
    """4.6 M residues in short records (the oracle's sorted insert is quadratic in the record): > 2^22 hashes at scaled = 1."""
    rng = np.random.default_rng(21)
    recs = [(f"s{i}", random_seq(rng, 200)) for i in range(23000)]
    path = write_fasta(tmp_path_factory.mktemp("hostsan_one") / "one.fasta", recs, width=80)
    want = expected(recs, 10, 1, "protein")
    assert len(want[1][1]) > 1 << 22
    return path, want


@pytest.mark.parametrize("san", BOTH)
def test_ingest_collect_four_threads(progs, one_batch_file, tmp_path, san):
    """One batch that keeps more than 2^22 hashes: collect() splits its copy over four threads (and pack() its raw copy
    over sixteen)."""
    path, want = one_batch_file
    out = tmp_path / "one_batch.bin"
    # measured: 3.6 s (asan), 13 s (tsan)
    st = stats(run(progs[san]["san_ingest"], ["sketch", path, 10, 1, "protein", 0, 16 << 20, 1, out, 1, 300], timeout=140))
    assert st["n_batches"] == 1 and st["n_hashes"] == len(want[1][1])
    assert_sketches(out, want)


@pytest.fixture(scope="session")
def big_batch(tmp_path_factory):
    """One batch of >= 1 MiB residues (pack() takes its multi-thread branch) with B / Z / J, lower case and '*'."""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(1500):
        s = bytearray(random_seq(rng, int(rng.integers(500, 1100))))
        for _ in range(6):
            s[int(rng.integers(0, len(s)))] = b"BZJ"[int(rng.integers(0, 3))]
        if i % 3 == 0:
            s = bytearray(bytes(s).lower())
        if i % 50 == 7:
            s[int(rng.integers(100, len(s)))] = ord("*")  # truncates (inclusive)
        recs.append((f"big{i}", bytes(s)))
    assert sum(len(s) for _, s in recs) >= (1 << 20) + 4096
    d = tmp_path_factory.mktemp("hostsan_big")
    path = write_fasta(d / "big.fasta", recs)
    assert oracle.read_fasta(path) == recs
    resolved = [(n, oracle.validate_and_resolve(s.upper())) for n, s in recs]  # (all-first choices: D, E, I)
    return d, path, recs, resolved


@pytest.mark.parametrize("san", BOTH)
def test_ingest_multithread_pack(progs, big_batch, tmp_path, san):
    d, path, recs, resolved = big_batch
    exe = progs[san]["san_ingest"]
    # raw bytes (validate = 0): one split copy.  measured: 1.1 s (asan), 5 s (tsan) per run of two seeds
    out = tmp_path / "raw.bin"
    st = stats(run(exe, ["sketch", path, K, SCALED, MOL, 0, 4 << 20, 1, out, 2, 300], timeout=60))
    assert st["n_batches"] == 1 and st["n_residues"] >= 1 << 20
    assert_sketches(out, expected(recs))
    # validated: lengths as the oracle's validator gives them; hp encodes both candidates of B / Z / J alike, so the
    # sketches are those of the oracle's resolution whatever was drawn
    out, cap = tmp_path / "val.bin", tmp_path / "val.cap"
    st = stats(run(exe, ["sketch", path, K, SCALED, MOL, 1, 4 << 20, 1, out, 2, 300, cap], timeout=60))
    assert st["n_batches"] == 1
    assert_sketches(out, expected(resolved))
    b = open(cap, "rb").read()
    n, n_res = np.frombuffer(b, np.uint64, 2).tolist()
    lens = np.frombuffer(b, np.uint64, n, 16)
    got = np.frombuffer(b, np.uint8, n_res, 16 + 8 * n)
    assert lens.tolist() == [len(s) for _, s in resolved] and n_res == st["n_residues"] == int(lens.sum())
    want = np.frombuffer(b"".join(s for _, s in resolved), np.uint8)
    orig = np.frombuffer(b"".join(s.upper()[:len(r)] for (_, s), (_, r) in zip(recs, resolved)), np.uint8)
    plain = ~np.isin(orig, np.frombuffer(b"BZJ", np.uint8))
    assert np.array_equal(got[plain], want[plain])
    for amb, pair in ((b"B", b"DN"), (b"Z", b"EQ"), (b"J", b"IL")):
        at = orig == amb[0]
        assert at.sum() > 100 and np.isin(got[at], np.frombuffer(pair, np.uint8)).all()
        assert len(np.unique(got[at])) == 2  # (both candidates are drawn)


def _invalid_message(seq):
    with pytest.raises(oracle.InvalidAminoAcid) as e:
        oracle.validate_and_resolve(seq.upper())
    return str(e.value)


@pytest.mark.parametrize("san", BOTH)
def test_ingest_clean_failures(progs, big_batch, tmp_path, san):
    """Every failure returns its documented code and message with all threads joined, nothing leaked, under several
    jitter seeds, pipelined and serial; a deadlock is the subprocess time limit."""
    exe = progs[san]["san_ingest"]
    base = oracle.read_fasta(BCL2)
    plain = write_fasta(tmp_path / "bcl2.fasta", base)
    n_batches = stats(run(exe, ["sketch", plain, K, SCALED, MOL, 1, 500, 1, tmp_path / "ok.bin", 1, 0], timeout=10))["n_batches"]
    assert n_batches >= 10
    # an invalid residue in the first, a middle and the last batch (measured: 0.3 s asan, 1 s tsan each)
    for at in (0, len(base) // 2, len(base) - 1):
        recs = list(base)
        s = recs[at][1]
        recs[at] = (recs[at][0], s[:17] + b"1" + s[17:])
        bad = write_fasta(tmp_path / f"bad{at}.fasta", recs)
        out = run(exe, ["expect", bad, K, SCALED, MOL, 1, 500, 3, 6, 200], timeout=15)
        assert f"msg={_invalid_message(recs[at][1])}\n" in out and "found at position 18" in out
    # several packer threads fail: the first failing record in file order is the one reported
    d, path, big, resolved = big_batch
    recs = list(big)
    first = None
    for at, ch in ((1400, b"1"), (700, b"2"), (90, b"3"), (91, b"4")):
        s = recs[at][1]
        cut = 5 + at % 40
        assert b"*" not in s[:cut]
        recs[at] = (recs[at][0], s[:cut] + ch + s[cut:])
    first = _invalid_message(recs[90][1])
    assert "'3'" in first
    bad = write_fasta(tmp_path / "bigbad.fasta", recs)
    out = run(exe, ["expect", bad, K, SCALED, MOL, 1, 4 << 20, 3, 3, 300], timeout=60)  # measured: 1 s (asan), 2.5 s (tsan)
    assert f"msg={first}\n" in out
    # a file that does not start with '>', and a gzip cut in the middle of its second member: code 11
    nohdr = tmp_path / "nohdr.fasta"
    nohdr.write_bytes(b"ACDEFG\n>x\nACDEFG\n")
    out = run(exe, ["expect", nohdr, K, SCALED, MOL, 0, 500, 11, 4, 200], timeout=10)  # measured: 0.1 s
    assert "msg=Parse error: FASTA record does not start with '>'" in out
    text = open(plain, "rb").read()
    rng = np.random.default_rng(3)
    second = gzip.compress(b"".join(b">x%d\n" % i + random_seq(rng, 700) + b"\n" for i in range(400)))
    cut = tmp_path / "cut.fasta.gz"
    cut.write_bytes(gzip.compress(text) + second[:len(second) // 2])
    out = run(exe, ["expect", cut, K, SCALED, MOL, 0, 500, 11, 4, 200], timeout=15)  # measured: 0.5 s
    assert "msg=Parse error: gzip stream is truncated or corrupt" in out
    # the first, a middle and the last call of hipHostMalloc, hipMemcpyAsync, ks_sketch_batch_device and
    # ks_sketches_copy_to_host fail in turn: code 13 (measured: 1.7 s asan, 5 s tsan)
    out = run(exe, ["faults", plain, K, SCALED, MOL, 0, 500, 4, 200], timeout=60)
    assert out.count("code 13 each") == 8 and "ok 96 cases" in out


# ---- san_index -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def many_fasta(tmp_path_factory):
    rng = np.random.default_rng(9)
    recs = []
    for i in range(300):
        s = bytearray(random_seq(rng, int(rng.integers(60, 400))))
        s[20 + i % 30] = b"BZJ"[i % 3]
        recs.append((f"many{i}", bytes(s).lower() if i % 4 == 0 else bytes(s)))
    return write_fasta(tmp_path_factory.mktemp("hostsan_many") / "many.fasta", recs)


@pytest.mark.parametrize("san", BOTH)
def test_index_search_save_load(progs, many_fasta, tmp_path, san):
    out = tmp_path / "rows.json"
    # measured: 1.2 s (asan), 4.8 s (tsan)
    run(progs[san]["san_index"], ["search", tmp_path, BCL2, CED9, many_fasta, out, 3, 200], timeout=60)
    rows = sorted(json.load(open(out)), key=lambda r: r["match_name"])
    exp_doc = json.load(open(os.path.join(GOLDEN, "search_expected.json")))
    exp = sorted(exp_doc["manysearch_rows"], key=lambda r: r["match_name"])
    assert len(rows) == len(exp) == 5
    assert list(rows[0].keys()) == exp_doc["manysearch_columns"]
    for g, w in zip(rows, exp):  # the tolerances of tests/test_host_index.py
        for col in exp_doc["manysearch_columns"]:
            if col in ("query_name", "query_md5", "match_name", "match_md5", "moltype"):
                assert str(g[col]) == w[col], col
            else:
                assert math.isclose(float(g[col]), float(w[col]), rel_tol=1e-12, abs_tol=1e-15), (col, g[col], w[col])


def test_index_hostile_state_files(progs, tmp_path):
    """Every truncation, every length / count field replaced by 0, 2^32, 2^63 and 2^64 - 1, and 2,000 seeded mutations of a
    small valid state file: each load is an error or a valid index (single-threaded: ASan + UBSan)."""
    out = run(progs["asan"]["san_index"], ["hostile", tmp_path, 2000], timeout=30)  # measured: 2 s
    print(out)
    line = {l.split(":")[0]: l for l in out.splitlines() if ":" in l}
    a, b = (int(x) for x in line["truncations"].split()[1:4:2])
    assert a == b and b > 1024  # every truncation is rejected
    fr, ft = (int(x) for x in line["fields"].split(",")[1].split()[0:3:2])
    mr = int(line["mutations"].split()[1])
    assert ft >= 4 * 40 and mr > 0
    assert a + fr + mr > (b + ft + 2000) // 2  # most loads are rejected


# ---- san_input -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def input_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostsan_input")
    text = b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in oracle.read_fasta(BCL2))
    (d / "plain.fasta").write_bytes(text)
    half = text.index(b"\n>", len(text) // 2) + 1
    (d / "two.fasta.gz").write_bytes(gzip.compress(text[:half]) + gzip.compress(text[half:]))  # two members
    (d / "text.fasta.bz2").write_bytes(bz2.compress(text))
    (d / "text.fasta.xz").write_bytes(lzma.compress(text, format=lzma.FORMAT_XZ))
    small = os.path.join(GOLDEN, "test_compression.fasta")
    big_zst = None  # the committed zstd fixture is 72 bytes: a larger archive is made where libzstd can be loaded
    try:
        import ctypes
        z = ctypes.CDLL("libzstd.so.1")
        z.ZSTD_compressBound.restype = z.ZSTD_compress.restype = ctypes.c_size_t
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
        buf = ctypes.create_string_buffer(z.ZSTD_compressBound(len(text)))
        n = z.ZSTD_compress(buf, len(buf), text, len(text), 3)
        if not z.ZSTD_isError(n):
            big_zst = d / "text.fasta.zst"
            big_zst.write_bytes(buf.raw[:n])
    except OSError:
        pass
    return {"zstd-made": (big_zst, d / "plain.fasta"), "plain": (d / "plain.fasta", d / "plain.fasta"), "gzip": (d / "two.fasta.gz", d / "plain.fasta"),
            "zstd": (small + ".zst", small), "bzip2": (d / "text.fasta.bz2", d / "plain.fasta"),
            "xz": (d / "text.fasta.xz", d / "plain.fasta")}


@pytest.mark.parametrize("fmt", ["plain", "gzip", "zstd", "zstd-made", "bzip2", "xz"])
def test_input_decompress(progs, input_files, tmp_path, fmt):
    """Whole file, >= 200 truncations and 500 seeded mutations per format (single-threaded: ASan + UBSan)."""
    path, plain = input_files[fmt]
    if path is None:
        print("skip zstd-made: libzstd.so.1 could not be loaded to make the archive")
        return
    fmt = fmt.split("-")[0]
    out = run(progs["asan"]["san_input"], [fmt, path, plain, tmp_path / "probe", 200, 500], timeout=25)  # measured: 0.3 - 2.5 s
    print(out)
    if out.startswith("skip"):
        return  # (the decompressor library is not on this machine: printed, as the product reports it)
    assert out.startswith(f"ok {fmt}:")
    cuts = int(out.split(";")[1].split()[0])
    assert cuts >= min(200, os.path.getsize(path)) and " 500 mutations" in out
