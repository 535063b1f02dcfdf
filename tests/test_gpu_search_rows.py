"""GPU: the search options — per-row abundance statistics (KS_SEARCH_ABUND_STATS) and the containment filter
(min_containment) — through ks_search_ex, ks_sketch_search_ex and ks_sketch_search_device_ex, on gapped query batches.

- the statistics equal a pure-Python replica of the host's sequential f64 loops bit for bit (median = median2 / 2,
  std = sqrt(ss / n), ss itself), and oracle.manysearch_row to rel 1e-12;
- the four plain columns are those of ks_search, with or without the statistics;
- a threshold keeps exactly the rows the host's f64 test keeps, in (qid, tid) order;
- the same under the forced paths (LSD match sort, small MSD buckets, query slices by record width and by pair count,
  no rows hint, the row pass's ticket repeat, ticket-ordered tiles);
- a row pass that is repeated with statistics and threshold both on (more rows than the context's hint; a forced ticket repeat)
  gives the same rows and leaves no pool block behind;
- the object API (PyProteomeIndex.search_sequences / search_fasta) computes its abundance columns on the device, and its
  threshold keeps the rows with containment >= threshold, in the rows and in the CSV."""
import csv
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import host, synth
from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crafted_sketches import keep as _keep, replica as _replica  # noqa: E402  (the host's row loop and keep test live there)
from crafted_sketches import ref_join as _ref_join, ref_stats as _ref_stats  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
THRESHOLDS = (0.0, 1e-300, 0.05, 0.5, 1.0, 1.5)
ENTRIES = ("search", "sketch_search", "sketch_search_device")


def _repeats(rng, n):
    """n residues full of repeated k-mers (homopolymer runs, tandem repeats, low-complexity stretches, plain protein)."""
    out, m_tot = [], 0
    while m_tot < n:
        kind, m = int(rng.integers(0, 4)), int(rng.integers(10, 120))
        if kind == 0:
            out.append(np.full(m, rng.choice(PROTEIN), np.uint8))
        elif kind == 1:
            unit = rng.choice(PROTEIN, int(rng.integers(2, 9)))
            out.append(np.tile(unit, m // len(unit) + 1)[:m])
        elif kind == 2:
            out.append(rng.choice(rng.choice(PROTEIN, 3, replace=False), m))
        else:
            out.append(rng.choice(PROTEIN, m))
        m_tot += m
    return np.concatenate(out)[:n].astype(np.uint8)


def _repeat_batch(seed, n, long_lens=()):
    rng = np.random.default_rng(seed)
    lens = list(np.clip(np.rint(rng.lognormal(np.log(400.0), 0.8, n)), 20, 6000).astype(int)) + list(long_lens)
    return ks.pack([bytes(_repeats(rng, int(L))) for L in lens])


def _split(res, offs, a, b):
    return res[int(offs[a]):int(offs[b])], (offs[a:b + 1] - offs[a]).astype(np.uint64)


def _case(name):
    """(t_res, t_offs, q_res, q_offs, k, scaled, mol)"""
    if name in ("hp5", "hp7"):  # abundances into the hundreds (a 12k-residue target: ~375 per hp 5-mer), odd and even sizes
        res, offs = _repeat_batch(5, 150, long_lens=(12000, 9000))
        t = _split(res, offs, 0, 100)
        q = _split(res, offs, 70, 152)
        return t + q + ((5, 1, "hp") if name == "hp5" else (7, 1, "hp"))
    if name == "protein10":
        t_res, t_off = synth.proteome(600, stream=811)
        q_res, q_off = synth.queries(400, t_res, t_off, stream=812)
        r2, o2 = _repeat_batch(13, 40)
        q_res, q_off = ks.pack([bytes(q_res[int(q_off[i]):int(q_off[i + 1])]) for i in range(400)] +
                               [bytes(r2[int(o2[i]):int(o2[i + 1])]) for i in range(40)])
        return t_res, t_off, q_res, q_off, 10, 1, "protein"
    if name == "dayhoff16s5":
        res, offs = _repeat_batch(16, 300, long_lens=(8000,))
        return _split(res, offs, 0, 200) + _split(res, offs, 120, 301) + (16, 5, "dayhoff")
    if name == "bcl2":
        recs = oracle.read_fasta(os.path.join(GOLDEN, "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"))
        seqs = [s.upper() for _, s in recs]
        t_res, t_off = ks.pack(seqs)
        q_res, q_off = ks.pack(seqs[::-1])
        return t_res, t_off, q_res, q_off, 10, 1, "dayhoff"
    if name == "self30k":  # one ~30k-residue sequence against itself at scaled=1: a row of ~30k records
        rng = np.random.default_rng(30)
        big = np.concatenate([rng.choice(PROTEIN, 26000), _repeats(rng, 4000)]).astype(np.uint8)
        small = [bytes(big[i:i + 300]) for i in range(0, 3000, 500)]
        t_res, t_off = ks.pack(small + [bytes(big)])
        q_res, q_off = ks.pack([bytes(big)] + small[:3])
        return t_res, t_off, q_res, q_off, 10, 1, "protein"
    raise KeyError(name)


def _sketches(res, offs, k, scaled, mol):
    o, m, a = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
    return o, m, a


def _run(ctx, entry, ix, q_res, q_offs, k, scaled, mol, **kw):
    """The rows ((qid, tid, isect, nw), Hits) of one entry point."""
    if entry == "search":
        H = ctx.search(ix, ctx.sketch_batch(q_res, q_offs, k, scaled, mol), **kw)
    elif entry == "sketch_search":
        _, H = ctx.sketch_search(ix, q_res, q_offs, want_sketches=False, **kw)
    else:
        d_res, d_off = ctx.to_device(q_res if len(q_res) else np.zeros(1, np.uint8)), ctx.to_device(q_offs)
        _, H = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, len(q_offs) - 1, len(q_res), want_sketches=False, **kw)
    return H.to_host(), H


def _check_stats(rows, H, qs, ts, label, n_oracle=40):
    assert H.has_abund_stats
    median2, ss = H.abund_stats_to_host()
    qid, tid, isect, nw = rows
    assert len(median2) == len(qid)
    qo, qm, _ = qs
    to, tm, ta = ts
    odd = even = 0
    for r in range(len(qid)):
        q, t = int(qid[r]), int(tid[r])
        q_mins = qm[int(qo[q]):int(qo[q + 1])]
        t_mins, t_ab = tm[int(to[t]):int(to[t + 1])], ta[int(to[t]):int(to[t + 1])]
        n, mean, median, want_ss = _replica(q_mins, t_mins, t_ab)
        assert n == isect[r], (label, r)
        assert float(median2[r]) / 2.0 == median, (label, r, int(median2[r]), median)
        assert ss[r] == want_ss, (label, r, float(ss[r]), want_ss)
        assert math.sqrt(ss[r] / n) == math.sqrt(want_ss / n)
        assert float(nw[r]) / n == mean, (label, r)  # the host's average_abund
        odd += n % 2
        even += 1 - n % 2
    if label[0] in ("hp5", "hp7"):
        assert odd and even, label
    for r in np.linspace(0, len(qid) - 1, min(n_oracle, len(qid))).astype(int).tolist():
        q, t = int(qid[r]), int(tid[r])
        w = oracle.manysearch_row("q", qm[int(qo[q]):int(qo[q + 1])], "t", tm[int(to[t]):int(to[t + 1])],
                                  ta[int(to[t]):int(to[t + 1])], 10, 1, "protein")
        n = int(isect[r])
        assert math.isclose(float(median2[r]) / 2.0, w["median_abund"], rel_tol=1e-12), (label, r)
        assert math.isclose(math.sqrt(ss[r] / n), w["std_abund"], rel_tol=1e-12, abs_tol=1e-300), (label, r)
        assert math.isclose(float(nw[r]) / n, w["average_abund"], rel_tol=1e-12), (label, r)
    return median2, ss


def _eq_rows(got, want, label):
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (label, j, len(g), len(w))


def _check_thresholds(ctx, entry, ix, case, plain, stats, qs, label):
    t_res, t_off, q_res, q_off, k, scaled, mol = case
    assert any(0 < _keep(plain, qs, thr).sum() < len(plain[0]) for thr in THRESHOLDS), label
    for thr in THRESHOLDS:
        sel = _keep(plain, qs, thr)
        for with_stats in (False, True):
            rows, H = _run(ctx, entry, ix, q_res, q_off, k, scaled, mol, min_containment=thr, abund_stats=with_stats)
            _eq_rows(rows, [a[sel] for a in plain], (label, thr, with_stats))
            if with_stats:
                m2, ss = H.abund_stats_to_host()
                assert np.array_equal(m2, stats[0][sel]) and np.array_equal(ss, stats[1][sel]), (label, thr)
            else:
                assert not H.has_abund_stats
        if thr == 0.0:
            assert sel.all()
        if thr == 1.5:
            assert not sel.any() and len(rows[0]) == 0


_CASES = {}


def _prepared(name):
    if name not in _CASES:
        case = _case(name)
        t_res, t_off, q_res, q_off, k, scaled, mol = case
        _CASES[name] = (case, _sketches(t_res, t_off, k, scaled, mol), _sketches(q_res, q_off, k, scaled, mol))
    return _CASES[name]


@pytest.mark.parametrize("name", ["hp5", "hp7", "protein10", "dayhoff16s5", "bcl2", "self30k"])
def test_stats_match_the_host_replica(name):
    case, ts, qs = _prepared(name)
    t_res, t_off, q_res, q_off, k, scaled, mol = case
    with ks.Context(0) as ctx:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
        Q = ctx.sketch_batch(q_res, q_off, k, scaled, mol)
        plain = ctx.search(ix, Q).to_host()
        assert len(plain[0]) > 0
        _eq_rows(plain, oracle.manysearch(qs[0], qs[1], *ts, n_threads=8), (name, "oracle"))
        if name == "self30k":
            assert plain[2].max() > 25000
        for entry in ENTRIES:
            rows, H = _run(ctx, entry, ix, q_res, q_off, k, scaled, mol, abund_stats=True)
            _eq_rows(rows, plain, (name, entry))
            _check_stats(rows, H, qs, ts, (name, entry))


@pytest.mark.parametrize("name", ["hp5", "protein10", "dayhoff16s5"])
def test_threshold_keeps_the_rows_of_the_host_test(name):
    case, ts, qs = _prepared(name)
    t_res, t_off, q_res, q_off, k, scaled, mol = case
    with ks.Context(0) as ctx:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
        plain = ctx.search(ix, ctx.sketch_batch(q_res, q_off, k, scaled, mol)).to_host()
        rows, H = _run(ctx, "search", ix, q_res, q_off, k, scaled, mol, abund_stats=True)
        stats = H.abund_stats_to_host()
        for entry in ENTRIES:
            _check_thresholds(ctx, entry, ix, case, plain, stats, qs, (name, entry))


def _knobs(name):
    case, ts, qs = _prepared(name)
    n_t = len(ts[0]) - 1
    tbits, abits = (n_t - 1).bit_length(), int(ts[2].max()).bit_length()
    return [{"KS_DEBUG_PAIRS_LSD": "1"}, {"KS_DEBUG_MSD_LDS_CAP": "64"}, {"KS_DEBUG_RECORD_BITS": str(tbits + abits + 4)},
            {"KS_DEBUG_PAIR_LIMIT": "PAIRS/3"}, {"KS_DEBUG_NO_ROWS_HINT": "1"}, {"KS_DEBUG_FORCE_ROWS_TICKET_RETRY": "1"},
            {"KS_DEBUG_ROWS_TICKET": "1"}]


@pytest.mark.parametrize("name", ["hp5", "hp7", "protein10"])
@pytest.mark.parametrize("knob", range(7))
def test_forced_paths(monkeypatch, name, knob):
    case, ts, qs = _prepared(name)
    t_res, t_off, q_res, q_off, k, scaled, mol = case
    env = dict(_knobs(name)[knob])
    with ks.Context(0) as ctx:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
        base = ctx.search(ix, ctx.sketch_batch(q_res, q_off, k, scaled, mol))
        plain = base.to_host()
        rows, H = _run(ctx, "search", ix, q_res, q_off, k, scaled, mol, abund_stats=True)
        stats = H.abund_stats_to_host()
        pairs = base.n_pair_instances
    if env.get("KS_DEBUG_PAIR_LIMIT") == "PAIRS/3":
        env["KS_DEBUG_PAIR_LIMIT"] = str(pairs // 3)
    if name != "protein10":
        assert pairs >= 65536  # (the MSD match sort is the default path of these lists)
    for entry in ENTRIES:
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        ctx = ks.Context(0, follow_debug_env=True)  # (fresh: the row pass's ticket repeat happens once per context)
        try:
            ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
            rows, H = _run(ctx, entry, ix, q_res, q_off, k, scaled, mol, abund_stats=True)
            _eq_rows(rows, plain, (name, env, entry))
            m2, ss = H.abund_stats_to_host()
            assert np.array_equal(m2, stats[0]) and np.array_equal(ss, stats[1]), (name, env, entry)
            if "KS_DEBUG_FORCE_ROWS_TICKET_RETRY" in env:
                assert ctx.search_stats()["rows_ticket_fallbacks"] == 1
            for thr in (0.05, 0.5, 1.5):
                sel = _keep(plain, qs, thr)
                rows, H = _run(ctx, entry, ix, q_res, q_off, k, scaled, mol, min_containment=thr, abund_stats=True)
                _eq_rows(rows, [a[sel] for a in plain], (name, env, entry, thr))
                m2, ss = H.abund_stats_to_host()
                assert np.array_equal(m2, stats[0][sel]) and np.array_equal(ss, stats[1][sel]), (name, env, entry, thr)
        finally:
            ctx.close()
            for key in env:
                monkeypatch.delenv(key)


def test_invalid_options_with_a_context():
    with ks.Context(0) as ctx:
        res, offs = synth.proteome(50, stream=5)
        ix = ctx.index_build(ctx.sketch_batch(res, offs, 10, 1, "protein"))
        Q = ctx.sketch_batch(res, offs, 10, 1, "protein")
        for bad in (-0.1, math.nan, -math.inf):
            with pytest.raises(ks.KmerseekError) as e:
                ctx.search(ix, Q, min_containment=bad)
            assert e.value.status == ks._lib.KS_ERR_INVALID_ARG and "min_containment" in str(e.value)
            with pytest.raises(ks.KmerseekError):
                ctx.sketch_search(ix, res, offs, min_containment=bad)
        plain = ctx.search(ix, Q)
        assert not plain.has_abund_stats
        with pytest.raises(ks.KmerseekError):
            plain.abund_stats_to_host()
        # an empty query batch and a query without hashes: no rows, the statistics columns exist (empty)
        e_res, e_off = ks.pack([b"AC"])
        H = ctx.search(ix, ctx.sketch_batch(e_res, e_off, 10, 1, "protein"), abund_stats=True, min_containment=0.5)
        assert H.count == 0 and H.has_abund_stats and all(len(a) == 0 for a in H.abund_stats_to_host())
        _eq_rows(ctx.search(ix, Q).to_host(), plain.to_host(), "context still fine")


def test_object_api_rows_and_threshold(tmp_path):
    case, ts, qs = _prepared("hp5")
    t_res, t_off, q_res, q_off, k, scaled, mol = case
    t_recs = [(bytes(t_res[int(t_off[i]):int(t_off[i + 1])]).decode(), f"t{i}") for i in range(len(t_off) - 1)]
    q_recs = [(bytes(q_res[int(q_off[i]):int(q_off[i + 1])]).decode(), f"q{i}") for i in range(len(q_off) - 1)]
    p = host.PyProteomeIndex(k, scaled, mol, str(tmp_path / "rows.db"))
    assert 0 < p.sketch_sequences(t_recs) <= len(t_recs)  # (signatures with equal sketches are stored once)
    rows = p.search_sequences(q_recs)
    assert len(rows) > 1000
    tmap = {n: i for i, (_, n) in enumerate(t_recs)}
    qmap = {n: i for i, (_, n) in enumerate(q_recs)}
    qo, qm, _ = qs
    to, tm, ta = ts
    for r in rows:
        q, t = qmap[r["query_name"]], tmap[r["match_name"]]
        n, mean, median, ss = _replica(qm[int(qo[q]):int(qo[q + 1])], tm[int(to[t]):int(to[t + 1])], ta[int(to[t]):int(to[t + 1])])
        assert r["intersect_hashes"] == n
        assert r["average_abund"] == mean and r["median_abund"] == median and r["std_abund"] == math.sqrt(ss / n), r
    fasta = tmp_path / "q.fasta"
    fasta.write_text("".join(f">{n}\n{s}\n" for s, n in q_recs))
    assert p.search_fasta(str(fasta)) == rows
    assert any(0 < sum(r["containment"] >= thr for r in rows) < len(rows) for thr in (0.05, 0.5, 1.0))
    for thr in (0.05, 0.5, 1.0):
        want = [r for r in rows if r["containment"] >= thr]
        assert p.search_sequences(q_recs, threshold=thr) == want
        out = tmp_path / f"rows_{thr}.csv"
        assert p.search_fasta(str(fasta), output=str(out), threshold=thr) == want
        back = list(csv.DictReader(open(out)))
        assert [(b["query_name"], b["match_name"]) for b in back] == [(w["query_name"], w["match_name"]) for w in want]
    assert p.search_sequences(q_recs, threshold=1.5) == []
    with pytest.raises(Exception, match="min_containment"):
        p.search_sequences(q_recs, threshold=-1.0)


# ---- a repeated row pass with both extras on: hand-made sketches (ks_sketches_from_host), exact against the numpy join ----
H0 = 0x9E3779B97F4A7C15  # the hash every sketch of the 80 x 80 case holds


def _square(n=80):
    """n targets and n queries that all hold H0, and one private hash each (targets: odd ones, queries: even ones, so no other
    hash is shared); target t holds H0 with abundance t + 1.  Every (query, target) pair is a row of one shared hash: n * n rows,
    each with containment 1 / 2, median2 = 2 * (t + 1) and ss = 0."""
    offs = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    t_h, q_h = np.empty(2 * n, np.uint64), np.empty(2 * n, np.uint64)
    t_h[0::2], q_h[0::2] = 2 * np.arange(n) + 1, 2 * np.arange(n) + 2  # (all below H0: ascending inside a sketch)
    t_h[1::2] = q_h[1::2] = H0
    t_ab = np.ones(2 * n, np.uint32)
    t_ab[1::2] = np.arange(n) + 1
    T, Q = (offs, t_h, t_ab), (offs.copy(), q_h, np.ones(2 * n, np.uint32))
    rows = _ref_join(T, Q)
    assert len(rows[0]) == n * n and np.all(rows[2] == 1)
    sel = _keep(rows, Q, 0.5)
    assert sel.all()  # (1 / 2 >= 0.5: the filter runs and keeps every row)
    m2, ss = _ref_stats(rows, T, Q)
    assert np.array_equal(m2, 2 * (rows[1].astype(np.uint64) + 1)) and not ss.any()
    return T, Q, [a[sel] for a in rows], m2[sel], ss[sel]


def _search_both_extras(ctx, case, label):
    """the 80 x 80 search with threshold and statistics on `ctx`, held against the replica's kept rows; the pool is back where it
    was before the search once the result is freed"""
    T, Q, rows, m2, ss = case
    dT, dQ = ctx.sketches_from_host(*T, 10, 1, "protein"), ctx.sketches_from_host(*Q, 10, 1, "protein")
    ix = ctx.index_build(dT)
    before = ctx.pool_stats()["bytes_in_use"]
    H = ctx.search(ix, dQ, min_containment=0.5, abund_stats=True)
    assert H.count == len(rows[0]) == 6400, (label, H.count)
    _eq_rows(H.to_host(), rows, label)
    got_m2, got_ss = H.abund_stats_to_host()
    assert np.array_equal(got_m2, m2) and np.array_equal(got_ss, ss), label
    H.free()
    assert ctx.pool_stats()["bytes_in_use"] == before, label


def test_rows_cap_repeat_with_stats_and_threshold():
    """The first search of the context yields one row, so the second one's row arrays are sized for 1 + 0 + 4096 rows: its 6,400
    rows do not fit, and the row pass, the statistics and the filter run a second time with exact arrays."""
    case = _square()
    with ks.Context(0) as ctx:
        one = (np.array([0, 1], np.uint64), np.array([H0], np.uint64), np.ones(1, np.uint32))
        d1 = ctx.sketches_from_host(*one, 10, 1, "protein")
        H1 = ctx.search(ctx.index_build(d1), d1)
        assert H1.count == 1
        ctx.timing_enable(True)
        _search_both_extras(ctx, case, "rows-cap repeat")
        assert ctx.timing()["pair_rows"][0] == 2  # (the pass did run twice)


def test_forced_ticket_repeat_with_stats_and_threshold(monkeypatch):
    case = _square()
    monkeypatch.setenv("KS_DEBUG_FORCE_ROWS_TICKET_RETRY", "1")
    ctx = ks.Context(0, follow_debug_env=True)  # (fresh: the first search of the context repeats its row pass with tickets)
    try:
        _search_both_extras(ctx, case, "ticket repeat")
        assert ctx.search_stats()["rows_ticket_fallbacks"] == 1
    finally:
        ctx.close()
