"""GPU: the rarely taken paths (KS_DEBUG_* knobs, max_seq_len hints) against the oracle.

- the sketch's ticket repeat (a look-back that gave up) on batches that repeat k-mers inside their sequences, so that the
  repeat has counts to get wrong: sketches, n_hashes, the dense view, postings and hits, k-mer positions;
- max_seq_len hints that are too small, through every entry that takes one and every plan that trusts one: refused with
  KS_ERR_INVALID_ARG, nothing leaked, the context still right afterwards; exact hints at the tile-size boundaries;
- the slab path and the copy of the deferred runs (ks_sketch_long.hip) on batches of three sequences: every branch of the two
  kernels, sketches against the oracle, their postings through the one-call sketch + search;
- the randomised differential test (tools/fuzz_parity.py) under every knob set, bit for bit against the oracle."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks
from kmerseek_amd import synth
from oracle import oracle

PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
PK_MAX_LEN = 4064  # longest sequence a packed tile holds (ks_sketch.hip, next to SK_MED_MAX)
SK_MED_MAX = 4080  # longest sequence that fits one tile on its own


def _seq_with_repeats(rng, n, run_max):
    """n residues full of repeated k-mers: homopolymer runs, tandem repeats, low-complexity stretches (each up to run_max
    residues), some plain protein."""
    out = []
    while sum(len(x) for x in out) < n:
        kind = int(rng.integers(0, 4))
        m = int(rng.integers(10, run_max))
        if kind == 0:
            out.append(np.full(m, rng.choice(PROTEIN), np.uint8))
        elif kind == 1:
            unit = rng.choice(PROTEIN, int(rng.integers(2, 13)))
            t = np.tile(unit, m // len(unit) + 1)[:m]
            mut = rng.random(m) < 0.02
            t[mut] = rng.choice(PROTEIN, int(mut.sum()))
            out.append(t)
        elif kind == 2:
            out.append(rng.choice(rng.choice(PROTEIN, int(rng.integers(2, 4)), replace=False), m))
        else:
            out.append(rng.choice(PROTEIN, m))
    return np.concatenate(out)[:n].astype(np.uint8)


def repeat_batch(seed, n=1500, run_max=200):
    """Proteome-like lengths with repeats everywhere, plus medium (4081-8000) and long (>= 9000) sequences among them.
    (The compacting tiles want shorter runs: a tile that keeps far more than 1 / scaled of its windows repeats the batch
    without them, and then the ticket repeat is not what produced the result.)"""
    rng = np.random.default_rng(seed)
    lens = list(np.clip(np.rint(rng.lognormal(np.log(260.0), 0.55, n)), 0, 3000).astype(int))
    for L in (4081, 5600, 8000, 9000, 14000):
        lens.insert(int(rng.integers(0, len(lens))), L)
    seqs = [_seq_with_repeats(rng, L, run_max) if L else np.zeros(0, np.uint8) for L in lens]
    offs = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return np.concatenate(seqs).astype(np.uint8), offs


def _eq(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{what}: array {i} differs"


def _maxlen(offs):
    return int((offs[1:] - offs[:-1]).max()) if len(offs) > 1 else 0


def _oracle_positions(res, offs, k, mol, want):
    o, mins, _ = want
    ws, wst, wh = [], [], []
    for i in range(len(offs) - 1):
        st, hh = oracle.kmer_positions(bytes(res[int(offs[i]):int(offs[i + 1])]), k, mol, mins[int(o[i]):int(o[i + 1])])
        ws.append(np.full(len(st), i, np.uint32)); wst.append(st); wh.append(hh)
    return np.concatenate(ws), np.concatenate(wst), np.concatenate(wh)


def _slice_sketches(want, lo, hi):
    o, m, a = want
    return (o[lo:hi + 1] - o[lo]), m[int(o[lo]):int(o[hi])], a[int(o[lo]):int(o[hi])]


# ---------------------------------------------------------------- B1: the ticket repeat on batches that repeat k-mers
SETTINGS = [("hp", 5, 1), ("hp", 7, 1), ("dayhoff", 16, 5), ("protein", 10, 1)]


@pytest.mark.parametrize("mol,k,scaled", SETTINGS)
def test_ticket_repeat_counts_repeated_kmers_once(monkeypatch, mol, k, scaled):
    """KS_DEBUG_FORCE_TICKET_RETRY: the shared-tile launch runs twice.  Every tile of the first attempt has already counted its
    repeated k-mers; the repeat must not count them again (n_hashes, the gapped -> dense gather), and the medium / long
    sequences' repeats, counted before the loop, must survive it."""
    res, offs = repeat_batch(100 + k, run_max=40 if scaled > 1 else 200)
    n = len(offs) - 1
    want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
    assert np.any(want[2] > 1), "the batch must repeat k-mers inside its sequences"
    total = len(want[1])
    n_t = 300
    t_want = _slice_sketches(want, 0, n_t)

    # sketch_batch -> n_hashes, index build from the gapped sketches, union, to_host
    c = ks.Context(0, follow_debug_env=True)
    try:
        monkeypatch.setenv("KS_DEBUG_FORCE_TICKET_RETRY", "1")
        S = c.sketch_batch(res, offs, k, scaled, mol)
        monkeypatch.delenv("KS_DEBUG_FORCE_TICKET_RETRY")
        st = c.sketch_stats()
        assert st["ticket_fallbacks"] == 1 and st["compact_fallbacks"] == 0 and st["cap_fallbacks"] == 0, st
        assert S.n_hashes == total
        ix = c.index_build(S)  # (gapped slots: made dense on the way)
        u, inv = np.unique(want[1], return_inverse=True)
        U = S.union().to_host()
        assert np.array_equal(U[0], np.array([0, len(u)], np.uint64)) and np.array_equal(U[1], u)
        assert np.array_equal(U[2].astype(np.int64), np.bincount(inv, weights=want[2].astype(np.float64)).astype(np.int64))
        _eq(S.to_host(), want, "sketches")
        # the index of the repeated sketches answers like the oracle (a sample of queries)
        qo, qm, qa = _slice_sketches(want, n - 40, n)
        H = c.search(ix, c.sketches_from_host(qo, qm, qa, k, scaled, mol)).to_host()
        _eq(H, oracle.manysearch(qo, qm, *want, n_threads=8), "hits against the repeated index")
    finally:
        c.close()

    # sketch_queries_device -> fused search (postings from the repeated launch), then a forced row-pass repeat
    c = ks.Context(0, follow_debug_env=True)
    try:
        T = c.sketch_batch(res[:int(offs[n_t])], offs[:n_t + 1], k, scaled, mol)
        ix = c.index_build(T)
        d_res, d_off = c.to_device(res), c.to_device(offs)
        monkeypatch.setenv("KS_DEBUG_FORCE_TICKET_RETRY", "1")
        Q = c.sketch_queries_device(ix, d_res.ptr, d_off.ptr, n, len(res), max_seq_len=_maxlen(offs))
        monkeypatch.delenv("KS_DEBUG_FORCE_TICKET_RETRY")
        st = c.sketch_stats()
        assert st["ticket_fallbacks"] == 1 and st["compact_fallbacks"] == 0 and st["cap_fallbacks"] == 0, st
        assert Q.n_hashes == total
        fused = c.search(ix, Q).to_host()
        monkeypatch.setenv("KS_DEBUG_FORCE_ROWS_TICKET_RETRY", "1")
        rows_repeat = c.search(ix, Q).to_host()
        monkeypatch.delenv("KS_DEBUG_FORCE_ROWS_TICKET_RETRY")
        assert c.search_stats()["rows_ticket_fallbacks"] == 1
        _eq(Q.to_host(), want, "query sketches")
    finally:
        c.close()
    c = ks.Context(0)
    try:
        plain = c.search(c.index_build(c.sketch_batch(res[:int(offs[n_t])], offs[:n_t + 1], k, scaled, mol)),
                         c.sketch_batch(res, offs, k, scaled, mol)).to_host()
    finally:
        c.close()
    _eq(fused, plain, "fused search after the repeat vs plain search")
    _eq(rows_repeat, plain, "row-pass repeat vs plain search")
    assert len(plain[0]) > 0
    rng = np.random.default_rng(k)
    for qi in rng.choice(n, 12, replace=False).tolist():
        qo, qm, _ = _slice_sketches(want, qi, qi + 1)
        w = oracle.manysearch(qo, qm, *t_want, n_threads=8)
        sel = plain[0] == qi
        for j in (1, 2, 3):
            assert np.array_equal(plain[j][sel], w[j]), f"query {qi}"

    # k-mer positions (the same repeat scheme: dispatch order, then tickets)
    c = ks.Context(0, follow_debug_env=True)
    try:
        monkeypatch.setenv("KS_DEBUG_FORCE_TICKET_RETRY", "1")
        got = c.kmer_positions(res, offs, k, scaled, mol)
        monkeypatch.delenv("KS_DEBUG_FORCE_TICKET_RETRY")
        assert c.sketch_stats()["ticket_fallbacks"] == 1
    finally:
        c.close()
    _eq(got, _oracle_positions(res, offs, k, mol, want), "k-mer positions")


def test_really_expired_lookback_on_repeated_kmers(monkeypatch):
    """KS_DEBUG_LOOKBACK_SKIP: a tile of the first attempt never publishes, its successors' spins expire (~2 s), and the
    repeat starts from a launch that did count repeats in every tile that ran."""
    mol, k, scaled = "dayhoff", 16, 5
    res, offs = repeat_batch(200, run_max=40)
    want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
    assert np.any(want[2] > 1)
    c = ks.Context(0, follow_debug_env=True)
    try:
        monkeypatch.setenv("KS_DEBUG_LOOKBACK_SKIP", "3")
        S = c.sketch_batch(res, offs, k, scaled, mol)
        monkeypatch.delenv("KS_DEBUG_LOOKBACK_SKIP")
        st = c.sketch_stats()
        assert st["ticket_fallbacks"] == 1 and st["uses_ticket"] == 1 and st["compact_fallbacks"] == 0, st
        assert S.n_hashes == len(want[1])
        _eq(S.to_host(), want, "sketches")
    finally:
        c.close()


# ---------------------------------------------------------------- B2: max_seq_len hints
# (plan: parameters, knobs) — the packed plan that trusts the hint for its tile count (pk_bound, hint <= PK_MAX_LEN), the
# packed plan that measures it (PLAN_SYNC), the plain-tile plan (NO_PACK) and the compacting plan (scaled > 1)
PLANS = {
    "pk_bound": ((10, 1, "protein"), {}),
    "plan_sync": ((10, 1, "protein"), {"KS_DEBUG_PLAN_SYNC": "1"}),
    "no_pack": ((10, 1, "protein"), {"KS_DEBUG_NO_PACK": "1"}),
    "compacting": ((16, 5, "dayhoff"), {}),
}


def _batch(lens, seed):
    rng = np.random.default_rng(seed)
    seqs = [rng.choice(PROTEIN, int(L)).astype(np.uint8) for L in lens]
    return ks.pack([bytes(s) for s in seqs])


def _short_with(extra, seed, n=400):
    rng = np.random.default_rng(seed)
    lens = list(rng.integers(20, 400, n))
    for L in extra:
        lens.insert(int(rng.integers(0, len(lens))), L)
    return _batch(lens, seed)


# (name, batch, hint)
def _hint_batches():
    out = [("long_vs_1000", _short_with([9000, 20000], 1), 1000),
           ("many_2k_4k_vs_100", _batch(np.random.default_rng(2).integers(2000, 4001, 300), 2), 100)]
    for real in (PK_MAX_LEN, PK_MAX_LEN + 1, SK_MED_MAX, SK_MED_MAX + 1):
        out.append((f"real_{real}_minus_1", _short_with([real, real, real], real), real - 1))
    return out


def _entries(ctx, ix, k, scaled, mol):
    return {
        "batch_device": lambda r, o, n, nr, h: ctx.sketch_batch_device(r, o, n, nr, k, scaled, mol, max_seq_len=h),
        "queries_device": lambda r, o, n, nr, h: ctx.sketch_queries_device(ix, r, o, n, nr, max_seq_len=h),
        "search_device": lambda r, o, n, nr, h: ctx.sketch_search_device(ix, r, o, n, nr, max_seq_len=h),
        "search_device_no_sketches": lambda r, o, n, nr, h: ctx.sketch_search_device(ix, r, o, n, nr, max_seq_len=h,
                                                                                      want_sketches=False),
    }


@pytest.mark.parametrize("plan", list(PLANS))
def test_too_small_max_seq_len_is_refused_everywhere(monkeypatch, plan):
    """A hint below the batch's longest sequence is refused with KS_ERR_INVALID_ARG (the deferred read-back of the one-call
    search included), returns every pool block it took, and leaves a context that sketches the batch right with the correct
    hint and without one.  Before the fix, the plans that deferred nothing on the hint's word read a null kept-count array."""
    (k, scaled, mol), env = PLANS[plan]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        t_res, t_off = synth.proteome(200, stream=500)
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
        entries = _entries(ctx, ix, k, scaled, mol)
        for name, (res, offs), hint in _hint_batches():
            real = _maxlen(offs)
            assert hint < real
            n, nr = len(offs) - 1, len(res)
            d_res, d_off = ctx.to_device(res), ctx.to_device(offs)
            for entry, call in entries.items():  # (first with the true bound: whatever the context keeps is in use from here on)
                out = call(d_res.ptr, d_off.ptr, n, nr, real)
                del out
            for entry, call in entries.items():
                before = ctx.pool_stats()["bytes_in_use"]
                with pytest.raises(ks.KmerseekError) as e:
                    call(d_res.ptr, d_off.ptr, n, nr, hint)
                assert "max_seq_len" in str(e.value), (plan, name, entry, str(e.value))
                assert ctx.pool_stats()["bytes_in_use"] == before, (plan, name, entry)
            want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
            for h in (real, 0):
                S = ctx.sketch_batch_device(d_res.ptr, d_off.ptr, n, nr, k, scaled, mol, max_seq_len=h)
                _eq(S.to_host(), want, f"{plan} {name} hint {h}")
                S.free()
            d_res.free(); d_off.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("plan", list(PLANS))
def test_exact_max_seq_len_at_the_tile_boundaries(monkeypatch, plan):
    """Exact hints around PK_MAX_LEN and SK_MED_MAX (where the pk_bound plan gives way to the measured one, and a sequence
    stops fitting a tile of its own): sketches and hits of every entry equal the oracle."""
    (k, scaled, mol), env = PLANS[plan]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        t_res, t_off = synth.proteome(200, stream=501)
        T = ctx.sketch_batch(t_res, t_off, k, scaled, mol)
        ix = ctx.index_build(T)
        t_want = oracle.sketch_batch(t_res, t_off, k, scaled, mol, n_threads=8)
        entries = _entries(ctx, ix, k, scaled, mol)
        for real in (PK_MAX_LEN - 1, PK_MAX_LEN, PK_MAX_LEN + 1, SK_MED_MAX - 1, SK_MED_MAX, SK_MED_MAX + 1):
            # the longest ones among short sequences and proteins that share k-mers with the targets
            res, offs = _short_with([real, real - 7, real], real, n=150)
            seqs = [bytes(res[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
            seqs += [bytes(t_res[int(t_off[i]):int(t_off[i + 1])]) for i in range(0, 200, 20)]
            res, offs = ks.pack(seqs)
            assert _maxlen(offs) == real
            n, nr = len(offs) - 1, len(res)
            want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
            hits = oracle.manysearch(want[0], want[1], *t_want, n_threads=8)
            d_res, d_off = ctx.to_device(res), ctx.to_device(offs)
            for entry, call in entries.items():
                out = call(d_res.ptr, d_off.ptr, n, nr, real)
                S, H = (out, None) if entry in ("batch_device", "queries_device") else out
                if S is not None:
                    _eq(S.to_host(), want, f"{plan} real {real} {entry}")
                if H is not None:
                    _eq(H.to_host(), hits, f"{plan} real {real} {entry} hits")
            d_res.free(); d_off.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------- B2b: the slab path and the deferred runs, three sequences
# One sequence beyond SK_MED_MAX (the slab path: k_sketch_long, then k_place_long with its postings), one of 4,070 residues
# (a tile of its own under plain tiles: the copy-only k_place_long launch) and a short one.  "homopolymer": the long one
# repeats one k-mer 4,991 / 4,985 times — kept != distinct, so the slab path adds to the drop count and its flag scan has
# gaps to close ('E' because its dayhoff 16-mer passes the threshold at scaled = 5).  The sequences are cut from the targets
# (and the targets hold a run of E) so that every query has hits and the long sequences' postings carry them.
LONG_SETTINGS = {"protein": ("protein", 10, 1), "dayhoff": ("dayhoff", 16, 5)}
# way -> (knobs, max_seq_len given).  At scaled = 5 the compacting tiles span 19,200 residues and defer none of these
# sequences (only the homopolymer batch, whose tile overflows, is repeated without them): NO_COMPACT takes the dayhoff
# batches to the same two kernels.
LONG_WAYS = {
    "plain": ({}, False),
    "hint": ({}, True),
    "no_pack": ({"KS_DEBUG_NO_PACK": "1"}, False),
    "hint_no_pack": ({"KS_DEBUG_NO_PACK": "1"}, True),  # lists sized by upper bounds, longer than what is listed
    "no_compact": ({"KS_DEBUG_NO_COMPACT": "1"}, False),
    "no_compact_no_pack": ({"KS_DEBUG_NO_COMPACT": "1", "KS_DEBUG_NO_PACK": "1"}, False),
}
_long_cache = {}


def _assert_long_launches(timing, setting, batch, knobs, what):
    """The launches of the slab path and of the deferred copies ran (Context.timing): a case that stops reaching them fails."""
    scaled = LONG_SETTINGS[setting][2]
    long_path = scaled == 1 or "KS_DEBUG_NO_COMPACT" in knobs or batch == "homopolymer"
    medium = long_path and "KS_DEBUG_NO_PACK" in knobs  # plain tiles: the 4,070 residues end outside their shared tile
    if long_path:
        assert "sketch_long" in timing and timing.get("place_long", (0, 0.0))[0] >= 1 + medium, (what, timing)
    if medium:
        assert "sketch_medium" in timing, (what, timing)


def _long_targets():
    if "t" not in _long_cache:
        t_res, t_off = synth.proteome(200, stream=77)
        seqs = [bytes(t_res[int(t_off[i]):int(t_off[i + 1])]) for i in range(200)]
        seqs.insert(100, seqs[3][:50] + b"E" * 40 + seqs[4][:50])
        _long_cache["t"] = ks.pack(seqs)
    return _long_cache["t"]


def _long_case(batch, setting):
    """(query batch, target batch, oracle query sketches, oracle target sketches, oracle hits), computed once per pair"""
    key = (batch, setting)
    if key not in _long_cache:
        mol, k, scaled = LONG_SETTINGS[setting]
        t_res, t_off = _long_targets()
        first = b"E" * 5000 if batch == "homopolymer" else bytes(t_res[:5000])
        q = ks.pack([first, bytes(t_res[6000:6000 + 4070]), bytes(t_res[int(t_off[50]):int(t_off[50]) + 30])])
        assert [int(x) for x in q[1][1:] - q[1][:-1]] == [5000, 4070, 30]
        wq = oracle.sketch_batch(q[0], q[1], k, scaled, mol, n_threads=4)
        wt = oracle.sketch_batch(t_res, t_off, k, scaled, mol, n_threads=4)
        _long_cache[key] = (q, (t_res, t_off), wq, wt, oracle.manysearch(wq[0], wq[1], *wt, n_threads=4))
    return _long_cache[key]


@pytest.mark.parametrize("way", list(LONG_WAYS))
@pytest.mark.parametrize("setting", list(LONG_SETTINGS))
@pytest.mark.parametrize("batch", ["random", "homopolymer"])
def test_long_and_medium_sequences_of_a_three_sequence_batch(monkeypatch, batch, setting, way):
    """Sketches equal the oracle's exactly, whichever of the plans takes the 5,000- and the 4,070-residue sequence."""
    mol, k, scaled = LONG_SETTINGS[setting]
    knobs, hint = LONG_WAYS[way]
    (res, offs), _, want, _, _ = _long_case(batch, setting)
    if batch == "homopolymer":
        assert int(want[2][0]) == 5000 - k + 1 and int(want[0][1]) == 1  # the long sequence: one hash, kept 5000 - k + 1 times
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        d_res, d_off = ctx.to_device(res), ctx.to_device(offs)
        ctx.timing_enable(True)
        S = ctx.sketch_batch_device(d_res.ptr, d_off.ptr, 3, len(res), k, scaled, mol, max_seq_len=5000 if hint else 0)
        assert S.n_hashes == len(want[1])
        _eq(S.to_host(), want, f"{batch} {setting} {way}")
        _assert_long_launches(ctx.timing(), setting, batch, knobs, f"{batch} {setting} {way}")
    finally:
        ctx.close()


# 10-byte postings need a join on more than 8 prefix bits whose prefix is a bit field of the hash (scaled = 1), against an
# index in the fingerprint layout: small buckets make the 201-protein index one.  At scaled = 5 the same knobs leave 12 bytes.
LONG_POSTINGS = {
    "12": {},
    "10": {"KS_DEBUG_JOIN_FP": "1", "KS_DEBUG_BUCKET": "64"},
}


@pytest.mark.parametrize("fmt", list(LONG_POSTINGS))
@pytest.mark.parametrize("setting,no_compact", [("protein", False), ("dayhoff", False), ("dayhoff", True)])
@pytest.mark.parametrize("batch", ["random", "homopolymer"])
def test_long_sequences_as_queries_of_the_one_call_search(monkeypatch, batch, setting, no_compact, fmt):
    """The same batches as the query side of ks_sketch_search_device: the long sequence's postings come from k_place_long, in
    the 12-byte and in the 10-byte form.  Hits equal those of the two calls (sketch_batch, which makes no postings, then
    search) and the oracle's; with and without max_seq_len."""
    mol, k, scaled = LONG_SETTINGS[setting]
    (res, offs), (t_res, t_off), want, _, want_hits = _long_case(batch, setting)
    assert set(want_hits[0].tolist()) == {0, 1, 2}, "every query must have hits"
    for key, v in LONG_POSTINGS[fmt].items():
        monkeypatch.setenv(key, v)
    if no_compact:
        monkeypatch.setenv("KS_DEBUG_NO_COMPACT", "1")
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        ix = ctx.index_build(ctx.sketch_batch(t_res, t_off, k, scaled, mol))
        two_calls = ctx.search(ix, ctx.sketch_batch(res, offs, k, scaled, mol)).to_host()
        _eq(two_calls, want_hits, f"{batch} {setting} two calls vs oracle")
        d_res, d_off = ctx.to_device(res), ctx.to_device(offs)
        for bound in (5000, 0):
            ctx.timing_enable(True)
            ctx.timing_reset()
            Q, H = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, 3, len(res), max_seq_len=bound)
            _assert_long_launches(ctx.timing(), setting, batch, {"KS_DEBUG_NO_COMPACT": "1"} if no_compact else {},
                                  f"{batch} {setting} {fmt} bound {bound}")
            assert Q.posting_bytes == (10 if fmt == "10" and scaled == 1 else 12)
            assert H.partition_path != 3, "the search must read the sketch's postings"
            _eq(Q.to_host(), want, f"{batch} {setting} {fmt} bound {bound} sketches")
            _eq(H.to_host(), two_calls, f"{batch} {setting} {fmt} bound {bound} hits")
            Q.free(); H.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------- B3: the randomised differential test under every knob set
def _fuzz():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
    spec = importlib.util.spec_from_file_location("fuzz_parity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# name -> (knobs without the KS_DEBUG_ prefix, counter that must show the path was taken or None)
KNOB_SETS = {
    # the forced-path configurations of tools/gpu/fuzz_campaign.sh
    "key_columns": ({"JOIN_FP": "0"}, None),
    "key_columns_split": ({"JOIN_FP": "0", "JOIN_SPLIT": "3"}, None),
    "fp_staged": ({"JOIN_FP": "1", "JOIN_SPARSE": "0"}, None),
    "fp_sparse": ({"JOIN_FP": "1", "JOIN_SPARSE": "1"}, None),
    "fp_sparse_segs_coarse": ({"JOIN_FP": "1", "JOIN_SPARSE": "1", "JOIN_SEGS": "1", "FP_COARSEN": "18"}, None),
    "fp_staged_segs_coarse": ({"JOIN_FP": "1", "JOIN_SPARSE": "0", "JOIN_SEGS": "1", "FP_COARSEN": "10"}, None),
    "rows_ticket_planless": ({"ROWS_TICKET": "1", "NO_PLAN": "1"}, None),
    "nocompact_nopack": ({"NO_COMPACT": "1", "NO_PACK": "1"}, None),
    "lsd_paths": ({"PAIRS_LSD": "1", "INDEX_LSD": "1"}, None),
    "full_lists": ({"QCAP": "2"}, None),
    "nopack": ({"NO_PACK": "1"}, None),
    "nopack_full_lists": ({"NO_PACK": "1", "QCAP": "1"}, None),
    "nine_byte_buckets": ({"JOIN_FP": "1", "BUCKET": "64"}, None),
    # the forced repeats (a fresh context per case: a context that repeated once draws tickets from then on)
    "ticket_retry": ({"FORCE_TICKET_RETRY": "1"}, "ticket_fallbacks"),
    "rows_ticket_retry": ({"FORCE_ROWS_TICKET_RETRY": "1"}, "rows_ticket_fallbacks"),
    # knobs no other test forces (values inside the ranges their parsers accept)
    "staged_h2d": ({"STAGED_H2D": "1"}, None),
    "scan_3pass": ({"SCAN_3PASS": "1"}, None),
    "pbits_max": ({"PBITS_MAX": "4"}, None),
    "rows_ticket": ({"ROWS_TICKET": "1"}, None),
    "no_plan": ({"NO_PLAN": "1"}, None),
    "no_compact": ({"NO_COMPACT": "1"}, None),
    "span": ({"SPAN": "6144"}, None),            # compacting tiles: a multiple of 512 in [4096, 3840 * min(scaled, 64)]
    "plan_sync": ({"PLAN_SYNC": "1"}, None),
    "tile_r": ({"TILE_R": "2800", "NO_PLAN": "1"}, None),  # one of the counted strides; read only by a measured plan
    "sync_api": ({"SYNC_API": "1"}, None),
    "subshift": ({"SUBSHIFT": "2", "BUCKET": "64"}, None),  # 0..3, applies above 8 prefix bits (small buckets: more bits)
}


@pytest.mark.parametrize("name", list(KNOB_SETS))
def test_fuzz_under_knob_set(name):
    knobs, counter = KNOB_SETS[name]
    stats = {}
    seed = 7000 + list(KNOB_SETS).index(name)
    fz = _fuzz()
    assert fz.run(25, seed, knobs=knobs, entries=True, ctx_per_case=name.endswith("retry"), stats=stats) == 0
    if counter:
        assert stats[counter] >= 1, stats
    if name == "staged_h2d":  # (only host batches of >= 4 MiB take the staged copy)
        assert fz.run_staged_copy(seed, knobs) == 0
