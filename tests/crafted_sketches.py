"""Hand-made sketches for the search half, and plain numpy / Python references for what it computes on them.

Every other search test starts from residues, so every hash it ever saw came out of MurmurHash3 and every abundance was a
window count.  The families here are valid inputs of ks_sketches_from_host (strictly ascending per sequence,
0 < h <= max_hash(scaled)) that sit on the edges of the search arithmetic instead: hashes on the join-bucket boundaries, all
postings in one bucket, buckets of one key, consecutive integers, match records that use all 64 bits, abundances 0 and
2^32 - 1, abundance sums around the union's saturation point, rows whose lengths sit on the thresholds of the lane / wave
row splits.  Each family asserts its own property while it is built, so
importing the case proves the input is what its name says.  No GPU is needed here (tests/test_crafted_cpu.py).

families() yields (name, ksize, scaled, moltype, T, Q) with T = (offs u64, mins u64, ab u32) and Q likewise."""
import numpy as np

U32_MAX = (1 << 32) - 1
U64_MAX = (1 << 64) - 1
ABUND_EDGES = (0, 1, 2, (1 << 16) - 1, 1 << 16, 1 << 31, U32_MAX - 1, U32_MAX)
PBITS_EDGES = (1, 8, 9, 15, 16, 17)
PREFIX_SCALED = (1, 3, 5, 1000, U32_MAX)
JN_CAP = 6144          # index postings one workgroup stages per chunk (ks_search.hip)
JN_STAGE_ROUND = 5120  # fingerprints per staging round (JN_THREADS * JN_FILLU)
PAIR_BOUND = 1 << 26   # every case stays far below KS_PAIR_LIMIT: no case leans on pair-count slicing
WIDE_N_T = 4096
WIDE_N_Q = 1 << 20     # 12 + 20 + 32 = 64 record bits; one sequence more needs 65


# ---- the library's host arithmetic, restated ---------------------------------------------------------------------------

def max_hash(scaled):
    """sourmash max_hash_for_scaled as ks_max_hash computes it (the division is done in f64)."""
    if scaled == 1:
        return U64_MAX
    v = 18446744073709551616.0 / float(scaled)
    return U64_MAX if v >= 18446744073709551616.0 else int(v)


def bits_for(n):
    """bits needed for ids 0..n-1 (>= 1)"""
    b = 0
    while b < 32 and n > (1 << b):
        b += 1
    return max(b, 1)


def bits_for_value(v):
    """bits needed for the value v itself (>= 1)"""
    b = 1
    while b < 32 and (v >> b):
        b += 1
    return b


def prefix_mul(pbits, mh):
    """K = min(2^32 - 1, 2^(pbits + 32) / ((max_hash >> 32) + 1))"""
    return min(U32_MAX, (1 << (pbits + 32)) // ((mh >> 32) + 1))


def join_prefix(h, K):
    """umulhi(h >> 32, K)"""
    return ((int(h) >> 32) * K) >> 32


def prefix_boundaries(pbits, mh):
    """[(b, last hash with a prefix < b, first hash with prefix >= b)] for every bucket b >= 1 the formula can reach"""
    K = prefix_mul(pbits, mh)
    top = join_prefix(mh, K)
    hi = [((b << 32) + K - 1) // K for b in range(1, top + 1)]  # smallest top word whose product reaches b << 32
    return K, top, [(b + 1, (w << 32) - 1, w << 32) for b, w in enumerate(hi)]


def check_valid(S, scaled):
    """ks_sketches_from_host's checks, restated."""
    offs, mins, ab = S
    assert offs.dtype == np.uint64 and mins.dtype == np.uint64 and ab.dtype == np.uint32
    assert offs[0] == 0 and len(mins) == len(ab) == int(offs[-1])
    assert np.all(offs[1:] >= offs[:-1])
    mh = max_hash(scaled)
    if len(mins):
        assert mins.min() > 0 and int(mins.max()) <= mh
        asc = mins[1:] > mins[:-1]
        starts = offs[1:-1][(offs[1:-1] > 0) & (offs[1:-1] < len(mins))].astype(np.int64)
        asc[starts - 1] = True  # (the first hash of a sequence is compared with nothing)
        assert asc.all(), "not strictly ascending inside a sequence"


# ---- builders ----------------------------------------------------------------------------------------------------------

def _csr(seq, h, a, n_seqs):
    """(sequence id, hash, abundance) triples -> CSR; a (sequence, hash) pair that repeats is kept once (the first)."""
    seq = np.asarray(seq, np.int64); h = np.asarray(h, np.uint64); a = np.asarray(a, np.uint32)
    o = np.lexsort((h, seq))
    seq, h, a = seq[o], h[o], a[o]
    if len(h):
        keep = np.ones(len(h), bool)
        keep[1:] = (seq[1:] != seq[:-1]) | (h[1:] != h[:-1])
        seq, h, a = seq[keep], h[keep], a[keep]
    offs = np.zeros(n_seqs + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(seq, minlength=n_seqs))
    return offs, np.ascontiguousarray(h), np.ascontiguousarray(a)


def _deal(rng, hashes, n_seqs, copies, abunds=(1, 2, 3, 7)):
    """every hash into `copies` different sequences (a random first one, then 7 further on each time)"""
    hashes = np.asarray(hashes, np.uint64)
    assert n_seqs > 7 * copies or copies == 1
    first = rng.integers(0, n_seqs, len(hashes))
    seq = np.concatenate([(first + 7 * j) % n_seqs for j in range(copies)])
    h = np.tile(hashes, copies)
    return _csr(seq, h, rng.choice(np.asarray(abunds, np.uint32), len(h)), n_seqs)


def _u64(vals):
    return np.array(sorted(set(int(v) for v in vals)), dtype=np.uint64)


def _uniform(rng, n, lo, hi):
    """n values in [lo, hi]"""
    return rng.integers(lo, hi, n, dtype=np.uint64, endpoint=True)


def _seq(S, i):
    return S[1][int(S[0][i]):int(S[0][i + 1])]


# ---- the families ------------------------------------------------------------------------------------------------------

def prefix_edges(scaled):
    rng = np.random.default_rng([101, scaled])
    mh = max_hash(scaled)
    special = {1, mh, mh - 1}
    edges = set()
    for pbits in PBITS_EDGES:
        K, top, bounds = prefix_boundaries(pbits, mh)
        assert join_prefix(1, K) == 0 and join_prefix(mh, K) == top < (1 << pbits)
        for b, below, above in bounds:
            assert above - below == 1 and join_prefix(below, K) < b <= join_prefix(above, K)
            edges.update(x for x in (below - 1, below, above, above + 1) if 0 < x <= mh)
        if scaled == U32_MAX:
            assert top == 0  # (max_hash = 2^32 + 1: every prefix is 0, one bucket holds everything)
    filler = _u64(_uniform(rng, 3000, 1, mh).tolist())
    if scaled == U32_MAX:
        edges.update(((1 << 32) - 1, 1 << 32))
    edge = _u64(edges - special)
    t_h = _u64(list(special) + edge.tolist() + filler[:2000].tolist())
    pick = edge[rng.random(len(edge)) < 0.6]
    q_h = _u64(list(special) + pick.tolist() + filler[1000:].tolist())  # (filler[2000:]: absent from the targets)
    T = _deal(rng, t_h, 64, 3, ABUND_EDGES[1:5])
    Q = _deal(rng, q_h, 24, 2)
    for pbits in PBITS_EDGES:  # the property: prefix 0 and the largest prefix are both present, on both sides
        K = prefix_mul(pbits, mh)
        for S in (T, Q):
            p = {join_prefix(int(S[1].min()), K), join_prefix(int(S[1].max()), K)}
            assert p == {0, join_prefix(mh, K)}
    assert {1, mh, mh - 1} <= set(T[1].tolist()) & set(Q[1].tolist())
    return f"prefix_edges_s{scaled}", 10, scaled, "protein", T, Q


def one_bucket():
    rng = np.random.default_rng(102)
    top17 = 0x15A5B
    low = _u64([0, 1, (1 << 47) - 1, (1 << 47) - 2] + rng.integers(0, 1 << 47, 42000, dtype=np.uint64).tolist())
    hashes = (np.uint64(top17) << np.uint64(47)) | low
    t_h, absent = hashes[::2], hashes[1::2]
    t_h = _u64(t_h.tolist() + [int(hashes[0]), int(hashes[-1])])
    T = _deal(rng, t_h, 100, 3)
    q_h = _u64(rng.choice(t_h, 4000, replace=False).tolist() + rng.choice(absent, 4000, replace=False).tolist() +
               [int(hashes[0]), int(hashes[-1])])
    Q = _deal(rng, q_h, 60, 2)
    n_post = len(T[1])
    assert n_post >= 50000 and n_post > JN_CAP and n_post > JN_STAGE_ROUND
    assert np.all(T[1] >> np.uint64(47) == top17) and np.all(Q[1] >> np.uint64(47) == top17)
    return "one_bucket", 10, 1, "protein", T, Q


def flat_bucket_single():
    """300 targets that hold the same single hash: one bucket whose first and last key are equal (largest fingerprint 0)"""
    h0 = 0x9E3779B97F4A7C15
    n_t = 300
    T = _csr(np.arange(n_t), np.full(n_t, h0, np.uint64), np.arange(n_t) % 5, n_t)
    q = [[h0], [h0 - 1, h0, h0 + 1], [h0 - 1, h0 + 1], [1, h0], [h0, U64_MAX], [1, U64_MAX], []]
    Q = _csr(np.concatenate([np.full(len(x), i) for i, x in enumerate(q)]), np.concatenate([np.array(x, np.uint64) for x in q]),
             np.ones(sum(len(x) for x in q)), len(q))
    assert T[1].min() == T[1].max() and len(T[1]) == n_t
    return "flat_bucket_single", 10, 1, "protein", T, Q


FLAT_FP_SHIFT = 32  # the fingerprint shift of a small index (no prefix bits): 32 - pbits


def flat_bucket_runs():
    """keys that differ only below the fingerprint shift: runs of distinct keys under one fingerprint"""
    rng = np.random.default_rng(104)
    base = 1 << 32  # the smallest target key: the fingerprints of the (one) bucket count from it
    groups = sorted(set(int(g) for g in rng.integers(2, 1 << 31, 40)))
    low_t, low_q = (0, 2, 4, 1 << 31, U32_MAX), (2, 3, 4, 1 << 31, U32_MAX - 1)  # (3 and 2^32 - 2: absent)
    t_h = _u64([base] + [(g << 32) + x for g in groups for x in low_t])
    q_h = _u64([base, base + 1] + [(g << 32) + x for g in groups for x in low_q])
    T = _deal(rng, t_h, 30, 3)
    Q = _deal(rng, q_h, 24, 2)
    assert len(T[1]) <= 3072  # (one join bucket: the index joins on no prefix bits)
    assert int(T[1].min()) == base
    t_set, q_set = set(T[1].tolist()), set(Q[1].tolist())
    ok = 0
    for g in groups:
        run = sorted(k for k in t_set if (k - base) >> FLAT_FP_SHIFT == ((g << 32) - base) >> FLAT_FP_SHIFT)
        absent = [k for k in q_set if k not in t_set and run[0] < k < run[-1]]
        ok += len(run) >= 3 and run[len(run) // 2] in q_set and len(absent) > 0
    assert ok == len(groups)
    return "flat_bucket_runs", 10, 1, "protein", T, Q


def consecutive(scaled):
    mh = max_hash(scaled)
    n = 3000
    vals = np.concatenate([np.arange(1, n + 1, dtype=np.uint64), np.uint64(mh - n) + np.arange(n + 1, dtype=np.uint64)])
    assert len(vals) == 2 * n + 1 and int(vals[-1]) == mh and int(vals[0]) == 1
    T = _csr(np.arange(len(vals)) % 40, vals, 1 + np.arange(len(vals)) % 9, 40)
    qv = vals[::3]
    Q = _csr(np.arange(len(qv)) % 30, qv, np.ones(len(qv)), 30)
    assert np.all(np.diff(vals[:n]) == 1) and np.all(np.diff(vals[n:]) == 1)
    return f"consecutive_s{scaled}", 10, scaled, "protein", T, Q


def wide_records():
    """4,096 targets with abundances up to 2^32 - 1 and a query batch of 2^20 + 1 sequences, almost all of them empty: the
    first 2^20 give match records of exactly 64 bits (the all-ones record among them), one more forces slices of 2^20."""
    rng = np.random.default_rng(105)
    n_t, n_q = WIDE_N_T, WIDE_N_Q + 1
    pool = np.unique(rng.integers(1 << 20, 1 << 63, 40000, dtype=np.uint64) * np.uint64(2))  # even: private hashes are odd
    hx = int(pool[-1]) + 2  # the hash of the all-ones record
    seq, h, a = [], [], []
    mode = rng.integers(0, 8, n_t)  # 0: shared abundances all 0; 1: all 2^32 - 1; else drawn from the edge set
    mode[[0, 1, 2, 3]] = (0, 1, 0, 1)
    edges = np.asarray(ABUND_EDGES, np.uint32)
    for t in range(n_t):
        m = int(rng.integers(20, 60))
        hs = np.unique(pool[rng.integers(0, len(pool), m)])
        m = len(hs)
        ab = np.zeros(m, np.uint32) if mode[t] == 0 else (np.full(m, U32_MAX, np.uint32) if mode[t] == 1 else rng.choice(edges, m))
        seq += [t] * (m + 1); h += hs.tolist() + [2 * t + 1]; a += ab.tolist() + [1]  # (+ a private hash: no target sums to 0)
    seq.append(n_t - 1); h.append(hx); a.append(U32_MAX)
    T = _csr(seq, h, a, n_t)
    ids = np.unique(np.concatenate([np.arange(0, 100), np.arange(n_q // 2 - 50, n_q // 2 + 50), np.arange(WIDE_N_Q - 100, n_q)]))
    seq, h = [], []
    for j, q in enumerate(ids.tolist()):
        t = j % 8 if j < 64 else int(rng.integers(0, n_t))  # (the first ones copy the all-0 and all-max targets)
        src = _seq(T, t)
        src = src[src % np.uint64(2) == 0]
        own = rng.choice(src, int(rng.integers(1, min(30, len(src)))), replace=False)
        other = pool[rng.integers(0, len(pool), int(rng.integers(40, 100)))]
        absent = rng.integers(1, 1 << 20, 3, dtype=np.uint64) * np.uint64(2)
        hs = _u64(own.tolist() + other.tolist() + absent.tolist() + ([hx] if q >= WIDE_N_Q - 1 else []))
        seq += [q] * len(hs); h += hs.tolist()
    Q = _csr(seq, h, np.ones(len(h)), n_q)
    # the properties, with the library's bit counts replayed
    tbits, abits = bits_for(n_t), bits_for_value(int(T[2].max()))
    assert (tbits, bits_for(WIDE_N_Q), abits) == (12, 20, 32) and tbits + bits_for(WIDE_N_Q) + abits == 64
    assert tbits + bits_for(n_q) + abits == 65 and 1 << (64 - tbits - abits) == WIDE_N_Q  # slices of 2^20 sequences
    assert all(np.uint64(hx) in x for x in (_seq(T, n_t - 1), _seq(Q, WIDE_N_Q - 1), _seq(Q, WIDE_N_Q)))
    assert int(T[2][int(T[0][n_t]) - 1]) == U32_MAX and int(T[1][-1]) == hx  # the record (2^20 - 1, 4095, 2^32 - 1) is all ones
    assert (((WIDE_N_Q - 1) << tbits | (n_t - 1)) << abits) | U32_MAX == U64_MAX
    assert np.count_nonzero(np.diff(Q[0])) == len(ids) >= 300 and len(_seq(Q, 0)) and len(_seq(Q, n_q // 2))
    rows = ref_join(T, Q)
    assert np.any(rows[3] >= np.uint64(1 << 32)) and np.any(rows[2] % 2 == 1) and np.any(rows[2] % 2 == 0)
    assert np.any((rows[3] == 0) & (rows[2] >= 2))  # a row whose shared abundances are all 0
    # a median2 >= 2^32.  Deliberately looked for among the first 400 rows only (the replica is slow): they belong to the first
    # queries, which copy targets 0 .. 7, and targets 1 and 3 hold 2^32 - 1 everywhere (mode[[0, 1, 2, 3]] above)
    assert np.any(ref_stats(rows, T, Q, range(0, min(400, len(rows[0]))))[0] >= np.uint64(1 << 32))
    assert np.any(rows[0] == WIDE_N_Q - 1) and np.any(rows[0] == WIDE_N_Q)  # the last sequence of either batch has hits
    assert int(rows[2][rows[0] < WIDE_N_Q].sum()) >= 65536  # (enough matches for the MSD match sort to be the default)
    return "wide_records", 10, 1, "protein", T, Q


def wide_batches(Q):
    """the two query batches of wide_records, sharing one offsets array: 2^20 sequences, and one more"""
    offs, mins, ab = Q
    n = int(offs[WIDE_N_Q])
    return (offs[:WIDE_N_Q + 1], mins[:n], ab[:n]), Q


def zero_abund():
    rng = np.random.default_rng(106)
    t_h = _u64(_uniform(rng, 4000, 1, U64_MAX - 1).tolist())
    T = _deal(rng, t_h, 200, 3, abunds=(0,))
    q_h = _u64(rng.choice(t_h, 1500, replace=False).tolist() + _uniform(rng, 500, 1, U64_MAX - 1).tolist())
    Q = _deal(rng, q_h, 90, 2)
    assert len(T[2]) and int(T[2].max()) == 0 and bits_for_value(0) == 1
    return "zero_abund", 10, 1, "protein", T, Q


UNION_LONG_RUN = 70000
UNION_SUMS = {"below": U32_MAX - 1, "at": U32_MAX, "above": 1 << 32, "zero": 0}


def union_saturation():
    rng = np.random.default_rng(107)
    n_long = UNION_LONG_RUN
    A, F = 0x7000000000000001, 0x7000000000000002  # carried by 70,000 sequences: sums far above 2^32, and 70,000
    named = {"below": 0x1000, "at": 0x2000, "above": 0x3000, "zero": 0x4000, "alone": 0x5000}
    extra = rng.integers(1 << 40, 1 << 62, n_long, dtype=np.uint64)
    seq = np.concatenate([np.arange(n_long)] * 3).tolist()
    h = [A] * n_long + [F] * n_long + extra.tolist()
    a = [U32_MAX] * n_long + [1] * n_long + rng.choice(np.asarray(ABUND_EDGES, np.uint32), n_long).tolist()
    parts = {"below": ((1 << 31) - 1, (1 << 31) - 1), "at": (1 << 31, (1 << 31) - 1), "above": (1 << 31, 1 << 31), "zero": (0, 0, 0),
             "alone": (U32_MAX,)}
    s = n_long
    for name, abs_ in parts.items():
        for x in abs_:
            seq.append(s); h.append(named[name]); a.append(x); s += 1
    n_t = s + 1  # (+ an empty sequence at the end)
    T = _csr(seq, h, a, n_t)
    q = [[A, F], [named["below"], named["at"], named["above"], named["zero"], named["alone"]], [F, named["zero"], 0x4001],
         extra[:50].tolist(), [1, U64_MAX]]
    Q = _csr(np.concatenate([np.full(len(x), i) for i, x in enumerate(q)]), np.concatenate([np.array(x, np.uint64) for x in q]),
             np.ones(sum(len(x) for x in q)), len(q))
    sums = {}
    for hh, aa in zip(T[1].tolist(), T[2].tolist()):
        sums[hh] = sums.get(hh, 0) + aa
    assert all(sums[named[k]] == v for k, v in UNION_SUMS.items()) and sums[named["alone"]] == U32_MAX
    assert sums[A] == n_long * U32_MAX > 1 << 40 and sums[F] == n_long
    assert int(np.count_nonzero(T[1] == np.uint64(A))) >= UNION_LONG_RUN
    return "union_saturation", 10, 1, "protein", T, Q


ROW_SHARED = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)  # both sides of RA_LONG (ks_rows.hip) and of the 64-element chunk edges
RA_LONG = 64   # a row with more shared hashes is listed for the wave kernel of the statistics
SG_CUT = 128   # |q| + |t| above it: the wave kernel of the significance pass (ks_signif.hip)


def row_lengths():
    """Rows whose lengths sit on the thresholds of the two lane / wave splits: query 0 holds 193 hashes and target i shares
    exactly ROW_SHARED[i] of them (a random subset) beside five of its own; query 1 holds 64 hashes, and the last two targets,
    of 64 and 65 hashes, make |q| + |t| 128 and 129 with it.  Abundances come from the edge set on both sides."""
    rng = np.random.default_rng(108)
    edges = np.asarray(ABUND_EDGES, np.uint32)
    pool = np.unique(rng.integers(1 << 20, 1 << 63, 700, dtype=np.uint64) * np.uint64(2))  # even; the targets' own hashes are odd
    q0, q1 = pool[:193], pool[193:257]
    assert len(pool) >= 257 and len(q0) == 193 and len(q1) == 64
    want, seq, h = {}, [], []
    for t, n in enumerate(ROW_SHARED):
        hs = rng.choice(q0, n, replace=False).tolist() + [2 * (10 * t + j) + 1 for j in range(5)]
        seq += [t] * len(hs); h += hs
        want[(0, t)] = n
    for t, (n, size) in enumerate(((40, 64), (41, 65)), len(ROW_SHARED)):
        hs = rng.choice(q1, n, replace=False).tolist() + [2 * (10 * t + j) + 1 for j in range(size - n)]
        seq += [t] * len(hs); h += hs
        want[(1, t)] = n
    n_t = len(ROW_SHARED) + 2
    T = _csr(seq, h, rng.choice(edges, len(h)), n_t)
    qh = np.concatenate([q0, q1])
    Q = _csr([0] * 193 + [1] * 64, qh, rng.choice(edges[1:], len(qh)), 2)
    rows = ref_join(T, Q)
    got = {(int(q), int(t)): int(n) for q, t, n in zip(rows[0], rows[1], rows[2])}
    assert got == want, got  # the intersect of every row is the intended number, and there is no other row
    assert set(ROW_SHARED) >= {RA_LONG - 1, RA_LONG, RA_LONG + 1, 127, 128, 129, 192, 193}
    sizes_q, sizes_t = np.diff(Q[0]).astype(np.int64), np.diff(T[0]).astype(np.int64)
    assert sorted(int(sizes_q[q] + sizes_t[t]) for q, t in want if q == 1) == [SG_CUT, SG_CUT + 1]
    assert int(sizes_q[0]) == 193 and all(int(sizes_q[0] + sizes_t[t]) > SG_CUT for q, t in want if q == 0)
    for (q, t), n in want.items():  # every long row mixes abundances: the order of its f64 additions shows
        if n >= RA_LONG - 1:
            ab = _seq((T[0], T[2], None), t)
            assert len(set(ab.tolist())) >= 4
    return "row_lengths", 10, 1, "protein", T, Q


_BUILDERS = ([lambda s=s: prefix_edges(s) for s in PREFIX_SCALED] +
             [one_bucket, flat_bucket_single, flat_bucket_runs, lambda: consecutive(1), lambda: consecutive(5), wide_records, zero_abund,
              union_saturation, row_lengths])
NAMES = [f"prefix_edges_s{s}" for s in PREFIX_SCALED] + ["one_bucket", "flat_bucket_single", "flat_bucket_runs", "consecutive_s1",
                                                         "consecutive_s5", "wide_records", "zero_abund", "union_saturation",
                                                         "row_lengths"]
_CACHE = {}


def family(name, fresh=False):
    """the case of that name (built once per process unless fresh)"""
    if fresh or name not in _CACHE:
        case = _BUILDERS[NAMES.index(name)]()
        assert case[0] == name
        check_valid(case[4], case[2]); check_valid(case[5], case[2])
        assert ref_pairs(case[4], case[5]) < PAIR_BOUND, name
        if fresh:
            return case
        _CACHE[name] = case
    return _CACHE[name]


def families():
    for name in NAMES:
        yield family(name)


# ---- references --------------------------------------------------------------------------------------------------------

def _matches(T, Q):
    """(query sequence, target posting) of every matched posting pair"""
    to, tm, _ = T
    qo, qm, _ = Q
    order = np.argsort(tm, kind="stable")
    th = tm[order]
    lo = np.searchsorted(th, qm, side="left").astype(np.int64)
    cnt = np.searchsorted(th, qm, side="right").astype(np.int64) - lo
    q_of = np.repeat(np.arange(len(qo) - 1, dtype=np.int64), np.diff(qo).astype(np.int64))
    n = int(cnt.sum())
    within = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.repeat(q_of, cnt), order[np.repeat(lo, cnt) + within]


def ref_pairs(T, Q):
    """sum over hashes of q(h) * t(h): the matched posting pairs"""
    return len(_matches(T, Q)[0])


def ref_join(T, Q):
    """(qid u32, tid u32, intersect u32, n_weighted u64) in (qid, tid) order — sort and searchsorted, u64 sums"""
    to, tm, ta = T
    qi, tp = _matches(T, Q)
    t_of = np.repeat(np.arange(len(to) - 1, dtype=np.int64), np.diff(to).astype(np.int64))
    key = (qi.astype(np.uint64) << np.uint64(32)) | t_of[tp].astype(np.uint64)
    o = np.argsort(key, kind="stable")
    key, w = key[o], ta[tp][o].astype(np.uint64)
    if len(key) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    starts = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    rows = key[starts]
    isect = np.diff(np.concatenate([starts, [len(key)]])).astype(np.uint32)
    return (rows >> np.uint64(32)).astype(np.uint32), (rows & np.uint64(U32_MAX)).astype(np.uint32), isect, np.add.reduceat(w, starts)


def ref_union(T):
    """(offsets [0, n], unique hashes, u64 abundance sums clipped to 2^32 - 1)"""
    _, tm, ta = T
    hashes, inv = np.unique(tm, return_inverse=True)
    sums = np.zeros(len(hashes), np.uint64)
    np.add.at(sums, inv, ta.astype(np.uint64))
    return np.array([0, len(hashes)], np.uint64), hashes, np.minimum(sums, np.uint64(U32_MAX)).astype(np.uint32)


def replica(q_mins, t_mins, t_ab):
    """The host's row loop: the shared target abundances, sorted, then sequential f64 sums -> (n, mean, median, ss).
    (Python floats are IEEE doubles; no contraction.)"""
    _, _, ti = np.intersect1d(q_mins, t_mins, assume_unique=True, return_indices=True)
    shared = sorted(float(x) for x in t_ab[ti])
    n = len(shared)
    s = 0.0
    for x in shared:
        s += x
    mean = s / float(n)
    ss = 0.0
    for x in shared:
        ss += (x - mean) * (x - mean)
    median = shared[n // 2] if n % 2 else (shared[n // 2 - 1] + shared[n // 2]) / 2.0
    return n, mean, median, ss


def keep(rows, qs, thr):
    """the containment keep-mask: (double)intersect / (double)|q| >= thr"""
    qo = qs[0]
    qsize = (qo[1:] - qo[:-1]).astype(np.float64)
    c = rows[2].astype(np.float64) / qsize[rows[0].astype(np.int64)]
    return c >= thr


def ref_stats(rows, T, Q, which=None):
    """(median2 u64, ss f64) of the rows `which` (all of them by default) through replica()"""
    to, tm, ta = T
    qo, qm, _ = Q
    which = range(len(rows[0])) if which is None else which
    m2, ss = [], []
    for r in which:
        q, t = int(rows[0][r]), int(rows[1][r])
        n, mean, median, s = replica(qm[int(qo[q]):int(qo[q + 1])], tm[int(to[t]):int(to[t + 1])], ta[int(to[t]):int(to[t + 1])])
        assert n == int(rows[2][r]) and int(rows[3][r]) < 1 << 53 and float(int(rows[3][r])) / n == mean
        m2.append(int(median * 2.0)); ss.append(s)
        assert float(m2[-1]) == median * 2.0
    return np.array(m2, np.uint64), np.array(ss, np.float64)


def wide_stat_rows(rows):
    """the rows of the largest family whose statistics are held against replica(): a fixed stride, the first and the last
    row, and every row with n_weighted >= 2^31.  That holds every row with n_weighted >= 2^32 and every row with
    median2 >= 2^32: a median2 that large is one middle value doubled or the sum of two, so one shared abundance is >= 2^31
    (a row of one record with abundance 2^31 has median2 = 2^32 and n_weighted = 2^31)."""
    n = len(rows[0])
    pick = set(range(0, n, 7)) | {0, n - 1} | set(np.nonzero(rows[3] >= np.uint64(1 << 31))[0].tolist())
    return sorted(pick)
