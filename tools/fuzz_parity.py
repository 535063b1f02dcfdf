"""Randomised differential test of the HIP path against the oracle (sketch, k-mer positions, search).

    python tools/fuzz_parity.py [--cases N] [--seed S] [--entries] [--matchpos] [--crafted] [--knob NAME=VALUE ...]

Every case draws k, scaled, moltype, a length distribution (peptides / proteome-like / long / degenerate), an alphabet
(full, 2-letter, single residue, with ambiguity codes and lower case) and a batch size, sketches it through the C ABI and
compares with the oracle bit for bit; every third case also builds an index and searches it.  Prints one line per failure.
With --entries every case also goes through ks_sketch_batch_device, and the one-call search takes, with a hint of 0, the exact
longest sequence or more.  --matchpos runs match-position cases instead (run_matchpos), --crafted hand-made
sketches on the edges of the search arithmetic (run_crafted: no residues, no oracle — numpy references).  --knob sets a KS_DEBUG_* knob around every case (the context follows the environment).
"""
import argparse
import contextlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import kmerseek_amd as ks
from oracle import oracle

ALPHABETS = [b"ACDEFGHIKLMNPQRSTVWY", b"AC", b"A", b"ACDEFGHIKLMNPQRSTVWYXUO*BZJ", b"acdefghiklmnpqrstvwyACDEFG", b"LLLLLLLLLS"]


def draw_batch(rng):
    kind = rng.integers(0, 6)
    n = int(rng.integers(1, 400))
    if kind == 0:
        lens = rng.integers(0, 40, n)
    elif kind == 1:
        lens = np.clip(np.rint(rng.lognormal(np.log(260.0), 0.55, n)), 0, 3000)
    elif kind == 2:
        lens = rng.integers(700, 4200, max(1, n // 8))
    elif kind == 3:
        lens = rng.choice([0, 1, 5, 4079, 4080, 4081, 8200, 300], size=max(1, n // 10))
    elif kind == 4:
        lens = rng.integers(0, 12, n * 4)
    else:
        lens = np.concatenate([rng.integers(0, 300, n), [int(rng.integers(5000, 30000))]])
        rng.shuffle(lens)
    lens = lens.astype(np.uint64)
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    alpha = np.frombuffer(ALPHABETS[int(rng.integers(0, len(ALPHABETS)))], np.uint8)
    res = rng.choice(alpha, size=int(offs[-1])).astype(np.uint8)
    if rng.random() < 0.3 and len(res) > 50:  # planted repeats: abundances > 1, heavy buckets
        unit = res[:int(rng.integers(3, 40))]
        reps = np.tile(unit, len(res) // len(unit) + 1)[:len(res)]
        mask = rng.random(len(res)) < 0.5
        res = np.where(mask, reps, res).astype(np.uint8)
    return res, offs


@contextlib.contextmanager
def knobs_set(knobs):
    """KS_DEBUG_<name> = value for each knob inside the block (a follow_debug_env context reads them on every call)."""
    old = {n: os.environ.get("KS_DEBUG_" + n) for n in knobs}
    os.environ.update({"KS_DEBUG_" + n: str(v) for n, v in knobs.items()})
    try:
        yield
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop("KS_DEBUG_" + n, None)
            else:
                os.environ["KS_DEBUG_" + n] = v


STAT_KEYS = ("ticket_fallbacks", "compact_fallbacks", "cap_fallbacks", "join_retries", "rows_ticket_fallbacks", "deferred", "redos")


def _add_stats(ctx, stats):
    if stats is None:
        return
    cur = {**ctx.sketch_stats(), **ctx.search_stats(), **ctx.fused_stats()}
    for key in STAT_KEYS:
        stats[key] = stats.get(key, 0) + cur[key]


def _hint(erng, offs):
    """0 (the batch is measured), the exact longest sequence, or more than that"""
    mx = int((offs[1:] - offs[:-1]).max()) if len(offs) > 1 else 0
    c = int(erng.integers(0, 3))
    return 0 if c == 0 else (mx if c == 1 else mx + int(erng.integers(1, 5000)))


def run(cases: int, seed: int, knobs=None, entries: bool = False, ctx_per_case: bool = False, stats=None) -> int:
    """Runs `cases` random cases; prints one line per failure; returns the number of failures.
    knobs: {name: value} of KS_DEBUG_* knobs set around every case.  entries: every case also goes through
    ks_sketch_batch_device, and the one-call search takes a random hint (0, exact, more).  ctx_per_case: a fresh context per
    case (forced repeats: a context that repeated once keeps the repeat's scheme).  stats: summed counters of the contexts
    (STAT_KEYS).  The batches do not depend on knobs or entries: one seed, the same cases."""
    rng = np.random.default_rng(seed)
    erng = np.random.default_rng([seed, 1])  # (the entry choices: a stream of their own)
    knobs = knobs or {}
    ctx = None
    bad = 0
    for case in range(cases):
        k = int(rng.choice([1, 2, 3, 5, 7, 8, 9, 10, 15, 16, 17, 21, 24, 31, 32, 33, 48, 64, 100, 128]))
        scaled = int(rng.choice([1, 1, 1, 2, 5, 10, 50, 1000]))
        mol = str(rng.choice(["protein", "dayhoff", "hp"]))
        res, offs = draw_batch(rng)
        tag = f"case {case}: k={k} scaled={scaled} {mol} n_seqs={len(offs) - 1} n_res={len(res)}"
        if ctx is None or ctx_per_case:
            if ctx is not None:
                _add_stats(ctx, stats)
                ctx.close()
            ctx = ks.Context(0, follow_debug_env=True)
        with knobs_set(knobs):
            bad += _case(ctx, rng, erng, case, k, scaled, mol, res, offs, tag, entries)
    _add_stats(ctx, stats)
    ctx.close()
    return bad


def run_staged_copy(seed: int, knobs=None) -> int:
    """One host batch above the staged-copy threshold (4 MiB of residues): sketch vs oracle.  Returns the number of failures."""
    from kmerseek_amd import synth
    res, offs = synth.proteome(16000, stream=seed)
    assert len(res) >= 4 << 20
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        with knobs_set(knobs or {}):
            got = ctx.sketch_batch(res, offs, 10, 1, "protein").to_host()
        if not all(np.array_equal(g, w) for g, w in zip(got, oracle.sketch_batch(res, offs, 10, 1, "protein", n_threads=8))):
            print("SKETCH MISMATCH staged copy"); return 1
    finally:
        ctx.close()
    return 0


def _case(ctx, rng, erng, case, k, scaled, mol, res, offs, tag, entries) -> int:
    """One case of run(): 0 if it matches the oracle, 1 otherwise (with one line printed)."""
    try:
        S = ctx.sketch_batch(res, offs, k, scaled, mol)
        got = S.to_host()
        want = oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=8)
        if not all(np.array_equal(g, w) for g, w in zip(got, want)):
            print("SKETCH MISMATCH", tag); return 1
        if entries:
            hint = _hint(erng, offs)
            d_res, d_off = ctx.to_device(res), ctx.to_device(offs)
            got = ctx.sketch_batch_device(d_res.ptr, d_off.ptr, len(offs) - 1, len(res), k, scaled, mol, max_seq_len=hint).to_host()
            if not all(np.array_equal(g, w) for g, w in zip(got, want)):
                print("DEVICE SKETCH MISMATCH", tag, f"max_seq_len={hint}"); return 1
        # (process_kmers hashes the validated, already upper-case sequence as given — src/rust/index.rs:749-786 — so the
        # oracle's position pass does not fold case; lower-case input never reaches it in the reference)
        if case % 4 == 1 and len(res) < 200000 and not np.any((res >= 97) & (res <= 122)):
            ps, pst, ph = ctx.kmer_positions(res, offs, k, scaled, mol)
            o, mins, _ = want
            ws, wst, wh = [], [], []
            for i in range(len(offs) - 1):
                st, hh = oracle.kmer_positions(bytes(res[int(offs[i]):int(offs[i + 1])]), k, mol, mins[int(o[i]):int(o[i + 1])])
                ws.append(np.full(len(st), i, np.uint32)); wst.append(st); wh.append(hh)
            if not (np.array_equal(ps, np.concatenate(ws)) and np.array_equal(pst, np.concatenate(wst)) and np.array_equal(ph, np.concatenate(wh))):
                ws_, wst_, wh_ = np.concatenate(ws), np.concatenate(wst), np.concatenate(wh)
                m = min(len(ps), len(ws_))
                d = np.nonzero((ps[:m] != ws_[:m]) | (pst[:m] != wst_[:m]) | (ph[:m] != wh_[:m]))[0]
                j = int(d[0]) if len(d) else m
                ctxt = ""
                if j < len(ws_):
                    sq, st0 = int(ws_[j]), int(wst_[j])
                    ctxt = f" want(seq={sq},start={st0},h={int(wh_[j])}) window={bytes(res[int(offs[sq]) + st0:int(offs[sq]) + st0 + k])!r} seqlen={int(offs[sq + 1] - offs[sq])} seqoff={int(offs[sq])}"
                if j < len(ps):
                    ctxt += f" got(seq={int(ps[j])},start={int(pst[j])},h={int(ph[j])})"
                print("POSITIONS MISMATCH", tag, f"n_got={len(ps)} n_want={len(ws_)} first_diff={j}" + ctxt); return 1
        if case % 3 == 0:
            res2, offs2 = draw_batch(rng)
            if rng.random() < 0.5 and len(offs) > 2:  # make the queries overlap the targets
                cut = int(offs[len(offs) // 2])
                res2 = np.concatenate([res[:cut], res2]).astype(np.uint8)
                offs2 = np.concatenate([offs[:len(offs) // 2], offs2 + np.uint64(cut)]).astype(np.uint64)
            Q = ctx.sketch_batch(res2, offs2, k, scaled, mol)
            ix = ctx.index_build(S)
            h = ctx.search(ix, Q).to_host()
            qo, qm, _ = Q.to_host()
            w = oracle.manysearch(qo, qm, want[0], want[1], want[2], n_threads=8)
            if not all(np.array_equal(x, y) for x, y in zip(h, w)):
                print("SEARCH MISMATCH", tag, f"n_q={len(offs2) - 1} hits={len(h[0])}/{len(w[0])}"); return 1
            d_res, d_off = ctx.to_device(res2), ctx.to_device(offs2)
            Q2 = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, len(offs2) - 1, len(res2))
            h2 = ctx.search(ix, Q2).to_host()
            if not all(np.array_equal(x, y) for x, y in zip(h2, w)):
                print("FUSED SEARCH MISMATCH", tag); return 1
            # one call (ks_sketch_search_device), with the bound that lets it defer the sketch's read-back (--entries: a
            # random one of 0, exact, more)
            mx = int((offs2[1:] - offs2[:-1]).max()) if len(offs2) > 1 else 0
            if entries:
                mx = _hint(erng, offs2)
            Q3, H3 = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, len(offs2) - 1, len(res2), max_seq_len=mx)
            if not (all(np.array_equal(x, y) for x, y in zip(H3.to_host(), w)) and
                    all(np.array_equal(x, y) for x, y in zip(Q3.to_host(), Q.to_host()))):
                print("ONE-CALL SEARCH MISMATCH", tag); return 1
    except Exception as e:  # noqa: BLE001
        print("ERROR", tag, repr(e)); return 1
    return 0


def _join_tables(q_tab, t_tab, hit_qid, hit_tid, ksize):
    """numpy restatement of ks_match_positions on host copies of the two k-mer tables: (row_offsets, q_start, t_start, q_lo,
    q_hi, t_lo, t_hi) for the hit rows (qid, tid), pairs ordered by (row, query start, target start)."""
    (q_seq, q_start, q_hash), (t_seq, t_start, t_hash) = q_tab, t_tab
    n_rows = len(hit_qid)
    order = np.argsort(t_hash, kind="stable")
    th = t_hash[order]
    lo = np.searchsorted(th, q_hash, side="left").astype(np.int64)
    cnt = np.searchsorted(th, q_hash, side="right").astype(np.int64) - lo
    qi = np.repeat(np.arange(len(q_hash), dtype=np.int64), cnt)
    ti = order[np.repeat(lo, cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    pair_key = (q_seq[qi].astype(np.uint64) << np.uint64(32)) | t_seq[ti].astype(np.uint64)
    hit_key = (hit_qid.astype(np.uint64) << np.uint64(32)) | hit_tid.astype(np.uint64)
    row = np.searchsorted(hit_key, pair_key)
    found = (row < n_rows) & (hit_key[np.minimum(row, max(n_rows - 1, 0))] == pair_key) if n_rows else np.zeros(len(qi), bool)
    row, a, b = row[found], q_start[qi][found], t_start[ti][found]
    o = np.lexsort((b, a, row))
    row, a, b = row[o], a[o].astype(np.uint32), b[o].astype(np.uint32)
    offs = np.zeros(n_rows + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    first, last = offs[:-1].astype(np.int64), offs[1:].astype(np.int64) - 1
    if n_rows == 0 or len(a) == 0 or np.any(last < first):
        return offs, a, b, None
    ext = (a[first], a[last] + np.uint32(ksize), np.minimum.reduceat(b, first), np.maximum.reduceat(b, first) + np.uint32(ksize))
    return offs, a, b, ext


def _regions_ref():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import regions_ref
    return regions_ref


MATCHPOS_MAX_PAIRS = 4_000_000  # low-complexity batches join into far more: those cases check the refusal instead


def run_matchpos(cases: int, seed: int, knobs=None) -> int:
    """Match-position cases: a target batch, a query batch that overlaps it, search (every other case thresholded), the two
    k-mer tables, ks_match_positions with max_pairs = MATCHPOS_MAX_PAIRS — compared with a numpy join of the host copies of the
    same tables and hits (which the other cases hold against the oracle).  A join beyond the limit must be refused with
    KS_ERR_CAPACITY and the count.  The pairs that agree are then chained (ks_match_regions, random max_gap / min_kmers) and
    compared with the numpy chaining of tests/regions_ref.py.  Returns the number of failures."""
    from kmerseek_amd import _lib
    rng = np.random.default_rng(seed)
    knobs = knobs or {}
    bad = n_refused = 0
    ctx = ks.Context(0, follow_debug_env=True)
    for case in range(cases):
        k = int(rng.choice([3, 5, 7, 8, 10, 15, 16, 17, 21, 24, 32, 48]))
        scaled = int(rng.choice([1, 1, 1, 2, 5, 10]))
        mol = str(rng.choice(["protein", "dayhoff", "hp"]))
        t_res, t_off = draw_batch(rng)
        q_res, q_off = draw_batch(rng)
        if len(t_off) > 2:  # the queries overlap the targets
            cut = int(t_off[len(t_off) // 2])
            q_res = np.concatenate([t_res[:cut], q_res]).astype(np.uint8)
            q_off = np.concatenate([t_off[:len(t_off) // 2], q_off + np.uint64(cut)]).astype(np.uint64)
        min_c = 0.0 if case % 2 == 0 else float(rng.choice([0.05, 0.3, 0.8]))
        tag = f"matchpos case {case}: k={k} scaled={scaled} {mol} n_t={len(t_off) - 1} n_q={len(q_off) - 1} min_containment={min_c}"
        try:
            with knobs_set(knobs):
                T = ctx.sketch_batch(t_res, t_off, k, scaled, mol)
                Q = ctx.sketch_batch(q_res, q_off, k, scaled, mol)
                hits = ctx.search(ctx.index_build(T), Q, min_containment=min_c)
                qp = ctx.kmer_positions_table(q_res, q_off, k, scaled, mol)
                tp = ctx.kmer_positions_table(t_res, t_off, k, scaled, mol)
                q_tab, t_tab = qp.to_host(), tp.to_host()
                n_join = int(np.sum(np.searchsorted(np.sort(t_tab[2]), q_tab[2], side="right") -
                                    np.searchsorted(np.sort(t_tab[2]), q_tab[2], side="left")))
                in_use = ctx.pool_stats()["bytes_in_use"]
                try:
                    mp = ctx.match_positions(qp, tp, hits, max_pairs=MATCHPOS_MAX_PAIRS)
                except ks.KmerseekError as e:
                    if hits.count and n_join > MATCHPOS_MAX_PAIRS and e.status == _lib.KS_ERR_CAPACITY and str(n_join) in str(e) \
                            and ctx.pool_stats()["bytes_in_use"] == in_use:
                        n_refused += 1
                        continue
                    raise
                if hits.count and n_join > MATCHPOS_MAX_PAIRS:
                    print("MATCHPOS NOT REFUSED", tag, f"join={n_join}"); bad += 1; continue
                got = mp.to_host()
            qid, tid, isect, _ = hits.to_host()
            offs, a, b, ext = _join_tables(q_tab, t_tab, qid, tid, k)
            ok = np.array_equal(got[0], offs) and np.array_equal(got[1], a) and np.array_equal(got[2], b) and \
                np.all((offs[1:] - offs[:-1]) >= isect)
            if ok and len(qid):
                ok = ext is not None and all(np.array_equal(g, w) for g, w in zip(got[3:], ext))
            if not ok:
                print("MATCHPOS MISMATCH", tag, f"rows={len(qid)} pairs={len(got[1])}/{len(a)} slices={mp.n_slices}"); bad += 1
            else:  # the region pass on the same pairs, against the numpy chaining of tests/regions_ref.py
                max_gap, min_kmers = int(rng.choice([0, 0, 1, k, 2 ** 32 - 1])), int(rng.choice([0, 1, 2, 5]))
                with knobs_set(knobs):
                    rg = ctx.match_regions(mp, max_gap=max_gap, min_kmers=min_kmers)
                    got_rg = rg.to_host()
                    rg.free()
                want_rg = _regions_ref().chain(offs, a, b, k, max_gap, min_kmers)
                if not all(np.array_equal(g, w) for g, w in zip(got_rg, want_rg)):
                    print("REGIONS MISMATCH", tag, f"max_gap={max_gap} min_kmers={min_kmers} regions={len(got_rg[1])}/{len(want_rg[1])}"); bad += 1
            for o in (mp, qp, tp, hits, Q, T):
                o.free()
        except Exception as e:  # noqa: BLE001
            print("ERROR", tag, repr(e)); bad += 1
    ctx.close()
    print(f"matchpos: {n_refused} of {cases} cases refused by max_pairs")
    return bad


def run_crafted(cases: int, seed: int, knobs=None) -> int:
    """Hand-made sketches (ks_sketches_from_host) instead of residues: random mixtures of the ingredients of
    tests/crafted_sketches.py — hashes on both sides of join-bucket boundaries, clusters that share their prefix, 1 and
    max_hash, abundances from the edge set (0 .. 2^32 - 1) — with at most 400 targets and 400 queries.  Search rows, matched
    pairs, the per-row statistics, one containment threshold and the union are compared with the numpy / Python references
    there.  Returns the number of failures."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import crafted_sketches as cs
    rng = np.random.default_rng([seed, 2])
    knobs = knobs or {}
    bad = 0
    ctx = ks.Context(0, follow_debug_env=True)
    try:
        for case in range(cases):
            bad += _crafted_case(ctx, cs, rng, case, knobs)
    finally:
        ctx.close()
    return bad


def _crafted_case(ctx, cs, rng, case, knobs) -> int:
    """One case of run_crafted(): 0 if it matches the references, 1 otherwise (with one line printed)."""
    scaled = int(rng.choice([1, 1, 3, 5, 1000, cs.U32_MAX]))
    mh = cs.max_hash(scaled)
    n_t, n_q = int(rng.integers(1, 401)), int(rng.integers(1, 401))
    pool = [1, mh, mh - 1]
    for pbits in rng.choice(cs.PBITS_EDGES, 2, replace=False).tolist():
        K = cs.prefix_mul(pbits, mh)
        top = cs.join_prefix(mh, K)
        for b in (rng.integers(1, top + 1, 150).tolist() if top else []):
            w = ((b << 32) + K - 1) // K
            pool += [x for x in ((w << 32) - 1, w << 32) if 0 < x <= mh]
    for _ in range(int(rng.integers(1, 5))):  # clusters: equal prefixes, equal fingerprints, consecutive values
        base, width = int(rng.integers(1, mh, dtype=np.uint64, endpoint=True)), 1 << int(rng.integers(1, 34))
        pool += [min(base + int(x), mh) for x in rng.integers(0, width, int(rng.integers(20, 400)))]
    pool += rng.integers(1, mh, 200, dtype=np.uint64, endpoint=True).tolist()
    pool = np.array(sorted(set(pool)), np.uint64)
    edges = np.asarray(cs.ABUND_EDGES if rng.random() < 0.85 else (0,), np.uint32)
    tag = f"crafted case {case}: scaled={scaled} n_t={n_t} n_q={n_q} hashes={len(pool)} abundances={'edges' if len(edges) > 1 else '0'}"
    held = []
    try:
        in_t = pool[rng.random(len(pool)) < 0.8]
        in_q = np.concatenate([in_t[rng.random(len(in_t)) < 0.6], pool[rng.random(len(pool)) < 0.25]])
        ct, cq = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        th, qh = np.tile(in_t, ct), np.tile(in_q, cq)
        T = cs._csr(rng.integers(0, n_t, len(th)), th, rng.choice(edges, len(th)), n_t)
        Q = cs._csr(rng.integers(0, n_q, len(qh)), qh, np.ones(len(qh)), n_q)
        cs.check_valid(T, scaled); cs.check_valid(Q, scaled)
        rows = cs.ref_join(T, Q)
        assert int(rows[2].sum()) < cs.PAIR_BOUND
        thr = float(rng.choice([1e-300, 0.05, 0.5, 1.0]))
        sel = cs.keep(rows, Q, thr)
        with knobs_set(knobs):
            dT = ctx.sketches_from_host(*T, 10, scaled, "protein"); held.append(dT)
            dQ = ctx.sketches_from_host(*Q, 10, scaled, "protein"); held.append(dQ)
            ix = ctx.index_build(dT); held.append(ix)
            H = ctx.search(ix, dQ, abund_stats=True); held.append(H)
            got, (m2, ss) = H.to_host(), H.abund_stats_to_host()
            pairs = H.n_pair_instances
            Hp = ctx.search(ix, dQ); held.append(Hp)
            plain = Hp.to_host()
            Hk = ctx.search(ix, dQ, min_containment=thr); held.append(Hk)
            kept = Hk.to_host()
            U = dT.union(); held.append(U)
            union = U.to_host()
        if not (all(np.array_equal(g, w) for g, w in zip(got, rows)) and all(np.array_equal(g, w) for g, w in zip(plain, rows))
                and pairs == int(rows[2].sum())):
            print("CRAFTED SEARCH MISMATCH", tag, f"hits={len(got[0])}/{len(rows[0])} pairs={pairs}/{int(rows[2].sum())}"); return 1
        want_m2, want_ss = cs.ref_stats(rows, T, Q)
        if not (np.array_equal(m2, want_m2) and np.array_equal(ss.view(np.uint64), want_ss.view(np.uint64))):
            print("CRAFTED STATISTICS MISMATCH", tag); return 1
        if not all(np.array_equal(g, w[sel]) for g, w in zip(kept, rows)):
            print("CRAFTED THRESHOLD MISMATCH", tag, f"min_containment={thr}"); return 1
        if not all(np.array_equal(g, w) for g, w in zip(union, cs.ref_union(T))):
            print("CRAFTED UNION MISMATCH", tag); return 1
    except Exception as e:  # noqa: BLE001
        print("ERROR", tag, repr(e)); return 1
    finally:
        for o in reversed(held):  # (device objects of the case, on every path)
            o.free()
    return 0


def run_big(cases: int, seed: int) -> int:
    """Batches of 5k-60k proteins (many tiles, look-back chains, full partition paths): sketch vs oracle; search by the
    fused path (postings from the sketch kernel) vs the plain path, and partitioned vs LSD index build — GPU vs GPU,
    the pairwise oracle search is quadratic."""
    from kmerseek_amd import synth
    rng = np.random.default_rng(seed)
    ctx = ks.Context(0, follow_debug_env=True)
    bad = 0
    for case in range(cases):
        k = int(rng.choice([5, 7, 10, 16, 21, 24, 32]))
        scaled = int(rng.choice([1, 1, 2, 5, 20]))
        mol = str(rng.choice(["protein", "dayhoff", "hp"]))
        if mol == "hp" and k < 16:
            k = 16  # 2-letter alphabet: below ~16 every protein shares every k-mer and the match list exceeds its 2^32 cap
        nt, nq = int(rng.integers(5000, 60000)), int(rng.integers(5000, 60000))
        t_res, t_off = synth.proteome(nt, stream=5000 + case, hi=int(rng.choice([300, 3000, 9000])))
        q_res, q_off = synth.queries(nq, t_res, t_off, stream=6000 + case, frac_related=float(rng.choice([0.0, 0.2, 0.9])))
        tag = f"big case {case}: k={k} scaled={scaled} {mol} nt={nt} nq={nq}"
        if case % 4 == 3:
            # a big batch of PEPTIDES (>= 262,144 sequences: packed tiles then take up to 1024 sequences each — more than a
            # tile's LDS tables hold — and neighbouring peptides share k-mers)
            n = int(rng.integers(270000, 400000))
            lens = rng.integers(0, int(rng.choice([12, 20, 40])), n).astype(np.uint64)
            offs = np.zeros(n + 1, np.uint64)
            np.cumsum(lens, out=offs[1:])
            alpha = np.frombuffer(ALPHABETS[int(rng.integers(0, len(ALPHABETS)))], np.uint8)
            res = rng.choice(alpha, size=int(offs[-1])).astype(np.uint8)
            kk = int(rng.choice([2, 3, 5, 7]))
            tag = f"big case {case}: peptides k={kk} scaled={scaled} {mol} n={n}"
            try:
                got = ctx.sketch_batch(res, offs, kk, scaled, mol).to_host()
                if not all(np.array_equal(g, w) for g, w in zip(got, oracle.sketch_batch(res, offs, kk, scaled, mol, n_threads=16))):
                    print("SKETCH MISMATCH", tag); bad += 1
            except Exception as e:  # noqa: BLE001
                print("ERROR", tag, repr(e)); bad += 1
            continue
        try:
            T = ctx.sketch_batch(t_res, t_off, k, scaled, mol)
            if not all(np.array_equal(g, w) for g, w in zip(T.to_host(), oracle.sketch_batch(t_res, t_off, k, scaled, mol, n_threads=16))):
                print("SKETCH MISMATCH", tag); bad += 1; continue
            ix = ctx.index_build(T)
            Q = ctx.sketch_batch(q_res, q_off, k, scaled, mol)
            plain = ctx.search(ix, Q).to_host()
            d_res, d_off = ctx.to_device(q_res), ctx.to_device(q_off)
            Qf = ctx.sketch_queries_device(ix, d_res.ptr, d_off.ptr, nq, len(q_res))
            fused = ctx.search(ix, Qf).to_host()
            os.environ["KS_DEBUG_INDEX_LSD"] = "1"
            lsd = ctx.search(ctx.index_build(T), Q).to_host()
            del os.environ["KS_DEBUG_INDEX_LSD"]
            if not all(np.array_equal(x, y) for x, y in zip(plain, fused)):
                print("FUSED != PLAIN", tag); bad += 1; continue
            one = ctx.sketch_search_device(ix, d_res.ptr, d_off.ptr, nq, len(q_res), max_seq_len=int((q_off[1:] - q_off[:-1]).max()),
                                           want_sketches=False)[1].to_host()
            if not all(np.array_equal(x, y) for x, y in zip(plain, one)):
                print("ONE CALL != PLAIN", tag); bad += 1; continue
            if not all(np.array_equal(x, y) for x, y in zip(plain, lsd)):
                print("PARTITIONED INDEX != LSD INDEX", tag); bad += 1; continue
            # oracle on a few queries
            qo, qm, _ = Q.to_host()
            to, tm, ta = T.to_host()
            pick = rng.choice(nq, size=6, replace=False)
            for qi in pick.tolist():
                w = oracle.manysearch(np.array([0, qo[qi + 1] - qo[qi]], np.uint64), qm[int(qo[qi]):int(qo[qi + 1])], to, tm, ta, n_threads=16)
                sel = plain[0] == qi
                if not (np.array_equal(plain[1][sel], w[1]) and np.array_equal(plain[2][sel], w[2]) and np.array_equal(plain[3][sel], w[3])):
                    print("SEARCH MISMATCH", tag, f"query {qi}"); bad += 1; break
        except Exception as e:  # noqa: BLE001
            print("ERROR", tag, repr(e)); bad += 1
    ctx.close()
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--big", action="store_true", help="few large batches instead of many small ones")
    ap.add_argument("--entries", action="store_true", help="also ks_sketch_batch_device, and random hints for the one-call search")
    ap.add_argument("--matchpos", action="store_true", help="match-position cases (ks_match_positions against a numpy join)")
    ap.add_argument("--crafted", action="store_true", help="hand-made sketches on the edges of the search arithmetic (numpy references)")
    ap.add_argument("--knob", action="append", default=[], help="NAME=VALUE: KS_DEBUG_NAME around every case (repeatable)")
    a = ap.parse_args()
    knobs = dict(kv.split("=", 1) for kv in a.knob)
    if a.matchpos:
        bad = run_matchpos(a.cases, a.seed, knobs=knobs)
    elif a.crafted:
        bad = run_crafted(a.cases, a.seed, knobs=knobs)
    else:
        bad = run_big(a.cases, a.seed) if a.big else run(a.cases, a.seed, knobs=knobs, entries=a.entries)
    print(f"{a.cases} cases, {bad} failures")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
