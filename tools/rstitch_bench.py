#!/usr/bin/env python3
"""Cost and effect of the stitch (ks_regions_stitch) on one MI355X, inputs resident on the device.

    python tools/rstitch_bench.py [--repeats 7] [--max-overlap 5] [--skew-cost 1] [--skip-200k] [--max-pairs N] [--planted N]

On the alignments the cull kept (default options) of three inputs
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
    planted insertions   protein k=7 scaled=1    --planted targets of 250 .. 400 residues; query i is target i with one or two
                         stretches of 20 .. 60 residues inserted, and in every fourth pair a stretch of 5 .. 50 replaced by one
                         of 5 .. 50 (generated here, seeded: the first two inputs chain almost nothing)
in one process, the calls interleaved round by round:
    counts   chain members, rows of more than one member, links by class (pure run / filled / open), trimmed columns, ops
    stitch   wall time of the synchronous call and event time of its kernels (ks_timing), beside the traceback
             (ks_regions_traceback) of the SAME alignments, timed the same way: the yardstick of a pass that runs a dynamic
             program with directions and walks it back
    ratio    stitch kernels / traceback kernels
Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4), "n": len(xs)}


def _done(out):
    if hasattr(out, "free"):
        out.free()


def _kernels(ctx, fn):
    ctx.timing_enable(1)
    ctx.timing_reset()
    _done(fn())
    kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items() if c}  # (names of earlier passes stay listed with 0 launches)
    ctx.timing_enable(0)
    return kern


def _interleaved(ctx, calls, repeats):
    """calls: name -> a function that returns an object to free.  Every round runs each call once, wall-timed; then every round
    once more under event timing.  -> name -> {wall, kernel, kernel_median_ms_by_name}"""
    for fn in calls.values():
        _done(fn())  # warm-up: pool blocks
    wall = {n: [] for n in calls}
    for _ in range(repeats):
        for n, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall[n].append(time.perf_counter() - t0)
            _done(out)
    runs = {n: [] for n in calls}
    for _ in range(repeats):
        for n, fn in calls.items():
            runs[n].append(_kernels(ctx, fn))
    res = {}
    for n in calls:
        ks_ms = [sum(ms for _, ms in r.values()) for r in runs[n]]
        by_kernel = {kn: round(sorted(r.get(kn, [0, 0.0])[1] for r in runs[n])[repeats // 2], 4) for kn in runs[n][0]}
        res[n] = {"wall": _spread(wall[n]), "kernel": _spread([ms * 1e-3 for ms in ks_ms]), "kernel_median_ms_by_name": by_kernel}
    return res


def measure(ctx, name, hits, qp, tp, q_batch, t_batch, args):
    """q_batch / t_batch: (d_res, d_off, n_seqs, n_res)"""
    import numpy as np
    import kmerseek_amd as ks
    try:
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_region_stitch", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    rg_all = ctx.match_regions(mp)
    al_all = ctx.align_regions_device(rg_all, hits, *q_batch, *t_batch)
    cu = ctx.cull_regions(al_all)
    rg, al = cu.take(rg_all), cu.take(al_all)
    for o in (cu, al_all, rg_all, mp):
        o.free()
    kw = {"max_overlap": args.max_overlap, "skew_cost": args.skew_cost}
    ch = ctx.chain_regions(al, **kw)
    cg = ctx.trace_regions_device(rg, hits, *q_batch, *t_batch, al)
    st = ctx.stitch_chains_device(ch, al, cg, hits, *q_batch, *t_batch)
    h = st.to_host()
    members = h[12].astype(np.int64)
    links = int((members - 1).clip(min=0).sum())
    counts = {"rows": st.n_rows, "alignments": al.n_regions, "chain_members": ch.n_chained, "rows_of_more_than_one_member": int((members > 1).sum()),
              "longest_chain": int(members.max()) if len(members) else 0, "links": links, "filled": int(h[13].sum()), "open": int(h[14].sum()),
              "pure_or_touching": links - int(h[13].sum()) - int(h[14].sum()), "trimmed_columns": int(h[15].sum()), "ops": st.n_ops,
              "traceback_ops": cg.n_ops, "columns": int(h[11].sum()), "stitch_scratch_bytes": st.scratch_bytes,
              "traceback_scratch_bytes": cg.scratch_bytes}
    st.free()
    calls = {
        "stitch": lambda: ctx.stitch_chains_device(ch, al, cg, hits, *q_batch, *t_batch),
        "traceback": lambda: ctx.trace_regions_device(rg, hits, *q_batch, *t_batch, al),
    }
    cases = _interleaved(ctx, calls, args.repeats)
    k_med = lambda c: cases[c]["kernel"]["median_ms"]
    out = {"what": "device_region_stitch", "workload": name, "chain_options": kw, "counts": counts, **cases,
           "stitch_over_traceback_kernels": round(k_med("stitch") / max(k_med("traceback"), 1e-9), 3),
           "stitch_over_traceback_wall": round(cases["stitch"]["wall"]["median_ms"] / max(cases["traceback"]["wall"]["median_ms"], 1e-9), 3)}
    for o in (cg, ch, al, rg):
        o.free()
    print(json.dumps(out), flush=True)


def _device_batch(ctx, res, off):
    import numpy as np
    return ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(off)


def _pipeline(ctx, name, q, t, k, scaled, mol, args):
    """q, t: (res, off) host batches; sketches, search, position tables, then `measure`."""
    dq, dt = _device_batch(ctx, *q), _device_batch(ctx, *t)
    qb, tb = (dq[0].ptr, dq[1].ptr, len(q[1]) - 1, int(q[1][-1])), (dt[0].ptr, dt[1].ptr, len(t[1]) - 1, int(t[1][-1]))
    T = ctx.sketch_batch_device(*tb, k, scaled, mol)
    Q = ctx.sketch_batch_device(*qb, k, scaled, mol)
    hits = ctx.search(ctx.index_build(T), Q)
    qp = ctx.kmer_positions_table_device(*qb, k, scaled, mol)
    tp = ctx.kmer_positions_table_device(*tb, k, scaled, mol)
    measure(ctx, name, hits, qp, tp, qb, tb, args)


def ten_k(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n = 10_000
    t_res, t_off = synth.proteome(n, stream=0)
    q_res, q_off = synth.queries(n, t_res, t_off, stream=1)
    with ks.Context(0) as ctx:
        _pipeline(ctx, "10k_x_10k_protein_k7_s1", (q_res, q_off), (t_res, t_off), 7, 1, "protein", args)


def all_vs_all(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 200_000, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    with ks.Context(0) as ctx:
        d = _device_batch(ctx, res, off)
        b = (d[0].ptr, d[1].ptr, n, int(off[-1]))
        T = ctx.sketch_batch_device(*b, k, scaled, mol)
        all_hits = ctx.search(ctx.index_build(T), T)
        hits = ctx.best_hits(all_hits, 10)
        all_hits.free()
        tab = ctx.kmer_positions_table_device(*b, k, scaled, mol)
        measure(ctx, "200k_all_vs_all_hp_k24_s5_best10", hits, tab, tab, b, b, args)


def planted_batch(n, seed=2028):
    """(queries, targets): target i random over the 20 residues, query i that target with planted insertions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    seq = lambda m: bytes(aa[rng.integers(0, 20, m)])
    qs, ts = [], []
    for i in range(n):
        t = seq(int(rng.integers(250, 401)))
        cuts = sorted(int(c) for c in rng.integers(40, len(t) - 40, int(rng.integers(1, 3))))
        q, last = b"", 0
        for c in cuts:
            q += t[last:c] + seq(int(rng.integers(20, 61)))
            last = c
        q += t[last:]
        if i % 4 == 0:  # a replaced stretch: a rectangle with two sides
            c, m = int(rng.integers(20, len(q) - 80)), int(rng.integers(5, 51))
            q = q[:c] + seq(int(rng.integers(5, 51))) + q[c + m:]
        qs.append(q); ts.append(t)
    return qs, ts


def planted(args):
    import kmerseek_amd as ks
    qs, ts = planted_batch(args.planted)
    with ks.Context(0) as ctx:
        _pipeline(ctx, f"planted_insertions_{args.planted}_protein_k7_s1", ks.pack(qs), ks.pack(ts), 7, 1, "protein", args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-overlap", type=int, default=5)
    ap.add_argument("--skew-cost", type=int, default=1)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--planted", type=int, default=20_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)
    planted(args)


if __name__ == "__main__":
    main()
