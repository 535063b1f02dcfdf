#!/usr/bin/env python3
"""Cost and effect of the region chain (ks_regions_chain_device) on one MI355X, inputs resident on the device.

    python tools/rchain_bench.py [--repeats 7] [--max-overlap 5] [--skew-cost 1] [--skip-200k] [--max-pairs N]

On the regions (max_gap 0, min_kmers 1) of the two workloads of tools/rcull_bench.py
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
aligned with the default options, in one process, the calls interleaved round by round:
    counts   per input (the alignments the cull kept; all alignments): regions, chained, hit rows whose chain has more than one
             member, the longest chain
    chain    wall time of the synchronous call and event time of its kernels (ks_timing), for both inputs, beside the cull
             (ks_raligns_cull, the default options) on the same regions, timed the same way, and the coverage pass
    ratio    chain kernels / cull kernels on the same regions: the two run the same loop structure on the same bytes
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
    """calls: name -> a function that returns an object to free (or nothing).  Every round runs each call once, wall-timed; then
    every round once more under event timing.  -> name -> {wall, kernel, kernel_median_ms_by_name}"""
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
        by_kernel = {kn: round(sorted(r[kn][1] for r in runs[n])[repeats // 2], 4) for kn in runs[n][0]}
        res[n] = {"wall": _spread(wall[n]), "kernel": _spread([ms * 1e-3 for ms in ks_ms]), "kernel_median_ms_by_name": by_kernel}
    return res


def _counts(ch, in_offs):
    import numpy as np
    n_mem = np.diff(ch.to_host()[0].astype("int64"))
    n_in = np.diff(np.asarray(in_offs).astype("int64"))
    return {"regions": ch.n_regions, "chained": ch.n_chained, "rows": ch.n_rows, "rows_that_chain_more_than_one": int((n_mem > 1).sum()),
            "rows_of_more_than_one_region": int((n_in > 1).sum()), "longest_row": int(n_in.max()) if len(n_in) else 0,
            "longest_chain": int(n_mem.max()) if len(n_mem) else 0}


def measure(ctx, name, hits, qp, tp, q_batch, t_batch, args):
    """q_batch / t_batch: (d_res, d_off, n_seqs, n_res)"""
    import kmerseek_amd as ks
    try:
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_region_chain", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    rg = ctx.match_regions(mp)
    al = ctx.align_regions_device(rg, hits, *q_batch, *t_batch)
    cu = ctx.cull_regions(al)
    kept = cu.take(al)
    kw = {"max_overlap": args.max_overlap, "skew_cost": args.skew_cost}
    ch_kept, ch_all = ctx.chain_regions(kept, **kw), ctx.chain_regions(al, **kw)
    counts = {"culled_alignments": _counts(ch_kept, kept.to_host()[0]), "all_alignments": _counts(ch_all, al.to_host()[0])}
    calls = {
        "chain_culled_alignments": lambda: ctx.chain_regions(kept, **kw),
        "cull_culled_alignments": lambda: ctx.cull_regions(kept),
        "chain_all_alignments": lambda: ctx.chain_regions(al, **kw),
        "cull_all_alignments": lambda: ctx.cull_regions(al),
        "coverage_min": lambda: ch_kept.coverage(hits, q_batch[1], q_batch[2], t_batch[1], t_batch[2], mode="min"),
    }
    cases = _interleaved(ctx, calls, args.repeats)
    k_med = lambda c: cases[c]["kernel"]["median_ms"]
    out = {"what": "device_region_chain", "workload": name, "options": kw, "counts": counts, **cases,
           "chain_over_cull_kernels_culled": round(k_med("chain_culled_alignments") / max(k_med("cull_culled_alignments"), 1e-9), 3),
           "chain_over_cull_kernels_all": round(k_med("chain_all_alignments") / max(k_med("cull_all_alignments"), 1e-9), 3)}
    for o in (ch_kept, ch_all, kept, cu, al, rg, mp):
        o.free()
    print(json.dumps(out), flush=True)


def _device_batch(ctx, res, off):
    import numpy as np
    return ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(off)


def ten_k(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 10_000, 7, 1, "protein"
    t_res, t_off = synth.proteome(n, stream=0)
    q_res, q_off = synth.queries(n, t_res, t_off, stream=1)
    with ks.Context(0) as ctx:
        dq, dt = _device_batch(ctx, q_res, q_off), _device_batch(ctx, t_res, t_off)
        qb, tb = (dq[0].ptr, dq[1].ptr, n, int(q_off[-1])), (dt[0].ptr, dt[1].ptr, n, int(t_off[-1]))
        T = ctx.sketch_batch_device(*tb, k, scaled, mol)
        Q = ctx.sketch_batch_device(*qb, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table_device(*qb, k, scaled, mol)
        tp = ctx.kmer_positions_table_device(*tb, k, scaled, mol)
        measure(ctx, "10k_x_10k_protein_k7_s1", hits, qp, tp, qb, tb, args)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-overlap", type=int, default=5)
    ap.add_argument("--skew-cost", type=int, default=1)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
