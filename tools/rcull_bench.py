#!/usr/bin/env python3
"""Cost and effect of the region cull (ks_regions_cull_device) on one MI355X, inputs resident on the device.

    python tools/rcull_bench.py [--repeats 7] [--overlap 100] [--x-drop 20] [--skip-200k] [--max-pairs N]

On the regions (max_gap 0, min_kmers 1) of the two workloads of tools/rtrace_bench.py
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
aligned with the default options and scored with extension (x_drop as tools/rscore_bench.py), in one process, the calls
interleaved round by round:
    counts   kept / removed (they name a keeper) / dropped, of the alignments' cull and of the extended regions' cull
    cull     wall time of the synchronous call and event time of its kernels (ks_timing), for both inputs, beside ks_regions_score
             with extension on the same regions, timed the same way
    take     the three takes (regions, scores, alignments) by the alignments' cull
    trace    the kernels of ks_regions_traceback on all regions against those on the kept ones (taken regions and alignments)
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


def _kernels(ctx, fn):
    ctx.timing_enable(1)
    ctx.timing_reset()
    fn().free()
    kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items() if c}  # (names of earlier passes stay listed with 0 launches)
    ctx.timing_enable(0)
    return kern


def _interleaved(ctx, calls, repeats):
    """calls: name -> a function that returns an object to free.  Every round runs each call once, wall-timed; then every round
    once more under event timing.  -> name -> {wall, kernel, kernel_median_ms_by_name}"""
    for fn in calls.values():
        fn().free()  # warm-up: pool blocks
    wall = {n: [] for n in calls}
    for _ in range(repeats):
        for n, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall[n].append(time.perf_counter() - t0)
            out.free()
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


def _counts(cu, in_offs):
    """in_offs: the row offsets of the cull's input"""
    import numpy as np
    offs, _, _, nm, keeper, _ = cu.to_host()
    dropped = int((keeper == 0xFFFFFFFF).sum())
    return {"regions": cu.n_regions, "kept": cu.n_kept, "removed": cu.n_regions - cu.n_kept - dropped, "dropped": dropped,
            "rows": cu.n_rows, "rows_that_lose_a_region": int((np.diff(offs.astype("int64")) < np.diff(in_offs.astype("int64"))).sum()),
            "largest_n_merged": int(nm.max()) if len(nm) else 0}


def measure(ctx, name, hits, qp, tp, q_batch, t_batch, args):
    """q_batch / t_batch: (d_res, d_off, n_seqs, n_res)"""
    import kmerseek_amd as ks
    try:
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_region_cull", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    rg = ctx.match_regions(mp)
    al = ctx.align_regions_device(rg, hits, *q_batch, *t_batch)
    sc = ctx.score_regions_device(rg, hits, *q_batch, *t_batch, extend=True, x_drop=args.x_drop)
    kw = {"overlap_pct": args.overlap}
    cu_al, cu_sc = ctx.cull_regions(al, **kw), ctx.cull_regions(sc, **kw)
    in_offs = rg.to_host()[0]
    counts = {"alignments": _counts(cu_al, in_offs), "extended_regions": _counts(cu_sc, in_offs)}
    t_rg, t_al = cu_al.take(rg), cu_al.take(al)
    calls = {
        "cull_alignments": lambda: ctx.cull_regions(al, **kw),
        "cull_extended_regions": lambda: ctx.cull_regions(sc, **kw),
        "regions_score_extend": lambda: ctx.score_regions_device(rg, hits, *q_batch, *t_batch, extend=True, x_drop=args.x_drop),
        "take_regions": lambda: cu_al.take(rg),
        "take_scores": lambda: cu_al.take(sc),
        "take_alignments": lambda: cu_al.take(al),
        "traceback_all": lambda: ctx.trace_regions_device(rg, hits, *q_batch, *t_batch, al),
        "traceback_kept": lambda: ctx.trace_regions_device(t_rg, hits, *q_batch, *t_batch, t_al),
    }
    cases = _interleaved(ctx, calls, args.repeats)
    k_med = lambda c: cases[c]["kernel"]["median_ms"]
    out = {"what": "device_region_cull", "workload": name, "overlap_pct": args.overlap, "counts": counts, **cases,
           "cull_kernel_ratio_to_score_extend": round(k_med("cull_alignments") / max(k_med("regions_score_extend"), 1e-9), 3),
           "traceback_kernel_kept_over_all": round(k_med("traceback_kept") / max(k_med("traceback_all"), 1e-9), 3)}
    for o in (t_rg, t_al, cu_al, cu_sc, sc, al, rg, mp):
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
    ap.add_argument("--overlap", type=int, default=100)
    ap.add_argument("--x-drop", type=int, default=20)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
