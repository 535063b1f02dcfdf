#!/usr/bin/env python3
"""Cost of the traceback pass (ks_regions_traceback) on one MI355X, inputs resident on the device.

    python tools/rtrace_bench.py [--repeats 5] [--band 16] [--gap-open 11] [--gap-extend 1] [--x-drop 30] [--eqx]
                                 [--max-scratch-bytes N] [--skip-200k] [--max-pairs N]

Wall time of the synchronous call (median, min, max over the repeats) and the event time of its kernels (ks_timing: the plan,
the trace launches, the two run-length passes, the scans), under the +1 / -1 matrix, on the regions (max_gap 0, min_kmers 1) of
the two workloads of tools/ralign_bench.py
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
beside ks_regions_align on the same regions, timed the same way in the same process: the traceback as a ratio to the align
kernel.  Also: the direction bytes allocated, the slices, the ops, the rows of directions the alignments need and the columns
they have.  Prints one JSON line per workload."""
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


def _timed(ctx, fn, repeats):
    ts, out = [], None
    for _ in range(repeats):
        if out is not None:
            out.free()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _kernels(ctx, fn):
    ctx.timing_enable(1)
    ctx.timing_reset()
    fn().free()
    kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items() if c}  # (names of earlier passes stay listed with 0 launches)
    ctx.timing_enable(0)
    return kern


def measure(ctx, name, hits, qp, tp, q_batch, t_batch, args):
    """q_batch / t_batch: (d_res, d_off, n_seqs, n_res)"""
    import kmerseek_amd as ks
    try:
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_region_traceback", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    rg = ctx.match_regions(mp)
    opts = {"band": args.band, "gap_open": args.gap_open, "gap_extend": args.gap_extend, "x_drop": args.x_drop}
    al = ctx.align_regions_device(rg, hits, *q_batch, *t_batch, **opts)
    al_host = al.to_host()
    cases = {}
    for what, call in (("regions_align", lambda: ctx.align_regions_device(rg, hits, *q_batch, *t_batch, **opts)),
                       ("regions_traceback", lambda: ctx.trace_regions_device(rg, hits, *q_batch, *t_batch, al, eqx=args.eqx,
                                                                              max_scratch_bytes=args.max_scratch_bytes))):
        call().free()  # warm-up: pool blocks
        ts, out = _timed(ctx, call, args.repeats)
        if what == "regions_traceback":
            extra = {"direction_bytes": out.scratch_bytes, "slices": out.n_slices, "ops": out.n_ops,
                     "mean_ops": round(out.n_ops / max(rg.n_regions, 1), 3)}
        else:
            extra = {"opts": opts}
        out.free()
        runs = [_kernels(ctx, call) for _ in range(args.repeats)]
        ks_ms = [sum(ms for _, ms in r.values()) for r in runs]
        by_kernel = {kn: round(sorted(r[kn][1] for r in runs)[len(runs) // 2], 4) for kn in runs[0]}
        cases[what] = {"wall": _spread(ts), "kernel": _spread([ms * 1e-3 for ms in ks_ms]), "kernel_median_ms_by_name": by_kernel,
                       "regions_per_s": round(rg.n_regions / max(sorted(ks_ms)[len(ks_ms) // 2], 1e-9) * 1e3), **extra}
    k_med = lambda c: cases[c]["kernel"]["median_ms"]
    out = {"what": "device_region_traceback", "workload": name, "rows": rg.n_rows, "regions": rg.n_regions,
           "direction_rows": int((al_host[2].astype("int64") - 1).sum()), "columns": int(al_host[10].sum()),
           "with_gaps": int((al_host[9] > 0).sum()), **cases,
           "kernel_ratio_to_align": round(k_med("regions_traceback") / max(k_med("regions_align"), 1e-9), 3)}
    al.free()
    rg.free()
    mp.free()
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--gap-open", type=int, default=11)
    ap.add_argument("--gap-extend", type=int, default=1)
    ap.add_argument("--x-drop", type=int, default=30)
    ap.add_argument("--eqx", action="store_true")
    ap.add_argument("--max-scratch-bytes", type=int, default=0)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
