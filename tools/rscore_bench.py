#!/usr/bin/env python3
"""Cost of the region-score pass (ks_regions_score) on one MI355X, inputs resident on the device.

    python tools/rscore_bench.py [--repeats 7] [--x-drop 20] [--skip-200k] [--max-pairs N]

Wall time of the synchronous call (median, min, max over the repeats) and the event time of its one kernel (ks_timing), without
and with KS_RSCORE_EXTEND (the +1 / -1 matrix), on the regions (max_gap 0, min_kmers 1) of
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query, as tools/regions_bench.py does
beside the ks_match_regions call that made them, timed the same way in the same process.  Also: regions per second, the mean
region length before and after the extension, and the bytes the pass has to move (per region 12 of placement read, a row search,
36 of columns written; per residue pair of the core and of the kept extension 2 — the pairs a walk reads past
its best prefix are not counted) against the device's measured copy rate.  Prints one JSON line per workload."""
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


def measure(ctx, name, hits, qp, tp, q_batch, t_batch, args, rates):
    """q_batch / t_batch: (d_res, d_off, n_seqs, n_res)"""
    import kmerseek_amd as ks
    try:
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_region_scores", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    ctx.match_regions(mp).free()  # warm-up: pool blocks
    t_rg, rg = _timed(ctx, lambda: ctx.match_regions(mp), args.repeats)
    k_rg = _kernels(ctx, lambda: ctx.match_regions(mp))
    seed_len = rg.to_host()[3]
    cases = []
    for extend in (False, True):
        call = lambda: ctx.score_regions_device(rg, hits, *q_batch, *t_batch, extend=extend, x_drop=args.x_drop)
        call().free()
        ts, sc = _timed(ctx, call, args.repeats)
        length = sc.to_host()[3]
        sc.free()
        kern = _kernels(ctx, call)
        kern_ms = sum(ms for _, ms in kern.values())
        # the residue pairs of the cores, and with the extension of what the walks kept
        pairs = int(seed_len.sum()) + (int((length - seed_len).sum()) if extend else 0)
        b = rg.n_regions * (12 + 36) + 2 * pairs
        cases.append({"extend": extend, "x_drop": args.x_drop if extend else None, "wall": _spread(ts), "kernels": kern,
                      "kernel_ms": round(kern_ms, 4), "regions_per_s": round(rg.n_regions / max(kern_ms, 1e-9) * 1e3),
                      "mean_length": round(float(length.mean()), 2) if len(length) else 0.0, "model_bytes": b,
                      "gb_per_s": round(b / max(kern_ms, 1e-9) / 1e6, 2), "ms_at_copy_rate": round(b / (rates["copy_gb_per_s"] * 1e6), 4)})
    out = {"what": "device_region_scores", "workload": name, "rows": rg.n_rows, "pairs": mp.n_pairs, "regions": rg.n_regions,
           "mean_seed_length": round(float(seed_len.mean()), 2) if len(seed_len) else 0.0,
           "match_regions": {"wall": _spread(t_rg), "kernels": k_rg, "kernel_ms": round(sum(ms for _, ms in k_rg.values()), 4)},
           "cases": cases, "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}
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
        rates = ctx.device_rates()
        dq, dt = _device_batch(ctx, q_res, q_off), _device_batch(ctx, t_res, t_off)
        qb, tb = (dq[0].ptr, dq[1].ptr, n, int(q_off[-1])), (dt[0].ptr, dt[1].ptr, n, int(t_off[-1]))
        T = ctx.sketch_batch_device(*tb, k, scaled, mol)
        Q = ctx.sketch_batch_device(*qb, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qp = ctx.kmer_positions_table_device(*qb, k, scaled, mol)
        tp = ctx.kmer_positions_table_device(*tb, k, scaled, mol)
        measure(ctx, "10k_x_10k_protein_k7_s1", hits, qp, tp, qb, tb, args, rates)


def all_vs_all(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 200_000, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    with ks.Context(0) as ctx:
        rates = ctx.device_rates()
        d = _device_batch(ctx, res, off)
        b = (d[0].ptr, d[1].ptr, n, int(off[-1]))
        T = ctx.sketch_batch_device(*b, k, scaled, mol)
        all_hits = ctx.search(ctx.index_build(T), T)
        hits = ctx.best_hits(all_hits, 10)
        all_hits.free()
        tab = ctx.kmer_positions_table_device(*b, k, scaled, mol)
        measure(ctx, "200k_all_vs_all_hp_k24_s5_best10", hits, tab, tab, b, b, args, rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--x-drop", type=int, default=20)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
