#!/usr/bin/env python3
"""Cost of the profile passes on one MI355X, inputs resident on the device.

    python tools/profile_bench.py [--repeats 7] [--band 16] [--gap-open 11] [--gap-extend 1] [--x-drop 30] [--beta 10]

On the 10k x 10k workload of tools/ralign_bench.py (protein k=7 scaled=1, synthetic proteome, queries related to it; +1 / -1
matrix): the regions are aligned, culled and traced, the kept alignments piled up on the queries with their residue counts, and
then, each timed as the wall time of the synchronous call and as the event time of its kernels (ks_timing), median [min - max]:
    profile_build     ks_profile_build_pileup on that pileup
    align / trace     ks_regions_align and ks_regions_traceback under the matrix, on the kept regions
    align_profile / trace_profile   the same two against the profile, on the same regions
kernel_ratio_align / kernel_ratio_trace: profile over matrix, the kernels alone — what the staged profile rows (64 x 28 bytes a
chunk into the wave's LDS rows, where the matrix form reads one staged matrix) cost a row of the program.
Prints one JSON line."""
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


def _measure(ctx, call, repeats):
    call().free()  # warm-up: pool blocks
    wall, kern = [], []
    for _ in range(repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
        out.free()
    for _ in range(repeats):
        ctx.timing_enable(1)
        ctx.timing_reset()
        call().free()
        kern.append(sum(ms for c, ms in ctx.timing().values() if c) * 1e-3)
        ctx.timing_enable(0)
    return {"wall": _spread(wall), "kernel": _spread(kern)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--gap-open", type=int, default=11)
    ap.add_argument("--gap-extend", type=int, default=1)
    ap.add_argument("--x-drop", type=int, default=30)
    ap.add_argument("--beta", type=float, default=10.0)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 10_000, 7, 1, "protein"
    t_res, t_off = synth.proteome(n, stream=0)
    q_res, q_off = synth.queries(n, t_res, t_off, stream=1)
    opts = {"band": args.band, "gap_open": args.gap_open, "gap_extend": args.gap_extend, "x_drop": args.x_drop}
    with ks.Context(0) as ctx:
        pad = np.zeros(16, np.uint8)
        dq, dqo = ctx.to_device(np.concatenate([q_res, pad])), ctx.to_device(q_off)
        dt, dto = ctx.to_device(np.concatenate([t_res, pad])), ctx.to_device(t_off)
        qb, tb = (dq.ptr, dqo.ptr, n, int(q_off[-1])), (dt.ptr, dto.ptr, n, int(t_off[-1]))
        T, Q = ctx.sketch_batch_device(*tb, k, scaled, mol), ctx.sketch_batch_device(*qb, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qp, tp = ctx.kmer_positions_table_device(*qb, k, scaled, mol), ctx.kmer_positions_table_device(*tb, k, scaled, mol)
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
        rg_all = ctx.match_regions(mp)
        al_all = ctx.align_regions_device(rg_all, hits, *qb, *tb, **opts)
        cu = ctx.cull_regions(al_all)
        rg, al = cu.take(rg_all), cu.take(al_all)
        cg = ctx.trace_regions_device(rg, hits, *qb, *tb, al)
        pu = ctx.pileup(cg, hits, side="query", offsets=q_off, alignments=al, profile=True, other_res=t_res, other_off=t_off)
        params = ks.profile_params(None, beta=args.beta)
        import ctypes as C

        def build():
            o, keep = params._opts()
            out = C.c_void_p()
            ctx._check(ctx._L.ks_profile_build_pileup(ctx._h, pu._h, C.c_void_p(qb[0]), C.c_void_p(qb[1]), qb[2], qb[3], C.byref(o), C.byref(out)))
            return ks.Profile(ctx, out)
        prof = build()
        n_obs = prof.to_host()[2]
        al_p = ctx.align_regions_device(rg, hits, *qb, *tb, profile=prof, **opts)
        cases = {
            "profile_build": _measure(ctx, build, args.repeats),
            "align": _measure(ctx, lambda: ctx.align_regions_device(rg, hits, *qb, *tb, **opts), args.repeats),
            "align_profile": _measure(ctx, lambda: ctx.align_regions_device(rg, hits, *qb, *tb, profile=prof, **opts), args.repeats),
            "trace": _measure(ctx, lambda: ctx.trace_regions_device(rg, hits, *qb, *tb, al), args.repeats),
            "trace_profile": _measure(ctx, lambda: ctx.trace_regions_device(rg, hits, *qb, *tb, al_p, profile=prof), args.repeats),
        }
        k_med = lambda c: cases[c]["kernel"]["median_ms"]
        host_m, host_p = al.to_host(), al_p.to_host()
        print(json.dumps({"what": "device_profile", "workload": "10k_x_10k_protein_k7_s1", "rows": rg.n_rows, "kept_regions": rg.n_regions,
                          "query_residues": int(q_off[-1]), "residues_observed": int((n_obs > 0).sum()), "opts": opts, "beta": args.beta, **cases,
                          "residues_per_s_build": round(int(q_off[-1]) / max(k_med("profile_build"), 1e-9) * 1e3),
                          "kernel_ratio_align": round(k_med("align_profile") / max(k_med("align"), 1e-9), 3),
                          "kernel_ratio_trace": round(k_med("trace_profile") / max(k_med("trace"), 1e-9), 3),
                          "mean_q_length": [round(float(host_m[2].mean()), 2), round(float(host_p[2].mean()), 2)],
                          "mean_score": [round(float(host_m[5].mean()), 2), round(float(host_p[5].mean()), 2)]}), flush=True)


if __name__ == "__main__":
    main()
