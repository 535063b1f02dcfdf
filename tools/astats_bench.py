#!/usr/bin/env python3
"""Cost of the alignment statistics (ks_residue_composition_device, ks_raligns_stats) on one MI355X, inputs resident on the device.

    python tools/astats_bench.py [--repeats 7] [--skip-200k] [--max-pairs N] [--lambda 0.267] [--K 0.041]

On the gapped alignments (ks_regions_align, default options) of two inputs
    10k x 10k            protein k=7 scaled=1    (synthetic proteome, queries related to it)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
in one process, the calls interleaved round by round:
    composition   the residue composition of the target batch alone: wall time of the synchronous call, event time of its
                  kernels (ks_timing) and the residues per second of those kernels
    stats         ks_raligns_stats with the caller's (lambda, K), with the composition-based rescaling and — stats_plain —
                  with KS_ASTATS_NO_COMPOSITION, timed the same way
    align         ks_regions_align on the SAME regions in the same job: the yardstick (the pass whose scores these are)
    ratio         stats kernels / align kernels
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
        print(json.dumps({"what": "device_alignment_stats", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    rg = ctx.match_regions(mp)
    mp.free()
    al = ctx.align_regions_device(rg, hits, *q_batch, *t_batch)
    qc, tc = ctx.residue_composition_device(*q_batch), ctx.residue_composition_device(*t_batch)
    params = (args.lam, args.K)
    st = ctx.alignment_stats(al, hits, qc, tc, params=params)
    status, _, ratio, _, evalue, _, _ = st.to_host()
    counts = {"rows": st.n_rows, "alignments": st.n_entries, "fallback_rows": st.n_fallback, "lambda_std": st.lambda_std,
              "ratio_median": float(np.median(ratio)) if len(ratio) else None, "rows_at_ratio_max": int((ratio == 1.0).sum()),
              "evalue_below_1e-3": int((evalue < 1e-3).sum()), "target_residues": t_batch[3], "target_seqs": t_batch[2]}
    st.free()
    calls = {
        "composition": lambda: ctx.residue_composition_device(*t_batch),
        "stats": lambda: ctx.alignment_stats(al, hits, qc, tc, params=params),
        "stats_plain": lambda: ctx.alignment_stats(al, hits, qc, tc, params=params, composition=False),
        "align": lambda: ctx.align_regions_device(rg, hits, *q_batch, *t_batch),
    }
    cases = _interleaved(ctx, calls, args.repeats)
    k_med = lambda c: cases[c]["kernel"]["median_ms"]
    out = {"what": "device_alignment_stats", "workload": name, "params": params, "counts": counts, **cases,
           "composition_residues_per_s": round(t_batch[3] / max(k_med("composition") * 1e-3, 1e-12)),
           "stats_over_align_kernels": round(k_med("stats") / max(k_med("align"), 1e-9), 4),
           "stats_plain_over_align_kernels": round(k_med("stats_plain") / max(k_med("align"), 1e-9), 4)}
    for o in (qc, tc, al, rg):
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
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.267)
    ap.add_argument("--K", type=float, default=0.041)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
