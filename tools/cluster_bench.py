#!/usr/bin/env python3
"""Cost of the cluster pass (ks_hits_cluster) on one MI355X, inputs resident on the device.

    python tools/cluster_bench.py [--repeats 7] [--nodes 200000]

Workload: BASELINE configs[4], 200k proteins all-vs-all, hp k=24 scaled=5.  Wall time of the synchronous call (median, min, max
over the repeats) at jaccard thresholds 0, 0.1 and 0.5, on both hooking paths (KS_DEBUG_CLUSTER_PATH = 1: the plain lane-per-row
path; 2: the wave-uniform query path), beside the search step of the same run and the per-kernel event times of one timed
pass (ks_timing).  The yardstick: the bytes the pass must read once — 12 bytes per row (qid, tid, intersect) plus the size
lookups (the offsets table, 8 bytes per node: the rows hit it in cache) — against the device's measured copy rate
(ks_bench_device_rates).  The per-node work (36 bytes of scratch per node, a key sort of n keys) does not
show at 150 rows per node.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = (0.0, 0.1, 0.5)
PATHS = (("plain", "1"), ("wave_uniform", "2"))
KNOB = "KS_DEBUG_CLUSTER_PATH"


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


def model_bytes(rows, nodes):
    """bytes the pass has to read once: see the module docstring"""
    return rows * 12 + (nodes + 1) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=200_000)
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = args.nodes, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    os.environ.pop(KNOB, None)
    with ks.Context(0, follow_debug_env=True) as ctx:
        rates = ctx.device_rates()
        d_r, d_o = ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(off)
        S = ctx.sketch_batch_device(d_r.ptr, d_o.ptr, n, int(off[-1]), k, scaled, mol)
        ix = ctx.index_build(S)
        for _ in range(2):  # warm-up: pool blocks, row hint
            hits = ctx.search(ix, S)
            ctx.cluster(hits, "jaccard", 0.1, nodes=S).free()
            hits.free()
        t_search, hits = _timed(ctx, lambda: ctx.search(ix, S), args.repeats)
        b = model_bytes(hits.count, n)
        cases = []
        for thr in THRESHOLDS:
            for name, knob in PATHS:
                os.environ[KNOB] = knob
                ts, cl = _timed(ctx, lambda: ctx.cluster(hits, "jaccard", thr, nodes=S), args.repeats)
                shape = {"n_clusters": cl.n_clusters, "n_edges": cl.n_edges, "largest": cl.largest}
                cl.free()
                ctx.timing_enable(1)
                ctx.timing_reset()
                ctx.cluster(hits, "jaccard", thr, nodes=S).free()
                kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
                ctx.timing_enable(0)
                kern_ms = sum(ms for _, ms in kern.values())
                hook_ms = kern.get("cluster_hook", [0, 0.0])[1]
                cases.append(dict(shape, threshold=thr, path=name, wall=_spread(ts), kernels=kern, kernel_ms=round(kern_ms, 4),
                                  hook_gb_per_s=round(b / max(hook_ms, 1e-9) / 1e6, 2)))
        os.environ.pop(KNOB, None)
        print(json.dumps({
            "what": "device_cluster", "workload": f"{n}_all_vs_all_{mol}_k{k}_s{scaled}", "nodes": n, "rows": hits.count,
            "search": _spread(t_search), "cases": cases, "model_bytes": b,
            "ms_at_copy_rate": round(b / (rates["copy_gb_per_s"] * 1e6), 4), "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}), flush=True)


if __name__ == "__main__":
    main()
