#!/usr/bin/env python3
"""Cost of the greedy cluster pass (ks_hits_cluster_greedy) on one MI355X, inputs resident on the device.

    python tools/greedy_bench.py [--repeats 7] [--nodes 200000] [--no-crossover]

Workload: that of tools/cluster_bench.py — BASELINE configs[4], 200k proteins all-vs-all, hp k=24 scaled=5 — at the same three
jaccard thresholds 0, 0.1 and 0.5, under both assign modes.  Per case: wall time of the synchronous call (median, min, max over
the repeats), the round count, the per-kernel event times of one further timed pass (ks_timing), and beside them
ks_hits_cluster at the same threshold and the search step, all in the same run.

Crossover (where GR_TAIL_EDGES belongs): a random subset of L non-self rows of the same hit list passes (an uploaded score
column, KS_BEST_SCORE), for L from 1k to 1M; the call is timed with grid rounds only (KS_DEBUG_GREEDY_PATH = 1), with the one
workgroup straight after the first round (= 2) and with the built-in threshold (unset).  The rest of the pass — the edge
kernel and the assign kernel over all rows, the tail — is the same in all three, so the difference of the walls is the
difference of the rounds: one tail launch against grid rounds and their waits.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = (0.0, 0.1, 0.5)
ASSIGN = ("first", "best")
KNOB = "KS_DEBUG_GREEDY_PATH"
PATHS = (("grid", "1"), ("tail", "2"), ("default", None))
CROSSOVER_EDGES = (1 << 10, 1 << 12, 1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 20)


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
    kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
    ctx.timing_enable(0)
    return kern, round(sum(ms for _, ms in kern.values()), 4)


def _set(knob):
    if knob is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = knob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--no-crossover", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = args.nodes, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    _set(None)
    with ks.Context(0, follow_debug_env=True) as ctx:
        rates = ctx.device_rates()
        d_r, d_o = ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(off)
        S = ctx.sketch_batch_device(d_r.ptr, d_o.ptr, n, int(off[-1]), k, scaled, mol)
        ix = ctx.index_build(S)
        for _ in range(2):  # warm-up: pool blocks, row hint
            hits = ctx.search(ix, S)
            ctx.cluster_greedy(hits, "jaccard", 0.1, nodes=S, assign="best").free()
            ctx.cluster(hits, "jaccard", 0.1, nodes=S).free()
            hits.free()
        t_search, hits = _timed(ctx, lambda: ctx.search(ix, S), args.repeats)
        cases = []
        for thr in THRESHOLDS:
            ts, cl = _timed(ctx, lambda: ctx.cluster(hits, "jaccard", thr, nodes=S), args.repeats)
            comp = {"n_clusters": cl.n_clusters, "largest": cl.largest, "wall": _spread(ts)}
            cl.free()
            for assign in ASSIGN:
                fn = lambda: ctx.cluster_greedy(hits, "jaccard", thr, nodes=S, assign=assign)  # noqa: E731
                fn().free()  # (the second live list is sized per threshold: the pool grows here, not in the timed calls)
                ts, cl = _timed(ctx, fn, args.repeats)
                shape = {"n_clusters": cl.n_clusters, "n_edges": cl.n_edges, "largest": cl.largest, "n_rounds": cl.n_rounds}
                cl.free()
                kern, kern_ms = _kernels(ctx, fn)
                cases.append(dict(shape, threshold=thr, assign=assign, wall=_spread(ts), kernels=kern, kernel_ms=kern_ms, components=comp))
        crossover = []
        if not args.no_crossover:
            h = hits.to_host()
            offdiag = np.nonzero(h[0] != h[1])[0]
            rng = np.random.default_rng(7)
            for n_live in CROSSOVER_EDGES:
                if n_live > len(offdiag):
                    break
                score = np.zeros(hits.count)
                score[rng.choice(offdiag, n_live, replace=False)] = 1.0
                d_score = ctx.to_device(score)
                row = {"live_edges": n_live}
                for name, knob in PATHS:
                    _set(knob)
                    fn = lambda: ctx.cluster_greedy(hits, "score", 0.5, nodes=S, score=d_score.ptr)  # noqa: E731
                    fn().free()
                    ts, cl = _timed(ctx, fn, args.repeats)
                    kern, _ = _kernels(ctx, fn)
                    rounds_ms = sum(kern.get(kn, [0, 0.0])[1] for kn in ("greedy_round", "greedy_promote", "greedy_tail"))
                    row[name] = {"wall": _spread(ts), "n_rounds": cl.n_rounds, "n_clusters": cl.n_clusters, "round_kernels_ms": round(rounds_ms, 4),
                                 "launches": {kn: kern[kn][0] for kn in ("greedy_round", "greedy_promote", "greedy_tail") if kn in kern}}
                    cl.free()
                _set(None)
                d_score.free()
                crossover.append(row)
        tail_edges = int(ctx._L.ks_debug_greedy_tail_edges())
        print(json.dumps({
            "what": "device_cluster_greedy", "workload": f"{n}_all_vs_all_{mol}_k{k}_s{scaled}", "nodes": n, "rows": hits.count,
            "search": _spread(t_search), "cases": cases, "crossover": crossover, "tail_edges": tail_edges,
            "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}), flush=True)


if __name__ == "__main__":
    main()
