#!/usr/bin/env python3
"""Cost of the best-hits pass (ks_hits_best) on one MI355X, inputs resident on the device.

    python tools/best_bench.py [--repeats 7] [--skip-200k]

Wall time of the synchronous call (median, min, max over the repeats) for k in {1, 10, 100} and rank_by intersect and jaccard, on
    10k x 10k   protein k=7 scaled=1           (BASELINE configs[1])
    200k all-vs-all  hp k=24 scaled=5          (BASELINE configs[4])
beside the search step of the same run, the per-kernel event times of one timed pass (ks_timing), and the achieved bytes/s
against the pass's own model — 12 bytes read per input row (qid, tid, intersect), the size lookups (jaccard: 16 bytes of
offsets per row and side; they hit in cache, the model counts them once per row), and per kept row the columns written and
read for it (20 bytes of row columns in and out, 8 bytes of rank and src_row) — and against the device's measured copy rate
(ks_bench_device_rates).  What the pass saves: ks_hits_significance on all rows beside significance on the best-10 list.
Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 10, 100)
KEYS = ("intersect", "jaccard")


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


def model_bytes(rows, kept, key):
    """bytes the pass has to move: see the module docstring"""
    return rows * (12 + (32 if key == "jaccard" else 0)) + kept * (20 + 20 + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    work = [("10k_x_10k_protein_k7_s1", 10_000, 7, 1, "protein", False)]
    if not args.skip_200k:
        work.append(("200k_all_vs_all_hp_k24_s5", 200_000, 24, 5, "hp", True))
    for name, n, k, scaled, mol, all_vs_all in work:
        t_res, t_off = synth.proteome(n, stream=0)
        q_res, q_off = (t_res, t_off) if all_vs_all else synth.queries(n, t_res, t_off, stream=1000)
        with ks.Context(0) as ctx:
            rates = ctx.device_rates()
            pad = np.zeros(16, np.uint8)
            d_t, d_to = ctx.to_device(np.concatenate([t_res, pad])), ctx.to_device(t_off)
            d_q, d_qo = ctx.to_device(np.concatenate([q_res, pad])), ctx.to_device(q_off)
            T = ctx.sketch_batch_device(d_t.ptr, d_to.ptr, n, int(t_off[-1]), k, scaled, mol)
            Q = ctx.sketch_batch_device(d_q.ptr, d_qo.ptr, n, int(q_off[-1]), k, scaled, mol)
            ix = ctx.index_build(T)
            for _ in range(2):  # warm-up: pool blocks, row hint
                hits = ctx.search(ix, Q)
                ctx.best_hits(hits, 10, "jaccard", Q, T).free()
                hits.free()
            t_search, hits = _timed(ctx, lambda: ctx.search(ix, Q), args.repeats)
            qid = hits.to_host()[0]
            seg = np.bincount(qid.astype(np.int64)) if len(qid) else np.zeros(1, np.int64)
            seg = seg[seg > 0]
            cases = []
            for key in KEYS:
                for kk in KS:
                    ts, best = _timed(ctx, lambda: ctx.best_hits(hits, kk, key, Q, T), args.repeats)
                    kept = best.count
                    best.free()
                    ctx.timing_enable(1)
                    ctx.timing_reset()
                    ctx.best_hits(hits, kk, key, Q, T).free()
                    kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
                    ctx.timing_enable(0)
                    b = model_bytes(hits.count, kept, key)
                    kern_ms = sum(ms for _, ms in kern.values())
                    cases.append({"rank_by": key, "k": kk, "kept": kept, "wall": _spread(ts), "kernels": kern,
                                  "model_bytes": b, "kernel_ms": round(kern_ms, 4),
                                  "gb_per_s": round(b / max(kern_ms, 1e-9) / 1e6, 2),
                                  "ms_at_copy_rate": round(b / (rates["copy_gb_per_s"] * 1e6), 4)})
            # what the pass saves: significance on every row beside significance on the best 10
            cq, ct = Q.corpus(), T.corpus()
            best10 = ctx.best_hits(hits, 10, "jaccard", Q, T)
            ctx.significance(Q, T, best10, cq, ct).free()
            t_all, s = _timed(ctx, lambda: ctx.significance(Q, T, hits, cq, ct), args.repeats)
            s.free()
            t_b10, s = _timed(ctx, lambda: ctx.significance(Q, T, best10, cq, ct), args.repeats)
            s.free()
            print(json.dumps({
                "what": "device_best_hits", "workload": name, "rows": hits.count, "queries_with_rows": int(len(seg)),
                "segment_rows": {"median": int(np.median(seg)), "max": int(seg.max()), "le_64": int((seg <= 64).sum())},
                "search": _spread(t_search), "cases": cases,
                "significance_all_rows": _spread(t_all), "significance_best10": dict(_spread(t_b10), rows=best10.count),
                "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}), flush=True)


if __name__ == "__main__":
    main()
