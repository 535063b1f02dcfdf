#!/usr/bin/env python3
"""Cost of the gather pass (ks_hits_gather) on one MI355X, inputs resident on the device.

    python tools/gather_bench.py [--repeats 5] [--skip-200k]

Workloads: 10k queries x 10k targets, protein k=7 scaled=1 (mutated copies: a few related targets per query), and BASELINE
configs[4], 200k proteins all-vs-all, hp k=24 scaled=5 (31.6 M rows).  Per workload: wall time of the synchronous call (median,
min, max over the repeats) beside the search step of the same run — the number to set it against —, the per-kernel event times
of one timed pass (ks_timing) summed into the three phases (incidence: the scan of the intersect column and the two row kernels;
rounds: the wave and the workgroup kernel; move: the scan of the keep flags and the scatter), and the split the by-length rule
makes: segments per path, and rounds per segment (mean and max; a segment's rounds are the rows it keeps, plus the one that
finds nothing unless every row was kept).  Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GA_WAVE_MAX, GA_WAVE_BITS, GA_LIVE_BITS = 64, 8192, 65536  # ks_gather.hip
PHASES = {"incidence": ("scan", "gather_rows", "gather_rows_wave"), "rounds": ("gather_wave", "gather_wg"), "move": ("best_move",)}


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


def phases(kern):
    """the kernels of one pass by phase; the pass runs two scans over the rows under one timer name, one for the incidence and
    one for the move: each phase gets half of their time"""
    out = {}
    for phase, names in PHASES.items():
        out[phase] = sum(ms for kn, (c, ms) in kern.items() if any(kn.startswith(n) for n in names))
    scans = sum(ms for kn, (c, ms) in kern.items() if kn.startswith("scan"))
    out["incidence"] -= scans / 2
    out["move"] += scans / 2
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    os.environ.pop("KS_DEBUG_GATHER_PATH", None)
    work = [("10k_x_10k_protein_k7_s1", 10_000, 7, 1, "protein", False)]
    if not args.skip_200k:
        work.append(("200k_all_vs_all_hp_k24_s5", 200_000, 24, 5, "hp", True))
    for name, n, k, scaled, mol, all_vs_all in work:
        t_res, t_off = synth.proteome(n, stream=0)
        q_res, q_off = (t_res, t_off) if all_vs_all else synth.queries(n, t_res, t_off, stream=1000)
        with ks.Context(0) as ctx:
            pad = np.zeros(16, np.uint8)
            d_t, d_to = ctx.to_device(np.concatenate([t_res, pad])), ctx.to_device(t_off)
            d_q, d_qo = ctx.to_device(np.concatenate([q_res, pad])), ctx.to_device(q_off)
            T = ctx.sketch_batch_device(d_t.ptr, d_to.ptr, n, int(t_off[-1]), k, scaled, mol)
            Q = ctx.sketch_batch_device(d_q.ptr, d_qo.ptr, n, int(q_off[-1]), k, scaled, mol)
            ix = ctx.index_build(T)
            for _ in range(2):  # warm-up: pool blocks, row hint
                hits = ctx.search(ix, Q)
                ctx.gather(hits, Q, T).free()
                hits.free()
            t_search, hits = _timed(ctx, lambda: ctx.search(ix, Q), args.repeats)
            ts, g = _timed(ctx, lambda: ctx.gather(hits, Q, T), args.repeats)
            kept_q = g.to_host()[0].astype(np.int64)
            kept = g.count
            g.free()
            ctx.timing_enable(1)
            ctx.timing_reset()
            ctx.gather(hits, Q, T).free()
            kern = {kn: (c, ms) for kn, (c, ms) in ctx.timing().items()}
            ctx.timing_enable(0)
            # the by-length split, restated on the host
            qid = hits.to_host()[0].astype(np.int64)
            seg = np.bincount(qid, minlength=n)
            nq = np.diff(Q.to_host()[0]).astype(np.int64)
            has = seg > 0
            wave = has & (seg <= GA_WAVE_MAX) & (nq <= GA_WAVE_BITS)
            rounds = np.bincount(kept_q, minlength=n)
            rounds = (rounds + (rounds < seg))[has]
            print(json.dumps({
                "what": "device_gather", "workload": name, "rows": hits.count, "shared_hashes": hits.n_pair_instances, "kept": kept,
                "search": _spread(t_search), "gather": _spread(ts),
                "kernels": {kn: [c, round(ms, 4)] for kn, (c, ms) in kern.items()}, "phase_ms": phases(kern),
                "segments": {"wave": int(wave.sum()), "workgroup_lds": int((has & ~wave & (nq <= GA_LIVE_BITS)).sum()),
                             "workgroup_streamed": int((has & (nq > GA_LIVE_BITS)).sum()),
                             "rows_median": int(np.median(seg[has])) if has.any() else 0, "rows_max": int(seg.max())},
                "rounds_per_segment": {"mean": round(float(rounds.mean()), 2) if len(rounds) else 0.0,
                                       "max": int(rounds.max()) if len(rounds) else 0}}), flush=True)


if __name__ == "__main__":
    main()
