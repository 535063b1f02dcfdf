#!/usr/bin/env python3
"""Cost of the significance columns (ks_corpus_build + ks_hits_significance) on one MI355X, inputs resident on the device.

    python tools/signif_bench.py [--repeats 7] [--skip-200k]

Wall time of the synchronous calls (median, min, max over the repeats), beside the search step of the same run, for
    10k x 10k   protein k=7 scaled=1           (BASELINE configs[1])
    200k all-vs-all  hp k=24 scaled=5          (BASELINE configs[4])
plus the per-kernel event times of one timed pass (ks_timing: corpus build, weight pass, row pass) and the row pass's achieved
bytes/s against its own model — per hit row both runs' hashes (8 bytes each) plus the query run's two weight columns (16 bytes
per query hash) — and against the device's measured copy rate (ks_bench_device_rates).  Prints one JSON line per workload."""
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
                hits, cq, ct = ctx.search(ix, Q), Q.corpus(), T.corpus()
                ctx.significance(Q, T, hits, cq, ct).free()
                for o in (hits, cq, ct):
                    o.free()
            t_search, hits = _timed(ctx, lambda: ctx.search(ix, Q), args.repeats)
            t_cq, cq = _timed(ctx, Q.corpus, args.repeats)
            t_ct, ct = _timed(ctx, T.corpus, args.repeats)
            t_sig, sig = _timed(ctx, lambda: ctx.significance(Q, T, hits, cq, ct), args.repeats)
            sig.free()
            ctx.timing_enable(1)
            ctx.timing_reset()
            ctx.significance(Q, T, hits, cq, ct).free()
            kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
            ctx.timing_enable(0)
            # the row pass's bytes by its own model: per row 8 (|q| + |t|) + 16 |q|
            qid, tid, _, _ = hits.to_host()
            q_len = np.diff(Q.to_host()[0]).astype(np.int64)
            t_len = np.diff(T.to_host()[0]).astype(np.int64)
            row_bytes = int((24 * q_len[qid] + 8 * t_len[tid]).sum())
            row_ms = sum(ms for kn, (_, ms) in kern.items() if kn in ("signif_rows", "signif_rows_wave"))
            print(json.dumps({
                "what": "device_significance", "workload": name, "q_hashes": Q.n_hashes, "t_hashes": T.n_hashes, "rows": hits.count,
                "q_corpus_hashes": cq.n_hashes, "t_corpus_hashes": ct.n_hashes, "search": _spread(t_search),
                "corpus_build_queries": _spread(t_cq), "corpus_build_targets": _spread(t_ct), "significance": _spread(t_sig),
                "kernels": kern,
                "row_pass": {"model_bytes": row_bytes, "kernel_ms": round(row_ms, 4),
                             "gb_per_s": round(row_bytes / max(row_ms, 1e-9) / 1e6, 2),
                             "ms_at_copy_rate": round(row_bytes / (rates["copy_gb_per_s"] * 1e6), 4)},
                "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}), flush=True)


if __name__ == "__main__":
    main()
