#!/usr/bin/env python3
"""Cost of the frame fold (ks_frames_fold_device) on one MI355X, beside the chain over it and the whole translated pipeline.

    python tools/ffold_bench.py [--proteins 20000] [--targets 20000] [--repeats 7]

Workload: the synthetic DNA of tools/translate_bench.py (synth.proteome reverse-translated, every second record reverse-
complemented: 20,000 records, 18.1 M bases) searched at protein k=7 scaled=1 against the first --targets of the proteins it was made
from.  The pipeline is the one of wire.search_translated_device, from arrays: translate6, sketch of the frames, search, position
tables, match_positions, match_regions, score_regions_device (extended), cull and take, fold_frames, chain_frames.  Reported: wall
time of the fold (median, min, max over the repeats) and the event times of its kernels in one timed pass (ks_timing); the same for
chain_frames on the same regions, and the ratio of the two; the wall time of every stage of one pipeline pass and their sum.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from translate_bench import _spread, _timed, reverse_translate  # noqa: E402

K, SCALED, MOL = 7, 1, "protein"


def kernels(ctx, fn):
    ctx.timing_enable(1)
    ctx.timing_reset()
    out = fn()
    kern = {name: {"launches": c, "ms": round(ms, 4)} for name, (c, ms) in sorted(ctx.timing().items())}
    ctx.timing_enable(0)
    out.free()
    return kern, round(sum(v["ms"] for v in kern.values()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=20000)
    ap.add_argument("--targets", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth

    p_res, p_off = synth.proteome(args.proteins, stream=31)
    nt, nt_off = reverse_translate(np, p_res, p_off)
    n_t = min(args.targets, args.proteins)
    t_off = p_off[:n_t + 1].copy()
    t_res = p_res[:int(t_off[-1])].copy()
    n, n6 = len(nt_off) - 1, 6 * (len(nt_off) - 1)
    ctx = ks.Context(0)
    stages, obj = {}, {}

    def stage(name, fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        obj[name] = fn()
        ctx.synchronize()
        stages[name] = round((time.perf_counter() - t0) * 1e3, 4)
        return obj[name]

    def pipeline():
        frames, foff, n_res = stage("translate6", lambda: ctx.translate6(nt, nt_off))
        Q = stage("sketch_frames", lambda: ctx.sketch_batch_device(frames.ptr, foff.ptr, n6, n_res, K, SCALED, MOL))
        T = stage("sketch_targets", lambda: ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
        ix = stage("index_build", lambda: ctx.index_build(T))
        hits = stage("search", lambda: ctx.search(ix, Q))
        qp = stage("positions_frames", lambda: ctx.kmer_positions_table_device(frames.ptr, foff.ptr, n6, n_res, K, SCALED, MOL))
        tp = stage("positions_targets", lambda: ctx.kmer_positions_table(t_res, t_off, K, SCALED, MOL))
        mp = stage("match_positions", lambda: ctx.match_positions(qp, tp, hits))
        rg = stage("match_regions", lambda: ctx.match_regions(mp))
        d_t, d_to = stage("upload_targets", lambda: (ctx.to_device(t_res), ctx.to_device(t_off)))
        sc = stage("score_regions", lambda: ctx.score_regions_device(rg, hits, frames.ptr, foff.ptr, n6, n_res, d_t.ptr, d_to.ptr, n_t, len(t_res),
                                                                     extend=True, x_drop=20))
        cu = stage("cull", lambda: ctx.cull_regions(sc))
        kept = stage("take", lambda: cu.take(sc))
        fold = stage("fold_frames", lambda: ctx.fold_frames(hits, kept, nt_off))
        stage("chain_frames", lambda: ctx.chain_frames(fold))
        return hits, kept, fold

    pipeline()  # (the first pass sizes the pool: not counted)
    for o in obj.values():
        for x in (o if isinstance(o, tuple) else (o,)):
            if hasattr(x, "free"):
                x.free()
    hits, kept, fold = pipeline()
    counts = {"records": n, "bases": int(len(nt)), "targets": n_t, "frame_hit_rows": hits.count, "regions": kept.n_regions, "folded_rows": fold.n_rows,
              "chained": obj["chain_frames"].n_chained}
    t_fold, _ = _timed(ctx, lambda: ctx.fold_frames(hits, kept, nt_off), args.repeats)
    t_chain, _ = _timed(ctx, lambda: ctx.chain_frames(fold), args.repeats)
    k_fold, ms_fold = kernels(ctx, lambda: ctx.fold_frames(hits, kept, nt_off))
    k_chain, ms_chain = kernels(ctx, lambda: ctx.chain_frames(fold))
    row = {"what": "frame fold", "ksize": K, "scaled": SCALED, "moltype": MOL, **counts, "fold": _spread(t_fold), "fold_kernels_ms": ms_fold,
           "chain": _spread(t_chain), "chain_kernels_ms": ms_chain,
           "fold_over_chain_wall": round(_spread(t_fold)["median_ms"] / _spread(t_chain)["median_ms"], 3),
           "fold_over_chain_kernels": round(ms_fold / ms_chain, 3) if ms_chain else None,
           "pipeline_ms": round(sum(stages.values()), 3), "stages_ms": stages, "kernels": {"fold": k_fold, "chain": k_chain}, "library": ks.SO_PATH}
    print(json.dumps(row))


if __name__ == "__main__":
    main()
