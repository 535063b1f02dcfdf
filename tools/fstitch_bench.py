#!/usr/bin/env python3
"""Cost of the frame stitch (ks_frames_stitch) on one MI355X, beside the fold, the chain and the traceback of the same alignments.

    python tools/fstitch_bench.py [--proteins 20000] [--targets 20000] [--repeats 7] [--indel-every 2]

Workload: that of tools/ffold_bench.py — the synthetic DNA of tools/translate_bench.py (20,000 records, 18.1 M bases) searched at
protein k=7 scaled=1 against the proteins it was made from — aligned with gaps (band 16, 11 / 1, x_drop 30), culled and traced.
Two variants: "clean", the records as they are (almost every chain is one alignment: no links), and "indels", where every
--indel-every-th record has one base inserted or deleted in its middle third, so that chains of two frames and their links exist.
Per variant: the wall time of stitch_frames, fold_frames, chain_frames and trace_regions on the same alignments, the four calls
interleaved in one process (median, min, max over the repeats), and the event times of the stitch's kernels in one timed pass
(ks_timing).  Prints one JSON line per variant."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from translate_bench import _spread, reverse_translate  # noqa: E402

K, SCALED, MOL = 7, 1, "protein"
ALIGN = dict(band=16, gap_open=11, gap_extend=1, x_drop=30)
CHAIN = dict(max_overlap=15)


def plant_indels(np, nt, nt_off, every, seed=11):
    """every `every`-th record gets one base inserted or deleted (alternating) somewhere in its middle third"""
    rng = np.random.default_rng(seed)
    parts, offs = [], [0]
    for s in range(len(nt_off) - 1):
        rec = nt[int(nt_off[s]):int(nt_off[s + 1])]
        if s % every == 0 and len(rec) >= 90:
            at = int(rng.integers(len(rec) // 3, 2 * len(rec) // 3))
            rec = np.concatenate([rec[:at], rec[at:at + 1], rec[at:]]) if (s // every) % 2 == 0 else np.concatenate([rec[:at], rec[at + 1:]])
        parts.append(rec)
        offs.append(offs[-1] + len(rec))
    return np.concatenate(parts), np.array(offs, np.uint64)


def run(ctx, np, name, nt, nt_off, t_res, t_off, n_t, repeats):
    n6 = 6 * (len(nt_off) - 1)
    made = []

    def keep(o):
        made.append(o)
        return o
    frames, foff, n_res = ctx.translate6(nt, nt_off)
    keep(frames); keep(foff)
    f = (frames.ptr, foff.ptr, n6, n_res)
    Q, T = keep(ctx.sketch_batch_device(*f, K, SCALED, MOL)), keep(ctx.sketch_batch(t_res, t_off, K, SCALED, MOL))
    ix = keep(ctx.index_build(T))
    hits = keep(ctx.search(ix, Q))
    qp, tp = keep(ctx.kmer_positions_table_device(*f, K, SCALED, MOL)), keep(ctx.kmer_positions_table(t_res, t_off, K, SCALED, MOL))
    mp = keep(ctx.match_positions(qp, tp, hits))
    rg = keep(ctx.match_regions(mp))
    d_t, d_to = keep(ctx.to_device(t_res)), keep(ctx.to_device(t_off))
    b = (*f, d_t.ptr, d_to.ptr, n_t, len(t_res))
    al = keep(ctx.align_regions_device(rg, hits, *b, **ALIGN))
    cu = keep(ctx.cull_regions(al))
    kept, kept_rg = keep(cu.take(al)), keep(cu.take(rg))
    fold = keep(ctx.fold_frames(hits, kept, nt_off))
    chain = keep(ctx.chain_frames(fold, **CHAIN))
    cg = keep(ctx.trace_regions_device(kept_rg, hits, *b, kept))
    calls = {"stitch_frames": lambda: ctx.stitch_frames_device(fold, chain, kept, cg, *b),
             "fold_frames": lambda: ctx.fold_frames(hits, kept, nt_off),
             "chain_frames": lambda: ctx.chain_frames(fold, **CHAIN),
             "trace_regions": lambda: ctx.trace_regions_device(kept_rg, hits, *b, kept)}
    times = {k: [] for k in calls}
    for i in range(repeats + 1):  # (the first round sizes the pool: not counted)
        for k, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            out.free()
            if i:
                times[k].append(dt)
    ctx.timing_enable(1)
    ctx.timing_reset()
    st = calls["stitch_frames"]()
    kern = {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in sorted(ctx.timing().items())}
    ctx.timing_enable(0)
    got = st.to_host()
    row = {"what": "frame stitch", "variant": name, "records": len(nt_off) - 1, "bases": int(len(nt)), "targets": n_t, "frame_hit_rows": hits.count,
           "alignments": kept.n_regions, "folded_rows": fold.n_rows, "chained": chain.n_chained, "ops": st.n_ops,
           "frameshifts": int(got[17].sum()), "filled": int(got[14].sum()), "open": int(got[15].sum()), "trimmed_columns": int(got[16].sum()),
           "scratch_bytes": st.scratch_bytes, "slices": st.n_slices, **{k: _spread(v) for k, v in times.items()},
           "stitch_kernels_ms": round(sum(v["ms"] for v in kern.values()), 4), "kernels": kern}
    st.free()
    for o in reversed(made):
        o.free()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=20000)
    ap.add_argument("--targets", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--indel-every", type=int, default=2)
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
    ctx = ks.Context(0)
    run(ctx, np, "clean", nt, nt_off, t_res, t_off, n_t, args.repeats)
    run(ctx, np, "indels", *plant_indels(np, nt, nt_off, args.indel_every), t_res, t_off, n_t, args.repeats)
    ctx.close()


if __name__ == "__main__":
    main()
