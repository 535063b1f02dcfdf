#!/usr/bin/env python3
"""Cost of the region pass (ks_match_regions) on one MI355X, inputs resident on the device.

    python tools/regions_bench.py [--repeats 7] [--skip-200k] [--max-pairs N]

Wall time of the synchronous call (median, min, max over the repeats) for (max_gap, min_kmers) in {(0, 1), (16, 3)} on
    300 x 500 real proteins   protein k=10 scaled=1   (the BCL2 family against the first 500 uncharacterized records)
    200k all-vs-all           hp k=24 scaled=5        (BASELINE configs[4]), the hits thinned to the best 10 per query
beside the ks_match_positions call that made its input and — on the real proteins, where it is affordable — the Python loop it
replaces (wire.stitch_match_positions on the downloaded pairs), the per-kernel event times of one timed pass (ks_timing), and
the achieved bytes/s against the pass's own model and the device's measured copy rate (ks_bench_device_rates).  The model, per
pair: 8 bytes of starts read and 8 of key written, 16 per sort pass, 8 + 8 through the head kernel, 16 through the two scans,
12 read by the position kernel; per region: 24 bytes of columns written, read and written again, and 12 per order-sort pass.
A join beyond --max-pairs is reported as refused.  Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

OPTIONS = ((0, 1), (16, 3))


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


def model_bytes(n_pairs, n_regions, sort_passes, order_passes):
    """bytes the pass has to move: see the module docstring"""
    return n_pairs * (8 + 8 + 16 * sort_passes + 16 + 16 + 12) + n_regions * (3 * 24 + 12 * order_passes)


def measure(ctx, name, hits, qp, tp, repeats, max_pairs, rates, stitch=None):
    import kmerseek_amd as ks
    try:
        ctx.match_positions(qp, tp, hits, max_pairs=max_pairs).free()  # warm-up: pool blocks
    except ks.KmerseekError as e:
        print(json.dumps({"what": "device_match_regions", "workload": name, "rows": hits.count, "refused": str(e)}), flush=True)
        return
    t_mp, mp = _timed(ctx, lambda: ctx.match_positions(qp, tp, hits, max_pairs=max_pairs), repeats)
    cases = []
    for max_gap, min_kmers in OPTIONS:
        ctx.match_regions(mp, max_gap, min_kmers).free()
        ts, rg = _timed(ctx, lambda: ctx.match_regions(mp, max_gap, min_kmers), repeats)
        n_regions, n_slices = rg.n_regions, rg.n_slices
        offs = rg.to_host()[0]
        rg.free()
        ctx.timing_enable(1)
        ctx.timing_reset()
        ctx.match_regions(mp, max_gap, min_kmers).free()
        kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
        ctx.timing_enable(0)
        passes = sum(c for kn, (c, _) in kern.items() if kn in ("msd_scatter", "radix_scatter.pairs"))
        order_passes = min(passes, -(-64 // 8))  # (an LSD chain sort and the order sort share a kernel name; the model is a bound)
        b = model_bytes(mp.n_pairs, n_regions, passes, order_passes)
        kern_ms = sum(ms for _, ms in kern.values())
        per_row = offs[1:] - offs[:-1]
        cases.append({"max_gap": max_gap, "min_kmers": min_kmers, "regions": n_regions, "slices": n_slices,
                      "rows_with_more_than_one": int((per_row > 1).sum()), "most_in_a_row": int(per_row.max()) if len(per_row) else 0,
                      "wall": _spread(ts), "kernels": kern, "model_bytes": b, "kernel_ms": round(kern_ms, 4),
                      "gb_per_s": round(b / max(kern_ms, 1e-9) / 1e6, 2), "ms_at_copy_rate": round(b / (rates["copy_gb_per_s"] * 1e6), 4)})
    out = {"what": "device_match_regions", "workload": name, "rows": mp.n_rows, "pairs": mp.n_pairs, "match_positions": _spread(t_mp),
           "cases": cases, "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}
    if stitch is not None:
        out.update(stitch(mp))
    mp.free()
    print(json.dumps(out), flush=True)


def real_proteins(args):
    import kmerseek_amd as ks
    from kmerseek_amd import wire
    k, scaled, mol = 10, 1, "protein"
    q_recs = [(nm, s.upper()) for nm, s in wire.read_fasta(os.path.join(GOLDEN, "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"))]
    t_recs = [(nm, s.upper()) for nm, s in wire.read_fasta(os.path.join(GOLDEN, "uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz"))][:500]
    with ks.Context(0) as ctx:
        rates = ctx.device_rates()
        q, t = ks.pack([s for _, s in q_recs]), ks.pack([s for _, s in t_recs])
        Q, T = ctx.sketch_batch(*q, k, scaled, mol), ctx.sketch_batch(*t, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qid, tid, _, _ = hits.to_host()
        qp, tp = ctx.kmer_positions_table(*q, k, scaled, mol), ctx.kmer_positions_table(*t, k, scaled, mol)

        def stitch(mp):
            """the Python loop over every pair, and the host half of the device path, on the same input"""
            offs, qs, ts_ = mp.to_host()[:3]
            t_loop, t_rows, n_fail = [], [], 0
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                try:
                    wire.stitch_match_positions(q_recs, t_recs, qid, tid, offs, qs, ts_, k, mol)
                except AssertionError:  # the stitcher's own length assertion: a match that is not one colinear run
                    n_fail += 1
                t_loop.append(time.perf_counter() - t0)
            rg = ctx.match_regions(mp)
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                rows = wire.region_rows(q_recs, t_recs, qid, tid, rg.to_host(), mol)
                t_rows.append(time.perf_counter() - t0)
            rg.free()
            return {"stitch_match_positions_loop": dict(_spread(t_loop), assertion_tripped=bool(n_fail)),
                    "regions_download_and_region_rows": dict(_spread(t_rows), rows=len(rows))}

        measure(ctx, "bcl2_300_x_uncharacterized_500_protein_k10_s1", hits, qp, tp, args.repeats, args.max_pairs, rates, stitch)


def all_vs_all(args):
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 200_000, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    with ks.Context(0) as ctx:
        rates = ctx.device_rates()
        d_r, d_o = ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(off)
        T = ctx.sketch_batch_device(d_r.ptr, d_o.ptr, n, int(off[-1]), k, scaled, mol)
        all_hits = ctx.search(ctx.index_build(T), T)
        hits = ctx.best_hits(all_hits, 10)
        all_hits.free()
        tab = ctx.kmer_positions_table_device(d_r.ptr, d_o.ptr, n, int(off[-1]), k, scaled, mol)
        measure(ctx, "200k_all_vs_all_hp_k24_s5_best10", hits, tab, tab, args.repeats, args.max_pairs, rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--skip-200k", action="store_true")
    args = ap.parse_args()
    real_proteins(args)
    if not args.skip_200k:
        all_vs_all(args)


if __name__ == "__main__":
    main()
