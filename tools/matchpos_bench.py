#!/usr/bin/env python3
"""Cost of ks_match_positions (where each hit's shared k-mers lie) on one MI355X, inputs resident on the device.

    python tools/matchpos_bench.py [--repeats 7] [--skip-100k] [--skip-host]

device : wall time of the synchronous call (median, min, max over the repeats) for
           10k x 10k   protein k=7  scaled=1
           100k x 100k dayhoff k=16 scaled=5   (with the search and the two k-mer position calls that feed it timed beside it)
         plus the per-kernel event times of one timed pass (ks_timing), and the bytes the expand + sort + rows kernels have to
         move (8 n_pairs written by expand, 16 n_pairs per sort pass, 8 n_pairs + 24 n_rows out) against the device's measured
         copy rate (ks_bench_device_rates): how far from the memory roofline the new kernels are.
host   : the path it replaces — wire.stitch_hits' dict join — on the real-protein case of the tests (300 BCL2-family records
         against the first 500 uncharacterized ones, protein k=10 scaled=1), beside the device call + stitch_match_positions.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


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


def device(args):
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    work = [("10k_protein_k7_s1", 10_000, 7, 1, "protein")]
    if not args.skip_100k:
        work.append(("100k_dayhoff_k16_s5", 100_000, 16, 5, "dayhoff"))
    for name, n, k, scaled, mol in work:
        t_res, t_off = synth.proteome(n, stream=0)
        q_res, q_off = synth.queries(n, t_res, t_off, stream=1000)
        with ks.Context(0) as ctx:
            rates = ctx.device_rates()
            pad = np.zeros(16, np.uint8)
            d_t, d_to = ctx.to_device(np.concatenate([t_res, pad])), ctx.to_device(t_off)
            d_q, d_qo = ctx.to_device(np.concatenate([q_res, pad])), ctx.to_device(q_off)
            T = ctx.sketch_batch_device(d_t.ptr, d_to.ptr, n, int(t_off[-1]), k, scaled, mol)
            ix = ctx.index_build(T)
            Q = ctx.sketch_batch_device(d_q.ptr, d_qo.ptr, n, int(q_off[-1]), k, scaled, mol)
            pos_q = lambda: ctx.kmer_positions_table_device(d_q.ptr, d_qo.ptr, n, int(q_off[-1]), k, scaled, mol)
            pos_t = lambda: ctx.kmer_positions_table_device(d_t.ptr, d_to.ptr, n, int(t_off[-1]), k, scaled, mol)
            for _ in range(2):  # warm-up: pool blocks, row hint
                hits, qp, tp = ctx.search(ix, Q), pos_q(), pos_t()
                ctx.match_positions(qp, tp, hits).free()
                for o in (hits, qp, tp):
                    o.free()
            t_search, hits = _timed(ctx, lambda: ctx.search(ix, Q), args.repeats)
            t_qp, qp = _timed(ctx, pos_q, args.repeats)
            t_tp, tp = _timed(ctx, pos_t, args.repeats)
            t_mp, mp = _timed(ctx, lambda: ctx.match_positions(qp, tp, hits), args.repeats)
            n_rows, n_pairs, n_slices = mp.n_rows, mp.n_pairs, mp.n_slices
            mp.free()
            ctx.timing_enable(1)
            ctx.timing_reset()
            ctx.match_positions(qp, tp, hits).free()
            kern = {kn: [c, round(ms, 4)] for kn, (c, ms) in ctx.timing().items()}
            ctx.timing_enable(0)
            sort_passes = sum(c for kn, (c, _) in kern.items() if kn in ("msd_scatter", "radix_scatter.pairs"))
            hot_ms = sum(ms for kn, (_, ms) in kern.items()
                         if kn in ("matchpos_expand", "matchpos_rows") or kn.startswith(("msd_", "radix_hist.pairs", "radix_scatter.pairs")))
            hot_bytes = 8 * n_pairs + 16 * n_pairs * sort_passes + 8 * n_pairs + 24 * n_rows
            print(json.dumps({
                "what": "device_match_positions", "workload": name, "q_windows": qp.count, "t_windows": tp.count, "rows": n_rows,
                "pairs": n_pairs, "slices": n_slices, "match_positions": _spread(t_mp), "search": _spread(t_search),
                "kmer_positions_queries": _spread(t_qp), "kmer_positions_targets": _spread(t_tp), "kernels": kern,
                "expand_sort_rows": {"bytes": hot_bytes, "sort_passes": sort_passes, "kernel_ms": round(hot_ms, 4),
                                     "gb_per_s": round(hot_bytes / max(hot_ms, 1e-9) / 1e6, 2),
                                     "ms_at_copy_rate": round(hot_bytes / (rates["copy_gb_per_s"] * 1e6), 4)},
                "copy_gb_per_s": round(rates["copy_gb_per_s"], 1)}), flush=True)


def host(args):
    import kmerseek_amd as ks
    from kmerseek_amd import wire
    k, scaled, mol = 10, 1, "protein"
    q_recs = [(nm, s.upper()) for nm, s in wire.read_fasta(os.path.join(GOLDEN, "uniprotkb_BCL2_AND_model_organism_9606_2025_02_06.fasta.gz"))]
    t_recs = [(nm, s.upper()) for nm, s in wire.read_fasta(os.path.join(GOLDEN, "uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz"))][:500]
    with ks.Context(0) as ctx:
        q, t = ks.pack([s for _, s in q_recs]), ks.pack([s for _, s in t_recs])
        Q, T = ctx.sketch_batch(*q, k, scaled, mol), ctx.sketch_batch(*t, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qid, tid, _, _ = hits.to_host()
        t0 = time.perf_counter()
        qk, tk = wire.extract_kmers(ctx, q_recs, k, scaled, mol), wire.extract_kmers(ctx, t_recs, k, scaled, mol)
        t_tables = time.perf_counter() - t0
        pairs = [(q_recs[a][0], t_recs[b][0]) for a, b in zip(qid.tolist(), tid.tolist())]
        ts_host = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            rows_host = wire.stitch_hits(qk, tk, pairs)
            ts_host.append(time.perf_counter() - t0)
        ts_dev, ts_stitch = [], []
        for _ in range(args.repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            qp, tp = ctx.kmer_positions_table(*q, k, scaled, mol), ctx.kmer_positions_table(*t, k, scaled, mol)
            mp = ctx.match_positions(qp, tp, hits)
            offs, qs, tst = mp.to_host()[:3]
            ts_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            rows_dev = wire.stitch_match_positions(q_recs, t_recs, qid, tid, offs, qs, tst, k, mol)
            ts_stitch.append(time.perf_counter() - t0)
            for o in (mp, qp, tp):
                o.free()
        print(json.dumps({"what": "host_vs_device_join", "workload": "bcl2_300_x_uncharacterized_500_protein_k10_s1",
                          "rows": int(len(qid)), "pairs": int(offs[-1]), "q_windows": len(qk), "t_windows": len(tk),
                          "host_kmer_tables_ms": round(t_tables * 1e3, 2), "host_stitch_hits": _spread(ts_host),
                          "device_tables_join_download": _spread(ts_dev), "stitch_match_positions": _spread(ts_stitch),
                          "stitched_rows": [len(rows_host), len(rows_dev)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--skip-100k", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if not a.skip_device:
        device(a)
    if not a.skip_host:
        host(a)


if __name__ == "__main__":
    main()
