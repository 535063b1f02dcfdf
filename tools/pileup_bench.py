#!/usr/bin/env python3
"""Cost of the pileup (ks_pileup_device) on one MI355X, inputs resident on the device, beside the re-scoring kernel of the stitch
that made the alignments.

    python tools/pileup_bench.py [--repeats 7] [--skip-10k] [--skip-200k] [--skip-translated] [--proteins 20000]

On the stitched alignments (target side) of three inputs
    10k x 10k            protein k=7 scaled=1    as tools/rstitch_bench.py makes them (synthetic proteome, related queries)
    200k all-vs-all      hp k=24 scaled=5        the hits thinned to the best 10 per query
    translated           protein k=7 scaled=1    the 20,000 records of tools/fstitch_bench.py, "indels" variant (depth only: frame
                                                 alignments have no profile)
two variants, depth only and depth + profile, in one process, the calls interleaved round by round:
    wall      the synchronous call, median [min - max] of --repeats
    kernels   event time per kernel (ks_timing), the median over --repeats timed calls
    yardstick the rstitch_rescore / fstitch_rescore kernel of the stitch of the SAME alignments, timed the same way in the same
              rounds: it walks the same columns once and reads both residues of every pair
    ratio     pileup kernels / that kernel
Prints one JSON line per workload."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rstitch_bench as RB  # noqa: E402


def measure(ctx, name, stitched, t_start_col, hits, stitch, rescore, q_batch, t_batch, repeats, profile=True):
    """stitched: a HitAlignments / FrameAlignments; stitch: the call that makes it again (the yardstick's kernel is read from its
    timing); q_batch / t_batch: (d_res, d_off, n_seqs, n_res), q_batch None where there is no profile"""
    import numpy as np
    p = stitched.device_ptrs()
    entries = dict(d_row_offsets=None, d_op_offsets=p[0], d_ops=p[1], n_rows=stitched.n_rows, n_entries=stitched.n_rows, n_ops=stitched.n_ops,
                   d_start=p[t_start_col], d_row_mask=None, hits=hits, d_offsets=t_batch[1], n_seqs=t_batch[2], n_res=t_batch[3], side="target")
    calls = {"depth": lambda: ctx.pileup_device(d_other_start=None, **entries), "stitch": stitch}
    if profile:
        calls["depth_profile"] = lambda: ctx.pileup_device(d_other_start=p[2], profile=True, d_other_res=q_batch[0], d_other_off=q_batch[1],
                                                           n_other=q_batch[2], n_other_res=q_batch[3], **entries)
    pu = calls["depth_profile" if profile else "depth"]()
    h = pu.to_host()
    counts = {"rows": stitched.n_rows, "ops": stitched.n_ops, "sequences": pu.n_seqs, "residues": pu.n_residues, "pair_columns": int(h[6].sum()),
              "covered": int(h[4].sum()), "max_depth": int(h[5].max()) if len(h[5]) else 0,
              "sequences_with_an_alignment": int((h[3] > 0).sum()), "profile_bytes": 4 * pu.n_profile}
    if profile:
        assert np.array_equal(h[1].reshape(-1, 28).sum(axis=1, dtype=np.uint64), h[0])
    pu.free()
    del h
    cases = RB._interleaved(ctx, calls, repeats)
    yard = cases["stitch"]["kernel_median_ms_by_name"][rescore]
    out = {"what": "device_pileup", "workload": name, "side": "target", "counts": counts,
           **{k: v for k, v in cases.items() if k != "stitch"}, rescore + "_ms": yard}
    for k in cases:
        if k != "stitch":
            out[k + "_kernels_over_rescore"] = round(cases[k]["kernel"]["median_ms"] / max(yard, 1e-9), 2)
    print(json.dumps(out), flush=True)


def protein_workload(ctx, name, hits, qp, tp, qb, tb, args):
    mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
    rg_all = ctx.match_regions(mp)
    al_all = ctx.align_regions_device(rg_all, hits, *qb, *tb)
    cu = ctx.cull_regions(al_all)
    rg, al = cu.take(rg_all), cu.take(al_all)
    for o in (cu, al_all, rg_all, mp):
        o.free()
    ch = ctx.chain_regions(al, max_overlap=5, skew_cost=1)
    cg = ctx.trace_regions_device(rg, hits, *qb, *tb, al)
    stitch = lambda: ctx.stitch_chains_device(ch, al, cg, hits, *qb, *tb)  # noqa: E731
    st = stitch()
    measure(ctx, name, st, 4, hits, stitch, "rstitch_rescore", qb, tb, args.repeats)
    for o in (st, cg, ch, al, rg):
        o.free()


def ten_k(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n = 10_000
    t_res, t_off = synth.proteome(n, stream=0)
    q_res, q_off = synth.queries(n, t_res, t_off, stream=1)
    with ks.Context(0) as ctx:
        dq, dt = RB._device_batch(ctx, q_res, q_off), RB._device_batch(ctx, t_res, t_off)
        qb, tb = (dq[0].ptr, dq[1].ptr, n, int(q_off[-1])), (dt[0].ptr, dt[1].ptr, n, int(t_off[-1]))
        T, Q = ctx.sketch_batch_device(*tb, 7, 1, "protein"), ctx.sketch_batch_device(*qb, 7, 1, "protein")
        hits = ctx.search(ctx.index_build(T), Q)
        qp, tp = ctx.kmer_positions_table_device(*qb, 7, 1, "protein"), ctx.kmer_positions_table_device(*tb, 7, 1, "protein")
        protein_workload(ctx, "10k_x_10k_protein_k7_s1", hits, qp, tp, qb, tb, args)


def all_vs_all(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    n, k, scaled, mol = 200_000, 24, 5, "hp"
    res, off = synth.proteome(n, stream=0)
    with ks.Context(0) as ctx:
        d = RB._device_batch(ctx, res, off)
        b = (d[0].ptr, d[1].ptr, n, int(off[-1]))
        T = ctx.sketch_batch_device(*b, k, scaled, mol)
        all_hits = ctx.search(ctx.index_build(T), T)
        hits = ctx.best_hits(all_hits, 10)
        all_hits.free()
        tab = ctx.kmer_positions_table_device(*b, k, scaled, mol)
        protein_workload(ctx, "200k_all_vs_all_hp_k24_s5_best10", hits, tab, tab, b, b, args)


def translated(args):
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    import fstitch_bench as FB
    from translate_bench import reverse_translate
    p_res, p_off = synth.proteome(args.proteins, stream=31)
    nt, nt_off = FB.plant_indels(np, *reverse_translate(np, p_res, p_off), 2)
    n_t, n6 = args.proteins, 6 * args.proteins
    with ks.Context(0) as ctx:
        frames, foff, n_res = ctx.translate6(nt, nt_off)
        f = (frames.ptr, foff.ptr, n6, n_res)
        Q, T = ctx.sketch_batch_device(*f, FB.K, FB.SCALED, FB.MOL), ctx.sketch_batch(p_res, p_off, FB.K, FB.SCALED, FB.MOL)
        hits = ctx.search(ctx.index_build(T), Q)
        qp, tp = ctx.kmer_positions_table_device(*f, FB.K, FB.SCALED, FB.MOL), ctx.kmer_positions_table(p_res, p_off, FB.K, FB.SCALED, FB.MOL)
        rg = ctx.match_regions(ctx.match_positions(qp, tp, hits))
        d_t, d_to = ctx.to_device(p_res), ctx.to_device(p_off)
        tb = (d_t.ptr, d_to.ptr, n_t, len(p_res))
        al = ctx.align_regions_device(rg, hits, *f, *tb, **FB.ALIGN)
        cu = ctx.cull_regions(al)
        kept, kept_rg = cu.take(al), cu.take(rg)
        fold = ctx.fold_frames(hits, kept, nt_off)
        chain = ctx.chain_frames(fold, **FB.CHAIN)
        cg = ctx.trace_regions_device(kept_rg, hits, *f, *tb, kept)
        stitch = lambda: ctx.stitch_frames_device(fold, chain, kept, cg, *f, *tb)  # noqa: E731
        st = stitch()
        measure(ctx, f"translated_{args.proteins}_records_indels", st, 5, fold.hits, stitch, "fstitch_rescore", None, tb, args.repeats, profile=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    ap.add_argument("--proteins", type=int, default=20000)
    ap.add_argument("--skip-10k", action="store_true")
    ap.add_argument("--skip-200k", action="store_true")
    ap.add_argument("--skip-translated", action="store_true")
    args = ap.parse_args()
    if not args.skip_10k:
        ten_k(args)
    if not args.skip_200k:
        all_vs_all(args)
    if not args.skip_translated:
        translated(args)


if __name__ == "__main__":
    main()
