#!/usr/bin/env python3
"""Cost of the sequence-weighting passes on one MI355X, inputs resident on the device.

    python tools/pweights_bench.py [--repeats 7] [--beta 10]

On the 10k x 10k workload of tools/profile_bench.py (protein k=7 scaled=1, synthetic proteome, queries related to it; +1 / -1
matrix): the regions are aligned, culled and traced, and then, each timed as the wall time of the synchronous call and as the
event time of its kernels (ks_timing), median [min - max], on the query side:
    pileup            ks_cigars_pileup with KS_PILEUP_PROFILE            (the unweighted sibling of the next two)
    weights           ks_cigars_pileup_weights with KS_PWEIGHTS_INCLUDE_QUERY on that pileup's counts
    pileup_weighted   ks_cigars_pileup_weighted with KS_PILEUP_PROFILE under those weights
    build             ks_profile_build_pileup                           (the unweighted sibling of the next)
    build_weighted    ks_profile_build_weighted_pileup on the weighted pileup
ratio_*: weighted over unweighted, wall and kernel.  bytes: what each pass moves at the least — the weighted pileup clears and
the weighted build reads 224 bytes of wcounts a residue beside the 112 of counts.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--beta", type=float, default=10.0)
    ap.add_argument("--max-pairs", type=int, default=400_000_000)
    args = ap.parse_args()
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import _lib, synth
    from profile_bench import _measure
    n, k, scaled, mol = 10_000, 7, 1, "protein"
    t_res, t_off = synth.proteome(n, stream=0)
    q_res, q_off = synth.queries(n, t_res, t_off, stream=1)
    opts = {"band": 16, "gap_open": 11, "gap_extend": 1, "x_drop": 30}
    with ks.Context(0) as ctx:
        pad = np.zeros(16, np.uint8)
        dq, dqo = ctx.to_device(np.concatenate([q_res, pad])), ctx.to_device(q_off)
        dt, dto = ctx.to_device(np.concatenate([t_res, pad])), ctx.to_device(t_off)
        qb, tb = (dq.ptr, dqo.ptr, n, int(q_off[-1])), (dt.ptr, dto.ptr, n, int(t_off[-1]))
        T, Q = ctx.sketch_batch_device(*tb, k, scaled, mol), ctx.sketch_batch_device(*qb, k, scaled, mol)
        hits = ctx.search(ctx.index_build(T), Q)
        qp, tp = ctx.kmer_positions_table_device(*qb, k, scaled, mol), ctx.kmer_positions_table_device(*tb, k, scaled, mol)
        mp = ctx.match_positions(qp, tp, hits, max_pairs=args.max_pairs)
        rg_all = ctx.match_regions(mp)
        al_all = ctx.align_regions_device(rg_all, hits, *qb, *tb, **opts)
        cu = ctx.cull_regions(al_all)
        rg, al = cu.take(rg_all), cu.take(al_all)
        cg = ctx.trace_regions_device(rg, hits, *qb, *tb, al)
        L, vp = ctx._L, C.c_void_p
        po = _lib.ks_pileup_opts(_lib.KS_PILEUP_PROFILE, _lib.KS_PILEUP_QUERY, 0)
        side = (vp(qb[1]), qb[2], qb[3])
        other = (vp(tb[0]), vp(tb[1]), tb[2], tb[3])
        params = ks.profile_params(None, beta=args.beta)

        def pileup():
            out = vp()
            ctx._check(L.ks_cigars_pileup(ctx._h, cg._h, al._h, hits._h, None, *side, *other, C.byref(po), C.byref(out)))
            return ks.engine.Pileup(ctx, out)
        pu = pileup()

        def weights():
            out = vp()
            ctx._check(L.ks_cigars_pileup_weights(ctx._h, cg._h, al._h, pu._h, hits._h, None, vp(qb[0]), *side, *other, _lib.KS_PILEUP_QUERY,
                                                  _lib.KS_PWEIGHTS_INCLUDE_QUERY, C.byref(out)))
            return ks.EntryWeights(ctx, out)
        ew = weights()

        def pileup_weighted():
            out = vp()
            ctx._check(L.ks_cigars_pileup_weighted(ctx._h, cg._h, al._h, hits._h, None, *side, *other, vp(ew.weight_ptr), C.byref(po), C.byref(out)))
            return ks.engine.Pileup(ctx, out)
        wp = pileup_weighted()

        def build(fn, p):
            def call():
                o, keep = params._opts()
                out = vp()
                ctx._check(fn(ctx._h, p._h, vp(qb[0]), vp(qb[1]), qb[2], qb[3], C.byref(o), C.byref(out)))
                return ks.Profile(ctx, out)
            return call
        cases = {
            "pileup": _measure(ctx, pileup, args.repeats),
            "weights": _measure(ctx, weights, args.repeats),
            "pileup_weighted": _measure(ctx, pileup_weighted, args.repeats),
            "build": _measure(ctx, build(L.ks_profile_build_pileup, pu), args.repeats),
            "build_weighted": _measure(ctx, build(L.ks_profile_build_weighted_pileup, wp), args.repeats),
        }
        weight, n_cols = ew.to_host()
        depth = pu.to_host()[0]
        n_res, n_ent, cols, ops = int(q_off[-1]), int(cg.n_regions), int(n_cols.sum()), int(cg.n_ops)
        med = lambda c, w: cases[c][w]["median_ms"]  # noqa: E731
        ratio = lambda a, b: {w: round(med(a, w) / max(med(b, w), 1e-9), 3) for w in ("wall", "kernel")}  # noqa: E731
        entries = 8 * ops + 24 * n_ent  # the ops read twice, the offsets and the starts
        print(json.dumps({"what": "device_pweights", "workload": "10k_x_10k_protein_k7_s1", "rows": rg.n_rows, "entries": n_ent, "pair_columns": cols,
                          "query_residues": n_res, "residues_observed": int((depth > 0).sum()), "beta": args.beta, **cases,
                          "ratio_pileup_weighted": ratio("pileup_weighted", "pileup"), "ratio_build_weighted": ratio("build_weighted", "build"),
                          "ratio_weights": ratio("weights", "pileup"),
                          "mean_weight": round(float(weight[n_cols > 0].mean()) / _lib.KS_WEIGHT_ONE, 4),
                          "bytes": {"pileup": 112 * n_res + 16 * n_res + entries + 5 * cols,
                                    "weights": 112 * n_res + 2 * n_res + entries + 7 * cols + 8 * n_ent,
                                    "pileup_weighted": (112 + 224 + 8) * n_res + 16 * n_res + entries + 21 * cols,
                                    "build": (112 + 4 + 1 + 28 + 1 + 4) * n_res, "build_weighted": (112 + 4 + 1 + 28 + 1 + 4) * n_res + 224 * int((depth > 0).sum())}}),
              flush=True)


if __name__ == "__main__":
    main()
