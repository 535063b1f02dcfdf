#!/usr/bin/env python3
"""Cost and effect of low-complexity masking (ks_sketch_masked_device) on one MI355X, inputs resident on the device.

    python tools/mask_bench.py [--sets 10k,200k,golden] [--repeats 5] [--no-search]
    python tools/mask_bench.py --plain-only [--root <checkout of the parent commit>]

Workloads: "10k" = synth.proteome(10,000) at protein k=7 scaled=1, "200k" = synth.proteome(200,000) at hp k=24 scaled=5 (the
reference CLI's defaults), "golden" = tests/golden/uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz at hp k=24 scaled=5,
the file that is full of low-complexity regions.  Per set: wall time of the masked sketch call (median [min - max] of the
repeats) beside the plain sketch of the same batch, the four stages called one by one through the public entry points (mask,
split, sketch of the segments, union by record), the kernel event times of one masked call (ks_timing), masked share, segments per
record, and the rows of the all-vs-all search of the set with and without masking.
--plain-only times nothing but the plain sketch of the two synthetic sets, with the package under --root: run it on a checkout of
the parent commit in the same job for the baseline.  Prints one JSON line per set."""
import argparse
import json
import os
import sys
import time

SETS = {"10k": ("protein", 7, 1, 10000), "200k": ("hp", 24, 5, 200000), "golden": ("hp", 24, 5, 0)}
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden", "uniprotkb_protein_name_Uncharacterized_2025_04_15.fasta.gz")


def _spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4), "n": len(xs)}


def _timed(ctx, fn, repeats, keep=False):
    ts, out = [], None
    for _ in range(repeats + 1):  # (the first pass sizes the pool: not counted)
        if out is not None and hasattr(out, "free"):
            out.free()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    if not keep and hasattr(out, "free"):
        out.free()
        out = None
    return ts[1:], out


def _batch(name, np, synth, wire):
    mol, k, scaled, n = SETS[name]
    if n:
        res, offs = synth.proteome(n, stream=0)
    else:
        from kmerseek_amd import pack
        res, offs = pack([r for _, r in wire.read_fasta(GOLDEN)])
    return mol, k, scaled, res, offs


def _rows(ctx, sk):
    ix = ctx.index_build(sk)
    hits = ctx.search(ix, sk)
    n = hits.count
    hits.free(); ix.free()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="10k,200k,golden")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth, wire

    ctx = ks.Context(0)
    for name in args.sets.split(","):
        if args.plain_only and not SETS[name][3]:
            continue
        mol, k, scaled, res, offs = _batch(name, np, synth, wire)
        n, n_res = len(offs) - 1, len(res)
        mx = int((offs[1:] - offs[:-1]).max())
        d_res, d_off = ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(offs)
        plain_call = lambda: ctx.sketch_batch_device(d_res.ptr, d_off.ptr, n, n_res, k, scaled, mol, max_seq_len=mx)  # noqa: E731
        t_plain, P = _timed(ctx, plain_call, args.repeats, keep=True)
        row = {"what": "plain sketch" if args.plain_only else "masked sketch", "set": name, "moltype": mol, "ksize": k, "scaled": scaled, "records": n,
               "residues": n_res, "library": ks.SO_PATH, "plain": _spread(t_plain), "plain_windows": P.n_windows, "plain_hashes": P.n_hashes}
        if args.plain_only:
            P.free()
            print(json.dumps(row), flush=True)
            continue
        masked_call = lambda: ctx.sketch_masked_device(d_res.ptr, d_off.ptr, n, n_res, k, scaled, mol, max_seq_len=mx)  # noqa: E731
        t_masked, S = _timed(ctx, masked_call, args.repeats, keep=True)
        ctx.timing_enable(1); ctx.timing_reset()
        masked_call().free()
        kern = {kn: {"launches": c, "ms": round(ms, 4)} for kn, (c, ms) in sorted(ctx.timing().items())}
        ctx.timing_enable(0)
        # the stages one by one
        t_mask, M = _timed(ctx, lambda: ctx.mask_low_complexity_device(d_res.ptr, d_off.ptr, n, n_res), args.repeats, keep=True)
        t_split, G = _timed(ctx, lambda: ctx.split_masked_device(M, d_res.ptr, d_off.ptr, n, n_res, k), args.repeats, keep=True)
        seg_rec, seg_start, seg_off, seg_res, groups = G.device_ptrs()
        n_segs = G.n_segs
        t_sk, parts = _timed(ctx, lambda: ctx.sketch_batch_device(seg_res, seg_off, n_segs, G.n_residues, k, scaled, mol, max_seq_len=mx), args.repeats,
                             keep=True)
        go = G.to_host()[4]
        parts.union_groups(go).free()  # (makes the set dense once, outside the timed region)
        t_un, _ = _timed(ctx, lambda: parts.union_groups(go), args.repeats)
        per_rec = np.diff(go.astype(np.int64))
        row.update({"call": _spread(t_masked), "ratio": round(_spread(t_masked)["median_ms"] / _spread(t_plain)["median_ms"], 3),
                    "stages": {"mask": _spread(t_mask), "split": _spread(t_split), "sketch_segments": _spread(t_sk), "union": _spread(t_un)},
                    "union_path": "sort" if per_rec.max() > int(ks._lib.load().ks_debug_union_rank_max()) else "rank",
                    "masked_residues": M.n_masked, "masked_share": round(M.n_masked / max(n_res, 1), 5), "segments": n_segs,
                    "segment_residues": G.n_residues, "segments_per_record_mean": round(float(per_rec.mean()), 4),
                    "segments_per_record_max": int(per_rec.max()), "records_without_segment": int((per_rec == 0).sum()),
                    "records_with_more_than_8_segments": int((per_rec > 8).sum()), "windows": S.n_windows, "hashes": S.n_hashes,
                    "windows_surviving": round(S.n_windows / max(P.n_windows, 1), 5), "kernels": kern})
        parts.free(); G.free(); M.free()
        if not args.no_search:
            row["search_rows_plain"] = _rows(ctx, P)
            row["search_rows_masked"] = _rows(ctx, S)
        P.free(); S.free(); d_res.free(); d_off.free()
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
