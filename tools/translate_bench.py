#!/usr/bin/env python3
"""Cost of the translated sketch (ks_sketch_translated_device) on one MI355X, inputs resident on the device.

    python tools/translate_bench.py [--proteins 20000] [--repeats 5] [--dump-frames frames.npz]
    python tools/translate_bench.py --plain-only --frames frames.npz [--root <checkout of the parent commit>]

Workload: synthetic DNA made by reverse-translating synth.proteome (for every residue one of its codons of the standard code, at
random), every second record reverse-complemented, at protein k=7 scaled=1 and hp k=24 scaled=5.  Per parameter set: wall time of
the synchronous call (median, min, max over the repeats), the per-kernel event times of one timed pass (ks_timing), and the three
stages called one by one through the public entry points — ks_translate6_device, ks_sketch_batch_device on the frames,
ks_sketches_union_groups with groups of six (rank path and sort path) — so that the stage that takes the time can be named.

The number to set the call against is the plain sketch of its own frames: a protein batch with the same residue count and the
same sequence lengths.  This build measures it too ("plain_frames"); for the plain sketch of the PARENT commit, dump the frames
(--dump-frames) and run the second form from (or with --root pointing at) a built checkout of that commit: that mode only uses
entry points the parent has.  Prints one JSON line per parameter set; "ratio" = translated call / plain sketch of the frames."""
import argparse
import ctypes as C
import json
import os
import sys
import time

PARAMS = (("protein", 7, 1), ("hp", 24, 5))
TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"


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


def reverse_translate(np, residues, offsets, seed=7):
    """(bases u8, offsets u64): a random codon per residue; every second record reverse-complemented"""
    rng = np.random.default_rng(seed)
    codons = {}
    for i, r in enumerate(TABLE):
        codons.setdefault(ord(r), []).append([b"TCAG"[i >> 4], b"TCAG"[(i >> 2) & 3], b"TCAG"[i & 3]])
    n_of = np.zeros(256, np.int64)
    tab = np.zeros((256, 6, 3), np.uint8)
    for r, cs in codons.items():
        n_of[r] = len(cs)
        tab[r, :len(cs)] = cs
    assert n_of[residues].min() > 0, "a residue without a codon"
    pick = (rng.random(len(residues)) * n_of[residues]).astype(np.int64)
    nt = tab[residues, pick].reshape(-1).copy()
    offs = (3 * offsets.astype(np.uint64)).astype(np.uint64)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    for s in range(1, len(offs) - 1, 2):
        b, e = int(offs[s]), int(offs[s + 1])
        nt[b:e] = comp[nt[b:e][::-1]]
    return nt, offs


def plain_only(args):
    import numpy as np
    import kmerseek_amd as ks
    z = np.load(args.frames)
    res, offs = z["residues"], z["offsets"]
    ctx = ks.Context(0)
    d_res, d_off = ctx.to_device(np.concatenate([res, np.zeros(16, np.uint8)])), ctx.to_device(offs)
    mx = int((offs[1:] - offs[:-1]).max()) if len(offs) > 1 else 0
    for mol, k, scaled in PARAMS:
        ts, _ = _timed(ctx, lambda: ctx.sketch_batch_device(d_res.ptr, d_off.ptr, len(offs) - 1, len(res), k, scaled, mol, max_seq_len=mx), args.repeats)
        print(json.dumps({"what": "plain sketch of the dumped frames", "moltype": mol, "ksize": k, "scaled": scaled, "sequences": len(offs) - 1,
                          "residues": int(len(res)), "library": ks.SO_PATH, "plain_frames": _spread(ts)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dump-frames")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--frames")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if args.plain_only:
        return plain_only(args)
    import numpy as np
    import kmerseek_amd as ks
    from kmerseek_amd import synth

    nt, offs = reverse_translate(np, *synth.proteome(args.proteins, stream=31))
    n, n_nt, mx = len(offs) - 1, len(nt), int((offs[1:] - offs[:-1]).max())
    ctx = ks.Context(0, follow_debug_env=True)
    d_nt, d_off = ctx.to_device(nt), ctx.to_device(offs)
    frames, foff, n_res = ctx.translate6(nt, offs)
    if args.dump_frames:
        np.savez(args.dump_frames, residues=frames.to_host(np.uint8, n_res), offsets=foff.to_host(np.uint64, 6 * n + 1))
    for mol, k, scaled in PARAMS:
        os.environ.pop("KS_DEBUG_UNION_PATH", None)
        call = lambda: ctx.sketch_translated_device(d_nt.ptr, d_off.ptr, n, n_nt, k, scaled, mol, max_seq_len=mx)  # noqa: E731
        whole, sk = _timed(ctx, call, args.repeats, keep=True)
        n_hashes, n_windows = sk.n_hashes, sk.n_windows
        sk.free()
        ctx.timing_enable(1)
        ctx.timing_reset()
        call().free()
        kern = {name: {"launches": c, "ms": round(ms, 4)} for name, (c, ms) in sorted(ctx.timing().items())}
        ctx.timing_enable(0)
        # the three stages one by one
        scratch = [ctx.to_device(np.zeros(2 * n_nt + 16, np.uint8)), ctx.to_device(np.zeros(6 * n + 1, np.uint64))]
        out_n = C.c_uint64(0)
        t_tr, _ = _timed(ctx, lambda: ctx._check(ctx._L.ks_translate6_device(ctx._h, d_nt._p, d_off._p, n, n_nt, scratch[0]._p, scratch[1]._p,
                                                                               C.byref(out_n))), args.repeats)
        t_sk, six = _timed(ctx, lambda: ctx.sketch_batch_device(frames.ptr, foff.ptr, 6 * n, n_res, k, scaled, mol, max_seq_len=max(mx // 3, 1)),
                           args.repeats, keep=True)
        go = 6 * np.arange(n + 1, dtype=np.uint32)
        six.union_groups(go).free()  # (makes the six-fold set dense once, outside the timed region of both paths)
        t_un = {}
        for name, knob in (("rank", "1"), ("sort", "2")):
            os.environ["KS_DEBUG_UNION_PATH"] = knob
            t_un[name], _ = _timed(ctx, lambda: six.union_groups(go), args.repeats)
        os.environ.pop("KS_DEBUG_UNION_PATH", None)
        six_hashes = six.n_hashes
        six.free()
        for b in scratch:
            b.free()
        plain = _spread(t_sk)
        row = {"what": "translated sketch", "moltype": mol, "ksize": k, "scaled": scaled, "records": n, "bases": n_nt, "frame_residues": n_res,
               "windows": n_windows, "hashes": n_hashes, "six_fold_hashes": six_hashes, "call": _spread(whole), "plain_frames": plain,
               "ratio": round(_spread(whole)["median_ms"] / plain["median_ms"], 3),
               "stages": {"translate6": _spread(t_tr), "sketch_frames": plain, "union_rank": _spread(t_un["rank"]), "union_sort": _spread(t_un["sort"])},
               "gbases_per_s": round(n_nt / (_spread(whole)["median_ms"] * 1e-3) / 1e9, 3), "library": ks.SO_PATH, "kernels": kern}
        print(json.dumps(row))


if __name__ == "__main__":
    main()
