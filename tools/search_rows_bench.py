#!/usr/bin/env python3
"""Cost of the search options (ks_search_ex): per-row abundance statistics and the containment filter.

    python tools/search_rows_bench.py [--repeats R] [--skip-1m] [--host-lib OTHER.so ...]

device : wall time of the synchronous ks_search call (it returns after its last wait) on the 200k all-vs-all
         (hp k=24 scaled=5) and the 1M x 1M protein k=10 workloads, plain vs abund_stats vs abund_stats +
         min_containment=0.5, plus the per-kernel event times of the new launches from one timed pass.
host   : wall time of ksh_index_search (ProteomeIndex::search and its JSON rows) for 20k query records against a
         20k-target index, for this library and for every --host-lib (e.g. the parent tree's, built with
         tools/build_variant.py NAME --rev HEAD~1).  Each runs in a child process of its own.
Prints one JSON line per measurement (median, min, max over the repeats)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    xs = sorted(xs)
    return {"median_ms": xs[len(xs) // 2] * 1e3, "min_ms": xs[0] * 1e3, "max_ms": xs[-1] * 1e3, "n": len(xs)}


def device(args):
    import kmerseek_amd as ks
    from kmerseek_amd import synth
    work = [("c5_200k_hp_k24_s5", 200_000, 24, 5, "hp", True)]
    if not args.skip_1m:
        work.append(("c4_1m_protein_k10_s1", 1_000_000, 10, 1, "protein", False))
    variants = [("plain", {}), ("abund_stats", {"abund_stats": True}),
                ("abund_stats+min_containment=0.5", {"abund_stats": True, "min_containment": 0.5})]
    for name, n, k, scaled, mol, all_vs_all in work:
        t_res, t_off = synth.proteome(n, stream=40 if all_vs_all else 0)
        q_res, q_off = (t_res, t_off) if all_vs_all else synth.queries(n, t_res, t_off, stream=1000)
        with ks.Context(0) as ctx:
            T = ctx.sketch_batch(t_res, t_off, k, scaled, mol)
            ix = ctx.index_build(T)
            Q = ctx.sketch_batch(q_res, q_off, k, scaled, mol)
            T.free()
            counts = {}
            for label, kw in variants:  # warm-up (pool, row hint) and the row counts
                for _ in range(2):
                    H = ctx.search(ix, Q, **kw)
                    counts[label] = H.count
                    H.free()
            times = {label: [] for label, _ in variants}
            for _ in range(args.repeats):  # interleaved: drift hits every variant alike
                for label, kw in variants:
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    H = ctx.search(ix, Q, **kw)
                    times[label].append(time.perf_counter() - t0)
                    H.free()
            ctx.timing_enable(1)
            kern = {}
            for label, kw in variants:
                ctx.timing_reset()
                ctx.search(ix, Q, **kw).free()
                kern[label] = {kn: round(ms, 4) for kn, (_, ms) in ctx.timing().items()
                               if kn.startswith(("row_abund", "rows_", "scan", "msd", "sort", "pair_rows"))}
            ctx.timing_enable(0)
            for label, _ in variants:
                print(json.dumps({"what": "device_search", "workload": name, "variant": label, "rows": counts[label],
                                  **_spread(times[label]), "kernels_ms": kern[label]}), flush=True)


def host_child(lib_path, n_t, n_q, repeats):
    """ksh_index_search through ctypes on `lib_path` (works for libraries older than the search options)."""
    import tempfile
    import numpy as np
    from kmerseek_amd import synth
    L = C.CDLL(lib_path)
    L.ksh_index_new.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                C.c_char_p, C.c_size_t]
    L.ksh_index_add_records.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_char_p,
                                        C.c_size_t]
    L.ksh_index_search.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.c_int,
                                   C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.ksh_string_free.argtypes = [C.c_void_p]
    L.ksh_index_free.argtypes = [C.c_void_p]
    err = C.create_string_buffer(1024)
    t_res, t_off = synth.proteome(n_t, stream=40)
    q_res, q_off = synth.queries(n_q, t_res, t_off, stream=41)

    def recs(res, off, tag):
        seqs = [bytes(res[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
        return (C.c_char_p * len(seqs))(*seqs), (C.c_char_p * len(seqs))(*[f"{tag}{i}".encode() for i in range(len(seqs))]), len(seqs)

    out = {}
    with tempfile.TemporaryDirectory() as d:
        for (k, scaled, mol) in ((24, 5, "hp"), (10, 1, "protein")):
            h = C.c_void_p()
            assert L.ksh_index_new(os.path.join(d, f"{mol}{k}.db").encode(), k, scaled, mol.encode(), 0, 0, 0, C.byref(h), err, 1024) == 0, err.value
            s, nm, n = recs(t_res, t_off, "t")
            assert L.ksh_index_add_records(h, s, nm, n, 0, err, 1024) == 0, err.value
            qs, qn, nq = recs(q_res, q_off, "q")
            ts, n_rows = [], 0
            for r in range(repeats + 1):
                js = C.c_void_p()
                t0 = time.perf_counter()
                assert L.ksh_index_search(h, qs, qn, nq, 0, C.byref(js), err, 1024) == 0, err.value
                dt = time.perf_counter() - t0
                n_rows = C.string_at(js).count(b'{"query_name"')
                L.ksh_string_free(js)
                if r:  # (the first call builds the device index)
                    ts.append(dt)
            L.ksh_index_free(h)
            out[f"{mol}_k{k}_s{scaled}"] = {"rows": n_rows, **_spread(ts)}
    print(json.dumps(out), flush=True)


def host(args):
    from kmerseek_amd import build
    for lib in [build.SO] + args.host_lib:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child", lib, "--repeats", str(args.host_repeats)],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            print(json.dumps({"what": "host_search", "lib": os.path.basename(lib), "error": p.stderr[-2000:]}), flush=True)
            continue
        print(json.dumps({"what": "host_search", "lib": os.path.basename(lib), "records": [args.host_targets, args.host_queries],
                          **json.loads(p.stdout.strip().splitlines()[-1])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--host-lib", action="append", default=[])
    ap.add_argument("--host-targets", type=int, default=20_000)
    ap.add_argument("--host-queries", type=int, default=20_000)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-child")
    a = ap.parse_args()
    if a.host_child:
        host_child(a.host_child, a.host_targets, a.host_queries, a.repeats)
        return
    if not a.skip_device:
        device(a)
    host(a)


if __name__ == "__main__":
    main()
