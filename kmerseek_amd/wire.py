"""Wire formats around the hot path, so the reference's Python callers can consume GPU results unchanged.

* ``sketch()``        — drop-in for src/python/kmerseek/sketch.py:28-40 (branchwater ``do_manysketch(singleton=True)``):
                        writes ``<fasta>.manysketch.csv`` and a sourmash-compatible ``<fasta>.{moltype}.k{k}.scaled{s}.sig.zip``
                        (gzipped JSON signatures + SOURMASH-MANIFEST.csv).
* ``do_manysearch()`` — drop-in for src/python/kmerseek/search.py:125-141 (branchwater ``do_manysearch`` with threshold 0,
                        abundance on, output_all off): writes the 22-column CSV pinned by tests/test_search.py:33-39.
* ``do_multisearch()`` — drop-in for src/python/kmerseek/search.py:144-158 (branchwater ``do_multisearch`` with threshold 0, no
                        ANI, probability of overlap on, output_all off): the 16-column CSV of the reference's fixture
                        tests/testdata/index/ced9-bcl2-first25.hp.k16.manysearch.csv.
* ``do_cluster()``    — all-vs-all search of one .sig.zip, then the connected components at a similarity threshold: a CSV of
                        clusters in this project's own format (modelled on branchwater ``cluster``; no parity claimed).
* ``do_gather()``     — search, then per query the greedy non-redundant targets (Context.gather): a CSV in this project's own
                        format (modelled on branchwater ``fastmultigather``; no parity claimed).
Hashing, sorting, joining and counting all run in the HIP library; this module only formats.  The ratio columns are
f64 arithmetic on the integer results (formulas: SURVEY.md §8(a) row a10).
"""
from __future__ import annotations

import csv
import gzip
import hashlib
import io
import json
import math
import os
import zipfile
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .engine import Context, max_hash, pack

MANYSEARCH_COLUMNS = [
    "query_name", "query_md5", "match_name", "containment", "intersect_hashes", "ksize", "scaled", "moltype",
    "match_md5", "jaccard", "max_containment", "average_abund", "median_abund", "std_abund",
    "query_containment_ani", "match_containment_ani", "average_containment_ani", "max_containment_ani",
    "n_weighted_found", "total_weighted_hashes", "containment_target_in_query", "f_weighted_target_in_query",
]

MULTISEARCH_COLUMNS = [
    "query_name", "query_md5", "match_name", "match_md5", "containment", "max_containment", "jaccard", "intersect_hashes",
    "ksize", "scaled", "moltype", "prob_overlap", "prob_overlap_adjusted", "containment_adjusted",
    "containment_adjusted_log10", "tf_idf_score",
]


def read_fasta(path: str) -> List[Tuple[str, bytes]]:
    """[(full header, sequence bytes)] from a plain or gzipped FASTA (manysketch hashes records as given)."""
    op = gzip.open if str(path).endswith(".gz") else open
    recs: List[Tuple[str, List[bytes]]] = []
    with op(path, "rb") as f:
        for line in f.read().splitlines():
            if line.startswith(b">"):
                recs.append((line[1:].decode(), []))
            elif recs and line.strip():
                recs[-1][1].append(line.strip())
    return [(n, b"".join(p)) for n, p in recs]


def sourmash_md5(mins: np.ndarray, protein_ksize: int) -> str:
    """md5sum field of a sourmash signature: MD5(ascii(3k) || ascii(min) ...)."""
    m = hashlib.md5()
    m.update(str(protein_ksize * 3).encode())
    m.update("".join(map(str, np.asarray(mins, dtype=np.uint64).tolist())).encode())
    return m.hexdigest()


# ---------------------------------------------------------------------------------------------------------
# .sig.zip
# ---------------------------------------------------------------------------------------------------------
def write_sig_zip(path: str, names: Sequence[str], offsets: np.ndarray, mins: np.ndarray, abunds: np.ndarray,
                  ksize: int, scaled: int, moltype: str, filename: str) -> None:
    """One gzipped JSON signature per record under signatures/<md5>.sig.gz + SOURMASH-MANIFEST.csv (stored, not deflated)."""
    mh = max_hash(scaled)
    rows = []
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
        for i, name in enumerate(names):
            m = mins[int(offsets[i]):int(offsets[i + 1])]
            a = abunds[int(offsets[i]):int(offsets[i + 1])]
            md5 = sourmash_md5(m, ksize)
            doc = [{"class": "sourmash_signature", "email": "", "hash_function": "0.murmur64", "filename": filename,
                    "name": name, "license": "CC0",
                    "signatures": [{"num": 0, "ksize": 3 * ksize, "seed": 42, "max_hash": mh, "mins": m.tolist(),
                                    "md5sum": md5, "abundances": a.tolist(), "molecule": moltype}],
                    "version": 0.4}]
            loc = f"signatures/{md5}.sig.gz"
            buf = io.BytesIO()
            with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as g:
                g.write(json.dumps(doc, separators=(",", ":")).encode())
            z.writestr(loc, buf.getvalue())
            rows.append([loc, md5, md5[:8], ksize, moltype, 0, scaled, len(m), 1, name, filename])
        out = io.StringIO()
        out.write("# SOURMASH-MANIFEST-VERSION: 1.0\n")
        w = csv.writer(out, lineterminator="\n")
        w.writerow(["internal_location", "md5", "md5short", "ksize", "moltype", "num", "scaled", "n_hashes",
                    "with_abundance", "name", "filename"])
        w.writerows(rows)
        z.writestr("SOURMASH-MANIFEST.csv", out.getvalue())


def read_sig_zip(path: str):
    """-> (names, offsets u64[n+1], mins u64, abunds u32, ksize (protein), scaled, moltype), in manifest order."""
    z = zipfile.ZipFile(path)
    text = "\n".join(l for l in z.read("SOURMASH-MANIFEST.csv").decode().splitlines() if not l.startswith("#"))
    names, mins, abunds, offs = [], [], [], [0]
    ksize = scaled = None
    moltype = None
    for row in csv.DictReader(io.StringIO(text)):
        doc = json.loads(gzip.decompress(z.read(row["internal_location"])))
        sig = doc[0]["signatures"][0]
        names.append(doc[0]["name"])
        mins.extend(sig["mins"])
        abunds.extend(sig.get("abundances") or [1] * len(sig["mins"]))
        offs.append(len(mins))
        have = (sig["ksize"] // 3, int(row["scaled"]), sig["molecule"])
        if ksize is not None and have != (ksize, scaled, moltype):  # every row, not only the last one
            raise ValueError(f"{path}: sketch {doc[0]['name']!r} was made with {have}, earlier ones with "
                             f"{(ksize, scaled, moltype)}: one search takes one set of parameters")
        ksize, scaled, moltype = have
        mh = max_hash(scaled)
        if any(h == 0 or h > mh for h in sig["mins"]) or (sig.get("max_hash") not in (None, 0, mh)):
            raise ValueError(f"{path}: sketch {doc[0]['name']!r} holds hashes outside (0, max_hash(scaled={scaled})]")
    return (names, np.array(offs, np.uint64), np.array(mins, np.uint64), np.array(abunds, np.uint32), ksize, scaled,
            moltype)


# ---------------------------------------------------------------------------------------------------------
# sketch()  — src/python/kmerseek/sketch.py
# ---------------------------------------------------------------------------------------------------------
def make_sketch_kws(moltype: str, ksize: int, scaled: int):
    return dict(ksize=ksize, moltype=moltype, scaled=scaled)


def _make_manysketch_csv(fasta: str) -> str:
    path = f"{fasta}.manysketch.csv"
    with open(path, "w") as f:
        f.write("name,genome_filename,protein_filename\n")
        f.write(f"{os.path.basename(fasta)},,{fasta}\n")
    return path


def _make_sigfile(fasta: str, moltype: str, ksize: int, scaled: int) -> str:
    return f"{fasta}.{moltype}.k{ksize}.scaled{scaled}.sig.zip"


def sketch(fasta: str, moltype: str, ksize: int, scaled: int, ctx: Optional[Context] = None, translate: bool = False,
           mask: bool = False, mask_opts: Optional[dict] = None) -> str:
    """sketch() of src/python/kmerseek/sketch.py:28-40.  The records go through the native pipelined ingest
    (csrc/ks_ingest.cpp: parse, pinned staging, H2D and the sketch kernels overlap); `ctx` only picks the device.
    translate=True: the records are NUCLEOTIDES; each is translated in six frames on the device and sketched as the union of
    its frames (Context.sketch_translated).  The .sig.zip is written by the same code: same molecule, same names.
    mask=True: the low-complexity stretches of every record are left out of its sketch (Context.sketch_masked; mask_opts: its
    window / k1 / k2 keywords, None for the defaults).  Same file, same names; a record masked throughout has an empty sketch.
    Not together with translate=True: translated frames are not masked."""
    from . import host
    if mask and translate:
        raise ValueError("mask=True and translate=True: masking of translated frames is not built")
    if mask_opts is not None and not mask:
        raise ValueError("mask_opts needs mask=True")
    sigfile = _make_sigfile(fasta, moltype, ksize, scaled)
    _make_manysketch_csv(fasta)
    if translate or mask:
        recs = read_fasta(fasta)
        own = ctx is None
        c = Context(0) if own else ctx
        try:
            if mask:
                sk = c.sketch_masked(*pack([r for _, r in recs]), ksize, scaled, moltype, **(mask_opts or {}))
            else:
                sk = c.sketch_translated(*pack([r for _, r in recs]), ksize, scaled, moltype)
            o, m, a = sk.to_host()
            sk.free()
        finally:
            if own:
                c.close()
        write_sig_zip(sigfile, [n for n, _ in recs], o, m, a, ksize, scaled, moltype, os.path.abspath(fasta))
        return sigfile
    names, o, m, a, _ = host.sketch_fasta(fasta, ksize, scaled, moltype, validate=False,
                                          device=ctx.device if ctx is not None and hasattr(ctx, "device") else 0)
    write_sig_zip(sigfile, names, o, m, a, ksize, scaled, moltype, os.path.abspath(fasta))
    return sigfile


# ---------------------------------------------------------------------------------------------------------
# do_manysearch()  — src/python/kmerseek/search.py:125-141
# ---------------------------------------------------------------------------------------------------------
def manysearch_rows(q_names, q_off, q_mins, t_names, t_off, t_mins, t_abund, hits, ksize: int, scaled: int,
                    moltype: str) -> List[dict]:
    """The 22 CSV columns for every COO hit (qid, tid, intersect, n_weighted)."""
    qid, tid, isect, nw = hits
    k3 = 3 * ksize
    t_tot = np.add.reduceat(t_abund.astype(np.uint64), t_off[:-1].astype(np.int64)) if len(t_abund) else np.zeros(len(t_off) - 1, np.uint64)
    t_tot = np.where((t_off[1:] - t_off[:-1]) > 0, t_tot, 0)
    md5_q, md5_t = {}, {}
    rows = []
    for q, t, i, w in zip(qid.tolist(), tid.tolist(), isect.tolist(), nw.tolist()):
        qm = q_mins[int(q_off[q]):int(q_off[q + 1])]
        tm = t_mins[int(t_off[t]):int(t_off[t + 1])]
        ta = t_abund[int(t_off[t]):int(t_off[t + 1])]
        # abundance statistics need the per-hash target abundances of the shared hashes (not just their sum)
        shared = ta[np.isin(tm, qm, assume_unique=True)].astype(np.float64)
        assert len(shared) == i
        shared.sort()
        n = len(shared)
        mean = float(shared.mean())
        median = float(shared[n // 2]) if n % 2 else float((shared[n // 2 - 1] + shared[n // 2]) / 2.0)
        std = math.sqrt(float(((shared - mean) ** 2).sum()) / n)
        nq, nt = len(qm), len(tm)
        cq, ct = i / nq, i / nt
        q_ani, t_ani = cq ** (1.0 / k3), ct ** (1.0 / k3)
        if q not in md5_q:
            md5_q[q] = sourmash_md5(qm, ksize)
        if t not in md5_t:
            md5_t[t] = sourmash_md5(tm, ksize)
        tot_w = int(t_tot[t])
        rows.append({
            "query_name": q_names[q], "query_md5": md5_q[q], "match_name": t_names[t], "containment": cq,
            "intersect_hashes": i, "ksize": k3, "scaled": scaled, "moltype": moltype, "match_md5": md5_t[t],
            "jaccard": i / (nq + nt - i), "max_containment": max(cq, ct), "average_abund": mean,
            "median_abund": median, "std_abund": std, "query_containment_ani": q_ani, "match_containment_ani": t_ani,
            "average_containment_ani": (q_ani + t_ani) / 2.0, "max_containment_ani": max(q_ani, t_ani),
            "n_weighted_found": w, "total_weighted_hashes": tot_w, "containment_target_in_query": ct,
            "f_weighted_target_in_query": w / tot_w,
        })
    return rows


def do_manysearch(query_sig: str, target_sig: str, output: str, ksize: int, scaled: int, moltype: str,
                  ctx: Optional[Context] = None, top_k: int = 0, rank_by: str = "intersect") -> int:
    """Search every sketch of query_sig (.sig.zip) against every sketch of target_sig; CSV rows for pairs that share
    at least one hash.  top_k > 0 keeps only the top_k best matches of every query (Context.best_hits; rank_by: intersect |
    target_containment | max_containment | jaccard), in the same order as before.  Returns the number of rows written."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        qn, qo, qm, qa, qk, qs, qmol = read_sig_zip(query_sig)
        tn, to, tm, ta, tk, ts, tmol = read_sig_zip(target_sig)
        for have in ((qk, qs, qmol), (tk, ts, tmol)):
            if have != (ksize, scaled, moltype):
                raise ValueError(f"sketch parameters {have} do not match the requested {(ksize, scaled, moltype)}")
        Q = ctx.sketches_from_host(qo, qm, qa, ksize, scaled, moltype)
        T = ctx.sketches_from_host(to, tm, ta, ksize, scaled, moltype)
        hits = ctx.search(ctx.index_build(T), Q)
        if top_k > 0:
            hits = ctx.best_hits(hits, top_k, rank_by, queries=Q, targets=T)
        hits = hits.to_host()
        rows = manysearch_rows(qn, qo, qm, tn, to, tm, ta, hits, ksize, scaled, moltype)
        with open(output, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=MANYSEARCH_COLUMNS, lineterminator="\n")
            w.writeheader()
            w.writerows(rows)
        return len(rows)
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------
# do_multisearch()  — src/python/kmerseek/search.py:144-158
# ---------------------------------------------------------------------------------------------------------
def format_f64(x: float) -> str:
    """An f64 as the reference's CSV prints it: the shortest digits that read back as the same value, never an exponent,
    and '.0' behind a whole number (2.0, 0.000023191094619666044)."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    r = repr(x)
    if "e" not in r and "E" not in r:
        return r
    from decimal import Decimal
    t = format(Decimal(r), "f")
    return t if "." in t else t + ".0"


def multisearch_rows(q_names, q_off, q_mins, t_names, t_off, t_mins, hits, prob_overlap, tf_idf, ksize: int, scaled: int,
                     moltype: str) -> List[dict]:
    """The 16 CSV columns for every COO hit (qid, tid, intersect, n_weighted) with its two significance sums
    (Context.significance).  Derived here, in f64: prob_overlap_adjusted = prob_overlap * (n_queries * n_targets) — every
    sequence of either batch counts, empty sketches included —, containment_adjusted = containment / prob_overlap_adjusted
    and its log10."""
    qid, tid, isect, _ = hits
    n_comparisons = float((len(q_off) - 1) * (len(t_off) - 1))
    md5_q, md5_t = {}, {}
    rows = []
    for q, t, i, po, tf in zip(qid.tolist(), tid.tolist(), isect.tolist(), np.asarray(prob_overlap, np.float64).tolist(),
                               np.asarray(tf_idf, np.float64).tolist()):
        qm = q_mins[int(q_off[q]):int(q_off[q + 1])]
        tm = t_mins[int(t_off[t]):int(t_off[t + 1])]
        nq, nt = len(qm), len(tm)
        if q not in md5_q:
            md5_q[q] = sourmash_md5(qm, ksize)
        if t not in md5_t:
            md5_t[t] = sourmash_md5(tm, ksize)
        cq, ct = float(i) / float(nq), float(i) / float(nt)
        adj = po * n_comparisons
        c_adj = cq / adj if adj != 0.0 else math.inf  # (f64 division: cq > 0, every row shares a hash)
        c_log = math.log10(c_adj) if 0.0 < c_adj < math.inf else (-math.inf if c_adj == 0.0 else c_adj)
        rows.append({
            "query_name": q_names[q], "query_md5": md5_q[q], "match_name": t_names[t], "match_md5": md5_t[t],
            "containment": format_f64(cq), "max_containment": format_f64(max(cq, ct)), "jaccard": format_f64(float(i) / float(nq + nt - i)),
            "intersect_hashes": format_f64(float(i)), "ksize": 3 * ksize, "scaled": scaled, "moltype": moltype,
            "prob_overlap": format_f64(po), "prob_overlap_adjusted": format_f64(adj), "containment_adjusted": format_f64(c_adj),
            "containment_adjusted_log10": format_f64(c_log), "tf_idf_score": format_f64(tf),
        })
    return rows


def do_multisearch(query_sig: str, target_sig: str, output: str, ksize: int, scaled: int, moltype: str,
                   ctx: Optional[Context] = None, top_k: int = 0, rank_by: str = "intersect") -> int:
    """Search every sketch of query_sig (.sig.zip) against every sketch of target_sig and weigh every hit (prob_overlap,
    tf_idf_score and the columns derived from them); CSV rows for pairs that share at least one hash.  top_k > 0 keeps only the
    top_k best matches of every query, in the same order as before: by one of do_manysearch's keys (the hits are thinned
    first and only the kept rows are weighed), or by tf_idf_score (every row is weighed, the best are chosen by that column
    on the device, and the kept rows' sums are gathered through src_row).  Returns the number of rows written."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        qn, qo, qm, qa, qk, qs, qmol = read_sig_zip(query_sig)
        tn, to, tm, ta, tk, ts, tmol = read_sig_zip(target_sig)
        for have in ((qk, qs, qmol), (tk, ts, tmol)):
            if have != (ksize, scaled, moltype):
                raise ValueError(f"sketch parameters {have} do not match the requested {(ksize, scaled, moltype)}")
        Q = ctx.sketches_from_host(qo, qm, qa, ksize, scaled, moltype)
        T = ctx.sketches_from_host(to, tm, ta, ksize, scaled, moltype)
        ix = ctx.index_build(T)
        hits = ctx.search(ix, Q)
        if top_k > 0 and rank_by == "tf_idf_score":
            sig = ctx.significance(Q, T, hits)
            best = ctx.best_hits(hits, top_k, score=sig.tf_idf_ptr)
            src = best.best_to_host()[1]
            po, tf = (c[src] for c in sig.to_host())
            hits.free()
            hits = best
        else:
            if top_k > 0:
                best = ctx.best_hits(hits, top_k, rank_by, queries=Q, targets=T)
                hits.free()
                hits = best
            sig = ctx.significance(Q, T, hits)
            po, tf = sig.to_host()
        rows = multisearch_rows(qn, qo, qm, tn, to, tm, hits.to_host(), po, tf, ksize, scaled, moltype)
        for o in (sig, hits, ix, Q, T):
            o.free()
        with open(output, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=MULTISEARCH_COLUMNS, lineterminator="\n")
            w.writeheader()
            w.writerows(rows)
        return len(rows)
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------
# do_cluster()  — all-vs-all, then the connected components of the similarity graph
# ---------------------------------------------------------------------------------------------------------
CLUSTER_COLUMNS = ["cluster", "representative", "size", "nodes"]


def cluster_rows(names: Sequence[str], offsets, members, representative, prefix: str = "Component") -> List[Tuple[str, str, int, str]]:
    """One row per cluster of a Clusters.to_host() CSR, in its order: (<prefix>_<i>, name of the representative, size, the
    members' names joined by ';' in ascending id order)."""
    offsets = np.asarray(offsets).astype(np.int64).tolist()
    members = np.asarray(members).tolist()
    rows = []
    for i, rep in enumerate(np.asarray(representative).tolist()):
        ids = members[offsets[i]:offsets[i + 1]]
        rows.append((f"{prefix}_{i}", names[rep], len(ids), ";".join(names[j] for j in ids)))
    return rows


def cluster_size_histogram(offsets) -> List[Tuple[int, int]]:
    """[(cluster_size, count)] ascending by size, over every cluster of the CSR."""
    sizes, counts = np.unique(np.diff(np.asarray(offsets).astype(np.int64)), return_counts=True)
    return list(zip(sizes.tolist(), counts.tolist()))


def do_cluster(sig: str, output: str, ksize: int, scaled: int, moltype: str, similarity: str = "jaccard", threshold: float = 0.0,
               sizes_output: Optional[str] = None, min_size: int = 1, ctx: Optional[Context] = None, method: str = "components",
               assign: str = "first") -> int:
    """Cluster the sketches of one .sig.zip: the set is searched against an index of itself and the hit list becomes a graph
    (Context.cluster: a pair is joined iff its `similarity` — intersect | target_containment | max_containment | jaccard —
    is >= threshold); the clusters are its connected components.  Writes a CSV with the columns cluster, representative,
    size, nodes: one row per cluster of at least min_size members, clusters named Component_<i> by ascending first member,
    `nodes` the member names joined by ';'.  sizes_output: a second CSV, cluster_size,count, over every cluster.
    The format is this project's own, modelled on the output of branchwater's `cluster`; no parity with that tool is
    claimed.  method="greedy": greedy representative clusters instead (Context.cluster_greedy, with `assign` first | best:
    every member is within the threshold of its representative, no two representatives are within it of each other), the
    same columns, clusters named Cluster_<i> by ascending representative.  Returns the number of cluster rows written."""
    if method not in ("components", "greedy"):
        raise ValueError(f"method must be components or greedy, not {method!r}")
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        names, so, sm, sa, sk, ss, smol = read_sig_zip(sig)
        if (sk, ss, smol) != (ksize, scaled, moltype):
            raise ValueError(f"sketch parameters {(sk, ss, smol)} do not match the requested {(ksize, scaled, moltype)}")
        made = []
        try:
            S = ctx.sketches_from_host(so, sm, sa, ksize, scaled, moltype); made.append(S)
            ix = ctx.index_build(S); made.append(ix)
            hits = ctx.search(ix, S); made.append(hits)
            if method == "greedy":
                cl = ctx.cluster_greedy(hits, similarity, threshold, nodes=S, assign=assign); made.append(cl)
            else:
                cl = ctx.cluster(hits, similarity, threshold, nodes=S); made.append(cl)
            _, _, offsets, members, rep = cl.to_host()
        finally:
            for o in reversed(made):
                o.free()
        rows = [r for r in cluster_rows(names, offsets, members, rep, "Cluster" if method == "greedy" else "Component") if r[2] >= min_size]
        with open(output, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(CLUSTER_COLUMNS)
            w.writerows(rows)
        if sizes_output:
            with open(sizes_output, "w", newline="") as f:
                w = csv.writer(f, lineterminator="\n")
                w.writerow(["cluster_size", "count"])
                w.writerows(cluster_size_histogram(offsets))
        return len(rows)
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------
# do_gather()  — search, then per query the greedy non-redundant targets
# ---------------------------------------------------------------------------------------------------------
GATHER_COLUMNS = [
    "query_name", "query_md5", "match_name", "match_md5", "gather_result_rank", "intersect_bp", "unique_intersect_bp",
    "remaining_bp", "f_orig_query", "f_unique_to_query", "f_match", "f_match_orig", "f_unique_weighted", "average_abund",
    "ksize", "scaled", "moltype",
]


def gather_rows(q_names, q_off, q_mins, q_abund, t_names, t_off, t_mins, hits, rank, gathered, ksize: int, scaled: int,
                moltype: str) -> List[dict]:
    """The 17 CSV columns for every row of a Context.gather result, ordered by (query, rank).  hits: its (qid, tid, intersect,
    n_weighted) columns; rank: Hits.best_to_host()[0]; gathered: Hits.gather_to_host() = (unique_intersect, remaining,
    unique_weighted).  The _bp columns are hashes x scaled; every ratio is one f64 division of two integers: f_orig_query =
    intersect / |q|, f_unique_to_query = unique_intersect / |q|, f_match = unique_intersect / |t|, f_match_orig = intersect / |t|,
    f_unique_weighted = unique_weighted / (sum of q's abundances), average_abund = unique_weighted / unique_intersect."""
    qid, tid, isect, _ = hits
    uniq, rem, uw = gathered
    order = np.lexsort((np.asarray(rank), np.asarray(qid)))
    md5_q, md5_t, q_tot = {}, {}, {}
    rows = []
    for r in order.tolist():
        q, t, i, u = int(qid[r]), int(tid[r]), int(isect[r]), int(uniq[r])
        qm = q_mins[int(q_off[q]):int(q_off[q + 1])]
        tm = t_mins[int(t_off[t]):int(t_off[t + 1])]
        nq, nt = len(qm), len(tm)
        if q not in md5_q:
            md5_q[q] = sourmash_md5(qm, ksize)
            q_tot[q] = int(np.asarray(q_abund[int(q_off[q]):int(q_off[q + 1])], np.uint64).sum())
        if t not in md5_t:
            md5_t[t] = sourmash_md5(tm, ksize)
        w = int(uw[r])
        rows.append({
            "query_name": q_names[q], "query_md5": md5_q[q], "match_name": t_names[t], "match_md5": md5_t[t],
            "gather_result_rank": int(rank[r]), "intersect_bp": i * scaled, "unique_intersect_bp": u * scaled,
            "remaining_bp": int(rem[r]) * scaled, "f_orig_query": format_f64(float(i) / float(nq)),
            "f_unique_to_query": format_f64(float(u) / float(nq)), "f_match": format_f64(float(u) / float(nt)),
            "f_match_orig": format_f64(float(i) / float(nt)),
            "f_unique_weighted": format_f64(float(w) / float(q_tot[q]) if q_tot[q] else math.nan),
            "average_abund": format_f64(float(w) / float(u)), "ksize": 3 * ksize, "scaled": scaled, "moltype": moltype,
        })
    return rows


def do_gather(query_sig: str, target_sig: str, output: str, ksize: int, scaled: int, moltype: str, min_unique: int = 1,
              max_results: int = 0, min_containment: float = 0.0, ctx: Optional[Context] = None) -> int:
    """Search every sketch of query_sig (.sig.zip) against every sketch of target_sig (min_containment > 0: only the rows at or
    above that containment are candidates), then per query the greedy non-redundant targets (Context.gather: every target is
    credited only with the hashes no earlier one covered; min_unique, max_results as there).  Writes one CSV row per kept row,
    ordered by (query, rank), with the columns GATHER_COLUMNS (gather_rows has the formulas).  The format is this project's
    own, modelled on the output of branchwater's `fastmultigather`; no parity with that tool is claimed.  Returns the number of
    rows written."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        qn, qo, qm, qa, qk, qs, qmol = read_sig_zip(query_sig)
        tn, to, tm, ta, tk, ts, tmol = read_sig_zip(target_sig)
        for have in ((qk, qs, qmol), (tk, ts, tmol)):
            if have != (ksize, scaled, moltype):
                raise ValueError(f"sketch parameters {have} do not match the requested {(ksize, scaled, moltype)}")
        made = []
        try:
            Q = ctx.sketches_from_host(qo, qm, qa, ksize, scaled, moltype); made.append(Q)
            T = ctx.sketches_from_host(to, tm, ta, ksize, scaled, moltype); made.append(T)
            ix = ctx.index_build(T); made.append(ix)
            hits = ctx.search(ix, Q, min_containment=min_containment); made.append(hits)
            g = ctx.gather(hits, Q, T, min_unique=min_unique, max_results=max_results); made.append(g)
            rows = gather_rows(qn, qo, qm, qa, tn, to, tm, g.to_host(), g.best_to_host()[0], g.gather_to_host(), ksize, scaled,
                               moltype)
        finally:
            for o in reversed(made):
                o.free()
        with open(output, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=GATHER_COLUMNS, lineterminator="\n")
            w.writeheader()
            w.writerows(rows)
        return len(rows)
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------
# k-mer tables and alignment stitching — src/python/kmerseek/sig2kmer.py:186-219, search.py:37-121,195-276
# ---------------------------------------------------------------------------------------------------------
_DAYHOFF = {**{c: "a" for c in "C"}, **{c: "b" for c in "AGPST"}, **{c: "c" for c in "DENQ"}, **{c: "d" for c in "HKR"},
            **{c: "e" for c in "ILMV"}, **{c: "f" for c in "FWY"}}
_HP = {**{c: "h" for c in "AFGILMPVWY"}, **{c: "p" for c in "NCSTDERHKQ"}}


def encode_kmer(kmer: str, moltype: str) -> str:
    """The `encoded` column: residue-wise re-encode (sig2kmer.py:40-58 / src/rust/encoding.rs:67-105)."""
    if moltype in ("protein", "raw"):
        return kmer
    table = _DAYHOFF if moltype == "dayhoff" else _HP
    return "".join(table.get(c, "X") for c in kmer)


def extract_kmers(ctx: Context, records: Sequence[Tuple[str, bytes]], ksize: int, scaled: int, moltype: str,
                  sequence_file: str = "") -> List[dict]:
    """Rows of the reference's k-mer table (sequence_file, sequence_name, kmer, hashval, encoded, start): one per window
    whose hash is in the sequence's sketch.  Positions and hashes come from the GPU (ks_kmer_positions)."""
    from .engine import pack
    res, offs = pack([s for _, s in records])
    seq_i, start, hashes = ctx.kmer_positions(res, offs, ksize, scaled, moltype)
    rows = []
    for s, st, h in zip(seq_i.tolist(), start.tolist(), hashes.tolist()):
        name, seq = records[s]
        kmer = seq[st:st + ksize].decode().upper()
        rows.append({"sequence_file": sequence_file, "sequence_name": name, "kmer": kmer, "hashval": h,
                     "encoded": encode_kmer(kmer, moltype), "start": st})
    return rows


def write_kmers_parquet(rows: List[dict], path: str) -> None:
    import pyarrow as pa
    import pyarrow.parquet as pq
    cols = ["sequence_file", "sequence_name", "kmer", "hashval", "encoded", "start"]
    tab = pa.table({
        "sequence_file": pa.array([r["sequence_file"] for r in rows], pa.string()),
        "sequence_name": pa.array([r["sequence_name"] for r in rows], pa.string()),
        "kmer": pa.array([r["kmer"] for r in rows], pa.string()),
        "hashval": pa.array([r["hashval"] for r in rows], pa.uint64()),
        "encoded": pa.array([r["encoded"] for r in rows], pa.string()),
        "start": pa.array([r["start"] for r in rows], pa.uint32()),
    })
    assert tab.column_names == cols
    pq.write_table(tab, path)


def single_stitch_together_kmers(kmers: Sequence[str], i_kmers: Sequence[int]) -> str:
    """search.py:37-60, quirks included (a zero step re-appends the whole k-mer: kmer[-0:])."""
    stitched = ""
    prev = 0
    for i, (pos, kmer) in enumerate(zip(i_kmers, kmers)):
        if i == 0:
            stitched = kmer
        else:
            step = pos - prev
            stitched += kmer[-step:]
        prev = pos
    return stitched


def stitch_hits(query_kmers: List[dict], target_kmers: List[dict], hit_pairs: Sequence[Tuple[str, str]]) -> List[dict]:
    """search.py:195-240: join query and target k-mers on (encoded, hashval), keep the pairs that are search hits,
    group by match_name, stitch overlapping k-mers into one aligned region per match; rows sorted by (query_start, query_end)."""
    by_key = {}
    for r in target_kmers:
        by_key.setdefault((r["encoded"], r["hashval"]), []).append(r)
    hitset = set(hit_pairs)
    groups = {}
    for q in query_kmers:
        for t in by_key.get((q["encoded"], q["hashval"]), ()):
            if (q["sequence_name"], t["sequence_name"]) in hitset:
                groups.setdefault(t["sequence_name"], []).append(
                    {"query_name": q["sequence_name"], "match_name": t["sequence_name"], "kmer_query": q["kmer"],
                     "kmer_match": t["kmer"], "encoded": q["encoded"], "start_query": q["start"], "start_match": t["start"]})
    out = []
    for match_name, rows in groups.items():
        rows.sort(key=lambda r: r["start_query"])
        # search.py:79-81: the query k-mers are stitched with the MATCH positions (as the reference does)
        query = single_stitch_together_kmers([r["kmer_query"] for r in rows], [r["start_match"] for r in rows])
        alpha = single_stitch_together_kmers([r["encoded"] for r in rows], [r["start_query"] for r in rows])
        match = single_stitch_together_kmers([r["kmer_match"] for r in rows], [r["start_match"] for r in rows])
        assert len(query) == len(alpha) == len(match)
        length = len(query)
        ms = min(r["start_match"] for r in rows)
        qs = min(r["start_query"] for r in rows)
        qn = rows[0]["query_name"]
        out.append({"match_name": match_name, "query_name": qn, "query_start": qs, "query_end": qs + length,
                    "query": query, "match_start": ms, "match_end": ms + length, "match": match, "encoded": alpha,
                    "length": length,
                    "to_print": f"\n---\nQuery Name: {qn}\nMatch Name: {match_name}\nquery: {query} ({qs}-{qs + length})\n"
                                f"alpha: {alpha}\nmatch: {match} ({ms}-{ms + length})"})
    out.sort(key=lambda r: (r["query_start"], r["query_end"]))
    return out


def search_extract_kmers(query_fasta: str, target_fasta: str, ksize: int, scaled: int, moltype: str,
                         ctx: Optional[Context] = None) -> List[dict]:
    """`kmerseek search --extract-kmers QUERY TARGET` end to end: sketch both, search, k-mer tables, stitch."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        from .engine import pack
        q_recs, t_recs = read_fasta(query_fasta), read_fasta(target_fasta)
        Q = ctx.sketch_batch(*pack([s for _, s in q_recs]), ksize, scaled, moltype)
        T = ctx.sketch_batch(*pack([s for _, s in t_recs]), ksize, scaled, moltype)
        qid, tid, _, _ = ctx.search(ctx.index_build(T), Q).to_host()
        pairs = [(q_recs[q][0], t_recs[t][0]) for q, t in zip(qid.tolist(), tid.tolist())]
        qk = extract_kmers(ctx, q_recs, ksize, scaled, moltype, query_fasta)
        tk = extract_kmers(ctx, t_recs, ksize, scaled, moltype, target_fasta)
        return stitch_hits(qk, tk, pairs)
    finally:
        if own:
            ctx.close()


def stitch_match_positions(q_records: Sequence[Tuple[str, bytes]], t_records: Sequence[Tuple[str, bytes]], qid, tid, row_offsets,
                           q_start, t_start, ksize: int, moltype: str) -> List[dict]:
    """The stitched rows of search.py:195-240 from the device's join (Context.match_positions): hit row r = (qid[r], tid[r])
    owns the (query start, target start) pairs [row_offsets[r], row_offsets[r + 1]), ordered by (query start, target start) —
    the order `stitch_hits` reaches by sorting on start_query.  The k-mer strings are sliced from the records; the stitcher's
    quirks (`single_stitch_together_kmers`) apply unchanged.  The device joins on the 64-bit hash alone, the reference on
    (encoded, hashval): the encoded k-mers of every pair are asserted equal here.

    One row per match_name comes out while all hits belong to ONE query, as the reference's group_by("match_name") gives it
    (the case its tests pin).  With several queries the reference would mix the k-mers of different queries that hit the same
    target into one region; here the rows are grouped by (query, match) then."""
    qid = np.asarray(qid).tolist(); tid = np.asarray(tid).tolist()
    offs = np.asarray(row_offsets).tolist()
    qs_all = np.asarray(q_start).tolist(); ts_all = np.asarray(t_start).tolist()
    single_query = len(set(qid)) <= 1
    groups = {}
    for r, (q, t) in enumerate(zip(qid, tid)):
        qn, qseq = q_records[q]
        tn, tseq = t_records[t]
        rows = groups.setdefault(tn if single_query else (qn, tn), [])
        for a, b in zip(qs_all[offs[r]:offs[r + 1]], ts_all[offs[r]:offs[r + 1]]):
            kq = qseq[a:a + ksize].decode().upper()
            kt = tseq[b:b + ksize].decode().upper()
            enc = encode_kmer(kq, moltype)
            assert enc == encode_kmer(kt, moltype), f"hash collision: {kq} ({qn} at {a}) and {kt} ({tn} at {b}) share a hash"
            rows.append({"query_name": qn, "match_name": tn, "kmer_query": kq, "kmer_match": kt, "encoded": enc,
                         "start_query": a, "start_match": b})
    out = []
    for rows in groups.values():
        rows.sort(key=lambda r: r["start_query"])  # (already so inside a hit row; a stable merge where hit rows share a group)
        match_name = rows[0]["match_name"]
        # search.py:79-81: the query k-mers are stitched with the MATCH positions (as the reference does)
        query = single_stitch_together_kmers([r["kmer_query"] for r in rows], [r["start_match"] for r in rows])
        alpha = single_stitch_together_kmers([r["encoded"] for r in rows], [r["start_query"] for r in rows])
        match = single_stitch_together_kmers([r["kmer_match"] for r in rows], [r["start_match"] for r in rows])
        assert len(query) == len(alpha) == len(match)
        length = len(query)
        ms = min(r["start_match"] for r in rows)
        qs = min(r["start_query"] for r in rows)
        qn = rows[0]["query_name"]
        out.append({"match_name": match_name, "query_name": qn, "query_start": qs, "query_end": qs + length,
                    "query": query, "match_start": ms, "match_end": ms + length, "match": match, "encoded": alpha,
                    "length": length,
                    "to_print": f"\n---\nQuery Name: {qn}\nMatch Name: {match_name}\nquery: {query} ({qs}-{qs + length})\n"
                                f"alpha: {alpha}\nmatch: {match} ({ms}-{ms + length})"})
    out.sort(key=lambda r: (r["query_start"], r["query_end"]))
    return out


def read_score_matrix(path: str) -> np.ndarray:
    """A substitution matrix in the NCBI text format (BLOSUM62, PAM250, ...: `#` comment lines, a header line of symbols, then
    one row per symbol: the symbol and one integer per header column) as the int8 [28, 28] array of Context.score_regions: row =
    the query's residue class, column = the target's; classes A..Z -> 0..25, `*` -> 26, everything else -> 27.  Symbols outside
    A-Z and `*` are ignored; every pair the file does not give gets the file's smallest value.  ValueError: no header, a row
    whose value count is not the header's, a value that is not an integer or does not fit int8, a symbol given twice."""
    def cls(sym):
        if len(sym) == 1 and "A" <= sym <= "Z":
            return ord(sym) - ord("A")
        return 26 if sym == "*" else None

    header, seen, given, values = None, set(), {}, []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.split("#", 1)[0].split()
            if not line:
                continue
            if header is None:
                header = line
                if len(set(header)) != len(header):
                    raise ValueError(f"{path}:{no}: a symbol appears twice in the header")
                continue
            sym, cells = line[0], line[1:]
            if len(cells) != len(header):
                raise ValueError(f"{path}:{no}: row {sym!r} holds {len(cells)} values, the header names {len(header)} symbols")
            if sym in seen:
                raise ValueError(f"{path}:{no}: row {sym!r} appears twice")
            seen.add(sym)
            for col, cell in zip(header, cells):
                try:
                    v = int(cell)
                except ValueError:
                    raise ValueError(f"{path}:{no}: {cell!r} is not an integer") from None
                if not -128 <= v <= 127:
                    raise ValueError(f"{path}:{no}: {v} does not fit int8")
                values.append(v)
                if cls(sym) is not None and cls(col) is not None:
                    given[(cls(sym), cls(col))] = v
    if header is None or not values:
        raise ValueError(f"{path}: no matrix rows")
    m = np.full((28, 28), min(values), np.int8)
    for (x, y), v in given.items():
        m[x, y] = v
    return m


def region_rows(q_records: Sequence[Tuple[str, bytes]], t_records: Sequence[Tuple[str, bytes]], qid, tid, regions_host,
                moltype: str, scores=None, alignments=None, cigars=None, cull=None, chain=None, stats=None, pssm=None) -> List[dict]:
    """One row per region of the device's chaining (Context.match_regions; regions_host = Regions.to_host()): hit row
    r = (qid[r], tid[r]) owns regions [row_offsets[r], row_offsets[r + 1]).  The stitched columns of search.py:195-240 —
    query / match / encoded are the residues the region spans, sliced from the records (a region lies on one diagonal, so
    no stitching is left to do) — plus n_kmers and covered.  Where a match is one colinear run the row equals the
    reference's stitched row; where it is not, every run gets a row of its own.  Sorted by (query's place in q_records,
    query_start, query_end).

    scores = RegionScores.to_host() of the same regions (Context.score_regions): the rows are those of the scored — with
    extend=True extended — regions: query_start / query_end, match_start / match_end, query / match / encoded and length span
    the extended region, and the columns score, identities, positives, pident (100 * identities / length) and seed_start /
    seed_length (the original region's query_start and length) are added.

    alignments = RegionAlignments.to_host() of the same regions (Context.align_regions): every row also carries its region's
    gapped alignment — aln_score, aln_q_start / aln_q_end and aln_t_start / aln_t_end (half-open), aln_length (aligned pairs +
    gap residues), aln_identities, aln_positives, aln_mismatches (aligned pairs that are no identity), aln_gap_opens, aln_gaps
    and aln_pident (100 * aln_identities / aln_length).  The other columns, and the order of the rows, do not change.

    cigars = RegionCigars.to_host() of those alignments (Context.trace_regions; needs alignments): every row also carries
    aln_cigar, its alignment's path as text with the query as the read ("35M2D17M1I40M"; = and X for M when traced with eqx).

    cull = RegionCull.to_host() of those alignments — or, without alignments, of those scores (Context.cull_regions; needs one
    of them): only the kept regions give rows, and every row carries aln_rank (0: the best alignment of its hit row) and
    aln_n_merged (the alignments it stands for, itself included) — region_rank and region_n_merged for a cull of scores.  The
    cigars may then be those of all regions or of the kept ones alone (traced from RegionCull.take's objects).  Everything
    else is unchanged; cull=None gives the rows of every region.

    chain = RegionChain.to_host() of those alignments — or, without alignments, of those scores (Context.chain_regions; needs
    one of them): every row also carries chain_pos, its region's place in the colinear chain of its hit row (0: the chain's
    first member), -1 for a region outside the chain.  With cull= as well the chain is that of the objects RegionCull.take
    gave: its src_region indexes the kept regions.  Nothing else changes; chain=None adds no column.

    stats = AlignmentStats.to_host() of those alignments — or, without alignments, of those scores (Context.alignment_stats;
    needs one of them): every row also carries aln_bit_score and aln_evalue (region_bit_score and region_evalue for the
    statistics of scores) and lambda_ratio, the composition-based factor its hit row's scores were rescaled with, as floats.
    With cull= the statistics may be those of all regions or of the kept ones alone.  stats=None adds no column.

    pssm = (RegionAlignments.to_host(), RegionCigars.to_host()) of the KEPT regions aligned and traced against a Profile of the
    queries (Context.align_regions / trace_regions with profile= on RegionCull.take's regions; needs cull): every row also carries
    pssm_score, pssm_identities, pssm_positives, pssm_q_start / pssm_q_end, pssm_t_start / pssm_t_end (half-open) and pssm_cigar.
    pssm=None adds no column."""
    offs, q_start, t_start, length, n_kmers, covered = [np.asarray(c).tolist() for c in regions_host]
    if scores is not None:
        s_offs, s_q, s_t, s_len, s_score, s_ident, s_pos, _ = [np.asarray(c).tolist() for c in scores]
        if s_offs != offs:
            raise ValueError("scores and regions are not of the same hit rows")
    if alignments is not None:
        al = [np.asarray(c).tolist() for c in alignments]
        if al[0] != offs:
            raise ValueError("alignments and regions are not of the same hit rows")
    if cigars is not None:
        if alignments is None:
            raise ValueError("cigars need alignments: they are the paths of alignments")
        from .engine import cigar_strings
        cg = cigar_strings(*cigars)
        if len(cg) != len(q_start) and (cull is None or len(cg) != len(cull[1])):
            raise ValueError("cigars and regions are not of the same regions")
    kept_at = None
    if cull is not None:
        if scores is None and alignments is None:
            raise ValueError("a cull needs scores or alignments: it is made of one of them")
        c_offs, c_src = np.asarray(cull[0]).tolist(), np.asarray(cull[1]).tolist()
        c_rank, c_nm = np.asarray(cull[2]).tolist(), np.asarray(cull[3]).tolist()
        if len(c_offs) != len(offs) or len(cull[4]) != len(q_start):
            raise ValueError("cull and regions are not of the same regions")
        kept_at = {g: i for i, g in enumerate(c_src)}
        rank_col, nm_col = ("aln_rank", "aln_n_merged") if alignments is not None else ("region_rank", "region_n_merged")
        cg_kept = cigars is not None and len(cg) != len(q_start)
    if stats is not None:
        if scores is None and alignments is None:
            raise ValueError("statistics need scores or alignments: they are made of one of them")
        st_ratio, st_bit, st_ev = [np.asarray(stats[i]).tolist() for i in (2, 3, 4)]
        if len(st_ratio) != len(offs) - 1 or (len(st_bit) != len(q_start) and (cull is None or len(st_bit) != len(cull[1]))):
            raise ValueError("statistics and regions are not of the same regions")
        st_kept = len(st_bit) != len(q_start)
        bit_col, ev_col = ("aln_bit_score", "aln_evalue") if alignments is not None else ("region_bit_score", "region_evalue")
    if pssm is not None:
        if cull is None:
            raise ValueError("pssm needs cull: the profile alignments are those of the kept regions")
        from .engine import cigar_strings
        p_al, p_cg = [np.asarray(c).tolist() for c in pssm[0]], cigar_strings(*pssm[1])
        if len(p_cg) != len(c_src) or any(len(c) != len(c_src) for c in p_al[1:]):
            raise ValueError("pssm and cull are not of the same regions")
    chain_pos = None
    if chain is not None:
        if scores is None and alignments is None:
            raise ValueError("a chain needs scores or alignments: it is made of one of them")
        h_offs, h_src = np.asarray(chain[0]).tolist(), np.asarray(chain[1]).tolist()
        if len(h_offs) != len(offs) or len(chain[2]) != (len(q_start) if cull is None else len(c_src)):
            raise ValueError("chain and regions are not of the same regions" if cull is None else
                             "chain and cull are not of the same regions: with a cull the chain is that of the kept regions")
        chain_pos = {}
        for r in range(len(h_offs) - 1):
            for i, k in enumerate(h_src[h_offs[r]:h_offs[r + 1]]):
                chain_pos[k if cull is None else c_src[k]] = i
    out = []
    for r, (q, t) in enumerate(zip(np.asarray(qid).tolist(), np.asarray(tid).tolist())):
        qn, qseq = q_records[q]
        tn, tseq = t_records[t]
        for g in range(offs[r], offs[r + 1]):
            if kept_at is not None and g not in kept_at:
                continue
            a, b, n = (q_start[g], t_start[g], length[g]) if scores is None else (s_q[g], s_t[g], s_len[g])
            query = qseq[a:a + n].decode().upper()
            row = {"match_name": tn, "query_name": qn, "query_start": a, "query_end": a + n, "query": query,
                   "match_start": b, "match_end": b + n, "match": tseq[b:b + n].decode().upper(),
                   "encoded": encode_kmer(query, moltype), "length": n, "n_kmers": n_kmers[g], "covered": covered[g]}
            if scores is not None:
                row.update({"score": s_score[g], "identities": s_ident[g], "positives": s_pos[g],
                            "pident": format_f64(100.0 * float(s_ident[g]) / float(n) if n else math.nan),
                            "seed_start": q_start[g], "seed_length": length[g]})
            if alignments is not None:
                qs_, ql_, ts_, tl_, sc_, id_, po_, go_, ga_, ln_ = [c[g] for c in al[1:]]
                row.update({"aln_score": sc_, "aln_q_start": qs_, "aln_q_end": qs_ + ql_, "aln_t_start": ts_, "aln_t_end": ts_ + tl_,
                            "aln_length": ln_, "aln_identities": id_, "aln_positives": po_, "aln_mismatches": ln_ - ga_ - id_,
                            "aln_gap_opens": go_, "aln_gaps": ga_,
                            "aln_pident": format_f64(100.0 * float(id_) / float(ln_) if ln_ else math.nan)})
                if cigars is not None:
                    row["aln_cigar"] = cg[kept_at[g]] if kept_at is not None and cg_kept else cg[g]
            if kept_at is not None:
                row[rank_col] = c_rank[kept_at[g]]
                row[nm_col] = c_nm[kept_at[g]]
            if chain_pos is not None:
                row["chain_pos"] = chain_pos.get(g, -1)
            if pssm is not None:
                e = kept_at[g]
                row.update({"pssm_score": p_al[5][e], "pssm_identities": p_al[6][e], "pssm_positives": p_al[7][e], "pssm_q_start": p_al[1][e],
                            "pssm_q_end": p_al[1][e] + p_al[2][e], "pssm_t_start": p_al[3][e], "pssm_t_end": p_al[3][e] + p_al[4][e],
                            "pssm_cigar": p_cg[e]})
            if stats is not None:
                e = kept_at[g] if st_kept else g
                row.update({bit_col: st_bit[e], ev_col: st_ev[e], "lambda_ratio": st_ratio[r]})
            out.append((q, row))
    out.sort(key=lambda e: (e[0], e[1]["query_start"], e[1]["query_end"]))
    return [row for _, row in out]


def hit_chain_rows(q_records: Sequence[Tuple[str, bytes]], t_records: Sequence[Tuple[str, bytes]], qid, tid, chain_host,
                   stitched=None, stats=None) -> List[dict]:
    """One row per hit row that has a chain (chain_host = RegionChain.to_host(); hit row r = (qid[r], tid[r])): what the
    alignments of the hit say together.  query_name, match_name, chain_score, n_alns (the chain's members), query_start /
    query_end and match_start / match_end (the chain's span, half-open), q_aligned and t_aligned (the positions its members
    cover), qcov and tcov (their share of the whole sequences) and pident (100 * identities / aln_length summed over the
    members, NaN where the chain was made without those columns).  Sorted by (query's place in q_records, -chain_score,
    target's place in t_records).
    stitched = HitAlignments.to_host() of that chain (Context.stitch_chains): every row also carries the ONE gapped alignment
    the chain was stitched into — aln_cigar (text, the query as the read), aln_score, aln_identities, aln_positives,
    aln_gap_opens, aln_gaps, aln_length, aln_pident (100 * identities / aln_length of that alignment: no column is counted
    twice) — and n_filled / n_open, the links between the chain's members that were aligned / left open.  stitched=None adds
    no column.
    stats = AlignmentStats.to_host() of those stitched alignments (Context.alignment_stats; needs stitched): every row also
    carries aln_bit_score and aln_evalue, as floats.  stats=None adds no column."""
    if stats is not None:
        if stitched is None:
            raise ValueError("statistics need stitched: they are those of the stitched alignments")
        st_bit, st_ev = np.asarray(stats[3]).tolist(), np.asarray(stats[4]).tolist()
        if len(st_bit) != len(np.asarray(qid)):
            raise ValueError("statistics and hits are not of the same hit rows")
    st = None
    if stitched is not None:
        from .engine import cigar_strings
        st = [np.asarray(c).tolist() for c in stitched]
        if len(st[0]) != len(np.asarray(chain_host[0])) or any(len(c) != len(st[0]) - 1 for c in st[2:]):
            raise ValueError("stitched alignments and chain are not of the same hit rows")
        st_cigar = cigar_strings(stitched[0], stitched[1])
    cols = [np.asarray(c).tolist() for c in chain_host]
    offs, score, qs, ql, ts, tl, qa, ta, ident, alen = [cols[i] for i in (0, 4, 5, 6, 7, 8, 9, 10, 11, 12)]
    qid, tid = np.asarray(qid).tolist(), np.asarray(tid).tolist()
    if len(offs) != len(qid) + 1 or len(qid) != len(tid):
        raise ValueError("chain and hits are not of the same hit rows")
    out = []
    for r, (q, t) in enumerate(zip(qid, tid)):
        n = offs[r + 1] - offs[r]
        if n == 0:
            continue
        (qn, qseq), (tn, tseq) = q_records[q], t_records[t]
        out.append((q, -score[r], t, {
            "query_name": qn, "match_name": tn, "chain_score": score[r], "n_alns": n,
            "query_start": qs[r], "query_end": qs[r] + ql[r], "match_start": ts[r], "match_end": ts[r] + tl[r],
            "q_aligned": qa[r], "t_aligned": ta[r],
            "qcov": format_f64(float(qa[r]) / float(len(qseq)) if len(qseq) else math.nan),
            "tcov": format_f64(float(ta[r]) / float(len(tseq)) if len(tseq) else math.nan),
            "pident": format_f64(100.0 * float(ident[r]) / float(alen[r]) if alen[r] else math.nan)}))
        if st is not None:
            out[-1][3].update({
                "aln_cigar": st_cigar[r], "aln_score": st[6][r], "aln_identities": st[7][r], "aln_positives": st[8][r],
                "aln_gap_opens": st[9][r], "aln_gaps": st[10][r], "aln_length": st[11][r],
                "aln_pident": format_f64(100.0 * float(st[7][r]) / float(st[11][r]) if st[11][r] else math.nan),
                "n_filled": st[13][r], "n_open": st[14][r]})
            if stats is not None:
                out[-1][3].update({"aln_bit_score": st_bit[r], "aln_evalue": st_ev[r]})
    out.sort(key=lambda e: e[:3])
    return [row for *_, row in out]


def coverage_rows(records: Sequence[Tuple[str, bytes]], pileup_host) -> List[dict]:
    """One row per sequence of the batch a Pileup was made on (pileup_host = Pileup.to_host(), records: that batch's, in its
    order): name, length, n_alignments (the alignments with a pair column on it), covered (positions with depth > 0), breadth
    (covered / length), depth_sum, mean_depth (depth_sum / length) and max_depth — the breadth-of-coverage table of a read-to-
    protein pipeline.  The two quotients are the device's f64 as text (NaN for an empty sequence).  In batch order."""
    length, n_aln, covered, max_depth, depth_sum, breadth, mean_depth = [np.asarray(c).tolist() for c in pileup_host[2:9]]
    if len(length) != len(records):
        raise ValueError(f"the pileup is of {len(length)} sequences, the records are {len(records)}")
    return [{"name": name, "length": length[s], "n_alignments": n_aln[s], "covered": covered[s], "breadth": format_f64(breadth[s]),
             "depth_sum": depth_sum[s], "mean_depth": format_f64(mean_depth[s]), "max_depth": max_depth[s]}
            for s, (name, _) in enumerate(records)]


PROFILE_WEIGHTINGS = (None, "henikoff")  # profile_weighting= of search_extract_kmers_device


def _coverage_check(coverage, allowed, needs) -> None:
    """coverage= of the two searches: one of `allowed`, and every (name, on) of `needs` switched on."""
    if coverage not in allowed:
        raise ValueError(f"coverage = {coverage!r} is none of " + ", ".join(repr(a) for a in allowed))
    if coverage:
        for name, on in needs:
            if not on:
                raise ValueError(f"coverage needs {name}=True: it is piled up from traced alignments")


def search_extract_kmers_device(query_fasta: str, target_fasta: str, ksize: int, scaled: int, moltype: str,
                                ctx: Optional[Context] = None, regions: bool = False, max_gap: int = 0,
                                min_kmers: int = 1, score: bool = False, extend: bool = False, x_drop: int = 0,
                                matrix=None, gapped: bool = False, band: int = 16, gap_open: int = 11, gap_extend: int = 1,
                                gapped_x_drop: int = 30, cigar: bool = False, eqx: bool = False, cull: bool = False,
                                cull_overlap: int = 100, min_aln_score=None, max_alns: int = 0, chain: bool = False,
                                chain_max_gap: int = 0, chain_max_overlap: int = 0, chain_link_cost: int = 0,
                                chain_skew_cost: int = 0, chain_overlap_cost: int = 0, hit_rows: bool = False,
                                stitch: bool = False, stitch_max_fill: int = 0, evalue: bool = False, stat_params=None,
                                max_evalue=None, mask: bool = False, mask_opts: Optional[dict] = None, coverage: Optional[str] = None,
                                profile: bool = False, profile_beta: float = 10.0, profile_weighting: Optional[str] = None):
    """`kmerseek search --extract-kmers QUERY TARGET` with the k-mer join on the device: sketch both, search, k-mer position
    tables (left on the GPU), ks_match_positions, then only the pairs of the hit rows come to the host to be stitched.
    Same rows as `search_extract_kmers`.  regions=True: the pairs are chained on the device too (ks_match_regions with
    max_gap / min_kmers) and only the regions come to the host: the rows of `region_rows`, one per colinear run.
    score=True (needs regions=True): the regions are scored on the device too (Context.score_regions with matrix, extend and
    x_drop) and the rows carry the columns `region_rows` adds for scores.
    gapped=True (needs regions=True): every region is aligned with gaps on the device (Context.align_regions with matrix, band,
    gap_open, gap_extend and gapped_x_drop) and the rows carry the aln_* columns `region_rows` adds for alignments.
    cigar=True (needs gapped=True): the alignments are traced back on the device too (Context.trace_regions, with eqx) and the
    rows carry aln_cigar.
    cull=True (needs gapped=True or score=True): redundant regions are culled per hit on the device (Context.cull_regions with
    cull_overlap, min_aln_score and max_alns) — the alignments with gapped=True, otherwise the scored regions — and only the
    kept ones give rows, with the rank and n_merged columns `region_rows` adds for a cull.  With cigar=True only the kept
    alignments are traced.
    chain=True (needs gapped=True or score=True): the alignments (with gapped=True, otherwise the scored regions) of each hit
    are chained on the device (Context.chain_regions with the chain_* options) — those the cull kept with cull=True — and the
    rows carry chain_pos.  hit_rows=True (needs chain=True): the rows of `hit_chain_rows`, one per hit, instead.
    stitch=True (needs gapped=True, cigar=True, chain=True and hit_rows=True): each hit's chain is stitched into one gapped
    alignment on the device (Context.stitch_chains with stitch_max_fill and eqx) and the hit rows carry the aln_* columns
    `hit_chain_rows` adds for stitched=.
    evalue=True (needs gapped=True or score=True; with hit_rows=True also stitch=True): the residue compositions of both files
    are counted on the device and the scores — the stitched alignments', else the alignments', else the scored regions' — get
    bit scores and E-values (Context.alignment_stats with matrix; the database is the target file) and the rows carry the
    columns `region_rows` / `hit_chain_rows` add for stats=.  stat_params = (lambda, K): the gapped parameters that belong to
    the matrix and the gap costs — gapped scores need them; None for scored regions: the ungapped ones the library derives.
    max_evalue: rows whose E-value is above it are dropped, on the host.
    mask=True: both files are sketched with their low-complexity stretches left out (Context.sketch_masked; mask_opts: its
    window / k1 / k2 keywords) and the position tables are made of the same windows (Context.kmer_positions_table_masked):
    hits, pairs and regions are those of the unmasked windows.  The passes that read residues (scores, alignments) read the
    records as they are.
    coverage="query" | "target" (needs cigar=True): the alignments are piled up on that file's sequences on the device
    (Context.pileup) — the stitched ones with stitch=True, otherwise the traced alignments of the kept regions — and the call
    returns (rows, coverage_rows): the rows as before and one `coverage_rows` row per sequence of that file.  max_evalue drops
    rows on the host and does not touch the coverage.
    profile=True (needs regions, gapped, cigar and cull; not with stitch, evalue or coverage): a second round against a
    position-specific matrix.  The traced alignments of the kept regions are piled up on the queries with their residue counts
    (Context.pileup, profile=True), the counts become a Profile (Context.build_profile with profile_params(matrix,
    beta=profile_beta)), the kept regions are aligned and traced again against it, and the rows carry the pssm_* columns
    `region_rows` adds for pssm=.
    profile_weighting="henikoff" (needs profile=True): the alignments are weighted before they are counted, so that many
    near-copies of one homolog say one thing once.  The profile is then made in four steps: the unweighted pileup, one
    position-based weight per alignment from its counts (Context.entry_weights, include_query=True), the pileup again under
    those weights (Context.pileup, weights=) and the weighted build (Context.build_profile, weighted=True).  The pssm_*
    columns keep their names.  None: every alignment counts once, as before."""
    if profile_weighting not in PROFILE_WEIGHTINGS:
        raise ValueError(f"profile_weighting = {profile_weighting!r} is none of {', '.join(repr(w) for w in PROFILE_WEIGHTINGS)}")
    if profile_weighting is not None and not profile:
        raise ValueError(f"profile_weighting = {profile_weighting!r} needs profile=True: it weights the alignments the profile is built from")
    _coverage_check(coverage, (None, "query", "target"), (("cigar", cigar),))
    if profile:
        for name, on in (("regions", regions), ("gapped", gapped), ("cigar", cigar), ("cull", cull)):
            if not on:
                raise ValueError(f"profile=True needs {name}=True: the profile is built from the traced alignments the cull kept")
        for name, on in (("stitch", stitch), ("evalue", evalue), ("coverage", coverage)):
            if on:
                raise ValueError(f"profile=True with {name}: not built (stitch, E-values and coverage read residues under a matrix)")
    if not profile_beta >= 0:
        raise ValueError(f"profile_beta = {profile_beta} is not a weight >= 0")
    if mask_opts is not None and not mask:
        raise ValueError("mask_opts needs mask=True")
    if (stat_params is not None or max_evalue is not None) and not evalue:
        raise ValueError("stat_params and max_evalue need evalue=True")
    if evalue:
        if not (gapped or score):
            raise ValueError("evalue=True needs gapped=True or score=True: statistics are of scores")
        if hit_rows and not stitch:
            raise ValueError("evalue=True with hit_rows=True needs stitch=True: a chain with open links has no one score")
        if gapped and stat_params is None:
            raise ValueError("evalue=True with gapped=True needs stat_params=(lambda, K), the gapped parameters of the matrix and gap costs")
    if stitch:
        for name, on in (("gapped", gapped), ("cigar", cigar), ("chain", chain), ("hit_rows", hit_rows)):
            if not on:
                raise ValueError(f"stitch=True needs {name}=True: a stitched alignment is made of the traced alignments of a hit's chain "
                                 "and is a column set of the hit rows")
    if chain and not (gapped or score):
        raise ValueError("chain=True needs gapped=True or score=True: a chain is made of alignments or of scored regions")
    if hit_rows and not chain:
        raise ValueError("hit_rows=True needs chain=True: the rows are those of the hits' chains")
    if cull and not (gapped or score):
        raise ValueError("cull=True needs gapped=True or score=True: a cull is made of alignments or of scored regions")
    if score and not regions:
        raise ValueError("score=True needs regions=True: scores are of regions")
    if gapped and not regions:
        raise ValueError("gapped=True needs regions=True: alignments are of regions")
    if cigar and not gapped:
        raise ValueError("cigar=True needs gapped=True: CIGARs are of gapped alignments")
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        from .engine import pack
        q_recs, t_recs = read_fasta(query_fasta), read_fasta(target_fasta)
        q_res, q_off = pack([s for _, s in q_recs])
        t_res, t_off = pack([s for _, s in t_recs])
        if mask:
            mo = mask_opts or {}
            Q = ctx.sketch_masked(q_res, q_off, ksize, scaled, moltype, **mo)
            T = ctx.sketch_masked(t_res, t_off, ksize, scaled, moltype, **mo)
        else:
            Q = ctx.sketch_batch(q_res, q_off, ksize, scaled, moltype)
            T = ctx.sketch_batch(t_res, t_off, ksize, scaled, moltype)
        hits = ctx.search(ctx.index_build(T), Q)
        if mask:
            qp = ctx.kmer_positions_table_masked(q_res, q_off, ksize, scaled, moltype, **mo)
            tp = ctx.kmer_positions_table_masked(t_res, t_off, ksize, scaled, moltype, **mo)
        else:
            qp = ctx.kmer_positions_table(q_res, q_off, ksize, scaled, moltype)
            tp = ctx.kmer_positions_table(t_res, t_off, ksize, scaled, moltype)
        mp = ctx.match_positions(qp, tp, hits)
        qid, tid, _, _ = hits.to_host()
        if regions:
            rg = ctx.match_regions(mp, max_gap=max_gap, min_kmers=min_kmers)
            rg_host = rg.to_host()
            sc_host = cg_host = cu = cov_rows = None
            kw = {}

            def covered(aligned, **more):  # coverage=: the rows of the side's file
                pu = ctx.pileup(aligned, hits, side=coverage, offsets=q_off if coverage == "query" else t_off, **more)
                host = pu.to_host()
                pu.free()
                return coverage_rows(q_recs if coverage == "query" else t_recs, host)
            if evalue:
                q_comp, t_comp = ctx.residue_composition(q_res, q_off), ctx.residue_composition(t_res, t_off)

                def stats_of(obj, **more):
                    s = ctx.alignment_stats(obj, hits, q_comp, t_comp, matrix=matrix, params=stat_params, **more)
                    host = s.to_host()
                    s.free()
                    return host

            def chained(obj):  # the chain of obj, or of what the cull kept of it
                kept = cu.take(obj) if cu is not None else obj
                ch = ctx.chain_regions(kept, max_gap=chain_max_gap, max_overlap=chain_max_overlap, link_cost=chain_link_cost,
                                       skew_cost=chain_skew_cost, overlap_cost=chain_overlap_cost)
                host = ch.to_host()
                ch.free()
                if kept is not obj:
                    kept.free()
                return host
            if score:
                sc = ctx.score_regions(rg, hits, q_res, q_off, t_res, t_off, matrix=matrix, extend=extend, x_drop=x_drop)
                sc_host = sc.to_host()
                if cull and not gapped:
                    cu = ctx.cull_regions(sc, overlap_pct=cull_overlap, min_score=min_aln_score, max_per_row=max_alns)
                if chain and not gapped:
                    kw["chain"] = chained(sc)
                if evalue and not gapped:
                    kw["stats"] = stats_of(sc)
                sc.free()
            if gapped:
                al = ctx.align_regions(rg, hits, q_res, q_off, t_res, t_off, matrix=matrix, band=band, gap_open=gap_open,
                                       gap_extend=gap_extend, x_drop=gapped_x_drop)
                al_host = al.to_host()
                if cull:
                    cu = ctx.cull_regions(al, overlap_pct=cull_overlap, min_score=min_aln_score, max_per_row=max_alns)
                if stitch:  # the kept alignments, their paths and their chain stay on the device until they are stitched
                    t_rg, t_al = (cu.take(rg), cu.take(al)) if cull else (rg, al)
                    cg = ctx.trace_regions(t_rg, hits, q_res, q_off, t_res, t_off, t_al, eqx=eqx)
                    ch = ctx.chain_regions(t_al, max_gap=chain_max_gap, max_overlap=chain_max_overlap, link_cost=chain_link_cost,
                                           skew_cost=chain_skew_cost, overlap_cost=chain_overlap_cost)
                    st = ctx.stitch_chains(ch, t_al, cg, hits, q_res, q_off, t_res, t_off, max_fill=stitch_max_fill, eqx=eqx)
                    kw["chain"], st_host = ch.to_host(), st.to_host()
                    if coverage:
                        cov_rows = covered(st)
                    if evalue:
                        kw["stats"] = stats_of(st, alignments=t_al)
                    for o in (st, ch, cg) + ((t_rg, t_al) if cull else ()):
                        o.free()
                elif cigar:
                    t_rg, t_al = (cu.take(rg), cu.take(al)) if cull else (rg, al)  # (trace what is kept, not everything)
                    cg = ctx.trace_regions(t_rg, hits, q_res, q_off, t_res, t_off, t_al, eqx=eqx)
                    cg_host = cg.to_host()
                    if coverage:
                        cov_rows = covered(cg, alignments=t_al)
                    if profile:  # round two: the kept alignments say what each query position likes
                        from .engine import profile_params
                        pu = ctx.pileup(cg, hits, side="query", offsets=q_off, alignments=t_al, profile=True, other_res=t_res, other_off=t_off)
                        if profile_weighting == "henikoff":
                            ew = ctx.entry_weights(cg, hits, pu, side="query", offsets=q_off, alignments=t_al, other_res=t_res, other_off=t_off,
                                                   include_query=True, res=q_res)
                            pu.free()
                            pu = ctx.pileup(cg, hits, side="query", offsets=q_off, alignments=t_al, profile=True, other_res=t_res, other_off=t_off,
                                            weights=ew)
                            ew.free()
                        pf = ctx.build_profile(pu, q_res, q_off, profile_params(matrix, beta=profile_beta), weighted=profile_weighting is not None)
                        p_al = ctx.align_regions(t_rg, hits, q_res, q_off, t_res, t_off, profile=pf, band=band, gap_open=gap_open,
                                                 gap_extend=gap_extend, x_drop=gapped_x_drop)
                        p_cg = ctx.trace_regions(t_rg, hits, q_res, q_off, t_res, t_off, p_al, eqx=eqx, profile=pf)
                        kw["pssm"] = (p_al.to_host(), p_cg.to_host())
                        for o in (p_cg, p_al, pf, pu):
                            o.free()
                    cg.free()
                    if cull:
                        t_rg.free(); t_al.free()
                if chain and not stitch:
                    kw["chain"] = chained(al)
                if evalue and not stitch:
                    kw["stats"] = stats_of(al)
                al.free()
            if cu is not None:
                kw["cull"] = cu.to_host()
                cu.free()
            if evalue:
                q_comp.free(); t_comp.free()
            for o in (rg, mp, qp, tp, hits, Q, T):
                o.free()

            def below(rows):  # max_evalue: on the host
                if max_evalue is not None:
                    col = "aln_evalue" if gapped else "region_evalue"
                    rows = [row for row in rows if not row[col] > max_evalue]
                return (rows, cov_rows) if coverage else rows
            if stitch:
                return below(hit_chain_rows(q_recs, t_recs, qid, tid, kw["chain"], stitched=st_host, stats=kw.get("stats")))
            if hit_rows:
                rows = hit_chain_rows(q_recs, t_recs, qid, tid, kw["chain"])
                return (rows, cov_rows) if coverage else rows
            if gapped:
                if cigar:
                    return below(region_rows(q_recs, t_recs, qid, tid, rg_host, moltype, scores=sc_host, alignments=al_host, cigars=cg_host, **kw))
                return below(region_rows(q_recs, t_recs, qid, tid, rg_host, moltype, scores=sc_host, alignments=al_host, **kw))
            return below(region_rows(q_recs, t_recs, qid, tid, rg_host, moltype, scores=sc_host, **kw))
        offs, qs, ts = mp.to_host()[:3]
        for o in (mp, qp, tp, hits, Q, T):
            o.free()
        return stitch_match_positions(q_recs, t_recs, qid, tid, offs, qs, ts, ksize, moltype)
    finally:
        if own:
            ctx.close()


def frame_chain_rows(nt_records: Sequence[Tuple[str, bytes]], t_records: Sequence[Tuple[str, bytes]], fold_hits_host, fold_host,
                     chain_host, keep_rows=None, stitched=None) -> List[dict]:
    """One row per folded row of a translated search that has a chain: where on the nucleotide record the protein lies, on which
    strand and in which frames.  fold_hits_host = FrameFold.hits.to_host() (qid = 2 * record + strand), fold_host =
    FrameFold.to_host(), chain_host = RegionChain.to_host() of Context.chain_frames on that fold.  Columns: query_name, strand
    (+ / -), match_name, nt_start / nt_end (on the record as given, 0-based half-open: for - they are L - (the chain's q_start +
    q_length) and L - q_start), t_start / t_end (residues: the chain's values over 3), chain_score, n_alns, frames (the members'
    frames in chain order in BLAST's numbering, +1 .. +3 and -1 .. -3, comma-joined), n_frameshifts (consecutive members whose
    frames differ), identities, aln_length, pident (100 * identities / aln_length, NaN where the fold had no such columns) and
    intersect_hashes (the shared hashes of the member frame rows, summed).  keep_rows: the folded rows to report (None: all).
    stitched = FrameAlignments.to_host() of Context.stitch_frames on that chain: every row also carries the one alignment of the
    strand's bases against the protein — aln_cigar (codon columns; N: skipped bases), aln_score, aln_identities, aln_positives,
    aln_gap_opens, aln_gaps, aln_length, aln_pident, n_filled, n_open (aln_length then CHANGES its meaning: it is the column count of
    that one alignment, no longer the members' sum, so that aln_pident = 100 * aln_identities / aln_length; identities and pident
    stay the members' sums and their ratio to the members' lengths) — and aln_frameshifts, the places of its N ops on the record
    as given as a comma-joined list of nt_pos:len (the first skipped base on the record, 0-based, and the bases skipped).  Without
    it the rows are what they were.  Sorted by (record, strand, -chain_score, target)."""
    qid, tid, isect = [np.asarray(c).tolist() for c in fold_hits_host[:3]]
    frame = np.asarray(fold_host[3]).tolist()
    cols = [np.asarray(c).tolist() for c in chain_host]
    offs, src, score, qs, ql, ts, tl, ident, alen = [cols[i] for i in (0, 1, 4, 5, 6, 7, 8, 11, 12)]
    if len(offs) != len(qid) + 1 or len(qid) != len(tid) or len(np.asarray(fold_host[1])) != len(offs):
        raise ValueError("chain, fold and folded hits are not of the same rows")
    keep = None if keep_rows is None else set(np.asarray(keep_rows).tolist())
    if stitched is not None:
        st = [np.asarray(c).tolist() for c in stitched]
        if len(st[0]) != len(offs) or any(len(c) != len(qid) for c in st[2:]):
            raise ValueError("stitched alignments and chain are not of the same rows")
        from .engine import cigar_strings
        st_text = cigar_strings(st[0], st[1])
    out = []
    for r, (x, t) in enumerate(zip(qid, tid)):
        n = offs[r + 1] - offs[r]
        if n == 0 or (keep is not None and r not in keep):
            continue
        s, minus = x // 2, x % 2 == 1
        (qn, qseq), (tn, _) = nt_records[s], t_records[t]
        L, a, e = len(qseq), qs[r], qs[r] + ql[r]
        fr = [frame[g] for g in src[offs[r]:offs[r + 1]]]
        more = {}
        if stitched is not None:
            p, shifts = st[2][r], []  # the strand position of the next column
            for v in st[1][st[0][r]:st[0][r + 1]]:
                k, c = v >> 4, v & 15
                if c == 3:
                    shifts.append(f"{L - p - k if minus else p}:{k}")
                    p += k
                elif c != 2:
                    p += 3 * k
            more = {"aln_cigar": st_text[r], "aln_score": st[7][r], "aln_identities": st[8][r], "aln_positives": st[9][r], "aln_gap_opens": st[10][r],
                    "aln_gaps": st[11][r], "aln_length": st[12][r],
                    "aln_pident": format_f64(100.0 * float(st[8][r]) / float(st[12][r]) if st[12][r] else math.nan),
                    "n_filled": st[14][r], "n_open": st[15][r], "aln_frameshifts": ",".join(shifts)}
        out.append((s, minus, -score[r], t, {
            "query_name": qn, "strand": "-" if minus else "+", "match_name": tn,
            "nt_start": L - e if minus else a, "nt_end": L - a if minus else e, "t_start": ts[r] // 3, "t_end": (ts[r] + tl[r]) // 3,
            "chain_score": score[r], "n_alns": n, "frames": ",".join(f"{'-' if f >= 3 else '+'}{f % 3 + 1}" for f in fr),
            "n_frameshifts": sum(1 for u, v in zip(fr, fr[1:]) if u != v), "identities": ident[r], "aln_length": alen[r],
            "pident": format_f64(100.0 * float(ident[r]) / float(alen[r]) if alen[r] else math.nan), "intersect_hashes": isect[r], **more}))
    out.sort(key=lambda e: e[:4])
    return [row for *_, row in out]


def search_translated_device(nt_fasta: str, protein_fasta: str, ksize: int, scaled: int, moltype: str, ctx: Optional[Context] = None,
                             matrix=None, extend: bool = True, x_drop: int = 20, gapped: bool = False, band: int = 16,
                             gap_open: int = 11, gap_extend: int = 1, gapped_x_drop: int = 30, cull: bool = True,
                             cull_overlap: int = 100, max_gap: int = 0, min_kmers: int = 1, chain_max_gap: int = 0,
                             chain_max_overlap: int = 0, chain_link_cost: int = 0, chain_skew_cost: int = 0,
                             chain_overlap_cost: int = 0, top_k: int = 0, cigar: bool = False, eqx: bool = False, stitch: bool = False,
                             max_fill: int = 0, frameshift_cost: int = 15, coverage: bool = False):
    """Translated search to the end, on the device: the records of a nucleotide FASTA against the proteins of a protein FASTA,
    the rows of `frame_chain_rows` — per (record, strand, protein) where the gene lies in bases, in which frames, and whether a
    frameshift joins two of them.  The records are translated in six frames (Context.translate6), the frames sketched
    (ksize, scaled, moltype: the protein sketch parameters) and searched against the index of the proteins; position tables of
    frames and proteins, match_positions and match_regions (max_gap, min_kmers) give each frame hit its regions, which are scored
    and extended without gaps (matrix, extend, x_drop) or, with gapped=True, aligned with gaps (matrix, band, gap_open,
    gap_extend, gapped_x_drop) with the frames as the query residues; cull=True removes redundant ones (cull_overlap);
    Context.fold_frames folds the frame rows per strand and Context.chain_frames chains their regions in bases (the chain_*
    options are in bases).  top_k > 0 keeps per (record, strand) the k proteins with the best chain score (Context.best_hits on
    the folded hits).  cigar=True says that paths may be traced; alone it adds nothing to the rows and costs nothing.
    stitch=True (needs gapped=True and cigar=True) traces the kept alignments (eqx: = / X for M), stitches every
    chain into ONE alignment of the strand's bases against the protein (Context.stitch_frames: max_fill, frameshift_cost), adds
    its columns to the rows (frame_chain_rows with stitched=) and ranks top_k by that alignment's score instead of the chain
    score.
    coverage=True (needs stitch=True): the stitched alignments are piled up on the proteins on the device (Context.pileup,
    target side; with top_k only those of the kept rows, through the row mask) and the call returns (rows, coverage_rows): one
    `coverage_rows` row per protein.  Every device object made on the way is freed."""
    _coverage_check(coverage, (False, True), (("stitch", stitch),))
    if stitch:
        for name, on in (("gapped", gapped), ("cigar", cigar)):
            if not on:
                raise ValueError(f"stitch=True needs {name}=True: a stitched alignment is made of the traced alignments of a strand's chain")
    if cigar and not gapped:
        raise ValueError("cigar=True needs gapped=True: CIGARs are of gapped alignments")
    if eqx and not cigar:
        raise ValueError("eqx=True needs cigar=True: = and X are ops of a CIGAR")
    own = ctx is None
    ctx = ctx or Context(0)
    made = []

    def keep(o):
        made.append(o)
        return o
    try:
        nt_recs, t_recs = read_fasta(nt_fasta), read_fasta(protein_fasta)
        nt, nt_off = pack([s for _, s in nt_recs])
        t_res, t_off = pack([s for _, s in t_recs])
        n6, n_t = 6 * len(nt_recs), len(t_recs)
        frames, foff, n_res = ctx.translate6(nt, nt_off)
        keep(frames); keep(foff)
        Q = keep(ctx.sketch_batch_device(frames.ptr, foff.ptr, n6, n_res, ksize, scaled, moltype))
        T = keep(ctx.sketch_batch(t_res, t_off, ksize, scaled, moltype))
        ix = keep(ctx.index_build(T))
        hits = keep(ctx.search(ix, Q))
        qp = keep(ctx.kmer_positions_table_device(frames.ptr, foff.ptr, n6, n_res, ksize, scaled, moltype))
        tp = keep(ctx.kmer_positions_table(t_res, t_off, ksize, scaled, moltype))
        mp = keep(ctx.match_positions(qp, tp, hits))
        rg = keep(ctx.match_regions(mp, max_gap=max_gap, min_kmers=min_kmers))
        d_t = keep(ctx.to_device(t_res if len(t_res) else np.zeros(16, np.uint8)))
        d_to = keep(ctx.to_device(t_off))
        batches = (frames.ptr, foff.ptr, n6, n_res, d_t.ptr, d_to.ptr, n_t, len(t_res))
        if gapped:
            sc = keep(ctx.align_regions_device(rg, hits, *batches, matrix=matrix, band=band, gap_open=gap_open, gap_extend=gap_extend,
                                               x_drop=gapped_x_drop))
        else:
            sc = keep(ctx.score_regions_device(rg, hits, *batches, matrix=matrix, extend=extend, x_drop=x_drop))
        kept, kept_rg = sc, rg
        if cull:
            cu = keep(ctx.cull_regions(sc, overlap_pct=cull_overlap))
            kept = keep(cu.take(sc))
            if stitch:
                kept_rg = keep(cu.take(rg))
        fold = keep(ctx.fold_frames(hits, kept, nt_off))
        chain = keep(ctx.chain_frames(fold, max_gap=chain_max_gap, max_overlap=chain_max_overlap, link_cost=chain_link_cost,
                                      skew_cost=chain_skew_cost, overlap_cost=chain_overlap_cost))
        stitched = None
        if stitch:  # (cigar=True alone traces nothing: the members' own CIGARs are not columns of these rows)
            cg = keep(ctx.trace_regions_device(kept_rg, hits, *batches, kept, eqx=eqx))
            stitched = keep(ctx.stitch_frames_device(fold, chain, kept, cg, *batches, max_fill=max_fill, eqx=eqx, frameshift_cost=frameshift_cost))
        keep_rows = None
        if top_k:
            best = keep(ctx.best_hits(fold.hits, k=top_k, score=stitched.row_score_ptr if stitch else chain.row_chain_score_ptr))
            keep_rows = best.best_to_host()[1]
        rows = frame_chain_rows(nt_recs, t_recs, fold.hits.to_host(), fold.to_host(), chain.to_host(), keep_rows=keep_rows,
                                stitched=stitched.to_host() if stitch else None)
        if not coverage:
            return rows
        row_mask = None
        if keep_rows is not None:
            row_mask = np.zeros(fold.hits.count, np.uint8)
            row_mask[np.asarray(keep_rows, dtype=np.int64)] = 1
        pu = keep(ctx.pileup(stitched, fold.hits, side="target", offsets=t_off, row_mask=row_mask))
        return rows, coverage_rows(t_recs, pu.to_host())
    finally:
        for o in reversed(made):
            o.free()
        if own:
            ctx.close()
