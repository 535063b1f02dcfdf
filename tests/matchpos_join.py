"""CPU restatement of ks_match_positions for the tests, built from what oracle/oracle.py offers: the sketches
(`sketch_batch`), the k-mer position table of every sequence (`kmer_positions`), the hit rows (`manysearch`), and a numpy
join of the two tables on the hash restricted to the hit rows.  Not a test module."""
import numpy as np

from oracle import oracle


def seqs_of(res, offs):
    return [bytes(res[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]


def position_table(res, offs, k, scaled, mol, sk=None):
    """(seq u32, start u32, hash u64) of every kept window, ordered by (seq, start) — what ks_kmer_positions leaves."""
    so, sm, _ = sk if sk is not None else oracle.sketch_batch(res, offs, k, scaled, mol, n_threads=4)
    seq, start, hashes = [], [], []
    for i, s in enumerate(seqs_of(res, offs)):
        st, hh = oracle.kmer_positions(s.upper(), k, mol, sm[int(so[i]):int(so[i + 1])])
        seq.append(np.full(len(st), i, np.uint32)); start.append(st); hashes.append(hh)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(seq, np.uint32), cat(start, np.uint32), cat(hashes, np.uint64)


def filter_hits(hits, q_sk_offs, min_containment):
    """The rows a search with min_containment keeps: (double)intersect / (double)|q| >= min_containment."""
    qid, tid, isect, nw = hits
    nq = (q_sk_offs[1:] - q_sk_offs[:-1]).astype(np.float64)[qid]
    keep = isect.astype(np.float64) / nq >= min_containment
    return qid[keep], tid[keep], isect[keep], nw[keep]


def join(q_tab, t_tab, hit_qid, hit_tid, ksize):
    """-> (row_offsets u64[n+1], q_start, t_start, q_lo, q_hi, t_lo, t_hi): per hit row the (query start, target start) pairs
    of windows with equal hashes, ordered by (query start, target start), and the extents (smallest start, largest start + k)."""
    qs_seq, qs_start, qs_hash = q_tab
    ts_seq, ts_start, ts_hash = t_tab
    n_rows = len(hit_qid)
    order = np.argsort(ts_hash, kind="stable")
    th = ts_hash[order]
    lo = np.searchsorted(th, qs_hash, side="left")
    hi = np.searchsorted(th, qs_hash, side="right")
    cnt = (hi - lo).astype(np.int64)
    total = int(cnt.sum())
    qi = np.repeat(np.arange(len(qs_hash), dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    ti = order[np.repeat(lo.astype(np.int64), cnt) + (np.arange(total, dtype=np.int64) - np.repeat(first, cnt))]
    assert np.array_equal(qs_hash[qi], ts_hash[ti])
    pq, pt = qs_seq[qi].astype(np.uint64), ts_seq[ti].astype(np.uint64)
    pair_key = (pq << np.uint64(32)) | pt
    hit_key = (hit_qid.astype(np.uint64) << np.uint64(32)) | hit_tid.astype(np.uint64)
    assert np.all(hit_key[1:] > hit_key[:-1])  # rows are ordered by (qid, tid), no duplicates
    row = np.searchsorted(hit_key, pair_key)
    found = (row < n_rows) & (hit_key[np.minimum(row, max(n_rows - 1, 0))] == pair_key) if n_rows else np.zeros(total, bool)
    row, a, b = row[found], qs_start[qi][found], ts_start[ti][found]
    o = np.lexsort((b, a, row))
    row, a, b = row[o], a[o], b[o]
    offs = np.zeros(n_rows + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    ext = [np.zeros(n_rows, np.uint32) for _ in range(4)]
    for r in range(n_rows):
        s, e = int(offs[r]), int(offs[r + 1])
        if e > s:
            ext[0][r], ext[1][r] = a[s:e].min(), a[s:e].max() + ksize
            ext[2][r], ext[3][r] = b[s:e].min(), b[s:e].max() + ksize
    return (offs, a.astype(np.uint32), b.astype(np.uint32), *ext)


def reference(q_res, q_offs, t_res, t_offs, k, scaled, mol, min_containment=0.0):
    """Everything a comparison needs: hits (qid, tid, intersect, n_weighted), the join, and the sketches."""
    q_sk = oracle.sketch_batch(q_res, q_offs, k, scaled, mol, n_threads=4)
    t_sk = oracle.sketch_batch(t_res, t_offs, k, scaled, mol, n_threads=4)
    hits = oracle.manysearch(q_sk[0], q_sk[1], t_sk[0], t_sk[1], t_sk[2], n_threads=4)
    if min_containment > 0.0:
        hits = filter_hits(hits, q_sk[0], min_containment)
    q_tab = position_table(q_res, q_offs, k, scaled, mol, q_sk)
    t_tab = position_table(t_res, t_offs, k, scaled, mol, t_sk)
    return hits, join(q_tab, t_tab, hits[0], hits[1], k), q_sk, t_sk
