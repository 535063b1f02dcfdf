"""The region chain in plain Python loops, straight from the contract in include/kmerseek_amd.h: the regions of a row in the
order of (q_start, index), best[i] = score[i] + max(0, best[j] - cost(j, i)) over the j that i follows, the end region, the walk
back.  Python integers (the one numpy expression per region works in int64 on values the contract bounds): nothing here can
overflow.  The yardstick of ks_regions_chain_device; `enumerate_row` is the yardstick's own: every ordered subset of a row."""
import itertools
import math

import numpy as np

NONE = 0xFFFFFFFF
NAMES = ("row_offsets", "src_region", "best", "pred", "chain_score", "q_start", "q_length", "t_start", "t_length", "q_aligned",
         "t_aligned", "identities", "aln_length", "row_chain_score")
DTYPES = (np.uint64, np.uint32, np.int64, np.uint32, np.int64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32,
          np.uint64, np.uint64, np.float64)


def follows(a, b, max_gap=0, max_overlap=0):
    """a, b: (q_start, q_length, t_start, t_length).  b can stand behind a in a chain."""
    aqe, ate, bqe, bte = a[0] + a[1], a[2] + a[3], b[0] + b[1], b[2] + b[3]
    if not (a[0] < b[0] and a[2] < b[2] and aqe < bqe and ate < bte):
        return False
    dq, dt = b[0] - aqe, b[2] - ate
    if max(0, -dq, -dt) > max_overlap:
        return False
    return not (max_gap > 0 and max(dq, dt, 0) > max_gap)


def cost(a, b, link_cost=0, skew_cost=0, overlap_cost=0):
    dq, dt = b[0] - (a[0] + a[1]), b[2] - (a[2] + a[3])
    return link_cost + skew_cost * abs(dq - dt) + overlap_cost * max(0, -dq, -dt)


def chain_row(ext, score, max_gap=0, max_overlap=0, link_cost=0, skew_cost=0, overlap_cost=0):
    """One row: ext[i] = (q_start, q_length, t_start, t_length), score[i].  -> (best, pred by local index or None, the chain's
    members in chain order).  The inner loop over the predecessors of a region is one numpy expression."""
    n = len(ext)
    if n == 0:
        return [], [], []
    e = np.array(ext, np.int64).reshape(n, 4)
    qs, ts, qe, te = e[:, 0], e[:, 2], e[:, 0] + e[:, 1], e[:, 2] + e[:, 3]
    idx = np.arange(n)
    best = np.array(score, np.int64)
    pred = [None] * n
    for i in sorted(range(n), key=lambda i: (ext[i][0], i)):  # every j that i follows has a smaller q_start: best[j] is final
        dq, dt = qs[i] - qe, ts[i] - te
        ov = np.maximum(0, np.maximum(-dq, -dt))
        ok = (qs < qs[i]) & (ts < ts[i]) & (qe < qe[i]) & (te < te[i]) & (ov <= max_overlap)
        if max_gap > 0:
            ok &= np.maximum(np.maximum(dq, dt), 0) <= max_gap
        if not ok.any():
            continue
        cand = np.where(ok, best - (link_cost + skew_cost * np.abs(dq - dt) + overlap_cost * ov), -1)
        top = int(cand.max())
        if top > 0:
            pred[i] = int(idx[cand == top][0])  # the smallest index among equal maxima
            best[i] += top
    best = [int(v) for v in best]
    end = max(range(n), key=lambda i: (best[i], -i))
    members = []
    while end is not None:
        members.append(end)
        end = pred[end]
    return best, pred, members[::-1]


def chain(row_offsets, q_start, q_length, t_start, t_length, score, identities=None, aln_length=None, **opts):
    """-> the arrays of RegionChain.to_host(), in the order of NAMES.  t_length None: the query lengths."""
    offs = [int(v) for v in row_offsets]
    qs, ql, ts = [[int(v) for v in c] for c in (q_start, q_length, t_start)]
    tl = ql if t_length is None else [int(v) for v in t_length]
    sc = [int(v) for v in score]
    n = len(qs)
    out = {k: [] for k in NAMES}
    out["row_offsets"].append(0)
    out["best"], out["pred"] = [0] * n, [NONE] * n
    for r in range(len(offs) - 1):
        b, e = offs[r], offs[r + 1]
        ext = [(qs[g], ql[g], ts[g], tl[g]) for g in range(b, e)]
        best, pred, mem = chain_row(ext, sc[b:e], **opts)
        for i in range(e - b):
            out["best"][b + i] = best[i]
            out["pred"][b + i] = NONE if pred[i] is None else b + pred[i]
        out["src_region"] += [b + m for m in mem]
        out["row_offsets"].append(len(out["src_region"]))
        if not mem:
            row = (0, 0, 0, 0, 0, 0, 0, 0, 0, math.nan)
        else:
            f, l = ext[mem[0]], ext[mem[-1]]
            qa, ta = f[1], f[3]
            for a, c in zip(mem, mem[1:]):
                qa += ext[c][0] + ext[c][1] - max(ext[c][0], ext[a][0] + ext[a][1])
                ta += ext[c][2] + ext[c][3] - max(ext[c][2], ext[a][2] + ext[a][3])
            row = (best[mem[-1]], f[0], l[0] + l[1] - f[0], f[2], l[2] + l[3] - f[2], qa, ta,
                   0 if identities is None else sum(int(identities[b + m]) for m in mem),
                   0 if aln_length is None else sum(int(aln_length[b + m]) for m in mem), float(best[mem[-1]]))
        for k, v in zip(NAMES[4:], row):
            out[k].append(v)
    return tuple(np.array(out[k], d) for k, d in zip(NAMES, DTYPES))


def enumerate_row(ext, score, **opts):
    """The largest value of any ordered subset of the row in which every region follows the one before it: the sum of its scores
    minus the sum of its link costs.  Exhaustive: rows of a handful of regions only."""
    gate = {k: opts.get(k, 0) for k in ("max_gap", "max_overlap")}
    price = {k: opts.get(k, 0) for k in ("link_cost", "skew_cost", "overlap_cost")}
    n = len(ext)
    top = None
    for m in range(1, n + 1):
        for sub in itertools.permutations(range(n), m):
            if all(follows(ext[a], ext[b], **gate) for a, b in zip(sub, sub[1:])):
                v = sum(score[i] for i in sub) - sum(cost(ext[a], ext[b], **price) for a, b in zip(sub, sub[1:]))
                top = v if top is None else max(top, v)
    return top


def coverage(chain_host, qid, tid, q_off, t_off, mode):
    """row_coverage f64[n_rows] of ks_rchain_coverage: one f64 division per side; NaN for a row without a chain or a sequence of
    length 0.  mode: 0 the query's share, 1 the target's, 2 the smaller, 3 the larger."""
    offs, qa, ta = np.asarray(chain_host[0]), np.asarray(chain_host[9]), np.asarray(chain_host[10])
    q_off, t_off = np.asarray(q_off, np.uint64), np.asarray(t_off, np.uint64)
    qid, tid = np.asarray(qid, np.int64), np.asarray(tid, np.int64)
    lq, lt = (q_off[qid + 1] - q_off[qid]).astype(np.float64), (t_off[tid + 1] - t_off[tid]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cq = np.where(lq > 0, qa.astype(np.float64) / lq, np.nan)
        ct = np.where(lt > 0, ta.astype(np.float64) / lt, np.nan)
    v = (cq, ct, np.minimum(cq, ct), np.maximum(cq, ct))[mode]
    return np.where(offs[1:] != offs[:-1], v, np.nan)


def chain_rows(seed, n_rows, max_len, lengths=None, n_tracks=3, top_end=True, columns=True):
    """Rows of 0 .. max_len regions (lengths: the rows' lengths instead).  Two thirds of a row's regions lie along n_tracks noisy
    diagonal tracks: their starts ascend by about their length on both sequences, so long chains exist; the rest are scattered
    over the same span and repeat starts, ends and scores of regions already there.  With top_end the last track region of the
    first row of 2 or more regions ends exactly at 0xffffffff on the target.
    -> (row_offsets, q_start, q_length, t_start, t_length, score, identities, aln_length) as numpy columns."""
    rng = np.random.default_rng(seed)
    offs, cols = [0], [[], [], [], [], [], [], []]
    done_top = not top_end
    for r in range(len(lengths) if lengths is not None else n_rows):
        m = int(rng.integers(0, max_len + 1)) if lengths is None else int(lengths[r])
        rows = []
        n_track = (2 * m + 2) // 3
        per = [n_track // n_tracks + (1 if k < n_track % n_tracks else 0) for k in range(n_tracks)]
        for k, cnt in enumerate(per):
            q, t = int(rng.integers(0, 50)), int(rng.integers(0, 50)) + 4000 * k
            for _ in range(cnt):
                ql = int(rng.integers(5, 40))
                tl = ql if rng.random() < 0.5 else max(1, ql + int(rng.integers(-3, 4)))
                rows.append([q, ql, t, tl, int(rng.integers(5, 60))])
                q += ql + int(rng.integers(-4, 12)); t += tl + int(rng.integers(-4, 12))
                q, t = max(q, rows[-1][0] + 1), max(t, rows[-1][2] + 1)
        span_q = max([g[0] + g[1] for g in rows] + [100])
        while len(rows) < m:
            kind = rng.random()
            if rows and kind < 0.5:  # a copy of a region's start, of its end, or of all of it, with a score from a small range
                g = list(rows[int(rng.integers(0, len(rows)))])
                if kind < 0.2:
                    g[1] = max(1, g[1] - int(rng.integers(0, 4))); g[3] = max(1, g[3] - int(rng.integers(0, 4)))  # same start
                elif kind < 0.4:
                    d = int(rng.integers(0, min(4, g[1], g[3])))
                    g[0] += d; g[1] -= d; g[2] += d; g[3] -= d  # same ends
                g[4] = int(rng.integers(-5, 12)) if rng.random() < 0.5 else g[4]
                rows.append(g)
            else:
                ql = int(rng.integers(1, 40))
                rows.append([int(rng.integers(0, span_q)), ql, int(rng.integers(0, span_q + 4000 * n_tracks)), int(rng.integers(1, 40)),
                             int(rng.integers(-5, 12))])
        if not done_top and m >= 2:  # the last region of track 0 (and whatever copied it later) up against the top of u32
            done_top = True
            g = rows[per[0] - 1]
            g[3] = g[1]  # (one length: the region is valid with the query lengths on both sides too)
            g[2] = 0xFFFFFFFF - g[3]
        order = rng.permutation(len(rows))  # the input order is not the evaluation order
        for i in order:
            g = rows[int(i)]
            for c in range(5):
                cols[c].append(g[c])
            alen = max(g[1], g[3])
            cols[5].append(int(rng.integers(0, min(g[1], g[3]) + 1))); cols[6].append(alen)
        offs.append(len(cols[0]))
    return (np.array(offs, np.uint64), *[np.array(cols[c], np.uint32) for c in range(4)], np.array(cols[4], np.int64),
            np.array(cols[5], np.uint32), np.array(cols[6], np.uint32))
