"""GPU: the column lists of the result objects, through the whole region pipeline once.

Six synthetic proteins, searched against themselves (protein, k = 10, scaled = 1): search, k-mer positions, match positions,
regions, scores, alignments, cull, the three takes, traceback, chain + coverage, stitch, both compositions and the alignment
statistics of the three score sources.  Every object's to_host() gives arrays of its table's dtypes and counts; each taken
column is the source's column gathered by the cull's src_region; and after every object is freed — in creation order, then
in a second run in reverse order — the pool holds as many bytes in use as before the pipeline: a column that the free walk
missed (row_coverage included) would stay behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kmerseek_amd as ks  # noqa: E402
from kmerseek_amd import engine  # noqa: E402

K, SCALED, MOL = 10, 1, "protein"
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


def proteins():
    """Six random proteins of 150 - 400 residues; the last two share a 120-residue segment, every 15th residue of it changed
    in one of them (windows of 10 between two changes are shared: the pair has regions besides the self hits)."""
    rng = np.random.default_rng(20)
    seqs = [AMINO[rng.integers(0, 20, n)] for n in (150, 233, 311, 400, 287, 365)]
    seg = AMINO[rng.integers(0, 20, 120)]
    mutated = seg.copy()
    mutated[7::15] = AMINO[(np.searchsorted(AMINO, seg[7::15]) + 1) % 20]
    seqs[4][50:170] = seg
    seqs[5][200:320] = mutated
    return [s.tobytes() for s in seqs]


def check_arrays(obj):
    """to_host() of a column object: the table's dtypes, and its counts as the object reports them."""
    counts = {c: getattr(obj, c) for c in obj._COUNTS}
    got = obj.to_host()
    assert len(got) == len(obj._TABLE) == len(obj.device_ptrs())
    for a, (name, dt, n) in zip(got, obj._TABLE):
        shape = eval(n, {"__builtins__": {}}, counts)
        assert a.dtype == np.dtype(dt) and a.shape == (shape if isinstance(shape, tuple) else (shape,)), (type(obj).__name__, name)
    return got


def pipeline(ctx, res, off, d_res, d_off, Q, T):
    """Every result object of the pipeline, in creation order."""
    n = len(off) - 1
    made = []

    def keep(o):
        made.append(o)
        return o

    ix = keep(ctx.index_build(T))
    hits = keep(ctx.search(ix, Q))
    qp = keep(ctx.kmer_positions_table(res, off, K, SCALED, MOL))
    tp = keep(ctx.kmer_positions_table(res, off, K, SCALED, MOL))
    mp = keep(ctx.match_positions(qp, tp, hits))
    rg = keep(ctx.match_regions(mp))
    sc = keep(ctx.score_regions(rg, hits, res, off, res, off, extend=True, x_drop=10))
    al = keep(ctx.align_regions(rg, hits, res, off, res, off))
    cu = keep(ctx.cull_regions(al, overlap_pct=50))
    taken = [keep(cu.take(o)) for o in (rg, sc, al)]
    cg = keep(ctx.trace_regions(taken[0], hits, res, off, res, off, taken[2]))
    ch = keep(ctx.chain_regions(taken[2]))
    assert ch.coverage(hits, d_off.ptr, n, d_off.ptr, n) == ch.row_coverage_ptr != 0
    st = keep(ctx.stitch_chains(ch, taken[2], cg, hits, res, off, res, off))
    qc = keep(ctx.residue_composition_device(d_res.ptr, d_off.ptr, n, len(res)))
    tc = keep(ctx.residue_composition(res, off))
    stats = [keep(ctx.alignment_stats(sc, hits, qc, tc)), keep(ctx.alignment_stats(al, hits, qc, tc, allow_ungapped=True)),
             keep(ctx.alignment_stats(st, hits, qc, tc, allow_ungapped=True, alignments=taken[2]))]

    assert hits.count >= n + 2 and rg.n_regions > rg.n_rows == hits.count  # the self hits and the pair, both ways; some row has two regions
    for o in made:
        if isinstance(o, engine._Columns):
            check_arrays(o)
    assert sum(isinstance(o, engine._Columns) for o in made) == 16 and len(ch.coverage_to_host()) == hits.count
    assert (stats[0].n_entries, stats[1].n_entries, stats[2].n_entries) == (sc.n_regions, al.n_regions, hits.count)

    # the takes: row_offsets are the cull's, every other column is the source's gathered by src_region
    c_offs, src = cu.to_host()[:2]
    assert 0 < cu.n_kept == len(src) <= cu.n_regions == al.n_regions
    for whole, part in zip((rg, sc, al), taken):
        assert type(part) is type(whole) and (part.n_rows, part.n_regions) == (cu.n_rows, cu.n_kept)
        w, p = whole.to_host(), part.to_host()
        assert np.array_equal(p[0], c_offs)
        for name, a, b in zip(whole._COLUMNS[1:], w[1:], p[1:]):
            assert np.array_equal(b, a[src]), (type(whole).__name__, name)
    return made


@pytest.mark.parametrize("order", ["creation", "reverse"])
def test_pipeline_columns_and_what_free_gives_back(order):
    res, off = ks.pack(proteins())
    with ks.Context(0) as ctx:
        d_res, d_off = ctx.to_device(res), ctx.to_device(off)
        T = ctx.sketch_batch(res, off, K, SCALED, MOL)
        Q = ctx.sketch_batch(res, off, K, SCALED, MOL)
        before = ctx.pool_stats()["bytes_in_use"]
        made = pipeline(ctx, res, off, d_res, d_off, Q, T)
        held = ctx.pool_stats()["bytes_in_use"]
        for o in (made if order == "creation" else reversed(made)):
            o.free()
        after = ctx.pool_stats()["bytes_in_use"]
        print(f"{order}: {len(made)} objects, bytes in use {before} -> {held} -> {after}")
        assert held > before and after == before
        for o in (Q, T, d_res, d_off):
            o.free()
