"""Fused search (ops.search) against the materialised rank list, one process,
alternating:

  A  ops.compute_dist into a preallocated dist_buffer, then ops.topk
  B  ops.search with a preallocated workspace (no [Q, G] matrix)

on the Market shape (3368 x 15,913, D = 3968, k = 100) and one shard of the
1M-gallery configuration (10,000 x 125,000, D = 2048, k = 100); --segmented
adds 2,000 x 500,000, D = 2048 through GalleryIndex.split (no path A exists at
that size: one index cannot hold the gallery).  The gallery index is built
once; A's GEMM tile is the best of one timed pass over the h2 tiles (as
scripts/bench_shard_1m.py chooses it), B's tile and segment count likewise.
One warm-up of each path, then --reps alternating repetitions timed by device
events; medians.  Features: normalised Gaussian, seed 0.  One JSON line per
shape, with max|vals_A - vals_B| and idx equality on the timed inputs (0 /
true by construction).

  python scripts/bench_search.py [--reps 5] [--shapes market,shard] [--segmented]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SHAPES = {'market': (3368, 15913, 3968, 100), 'shard': (10000, 125000, 2048, 100)}
SEGMENTED = (2000, 500000, 2048, 100)


def _ev():
    return torch.cuda.Event(enable_timing=True)


def _time(fn):
    e0, e1 = _ev(), _ev()
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def _feats(n, d, gen):
    x = torch.randn(n, d, generator=gen, device='cuda')
    x /= x.norm(dim=1, keepdim=True)
    return x


def _peak(fn):
    """Peak allocation of fn above what is resident before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _median(v):
    return sorted(v)[len(v) // 2]


def bench_shape(name, Q, G, D, k, reps, ops):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    q, gal = _feats(Q, D, gen), _feats(G, D, gen)
    index = ops.GalleryIndex(gal, math='h2')
    out = ops.dist_buffer(Q, G, 'cuda')

    # A's tile: one timed pass over the h2 tiles
    best_a = None
    for t in range(ops.h2_num_tiles()):
        ops.compute_dist(q, index, out=out, math='h2', tile=t)
        ms, _ = _time(lambda: ops.compute_dist(q, index, out=out, math='h2', tile=t))
        if best_a is None or ms < best_a[1]:
            best_a = (t, ms)
    tile_a = best_a[0]

    # B's tile and segment count: one timed pass each
    seg_cands = [0, 1, 2, 4, 8, 16]
    ws = torch.empty((max(ops.search_workspace_bytes(Q, G, k, s) for s in seg_cands),),
                     dtype=torch.uint8, device='cuda')
    best_b = None
    for t in range(1, ops.search_num_tiles()):
        for s in seg_cands:
            ops.search(q, index, k, segments=s, tile=t, workspace=ws)
            ms, _ = _time(lambda: ops.search(q, index, k, segments=s, tile=t, workspace=ws))
            if best_b is None or ms < best_b[2]:
                best_b = (t, s, ms)
    tile_b, seg_b = best_b[0], best_b[1]

    def path_a():
        ops.compute_dist(q, index, out=out, math='h2', tile=tile_a)
        return ops.topk(out, k)

    def path_b():
        return ops.search(q, index, k, segments=seg_b, tile=tile_b, workspace=ws)

    path_a()
    path_b()
    ta, tb = [], []
    for _ in range(max(reps, 5)):
        ms, ra = _time(path_a)
        ta.append(ms)
        ms, rb = _time(path_b)
        tb.append(ms)
    diff = float((ra[0] - rb[0]).abs().max())
    same = bool(torch.equal(ra[1], rb[1]))
    # peaks: A owns its [Q, G] buffer, B its workspace (both counted)
    del out
    torch.cuda.empty_cache()

    def alloc_a():
        o = ops.dist_buffer(Q, G, 'cuda')
        ops.compute_dist(q, index, out=o, math='h2', tile=tile_a)
        ops.topk(o, k)
    peak_a = _peak(alloc_a)
    del ws
    torch.cuda.empty_cache()
    peak_b = _peak(lambda: ops.search(q, index, k, segments=seg_b, tile=tile_b))
    a_ms, b_ms = _median(ta), _median(tb)
    return dict(shape=name, Q=Q, G=G, D=D, k=k, materialised_ms=round(a_ms, 3),
                search_ms=round(b_ms, 3), search_over_materialised=round(b_ms / a_ms, 4),
                materialised_tile=tile_a, search_tile=tile_b, search_segments=seg_b,
                materialised_peak_bytes=int(peak_a), search_peak_bytes=int(peak_b),
                workspace_bytes=int(ops.search_workspace_bytes(Q, G, k, seg_b)),
                max_abs_vals_diff=diff, idx_equal=same,
                materialised_ms_all=[round(x, 3) for x in ta],
                search_ms_all=[round(x, 3) for x in tb])


def bench_segmented(Q, G, D, k, reps, ops):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    q, gal = _feats(Q, D, gen), _feats(G, D, gen)
    parts = ops.GalleryIndex.split(gal)
    rows = [p.shape[0] for p in parts]
    need = ops.search_workspace_bytes(Q, max(rows), k, 0)
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')

    def run():
        return ops.search(q, parts, k, workspace=ws)

    run()
    t = [_time(run)[0] for _ in range(max(reps, 5))]
    peak = _peak(run)
    vals, idx = run()
    return dict(shape='segmented', Q=Q, G=G, D=D, k=k, index_segments=rows,
                search_ms=round(_median(t), 3), search_ms_all=[round(x, 3) for x in t],
                workspace_bytes=int(need), search_peak_bytes=int(peak),
                idx_max=int(idx.max()), sorted=bool((vals[:, 1:] >= vals[:, :-1]).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='market,shard')
    ap.add_argument('--segmented', action='store_true')
    a = ap.parse_args()
    from pps_amd import ops
    for name in [s for s in a.shapes.split(',') if s]:
        Q, G, D, k = SHAPES[name]
        print(json.dumps(bench_shape(name, Q, G, D, k, a.reps, ops)), flush=True)
        torch.cuda.empty_cache()
    if a.segmented:
        print(json.dumps(bench_segmented(*SEGMENTED, a.reps, ops)), flush=True)


if __name__ == '__main__':
    main()
