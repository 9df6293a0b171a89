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

--exclude replaces those legs by the group-excluding ones at the same two
shapes, with synthetic Market-like labels (751 ids x 6 cams over the gallery,
queries drawn from the same ids, the junk rule as exclusion groups):

  B   the unfiltered ops.search -- from the library --parent-lib names (a
      libpps_hip.so built from the commit to compare against; its
      pps_search_h2_tiled is called on the same operands), else this build's
  B'  ops.search(..., q_group, g_group) of this build; and to say what of
      B' - B costs what: B0 = this build's unfiltered search, B'off = the
      excluding kernel with every query group -1 (its fixed part: the code
      shape and the row's group read), B'miss = gallery groups no query has
      (every survivor's group load, nothing excluded)
  A'  ops.compute_dist into a preallocated buffer, then ops.topk_excluding

alternating in one process under the same repetition scheme (B and B' on the
tile and segment count one timed sweep of the unfiltered search picks), with
peaks; and, at the shard shape, the matrix-free first-match CMC
(reid_dataset_evaluator.cmc_from_search, topk = k) against cmc(
first_match_break=True) on the materialised matrix: wall clock around a
device synchronize (both have host parts), peaks, equality of the curves.

--rank replaces them by the matrix-free mAP legs at the same two shapes and
labels:

  A  ops.compute_dist into a preallocated buffer, then rank_eval on it
  B  ops.rank_eval_fused (no [Q, G] matrix)

alternating under the same repetition scheme, on two kinds of features --
normalised Gaussians unrelated to the labels (every column ranks before some
last positive: the count kernels' worst case) and identity centroids + noise
(_clustered_feats: a few percent of the columns do) -- both with the MatchIndex
built once beforehand, B on the count kernel's tile and segment count one timed
sweep picks; peaks; each path's kernels alone (the distance GEMM,
collect_matches, rank_count_stream; the query split, collect_matches_h2 = the
pair-distance kernel, rank_count_h2 = the fused count kernel); and an error
unless B's per-query ap (float64 bits), valid and first_rank equal A's.

--cmc replaces them by the matrix-free fractional CMC legs, same shapes, labels
and both kinds of features, once in junk mode and once with
separate_camera_set:

  A  ops.compute_dist into a preallocated buffer, then cmc on it
  B  cmc_from_features (no [Q, G] matrix)

alternating under the same repetition scheme (wall clock around a device
synchronize: both build their MatchIndex on the host); the count kernels alone
on the same operands -- cmc_counts_h2 in both modes against rank_count_h2, on
the tile and segment count one timed sweep picks, and cmc_counts on the matrix
-- peaks, and an error unless B's per-query rows equal A's as float64 bits.

  python scripts/bench_search.py [--reps 5] [--shapes market,shard] [--segmented]
                                 [--exclude [--parent-lib PATH]] [--rank] [--cmc]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
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


def _market_labels(Q, G):
    """751 ids x 6 cams over the gallery, queries drawn from the same ids."""
    rng = np.random.RandomState(0)
    return (rng.randint(0, 751, Q), rng.randint(0, 6, Q),
            rng.randint(0, 751, G), rng.randint(0, 6, G))


def _parent_search(path):
    """ops.search's single-index fused call on another build's library: the
    queries split by this build (split_h2_tiled is the same kernel), then that
    library's pps_search_h2_tiled."""
    from pps_amd import _lib, ops
    L = ctypes.CDLL(path)
    fn = L.pps_search_h2_tiled
    fn.argtypes = _lib.SIGNATURES['pps_search_h2_tiled']
    fn.restype = ctypes.c_int

    def search(q, index, k, segments, tile, workspace):
        Q, D = q.shape
        G = index.shape[0]
        q2, qrs, qsq = ops.split_h2_tiled(q)
        g2, grs, gsq = index.h2
        vals = torch.empty((Q, k), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
        rc = fn(q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(), g2.data_ptr(), gsq.data_ptr(),
                grs.data_ptr(), G, D, 0, k, segments, tile, workspace.data_ptr(),
                workspace.numel(), vals.data_ptr(), idx.data_ptr(),
                torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('parent pps_search_h2_tiled failed (status %d)' % rc)
        return vals, idx
    return search


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def bench_exclude(name, Q, G, D, k, reps, ops, parent_lib=None, cmc=False):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    q, gal = _feats(Q, D, gen), _feats(G, D, gen)
    index = ops.GalleryIndex(gal, math='h2')
    qid, qcam, gid, gcam = _market_labels(Q, G)
    qg, gg = ops.exclusion_groups(qid, qcam, gid, gcam, by='id_cam')
    excluded = float((torch.bincount(gg, minlength=int(max(qg.max(), gg.max())) + 1)[qg.long()])
                     .double().mean())
    out = ops.dist_buffer(Q, G, 'cuda')

    best_a = None
    for t in range(ops.h2_num_tiles()):
        ops.compute_dist(q, index, out=out, math='h2', tile=t)
        ms, _ = _time(lambda: ops.compute_dist(q, index, out=out, math='h2', tile=t))
        if best_a is None or ms < best_a[1]:
            best_a = (t, ms)
    tile_a = best_a[0]
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
    parent = _parent_search(parent_lib) if parent_lib else None

    def path_b():
        if parent is not None:
            return parent(q, index, k, seg_b, tile_b, ws)
        return ops.search(q, index, k, segments=seg_b, tile=tile_b, workspace=ws)

    def path_bx():
        return ops.search(q, index, k, segments=seg_b, tile=tile_b, workspace=ws, q_group=qg,
                          g_group=gg)

    def path_ax():
        ops.compute_dist(q, index, out=out, math='h2', tile=tile_a)
        return ops.topk_excluding(out, k, qg, gg)

    qg_off, gg_miss = torch.full_like(qg, -1), gg + (int(qg.max()) + 1)
    parts = dict(
        search_this_build=lambda: ops.search(q, index, k, segments=seg_b, tile=tile_b,
                                             workspace=ws),
        search_excl_off=lambda: ops.search(q, index, k, segments=seg_b, tile=tile_b, workspace=ws,
                                           q_group=qg_off, g_group=gg),
        search_excl_miss=lambda: ops.search(q, index, k, segments=seg_b, tile=tile_b,
                                            workspace=ws, q_group=qg, g_group=gg_miss))
    for f in (path_b, path_bx, path_ax) + tuple(parts.values()):
        f()
    tb, tbx, tax = [], [], []
    tparts = dict((n, []) for n in parts)
    for _ in range(max(reps, 5)):
        ms, rb = _time(path_b)
        tb.append(ms)
        ms, rbx = _time(path_bx)
        tbx.append(ms)
        ms, rax = _time(path_ax)
        tax.append(ms)
        for n, f in parts.items():
            tparts[n].append(_time(f)[0])
    diff = float((rax[0] - rbx[0]).nan_to_num(posinf=0.).abs().max())
    same = bool(torch.equal(rax[1], rbx[1]))
    plain_same = bool(torch.equal(rb[1], ops.search(q, index, k, segments=seg_b, tile=tile_b,
                                                    workspace=ws)[1]))
    del out, rax
    torch.cuda.empty_cache()

    def alloc_ax():
        o = ops.dist_buffer(Q, G, 'cuda')
        ops.compute_dist(q, index, out=o, math='h2', tile=tile_a)
        ops.topk_excluding(o, k, qg, gg)
    peak_ax = _peak(alloc_ax)
    del ws
    torch.cuda.empty_cache()
    peak_bx = _peak(lambda: ops.search(q, index, k, segments=seg_b, tile=tile_b, q_group=qg,
                                       g_group=gg))
    b_ms, bx_ms, ax_ms = _median(tb), _median(tbx), _median(tax)
    res = dict(shape=name, leg='exclude', Q=Q, G=G, D=D, k=k,
               unfiltered_from='parent library' if parent is not None else 'this build',
               excluded_rows_per_query=round(excluded, 2),
               search_ms=round(b_ms, 3), search_excl_ms=round(bx_ms, 3),
               materialised_excl_ms=round(ax_ms, 3),
               excl_over_unfiltered=round(bx_ms / b_ms, 4),
               excl_over_materialised=round(bx_ms / ax_ms, 4),
               materialised_tile=tile_a, search_tile=tile_b, search_segments=seg_b,
               search_excl_peak_bytes=int(peak_bx), materialised_excl_peak_bytes=int(peak_ax),
               max_abs_vals_diff=diff, idx_equal=same, unfiltered_idx_equal_this_build=plain_same,
               search_ms_all=[round(x, 3) for x in tb],
               search_excl_ms_all=[round(x, 3) for x in tbx],
               materialised_excl_ms_all=[round(x, 3) for x in tax])
    for n, t in tparts.items():
        res[n + '_ms'] = round(_median(t), 3)
        res[n + '_ms_all'] = [round(x, 3) for x in t]
    if cmc:
        from pps_amd import reid_dataset_evaluator as gev

        def from_search():
            return gev.cmc_from_search(q, index, qid, gid, qcam, gcam, topk=k)

        def from_matrix():
            d = ops.compute_dist(q, index, math='h2', tile=tile_a, pad_rows=True)
            return gev.cmc(d, qid, gid, qcam, gcam, topk=k, first_match_break=True)

        from_search()
        from_matrix()
        ts, tm = [], []
        for _ in range(max(reps, 5)):
            ms, cs = _wall(from_search)
            ts.append(ms)
            ms, cm = _wall(from_matrix)
            tm.append(ms)
        torch.cuda.empty_cache()
        res.update(cmc_from_search_ms=round(_median(ts), 3), cmc_matrix_ms=round(_median(tm), 3),
                   cmc_from_search_peak_bytes=int(_peak(from_search)),
                   cmc_matrix_peak_bytes=int(_peak(from_matrix)),
                   cmc_equal=bool(np.array_equal(cs, cm)), cmc_rank1=float(cs[0]),
                   cmc_from_search_ms_all=[round(x, 3) for x in ts],
                   cmc_matrix_ms_all=[round(x, 3) for x in tm])
    return res


def _clustered_feats(cent, ids, gen, z=2.5):
    """Identity centroid (cent [ids, D], shared by queries and gallery) + noise,
    normalised.  The noise level puts a same-id pair z standard deviations (of a
    different-id pair's squared distance, 2 / sqrt(D)) closer than a
    different-id pair: positives rank early but not first, and the columns at
    or before a query's LAST positive -- what the count kernels bin -- are a
    fraction of the gallery, not all of it."""
    D = cent.shape[1]
    ids = torch.from_numpy(np.asarray(ids)).cuda()
    sigma = max(D ** 0.5 / z - 1.0, 0.0) ** 0.5
    x = cent[ids] + sigma * torch.randn(len(ids), D, generator=gen, device='cuda')
    x /= x.norm(dim=1, keepdim=True)
    return x


def bench_rank(name, Q, G, D, reps, ops, features='gaussian'):
    """A = compute_dist into a preallocated buffer + rank_eval on it, B =
    rank_eval_fused (no [Q, G] matrix); both get the MatchIndex built once
    (host), so the timed part is device work and the wrappers between the
    launches.  Also each path's kernels alone.  Raises unless B's (ap, valid,
    first_rank) equal A's bit for bit.  features: 'gaussian' (unrelated to the
    labels: every column ranks before some query's last positive, the count
    kernels' worst case) or 'clustered' (_clustered_feats)."""
    from pps_amd import reid_dataset_evaluator as gev
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    qid, qcam, gid, gcam = _market_labels(Q, G)
    if features == 'clustered':
        cent = torch.randn(int(max(qid.max(), gid.max())) + 1, D, generator=gen, device='cuda')
        q, gal = _clustered_feats(cent, qid, gen), _clustered_feats(cent, gid, gen)
        del cent
    else:
        q, gal = _feats(Q, D, gen), _feats(G, D, gen)
    index = ops.GalleryIndex(gal, math='h2')
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    out = ops.dist_buffer(Q, G, 'cuda')

    best_a = None
    for t in range(ops.h2_num_tiles()):
        ops.compute_dist(q, index, out=out, math='h2', tile=t)
        ms, _ = _time(lambda: ops.compute_dist(q, index, out=out, math='h2', tile=t))
        if best_a is None or ms < best_a[1]:
            best_a = (t, ms)
    tile_a = best_a[0]

    # the kernels alone, on the lists and sorted positives both paths share
    q_split = ops.split_h2_tiled(q)
    pd, pi, pc, junk = ops.collect_matches_h2(q_split, index, mi)
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    best_b, sweep = None, {}
    for t in range(1, ops.search_num_tiles()):
        for s in [0, 1, 2, 4, 8, 16]:
            ops.rank_count_h2(q_split, index, 0, sp, junk, segments=s, tile=t)
            ms, _ = _time(lambda: ops.rank_count_h2(q_split, index, 0, sp, junk, segments=s,
                                                    tile=t))
            sweep['tile%d_segments%d' % (t, s)] = round(ms, 3)
            if best_b is None or ms < best_b[2]:
                best_b = (t, s, ms)
    tile_b, seg_b = best_b[0], best_b[1]

    def path_a():
        ops.compute_dist(q, index, out=out, math='h2', tile=tile_a)
        return gev.rank_eval(out, qid, gid, qcam, gcam, index=mi)

    def path_b():
        return ops.rank_eval_fused(q, index, qid, qcam, gid, gcam, segments=seg_b, tile=tile_b,
                                   match_index=mi)

    parts = dict(
        distmat=lambda: ops.compute_dist(q, index, out=out, math='h2', tile=tile_a),
        collect_matches=lambda: ops.collect_matches(out, mi),
        rank_count_stream=lambda: ops.rank_count_stream(out, 0, sp, junk),
        split_queries=lambda: ops.split_h2_tiled(q),
        collect_matches_h2=lambda: ops.collect_matches_h2(q_split, index, mi),
        rank_count_h2=lambda: ops.rank_count_h2(q_split, index, 0, sp, junk, segments=seg_b,
                                                tile=tile_b))
    for f in (path_a, path_b) + tuple(parts.values()):
        f()
    ta, tb = [], []
    tparts = dict((n, []) for n in parts)
    for _ in range(max(reps, 5)):
        ms, ra = _time(path_a)
        ta.append(ms)
        ms, rb = _time(path_b)
        tb.append(ms)
        for n, f in parts.items():
            tparts[n].append(_time(f)[0])
    equal = (torch.equal(ra[0].view(torch.int64), rb[0].view(torch.int64)) and
             torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]))
    if not equal:
        raise RuntimeError('bench_rank %s: rank_eval_fused differs from rank_eval' % name)
    valid = ra[1].bool()
    mAP = float(ra[0][valid].sum() / valid.sum())
    hits = int(valid.sum())
    # the share of the Q x G columns at or before their query's last positive
    binned = float(ops.rank_count_stream(out, 0, sp, junk)[0].sum()) / (float(Q) * G)
    del out, ra, rb
    torch.cuda.empty_cache()

    def alloc_a():
        o = ops.dist_buffer(Q, G, 'cuda')
        ops.compute_dist(q, index, out=o, math='h2', tile=tile_a)
        gev.rank_eval(o, qid, gid, qcam, gcam, index=mi)
    peak_a = _peak(alloc_a)
    torch.cuda.empty_cache()
    peak_b = _peak(path_b)
    a_ms, b_ms = _median(ta), _median(tb)
    res = dict(shape=name, leg='rank', features=features, Q=Q, G=G, D=D,
               list_width=int(sp.sorted_d.shape[1]), valid_queries=int(hits), mAP=mAP,
               binned_fraction=binned,
               materialised_ms=round(a_ms, 3), fused_ms=round(b_ms, 3),
               fused_over_materialised=round(b_ms / a_ms, 4),
               materialised_tile=tile_a, fused_tile=tile_b, fused_segments=seg_b,
               materialised_peak_bytes=int(peak_a), fused_peak_bytes=int(peak_b),
               outputs_equal=bool(equal), rank_count_h2_sweep_ms=sweep,
               materialised_ms_all=[round(x, 3) for x in ta],
               fused_ms_all=[round(x, 3) for x in tb])
    for n, t in tparts.items():
        res[n + '_ms'] = round(_median(t), 3)
        res[n + '_ms_all'] = [round(x, 3) for x in t]
    return res


def bench_cmc(name, Q, G, D, reps, ops, features='gaussian'):
    """A = compute_dist into a preallocated buffer + cmc on it, B =
    cmc_from_features (no [Q, G] matrix), the fractional CMC once in junk mode
    and once with separate_camera_set; wall clock around a device synchronize
    (both build their MatchIndex on the host).  Also the count kernels alone
    on the same operands (device events): cmc_counts_h2 in both modes against
    rank_count_h2, all three on the tile and segment count one timed sweep of
    cmc_counts_h2 picks, and cmc_counts on the matrix.  Raises unless B's
    per-query rows equal A's as float64 bits."""
    from pps_amd import reid_dataset_evaluator as gev
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    qid, qcam, gid, gcam = _market_labels(Q, G)
    if features == 'clustered':
        cent = torch.randn(int(max(qid.max(), gid.max())) + 1, D, generator=gen, device='cuda')
        q, gal = _clustered_feats(cent, qid, gen), _clustered_feats(cent, gid, gen)
        del cent
    else:
        q, gal = _feats(Q, D, gen), _feats(G, D, gen)
    index = ops.GalleryIndex(gal, math='h2')
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    out = ops.dist_buffer(Q, G, 'cuda')

    best_a = None
    for t in range(ops.h2_num_tiles()):
        ops.compute_dist(q, index, out=out, math='h2', tile=t)
        ms, _ = _time(lambda: ops.compute_dist(q, index, out=out, math='h2', tile=t))
        if best_a is None or ms < best_a[1]:
            best_a = (t, ms)
    tile_a = best_a[0]

    q_split = ops.split_h2_tiled(q)
    pd, pi, pc, junk = ops.collect_matches_h2(q_split, index, mi)
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    best_b, sweep = None, {}
    for t in range(1, ops.search_num_tiles()):
        for s in [0, 1, 2, 4, 8, 16]:
            ops.cmc_counts_h2(q_split, index, 0, sp, junk, segments=s, tile=t)
            ms, _ = _time(lambda: ops.cmc_counts_h2(q_split, index, 0, sp, junk, segments=s,
                                                    tile=t))
            sweep['tile%d_segments%d' % (t, s)] = round(ms, 3)
            if best_b is None or ms < best_b[2]:
                best_b = (t, s, ms)
    tile_b, seg_b = best_b[0], best_b[1]

    def path_a(sep):
        ops.compute_dist(q, index, out=out, math='h2', tile=tile_a)
        return gev.cmc(out, qid, gid, qcam, gcam, separate_camera_set=sep, average=False)

    def path_b(sep):
        return gev.cmc_from_features(q, index, qid, gid, qcam, gcam, separate_camera_set=sep,
                                     average=False)

    kw = dict(segments=seg_b, tile=tile_b)
    ops.compute_dist(q, index, out=out, math='h2', tile=tile_a)
    parts = dict(
        cmc_counts=lambda: ops.cmc_counts(out, 0, sp, junk),
        cmc_counts_sepcam=lambda: ops.cmc_counts(out, 0, sp, junk, mi, True),
        rank_count_h2=lambda: ops.rank_count_h2(q_split, index, 0, sp, junk, **kw),
        cmc_counts_h2=lambda: ops.cmc_counts_h2(q_split, index, 0, sp, junk, **kw),
        cmc_counts_h2_sepcam=lambda: ops.cmc_counts_h2(q_split, index, 0, sp, None, mi, True,
                                                       **kw))
    res = dict(shape=name, leg='cmc', features=features, Q=Q, G=G, D=D,
               list_width=int(sp.sorted_d.shape[1]), materialised_tile=tile_a,
               count_tile=tile_b, count_segments=seg_b, cmc_counts_h2_sweep_ms=sweep)
    for f in parts.values():
        f()
    tparts = dict((n, []) for n in parts)
    for _ in range(max(reps, 5)):
        for n, f in parts.items():
            tparts[n].append(_time(f)[0])
    for n, t in tparts.items():
        res[n + '_ms'] = round(_median(t), 3)
        res[n + '_ms_all'] = [round(x, 3) for x in t]
    res['cmc_counts_h2_over_rank_count_h2'] = round(
        res['cmc_counts_h2_ms'] / res['rank_count_h2_ms'], 4)
    res['cmc_counts_h2_sepcam_over_rank_count_h2'] = round(
        res['cmc_counts_h2_sepcam_ms'] / res['rank_count_h2_ms'], 4)
    for sep, mode in ((False, 'junk'), (True, 'sepcam')):
        path_a(sep)
        path_b(sep)
        ta, tb = [], []
        for _ in range(max(reps, 5)):
            ms, ra = _wall(lambda: path_a(sep))
            ta.append(ms)
            ms, rb = _wall(lambda: path_b(sep))
            tb.append(ms)
        equal = (np.array_equal(ra[0].view(np.int64), rb[0].view(np.int64)) and
                 np.array_equal(ra[1], rb[1]))
        if not equal:
            raise RuntimeError('bench_cmc %s (%s): cmc_from_features differs from cmc'
                               % (name, mode))
        a_ms, b_ms = _median(ta), _median(tb)
        res.update({mode + '_materialised_ms': round(a_ms, 3), mode + '_fused_ms': round(b_ms, 3),
                    mode + '_fused_over_materialised': round(b_ms / a_ms, 4),
                    mode + '_rows_equal': bool(equal),
                    mode + '_rank1': float(ra[0][:, 0].sum() / ra[1].sum()),
                    mode + '_materialised_ms_all': [round(x, 3) for x in ta],
                    mode + '_fused_ms_all': [round(x, 3) for x in tb]})
    del out
    torch.cuda.empty_cache()

    def alloc_a():
        o = ops.dist_buffer(Q, G, 'cuda')
        ops.compute_dist(q, index, out=o, math='h2', tile=tile_a)
        gev.cmc(o, qid, gid, qcam, gcam, average=False)
    res['materialised_peak_bytes'] = int(_peak(alloc_a))
    torch.cuda.empty_cache()
    res['fused_peak_bytes'] = int(_peak(lambda: path_b(False)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='market,shard')
    ap.add_argument('--segmented', action='store_true')
    ap.add_argument('--exclude', action='store_true')
    ap.add_argument('--rank', action='store_true')
    ap.add_argument('--cmc', action='store_true')
    ap.add_argument('--parent-lib', default=None)
    a = ap.parse_args()
    from pps_amd import ops
    for name in [s for s in a.shapes.split(',') if s]:
        Q, G, D, k = SHAPES[name]
        if a.cmc:
            for features in ('gaussian', 'clustered'):
                print(json.dumps(bench_cmc(name, Q, G, D, a.reps, ops, features)), flush=True)
                torch.cuda.empty_cache()
        elif a.rank:
            for features in ('gaussian', 'clustered'):
                print(json.dumps(bench_rank(name, Q, G, D, a.reps, ops, features)), flush=True)
                torch.cuda.empty_cache()
        elif a.exclude:
            print(json.dumps(bench_exclude(name, Q, G, D, k, a.reps, ops, a.parent_lib,
                                           cmc=name == 'shard')), flush=True)
        else:
            print(json.dumps(bench_shape(name, Q, G, D, k, a.reps, ops)), flush=True)
        torch.cuda.empty_cache()
    if a.segmented:
        print(json.dumps(bench_segmented(*SEGMENTED, a.reps, ops)), flush=True)


if __name__ == '__main__':
    main()
