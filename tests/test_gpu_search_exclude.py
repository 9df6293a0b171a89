"""GPU parity of the group-excluding fused search (search_h2_kernel's EXCL
instantiations, ops.search(..., q_group, g_group)), its materialised twin
ops.topk_excluding, ShardedEvaluator.rank_list(exclude=...) and the
matrix-free first-match CMC (reid_dataset_evaluator.cmc_from_search).

The yardstick is the definition, computed from the non-excluding operators
only: the matrix ops.compute_dist(..., math='h2') writes, the excluded cells
set to +inf by a torch mask, ops.topk, and the entries that landed on an
excluded cell overwritten with (+inf, -1).  It is never topk_excluding or
search themselves.  The claim is equality of the indices and of the values'
bits.  All inputs are finite: +inf appears only as the pad."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import evaluator as ev

pytestmark = pytest.mark.gpu

INF = float('inf')


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda()


def _feats(seed, n, d):
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _yardstick(dist, k, q_group, g_group):
    """The result definition from a materialised matrix (left unchanged)."""
    from pps_amd import ops
    Q, G = dist.shape
    mask = (g_group[None, :] == q_group[:, None]) & (q_group[:, None] >= 0)
    pv = torch.full((Q, k), INF, dtype=torch.float32, device=dist.device)
    pi = torch.full((Q, k), -1, dtype=torch.int32, device=dist.device)
    kin = min(k, G)
    if kin:
        vals, idx = ops.topk(dist.masked_fill(mask, INF), kin)
        hit = mask.gather(1, idx.long())
        pv[:, :kin] = vals.masked_fill(hit, INF)
        pi[:, :kin] = idx.masked_fill(hit, -1)
    return pv, pi


def _expect(q, index, metric, k, q_group, g_group):
    from pps_amd import ops
    return _yardstick(ops.compute_dist(q, index, metric=metric, math='h2'), k, q_group, g_group)


def _same(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert torch.equal(got[1], want[1]), 'indices differ'
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), 'values differ'


def _labels(seed, n, nid, ncam):
    rng = np.random.RandomState(seed)
    return rng.randint(0, nid, n), rng.randint(0, ncam, n)


_RAGGED = [(3, 5, 64, 10), (37, 1000, 96, 100), (300, 4099, 128, 21), (17, 2100, 32, 256)]
_LABELS = {'few': (23, 6), 'sixth': (3, 2)}
_cache = {}


def _case(Q, G, D, labels):
    """Features, index, groups and the expected lists, built once."""
    from pps_amd import ops
    key = (Q, G, D, labels)
    if key not in _cache:
        nid, ncam = _LABELS[labels]
        qid, qcam = _labels(21, Q, nid, ncam)
        gid, gcam = _labels(22, G, nid, ncam)
        qg, gg = ops.exclusion_groups(qid, qcam, gid, gcam, by='id_cam')
        q, g = _cuda(_feats(1, Q, D)), _cuda(_feats(2, G, D))
        _cache[key] = (q, ops.GalleryIndex(g, math='h2'), qg, gg, {})
    return _cache[key]


def _check_ragged(Q, G, D, k, labels, segments, metric):
    from pps_amd import ops
    q, index, qg, gg, want = _case(Q, G, D, labels)
    if (metric, k) not in want:
        want[(metric, k)] = _expect(q, index, metric, k, qg, gg)
    wv, wi = want[(metric, k)]
    # the label set does what it is there for
    excluded = int(((gg[None, :] == qg[:, None]) & (qg[:, None] >= 0)).sum())
    if G >= 1000:
        assert excluded > 0
        if labels == 'sixth':
            assert 0.1 < excluded / float(Q * G) < 0.25
    for tile in range(ops.search_num_tiles()):
        got = ops.search(q, index, k, metric=metric, segments=segments, tile=tile,
                         q_group=qg, g_group=gg)
        _same(got, (wv, wi))
    live = wi >= 0
    assert not bool((gg[wi.long().clamp(min=0)] == qg[:, None])[live].any())


@pytest.mark.parametrize('segments', [0, 1, 5])
@pytest.mark.parametrize('labels', sorted(_LABELS))
@pytest.mark.parametrize('Q,G,D,k', _RAGGED)
def test_exclude_ragged_shapes(Q, G, D, k, labels, segments):
    from pps_amd import ops
    assert max(s[3] for s in _RAGGED) == ops.search_max_k()
    _check_ragged(Q, G, D, k, labels, segments, 'euclidean')


@pytest.mark.parametrize('segments', [0, 1, 5])
@pytest.mark.parametrize('labels', sorted(_LABELS))
def test_exclude_ragged_cosine(labels, segments):
    _check_ragged(300, 4099, 128, 21, labels, segments, 'cosine')


def test_exclude_starved_rows():
    """G = 1030, k = 40: rows with no, k - 1 and five valid gallery rows (the
    five in the last tile and segment), a negative query group, negative
    gallery groups."""
    from pps_amd import ops
    G, D, k = 1030, 64, 40
    q, index = _cuda(_feats(31, 4, D)), ops.GalleryIndex(_cuda(_feats(32, G, D)), math='h2')
    plain = ops.search(q, index, k)

    def run(q_group, g_group):
        qg, gg = _i32(q_group), _i32(g_group)
        want = _expect(q, index, 'euclidean', k, qg, gg)
        for segments in (0, 1, 5):
            for tile in range(ops.search_num_tiles()):
                _same(ops.search(q, index, k, segments=segments, tile=tile, q_group=qg,
                                 g_group=gg), want)
        return want

    # every gallery row carries the query's group: nothing is left
    wv, wi = run([7, -1, 7, 3], np.full(G, 7))
    for r in (0, 2):
        assert torch.all(wi[r] == -1) and torch.all(torch.isinf(wv[r]))
    for r in (1, 3):   # a negative group / a group no gallery row has: unfiltered
        assert torch.equal(wi[r], plain[1][r]) and torch.equal(wv[r], plain[0][r])
    # exactly k - 1 rows are left: one pad at the end
    gg = np.full(G, 7)
    gg[np.arange(k - 1) * 26 + 3] = 9
    wv, wi = run([7, 7, 9, -1], gg)
    for r in (0, 1):
        assert torch.all(wi[r, :k - 1] >= 0) and int(wi[r, k - 1]) == -1
        assert torch.all(torch.isfinite(wv[r, :k - 1])) and bool(torch.isinf(wv[r, k - 1]))
    assert torch.all(wi[2] >= 0)
    # only rows 1025..1029 are left: the last tile and segment hold the answer
    gg = np.full(G, 7)
    gg[1025:] = 8
    wv, wi = run([7, 8, -1, 7], gg)
    for r in (0, 3):
        assert sorted(wi[r, :5].tolist()) == list(range(1025, 1030))
        assert torch.all(wi[r, 5:] == -1)
    assert torch.equal(wi[2], plain[1][2])
    # negative gallery groups are never excluded, whatever the query's group
    gg = np.random.RandomState(33).randint(-2, 3, G)
    wv, wi = run([0, -2, 2, -1], gg)
    ggd = _i32(gg)
    assert bool((ggd[wi.long()] < 0).any())
    assert not bool((ggd[wi[0].long()] == 0).any()) and not bool((ggd[wi[2].long()] == 2).any())
    for r in (1, 3):
        assert torch.equal(wi[r], plain[1][r]) and torch.equal(wv[r], plain[0][r])


@pytest.mark.parametrize('order', ['first', 'last'])
def test_exclude_nearest_rows_excluded(order):
    """600 near-duplicates of query 0 carry its group: more than k + 64 + 256,
    so an implementation that lets excluded rows into the candidate buffer
    cuts while it has seen nothing else, and loses members of the answer."""
    from pps_amd import ops
    G, D, k, ndup = 2100, 64, 100, 600
    rng = np.random.RandomState(41)
    q = _feats(42, 9, D)
    g = _feats(43, G, D)
    g[:ndup] = q[0][None] + 1e-3 * rng.randn(ndup, D).astype(np.float32)
    gg = rng.randint(0, 5, G)
    gg[:ndup] = 5
    if order == 'last':
        g, gg = g[::-1].copy(), gg[::-1].copy()
    qg = rng.randint(0, 5, 9)
    qg[0] = 5
    qd, index = _cuda(q), ops.GalleryIndex(_cuda(g), math='h2')
    qg, gg = _i32(qg), _i32(gg)
    want = _expect(qd, index, 'euclidean', k, qg, gg)
    assert torch.all(want[1][0] >= 0) and not bool((gg[want[1][0].long()] == 5).any())
    # unfiltered, row 0 is nothing but the near-duplicates
    assert bool((gg[ops.search(qd, index, k)[1][0].long()] == 5).all())
    for segments in (0, 1, 3):
        for tile in range(ops.search_num_tiles()):
            _same(ops.search(qd, index, k, segments=segments, tile=tile, q_group=qg,
                             g_group=gg), want)


@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
def test_exclude_ties_across_tile_and_segment_edges(metric):
    """Copies of one gallery row across a tile edge and a segment edge, every
    second copy excluded for the query that equals the copied row."""
    from pps_amd import ops
    D, k = 64, 40
    g = _feats(9, 1030, D)
    g[250:263] = g[3]
    g[1020:1030] = g[3]
    q = _feats(10, 12, D)
    q[0] = g[3]
    q[1] = g[3] + 0.01 * q[1]
    rng = np.random.RandomState(51)
    gg = rng.randint(0, 3, 1030)
    copies = np.concatenate([[3], np.arange(250, 263), np.arange(1020, 1030)])
    gg[copies] = np.arange(len(copies)) % 2
    qg = rng.randint(-1, 3, 12)
    qg[0] = qg[1] = 1
    qd, index = _cuda(q), ops.GalleryIndex(_cuda(g), math='h2')
    qg, gg = _i32(qg), _i32(gg)
    want = _expect(qd, index, metric, k, qg, gg)
    kept = [int(c) for c in copies[::2]]
    assert want[1][0, :len(kept)].tolist() == kept   # the tie goes by index
    for segments in (0, 1, 2, 5):
        for tile in range(ops.search_num_tiles()):
            _same(ops.search(qd, index, k, metric=metric, segments=segments, tile=tile,
                             q_group=qg, g_group=gg), want)


def test_exclude_self_search():
    """"Exclude myself": group = row number on both sides.  The yardstick
    matrix is asked for with symmetric=False: for q and g the same rows
    compute_dist would otherwise pick the mirrored upper-triangle kernel
    (pps_distmat_h2_self_tiled), whose lower triangle is a copy of the upper
    one and not the bits pps_distmat_h2_tiled -- the matrix the search is
    defined on -- writes."""
    from pps_amd import ops
    x = _cuda(_feats(61, 300, 64))
    me = torch.arange(300, dtype=torch.int32, device='cuda')
    got = ops.search(x, x, 20, q_group=me, g_group=me)
    assert not bool((got[1] == me[:, None]).any()) and torch.all(got[1] >= 0)
    assert torch.all(ops.search(x, x, 20)[1][:, 0] == me)   # unfiltered, each row finds itself
    dist = ops.compute_dist(x, ops.GalleryIndex(x, math='h2'), math='h2', symmetric=False)
    _same(got, _yardstick(dist, 20, me, me))


def test_exclude_segmented_gallery():
    from pps_amd import ops
    G, D, k = 1030, 64, 40
    qd, gd = _cuda(_feats(10, 12, D)), _cuda(_feats(9, G, D))
    qid, qcam = _labels(71, 12, 3, 2)
    gid, gcam = _labels(72, G, 3, 2)
    qg, gg = ops.exclusion_groups(qid, qcam, gid, gcam)
    one = ops.GalleryIndex(gd, math='h2')
    want = _expect(qd, one, 'euclidean', k, qg, gg)
    _same(ops.search(qd, one, k, q_group=qg, g_group=gg), want)
    parts = ops.GalleryIndex.split(gd, max_rows=400)
    assert [p.shape[0] for p in parts] == [400, 400, 230]
    got = ops.search(qd, parts, k, q_group=qg, g_group=gg)
    _same(got, want)
    assert int(got[1].max()) >= 800   # global indices
    many = ops.GalleryIndex.split(gd, max_rows=16)
    assert len(many) == 65
    _same(ops.search(qd, many, k, q_group=qg, g_group=gg), want)


def test_exclude_fallbacks():
    """The cases search answers from the materialised matrix: each equals the
    yardstick built on the matrix of the same arithmetic."""
    from pps_amd import ops
    rng = np.random.RandomState(14)
    # D % 32 != 0: an x3 index
    q, g = _cuda(rng.randn(7, 20)), _cuda(rng.randn(90, 20))
    qg, gg = _i32(rng.randint(-1, 3, 7)), _i32(rng.randint(-1, 3, 90))
    index = ops.GalleryIndex(g, math='h2')
    assert index.math == 'x3'
    dist = ops.compute_dist(q, index)
    keep = dist.clone()
    _same(ops.search(q, index, 10, q_group=qg, g_group=gg), _yardstick(dist, 10, qg, gg))
    _same(ops.search(q, g, 10, q_group=qg, g_group=gg), _yardstick(dist, 10, qg, gg))
    _same(ops.search(q, index, 100, q_group=qg, g_group=gg), _yardstick(dist, 100, qg, gg))
    # the twin itself, and it leaves the matrix alone
    _same(ops.topk_excluding(dist, 10, qg, gg), _yardstick(dist, 10, qg, gg))
    assert torch.equal(dist, keep)
    # a strided query view
    qs = _cuda(_feats(15, 9, 128))[:, :64]
    assert not qs.is_contiguous()
    index = ops.GalleryIndex(_cuda(_feats(16, 500, 64)), math='h2')
    qc = qs.contiguous()
    qg, gg = _i32(rng.randint(-1, 3, 9)), _i32(rng.randint(0, 3, 500))
    _same(ops.search(qs, index, 20, q_group=qg, g_group=gg),
          _yardstick(ops.compute_dist(qc, index), 20, qg, gg))
    # k beyond the fused kernel's
    assert ops.search_max_k() < 300
    _same(ops.search(qc, index, 300, q_group=qg, g_group=gg),
          _yardstick(ops.compute_dist(qc, index, math='h2'), 300, qg, gg))


def test_exclude_argument_contract():
    from pps_amd import _lib, ops
    Q, G, D, k = 33, 2100, 64, 100
    q, index = _cuda(_feats(1, Q, D)), ops.GalleryIndex(_cuda(_feats(2, G, D)), math='h2')
    qg = torch.zeros(Q, dtype=torch.int32, device='cuda')
    gg = torch.ones(G, dtype=torch.int32, device='cuda')
    ops.search(q, index, k, q_group=qg, g_group=gg)
    for kw in (dict(q_group=qg), dict(g_group=gg),
               dict(q_group=qg[:-1], g_group=gg), dict(q_group=qg, g_group=gg[:-1]),
               dict(q_group=qg.long(), g_group=gg), dict(q_group=qg, g_group=gg.float()),
               dict(q_group=qg.cpu(), g_group=gg), dict(q_group=qg, g_group=gg.cpu())):
        with pytest.raises(RuntimeError):
            ops.search(q, index, k, **kw)
    with pytest.raises(RuntimeError):
        ops.topk_excluding(ops.compute_dist(q, index), k, qg, gg[:-1])
    # the C entry: a null group pointer is an error and nothing is launched
    q2, qrs, qsq = ops.split_h2_tiled(q)
    g2, grs, gsq = index.h2
    need = ops.search_workspace_bytes(Q, G, k, 0)
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
    vals = torch.full((Q, k), -7.0, dtype=torch.float32, device='cuda')
    idx = torch.full((Q, k), -7, dtype=torch.int32, device='cuda')
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for a, b in ((None, gg.data_ptr()), (qg.data_ptr(), None), (None, None)):
        rc = L.pps_search_h2_tiled_excl(q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(),
                                        g2.data_ptr(), gsq.data_ptr(), grs.data_ptr(), G, D, 0,
                                        k, 0, 0, ws.data_ptr(), need, vals.data_ptr(),
                                        idx.data_ptr(), a, b, st)
        torch.cuda.synchronize()
        assert rc == -1   # PPS_ERR_INVALID_ARG
        assert torch.all(vals == -7.0) and torch.all(idx == -7)
    rc = L.pps_search_h2_tiled_excl(q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(),
                                    g2.data_ptr(), gsq.data_ptr(), grs.data_ptr(), G, D, 0, k, 0,
                                    0, ws.data_ptr(), need, vals.data_ptr(), idx.data_ptr(),
                                    qg.data_ptr(), gg.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0
    _same((vals, idx), ops.search(q, index, k))   # group 0 against all-1: nothing excluded


@pytest.mark.parametrize('exclude', ['id_cam', 'cam'])
@pytest.mark.parametrize('G', [1200, 60])
def test_exclude_sharded_rank_list(G, exclude):
    from pps_amd import distributed as pdist
    from pps_amd import ops
    Q, D, k = 40, 96, 100
    rng = np.random.RandomState(17)
    q, g = _cuda(_feats(18, Q, D)), _cuda(_feats(19, G, D))
    qid, gid = rng.randint(0, 10, Q), rng.randint(0, 10, G)
    qcam, gcam = rng.randint(0, 3, Q), rng.randint(0, 3, G)
    sh = pdist.ShardedEvaluator(qid, qcam, gid, gcam, 0, 1)
    qg, gg = ops.exclusion_groups(qid, qcam, gid, gcam, by=exclude)
    want = _yardstick(ops.compute_dist(q, g, math='h2'), k, qg, gg)
    fused = sh.rank_list(q, g, k=k, fused=True, exclude=exclude)
    mat = sh.rank_list(q, g, k=k, fused=False, exclude=exclude)
    _same(fused, mat)
    _same(fused, want)
    # no listed row is one the rule drops
    i = fused[1].cpu().numpy()
    same_cam = gcam[np.maximum(i, 0)] == qcam[:, None]
    drop = same_cam if exclude == 'cam' else same_cam & (gid[np.maximum(i, 0)] == qid[:, None])
    assert not (drop & (i >= 0)).any()
    with pytest.raises(RuntimeError):
        sh.rank_list(q, g, k=k, fused=True, exclude='id')


def _cmc_case():
    Q, G, D = 60, 1500, 96
    rng = np.random.RandomState(81)
    q, g = _feats(82, Q, D), _feats(83, G, D)
    qid, gid = rng.randint(0, 30, Q), rng.randint(0, 30, G)
    qcam, gcam = rng.randint(0, 6, Q), rng.randint(0, 6, G)
    qid[0] = 99                      # an id the gallery does not hold
    gcam[gid == 29] = 2              # id 29 is seen by camera 2 only ...
    qid[1], qcam[1] = 29, 2          # ... which is this query's: junk only
    qid[2], qcam[2] = 29, 3          # and this one's matches are all valid
    return q, g, qid, gid, qcam, gcam


@pytest.mark.parametrize('separate', [False, True])
def test_cmc_from_search_equals_oracle(separate):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    q, g, qid, gid, qcam, gcam = _cmc_case()
    topk = 50
    qd, gd = _cuda(q), _cuda(g)
    dist = ops.compute_dist(qd, gd, math='h2').cpu().numpy()
    ref, ref_valid = ev.cmc(dist, qid, gid, qcam, gcam, topk=topk, separate_camera_set=separate,
                            first_match_break=True, average=False)
    ret, valid = gev.cmc_from_search(qd, gd, qid, gid, qcam, gcam, topk=topk,
                                     separate_camera_set=separate, average=False)
    assert valid[0] == 0 and valid[1] == 0 and valid[2] == 1
    assert 0 < ret[:, -1].sum() < valid.sum()   # first matches inside and past topk
    assert np.array_equal(valid, ref_valid)
    assert np.array_equal(ret, ref)
    avg = gev.cmc_from_search(qd, ops.GalleryIndex(gd, math='h2'), qid, gid, qcam, gcam,
                              topk=topk, separate_camera_set=separate)
    assert np.array_equal(avg, ev.cmc(dist, qid, gid, qcam, gcam, topk=topk,
                                      separate_camera_set=separate, first_match_break=True))
    # host arrays and a segmented gallery are taken as ops.search takes them
    ret2, _ = gev.cmc_from_search(q, ops.GalleryIndex.split(gd, max_rows=400), qid, gid, qcam,
                                  gcam, topk=topk, separate_camera_set=separate, average=False)
    assert np.array_equal(ret2, ref)


def test_cmc_from_search_rejects():
    from pps_amd import reid_dataset_evaluator as gev
    q, g, qid, gid, qcam, gcam = _cmc_case()
    qd, gd = _cuda(q), _cuda(g)
    with pytest.raises(RuntimeError, match='No valid query'):
        gev.cmc_from_search(qd, gd, qid + 1000, gid, qcam, gcam, topk=50)
    with pytest.raises(RuntimeError, match='first_match_break'):
        gev.cmc_from_search(qd, gd, qid, gid, qcam, gcam, topk=50, first_match_break=False)
