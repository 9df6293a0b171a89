"""GPU parity of the fused distance + top-k search (csrc/search_h2.hip,
ops.search): the rank list without the [Q, G] matrix.

The expected value is the materialised path on the same GalleryIndex,
ops.topk(ops.compute_dist(q, idx, metric=metric, math='h2'), k), and the
claim is equality of the bits (values) and of the indices: ragged shapes x
metrics x segment counts, every tile, adversarial inflow orders, ties across
tile and segment edges, degenerate rows, a segmented gallery, the fallbacks,
the workspace contract and the sharded rank list.  One independent check
against the NumPy oracle holds the distances to the project's 1e-4 bound."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import evaluator as ev

pytestmark = pytest.mark.gpu

METRICS = ['euclidean', 'sqeuclidean', 'cosine']


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _feats(seed, n, d):
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _expect(q, index, metric, k):
    """The materialised path, padded with (+inf, -1) past G entries."""
    from pps_amd import ops
    G = index.shape[0]
    kin = min(k, G)
    vals, idx = ops.topk(ops.compute_dist(q, index, metric=metric, math='h2'), kin)
    if kin < k:
        pv = torch.full((q.shape[0], k), float('inf'), dtype=torch.float32, device=q.device)
        pi = torch.full((q.shape[0], k), -1, dtype=torch.int32, device=q.device)
        pv[:, :kin], pi[:, :kin] = vals, idx
        vals, idx = pv, pi
    return vals, idx


def _same(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert torch.equal(got[1], want[1]), 'indices differ'
    # bit equality of the values (torch.equal would call NaN != NaN)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), 'values differ'


_RAGGED = [(1, 1, 32, 1), (3, 5, 64, 10), (37, 1000, 96, 100), (33, 2100, 64, 100),
           (300, 4099, 128, 21), (17, 2100, 32, 256), (20, 700, 2048, 50),
           (64, 1000, 3968, 100)]
_cache = {}


def _case(Q, G, D):
    """Features, index and the three metrics' expected lists, built once."""
    from pps_amd import ops
    key = (Q, G, D)
    if key not in _cache:
        q, g = _cuda(_feats(1, Q, D)), _cuda(_feats(2, G, D))
        _cache[key] = (q, ops.GalleryIndex(g, math='h2'), {})
    return _cache[key]


@pytest.mark.parametrize('segments', [0, 1, 2, 5])
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('Q,G,D,k', _RAGGED)
def test_search_ragged_shapes(Q, G, D, k, metric, segments):
    from pps_amd import ops
    q, index, want = _case(Q, G, D)
    if (metric, k) not in want:
        want[(metric, k)] = _expect(q, index, metric, k)
    got = ops.search(q, index, k, metric=metric, segments=segments)
    _same(got, want[(metric, k)])
    if k > G:   # the tail is the pad, the head the top-G
        assert torch.all(got[1][:, G:] == -1) and torch.all(torch.isinf(got[0][:, G:]))
        assert torch.all(got[1][:, :G] >= 0)


def test_search_every_tile_same_bits():
    from pps_amd import ops
    q, index, _ = _case(33, 2100, 64)
    want = _expect(q, index, 'euclidean', 100)
    assert ops.search_num_tiles() >= 1
    for tile in range(ops.search_num_tiles()):
        for segments in (1, 3):
            _same(ops.search(q, index, 100, segments=segments, tile=tile), want)
    with pytest.raises(RuntimeError):
        ops.search(q, index, 100, tile=ops.search_num_tiles())


@pytest.mark.parametrize('order', ['decreasing', 'increasing'])
def test_search_adversarial_order(order):
    """Gallery rows q0 + a_j noise_j: with a_j decreasing every later tile
    beats the whole list (worst-case inflow, a cut per tile); increasing,
    nothing passes after the first tile."""
    from pps_amd import ops
    G, D, k = 2100, 64, 100
    rng = np.random.RandomState(5)
    q = _feats(6, 9, D)
    a = np.linspace(2.0, 0.01, G) if order == 'decreasing' else np.linspace(0.01, 2.0, G)
    g = q[0][None] + a[:, None].astype(np.float32) * rng.randn(G, D).astype(np.float32) / np.sqrt(D)
    qd, index = _cuda(q), ops.GalleryIndex(_cuda(g), math='h2')
    for tile in range(ops.search_num_tiles()):
        _same(ops.search(qd, index, k, segments=1, tile=tile), _expect(qd, index, 'euclidean', k))


def test_search_all_ties():
    """600 copies of one row: every distance ties, the order is the index."""
    from pps_amd import ops
    D, k = 64, 100
    g = np.repeat(_feats(7, 1, D), 600, axis=0)
    q = _cuda(_feats(8, 5, D))
    index = ops.GalleryIndex(_cuda(g), math='h2')
    for segments in (0, 1, 2, 5):
        vals, idx = ops.search(q, index, k, segments=segments)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device='cuda').expand(5, k))
        assert torch.all(vals == vals[:, :1])


@pytest.mark.parametrize('metric', METRICS)
def test_search_ties_across_tile_and_segment_edges(metric):
    from pps_amd import ops
    D, k = 64, 40
    g = _feats(9, 1030, D)
    g[250:263] = g[3]
    g[1020:1030] = g[3]
    q = _feats(10, 12, D)
    q[0] = g[3]
    q[1] = g[3] + 0.01 * q[1]
    qd, index = _cuda(q), ops.GalleryIndex(_cuda(g), math='h2')
    want = _expect(qd, index, metric, k)
    for segments in (0, 1, 2, 5):
        for tile in range(ops.search_num_tiles()):
            _same(ops.search(qd, index, k, metric=metric, segments=segments, tile=tile), want)


@pytest.mark.parametrize('metric', ['euclidean', 'sqeuclidean'])
def test_search_degenerate_rows(metric):
    """An all-zero query and gallery row, rows scaled by 1e-20 and 1e20: equal
    to the materialised path wherever that path's distances are finite."""
    from pps_amd import ops
    D, k = 128, 30
    rng = np.random.RandomState(11)
    q = rng.randn(6, D).astype(np.float32)
    q[1] = 0
    q[2] *= 1e20
    q[3] *= 1e-20
    g = rng.randn(300, D).astype(np.float32)
    g[0] = 0
    g[3] *= 1e-20
    g[5] *= 1e20
    qd, index = _cuda(q), ops.GalleryIndex(_cuda(g), math='h2')
    wv, wi = _expect(qd, index, metric, k)
    for segments in (0, 1, 2):
        gv, gi = ops.search(qd, index, k, metric=metric, segments=segments)
        fin = torch.isfinite(wv)
        assert fin.any()
        assert torch.equal(gv[fin], wv[fin]) and torch.equal(gi[fin], wi[fin])
        full = torch.isfinite(ops.compute_dist(qd, index, metric=metric, math='h2')).all(1)
        assert torch.equal(gi[full], wi[full])


def test_search_vs_cpu_oracle():
    from pps_amd import ops
    Q, G, D, k = 16, 1500, 64, 50
    q, g = _feats(12, Q, D), _feats(13, G, D)
    d_ref = ev.compute_dist(q, g)
    vals, idx = ops.search(_cuda(q), _cuda(g), k)
    vals, idx = vals.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    err_sorted = np.abs(vals - np.sort(d_ref, 1)[:, :k]).max()
    err_at_idx = np.abs(np.take_along_axis(d_ref, idx, 1) - vals).max()
    print('search vs oracle: sorted %.3g, at idx %.3g' % (err_sorted, err_at_idx))
    assert idx.min() >= 0 and idx.max() < G
    assert err_sorted <= 1e-4
    assert err_at_idx <= 1e-4


def test_search_segmented_gallery():
    from pps_amd import ops
    D, k = 64, 40
    g = _feats(9, 1030, D)
    g[250:263] = g[3]
    g[1020:1030] = g[3]
    q = _feats(10, 12, D)
    q[0] = g[3]
    qd, gd = _cuda(q), _cuda(g)
    parts = ops.GalleryIndex.split(gd, max_rows=400)
    assert [p.shape[0] for p in parts] == [400, 400, 230]
    want = ops.search(qd, ops.GalleryIndex(gd, math='h2'), k)
    got = ops.search(qd, parts, k)
    _same(got, want)
    assert int(got[1].max()) >= 800   # global indices: the last segment is reached
    # more lists than one merge call takes: merged in rounds
    many = ops.GalleryIndex.split(gd, max_rows=16)
    assert len(many) == 65
    _same(ops.search(qd, many, k), want)
    _same(ops.search(qd, many, 200), ops.search(qd, ops.GalleryIndex(gd, math='h2'), 200))


def test_search_fallbacks():
    from pps_amd import ops
    rng = np.random.RandomState(14)
    # D % 32 != 0: the index holds an x3 split, also when 'h2' was asked for
    q, g = _cuda(rng.randn(7, 20)), _cuda(rng.randn(90, 20))
    index = ops.GalleryIndex(g, math='h2')
    assert index.math == 'x3'
    want = ops.topk(ops.compute_dist(q, index), 10)
    _same(ops.search(q, index, 10), want)
    _same(ops.search(q, g, 10), want)
    v, i = ops.search(q, index, 100)   # k > G on the fallback: padded the same way
    assert torch.equal(i[:, :90], ops.topk(ops.compute_dist(q, index), 90)[1])
    assert torch.all(i[:, 90:] == -1) and torch.all(torch.isinf(v[:, 90:]))
    # a strided query view
    big = _cuda(_feats(15, 9, 128))
    qs = big[:, :64]
    assert not qs.is_contiguous()
    index = ops.GalleryIndex(_cuda(_feats(16, 500, 64)), math='h2')
    qc = qs.contiguous()
    _same(ops.search(qs, index, 20), ops.topk(ops.compute_dist(qc, index), 20))
    # k beyond the fused kernel's
    assert ops.search_max_k() == 256
    _same(ops.search(qc, index, 300), ops.topk(ops.compute_dist(qc, index, math='h2'), 300))


def test_search_workspace_contract():
    from pps_amd import _lib, ops
    Q, G, D, k = 33, 2100, 64, 100
    q, index, _ = _case(Q, G, D)
    want = _expect(q, index, 'euclidean', k)
    need = ops.search_workspace_bytes(Q, G, k, 2)
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
    _same(ops.search(q, index, k, segments=2, workspace=ws), want)
    _same(ops.search(q, index, k, segments=2, workspace=ws), want)   # reused
    with pytest.raises(RuntimeError):
        ops.search(q, index, k, segments=2, workspace=ws[:need - 1])
    # the C entry itself: one byte short is PPS_ERR_CAPACITY, nothing launched
    q2, qrs, qsq = ops.split_h2_tiled(q)
    g2, grs, gsq = index.h2
    vals = torch.full((Q, k), -7.0, dtype=torch.float32, device='cuda')
    idx = torch.full((Q, k), -7, dtype=torch.int32, device='cuda')
    L = _lib.lib()
    rc = L.pps_search_h2_tiled(q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(), g2.data_ptr(),
                               gsq.data_ptr(), grs.data_ptr(), G, D, 0, k, 2, 0, ws.data_ptr(),
                               need - 1, vals.data_ptr(), idx.data_ptr(),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -4   # PPS_ERR_CAPACITY
    assert torch.all(vals == -7.0) and torch.all(idx == -7)
    # degenerate calls
    e_v, e_i = ops.search(q[:0], index, k)
    assert e_v.shape == (0, k) and e_i.shape == (0, k)
    rc = L.pps_search_h2_tiled(q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(), g2.data_ptr(),
                               gsq.data_ptr(), grs.data_ptr(), 0, D, 0, k, 0, 0, None, 0,
                               vals.data_ptr(), idx.data_ptr(),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.all(idx == -1) and torch.all(torch.isinf(vals))


@pytest.mark.parametrize('G', [1200, 60])
def test_search_sharded_rank_list(G):
    """World 1: rank_list(fused=True) equals the materialised rank list; at
    G = 60 < k the short-shard padding path is taken."""
    from pps_amd import distributed as pdist
    Q, D, k = 40, 96, 100
    rng = np.random.RandomState(17)
    q, g = _cuda(_feats(18, Q, D)), _cuda(_feats(19, G, D))
    qid, gid = rng.randint(0, 10, Q), rng.randint(0, 10, G)
    qcam, gcam = rng.randint(0, 3, Q), rng.randint(0, 3, G)
    sh = pdist.ShardedEvaluator(qid, qcam, gid, gcam, 0, 1)
    want = sh.rank_list(q, g, k=k, fused=False)
    got = sh.rank_list(q, g, k=k, fused=True)
    _same(got, want)
    if G < k:
        assert torch.all(got[1][:, G:] == -1)
