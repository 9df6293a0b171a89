"""Host-side contracts of the fused search (no device needed): the library's
constants, the workspace function (positive, non-decreasing in G, bounded at
the 1M-gallery shape, clamped segment counts), GalleryIndex.split's row
arithmetic, and rank_list(fused=True) on a backend without `search`."""
import numpy as np
import pytest
import torch


def test_search_library_constants():
    from pps_amd import _lib, ops
    L = _lib.lib()
    assert L.pps_search_max_k() == 256
    assert L.pps_search_h2_num_tiles() >= 1
    assert ops.search_max_k() == 256
    assert ops.search_num_tiles() == L.pps_search_h2_num_tiles()


_GS = [1, 255, 256, 257, 10 ** 4, 125000, 10 ** 6]


@pytest.mark.parametrize('Q,k', [(1, 1), (3368, 100), (10000, 100), (10000, 256)])
def test_search_workspace_monotone_in_G(Q, k):
    from pps_amd import ops
    for segments in (0, 1, 7):
        sizes = [ops.search_workspace_bytes(Q, G, k, segments) for G in _GS]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes


def test_search_workspace_bound_and_clamps():
    from pps_amd import ops
    # one eighth of the 5.0 GB block a 1M-gallery shard materialises today
    assert ops.search_workspace_bytes(10000, 10 ** 6, 100, 0) <= 625000000
    # segments beyond the clamps give the clamped value: 64 lists, 8192 / k
    # merged entries, the gallery's tile count
    assert ops.search_workspace_bytes(10000, 10 ** 6, 100, 1000) == \
        ops.search_workspace_bytes(10000, 10 ** 6, 100, 8192 // 100)
    assert ops.search_workspace_bytes(100, 10 ** 6, 16, 1000) == \
        ops.search_workspace_bytes(100, 10 ** 6, 16, 64)
    assert ops.search_workspace_bytes(100, 300, 16, 50) == \
        ops.search_workspace_bytes(100, 300, 16, 2)
    for bad in [(-1, 5, 1, 0), (5, -1, 1, 0), (5, 5, 0, 0), (5, 5, 257, 0), (5, 5, 1, -1)]:
        with pytest.raises(RuntimeError):
            ops.search_workspace_bytes(*bad)


@pytest.mark.parametrize('D', [32, 2048, 3968])
def test_gallery_split_rows(D):
    from pps_amd.ops import GalleryIndex
    # the default keeps one segment's two f16 planes under 2 GiB
    G = 3 * (2 ** 31) // (4 * D) + 5
    rows = GalleryIndex.split_rows(G, D)
    assert len(rows) >= 3
    at = 0
    for i, (a, n) in enumerate(rows):
        assert a == at and n > 0      # cumulative offsets
        at += n
        if i + 1 < len(rows):
            assert n % 16 == 0
        r16 = (n + 15) // 16 * 16
        assert 2 * r16 * D * 2 < 2 ** 31
    assert at == G
    # the default is the largest such multiple of 16
    n0 = rows[0][1]
    assert 2 * (n0 + 16) * D * 2 >= 2 ** 31
    # explicit max_rows: rounded down to whole 16-row blocks
    assert GalleryIndex.split_rows(1030, D, 400) == [(0, 400), (400, 400), (800, 230)]
    assert GalleryIndex.split_rows(1030, D, 410) == [(0, 400), (400, 400), (800, 230)]
    assert GalleryIndex.split_rows(10, D, 400) == [(0, 10)]
    assert [n for _, n in GalleryIndex.split_rows(100, D, 1)] == [16] * 6 + [4]


@pytest.mark.parametrize('G', [300, 20])
def test_rank_list_fused_without_search_backend(G):
    """The oracle's CpuBackend has no `search`: fused=True keeps the
    materialised path and returns the same lists."""
    from oracle.rank_counts import CpuBackend
    from pps_amd import distributed as pdist
    assert not hasattr(CpuBackend, 'search')
    rng = np.random.RandomState(3)
    Q, D, k = 12, 16, 50
    q = torch.from_numpy(rng.randn(Q, D).astype(np.float32))
    g = torch.from_numpy(rng.randn(G, D).astype(np.float32))
    qid, gid = rng.randint(0, 5, Q), rng.randint(0, 5, G)
    qcam, gcam = rng.randint(0, 3, Q), rng.randint(0, 3, G)
    sh = pdist.ShardedEvaluator(qid, qcam, gid, gcam, 0, 1, backend=CpuBackend)
    v0, i0 = sh.rank_list(q, g, k=k, fused=False)
    v1, i1 = sh.rank_list(q, g, k=k, fused=True)
    assert torch.equal(torch.as_tensor(i0), torch.as_tensor(i1))
    assert torch.equal(torch.as_tensor(v0), torch.as_tensor(v1))
