"""Host-side parts of the group-excluding search (no device needed):
ops.exclusion_groups, ShardedEvaluator.rank_list(exclude=...) on the oracle's
CpuBackend (which has neither `search` nor `topk_excluding`), and the
first-match booking behind reid_dataset_evaluator.cmc_from_search."""
import numpy as np
import pytest
import torch

from oracle import evaluator as ev


@pytest.mark.parametrize('by', ['id_cam', 'cam'])
def test_exclusion_groups_codes(by):
    from pps_amd import ops
    rng = np.random.RandomState(1)
    qid, qcam = rng.randint(-3, 40, 50) * 1000003, rng.randint(0, 7, 50)
    gid, gcam = rng.randint(-3, 40, 400) * 1000003, rng.randint(0, 7, 400)
    qg, gg = ops.exclusion_groups(qid, qcam, gid, gcam, by=by, device='cpu')
    assert qg.dtype == torch.int32 and gg.dtype == torch.int32
    assert qg.shape == (50,) and gg.shape == (400,)
    assert int(qg.min()) >= 0 and int(gg.min()) >= 0
    same = qcam[:, None] == gcam[None, :]
    if by == 'id_cam':
        same &= qid[:, None] == gid[None, :]
    assert same.any() and not same.all()
    assert np.array_equal(qg.numpy()[:, None] == gg.numpy()[None, :], same)
    # torch tensors and lists are taken as well
    qg2, gg2 = ops.exclusion_groups(torch.from_numpy(qid), list(qcam), gid, torch.from_numpy(gcam),
                                    by=by, device='cpu')
    assert torch.equal(qg, qg2) and torch.equal(gg, gg2)


@pytest.mark.parametrize('by', ['id_cam', 'cam'])
def test_exclusion_groups_empty_sets(by):
    from pps_amd import ops
    ids, cams = np.array([4, 4, 9]), np.array([1, 2, 1])
    none = np.zeros(0, np.int64)
    qg, gg = ops.exclusion_groups(none, none, ids, cams, by=by, device='cpu')
    assert qg.shape == (0,) and gg.shape == (3,) and qg.dtype == torch.int32
    assert int(gg.min()) >= 0
    qg, gg = ops.exclusion_groups(ids, cams, none, none, by=by, device='cpu')
    assert qg.shape == (3,) and gg.shape == (0,) and gg.dtype == torch.int32
    qg, gg = ops.exclusion_groups(none, none, none, none, by=by, device='cpu')
    assert qg.shape == (0,) and gg.shape == (0,)
    with pytest.raises(RuntimeError):
        ops.exclusion_groups(ids, cams, ids, cams, by='id', device='cpu')


def _numpy_rank_list(dist, k, excluded):
    """Stable argsort, drop the excluded, first k, pad."""
    Q = dist.shape[0]
    vals = np.full((Q, k), np.inf, np.float32)
    idx = np.full((Q, k), -1, np.int32)
    for r in range(Q):
        order = np.argsort(dist[r], kind='stable')
        order = order[~excluded[r][order]][:k]
        vals[r, :len(order)] = dist[r][order]
        idx[r, :len(order)] = order
    return vals, idx


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('exclude', ['id_cam', 'cam'])
@pytest.mark.parametrize('G', [300, 20])
def test_rank_list_exclude_cpu_backend(G, exclude, fused):
    from oracle.rank_counts import CpuBackend
    from pps_amd import distributed as pdist
    assert not hasattr(CpuBackend, 'search') and not hasattr(CpuBackend, 'topk_excluding')
    rng = np.random.RandomState(3)
    Q, D, k = 12, 16, 50
    q = rng.randn(Q, D).astype(np.float32)
    g = rng.randn(G, D).astype(np.float32)
    g[5] = g[2]   # a tie: the order is the index
    qid, gid = rng.randint(0, 5, Q), rng.randint(0, 5, G)
    qcam, gcam = rng.randint(0, 3, Q), rng.randint(0, 3, G)
    sh = pdist.ShardedEvaluator(qid, qcam, gid, gcam, 0, 1, backend=CpuBackend)
    vals, idx = sh.rank_list(torch.from_numpy(q), torch.from_numpy(g), k=k, fused=fused,
                             exclude=exclude)
    excluded = qcam[:, None] == gcam[None, :]
    if exclude == 'id_cam':
        excluded &= qid[:, None] == gid[None, :]
    dist = CpuBackend.distmat(torch.from_numpy(q), torch.from_numpy(g), 'euclidean').numpy()
    wv, wi = _numpy_rank_list(dist, k, excluded)
    assert np.array_equal(np.asarray(idx), wi)
    assert np.array_equal(np.asarray(vals), wv)
    assert excluded.any() and ((wi == -1).any() == (G < k))
    # exclude=None is the list as it was
    v0, i0 = sh.rank_list(torch.from_numpy(q), torch.from_numpy(g), k=k)
    pv, pi = _numpy_rank_list(dist, k, np.zeros_like(excluded))
    assert np.array_equal(np.asarray(i0), pi) and np.array_equal(np.asarray(v0), pv)
    with pytest.raises(RuntimeError):
        sh.rank_list(torch.from_numpy(q), torch.from_numpy(g), k=k, exclude='id')


def test_first_match_cmc_hand_made():
    """A 5 x 8 matrix by hand: lists written down from it, then booked."""
    from pps_amd import reid_dataset_evaluator as gev
    gid = np.array([1, 1, 2, 2, 3, 3, 1, 4])
    gcam = np.array([0, 1, 0, 1, 0, 1, 2, 0])
    qid = np.array([1, 2, 3, 5, 4])
    qcam = np.array([0, 0, 1, 0, 0])
    dist = np.array([
        [0.1, 0.9, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7],    # junk 0 first; match 6 after 2, 3, 4, 5
        [0.5, 0.6, 0.1, 0.2, 0.3, 0.4, 0.7, 0.8],    # junk 2 first; match 3 at once
        [0.1, 0.2, 0.3, 0.4, 0.5, 0.05, 0.6, 0.7],   # junk 5 first; match 4 after 0, 1, 2, 3
        [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8],    # id 5: not in the gallery
        [0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.1],    # id 4: its only row is junk
    ])
    topk = 4
    ref, ref_valid = ev.cmc(dist, qid, gid, qcam, gcam, topk=topk, first_match_break=True,
                            average=False)
    assert ref_valid.tolist() == [1, 1, 1, 0, 0]
    # the lists an excluding search of depth topk returns for the junk rule
    lists = np.array([[2, 3, 4, 5], [3, 4, 5, 0], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]])
    ret = gev.first_match_cmc(lists, qid, gid, ref_valid, topk)
    assert np.array_equal(ret, ref)
    assert ret[0].tolist() == [0, 0, 0, 0] and ret[1].tolist() == [1, 1, 1, 1]   # past topk / first
    # deeper lists are cut at topk; pads never match; shallower ones are refused
    deep = np.concatenate([lists, np.full((5, 2), -1)], axis=1)
    assert np.array_equal(gev.first_match_cmc(deep, qid, gid, ref_valid, topk), ref)
    pads = np.full((5, topk), -1)
    assert not gev.first_match_cmc(pads, qid, gid, ref_valid, topk).any()
    with pytest.raises(ValueError):
        gev.first_match_cmc(lists[:, :3], qid, gid, ref_valid, topk)
    # an invalid query books nothing even if its id shows up in its list
    ret = gev.first_match_cmc(np.array([[7, 0, 1, 2]]), qid[4:], gid, [False], topk)
    assert not ret.any()
    # depth 8 = the whole gallery: every valid query books its hit
    ref8, _ = ev.cmc(dist, qid, gid, qcam, gcam, topk=8, first_match_break=True, average=False)
    lists8 = np.full((5, 8), -1)
    for r in range(5):
        order = np.argsort(dist[r], kind='stable')
        keep = order[~((gid[order] == qid[r]) & (gcam[order] == qcam[r]))]
        lists8[r, :len(keep)] = keep
    assert np.array_equal(gev.first_match_cmc(lists8, qid, gid, ref_valid, 8), ref8)
    assert ref8[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


def test_cmc_from_search_rejects_fractional_mode():
    from pps_amd import reid_dataset_evaluator as gev
    with pytest.raises(RuntimeError, match='first_match_break'):
        gev.cmc_from_search(np.zeros((2, 32), np.float32), np.zeros((3, 32), np.float32),
                            [1, 2], [1, 2, 3], [0, 0], [1, 1, 1], first_match_break=False)
