"""Re-ranking query batches against a gallery prepared once:
ops.RerankGallery(g).re_rank(q) against
ops.re_ranking_from_features(cat([q, g]), Q), bit for bit, and the two-part
pair distances against the gathered matrix.

Data follows test_gpu_rerank_features: identity centroids plus 2.5 sigma noise,
rows normalised, seeded.  Every comparison is torch.equal."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILES = (1, 2)          # 256 x 256 two-stage, 192 x 192 three-stage
SHAPE = (150, 650, 64, 60, 7)     # Q, G, D, ids, seed


def _feats(n_ids, ids, D, seed, noise=2.5):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    cent = torch.randn((n_ids + 1, D), generator=gen, device='cuda')
    x = cent[torch.from_numpy(np.asarray(ids)).cuda()] + \
        noise * torch.randn((len(ids), D), generator=gen, device='cuda')
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _ids(Q, G, n_ids, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(1, n_ids + 1, Q + G)


@functools.lru_cache(maxsize=None)
def _x(Q, G, D, n_ids, seed):
    """[queries; gallery] of one seeded shape, computed once and left unchanged."""
    return _feats(n_ids, _ids(Q, G, n_ids, seed), D, seed)


def _split(x, Q):
    return x[:Q].contiguous(), x[Q:].contiguous()


@functools.lru_cache(maxsize=None)
def _ref(k1, k2, metric):
    """The features path on SHAPE (default tile and segments; its own tests pin
    that every tile / segments choice gives these bits)."""
    from pps_amd import ops
    return ops.re_ranking_from_features(_x(*SHAPE), SHAPE[0], k1, k2, 0.3, metric=metric)


@functools.lru_cache(maxsize=None)
def _gallery(k1, metric, tile=0, segments=0):
    from pps_amd import ops
    return ops.RerankGallery(_split(_x(*SHAPE), SHAPE[0])[1], k1=k1, metric=metric, tile=tile,
                             segments=segments)


# ------------------------------------------------------------ 1. prepared == features path
@pytest.mark.parametrize('segments', [0, 3])
@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
@pytest.mark.parametrize('k1,k2', [(20, 6), (6, 3)])
def test_prepared_equals_the_features_path(k1, k2, metric, tile, segments):
    Q, G = SHAPE[:2]
    q, _ = _split(_x(*SHAPE), Q)
    rg = _gallery(k1, metric, tile, segments)
    assert tuple(rg.nn_vals.shape) == (G, k1 + 1) and tuple(rg.nn_idx.shape) == (G, k1 + 1)
    assert tuple(rg.rowmax.shape) == (G,) and rg.k1 == k1 and rg.metric == metric
    got = rg.re_rank(q, k2=k2, segments=segments, tile=tile)
    assert tuple(got.shape) == (Q, G)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _ref(k1, k2, metric))


def test_gallery_index_in_place_of_the_features():
    from pps_amd import ops
    Q = SHAPE[0]
    q, g = _split(_x(*SHAPE), Q)
    index = ops.GalleryIndex(g, math='h2')
    rg = ops.RerankGallery(index)
    assert rg.index is index
    assert torch.equal(rg.re_rank(q), _ref(20, 6, 'euclidean'))


# ------------------------------------------------------------ 2. prefix property
@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
def test_a_gallery_prepared_for_k1_20_serves_k1_6(metric):
    Q = SHAPE[0]
    q, _ = _split(_x(*SHAPE), Q)
    rg = _gallery(20, metric)
    assert rg.nn_vals.shape[1] == 21          # the row stride exceeds k1 + 1 = 7
    assert torch.equal(rg.re_rank(q, k1=6, k2=3), _ref(6, 3, metric))


# ------------------------------------------------------------ 3. ties across the parts
@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
@pytest.mark.parametrize('kind', ['gallery_x3', 'queries_are_gallery_rows', 'duplicated_queries'])
def test_ties_across_the_parts(kind, metric):
    """Exact ties inside the gallery part, between a query column and a gallery
    column, and inside the query part: the merge must order them by global
    index as the one search over all columns does."""
    from pps_amd import ops
    Q, Gb, D = 150, 217, 64
    x = _feats(60, _ids(Q, Gb, 60, 8), D, 8)
    q, g = x[:Q], x[Q:]
    if kind == 'gallery_x3':
        g = g.repeat(3, 1)
    elif kind == 'queries_are_gallery_rows':
        g = g.repeat(3, 1)[:650]
        q = torch.cat([g[5:80], q[:75]])          # 75 exact copies of gallery rows
    else:
        g = g.repeat(3, 1)[:650]
        q = torch.cat([q[:50], q[:50], q[:50]])   # every query three times
    q, g = q.contiguous(), g.contiguous()
    ref = ops.re_ranking_from_features(torch.cat([q, g]), Q, metric=metric)
    for tile in TILES:
        rg = ops.RerankGallery(g, metric=metric, tile=tile)
        assert torch.equal(rg.re_rank(q, tile=tile), ref)


# ------------------------------------------------------------ 4. Q < k1 + 1
@pytest.mark.parametrize('Q', [5, 1])
def test_fewer_queries_than_neighbours(Q):
    """The query-column lists are padded with (+inf, -1); the merge skips the pads."""
    from pps_amd import ops
    x = _x(*SHAPE)
    q, g = x[:Q].contiguous(), x[SHAPE[0]:].contiguous()
    ref = ops.re_ranking_from_features(torch.cat([q, g]), Q)
    assert torch.equal(_gallery(20, 'euclidean').re_rank(q), ref)


# ------------------------------------------------------------ 5. gallery windows
@pytest.mark.parametrize('g_window', [0, 256, 100])
def test_gallery_windows_give_one_windows_bits(g_window):
    Q = SHAPE[0]
    q, _ = _split(_x(*SHAPE), Q)
    got = _gallery(20, 'euclidean').re_rank(q, g_window=g_window)
    assert torch.equal(got, _ref(20, 6, 'euclidean'))


# ------------------------------------------------------------ 6. one gallery, two batches
def test_two_batches_against_one_gallery_leave_it_unchanged():
    from pps_amd import ops
    Q, G, D = SHAPE[:3]
    x = _x(*SHAPE)
    q1, g = _split(x, Q)
    q2 = _feats(60, _ids(93, 0, 60, 31), D, 31)            # another batch, another size
    rg = ops.RerankGallery(g)
    before = (rg.nn_vals.clone(), rg.nn_idx.clone(), rg.rowmax.clone())
    for q in (q1, q2, q1):
        ref = ops.re_ranking_from_features(torch.cat([q, g]), q.shape[0])
        assert torch.equal(rg.re_rank(q), ref)
    assert torch.equal(rg.nn_vals, before[0]) and torch.equal(rg.nn_idx, before[1])
    assert torch.equal(rg.rowmax, before[2])


# ------------------------------------------------------------ 7. two-part pair distances
@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
@pytest.mark.parametrize('D', [32, 96, 160])
def test_two_part_pair_dist_equals_the_gathered_matrix(D, metric):
    from pps_amd import ops
    Q, G, cap = 37, 203, 130         # rows 32..36 and 192..202: a ragged last 16-row block each
    N = Q + G
    x = _feats(20, _ids(Q, G, 20, 5), D, 5)
    q, g = _split(x, Q)
    W = ops.compute_dist(x, ops.GalleryIndex(x, math='h2'), metric=metric, math='h2',
                         symmetric=False)
    qi, gi = ops.GalleryIndex(q, math='h2'), ops.GalleryIndex(g, math='h2')
    rng = np.random.RandomState(D)
    cnt_of = np.array([0, 1, 63, 64, 65, cap, cap + 70], np.int32)
    for rows, a, r0 in ((Q, q, 0), (G, g, Q)):      # a-rows from the query part, the gallery part
        lists = rng.randint(0, N, (rows, cap)).astype(np.int32)   # both parts in every list
        lists[:, 0:4] = [0, Q - 1, Q, N - 1]         # the ends of both parts
        lists[:, 5] = lists[:, 4]                    # repeats
        lists[::3, 64] = lists[::3, 63]
        lists[:, 6] = -3                             # clamped to column 0
        lists[:, 7] = N + 11                         # clamped to column N - 1
        lists[1::2, 63] = N                          # the first index past the end
        counts = cnt_of[np.arange(rows) % 7]
        lt, ct = torch.from_numpy(lists).cuda(), torch.from_numpy(counts).cuda()
        out = ops.pair_dist(a, (qi, gi), lt, ct, metric=metric)
        live = torch.arange(cap, device='cuda')[None, :] < ct.clamp(max=cap)[:, None]
        cols = lt.long().clamp(0, N - 1)
        gathered = W[r0:r0 + rows].gather(1, cols)
        assert torch.equal(out, torch.where(live, gathered, torch.zeros_like(out)))
        # counts = None: every entry
        assert torch.equal(ops.pair_dist(a, (qi, gi), lt, None, metric=metric), gathered)


# ------------------------------------------------------------ 8. evaluator
def _eval_data():
    rng = np.random.RandomState(21)
    Q, G, MQ, D, n_ids = 120, 500, 180, 64, 40
    ids = rng.randint(1, n_ids + 1, Q + G + MQ)
    cams = rng.randint(1, 4, Q + G + MQ)
    marks = np.concatenate([np.zeros(Q, int), np.ones(G, int), np.full(MQ, 2)])
    perm = rng.permutation(Q + G + MQ)
    feat = _feats(n_ids, ids, D, 21)
    return feat[torch.from_numpy(perm).cuda()].contiguous(), ids[perm], cams[perm], marks[perm]


def test_evaluator_builds_one_gallery_and_keeps_the_scores(monkeypatch):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    from pps_amd.config import cfg
    feat, ids, cams, marks = _eval_data()
    q, g, mq = marks == 0, marks == 1, marks == 2
    qf = feat[torch.from_numpy(np.nonzero(q)[0]).cuda()]
    gf = feat[torch.from_numpy(np.nonzero(g)[0]).cuda()]

    def scores(rows, r_ids, r_cams):
        rr = ops.re_ranking_from_features(torch.cat([rows, gf]).contiguous(), len(rows))
        ap, valid, first = gev.rank_eval(rr, r_ids, ids[g], r_cams, cams[g])
        return gev.scores_from_ranks(ap, valid, first, topk=10)

    mAP, cmc = scores(qf, ids[q], cams[q])
    groups = OrderedDict()
    for k, key in enumerate(zip(ids[mq], cams[mq])):
        groups.setdefault(key, []).append(k)
    mq_rows = np.nonzero(mq)[0]
    pooled = ops.group_mean(feat, [mq_rows[v] for v in groups.values()])
    keys = np.array(list(groups.keys()))
    mq_mAP, mq_cmc = scores(pooled, keys[:, 0], keys[:, 1])

    built, direct = [], []
    real_init = ops.RerankGallery.__init__

    def counting_init(self, *a, **kw):
        built.append(1)
        real_init(self, *a, **kw)

    def counting_direct(*a, **kw):
        direct.append(1)
        raise AssertionError('evaluate_arrays called ops.re_ranking_from_features')

    monkeypatch.setattr(ops.RerankGallery, '__init__', counting_init)
    monkeypatch.setattr(ops, 're_ranking_from_features', counting_direct)
    monkeypatch.setattr(cfg.REID, 'RERANK', True)
    got = gev.evaluate_arrays(feat, ids, cams, marks, verbose=False, rerank_from_features=True)
    assert len(built) == 1 and not direct
    assert got[0] == mAP and np.array_equal(np.asarray(got[1]), np.asarray(cmc))
    assert got[2] == mq_mAP and np.array_equal(np.asarray(got[3]), np.asarray(mq_cmc))


def test_numpy_in_numpy_out_through_the_wrapper():
    from pps_amd import reid_dataset_evaluator as gev
    Q = SHAPE[0]
    q, _ = _split(_x(*SHAPE), Q)
    want = _ref(20, 6, 'euclidean')
    rg = _gallery(20, 'euclidean')
    out = gev.re_ranking_from_features(q.cpu().numpy(), rg)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want.cpu().numpy())
    out = gev.re_ranking_from_features(q, rg)
    assert isinstance(out, torch.Tensor) and torch.equal(out, want)
    out = gev.re_ranking_from_features(q, rg, k1=6, k2=3)
    assert torch.equal(out, _ref(6, 3, 'euclidean'))


# ------------------------------------------------------------ 9. refusals
def test_prepared_path_refuses_what_it_cannot_run(monkeypatch):
    """Each refusal raises before anything of [N, N] size exists: with every
    operand built beforehand, the peak allocation over all of them stays below
    one matrix (4 N^2 bytes)."""
    from pps_amd import ops
    Q, G = SHAPE[:2]
    N = Q + G
    q, g = _split(_x(*SHAPE), Q)
    rg, rg6 = _gallery(20, 'euclidean'), _gallery(6, 'euclidean')
    narrow, strided = g[:, :40].contiguous(), g[:, :32]
    x3_index = ops.GalleryIndex(g, math='x3')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match='re_ranking_rows'):
        ops.RerankGallery(narrow)                                # D % 32 != 0
    with pytest.raises(RuntimeError, match='re_ranking_rows'):
        ops.RerankGallery(strided)                               # strided
    with pytest.raises(RuntimeError, match='re_ranking_rows'):
        rg.re_rank(q[:, :32])                                    # strided queries, wrong width
    with pytest.raises(RuntimeError, match='above the prepared'):
        rg.re_rank(q, k1=21)
    with pytest.raises(RuntimeError, match='above the prepared'):
        rg6.re_rank(q, k1=20)
    monkeypatch.setenv('PPS_DIST_MATH', 'x3')
    with pytest.raises(RuntimeError, match='re_ranking_rows'):
        ops.RerankGallery(g)                                     # arithmetic not h2
    with pytest.raises(RuntimeError, match='re_ranking_rows'):
        ops.RerankGallery(x3_index)                              # an x3 index
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak < 4 * N * N, (peak, 4 * N * N)
