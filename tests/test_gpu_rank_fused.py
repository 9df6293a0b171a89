"""Matrix-free mAP: the pair kernel (ops.collect_matches_h2), the fused
distance + count kernel (ops.rank_count_h2) and everything built on them
(ops.rank_eval_fused, the *_from_features evaluators, ShardedEvaluator.run(
fused=True)) against the materialised path on the matrix of
compute_dist(q, g, math='h2', symmetric=False).  Every distance the fused
kernels compute has that matrix's bits, so every comparison here is an
equality: list entries as (distance bits, index), counts as integers, AP as
float64 bits.  Features are seeded normalised Gaussians; the labels (and a few
copied gallery rows) are built so that the edge cases named at each test
occur.  References are computed once per metric and shared."""
import functools

import numpy as np
import pytest
import torch
from _parity import check_rank_metrics

pytestmark = pytest.mark.gpu

METRICS = ('euclidean', 'sqeuclidean', 'cosine')
CAPACITY = -4


def _normed(n, D, gen):
    x = torch.randn((n, D), generator=gen, device='cuda')
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _matrix(q, g, metric):
    from pps_amd import ops
    return ops.compute_dist(q, g, metric=metric, math='h2', symmetric=False, pad_rows=True)


def _assert_rank_equal(got, ref):
    (ap, valid, first), (ap1, valid1, first1) = got, ref
    np.testing.assert_array_equal(valid.cpu().numpy(), valid1.cpu().numpy())
    np.testing.assert_array_equal(first.cpu().numpy(), first1.cpu().numpy())
    np.testing.assert_array_equal(ap.cpu().numpy().view(np.int64),
                                  ap1.cpu().numpy().view(np.int64))


# ---------------------------------------------------------------- 1. pair kernel
PQ, PG, POFF = 37, 531, 1000


@functools.lru_cache(maxsize=None)
def _pair_labels():
    """Identity 1: 70 gallery rows (more than one 64-member trip), identity 2:
    20 (more than one 16-column block), identity 5: every row on the query's
    camera (all junk), identity 99: no gallery row."""
    rng = np.random.RandomState(5)
    gid = rng.randint(10, 40, PG)
    gcam = rng.randint(1, 7, PG)
    rows = rng.permutation(PG)
    gid[rows[:70]] = 1
    gid[rows[70:90]] = 2
    gid[rows[90:96]] = 5
    gcam[rows[90:96]] = 4
    qid = rng.randint(10, 40, PQ)
    qcam = rng.randint(1, 7, PQ)
    qid[:4] = [1, 2, 5, 99]
    qcam[2] = 4
    return qid, qcam, gid, gcam


@functools.lru_cache(maxsize=None)
def _pair_data(D):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(100 + D)
    return _normed(PQ, D, gen), _normed(PG, D, gen)


def _list_sets(d, idx, cnt):
    d, idx, cnt = _bits(d), idx.cpu().numpy(), cnt.cpu().numpy()
    return [set(zip(d[i, :n].tolist(), idx[i, :n].tolist()))
            for i, n in enumerate(np.minimum(cnt, d.shape[1]))]


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('D', [32, 96, 160])   # one chunk; odd chunk counts
def test_collect_matches_h2_equals_collect_matches(D, metric):
    from pps_amd import ops
    qid, qcam, gid, gcam = _pair_labels()
    q, g = _pair_data(D)
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    assert mi.capacity == 70
    dist = _matrix(q, g, metric)
    q_split, index = ops.split_h2_tiled(q), ops.GalleryIndex(g, math='h2')
    for pmax in (None, 8):   # 8: shorter than identity 1's and 2's lists (clipping)
        pd, pi, pc, (jd, ji, jc) = ops.collect_matches_h2(q_split, index, mi, metric, POFF, pmax)
        rd, ri, rc, (rjd, rji, rjc) = ops.collect_matches(dist, mi, POFF, pmax)
        np.testing.assert_array_equal(pc.cpu().numpy(), rc.cpu().numpy())
        np.testing.assert_array_equal(jc.cpu().numpy(), rjc.cpu().numpy())
        assert _list_sets(pd, pi, pc) == _list_sets(rd, ri, rc)
        assert _list_sets(jd, ji, jc) == _list_sets(rjd, rji, rjc)
    pc, jc = pc.cpu().numpy(), jc.cpu().numpy()
    assert pc[0] > 8 and pc[0] + jc[0] == 70 and pc[1] + jc[1] == 20   # clipped lists
    assert pc[2] == 0 and jc[2] == 6                                   # all junk
    assert pc[3] == 0 and jc[3] == 0                                   # no member
    assert int(pi.cpu().numpy()[0, 0]) >= POFF                         # global indices


# ---------------------------------------------------------------- 2. count kernel
CQ, CG, CD = 300, 1100, 64
# column pairs on both sides of a tile edge (192 k, 256 k) or a segment edge
# (segments=3: columns 384 / 768 with the 192 tile, 512 / 1024 with the 256 tile)
EDGES = [(191, 192), (255, 256), (383, 384), (511, 512), (767, 768), (1023, 1024)]


@functools.lru_cache(maxsize=None)
def _count_data():
    """Q = 300, G = 1100, D = 64 (two ragged panels, five or six ragged tiles).
    Rows 0..39 and 1060..1099 are filler (identities no query has) that the
    constructed ties are copied into."""
    from pps_amd import ops
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11)
    g, q = _normed(CG, CD, gen), _normed(CQ, CD, gen)
    rng = np.random.RandomState(11)
    gid = (np.arange(CG) % 90) + 1          # about 12 rows per identity
    gcam = rng.randint(1, 7, CG)
    qid = rng.randint(1, 91, CQ)
    qcam = rng.randint(1, 7, CQ)
    fill = np.r_[0:40, 1060:1100]
    gid[fill] = 5000 + fill
    # identity 200: 150 positives (lists over more than one 64-lane register) + 30 junk
    big = np.arange(800, 980)
    gid[big] = 200
    gcam[big[:150]] = 2 + np.arange(150) % 5
    gcam[big[150:]] = 1
    qid[0:6], qcam[0:6] = 200, 1
    qid[6:9] = 999                          # P == 0: no gallery row at all
    gid[100:105], gcam[100:105] = 300, 3    # P == 0: every member is junk
    qid[9:11], qcam[9:11] = 300, 3
    # equal distances on both sides of a tile / segment edge: the query sits
    # next to row a, row b is a copy of it; even pairs tie two positives, odd
    # pairs the first positive with a valid non-match at the higher index
    for k, (a, b) in enumerate(EDGES):
        i = 30 + k
        x = g[a] + 0.05 * q[i]
        q[i] = x / x.norm()
        g[b] = g[a]
        qid[i], qcam[i] = 400 + k, 1
        gid[[a, a + 5, a + 9]] = 400 + k
        gcam[[a, a + 5, a + 9]] = 2
        if k % 2 == 0:
            gid[b], gcam[b] = 400 + k, 3
    # copies of a query's nearest positive: queries 12..21 get one at a lower
    # and one at a higher index (valid non-matches: `before`'s index rule),
    # queries 22..29 one that is junk (its id and camera)
    d0 = _matrix(q, g, 'euclidean').cpu().numpy()
    tied = []
    for i in range(12, 30):
        pos = np.nonzero((gid == qid[i]) & (gcam != qcam[i]))[0]
        if len(pos) == 0:
            continue
        c = int(pos[np.lexsort((pos, d0[i, pos]))[0]])
        if i < 22:
            lo, hi = i - 12, 1060 + i - 12
            g[lo] = g[c]
            g[hi] = g[c]
            tied.append((i, c, lo, hi))
        else:
            row = 20 + i - 22
            g[row] = g[c]
            gid[row], gcam[row] = qid[i], qcam[i]
    assert len(tied) >= 5
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    assert mi.capacity == 180
    return dict(q=q, g=g, qid=qid, qcam=qcam, gid=gid, gcam=gcam, mi=mi, tied=tied,
                q_split=ops.split_h2_tiled(q), index=ops.GalleryIndex(g, math='h2'))


@functools.lru_cache(maxsize=None)
def _count_ref(metric):
    """The materialised path on the h2 matrix: lists, sorted positives, counts."""
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _count_data()
    dist = _matrix(c['q'], c['g'], metric)
    pd, pi, pc, junk = ops.collect_matches(dist, c['mi'])
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    hist, before = ops.rank_count_stream(dist, 0, sp, junk)
    rank = gev.rank_eval(dist, c['qid'], c['gid'], c['qcam'], c['gcam'])
    return dict(dist=dist, sp=sp, junk=junk, hist=hist, before=before, rank=rank)


def test_count_data_holds_the_constructed_ties():
    c, r = _count_data(), _count_ref('euclidean')
    d = _bits(r['dist'])
    for i, col, lo, hi in c['tied']:
        assert d[i, lo] == d[i, col] == d[i, hi] and lo < col < hi
    for k, (a, b) in enumerate(EDGES):
        assert d[30 + k, a] == d[30 + k, b]
    ptot = r['sp'].pos_total.cpu().numpy()
    assert ptot[0] == 150 and (ptot[6:11] == 0).all() and r['sp'].sorted_d.shape[1] == 180


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('segments', [0, 1, 3])
@pytest.mark.parametrize('tile', [1, 2])
def test_rank_count_h2_equals_rank_count_stream(tile, segments, metric):
    from pps_amd import ops
    c, r = _count_data(), _count_ref(metric)
    hist, before = ops.rank_count_h2(c['q_split'], c['index'], 0, r['sp'], r['junk'], metric,
                                     segments=segments, tile=tile)
    assert hist.dtype == torch.int32 and before.dtype == torch.int32
    assert torch.equal(hist, r['hist'])
    assert torch.equal(before, r['before'])


def test_rank_count_h2_accumulates():
    from pps_amd import ops
    c, r = _count_data(), _count_ref('euclidean')
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    h0 = torch.randint(-5, 50, r['hist'].shape, generator=gen, device='cuda', dtype=torch.int32)
    b0 = torch.randint(-5, 50, r['before'].shape, generator=gen, device='cuda',
                       dtype=torch.int32)
    h, b = h0.clone(), b0.clone()
    out = ops.rank_count_h2(c['q_split'], c['index'], 0, r['sp'], r['junk'], hist=h, before=b)
    assert out[0] is h and out[1] is b
    assert torch.equal(h, h0 + r['hist']) and torch.equal(b, b0 + r['before'])


@pytest.mark.parametrize('tile', [1, 2])
def test_rank_count_h2_lists_over_several_rounds(tile):
    """An identity with about 600 positives: the kernel bins a list in rounds
    of 256 positives; 400 gallery rows are copies of 7, so ties sit on the
    round edges too."""
    from pps_amd import ops
    Q, G, D = 24, 900, 64
    gen = torch.Generator(device='cuda')
    gen.manual_seed(19)
    q, g = _normed(Q, D, gen), _normed(G, D, gen)
    g[100:500] = g[torch.arange(400, device='cuda') % 7 + 500]   # 7 distinct rows, 400 times
    rng = np.random.RandomState(19)
    gid = np.where(np.arange(G) < 700, 1, rng.randint(2, 6, G))
    gcam = rng.randint(1, 7, G)
    qid, qcam = rng.randint(1, 6, Q), rng.randint(1, 7, Q)
    qid[:12] = 1
    dist = _matrix(q, g, 'euclidean')
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    pd, pi, pc, junk = ops.collect_matches(dist, mi)
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    assert 512 < int(sp.pos_total.max()) <= ops.rank_count_h2_max_p()
    hist, before = ops.rank_count_stream(dist, 0, sp, junk)
    h, b = ops.rank_count_h2(ops.split_h2_tiled(q), ops.GalleryIndex(g, math='h2'), 0, sp, junk,
                             tile=tile)
    assert torch.equal(h, hist) and torch.equal(b, before)


def test_ptot_above_the_cap():
    """The C entry refuses a list width above pps_rank_count_h2_max_p() with
    the capacity status; rank_eval_fused then counts on the matrix and still
    returns the materialised answer."""
    from pps_amd import _lib, ops
    from pps_amd import reid_dataset_evaluator as gev
    cap = ops.rank_count_h2_max_p()
    assert cap >= 256
    n1 = cap + 100                          # identity 1's gallery rows, 1 in 50 of them junk
    Q, G, D = 40, n1 + 60, 64
    gen = torch.Generator(device='cuda')
    gen.manual_seed(7)
    q, g = _normed(Q, D, gen), _normed(G, D, gen)
    rng = np.random.RandomState(7)
    gid = np.full(G, 1)
    gid[n1:] = rng.randint(2, 9, G - n1)
    gcam = np.full(G, 2)
    gcam[::50] = 1
    qid, qcam = rng.randint(1, 9, Q), np.full(Q, 1)
    qid[:8] = 1
    assert ops.max_positives(qid, qcam, gid, gcam) > cap
    dist = _matrix(q, g, 'euclidean')
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    pd, pi, pc, junk = ops.collect_matches(dist, mi)
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    Ptot = sp.sorted_d.shape[1]
    assert Ptot > cap
    q2, qrs, qsq = ops.split_h2_tiled(q)
    g2, grs, gsq = ops.GalleryIndex(g, math='h2').h2
    hist = torch.zeros((Q, Ptot), dtype=torch.int32, device='cuda')
    before = torch.zeros((Q,), dtype=torch.int32, device='cuda')
    L = _lib.lib()
    status = L.pps_rank_count_h2_tiled(
        q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(), g2.data_ptr(), gsq.data_ptr(),
        grs.data_ptr(), G, D, 0, 0, Ptot, sp.sorted_d.data_ptr(), sp.sorted_idx.data_ptr(),
        sp.pos_total.data_ptr(), junk[0].shape[1], junk[0].data_ptr(), junk[1].data_ptr(),
        junk[2].data_ptr(), 0, 0, None, 0, hist.data_ptr(), before.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert status == CAPACITY
    assert str(cap) in L.pps_last_error().decode('utf-8')
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0 and int(before.abs().sum()) == 0
    _assert_rank_equal(ops.rank_eval_fused(q, g, qid, qcam, gid, gcam),
                       gev.rank_eval(dist, qid, gid, qcam, gcam))


# ---------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('kind', ['tensor', 'index', 'split'])
def test_rank_eval_fused_equals_rank_eval(kind, metric):
    from pps_amd import ops
    c, r = _count_data(), _count_ref(metric)
    if kind == 'tensor':
        gallery = c['g']
    elif kind == 'index':
        gallery = c['index']
    else:
        gallery = ops.GalleryIndex.split(c['g'], max_rows=400, math='h2')
        assert [p.shape[0] for p in gallery] == [400, 400, 300]
    got = ops.rank_eval_fused(c['q'], gallery, c['qid'], c['qcam'], c['gid'], c['gcam'],
                              metric=metric)
    _assert_rank_equal(got, r['rank'])


@pytest.mark.parametrize('tile,segments', [(1, 3), (2, 0)])
def test_rank_eval_fused_tile_and_segments(tile, segments):
    from pps_amd import ops
    c, r = _count_data(), _count_ref('euclidean')
    got = ops.rank_eval_fused(c['q'], c['index'], c['qid'], c['qcam'], c['gid'], c['gcam'],
                              segments=segments, tile=tile)
    _assert_rank_equal(got, r['rank'])


def test_rank_eval_fused_x3_index_falls_back():
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _count_data()
    index = ops.GalleryIndex(c['g'], math='x3')
    assert index.h2 is None
    ref = gev.rank_eval(ops.compute_dist(c['q'], index), c['qid'], c['gid'], c['qcam'],
                        c['gcam'])
    got = ops.rank_eval_fused(c['q'], index, c['qid'], c['qcam'], c['gid'], c['gcam'])
    _assert_rank_equal(got, ref)
    # one x3 segment among h2 ones: that segment alone takes its block
    parts = ops.GalleryIndex.split(c['g'], max_rows=400, math='h2')
    parts[1] = ops.GalleryIndex(c['g'][400:800], math='x3')
    dist = torch.cat([ops.compute_dist(c['q'], p) for p in parts], dim=1)
    ref = gev.rank_eval(dist, c['qid'], c['gid'], c['qcam'], c['gcam'])
    got = ops.rank_eval_fused(c['q'], parts, c['qid'], c['qcam'], c['gid'], c['gcam'])
    _assert_rank_equal(got, ref)


def test_rank_eval_fused_d40_falls_back():
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _count_data()
    q, g = c['q'][:, :40].contiguous(), c['g'][:, :40].contiguous()
    ref = gev.rank_eval(ops.compute_dist(q, g, math='h2', symmetric=False), c['qid'], c['gid'],
                        c['qcam'], c['gcam'])
    got = ops.rank_eval_fused(q, g, c['qid'], c['qcam'], c['gid'], c['gcam'])
    _assert_rank_equal(got, ref)


def test_rank_eval_fused_strided_queries():
    from pps_amd import ops
    c, r = _count_data(), _count_ref('euclidean')
    wide = torch.zeros((CQ, CD + 32), device='cuda')
    wide[:, :CD] = c['q']
    q = wide[:, :CD]
    assert not q.is_contiguous()
    got = ops.rank_eval_fused(q, c['index'], c['qid'], c['qcam'], c['gid'], c['gcam'])
    _assert_rank_equal(got, r['rank'])


@pytest.mark.parametrize('metric', METRICS)
def test_from_features_evaluators(metric):
    """mean_ap_from_features / evaluate_from_features against mean_ap and
    cmc(first_match_break=True) on the matrix, and against the oracle on that
    same matrix (eps = 0: only exact ties are left to the stable order)."""
    from pps_amd import reid_dataset_evaluator as gev
    c, r = _count_data(), _count_ref(metric)
    labels = (c['qid'], c['gid'], c['qcam'], c['gcam'])
    mAP = gev.mean_ap_from_features(c['q'], c['index'], *labels, metric=metric)
    assert mAP == gev.mean_ap(r['dist'], *labels)
    ap, valid = gev.mean_ap_from_features(c['q'], c['g'], *labels, average=False, metric=metric)
    ap1, valid1 = gev.mean_ap(r['dist'], *labels, average=False)
    np.testing.assert_array_equal(ap.view(np.int64), ap1.view(np.int64))
    np.testing.assert_array_equal(valid, valid1)
    mAP2, cmc = gev.evaluate_from_features(c['q'], c['index'], *labels, metric=metric, topk=10)
    assert mAP2 == mAP
    np.testing.assert_array_equal(cmc, gev.cmc(r['dist'], *labels, topk=10,
                                               first_match_break=True))
    got = gev.rank_eval_from_features(c['q'].cpu().numpy(), c['g'].cpu().numpy(), *labels,
                                      metric=metric)
    _assert_rank_equal(got, r['rank'])
    res = check_rank_metrics(got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(),
                             r['dist'].cpu().numpy(), c['qid'], c['gid'], c['qcam'], c['gcam'],
                             0.0)
    print('from features (%s): %s' % (metric, res))


def test_rank_eval_fused_self_search():
    """q = g, other labels on the query side: the matrix is the general
    kernel's (symmetric=False), not the mirrored self-distance."""
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _count_data()
    g, gid, gcam = c['g'], c['gid'], c['gcam']
    rng = np.random.RandomState(21)
    qid, qcam = rng.randint(1, 91, CG), rng.randint(1, 7, CG)
    ref = gev.rank_eval(_matrix(g, g, 'euclidean'), qid, gid, qcam, gcam)
    _assert_rank_equal(ops.rank_eval_fused(g, g, qid, qcam, gid, gcam), ref)
    _assert_rank_equal(ops.rank_eval_fused(g, c['index'], qid, qcam, gid, gcam), ref)


def test_rank_eval_fused_rejects_bad_input():
    from pps_amd import ops
    c = _count_data()
    with pytest.raises(RuntimeError, match='ids and cams'):
        ops.rank_eval_fused(c['q'], c['g'], c['qid'][:-1], c['qcam'], c['gid'], c['gcam'])
    with pytest.raises(RuntimeError, match='gallery must be'):
        ops.rank_eval_fused(c['q'], [], c['qid'], c['qcam'], c['gid'], c['gcam'])
    parts = [c['index']] * (ops.RANK_FUSED_MAX_SEGMENTS + 1)
    with pytest.raises(RuntimeError, match='at most 64 lists'):
        ops.rank_eval_fused(c['q'], parts, c['qid'], c['qcam'], np.tile(c['gid'], 65),
                            np.tile(c['gcam'], 65))


# ---------------------------------------------------------------- 4. sharded
def test_sharded_run_fused_world_1():
    from pps_amd.distributed import ShardedEvaluator
    c = _count_data()
    ev = ShardedEvaluator(c['qid'], c['qcam'], c['gid'], c['gcam'], 0, 1)
    a = ev.run(c['q'], c['g'])
    b = ev.run(c['q'], c['g'], fused=True)
    assert 'dist' not in b
    assert a['mAP'] == b['mAP']
    np.testing.assert_array_equal(a['ap'].view(np.int64), b['ap'].view(np.int64))
    np.testing.assert_array_equal(a['first_rank'], b['first_rank'])
    np.testing.assert_array_equal(a['valid'], b['valid'])
    np.testing.assert_array_equal(a['cmc'], b['cmc'])
    with pytest.raises(RuntimeError, match='keep_dist'):
        ev.run(c['q'], c['g'], keep_dist=True, fused=True)


def test_sharded_fused_four_shards_in_process():
    """Four evaluators as ranks 0..3 of 4 take the fused calls exactly as
    ShardedEvaluator.run(fused=True) drives them; the lists are stacked (the
    all-gather) and the counts summed (the all-reduce) by hand.  Equal to the
    one-shard result on the whole matrix."""
    from pps_amd import reid_dataset_evaluator as gev
    from pps_amd.distributed import HipBackend, ShardedEvaluator
    Q, G, D, R = 120, 900, 64, 4
    gen = torch.Generator(device='cuda')
    gen.manual_seed(13)
    q, g = _normed(Q, D, gen), _normed(G, D, gen)
    rng = np.random.RandomState(13)
    qid, gid = rng.randint(1, 61, Q), rng.randint(1, 61, G)
    qcam, gcam = rng.randint(1, 4, Q), rng.randint(1, 4, G)
    g[450] = g[449]                      # equal distances across a shard edge
    be = HipBackend
    evs = [ShardedEvaluator(qid, qcam, gid, gcam, r, R) for r in range(R)]
    ops_, lists, junks, states = [], [], [], []
    for ev in evs:
        a, b = ev.g_ranges[ev.rank]
        operands = be.fused_operands(q, g[a:b], R * ev.pmax)
        assert operands is not None
        st = be.prepare(ev)
        pd, pi, pc, junk = be.collect_fused(operands, ev, st, ev.pmax)
        ops_.append(operands)
        lists.append((pd, pi, pc))
        junks.append(junk)
        states.append(st)
    pos_d, pos_i, pos_c = (torch.stack([l[i] for l in lists]) for i in range(3))
    hist = before = None
    for ev, operands, st, junk in zip(evs, ops_, states, junks):
        sd, _, ptot, h, bf = be.counts_fused(operands, ev, st, pos_d, pos_i, pos_c, junk)
        hist = h if hist is None else hist + h
        before = bf if before is None else before + bf
    got = be.finalize(sd, ptot, hist, before)
    _assert_rank_equal(got, gev.rank_eval(_matrix(q, g, 'euclidean'), qid, gid, qcam, gcam))


def test_sharded_fused_takes_the_matrix_path_without_the_methods():
    from pps_amd.distributed import HipBackend, ShardedEvaluator

    class Plain(object):   # a backend without collect_fused / counts_fused
        device = HipBackend.device
        distmat = HipBackend.distmat   # bound to HipBackend
        prepare = staticmethod(HipBackend.prepare)
        collect = staticmethod(HipBackend.collect)
        counts = staticmethod(HipBackend.counts)
        finalize = staticmethod(HipBackend.finalize)

    c, r = _count_data(), _count_ref('euclidean')
    ev = ShardedEvaluator(c['qid'], c['qcam'], c['gid'], c['gcam'], 0, 1, backend=Plain)
    a = ev.run(c['q'], c['g'], fused=True)
    np.testing.assert_array_equal(a['ap'].view(np.int64),
                                  r['rank'][0].cpu().numpy().view(np.int64))


# ---------------------------------------------------------------- 5. memory claim
def test_rank_eval_fused_peak_memory_below_the_matrix():
    """Q = 2048, G = 32768, D = 64: the [Q, G] float32 matrix alone is 268 MB;
    the fused path (lists, counts, the queries' planes) needs a few MB."""
    from pps_amd import ops
    Q, G, D = 2048, 32768, 64
    gen = torch.Generator(device='cuda')
    gen.manual_seed(17)
    q, g = _normed(Q, D, gen), _normed(G, D, gen)
    rng = np.random.RandomState(17)
    qid, gid = rng.randint(0, 1000, Q), rng.randint(0, 1000, G)
    qcam, gcam = rng.randint(1, 7, Q), rng.randint(1, 7, G)
    index = ops.GalleryIndex(g, math='h2')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ap, valid, first = ops.rank_eval_fused(q, index, qid, qcam, gid, gcam)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print('rank_eval_fused peak allocation: %.1f MB (matrix: %.1f MB)'
          % (peak / 1e6, Q * G * 4 / 1e6))
    assert peak < Q * G * 4
    assert int(valid.sum()) > 0 and bool(torch.isfinite(ap).all())
