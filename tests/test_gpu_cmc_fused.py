"""Matrix-free fractional and separate-camera CMC: the fused distance + key-bin
count kernel (ops.cmc_counts_h2) and what is built on it (ops.cmc_eval_fused,
cmc_from_features, evaluate_from_features' new arguments) against the
materialised path -- ops.cmc_counts / cmc on the matrix of compute_dist(q, g,
math='h2', symmetric=False, pad_rows=True).  Every distance the fused kernel
computes has that matrix's bits, so every comparison is an equality: counts as
int32 tensors, CMC rows as float64 bits.  Features are seeded normalised
Gaussians; labels and copied gallery rows are built so that every tie the key
bins have to order by global index occurs (asserted on the reference matrix by
test_data_holds_the_constructed_ties).  References are computed once per
metric and shared."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

METRICS = ('euclidean', 'sqeuclidean', 'cosine')
CAPACITY = -4
CQ, CG, CD = 300, 1100, 64
# column pairs on both sides of a tile edge (192 k, 256 k) or a segment edge
# (segments=3: columns 384 / 768 with the 192 tile, 512 / 1024 with the 256 tile)
EDGES = [(191, 192), (255, 256), (383, 384), (511, 512), (767, 768), (1023, 1024)]
# query 40: positives 398 and 404 are copies of each other, valid non-match
# copies below both (15), between them (401) and above both (1075); 398 | 401
# also straddle the first edge of GalleryIndex.split(max_rows=400)
TWIN_Q, TWIN = 40, (15, 398, 401, 404, 1075)
# query 41: its last positive copied to a lower (13) and a higher (1076) index
LAST_Q, LAST_ROWS, LAST_LO, LAST_HI = 41, (610, 620, 630), 13, 1076
# query 42: a copy of its nearest positive on the query's camera, other identity
CAM_Q, CAM_ROWS, CAM_COPY = 42, (640, 650), 14


def _normed(n, D, gen):
    x = torch.randn((n, D), generator=gen, device='cuda')
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _matrix(q, g, metric):
    from pps_amd import ops
    return ops.compute_dist(q, g, metric=metric, math='h2', symmetric=False, pad_rows=True)


def _nearest_positive(d0, i, qid, qcam, gid, gcam, last=False):
    pos = np.nonzero((gid == qid[i]) & (gcam != qcam[i]))[0]
    if len(pos) == 0:
        return None
    return int(pos[np.lexsort((pos, d0[i, pos]))[-1 if last else 0]])


@functools.lru_cache(maxsize=None)
def _data():
    """Q = 300, G = 1100, D = 64 (two ragged panels, five or six ragged tiles).
    Rows 0..39 and 1060..1099 are filler (identities no query has) that the
    constructed ties are copied into."""
    from pps_amd import ops
    gen = torch.Generator(device='cuda')
    gen.manual_seed(23)
    g, q = _normed(CG, CD, gen), _normed(CQ, CD, gen)
    rng = np.random.RandomState(23)
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
        else:
            gcam[b] = 3
    # two positives that are copies of each other among three non-match copies
    n0, a1, n1, a2, n2 = TWIN
    x = g[a1] + 0.05 * q[TWIN_Q]
    q[TWIN_Q] = x / x.norm()
    for r in (n0, n1, a2, n2):
        g[r] = g[a1]
    qid[TWIN_Q], qcam[TWIN_Q] = 500, 1
    gid[[a1, a2]], gcam[[a1, a2]] = 500, 2
    gid[n1] = 5000 + n1
    gcam[[n0, n1, n2]] = 3
    qid[LAST_Q], qcam[LAST_Q] = 501, 1
    gid[list(LAST_ROWS)], gcam[list(LAST_ROWS)] = 501, 2
    gcam[[LAST_LO, LAST_HI]] = 3
    x = g[CAM_ROWS[0]] + 0.05 * q[CAM_Q]    # next to its first positive: nothing ranks before
    q[CAM_Q] = x / x.norm()
    qid[CAM_Q], qcam[CAM_Q] = 502, 1
    gid[list(CAM_ROWS)], gcam[list(CAM_ROWS)] = 502, 2
    gcam[CAM_COPY] = 1
    # copies of a query's nearest positive: queries 12..21 get one at a lower
    # and one at a higher index (valid non-matches of another camera), queries
    # 22..29 one that is junk (its id and camera)
    d0 = _matrix(q, g, 'euclidean').cpu().numpy()
    tied, junked = [], []
    for i in range(12, 30):
        c = _nearest_positive(d0, i, qid, qcam, gid, gcam)
        if c is None:
            continue
        if i < 22:
            lo, hi = i - 12, 1060 + i - 12
            g[lo] = g[c]
            g[hi] = g[c]
            gcam[[lo, hi]] = qcam[i] % 6 + 1
            tied.append((i, c, lo, hi))
        else:
            row = 20 + i - 22
            g[row] = g[c]
            gid[row], gcam[row] = qid[i], qcam[i]
            junked.append((i, c, row))
    last = _nearest_positive(d0, LAST_Q, qid, qcam, gid, gcam, last=True)
    g[LAST_LO] = g[last]
    g[LAST_HI] = g[last]
    cam_c = _nearest_positive(d0, CAM_Q, qid, qcam, gid, gcam)
    g[CAM_COPY] = g[cam_c]
    assert len(tied) >= 5 and len(junked) >= 3
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    return dict(q=q, g=g, qid=qid, qcam=qcam, gid=gid, gcam=gcam, mi=mi, tied=tied,
                junked=junked, last=last, cam_c=cam_c, q_split=ops.split_h2_tiled(q),
                index=ops.GalleryIndex(g, math='h2'))


@functools.lru_cache(maxsize=None)
def _ref(metric):
    """The materialised path on the h2 matrix: lists, sorted positives, the key
    bins of both modes."""
    from pps_amd import ops
    c = _data()
    dist = _matrix(c['q'], c['g'], metric)
    pd, pi, pc, junk = ops.collect_matches(dist, c['mi'])
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    hist = {False: ops.cmc_counts(dist, 0, sp, junk),
            True: ops.cmc_counts(dist, 0, sp, junk, c['mi'], True)}
    return dict(dist=dist, sp=sp, junk=junk, hist=hist)


@functools.lru_cache(maxsize=None)
def _ref_cmc(metric, sep, fmb):
    """cmc's per-query rows on the matrix."""
    from pps_amd import reid_dataset_evaluator as gev
    c, r = _data(), _ref(metric)
    return gev.cmc(r['dist'], c['qid'], c['gid'], c['qcam'], c['gcam'], separate_camera_set=sep,
                   first_match_break=fmb, average=False)


def _labels(c):
    return c['qid'], c['gid'], c['qcam'], c['gcam']


def _assert_rows_equal(got, ref):
    (ret, valid), (ret1, valid1) = got, ref
    np.testing.assert_array_equal(np.asarray(valid), np.asarray(valid1))
    np.testing.assert_array_equal(np.ascontiguousarray(ret).view(np.int64),
                                  np.ascontiguousarray(ret1).view(np.int64))


def _host_rows(ret, valid):
    return ret.cpu().numpy(), valid.cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------- 1. the data
def test_data_holds_the_constructed_ties():
    from pps_amd import ops
    c, r = _data(), _ref('euclidean')
    qid, gid, qcam, gcam = _labels(c)
    d = _bits(r['dist'])
    dv = r['dist'].cpu().numpy()
    sd, si = r['sp'].sorted_d.cpu().numpy(), r['sp'].sorted_idx.cpu().numpy()
    ptot = r['sp'].pos_total.cpu().numpy()

    def key_bin(i, col):   # positives of query i whose (distance, index) key is below col's
        return sum((float(sd[i, p]), int(si[i, p])) < (float(dv[i, col]), col)
                   for p in range(ptot[i]))

    valid_other = lambda i, col: gid[col] != qid[i] and gcam[col] != qcam[i]
    # a valid non-match copy of a positive below it (its bin) and above it (the next)
    for i, col, lo, hi in c['tied']:
        assert d[i, lo] == d[i, col] == d[i, hi] and lo < col < hi
        assert valid_other(i, lo) and valid_other(i, hi)
        p = key_bin(i, col)
        assert key_bin(i, lo) == p and key_bin(i, hi) == p + 1
    # two tied positives, non-match copies below both, between them, above both
    n0, a1, n1, a2, n2 = TWIN
    assert len(set(d[TWIN_Q, list(TWIN)].tolist())) == 1 and n0 < a1 < n1 < a2 < n2
    assert all(valid_other(TWIN_Q, x) for x in (n0, n1, n2))
    assert gid[a1] == gid[a2] == qid[TWIN_Q] and ptot[TWIN_Q] == 2
    assert [key_bin(TWIN_Q, x) for x in TWIN] == [0, 0, 1, 1, 2]   # 2 == P: not counted
    # the last positive's copies: the higher index is ordered after every positive
    last, P = c['last'], ptot[LAST_Q]
    assert P == 3 and d[LAST_Q, LAST_LO] == d[LAST_Q, last] == d[LAST_Q, LAST_HI]
    assert LAST_LO < last < LAST_HI
    assert valid_other(LAST_Q, LAST_LO) and valid_other(LAST_Q, LAST_HI)
    assert key_bin(LAST_Q, last) == P - 1 and key_bin(LAST_Q, LAST_LO) == P - 1
    assert key_bin(LAST_Q, LAST_HI) == P
    # a junk copy of a positive
    for i, col, row in c['junked']:
        assert d[i, row] == d[i, col] and gid[row] == qid[i] and gcam[row] == qcam[i]
    # a copy on the query's camera under another identity: valid only in junk mode
    assert c['cam_c'] == CAM_ROWS[0] and d[CAM_Q, CAM_COPY] == d[CAM_Q, c['cam_c']]
    assert gid[CAM_COPY] != qid[CAM_Q] and gcam[CAM_COPY] == qcam[CAM_Q]
    assert key_bin(CAM_Q, CAM_COPY) == 0
    hj, hs = r['hist'][False].cpu().numpy(), r['hist'][True].cpu().numpy()
    assert hj[CAM_Q, 0] == 2 and hs[CAM_Q, 0] == 1   # the positive itself, and the copy
    # copy pairs over every tile and segment edge
    for k, (a, b) in enumerate(EDGES):
        assert d[30 + k, a] == d[30 + k, b] and b == a + 1
    # empty lists, the long identity
    assert ptot[0] == 150 and (ptot[6:11] == 0).all() and r['sp'].sorted_d.shape[1] == 180
    assert int(r['junk'][2].cpu().numpy()[0]) == 30 and int(r['junk'][2].cpu().numpy()[9]) == 5
    # the key bins are not the distance bins where an entry ties with a positive
    # at a lower index: a kernel that ignores the index cannot pass
    dist_hist, _ = ops.rank_count_stream(r['dist'], 0, r['sp'], r['junk'])
    dist_hist = dist_hist.cpu().numpy()
    for i in [t[0] for t in c['tied']] + [TWIN_Q, LAST_Q]:
        assert (dist_hist[i] != hj[i]).any(), i


# ---------------------------------------------------------------- 2. count kernel
@pytest.mark.parametrize('sep', [False, True], ids=['junk', 'sepcam'])
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('segments', [0, 1, 3])
@pytest.mark.parametrize('tile', [1, 2])
def test_cmc_counts_h2_equals_cmc_counts(tile, segments, metric, sep):
    from pps_amd import ops
    c, r = _data(), _ref(metric)
    hist = ops.cmc_counts_h2(c['q_split'], c['index'], 0, r['sp'], None if sep else r['junk'],
                             c['mi'], sep, metric, segments=segments, tile=tile)
    assert hist.dtype == torch.int32
    assert torch.equal(hist, r['hist'][sep])


@pytest.mark.parametrize('sep', [False, True], ids=['junk', 'sepcam'])
def test_cmc_counts_h2_accumulates(sep):
    from pps_amd import ops
    c, r = _data(), _ref('euclidean')
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    h0 = torch.randint(-5, 50, r['hist'][sep].shape, generator=gen, device='cuda',
                       dtype=torch.int32)
    h = h0.clone()
    out = ops.cmc_counts_h2(c['q_split'], c['index'], 0, r['sp'], r['junk'], c['mi'], sep, hist=h)
    assert out is h
    assert torch.equal(h, h0 + r['hist'][sep])


@pytest.mark.parametrize('sep', [False, True], ids=['junk', 'sepcam'])
def test_cmc_counts_h2_g_offset(sep):
    """The gallery as rows [1000, 2100) of a larger one: the positives' and the
    junk entries' indices shifted, the columns' shifted by g_offset."""
    from pps_amd import ops
    c, r = _data(), _ref('euclidean')
    sp = r['sp']
    sp2 = ops.SortedPositives(sp.sorted_d, sp.sorted_idx + 1000, sp.pos_total, sp.cells)
    junk2 = (r['junk'][0], r['junk'][1] + 1000, r['junk'][2])
    ref = ops.cmc_counts(r['dist'], 1000, sp2, junk2, c['mi'], sep)
    assert torch.equal(ref, r['hist'][sep])
    got = ops.cmc_counts_h2(c['q_split'], c['index'], 1000, sp2, junk2, c['mi'], sep)
    assert torch.equal(got, ref)
    # the index decides: with unshifted columns every tie falls on the other side
    wrong = ops.cmc_counts_h2(c['q_split'], c['index'], 0, sp2, junk2, c['mi'], sep)
    assert not torch.equal(wrong, ref)


@functools.lru_cache(maxsize=None)
def _long_data():
    """An identity with about 600 positives: the kernel bins a list in rounds
    of 256 positives; 400 gallery rows are copies of 7, every fourth copy under
    another identity, so tie groups of positives and non-matches cross the
    round edges."""
    from pps_amd import ops
    Q, G, D = 24, 1000, 64
    gen = torch.Generator(device='cuda')
    gen.manual_seed(29)
    q, g = _normed(Q, D, gen), _normed(G, D, gen)
    g[100:500] = g[torch.arange(400, device='cuda') % 7 + 500]   # 7 distinct rows, 400 times
    rng = np.random.RandomState(29)
    gid = np.where(np.arange(G) < 850, 1, rng.randint(2, 6, G))
    gid[100:500:4] = 9                                           # copies no query looks for
    gcam = rng.randint(1, 7, G)
    qid, qcam = rng.randint(1, 6, Q), rng.randint(1, 7, Q)
    qid[:12] = 1
    dist = _matrix(q, g, 'euclidean')
    mi = ops.MatchIndex(qid, qcam, gid, gcam)
    pd, pi, pc, junk = ops.collect_matches(dist, mi)
    sp = ops.rank_prepare(pd[None], pi[None], pc[None])
    return dict(dist=dist, mi=mi, sp=sp, junk=junk, q_split=ops.split_h2_tiled(q),
                index=ops.GalleryIndex(g, math='h2'))


@pytest.mark.parametrize('sep', [False, True], ids=['junk', 'sepcam'])
@pytest.mark.parametrize('tile', [1, 2])
def test_cmc_counts_h2_lists_over_several_rounds(tile, sep):
    from pps_amd import ops
    c = _long_data()
    sp = c['sp']
    assert 512 < int(sp.pos_total.max()) <= ops.rank_count_h2_max_p()
    assert sp.sorted_d.shape[1] <= ops.rank_count_h2_max_p()
    sd, ptot = _bits(sp.sorted_d), sp.pos_total.cpu().numpy()
    crossed = [(i, e) for i in range(12) for e in (256, 512)
               if e < ptot[i] and sd[i, e - 1] == sd[i, e]]
    assert crossed   # some query's tie group lies on both sides of a round edge
    ref = ops.cmc_counts(c['dist'], 0, sp, c['junk'], c['mi'], sep)
    got = ops.cmc_counts_h2(c['q_split'], c['index'], 0, sp, c['junk'], c['mi'], sep, tile=tile)
    assert torch.equal(got, ref)


def test_ptot_above_the_cap():
    """The C entry refuses a list width above pps_rank_count_h2_max_p() with
    the capacity status and adds nothing; cmc_eval_fused then counts on the
    matrix and still returns the materialised answer."""
    from pps_amd import _lib, ops
    cap = ops.rank_count_h2_max_p()
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
    L = _lib.lib()
    for cams in ((None, None), (mi.qcam.data_ptr(), mi.gcam.data_ptr())):
        status = L.pps_cmc_count_h2_tiled(
            q2.data_ptr(), Q, qsq.data_ptr(), qrs.data_ptr(), g2.data_ptr(), gsq.data_ptr(),
            grs.data_ptr(), G, D, 0, 0, Ptot, sp.sorted_d.data_ptr(), sp.sorted_idx.data_ptr(),
            sp.pos_total.data_ptr(), cams[0], cams[1], junk[0].shape[1], junk[0].data_ptr(),
            junk[1].data_ptr(), junk[2].data_ptr(), 0, 0, None, 0, hist.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        assert status == CAPACITY
        assert str(cap) in L.pps_last_error().decode('utf-8')
        torch.cuda.synchronize()
        assert int(hist.abs().sum()) == 0
    for sep in (False, True):
        ref = ops.cmc_finalize(sp.pos_total, ops.cmc_counts(dist, 0, sp, junk, mi, sep), 100,
                               False)
        got = ops.cmc_eval_fused(q, g, qid, qcam, gid, gcam, separate_camera_set=sep)
        _assert_rows_equal(_host_rows(*got), _host_rows(*ref))


# ---------------------------------------------------------------- 3. end to end
MODES = [(False, False), (False, True), (True, False), (True, True)]


def _gallery(kind):
    from pps_amd import ops
    c = _data()
    if kind == 'tensor':
        return c['g']
    if kind == 'index':
        return c['index']
    parts = ops.GalleryIndex.split(c['g'], max_rows=400, math='h2')
    assert [p.shape[0] for p in parts] == [400, 400, 300]   # rows 398 | 401 tie across an edge
    return parts


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('sep,fmb', MODES)
@pytest.mark.parametrize('kind', ['tensor', 'index', 'split'])
def test_cmc_from_features_equals_cmc(kind, sep, fmb, metric):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _data()
    ref = _ref_cmc(metric, sep, fmb)
    gallery = _gallery(kind)
    got = ops.cmc_eval_fused(c['q'], gallery, c['qid'], c['qcam'], c['gid'], c['gcam'],
                             separate_camera_set=sep, first_match_break=fmb, metric=metric)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32
    assert tuple(got[0].shape) == (CQ, 100)
    _assert_rows_equal(_host_rows(*got), ref)
    rows = gev.cmc_from_features(c['q'], gallery, *_labels(c), separate_camera_set=sep,
                                 first_match_break=fmb, average=False, metric=metric)
    _assert_rows_equal(rows, ref)
    avg = gev.cmc_from_features(c['q'], gallery, *_labels(c), separate_camera_set=sep,
                                first_match_break=fmb, metric=metric)
    ref_avg = np.sum(ref[0], axis=0) / ref[1].sum()
    np.testing.assert_array_equal(avg.view(np.int64), ref_avg.view(np.int64))


def test_cmc_from_features_averaged_equals_cmc_averaged():
    """The averaged call against cmc's own averaged output, topk and NumPy inputs included."""
    from pps_amd import reid_dataset_evaluator as gev
    c, r = _data(), _ref('euclidean')
    for sep, fmb in MODES:
        ref = gev.cmc(r['dist'], *_labels(c), topk=20, separate_camera_set=sep,
                      first_match_break=fmb)
        got = gev.cmc_from_features(c['q'].cpu().numpy(), c['g'].cpu().numpy(), *_labels(c),
                                    topk=20, separate_camera_set=sep, first_match_break=fmb)
        assert got.shape == (20,)
        np.testing.assert_array_equal(got.view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize('tile,segments', [(1, 3), (2, 0)])
def test_cmc_eval_fused_tile_and_segments(tile, segments):
    from pps_amd import ops
    c = _data()
    for sep in (False, True):
        got = ops.cmc_eval_fused(c['q'], c['index'], c['qid'], c['qcam'], c['gid'], c['gcam'],
                                 separate_camera_set=sep, segments=segments, tile=tile,
                                 match_index=c['mi'])
        _assert_rows_equal(_host_rows(*got), _ref_cmc('euclidean', sep, False))


@pytest.mark.parametrize('sep,fmb', MODES)
def test_cmc_from_features_x3_index_falls_back(sep, fmb):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _data()
    kw = dict(separate_camera_set=sep, first_match_break=fmb, average=False)
    index = ops.GalleryIndex(c['g'], math='x3')
    assert index.h2 is None
    ref = gev.cmc(ops.compute_dist(c['q'], index), *_labels(c), **kw)
    _assert_rows_equal(gev.cmc_from_features(c['q'], index, *_labels(c), **kw), ref)
    # one x3 segment among h2 ones: that segment alone takes its block
    parts = ops.GalleryIndex.split(c['g'], max_rows=400, math='h2')
    parts[1] = ops.GalleryIndex(c['g'][400:800], math='x3')
    dist = torch.cat([ops.compute_dist(c['q'], p) for p in parts], dim=1)
    ref = gev.cmc(dist, *_labels(c), **kw)
    _assert_rows_equal(gev.cmc_from_features(c['q'], parts, *_labels(c), **kw), ref)


@pytest.mark.parametrize('sep,fmb', MODES)
def test_cmc_from_features_d40_falls_back(sep, fmb):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _data()
    kw = dict(separate_camera_set=sep, first_match_break=fmb, average=False)
    q, g = c['q'][:, :40].contiguous(), c['g'][:, :40].contiguous()
    ref = gev.cmc(ops.compute_dist(q, g, math='h2', symmetric=False), *_labels(c), **kw)
    _assert_rows_equal(gev.cmc_from_features(q, g, *_labels(c), **kw), ref)


@pytest.mark.parametrize('sep,fmb', MODES)
def test_cmc_eval_fused_strided_queries(sep, fmb):
    from pps_amd import ops
    c = _data()
    wide = torch.zeros((CQ, CD + 32), device='cuda')
    wide[:, :CD] = c['q']
    q = wide[:, :CD]
    assert not q.is_contiguous()
    got = ops.cmc_eval_fused(q, c['index'], c['qid'], c['qcam'], c['gid'], c['gcam'],
                             separate_camera_set=sep, first_match_break=fmb)
    _assert_rows_equal(_host_rows(*got), _ref_cmc('euclidean', sep, fmb))


def test_cmc_from_features_rejects_bad_input():
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    c = _data()
    with pytest.raises(RuntimeError, match='single_gallery_shot.*use cmc'):
        gev.cmc_from_features(c['q'], c['g'], *_labels(c), single_gallery_shot=True)
    with pytest.raises(RuntimeError, match='cmc_eval_fused: .*ids and cams'):
        gev.cmc_from_features(c['q'], c['g'], c['qid'][:-1], c['gid'], c['qcam'], c['gcam'])
    with pytest.raises(RuntimeError, match='cmc_eval_fused: .*ids and cams'):
        ops.cmc_eval_fused(c['q'], c['g'], c['qid'], c['qcam'], c['gid'][:-1], c['gcam'])
    with pytest.raises(RuntimeError, match='gallery must be'):
        ops.cmc_eval_fused(c['q'], [], c['qid'], c['qcam'], c['gid'], c['gcam'])
    with pytest.raises(RuntimeError, match='separate_camera_set needs the MatchIndex'):
        ops.cmc_counts_h2(c['q_split'], c['index'], 0, _ref('euclidean')['sp'], None, None, True)
    # rank_eval_fused keeps its own name in the shared checks
    with pytest.raises(RuntimeError, match='rank_eval_fused: .*ids and cams'):
        ops.rank_eval_fused(c['q'], c['g'], c['qid'][:-1], c['qcam'], c['gid'], c['gcam'])


@pytest.mark.parametrize('sep,fmb', MODES)
def test_cmc_from_features_no_valid_query(sep, fmb):
    from pps_amd import reid_dataset_evaluator as gev
    c = _data()
    rows = np.r_[6:11]    # no gallery row (6..8), every member junk (9, 10)
    q, qid, qcam = c['q'][6:11].contiguous(), c['qid'][rows], c['qcam'][rows]
    with pytest.raises(RuntimeError, match='No valid query'):
        gev.cmc_from_features(q, c['index'], qid, c['gid'], qcam, c['gcam'],
                              separate_camera_set=sep, first_match_break=fmb)


@pytest.mark.parametrize('metric', METRICS)
def test_evaluate_from_features(metric):
    from pps_amd import reid_dataset_evaluator as gev
    c, r = _data(), _ref(metric)
    labels = _labels(c)
    # the defaults: today's one-pass Market result
    rank = gev.rank_eval_from_features(c['q'], c['index'], *labels, metric=metric)
    mAP0, cmc0 = gev.scores_from_ranks(*rank, topk=10)
    mAP, cmc = gev.evaluate_from_features(c['q'], c['index'], *labels, metric=metric)
    assert mAP == mAP0 == gev.mean_ap(r['dist'], *labels)
    np.testing.assert_array_equal(cmc.view(np.int64), cmc0.view(np.int64))
    np.testing.assert_array_equal(cmc, gev.cmc(r['dist'], *labels, topk=10,
                                               first_match_break=True))
    # every other combination: mAP as before, the CMC of cmc on the matrix
    for sep, fmb in [(True, True), (True, False), (False, False)]:
        got = gev.evaluate_from_features(c['q'], c['index'], *labels, metric=metric, topk=10,
                                         separate_camera_set=sep, first_match_break=fmb)
        assert got[0] == mAP
        ref = gev.cmc(r['dist'], *labels, topk=10, separate_camera_set=sep,
                      first_match_break=fmb)
        np.testing.assert_array_equal(got[1].view(np.int64), ref.view(np.int64))


# ---------------------------------------------------------------- 4. memory claim
@pytest.mark.parametrize('sep', [False, True], ids=['junk', 'sepcam'])
def test_cmc_from_features_peak_memory_below_the_matrix(sep):
    """Q = 2048, G = 32768, D = 64: the [Q, G] float32 matrix alone is 268 MB;
    the fused path (lists, counts, the queries' planes) needs a few MB."""
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
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
    row = gev.cmc_from_features(q, index, qid, gid, qcam, gcam, separate_camera_set=sep)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print('cmc_from_features peak allocation: %.1f MB (matrix: %.1f MB)'
          % (peak / 1e6, Q * G * 4 / 1e6))
    assert peak < Q * G * 4
    assert row.shape == (100,) and 0 <= row[0] <= row[-1] <= 1 and row[-1] > 0
