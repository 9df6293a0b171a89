"""Guards and size functions of the row-form re-ranking entries
(pps_re_ranking_rows, pps_re_ranking_features, pps_search_h2_tiled_rowmax,
pps_pair_dist_h2), without a GPU: every guard returns before the first GPU
call, so dummy host pointers are enough.  Each case gives one bad argument and
expects the status and the end of pps_last_error()."""
import ctypes

import pytest

OK, INVALID_ARG, CAPACITY = 0, -1, -4
_BUF = ctypes.create_string_buffer(1024)
P = (ctypes.addressof(_BUF) + 255) & ~255        # a non-null, 256-byte aligned host pointer


def _lib():
    from pps_amd import _lib
    return _lib.lib()


def _call(name, args):
    L = _lib()
    status = getattr(L, name)(*args)
    return status, L.pps_last_error().decode('utf-8')


# argument positions (include/pps_abi.h)
FEAT = 'pps_re_ranking_features'
FEAT_POS = dict(x2t=0, xsq=1, xrs=2, g2t=3, gsq=4, grs=5, Q=6, G=7, D=8, metric=9, k1=10, k2=11,
                lam=12, segments=13, tile=14, g_window=15, workspace=16, ws_bytes=17, out=18,
                stream=19)
FEAT_GOOD = [P, P, P, P, P, P, 100, 400, 64, 0, 20, 6, 0.3, 0, 0, 0, P, 0, P, None]
ROWS = 'pps_re_ranking_rows'
ROWS_POS = dict(W=0, ldw=1, Q=2, G=3, k1=4, k2=5, lam=6, g_window=7, workspace=8, ws_bytes=9,
                out=10, stream=11)
ROWS_GOOD = [P, 500, 100, 400, 20, 6, 0.3, 0, P, 0, P, None]


def _with(good, pos, **kw):
    args = list(good)
    for k, v in kw.items():
        args[pos[k]] = v
    return tuple(args)


def _feat(**kw):
    return _with(FEAT_GOOD, FEAT_POS, **kw)


def _rows(**kw):
    return _with(ROWS_GOOD, ROWS_POS, **kw)


def _feat_cases():
    tiles = _lib().pps_search_h2_num_tiles()
    return [
        (_feat(D=40), 'bad shape (D % 32 == 0)'),
        (_feat(D=0), 'bad shape (D % 32 == 0)'),
        (_feat(metric=3), 'unknown metric'),
        (_feat(k1=64), 'k1 + 1 must be <= 64 and <= pps_search_max_k()'),
        (_feat(k1=0), 'k1 + 1 must be <= 64 and <= pps_search_max_k()'),
        (_feat(k2=0), 'k2 must be in [1, k1 + 1]'),
        (_feat(k2=22), 'k2 must be in [1, k1 + 1]'),
        (_feat(Q=5, G=10), 'need Q + G >= k1 + 1'),
        (_feat(Q=0), 'bad shape'),
        (_feat(G=0), 'bad shape'),
        (_feat(G=2 ** 31), 'N = Q + G must fit int32'),
        (_feat(G=2 ** 20, D=1024, k2=1), 'planes over 2 GiB'),
        (_feat(segments=-1), 'segments must be >= 0 (0 = auto)'),
        (_feat(tile=tiles), 'search tile must be 0..%d' % (tiles - 1)),
        (_feat(g_window=-1), 'g_window must be in [0, 38400] (0 = auto)'),
        (_feat(g_window=38401), 'g_window must be in [0, 38400] (0 = auto)'),
        (_feat(x2t=None), 'null pointer'),
        (_feat(grs=None), 'null pointer'),
        (_feat(out=None), 'null pointer'),
        (_feat(workspace=None), 'null pointer'),
        (_feat(x2t=P + 8), 'planes must be 16-byte aligned'),
        (_feat(workspace=P + 16), 'workspace must be 256-byte aligned'),
    ]


@pytest.mark.parametrize('i', range(22))
def test_features_guard_status_and_text(i):
    cases = _feat_cases()
    assert len(cases) == 22
    args, tail = cases[i]
    status, msg = _call(FEAT, args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.startswith('[enforce fail at '), msg
    assert msg.endswith('. ' + tail), msg


def _rows_cases():
    return [
        (_rows(W=None), 'null pointer'),
        (_rows(out=None), 'null pointer'),
        (_rows(ldw=499), 'ldw smaller than the rows'),
        (_rows(k1=64), 'k1 + 1 must be <= 64 and <= pps_search_max_k()'),
        (_rows(k2=22), 'k2 must be in [1, k1 + 1]'),
        (_rows(Q=5, G=10, ldw=15), 'need Q + G >= k1 + 1'),
        (_rows(G=2 ** 31, ldw=2 ** 32), 'N = Q + G must fit int32'),
        (_rows(g_window=38401), 'g_window must be in [0, 38400] (0 = auto)'),
        (_rows(G=10 ** 6, ldw=2 * 10 ** 6, g_window=1), 'more than 65535 gallery windows'),
        (_rows(workspace=P + 16), 'workspace must be 256-byte aligned'),
    ]


@pytest.mark.parametrize('i', range(10))
def test_rows_guard_status_and_text(i):
    cases = _rows_cases()
    assert len(cases) == 10
    args, tail = cases[i]
    status, msg = _call(ROWS, args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.endswith('. ' + tail), msg


@pytest.mark.parametrize('name', [FEAT, ROWS])
def test_capacity_errors_come_before_any_launch(name):
    """N * qcap >= 2^31 (qcap = k2 * 256 at k1 = 20) and a workspace smaller
    than the size function's value are PPS_ERR_CAPACITY."""
    big = dict(Q=10 ** 6, G=10 ** 6)          # 2e6 * 1536 >= 2^31
    args = _feat(**big) if name == FEAT else _rows(ldw=2 * 10 ** 6, **big)
    status, msg = _call(name, args)
    assert status == CAPACITY, (status, msg)
    assert msg.startswith(name + ': N * qcap = 2000000 * 1536 '), msg
    status, msg = _call(name, _feat() if name == FEAT else _rows())   # ws_bytes = 0
    assert status == CAPACITY, (status, msg)
    assert 'workspace too small: need ' in msg, msg


def _search_rowmax_args(**kw):
    pos = dict(q2t=0, Q=1, qsq=2, qrs=3, g2t=4, gsq=5, grs=6, G=7, D=8, metric=9, k=10,
               segments=11, tile=12, workspace=13, ws_bytes=14, vals=15, idx=16, rowmax=17,
               stream=18)
    good = [P, 1, P, P, P, P, P, 1, 32, 0, 5, 0, 0, P, 0, P, P, P, None]
    return _with(good, pos, **kw)


def test_search_rowmax_guards():
    name = 'pps_search_h2_tiled_rowmax'
    for kw, tail in [(dict(rowmax=None), 'null pointer'), (dict(vals=None), 'null pointer'),
                     (dict(D=40), 'bad shape (D % 32 == 0)'), (dict(metric=3), 'unknown metric'),
                     (dict(k=0), 'k must be in [1, %d]' % _lib().pps_search_max_k())]:
        status, msg = _call(name, _search_rowmax_args(**kw))
        assert status == INVALID_ARG and msg.endswith('. ' + tail), (kw, status, msg)
    status, msg = _call(name, _search_rowmax_args())          # no workspace bytes
    assert status == CAPACITY and msg.startswith(name + ': workspace of 0 bytes'), (status, msg)
    assert _call(name, _search_rowmax_args(Q=0))[0] == OK


def _pair_args(**kw):
    pos = dict(q2t=0, Q=1, qsq=2, qrs=3, g2t=4, gsq=5, grs=6, G=7, D=8, metric=9, lists=10,
               counts=11, cap=12, out=13, stream=14)
    good = [P, 1, P, P, P, P, P, 1, 32, 0, P, None, 4, P, None]
    return _with(good, pos, **kw)


def test_pair_dist_guards():
    name = 'pps_pair_dist_h2'
    for kw, tail in [(dict(lists=None), 'null pointer'), (dict(out=None), 'null pointer'),
                     (dict(D=40), 'bad shape (D % 32 == 0)'), (dict(metric=-1), 'unknown metric'),
                     (dict(cap=0), 'cap must be >= 1'),
                     (dict(Q=2 ** 20, D=1024), 'planes over 2 GiB'),
                     (dict(G=0), 'a listed pair needs a b-row (G > 0)'),
                     (dict(g2t=None), 'null pointer'),
                     (dict(q2t=P + 8), 'planes must be 16-byte aligned')]:
        status, msg = _call(name, _pair_args(**kw))
        assert status == INVALID_ARG and msg.endswith('. ' + tail), (kw, status, msg)
    assert _call(name, _pair_args(Q=0))[0] == OK


def test_size_functions():
    L = _lib()
    rows, feat = L.pps_rerank_rows_workspace_bytes, L.pps_rerank_features_workspace_bytes
    # bad arguments
    for bad in [(-1, 10, 20, 6), (10, -1, 20, 6), (10, 10, 0, 6), (10, 10, 64, 6), (10, 10, 20, 0),
                (10, 10, 20, 22)]:
        assert rows(*bad) == -1 and feat(*(bad + (0,))) == -1, bad
    assert feat(10, 10, 20, 6, -1) == -1
    # non-decreasing in G
    for Q in (1, 150, 2228, 10000):
        prev_r = prev_f = 0
        for G in list(range(0, 3000, 37)) + [17661, 38400, 38401, 150000, 10 ** 6]:
            r, f = rows(Q, G, 20, 6), feat(Q, G, 20, 6, 0)
            assert r >= prev_r and f >= prev_f and f >= r > 0, (Q, G, r, f)
            prev_r, prev_f = r, f
    # the features size holds the self-search's workspace for every N and request
    for N in list(range(22, 4000, 61)) + [16384, 19889, 40000, 152000, 10 ** 6]:
        for seg in (0, 1, 3, 64, 200):
            need = L.pps_search_h2_workspace_bytes(N, N, 21, seg)
            have = feat(1, N - 1, 20, 6, seg) - rows(1, N - 1, 20, 6)
            assert 0 < need <= have, (N, seg, need, have)
    # per-row structures of about 27 KB: far below the matrix
    Q, G = 10000, 1000000
    N = Q + G
    f = feat(Q, G, 20, 6, 0)
    assert f < 4 * N * N / 50, (f, 4 * N * N / f)
    assert 24 * 1024 * N < rows(Q, G, 20, 6) < 30 * 1024 * N


def test_abi_version_unchanged():
    assert _lib().pps_abi_version() == 1
