"""Guards and the size function of re-ranking against a prepared gallery
(pps_re_ranking_prepared, pps_pair_dist_h2_parts,
pps_rerank_prepared_workspace_bytes), without a GPU: every guard returns
before the first GPU call, so dummy host pointers are enough.  Each case gives
one bad argument and expects the status and the end of pps_last_error()."""
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
PREP = 'pps_re_ranking_prepared'
PREP_POS = dict(q2t=0, qsq=1, qrs=2, g2t=3, gsq=4, grs=5, Q=6, G=7, D=8, metric=9, nn_vals=10,
                nn_idx=11, nn_ld=12, g_rowmax=13, k1=14, k2=15, lam=16, segments=17, tile=18,
                g_window=19, workspace=20, ws_bytes=21, out=22, stream=23)
PREP_GOOD = [P, P, P, P, P, P, 100, 400, 64, 0, P, P, 21, P, 20, 6, 0.3, 0, 0, 0, P, 0, P, None]
PARTS = 'pps_pair_dist_h2_parts'
PARTS_POS = dict(q2t=0, Q=1, qsq=2, qrs=3, b0_2t=4, b0sq=5, b0rs=6, B0=7, b1_2t=8, b1sq=9,
                 b1rs=10, B1=11, D=12, metric=13, lists=14, counts=15, cap=16, out=17, stream=18)
PARTS_GOOD = [P, 1, P, P, P, P, P, 1, P, P, P, 1, 32, 0, P, None, 4, P, None]


def _with(good, pos, **kw):
    args = list(good)
    for k, v in kw.items():
        args[pos[k]] = v
    return tuple(args)


def _prep(**kw):
    return _with(PREP_GOOD, PREP_POS, **kw)


def _parts(**kw):
    return _with(PARTS_GOOD, PARTS_POS, **kw)


def _prep_cases():
    tiles = _lib().pps_search_h2_num_tiles()
    return [
        (_prep(D=40), 'bad shape (D % 32 == 0)'),
        (_prep(D=0), 'bad shape (D % 32 == 0)'),
        (_prep(metric=3), 'unknown metric'),
        (_prep(k1=64), 'k1 + 1 must be <= 64 and <= pps_search_max_k()'),
        (_prep(k1=0), 'k1 + 1 must be <= 64 and <= pps_search_max_k()'),
        (_prep(k2=0), 'k2 must be in [1, k1 + 1]'),
        (_prep(k2=22), 'k2 must be in [1, k1 + 1]'),
        (_prep(Q=5, G=10), 'need Q + G >= k1 + 1'),
        (_prep(Q=0), 'bad shape'),
        (_prep(G=0), 'bad shape'),
        (_prep(G=2 ** 31), 'N = Q + G must fit int32'),
        (_prep(G=2 ** 20, D=1024, k2=1), 'planes over 2 GiB'),       # the gallery's
        (_prep(Q=2 ** 20, D=1024, k2=1), 'planes over 2 GiB'),       # the queries'
        (_prep(segments=-1), 'segments must be >= 0 (0 = auto)'),
        (_prep(tile=tiles), 'search tile must be 0..%d' % (tiles - 1)),
        (_prep(g_window=-1), 'g_window must be in [0, 38400] (0 = auto)'),
        (_prep(g_window=38401), 'g_window must be in [0, 38400] (0 = auto)'),
        (_prep(nn_ld=20), 'nn_ld must be >= k1 + 1'),
        (_prep(q2t=None), 'null pointer'),
        (_prep(grs=None), 'null pointer'),
        (_prep(nn_vals=None), 'null pointer'),
        (_prep(nn_idx=None), 'null pointer'),
        (_prep(g_rowmax=None), 'null pointer'),
        (_prep(out=None), 'null pointer'),
        (_prep(workspace=None), 'null pointer'),
        (_prep(q2t=P + 8), 'planes must be 16-byte aligned'),
        (_prep(g2t=P + 8), 'planes must be 16-byte aligned'),
        (_prep(workspace=P + 16), 'workspace must be 256-byte aligned'),
    ]


@pytest.mark.parametrize('i', range(28))
def test_prepared_guard_status_and_text(i):
    cases = _prep_cases()
    assert len(cases) == 28
    args, tail = cases[i]
    status, msg = _call(PREP, args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.startswith('[enforce fail at '), msg
    assert PREP in msg, msg                       # the public entry is named
    assert msg.endswith('. ' + tail), msg


def test_prepared_accepts_a_wider_prepared_row():
    """nn_ld above k1 + 1 passes the guards: the call gets as far as the
    workspace check (ws_bytes = 0)."""
    status, msg = _call(PREP, _prep(nn_ld=64, k1=6, k2=3))
    assert status == CAPACITY and 'workspace too small: need ' in msg, (status, msg)


def test_capacity_errors_come_before_any_launch():
    """N * qcap >= 2^31 (qcap = k2 * 256 at k1 = 20) and a workspace smaller
    than the size function's value are PPS_ERR_CAPACITY."""
    status, msg = _call(PREP, _prep(Q=10 ** 6, G=10 ** 6))      # 2e6 * 1536 >= 2^31
    assert status == CAPACITY, (status, msg)
    assert msg.startswith(PREP + ': N * qcap = 2000000 * 1536 '), msg
    need = _lib().pps_rerank_prepared_workspace_bytes(100, 400, 20, 6, 0)
    for have in (0, need - 1):
        status, msg = _call(PREP, _prep(ws_bytes=have))
        assert status == CAPACITY, (status, msg)
        assert msg.endswith('workspace too small: need %d bytes' % need), msg


def test_pair_dist_parts_guards():
    for kw, tail in [(dict(lists=None), 'null pointer'), (dict(out=None), 'null pointer'),
                     (dict(D=40), 'bad shape (D % 32 == 0)'), (dict(metric=-1), 'unknown metric'),
                     (dict(cap=0), 'cap must be >= 1'),
                     (dict(Q=2 ** 20, D=1024), 'planes over 2 GiB'),
                     (dict(B0=2 ** 20, D=1024), 'planes over 2 GiB'),
                     (dict(B1=2 ** 20, D=1024), 'planes over 2 GiB'),
                     (dict(B0=0), 'a listed pair needs a b-row in each part (B0, B1 > 0)'),
                     (dict(B1=0), 'a listed pair needs a b-row in each part (B0, B1 > 0)'),
                     (dict(b0_2t=None), 'null pointer'), (dict(b1rs=None), 'null pointer'),
                     (dict(q2t=P + 8), 'planes must be 16-byte aligned'),
                     (dict(b1_2t=P + 8), 'planes must be 16-byte aligned')]:
        status, msg = _call(PARTS, _parts(**kw))
        assert status == INVALID_ARG and msg.endswith('. ' + tail), (kw, status, msg)
        assert PARTS in msg, msg
    assert _call(PARTS, _parts(Q=0))[0] == OK


def test_size_function():
    L = _lib()
    size, rows = L.pps_rerank_prepared_workspace_bytes, L.pps_rerank_rows_workspace_bytes
    search = L.pps_search_h2_workspace_bytes
    # bad arguments
    for bad in [(-1, 10, 20, 6, 0), (10, -1, 20, 6, 0), (10, 10, 0, 6, 0), (10, 10, 64, 6, 0),
                (10, 10, 20, 0, 0), (10, 10, 20, 22, 0), (10, 10, 20, 6, -1)]:
        assert size(*bad) == -1, bad
    gs = list(range(0, 3000, 37)) + [17661, 38400, 38401, 150000, 10 ** 6]
    qs = list(range(0, 3000, 37)) + [5000, 10000, 38401, 150000]
    segs = (0, 1, 3, 64, 200)
    # non-decreasing in G ...
    for Q in (1, 64, 150, 2228, 10000):
        for seg in segs:
            prev = 0
            for G in gs:
                s = size(Q, G, 20, 6, seg)
                assert s >= prev and s >= rows(Q, G, 20, 6) > 0, (Q, G, seg, s, prev)
                prev = s
    # ... and in Q
    for G in (1, 650, 17661, 150000):
        for seg in segs:
            prev = 0
            for Q in qs:
                s = size(Q, G, 20, 6, seg)
                assert s >= prev, (Q, G, seg, s, prev)
                prev = s
    # it holds rerank_rows' carves and each of the three searches' workspaces
    shapes = [(q, g) for q in (1, 5, 64, 150, 193, 2228, 10000)
              for g in (21, 650, 1100, 17661, 38401, 150000, 10 ** 6)]
    for Q, G in shapes:
        for k1 in (20, 6):
            for seg in segs:
                have = size(Q, G, k1, 3, seg) - rows(Q, G, k1, 3)
                for a, b in ((Q, Q), (G, Q), (Q, G)):
                    need = search(a, b, k1 + 1, seg)
                    assert 0 < need <= have, (Q, G, k1, seg, a, b, need, have)
    # per-row structures: far below the matrix
    Q, G = 10000, 1000000
    N = Q + G
    assert size(Q, G, 20, 6, 0) < 4 * N * N / 50


def test_abi_version_unchanged():
    assert _lib().pps_abi_version() == 1
