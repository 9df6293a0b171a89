"""Guards of the matrix-free rank entry points (pps_collect_matches_h2,
pps_rank_count_h2_tiled and its two host queries), without a GPU: every guard
returns before the first GPU call, so dummy host pointers are enough.  Each
case gives one bad argument and expects the status and the end of
pps_last_error(); the planes arguments carry pps_search_h2_tiled's texts."""
import ctypes

import pytest

OK, INVALID_ARG, CAPACITY = 0, -1, -4
_BUF = ctypes.create_string_buffer(256 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # a non-null, 16-byte aligned host pointer
CAP = 1024                                       # kRankH2MaxP (csrc/retrieval.hpp)


def _lib():
    from pps_amd import _lib
    return _lib.lib()


def _call(name, args):
    L = _lib()
    status = getattr(L, name)(*args)
    return status, L.pps_last_error().decode('utf-8')


# argument positions of the two entry points (include/pps_abi.h)
COUNT = dict(q2t=0, Q=1, qsq=2, qrs=3, g2t=4, gsq=5, grs=6, G=7, D=8, metric=9, g_offset=10,
             Ptot=11, sorted_d=12, sorted_idx=13, pos_total=14, Jmax=15, junk_d=16, junk_idx=17,
             junk_cnt=18, segments=19, tile=20, workspace=21, ws_bytes=22, hist=23, before=24,
             stream=25)
COUNT_GOOD = [P, 1, P, P, P, P, P, 1, 32, 0, 0, 1, P, P, P, 1, P, P, P, 0, 0, None, 0, P, P, None]
PAIR = dict(q2t=0, Q=1, qsq=2, qrs=3, g2t=4, gsq=5, grs=6, G=7, D=8, metric=9, qcam=10, gcam=11,
            members=12, q_beg=13, q_end=14, g_offset=15, Pmax=16, pos_d=17, pos_idx=18,
            pos_cnt=19, Jmax=20, junk_d=21, junk_idx=22, junk_cnt=23, stream=24)
PAIR_GOOD = [P, 1, P, P, P, P, P, 1, 32, 0, P, P, P, P, P, 0, 1, P, P, P, 1, P, P, P, None]


def _with(good, pos, **kw):
    args = list(good)
    for k, v in kw.items():
        args[pos[k]] = v
    return tuple(args)


CASES = [
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, D=33), 'bad shape (D % 32 == 0)'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, D=0), 'bad shape (D % 32 == 0)'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Q=-1), 'bad shape (D % 32 == 0)'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Q=2 ** 31), 'Q must fit int32'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, metric=3), 'unknown metric'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Q=2 ** 20, D=1024),
     'planes over 2 GiB'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Ptot=0), 'bad shape'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Jmax=0), 'bad shape'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, g_offset=2 ** 31 - 1),
     'gallery indices must fit int32'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, segments=-1),
     'segments must be >= 0 (0 = auto)'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, tile=3), 'search tile must be 0..2'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, tile=-1), 'search tile must be 0..2'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, hist=None), 'null pointer'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, sorted_d=None), 'null pointer'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, g2t=None), 'null pointer'),
    ('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, q2t=P + 8),
     'planes must be 16-byte aligned'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, D=40), 'bad shape (D % 32 == 0)'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, metric=-1), 'unknown metric'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, G=2 ** 20, D=1024), 'planes over 2 GiB'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, Pmax=0), 'bad shape'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, Jmax=0), 'bad shape'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, g_offset=2 ** 31 - 1),
     'gallery indices must fit int32'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, members=None), 'null pointer'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, pos_cnt=None), 'null pointer'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, qsq=None), 'null pointer'),
    ('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, g2t=P + 8),
     'planes must be 16-byte aligned'),
]


@pytest.mark.parametrize('name,args,tail', CASES,
                         ids=['%s-%d' % (c[0], i) for i, c in enumerate(CASES)])
def test_guard_status_and_text(name, args, tail):
    status, msg = _call(name, args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.startswith('[enforce fail at %s] ' % name), msg
    assert msg.endswith('. ' + tail), msg


def test_ptot_above_the_cap_is_a_capacity_error_naming_the_cap():
    status, msg = _call('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Ptot=CAP + 1))
    assert status == CAPACITY, (status, msg)
    assert msg.startswith('pps_rank_count_h2_tiled: Ptot = %d ' % (CAP + 1)), msg
    assert msg.endswith('at most %d (pps_rank_count_h2_max_p)' % CAP), msg
    # the cap itself passes the check: with Q == 0 the call then returns before any launch
    status, msg = _call('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, Ptot=CAP, Q=0))
    assert status == OK, (status, msg)


def test_empty_operands_return_ok_without_a_launch():
    for kw in (dict(Q=0), dict(G=0), dict(Q=0, G=0)):
        status, msg = _call('pps_rank_count_h2_tiled', _with(COUNT_GOOD, COUNT, **kw))
        assert status == OK, (kw, status, msg)
    status, msg = _call('pps_collect_matches_h2', _with(PAIR_GOOD, PAIR, Q=0))
    assert status == OK, (status, msg)


def test_max_p_exported():
    assert _lib().pps_rank_count_h2_max_p() == CAP
    assert CAP >= 256


def test_workspace_bytes_bad_arguments():
    ws = _lib().pps_rank_count_h2_workspace_bytes
    assert ws(100, 1000, 64, 0) >= 0
    for args in ((-1, 1000, 64, 0), (100, -1, 64, 0), (100, 1000, 0, 0),
                 (100, 1000, CAP + 1, 0), (100, 1000, 64, -1)):
        assert ws(*args) == -1, args


@pytest.mark.parametrize('Q,Ptot,segments', [(1, 1, 0), (300, 150, 0), (3368, 64, 3),
                                             (10000, CAP, 0), (10000, 64, 64)])
def test_workspace_bytes_non_decreasing_in_G(Q, Ptot, segments):
    ws = _lib().pps_rank_count_h2_workspace_bytes
    sizes = [0, 1, 191, 192, 193, 255, 256, 257, 1100, 15913, 125000, 10 ** 6]
    got = [ws(Q, G, Ptot, segments) for G in sizes]
    assert all(g >= 0 for g in got), got
    assert got == sorted(got), got
