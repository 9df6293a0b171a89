"""Guards of the matrix-free CMC count entry (pps_cmc_count_h2_tiled), without
a GPU: every guard returns before the first GPU call, so dummy host pointers
are enough.  Each case gives one bad argument and expects the status and the
end of pps_last_error(); the planes, segments, tile and capacity arguments
carry pps_rank_count_h2_tiled's texts, the camera and junk rules
pps_cmc_counts'."""
import ctypes

import pytest

OK, INVALID_ARG, CAPACITY = 0, -1, -4
NAME = 'pps_cmc_count_h2_tiled'
_BUF = ctypes.create_string_buffer(256 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # a non-null, 16-byte aligned host pointer

# argument positions (include/pps_abi.h)
POS = dict(q2t=0, Q=1, qsq=2, qrs=3, g2t=4, gsq=5, grs=6, G=7, D=8, metric=9, g_offset=10,
           Ptot=11, sorted_d=12, sorted_idx=13, pos_total=14, qcam=15, gcam=16, Jmax=17,
           junk_d=18, junk_idx=19, junk_cnt=20, segments=21, tile=22, workspace=23, ws_bytes=24,
           hist=25, stream=26)
JUNK_GOOD = [P, 1, P, P, P, P, P, 1, 32, 0, 0, 1, P, P, P, None, None, 1, P, P, P, 0, 0, None, 0,
             P, None]
CAMS = 'qcam and gcam are given together (separate_camera_set) or not at all'
JUNK = 'without separate_camera_set the junk lists are required'


def _lib():
    from pps_amd import _lib
    return _lib.lib()


def _call(args):
    L = _lib()
    status = getattr(L, NAME)(*args)
    return status, L.pps_last_error().decode('utf-8')


def _with(**kw):
    args = list(JUNK_GOOD)
    for k, v in kw.items():
        args[POS[k]] = v
    return tuple(args)


SEP = dict(qcam=P, gcam=P, Jmax=0, junk_d=None, junk_idx=None, junk_cnt=None)


def _cases():
    tiles = _lib().pps_search_h2_num_tiles()
    tile_text = 'search tile must be 0..%d' % (tiles - 1)
    return [
        (_with(D=40), 'bad shape (D % 32 == 0)'),
        (_with(D=40, **SEP), 'bad shape (D % 32 == 0)'),
        (_with(Q=2 ** 31), 'Q must fit int32'),
        (_with(metric=3), 'unknown metric'),
        (_with(Q=2 ** 20, D=1024), 'planes over 2 GiB'),
        (_with(Ptot=0), 'bad shape'),
        (_with(g_offset=2 ** 31 - 1), 'gallery indices must fit int32'),
        (_with(segments=-1), 'segments must be >= 0 (0 = auto)'),
        (_with(tile=tiles), tile_text),
        (_with(tile=-1), tile_text),
        (_with(qcam=P), CAMS),
        (_with(gcam=P), CAMS),
        (_with(junk_d=None), JUNK),
        (_with(junk_idx=None), JUNK),
        (_with(junk_cnt=None), JUNK),
        (_with(Jmax=0), JUNK),
        (_with(hist=None), 'null pointer'),
        (_with(sorted_idx=None), 'null pointer'),
        (_with(g2t=None), 'null pointer'),
        (_with(q2t=P + 8), 'planes must be 16-byte aligned'),
    ]


@pytest.mark.parametrize('i', range(20))
def test_guard_status_and_text(i):
    cases = _cases()
    assert len(cases) == 20
    args, tail = cases[i]
    status, msg = _call(args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.startswith('[enforce fail at %s] ' % NAME), msg
    assert msg.endswith('. ' + tail), msg


@pytest.mark.parametrize('mode', ['junk', 'separate_camera'])
def test_ptot_above_the_cap_is_a_capacity_error_naming_the_cap(mode):
    kw = SEP if mode == 'separate_camera' else {}
    cap = _lib().pps_rank_count_h2_max_p()
    status, msg = _call(_with(Ptot=cap + 1, **kw))
    assert status == CAPACITY, (status, msg)
    assert msg.startswith('%s: Ptot = %d ' % (NAME, cap + 1)), msg
    assert msg.endswith('at most %d (pps_rank_count_h2_max_p)' % cap), msg
    # the cap itself passes the check: with Q == 0 the call then returns before any launch
    status, msg = _call(_with(Ptot=cap, Q=0, **kw))
    assert status == OK, (status, msg)


def test_empty_operands_return_ok_without_a_launch():
    for kw in (dict(Q=0), dict(G=0), dict(Q=0, G=0), dict(Q=0, **SEP), dict(G=0, **SEP)):
        status, msg = _call(_with(**kw))
        assert status == OK, (kw, status, msg)


def test_separate_camera_mode_takes_null_junk_lists():
    # both cams given: the junk pointers and Jmax are not looked at (Q == 0 ends the call)
    status, msg = _call(_with(Q=0, **SEP))
    assert status == OK, (status, msg)


def test_abi_version_unchanged():
    assert _lib().pps_abi_version() == 1
