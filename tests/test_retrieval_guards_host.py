"""Capacity guards of the retrieval entry points, without a GPU: every guard
returns before the first GPU call, so dummy host pointers are enough.  Each
case gives one out-of-range argument and expects the status and the end of
pps_last_error() -- the limits are named once in csrc/retrieval.hpp, and the
texts a caller sees must not move with them."""
import ctypes

import pytest

INVALID_ARG = -1
_BUF = ctypes.create_string_buffer(256 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # a non-null, 16-byte aligned host pointer
_OFFS = (ctypes.c_int64 * 64)()
OFFS = ctypes.addressof(_OFFS)
CHUNK = 8192                                     # gallery entries per workgroup of the rank streams
G_CHUNKS = 65535 * CHUNK + 1                     # one chunk past the 65535-chunk grid
ARGSORT_CAP = 458752


def _fails(name, *args):
    from pps_amd import _lib
    L = _lib.lib()
    status = getattr(L, name)(*args)
    return status, L.pps_last_error().decode('utf-8')


CASES = [
    ('pps_topk', (P, 1, 4096, 4096, 0, P, P, None),
     'k must be in [1, 1024], got 0'),
    ('pps_topk', (P, 1, 4096, 4096, 1025, P, P, None),
     'k must be in [1, 1024], got 1025'),
    ('pps_topk_merge', (P, P, 65, 1, 1, OFFS, 1, P, P, None),
     'R must be in [1, 64]'),
    ('pps_topk_merge', (P, P, 1, 1, 8193, OFFS, 1, P, P, None),
     'R * k_in must be <= 8192 (LDS), got 8193'),
    ('pps_rank_prepare', (65, 1, 1, P, P, P, P, P, P, P, None),
     'R must be in [1, 64]'),
    ('pps_rank_count_stream',
     (P, 1, G_CHUNKS, G_CHUNKS, 0, 1, P, P, P, P, 1, P, P, P, P, P, None),
     'G too large for the chunk grid (65535 chunks of 8192)'),
    ('pps_cmc_counts',
     (P, 1, G_CHUNKS, G_CHUNKS, 0, 1, P, P, P, None, None, 1, P, P, P, P, None),
     'G too large for the chunk grid'),
    ('pps_sgs_keys', (P, 1, 1, 1, P, P, P, P, 0, 16385, P, None),
     'U (distinct gallery identities) must be in [1, 16384]'),
    ('pps_sgs_groups', (P, P, 1, 1, 16385, P, P, P, P, P, None),
     'U (distinct gallery identities) must be in [1, 16384]'),
    ('pps_sgs_ranks', (P, 1, 1, P, 1, P, P, P, P, 16385, 1, P, 1, P, None),
     'ldd must be in [1, U]'),
    ('pps_argsort_rows',
     (P, 1, ARGSORT_CAP + 1, ARGSORT_CAP + 1, P, ARGSORT_CAP + 1, None, 0, None),
     'rows longer than 458752 entries (pps_argsort_rows_cap): use pps_topk'),
]


@pytest.mark.parametrize('name,args,tail', CASES,
                         ids=['%s-%d' % (c[0], i) for i, c in enumerate(CASES)])
def test_guard_status_and_text(name, args, tail):
    status, msg = _fails(name, *args)
    assert status == INVALID_ARG, (status, msg)
    assert msg.startswith('[enforce fail at %s] ' % name), msg
    assert msg.endswith('. ' + tail), msg


def test_limits_exported():
    from pps_amd import _lib
    L = _lib.lib()
    assert L.pps_rank_cells() == 1024
    assert L.pps_argsort_rows_cap() == ARGSORT_CAP
