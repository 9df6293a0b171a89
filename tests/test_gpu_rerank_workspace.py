"""Guard bands around the workspace of every re-ranking form (RrCarve, DESIGN
6.1.7): each C entry, called directly with exactly its size function's bytes
between two 4 KiB bands of 0xA5, leaves both bands untouched and returns, bit
for bit, what it returns with a generously over-sized workspace.

Shapes are the smallest at which every region of the carve is non-empty and
the gallery is no multiple of any tile: Q = 5, G = 37 (N = 42), D = 32,
(k1, k2) = (6, 3), and k2 = 1 once for the prepared form (V_qe = V).  The
in-place dense path (N >= 16384) is compared with the dense one by
test_rerank_inplace_equals_dense_duke_shape."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

Q, G, D, K1, K2 = 5, 37, 32, 6, 3
N = Q + G
BAND = 4096
FILL = 0xA5
SYMMETRIC = 1


@functools.lru_cache(maxsize=None)
def _data():
    """Everything the entries read, built once and left unchanged."""
    from pps_amd import ops
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11)
    x = torch.randn((N, D), generator=gen, device='cuda')
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    q, g = x[:Q].contiguous(), x[Q:].contiguous()
    W = ops.compute_dist(x, ops.GalleryIndex(x, math='h2'), math='h2', symmetric=False)
    M = torch.maximum(W, W.t()).contiguous()           # exactly symmetric
    d = dict(x=x, W=W.contiguous(),
             q_g=M[:Q, Q:].contiguous(), q_q=M[:Q, :Q].contiguous(), g_g=M[Q:, Q:].contiguous(),
             x_split=ops.split_h2_tiled(x), g_split=ops.split_h2_tiled(g),
             q_split=ops.split_h2_tiled(q), gallery=ops.RerankGallery(g, k1=K1))
    torch.cuda.synchronize()
    return d


class _Banded(object):
    """nbytes of workspace at a 256-byte aligned address with a band on each
    side, all inside one tensor filled with FILL."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * BAND + 256,), FILL, dtype=torch.uint8, device='cuda')
        self.off = BAND + (-(self.buf.data_ptr() + BAND)) % 256
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0

    def bands_untouched(self):
        lo = self.buf[self.off - BAND:self.off]
        hi = self.buf[self.off + self.nbytes:self.off + self.nbytes + BAND]
        return bool((lo == FILL).all()) and bool((hi == FILL).all())


def _run(entry, size, args):
    """entry(*args, workspace, ws_bytes, out, stream) with the exact and
    with an over-sized workspace -> both results, after the band check."""
    from pps_amd import _lib
    assert size > 0 and size % 256 == 0
    stream = torch.cuda.current_stream().cuda_stream
    exact = _Banded(size)
    out = torch.full((Q, G), float('nan'), device='cuda')
    _lib.call(entry, *(args + (exact.ptr, size, out.data_ptr(), stream)))
    torch.cuda.synchronize()
    assert exact.bands_untouched()
    big = _Banded(4 * size + (1 << 20))
    ref = torch.full((Q, G), float('nan'), device='cuda')
    _lib.call(entry, *(args + (big.ptr, big.nbytes, ref.data_ptr(), stream)))
    torch.cuda.synchronize()
    assert big.bands_untouched()
    assert torch.isfinite(ref).all()
    assert torch.equal(out, ref)


@pytest.mark.parametrize('flags', [0, SYMMETRIC])
def test_dense_form_stays_inside_its_size(flags):
    from pps_amd import _lib
    d = _data()
    blocks = (d['q_g'].data_ptr(), G, d['q_q'].data_ptr(), Q, d['g_g'].data_ptr(), G)
    size = _lib.lib().pps_rerank_workspace_bytes_ld(*blocks, Q, G, K1, K2, flags)
    assert size == _lib.lib().pps_rerank_workspace_bytes(Q, G, K1, K2)      # N < 16384: dense
    _run('pps_re_ranking_ld', size, blocks + (Q, G, K1, K2, 0.3, flags))


def test_rows_form_stays_inside_its_size():
    from pps_amd import _lib
    d = _data()
    size = _lib.lib().pps_rerank_rows_workspace_bytes(Q, G, K1, K2)
    _run('pps_re_ranking_rows', size, (d['W'].data_ptr(), N, Q, G, K1, K2, 0.3, 0))


def test_features_form_stays_inside_its_size():
    from pps_amd import _lib, ops
    d = _data()
    size = _lib.lib().pps_rerank_features_workspace_bytes(Q, G, K1, K2, 0)
    operands = ops._h2_split_args(d['x_split'], 'x') + ops._h2_split_args(d['g_split'], 'g')
    _run('pps_re_ranking_features', size,
         operands + (Q, G, D, ops.METRICS['euclidean'], K1, K2, 0.3, 0, 0, 0))


@pytest.mark.parametrize('k2', [K2, 1])
def test_prepared_form_stays_inside_its_size(k2):
    from pps_amd import _lib, ops
    d = _data()
    rg = d['gallery']
    size = _lib.lib().pps_rerank_prepared_workspace_bytes(Q, G, K1, k2, 0)
    operands = ops._h2_split_args(d['q_split'], 'q') + ops._h2_split_args(rg.index.h2, 'g')
    _run('pps_re_ranking_prepared', size,
         operands + (Q, G, D, ops.METRICS[rg.metric], rg.nn_vals.data_ptr(),
                     rg.nn_idx.data_ptr(), rg.nn_vals.shape[1], rg.rowmax.data_ptr(), K1, k2, 0.3,
                     0, 0, 0))
