"""Device operators over torch CUDA tensors, backed by libpps_hip.so.

torch is used only for device memory and the current HIP stream; every
computation below is a libpps_hip.so kernel.  Each wrapper checks device,
dtype and contiguity, then calls the C ABI on torch's current stream.

Also hosts the operator registry that mirrors the reference's Caffe2 op names
(`model.net.PairWiseDistance(X, Z)`, detectron/modeling/triplet_loss.py:145;
registration detectron/ops/pairwise_distance_op.cu:124-127), so code written
against that registry can look ops up by the same names.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import METRICS, call


TILE_P_FIRST = 29  # first pipelined (gemm_x3p.hip) tile id, include/pps_abi.h
TILE_P16_FIRST = 38  # pipelined tiles on 16x16x32 MFMA blocks (their own rounding)
TILE_C16_FIRST = 56  # patch-staged 3x3 tiles (gemm_x3c.hip): K in (channel chunk, tap) order
TILE_B_TILED = 0x100  # PPS_TILE_B_TILED: or-ed into a conv tile, the weights are chunk-tiled
TILE_COL_ORDER = 0x200  # PPS_TILE_COL_ORDER: column-major output tile order (same bits)
TILE_SEAM = 0x400  # PPS_TILE_SEAM (whole-network plan): branch2c + next branch2a in one launch
TILE_H2 = 0x800    # PPS_TILE_H2 (whole-network plan): the layer in f16x2 arithmetic
TILE_H2P = 0x1000  # PPS_TILE_H2P: with TILE_H2, the input split once into f16x2 planes
TILE_H2E = 0x2000  # PPS_TILE_H2E: with TILE_H2, the input arrives as f16x2 planes its
                   # producer wrote on the scale of an output bound (conv2d_bn_act_h2out)
TILE_WS = 54       # the weight-stationary 1x1 tile (gemm_ws.hip)
TILE_H2_WIDE = 60  # 192x128 as 4 x 1 waves: f16x2 only (bf16x3 launches run tile 47)
TILE_FLAGS = TILE_B_TILED | TILE_COL_ORDER | TILE_SEAM | TILE_H2 | TILE_H2P | TILE_H2E   # every or-ed flag
# tiles built with the one-launch split-K epilogue (conv2d_bn_act_x3p(..., counters=))
FIX_TILES = (45, 47, 48, 49, 50)
PPS_FUSE_MAX_COLS = 256  # widest tile the fused part pooling takes (pps_internal.hpp)


def num_tiles():
    return _lib.lib().pps_gemm_num_tiles()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a device (HIP) tensor; the product path has no '
                           'CPU implementation' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    return t.data_ptr()


def _dev_rows(t, name, dtype=torch.float32):
    """A 2-D device matrix whose rows may be padded (stride(1) == 1,
    stride(0) >= columns): distance matrices are passed with their row
    stride (ld*) so a [Q, G] view of a wider buffer needs no copy."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise RuntimeError('%s must be a 2-D torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a device (HIP) tensor; the product path has no '
                           'CPU implementation' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        raise RuntimeError('%s must have unit column stride and row stride >= columns'
                           % name)
    return t.data_ptr()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


# ---------------------------------------------------------------------------
# Retrieval
# ---------------------------------------------------------------------------
def default_math():
    """'x3' (f32 products on bf16 matrix cores, f32-level error) unless the
    environment asks for the exact-f32 MFMA kernels with PPS_MATH=f32."""
    m = os.environ.get('PPS_MATH', 'x3')
    if m not in ('x3', 'f32'):
        raise ValueError('PPS_MATH must be x3 or f32, got %r' % m)
    return m


def dist_math():
    """Arithmetic of the distance GEMMs (compute_dist and everything built on
    it): 'h2' (default: f16x2, three f16 MFMA terms per product, f32-level
    error -- csrc/gemm_h2.hip), 'x3' (six bf16 terms) or 'f32' (exact f32
    MFMA), from PPS_DIST_MATH; PPS_MATH=f32 (exact f32 everywhere) also
    selects 'f32' here."""
    m = os.environ.get('PPS_DIST_MATH')
    if m is None:
        return 'f32' if default_math() == 'f32' else 'h2'
    if m not in ('h2', 'x3', 'f32'):
        raise ValueError('PPS_DIST_MATH must be h2, x3 or f32, got %r' % m)
    return m


def h2_num_tiles():
    return int(_lib.lib().pps_h2_num_tiles())


def split_h2_tiled(x):
    """f16x2 split of a [R, D] tensor (D % 32 == 0) for the h2 distance GEMM,
    one read of x: -> (planes, rscale, sqnorm) with planes the two f16 planes
    chunk-tiled as an int16 [2, R16, D] tensor, rscale [R] the per-row
    power-of-two inverse scales, sqnorm [R] = row_sqnorm(x) (same bits)."""
    R, D = x.shape
    r16 = (R + 15) // 16 * 16
    planes = torch.empty((2, r16, D), dtype=torch.int16, device=x.device)
    rs = torch.empty((R,), dtype=torch.float32, device=x.device)
    sq = torch.empty((R,), dtype=torch.float32, device=x.device)
    call('pps_split_f16x2_sqnorm_tiled', _dev(x, 'x'), R, D, D, _dev(planes, 'out2t', torch.int16), _dev(rs, 'rscale'), _dev(sq, 'sqnorm'), _stream())
    return planes, rs, sq


def row_sqnorm(x):
    """Squared L2 norm of every row of a [R, D] tensor (fixed summation order)."""
    R, D = x.shape
    out = torch.empty((R,), dtype=torch.float32, device=x.device)
    call('pps_row_sqnorm', _dev(x, 'x'), R, D, x.stride(0), _dev(out, 'out'), _stream())
    return out


def split_sqnorm(x):
    """(split_bf16x3(x), row_sqnorm(x)) of a [R, D] tensor from one read of x
    (pps_split_bf16x3_sqnorm; same bits as the two calls).  Planes [3, R, D]."""
    R, D = x.shape
    planes = torch.empty((3, R, D), dtype=torch.int16, device=x.device)
    sq = torch.empty((R,), dtype=torch.float32, device=x.device)
    call('pps_split_bf16x3_sqnorm', _dev(x, 'x'), R, D, x.stride(0),
         _dev(planes, 'out3', torch.int16), _dev(sq, 'sqnorm'), _stream())
    return planes, sq


def split_sqnorm_tiled(x):
    """split_sqnorm writing the planes chunk-tiled (tile_planes' layout, as an
    int16 [3, R16, D] tensor) from one read of x; D % 32 == 0.  Same bits."""
    R, D = x.shape
    r16 = (R + 15) // 16 * 16
    planes = torch.empty((3, r16, D), dtype=torch.int16, device=x.device)
    sq = torch.empty((R,), dtype=torch.float32, device=x.device)
    call('pps_split_bf16x3_sqnorm_tiled', _dev(x, 'x'), R, D, x.stride(0),
         _dev(planes, 'out3t', torch.int16), _dev(sq, 'sqnorm'), _stream())
    return planes, sq


class GalleryIndex(object):
    """A gallery prepared once for the distance GEMM; score any number of
    query batches against it with compute_dist(q, index).  math 'h2' (the
    dist_math() default when D % 32 == 0): the f16x2 split (split_h2_tiled:
    two chunk-tiled f16 planes, per-row scales, squared norms); 'x3': the
    features split into three bf16 planes + squared norms, tiled=True in the
    chunk-tiled layout the query-planes GEMM streams (one pass; the row-major
    planes are then split on first use)."""

    def __init__(self, g, tiled=False, math=None):
        if g.dim() != 2:
            raise RuntimeError('gallery must be [G, D], got %s' % (tuple(g.shape),))
        self.feats = g
        self._planes = self._tiled = self.h2 = None
        math = math or dist_math()
        if math == 'f32':
            math = 'x3'   # an index is a split; f32 distances take the features as they are
        if math == 'h2' and not (g.is_contiguous() and g.shape[1] % 32 == 0):
            math = 'x3'   # the f16x2 kernel needs D % 32 == 0 (chunk-tiled planes)
        self.math = math
        if math == 'h2':
            self.h2 = split_h2_tiled(g)   # (planes, rscale, sqnorm)
            self.sqnorm = self.h2[2]
        elif tiled and g.is_contiguous() and g.shape[1] % 32 == 0:
            self._tiled, self.sqnorm = split_sqnorm_tiled(g)
        elif g.is_contiguous() and g.shape[1] % 4 == 0:
            self._planes, self.sqnorm = split_sqnorm(g)
        else:
            self._planes = split_bf16x3(g)
            self.sqnorm = row_sqnorm(g)

    @staticmethod
    def split_rows(G, D, max_rows=None):
        """Row ranges [(start, rows), ...] of a G-row gallery cut into
        consecutive segments of at most max_rows rows; every segment but the
        last is a multiple of 16 rows.  max_rows None = the largest multiple of
        16 whose two f16 planes stay under the 2 GiB one index can address
        (2 * rows * D * 2 bytes < 2^31)."""
        G, D = int(G), int(D)
        limit = ((2 ** 31 - 1) // (4 * D)) // 16 * 16
        if limit < 16:
            raise RuntimeError('GalleryIndex.split: D=%d too wide for one 16-row block' % D)
        step = limit if max_rows is None else min(limit, max(16, int(max_rows) // 16 * 16))
        return [(a, min(step, G - a)) for a in range(0, G, step)] or [(0, 0)]

    @classmethod
    def split(cls, g, max_rows=None, math=None):
        """A gallery larger than one index may be: a list of GalleryIndex over
        consecutive row segments (split_rows), which ops.search takes as one
        logical gallery and answers with global indices."""
        if g.dim() != 2:
            raise RuntimeError('gallery must be [G, D], got %s' % (tuple(g.shape),))
        return [cls(g[a:a + n], math=math) for a, n in cls.split_rows(g.shape[0], g.shape[1], max_rows)]

    @property
    def shape(self):
        return self.feats.shape

    @property
    def planes(self):
        """Row-major planes [3, G, D]."""
        if self._planes is None:
            self._planes = split_bf16x3(self.feats)
        return self._planes

    @property
    def tiled_planes(self):
        """The planes chunk-tiled (tile_planes' layout), built on first use."""
        if self._tiled is None:
            self._tiled = tile_planes(self.planes)
        return self._tiled


# tiles the symmetric self-distance takes: every pipelined tile (the upper
# triangle is enumerated by lcm(BM, BN) super-blocks); 0 = tile 43
SELF_TILES = (0,) + tuple(range(TILE_P_FIRST, 54)) + (55,)


def dist_buffer(Q, G, device):
    """[Q, G] float32 view of a buffer whose rows are padded to a multiple of
    4 floats: every row starts 16-byte aligned, so the distance epilogue
    stores whole 16-byte vectors and the rank kernels stream 16-byte loads."""
    ld = (G + 3) // 4 * 4
    return torch.empty((Q, ld), dtype=torch.float32, device=device)[:, :G]


def compute_dist(q, g, metric='euclidean', out=None, tile=0, math=None, q_planes=None,
                 symmetric=None, pad_rows=False):
    """[Q,D] x [G,D] -> [Q,G] distance matrix (reid_dataset_evaluator.py:244).
    math: 'h2' / 'x3' / 'f32' (None = dist_math(), or the GalleryIndex's own).
    g may be a GalleryIndex (then the GEMM runs on its prepared split).
    h2: queries split by split_h2_tiled, pps_distmat_h2_tiled (tile = h2 tile
    id, 0 = default); D % 32 != 0 runs x3.
    q_planes (x3): also split the queries into bf16x3 planes first so the
    pipelined GEMM stages both operands by DMA (pps_distmat_x3p; pipelined
    tiles only).  Same bits either way; measured at the Market shape it is
    not faster (scripts/probes/dist_probe.py: the split in the K loop is hidden),
    so None = off.
    pad_rows: return a [Q, G] view of a buffer with 16-byte-aligned rows
    (dist_buffer) instead of a dense matrix.
    symmetric (h2, x3): a self-distance (q and g the same rows, e.g.
    compute_dist(g, g) of re-ranking) computed from the upper-triangle tiles
    and mirrored (pps_distmat_h2_self_tiled / pps_distmat_x3_self, half the
    work); None = whenever q IS g's data, D % 32 == 0 and (x3) the tile is a
    square one (SELF_TILES)."""
    if isinstance(g, GalleryIndex):
        # the index fixes the arithmetic; an explicit request for another one
        # is an error (f32 reads the index's features as they are)
        if math not in (None, 'f32', g.math):
            raise RuntimeError("compute_dist: math=%r but the GalleryIndex holds a %r split"
                               % (math, g.math))
        math = math or g.math
    math = math or dist_math()
    if q.dim() != 2 or len(g.shape) != 2 or q.shape[1] != g.shape[1]:
        raise RuntimeError('compute_dist expects [m1,n] and [m2,n], got %s %s'
                           % (tuple(q.shape), tuple(g.shape)))
    Q, D = q.shape
    G = g.shape[0]
    if out is None:
        out = dist_buffer(Q, G, q.device) if pad_rows else \
            torch.empty((Q, G), dtype=torch.float32, device=q.device)
    if tuple(out.shape) != (Q, G):
        raise RuntimeError('out must be [%d, %d], got %s' % (Q, G, tuple(out.shape)))
    # the mark re_ranking reads: set on every return, so a reused buffer
    # never carries a stale True from an earlier self-distance
    out._pps_symmetric = False
    if math == 'f32':
        gf = g.feats if isinstance(g, GalleryIndex) else g
        call('pps_distmat', _dev(q, 'q'), Q, D, _dev(gf, 'g'), G, D, D, METRICS[metric],
             _dev_rows(out, 'out'), _ld(out), int(tile), _stream())
        return out
    f = g.feats if isinstance(g, GalleryIndex) else g
    same = (f.data_ptr() == q.data_ptr() and tuple(f.shape) == tuple(q.shape) and
            f.stride() == q.stride() and q.is_contiguous() and D % 32 == 0)
    if math == 'h2' and D % 32 == 0 and q.is_contiguous():
        if symmetric is None:
            symmetric = same
        if symmetric:
            x2, xrs, xsq = g.h2 if isinstance(g, GalleryIndex) and g.h2 is not None else \
                split_h2_tiled(q)
            call('pps_distmat_h2_self_tiled', _dev(x2, 'x2t', torch.int16), Q, _dev(xsq, 'xsq'),
                 _dev(xrs, 'xrs'), D, METRICS[metric], _dev_rows(out, 'out'), _ld(out),
                 int(tile), _stream())
            out._pps_symmetric = True   # mirrored tiles: exactly symmetric
            return out
        # a strided raw gallery (e.g. big[:, :D]) is made contiguous first: the
        # f16x2 index needs whole rows
        idx = g if isinstance(g, GalleryIndex) and g.h2 is not None else \
            GalleryIndex(f if f.is_contiguous() else f.contiguous(), math='h2')
        q2, qrs, qsq = split_h2_tiled(q)
        return distmat_h2(q2, qrs, qsq, idx, out, metric, tile, Q=Q)
    if math == 'h2':
        math, tile = 'x3', 0   # D % 32 != 0 (or strided queries): the bf16x3 kernels
    tiled = bool(q_planes) and D % 32 == 0 and (tile == 0 or tile >= TILE_P_FIRST)
    if symmetric is None:
        symmetric = same and tile in SELF_TILES
    if symmetric:
        # one read of x -> chunk-tiled planes + norms; both operands staged
        # from that copy by DMA (pps_distmat_x3_self_tiled)
        if isinstance(g, GalleryIndex) and g._tiled is not None:
            x3t, xsq = g._tiled, g.sqnorm
        else:
            x3t, xsq = split_sqnorm_tiled(q)
        call('pps_distmat_x3_self_tiled', _dev(x3t, 'x3t', torch.int16), Q, _dev(xsq, 'xsq'),
             D, METRICS[metric], _dev_rows(out, 'out'), _ld(out), int(tile), _stream())
        out._pps_symmetric = True   # mirrored tiles: exactly symmetric (re_ranking uses it)
        return out
    idx = g if isinstance(g, GalleryIndex) else GalleryIndex(g, tiled=tiled, math='x3')
    if q_planes:
        if tiled and q.is_contiguous():  # both operands chunk-tiled, queries in one pass
            qt, qsq = split_sqnorm_tiled(q)
            return distmat_planes(None, qsq, idx, out, metric, tile, q_tiled=qt, Q=Q, D=D)
        q3, qsq = split_sqnorm(q) if q.is_contiguous() else (split_bf16x3(q), row_sqnorm(q))
        return distmat_planes(q3, qsq, idx, out, metric, tile)
    qsq = row_sqnorm(q)
    call('pps_distmat_x3', _dev(q, 'q'), Q, D, _dev(qsq, 'qsq'),
         _dev(idx.planes, 'g3', torch.int16), _dev(idx.sqnorm, 'gsq'), G, D, D,
         METRICS[metric], _dev_rows(out, 'out'), _ld(out), int(tile), _stream())
    return out


def distmat_h2(q2, qrs, qsq, idx, out, metric='euclidean', tile=0, Q=None):
    """The h2 distance GEMM alone on queries already split (split_h2_tiled)
    against an h2 GalleryIndex: what compute_dist(math='h2') launches after
    the split (pps_distmat_h2_tiled)."""
    Q = qsq.shape[0] if Q is None else Q
    G, D = idx.shape
    g2, grs, gsq = idx.h2
    call('pps_distmat_h2_tiled', _dev(q2, 'q2t', torch.int16), Q, _dev(qsq, 'qsq'),
         _dev(qrs, 'qrs'), _dev(g2, 'g2t', torch.int16), _dev(gsq, 'gsq'), _dev(grs, 'grs'), G,
         D, METRICS[metric], _dev_rows(out, 'out'), _ld(out), int(tile), _stream())
    return out


def tile_planes(planes):
    """bf16x3 planes [3, R, D] (D % 32 == 0) -> the chunk-tiled layout
    [3][R16 / 16][D / 32][16][32] (R16 = R rounded up to 16, zero rows),
    returned as an int16 [3, R16, D] tensor: a 16-row DMA piece of one
    32-wide K chunk is then one contiguous KiB (pps_tile_planes)."""
    _, R, D = planes.shape
    r16 = (R + 15) // 16 * 16
    out = torch.empty((3, r16, D), dtype=torch.int16, device=planes.device)
    call('pps_tile_planes', _dev(planes, 'planes', torch.int16), R, D, D, R * D,
         _dev(out, 'out', torch.int16), _stream())
    return out


def _tiled_tile(tile):
    """The tile a tiled-plane distance GEMM runs: pipelined ids 29-53 as
    given; ids 54+ (which a distance matrix runs as tile 38) -> 0 (tile 43,
    the same 16x16x32 rounding group)."""
    return int(tile) if TILE_P_FIRST <= tile < 54 else 0


def distmat_planes(q3, qsq, idx, out, metric='euclidean', tile=0, q_tiled=None, Q=None,
                   D=None):
    """The distance GEMM alone on queries already split into bf16x3 planes
    q3 [3, Q, D] with squared norms qsq, against a GalleryIndex: what
    compute_dist(q_planes=True) launches after the split.  With D % 32 == 0
    both operands go chunk-tiled (pps_distmat_x3p_tiled: same bits, Market
    1.98 -> 1.83 ms on tile 52, scripts/probes/dist_tiled_probe.py); q_tiled
    = tile_planes(q3) when the caller has it already (q3 may then be None,
    with Q and D given)."""
    if q3 is not None:
        _, Q, D = q3.shape
    G = idx.shape[0]
    if D % 32 == 0 and (tile == 0 or tile >= TILE_P_FIRST):
        qt = q_tiled if q_tiled is not None else tile_planes(q3)
        call('pps_distmat_x3p_tiled', _dev(qt, 'q3t', torch.int16), Q, _dev(qsq, 'qsq'),
             _dev(idx.tiled_planes, 'g3t', torch.int16), _dev(idx.sqnorm, 'gsq'), G, D,
             METRICS[metric], _dev_rows(out, 'out'), _ld(out), _tiled_tile(tile), _stream())
        return out
    call('pps_distmat_x3p', _dev(q3, 'q3', torch.int16), Q, D, _dev(qsq, 'qsq'),
         _dev(idx.planes, 'g3', torch.int16), _dev(idx.sqnorm, 'gsq'), G, D, D,
         METRICS[metric], _dev_rows(out, 'out'), _ld(out), int(tile), _stream())
    return out


def pairwise_distance(X):
    """Caffe2 PairWiseDistance: squared L2, [N,D] -> [N,N]."""
    if X.dim() != 2:
        raise RuntimeError('[enforce fail] X.dim() == 2 (got %d)' % X.dim())
    N, D = X.shape
    Z = torch.empty((N, N), dtype=torch.float32, device=X.device)
    call('pps_pairwise_distance', _dev(X, 'X'), N, D, _dev(Z, 'Z'), _stream())
    return Z


def argsort_rows(dist, with_values=False):
    """Every row's columns in stable (distance, index) order -> idx [Q, G]
    int32 (and the sorted distances): np.argsort(dist, axis=1,
    kind='stable') -- the reference's full rank list
    (reid_dataset_evaluator.py:319,420).  G <= pps_argsort_rows_cap()."""
    Q, G = dist.shape
    idx = torch.empty((Q, G), dtype=torch.int32, device=dist.device)
    vals = torch.empty((Q, G), dtype=torch.float32, device=dist.device) if with_values else None
    call('pps_argsort_rows', _dev_rows(dist, 'dist'), Q, G, _ld(dist), idx.data_ptr(), G,
         vals.data_ptr() if vals is not None else None, G, _stream())
    return (idx, vals) if with_values else idx


def sgs_groups(order, gid, gcam, qid, qcam, U, separate_camera_set):
    """Steps 1-3 of CMC single_gallery_shot (pps_sgs_keys, pps_argsort_rows,
    pps_sgs_groups) from the stable rank list `order` [Q, G] and dense
    identities (device int32).  Returns (perm, gstart, glen, nids, qt)."""
    Q, G = order.shape
    dev = order.device
    keys = torch.empty((Q, G), dtype=torch.float32, device=dev)
    call('pps_sgs_keys', _dev_rows(order, 'order', torch.int32), Q, G, _ld(order),
         _dev(gid, 'gid', torch.int32), _dev(gcam, 'gcam', torch.int32),
         _dev(qid, 'qid', torch.int32), _dev(qcam, 'qcam', torch.int32),
         1 if separate_camera_set else 0, U, keys.data_ptr(), _stream())
    perm, skeys = argsort_rows(keys, with_values=True)
    del keys
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    gstart, glen, nids, qt = i32(Q, U), i32(Q, U), i32(Q), i32(Q)
    call('pps_sgs_groups', skeys.data_ptr(), perm.data_ptr(), Q, G, U, _dev(qid, 'qid', torch.int32),
         gstart.data_ptr(), glen.data_ptr(), nids.data_ptr(), qt.data_ptr(), _stream())
    return perm, gstart, glen, nids, qt


def sgs_ranks(perm, gstart, glen, nids, qt, rows, draws):
    """Step 5 of CMC single_gallery_shot (pps_sgs_ranks): draws [nr, repeat,
    ldd] int32 for the query rows `rows` [nr] -> k [nr, repeat] int32."""
    Q, G = perm.shape
    U = gstart.shape[1]
    nr, repeat, ldd = draws.shape
    k = torch.empty((nr, repeat), dtype=torch.int32, device=perm.device)
    call('pps_sgs_ranks', perm.data_ptr(), Q, G, _dev(rows, 'rows', torch.int32), nr,
         gstart.data_ptr(), glen.data_ptr(), nids.data_ptr(), qt.data_ptr(), U, repeat,
         _dev(draws, 'draws', torch.int32), ldd, k.data_ptr(), _stream())
    return k


def topk(dist, k):
    """Stable ascending top-k per row -> (vals [Q,k] f32, idx [Q,k] i32)."""
    Q, G = dist.shape
    vals = torch.empty((Q, k), dtype=torch.float32, device=dist.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dist.device)
    call('pps_topk', _dev_rows(dist, 'dist'), Q, G, _ld(dist), k, vals.data_ptr(),
         idx.data_ptr(), _stream())
    return vals, idx


def topk_merge(vals, idx, offsets, k):
    """Merge R per-shard stable top-k lists vals/idx [R, Q, k_in] (local
    indices; list r starts at global index offsets[r]) into the global stable
    top-k [Q, k] (pps_topk_merge; (+inf, -1) past the available entries)."""
    R, Q, kin = vals.shape
    offs = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    if offs.shape[0] != R:
        raise RuntimeError('need one offset per list: %d lists, %d offsets'
                           % (R, offs.shape[0]))
    out_v = torch.empty((Q, k), dtype=torch.float32, device=vals.device)
    out_i = torch.empty((Q, k), dtype=torch.int32, device=vals.device)
    call('pps_topk_merge', _dev(vals, 'vals'), _dev(idx, 'idx', torch.int32), R, Q, kin,
         offs.ctypes.data_as(_lib.ctypes.c_void_p), k, out_v.data_ptr(), out_i.data_ptr(),
         _stream())
    return out_v, out_i


def search_max_k():
    """Largest k of the fused search kernel (pps_search_max_k)."""
    return int(_lib.lib().pps_search_max_k())


def search_num_tiles():
    return int(_lib.lib().pps_search_h2_num_tiles())


def search_workspace_bytes(Q, G, k, segments=0):
    """Bytes of device workspace one fused search of Q queries against a G-row
    index needs (pps_search_h2_workspace_bytes; host arithmetic only,
    non-decreasing in G)."""
    n = int(_lib.lib().pps_search_h2_workspace_bytes(int(Q), int(G), int(k), int(segments)))
    if n < 0:
        raise RuntimeError('search_workspace_bytes: bad arguments Q=%r G=%r k=%r segments=%r '
                           '(1 <= k <= %d)' % (Q, G, k, segments, search_max_k()))
    return n


def _search_workspace(fn, workspace, need, device):
    """The workspace tensor of a fused search: a new one of `need` bytes
    (search_workspace_bytes), or the caller's if it holds that much."""
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=device)
    if (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or
            not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise RuntimeError('%s: workspace must be a contiguous device tensor of at least '
                           '%d bytes (search_workspace_bytes)' % (fn, need))
    return workspace


def _pad_list(vals, idx, k):
    """[Q, kin] lists -> [Q, k], the tail (+inf, -1) (pps_topk_merge's pad)."""
    Q, kin = vals.shape
    if kin == k:
        return vals, idx
    pv = torch.full((Q, k), float('inf'), dtype=torch.float32, device=vals.device)
    pi = torch.full((Q, k), -1, dtype=torch.int32, device=vals.device)
    pv[:, :kin] = vals
    pi[:, :kin] = idx
    return pv, pi


def exclusion_groups(qid, qcam, gid, gcam, by='id_cam', device='cuda'):
    """(q_group [Q], g_group [G]) int32 tensors on `device` for the exclusion
    rule of search / topk_excluding: dense non-negative codes (np.unique over
    the query + gallery keys taken together, host numpy) such that q_group[i] ==
    g_group[j] iff the keys are equal.  by='id_cam': key = (id, cam), the
    reference's junk rule (reid_dataset_evaluator.py:327-331, :427);
    by='cam': key = cam, the separate_camera_set rule (:332-333), which
    contains the junk rule."""
    qid, qcam, gid, gcam = (np.asarray(a).astype(np.int64).reshape(-1)
                            for a in (qid, qcam, gid, gcam))
    if len(qid) != len(qcam) or len(gid) != len(gcam):
        raise RuntimeError('exclusion_groups: one id and one cam per row')
    nq = len(qid)
    dense = lambda a: np.asarray(np.unique(a, return_inverse=True)[1]).reshape(-1).astype(np.int64)
    if by == 'id_cam':
        # the pair as one key: dense id code x dense cam code (1-D sorts only)
        ids, cams = dense(np.concatenate([qid, gid])), dense(np.concatenate([qcam, gcam]))
        codes = dense(ids * (int(cams.max()) + 1 if len(cams) else 1) + cams)
    elif by == 'cam':
        codes = dense(np.concatenate([qcam, gcam]))
    else:
        raise RuntimeError("exclusion_groups: by must be 'id_cam' or 'cam', got %r" % (by,))
    codes = np.ascontiguousarray(codes.astype(np.int32))
    return (torch.from_numpy(codes[:nq].copy()).to(device),
            torch.from_numpy(codes[nq:].copy()).to(device))


def _check_groups(fn, q_group, g_group, Q, G, device):
    """The (q_group, g_group) pair of an excluding call, or (None, None)."""
    if q_group is None and g_group is None:
        return None, None
    if q_group is None or g_group is None:
        raise RuntimeError('%s: q_group and g_group go together (both or neither)' % fn)
    out = []
    for name, t, n in (('q_group', q_group, Q), ('g_group', g_group, G)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError('%s: %s must be a torch.Tensor' % (fn, name))
        if t.dtype != torch.int32:
            raise RuntimeError('%s: %s must be int32, got %s' % (fn, name, t.dtype))
        if t.dim() != 1 or t.shape[0] != n:
            raise RuntimeError('%s: %s must have shape (%d,), got %s'
                               % (fn, name, n, tuple(t.shape)))
        if t.device != device:
            raise RuntimeError('%s: %s is on %s, the search runs on %s'
                               % (fn, name, t.device, device))
        out.append(t if t.is_contiguous() else t.contiguous())
    return out[0], out[1]


def topk_excluding(dist, k, q_group, g_group):
    """The materialised twin of search(..., q_group, g_group): the stable
    (distance, index) top-k per row of `dist` [Q, G] over the columns c with
    not (q_group[r] >= 0 and g_group[c] == q_group[r]) -> (vals [Q, k] f32,
    idx [Q, k] i32), (+inf, -1) past their number.  pps_topk over a masked
    COPY of the matrix (excluded cells +inf; `dist` is left as it is), the
    entries that landed on an excluded cell turned into pads.  Holds a second
    [Q, G] matrix and a [Q, G] byte mask while it runs."""
    if not isinstance(dist, torch.Tensor) or dist.dim() != 2:
        raise RuntimeError('topk_excluding: dist must be a 2-D torch.Tensor')
    Q, G = dist.shape
    k = int(k)
    if k < 1:
        raise RuntimeError('topk_excluding: k must be >= 1')
    q_group, g_group = _check_groups('topk_excluding', q_group, g_group, Q, G, dist.device)
    if q_group is None:
        raise RuntimeError('topk_excluding: q_group and g_group are required')
    kin = min(k, G)
    if kin == 0 or Q == 0:
        return _pad_list(torch.empty((Q, 0), dtype=torch.float32, device=dist.device),
                         torch.empty((Q, 0), dtype=torch.int32, device=dist.device), k)
    mask = (g_group[None, :] == q_group[:, None]) & (q_group[:, None] >= 0)
    masked = dist_buffer(Q, G, dist.device)
    masked.copy_(dist)
    masked.masked_fill_(mask, float('inf'))
    vals, idx = topk(masked, kin)
    del masked
    hit = mask.gather(1, idx.long())
    vals.masked_fill_(hit, float('inf'))
    idx.masked_fill_(hit, -1)
    return _pad_list(vals, idx, k)


def _search_one(q, q_split, index, k, metric, segments, tile, workspace, q_group=None,
                g_group=None):
    """One index: the fused kernel when it applies, else the matrix."""
    Q, D = q.shape
    G = index.shape[0]
    fused = (index.h2 is not None and q_split is not None and 1 <= k <= search_max_k())
    if not fused or (q_group is not None and G == 0):
        kin = min(k, G)
        if kin == 0 or Q == 0:
            return _pad_list(torch.empty((Q, 0), dtype=torch.float32, device=q.device),
                             torch.empty((Q, 0), dtype=torch.int32, device=q.device), k)
        qc = q if q.is_contiguous() else q.contiguous()   # compute_dist takes whole rows
        dist = compute_dist(qc, index, metric=metric, pad_rows=True)
        if q_group is not None:
            return topk_excluding(dist, k, q_group, g_group)
        vals, idx = topk(dist, kin)
        return _pad_list(vals, idx, k)
    workspace = _search_workspace('search', workspace,
                                  search_workspace_bytes(Q, G, k, segments), q.device)
    vals = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    args = _h2_operands('search', q_split, index) + (
        METRICS[metric], int(k), int(segments), int(tile), workspace.data_ptr(),
        workspace.numel() * workspace.element_size(), vals.data_ptr(), idx.data_ptr())
    if q_group is None:
        call('pps_search_h2_tiled', *(args + (_stream(),)))
    else:
        call('pps_search_h2_tiled_excl', *(args + (_dev(q_group, 'q_group', torch.int32),
                                                   _dev(g_group, 'g_group', torch.int32),
                                                   _stream())))
    return vals, idx


def search(q, gallery, k, metric='euclidean', segments=0, tile=0, workspace=None,
           q_group=None, g_group=None):
    """The k nearest gallery rows of every query -> (vals [Q, k] float32,
    idx [Q, k] int32), ascending, ties by gallery index, (+inf, -1) past G
    entries: exactly topk(compute_dist(q, gallery, math='h2'), k), from a
    fused distance + top-k kernel (pps_search_h2_tiled) that never writes the
    [Q, G] matrix.

    gallery: a [G, D] tensor (indexed on the fly), a GalleryIndex, or a
    sequence of GalleryIndex objects holding consecutive row segments of one
    logical gallery (GalleryIndex.split: a gallery beyond one index's 2 GiB of
    planes).  Each segment is searched on its own and the lists are merged
    (topk_merge, in rounds when there are many); indices are global.
    segments: gallery segments searched by independent workgroups (0 = auto);
    tile: 0 .. search_num_tiles() - 1, same bits.  workspace: a device buffer
    of search_workspace_bytes(Q, G, k, segments) bytes (G = the largest
    segment) to reuse across calls; None allocates one.  All launches go on
    the current stream.  Measured (DESIGN.md "Fused search"), it is slower than
    the materialised path -- 1.25x at the Market shape, 1.04x at a 10,000 x
    125,000 shard -- and peaks at 0.4 GB where that path holds a 5 GB matrix.

    Falls back to compute_dist + topk -- which DOES materialise the [Q, G]
    matrix -- when the fused kernel does not apply: an index holding an x3
    split (also one the constructor downgraded from a requested 'h2'),
    D % 32 != 0, non-contiguous queries (copied to whole rows first), or
    k > search_max_k() (up to pps_topk's 1024).

    q_group [Q] / g_group [G] (int32 tensors on the queries' device, both or
    neither; g_group covers the whole logical gallery, each segment of a
    sequence gets its slice): gallery row c is excluded for query r iff
    q_group[r] >= 0 and g_group[c] == q_group[r] (exclusion_groups builds the
    reference's junk and separate-camera rules; arange on both sides is
    "exclude myself").  The rule runs inside the kernel's filter
    (pps_search_h2_tiled_excl), so the rows are the stable top-k of the
    non-excluded gallery rows, (+inf, -1) past their number -- exactly
    topk_excluding(compute_dist(q, gallery, math='h2'), k, q_group, g_group)
    (in a self-search, the matrix of compute_dist(..., symmetric=False): the
    mirrored self-distance kernel copies its upper triangle, other bits than
    the general kernel's below the diagonal).
    The fallback cases above then run compute_dist + topk_excluding, which
    materialises the matrix, a masked copy of it and a byte mask."""
    parts = _gallery_parts('search', q, gallery)
    k = int(k)
    if k < 1:
        raise RuntimeError('search: k must be >= 1')
    D = q.shape[1]
    starts = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    q_group, g_group = _check_groups('search', q_group, g_group, q.shape[0], int(starts[-1]),
                                     q.device)
    if q.shape[0] == 0:
        return (torch.empty((0, k), dtype=torch.float32, device=q.device),
                torch.empty((0, k), dtype=torch.int32, device=q.device))
    q_split = None
    if (D % 32 == 0 and q.is_contiguous() and k <= search_max_k() and
            any(p.h2 is not None for p in parts)):
        q_split = split_h2_tiled(q)   # once, as compute_dist splits them
    lists = [_search_one(q, q_split, p, k, metric, segments, tile, workspace, q_group,
                         None if g_group is None else g_group[int(a):int(a) + p.shape[0]])
             for p, a in zip(parts, starts[:-1])]
    if len(lists) == 1:
        return lists[0]
    offsets = starts[:-1]
    if offsets[-1] + parts[-1].shape[0] >= 2 ** 31:
        raise RuntimeError('search: gallery indices must fit int32')
    # merge rounds: each call takes at most R lists with R * k <= 8192, R <= 64;
    # a merged list carries global indices (offset 0) into the next round
    rmax = max(2, min(64, 8192 // k))
    lists = [(v, i, int(o)) for (v, i), o in zip(lists, offsets)]
    while len(lists) > 1:
        nxt = []
        for a in range(0, len(lists), rmax):
            grp = lists[a:a + rmax]
            if len(grp) == 1:
                nxt.append(grp[0])
                continue
            v, i = topk_merge(torch.stack([g[0] for g in grp]), torch.stack([g[1] for g in grp]),
                              [g[2] for g in grp], k)
            nxt.append((v, i, 0))
        lists = nxt
    v, i, o = lists[0]
    return v, i


class MatchIndex(object):
    """Per-identity index of a gallery (shard) for one query set, built once
    from the ids (host metadata, O(G log G)): members = local gallery indices
    sorted by (id, index); query q's identity occupies
    members[q_beg[q]:q_end[q]].  `capacity` = the most same-id entries any
    query has = an exact bound for its positive and junk lists."""

    def __init__(self, qid, qcam, gid, gcam, device='cuda'):
        qid, qcam = np.asarray(qid).astype(np.int64), np.asarray(qcam)
        gid, gcam = np.asarray(gid).astype(np.int64), np.asarray(gcam)
        order = np.lexsort((np.arange(len(gid)), gid))
        sid = gid[order]
        beg = np.searchsorted(sid, qid, 'left')
        end = np.searchsorted(sid, qid, 'right')
        self.capacity = max(1, int((end - beg).max()) if len(qid) else 1)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(device)
        self.members, self.q_beg, self.q_end = i32(order), i32(beg), i32(end)
        self.qcam, self.gcam = i32(qcam), i32(gcam)
        self.Q, self.G = len(qid), len(gid)


def collect_matches(dist, index, g_offset=0, pmax=None):
    """(pos_d, pos_idx, pos_cnt, junk_d, junk_idx, junk_cnt) of every query
    from the MatchIndex (pps_collect_matches)."""
    Q, G = dist.shape
    if (Q, G) != (index.Q, index.G):
        raise RuntimeError('distance matrix %s does not match the index (%d, %d)'
                           % (tuple(dist.shape), index.Q, index.G))
    pmax = pmax or index.capacity
    jmax = index.capacity
    dev = dist.device
    pos_d = torch.empty((Q, pmax), dtype=torch.float32, device=dev)
    pos_idx = torch.empty((Q, pmax), dtype=torch.int32, device=dev)
    pos_cnt = torch.empty((Q,), dtype=torch.int32, device=dev)
    junk_d = torch.empty((Q, jmax), dtype=torch.float32, device=dev)
    junk_idx = torch.empty((Q, jmax), dtype=torch.int32, device=dev)
    junk_cnt = torch.empty((Q,), dtype=torch.int32, device=dev)
    call('pps_collect_matches', _dev_rows(dist, 'dist'), Q, G, _ld(dist),
         _dev(index.qcam, 'qcam', torch.int32), _dev(index.gcam, 'gcam', torch.int32),
         _dev(index.members, 'members', torch.int32), _dev(index.q_beg, 'q_beg', torch.int32),
         _dev(index.q_end, 'q_end', torch.int32), int(g_offset), pmax, pos_d.data_ptr(),
         pos_idx.data_ptr(), pos_cnt.data_ptr(), jmax, junk_d.data_ptr(), junk_idx.data_ptr(),
         junk_cnt.data_ptr(), _stream())
    return pos_d, pos_idx, pos_cnt, (junk_d, junk_idx, junk_cnt)


class SortedPositives(object):
    """Merged, sorted positive lists of a query set (pps_rank_prepare):
    sorted_d / sorted_idx [Q, Ptot], pos_total [Q], bin-lookup cells."""

    def __init__(self, sorted_d, sorted_idx, pos_total, cells):
        self.sorted_d, self.sorted_idx, self.pos_total = sorted_d, sorted_idx, pos_total
        self.cells = cells

    def __iter__(self):   # (sorted_d, sorted_idx, pos_total), as the old triple
        return iter((self.sorted_d, self.sorted_idx, self.pos_total))


def rank_prepare(pos_d, pos_idx, pos_cnt):
    """Merge [R, Q, Pmax] positive lists, sorted -> SortedPositives
    (pps_rank_prepare)."""
    R, Q, Pmax = pos_d.shape
    dev = pos_d.device
    sd = torch.empty((Q, R * Pmax), dtype=torch.float32, device=dev)
    si = torch.empty((Q, R * Pmax), dtype=torch.int32, device=dev)
    tot = torch.empty((Q,), dtype=torch.int32, device=dev)
    cells = torch.empty((Q, _lib.lib().pps_rank_cells()), dtype=torch.int32, device=dev)
    call('pps_rank_prepare', R, Q, Pmax, _dev(pos_d, 'pos_d'), _dev(pos_idx, 'pos_idx',
                                                                   torch.int32),
         _dev(pos_cnt, 'pos_cnt', torch.int32), sd.data_ptr(), si.data_ptr(), tot.data_ptr(),
         cells.data_ptr(), _stream())
    return SortedPositives(sd, si, tot, cells)


def rank_count_stream(dist, g_offset, sp, junk, hist=None, before=None):
    """Additive (hist, before) counts of this shard's rows against the
    SortedPositives sp (pps_rank_count_stream); hist/before accumulate when
    given."""
    Q, G = dist.shape
    sorted_d, sorted_idx, pos_total = sp.sorted_d, sp.sorted_idx, sp.pos_total
    Ptot = sorted_d.shape[1]
    junk_d, junk_idx, junk_cnt = junk
    dev = dist.device
    if hist is None:
        hist = torch.zeros((Q, Ptot), dtype=torch.int32, device=dev)
    if before is None:
        before = torch.zeros((Q,), dtype=torch.int32, device=dev)
    call('pps_rank_count_stream', _dev_rows(dist, 'dist'), Q, G, _ld(dist), int(g_offset),
         Ptot, _dev(sorted_d, 'sorted_d'), _dev(sorted_idx, 'sorted_idx', torch.int32),
         _dev(pos_total, 'pos_total', torch.int32), _dev(sp.cells, 'cells', torch.int32),
         junk_d.shape[1], _dev(junk_d, 'junk_d'),
         _dev(junk_idx, 'junk_idx', torch.int32), _dev(junk_cnt, 'junk_cnt', torch.int32),
         _dev(hist, 'hist', torch.int32), _dev(before, 'before', torch.int32), _stream())
    return hist, before


def cmc_counts(dist, g_offset, sp, junk, index=None, separate_camera_set=False, hist=None):
    """Per-positive exact-rank bins for the reference's general cmc
    (pps_cmc_counts); with separate_camera_set the MatchIndex's qcam / gcam
    drop every same-camera entry.  hist accumulates when given."""
    Q, G = dist.shape
    Ptot = sp.sorted_d.shape[1]
    junk_d, junk_idx, junk_cnt = junk
    if hist is None:
        hist = torch.zeros((Q, Ptot), dtype=torch.int32, device=dist.device)
    qc = gc = 0
    if separate_camera_set:
        qc = _dev(index.qcam, 'qcam', torch.int32)
        gc = _dev(index.gcam, 'gcam', torch.int32)
    call('pps_cmc_counts', _dev_rows(dist, 'dist'), Q, G, _ld(dist), int(g_offset), Ptot,
         _dev(sp.sorted_d, 'sorted_d'), _dev(sp.sorted_idx, 'sorted_idx', torch.int32),
         _dev(sp.pos_total, 'pos_total', torch.int32), qc, gc, junk_d.shape[1],
         _dev(junk_d, 'junk_d'), _dev(junk_idx, 'junk_idx', torch.int32),
         _dev(junk_cnt, 'junk_cnt', torch.int32), _dev(hist, 'hist', torch.int32), _stream())
    return hist


def cmc_finalize(pos_total, hist, topk, first_match_break):
    """(ret [Q, topk] float64 after the reference's cumsum, valid [Q] int32)."""
    Q, Ptot = hist.shape
    ret = torch.empty((Q, topk), dtype=torch.float64, device=hist.device)
    valid = torch.empty((Q,), dtype=torch.int32, device=hist.device)
    call('pps_cmc_finalize', Q, Ptot, _dev(pos_total, 'pos_total', torch.int32),
         _dev(hist, 'hist', torch.int32), int(topk), int(bool(first_match_break)),
         ret.data_ptr(), valid.data_ptr(), _stream())
    return ret, valid


def ap_finalize(sorted_d, pos_total, hist, before):
    Q, Ptot = sorted_d.shape
    dev = sorted_d.device
    ap = torch.empty((Q,), dtype=torch.float64, device=dev)
    valid = torch.empty((Q,), dtype=torch.int32, device=dev)
    first = torch.empty((Q,), dtype=torch.int32, device=dev)
    call('pps_ap_finalize', Q, Ptot, _dev(sorted_d, 'sorted_d'),
         _dev(pos_total, 'pos_total', torch.int32), _dev(hist, 'hist', torch.int32),
         _dev(before, 'before', torch.int32), ap.data_ptr(), valid.data_ptr(),
         first.data_ptr(), _stream())
    return ap, valid, first


def rank_count_h2_max_p():
    """Longest merged positive list (sorted_d's width) the fused count kernel
    takes (pps_rank_count_h2_max_p)."""
    return int(_lib.lib().pps_rank_count_h2_max_p())


def rank_count_h2_workspace_bytes(Q, G, Ptot, segments=0):
    """Bytes of device workspace one rank_count_h2 call needs
    (pps_rank_count_h2_workspace_bytes; host arithmetic only, non-decreasing in
    G).  0 today: the kernel's counts leave it as atomics."""
    n = int(_lib.lib().pps_rank_count_h2_workspace_bytes(int(Q), int(G), int(Ptot),
                                                         int(segments)))
    if n < 0:
        raise RuntimeError('rank_count_h2_workspace_bytes: bad arguments Q=%r G=%r Ptot=%r '
                           'segments=%r (1 <= Ptot <= %d)'
                           % (Q, G, Ptot, segments, rank_count_h2_max_p()))
    return n


def _h2_split_args(split, name):
    """(planes, norms, scales) of a split_h2_tiled triple as the entry points
    take them."""
    x2, xrs, xsq = split
    return (_dev(x2, name + '2t', torch.int16), _dev(xsq, name + 'sq'), _dev(xrs, name + 'rs'))


def _h2_operands(fn, q_split, index):
    """The nine leading arguments of the fused h2 entry points (queries' and
    gallery's planes, norms, scales, shapes)."""
    if not isinstance(index, GalleryIndex) or index.h2 is None:
        raise RuntimeError('%s: the gallery must be a GalleryIndex holding an h2 split' % fn)
    q2, qsq = q_split[0], q_split[2]
    Q, G, D = qsq.shape[0], index.shape[0], index.shape[1]
    if q2.dim() != 3 or q2.shape[2] != D or q2.shape[1] != (Q + 15) // 16 * 16:
        raise RuntimeError('%s: q_split %s does not fit %d queries of width %d'
                           % (fn, tuple(q2.shape), Q, D))
    q = _h2_split_args(q_split, 'q')
    return (q[0], Q) + q[1:] + _h2_split_args(index.h2, 'g') + (G, D)


def _workspace_arg(fn, workspace):
    """(pointer, bytes) of the optional workspace of the fused count entries."""
    if workspace is None:
        return 0, 0
    if (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or
            not workspace.is_contiguous()):
        raise RuntimeError('%s: workspace must be a contiguous device tensor' % fn)
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def collect_matches_h2(q_split, index, match_index, metric='euclidean', g_offset=0, pmax=None):
    """collect_matches without the matrix (pps_collect_matches_h2): q_split =
    split_h2_tiled(queries), index an h2 GalleryIndex, match_index the
    MatchIndex of the same queries and gallery rows.  The same tuple, each
    distance with the bits compute_dist(q, index, math='h2') holds at that
    cell."""
    args = _h2_operands('collect_matches_h2', q_split, index)
    Q, G = args[1], args[7]
    if (Q, G) != (match_index.Q, match_index.G):
        raise RuntimeError('operands (%d, %d) do not match the index (%d, %d)'
                           % (Q, G, match_index.Q, match_index.G))
    pmax = pmax or match_index.capacity
    jmax = match_index.capacity
    dev = q_split[0].device
    pos_d = torch.empty((Q, pmax), dtype=torch.float32, device=dev)
    pos_idx = torch.empty((Q, pmax), dtype=torch.int32, device=dev)
    pos_cnt = torch.empty((Q,), dtype=torch.int32, device=dev)
    junk_d = torch.empty((Q, jmax), dtype=torch.float32, device=dev)
    junk_idx = torch.empty((Q, jmax), dtype=torch.int32, device=dev)
    junk_cnt = torch.empty((Q,), dtype=torch.int32, device=dev)
    mi = match_index
    call('pps_collect_matches_h2', *(args + (
        METRICS[metric], _dev(mi.qcam, 'qcam', torch.int32), _dev(mi.gcam, 'gcam', torch.int32),
        _dev(mi.members, 'members', torch.int32), _dev(mi.q_beg, 'q_beg', torch.int32),
        _dev(mi.q_end, 'q_end', torch.int32), int(g_offset), pmax, pos_d.data_ptr(),
        pos_idx.data_ptr(), pos_cnt.data_ptr(), jmax, junk_d.data_ptr(), junk_idx.data_ptr(),
        junk_cnt.data_ptr(), _stream())))
    return pos_d, pos_idx, pos_cnt, (junk_d, junk_idx, junk_cnt)


def rank_count_h2(q_split, index, g_offset, sp, junk, metric='euclidean', hist=None,
                  before=None, segments=0, tile=0, workspace=None):
    """rank_count_stream without the matrix (pps_rank_count_h2_tiled): the
    additive (hist, before) counts of this gallery (shard, segment) against
    the SortedPositives sp, distances computed on the fly from q_split and the
    h2 GalleryIndex; junk = this gallery's junk lists from collect_matches_h2.
    hist / before accumulate when given.  sp's width must not exceed
    rank_count_h2_max_p().  segments / tile: as in search (same counts)."""
    args = _h2_operands('rank_count_h2', q_split, index)
    Q, G = args[1], args[7]
    Ptot = sp.sorted_d.shape[1]
    junk_d, junk_idx, junk_cnt = junk
    dev = q_split[0].device
    if hist is None:
        hist = torch.zeros((Q, Ptot), dtype=torch.int32, device=dev)
    if before is None:
        before = torch.zeros((Q,), dtype=torch.int32, device=dev)
    if tuple(hist.shape) != (Q, Ptot) or tuple(before.shape) != (Q,):
        raise RuntimeError('rank_count_h2: hist must be [%d, %d] and before [%d]' % (Q, Ptot, Q))
    ws_ptr, ws_bytes = _workspace_arg('rank_count_h2', workspace)
    call('pps_rank_count_h2_tiled', *(args + (
        METRICS[metric], int(g_offset), Ptot, _dev(sp.sorted_d, 'sorted_d'),
        _dev(sp.sorted_idx, 'sorted_idx', torch.int32),
        _dev(sp.pos_total, 'pos_total', torch.int32), junk_d.shape[1], _dev(junk_d, 'junk_d'),
        _dev(junk_idx, 'junk_idx', torch.int32), _dev(junk_cnt, 'junk_cnt', torch.int32),
        int(segments), int(tile), ws_ptr, ws_bytes, _dev(hist, 'hist', torch.int32),
        _dev(before, 'before', torch.int32), _stream())))
    return hist, before


def cmc_counts_h2(q_split, index, g_offset, sp, junk, match_index=None,
                  separate_camera_set=False, metric='euclidean', hist=None, segments=0, tile=0,
                  workspace=None):
    """cmc_counts without the matrix (pps_cmc_count_h2_tiled): the additive
    per-positive key bins of this gallery (shard, segment) against the
    SortedPositives sp, distances computed on the fly from q_split and the h2
    GalleryIndex -- the counts cmc_counts gives on compute_dist(q, index,
    math='h2'), exactly.  junk = this gallery's junk lists from
    collect_matches_h2; with separate_camera_set the MatchIndex's qcam / gcam
    drop every same-camera column instead and junk is not read (None is
    accepted).  hist accumulates when given.  sp's width must not exceed
    rank_count_h2_max_p().  segments / tile: as in search (same counts)."""
    args = _h2_operands('cmc_counts_h2', q_split, index)
    Q, G = args[1], args[7]
    Ptot = sp.sorted_d.shape[1]
    if hist is None:
        hist = torch.zeros((Q, Ptot), dtype=torch.int32, device=q_split[0].device)
    if tuple(hist.shape) != (Q, Ptot):
        raise RuntimeError('cmc_counts_h2: hist must be [%d, %d]' % (Q, Ptot))
    qc = gc = jmax = jd = ji = jc = 0
    if separate_camera_set:
        if match_index is None or (Q, G) != (match_index.Q, match_index.G):
            raise RuntimeError('cmc_counts_h2: separate_camera_set needs the MatchIndex of '
                               'the %d queries and %d gallery rows' % (Q, G))
        qc = _dev(match_index.qcam, 'qcam', torch.int32)
        gc = _dev(match_index.gcam, 'gcam', torch.int32)
    else:
        junk_d, junk_idx, junk_cnt = junk
        jmax = junk_d.shape[1]
        jd, ji = _dev(junk_d, 'junk_d'), _dev(junk_idx, 'junk_idx', torch.int32)
        jc = _dev(junk_cnt, 'junk_cnt', torch.int32)
    ws_ptr, ws_bytes = _workspace_arg('cmc_counts_h2', workspace)
    call('pps_cmc_count_h2_tiled', *(args + (
        METRICS[metric], int(g_offset), Ptot, _dev(sp.sorted_d, 'sorted_d'),
        _dev(sp.sorted_idx, 'sorted_idx', torch.int32),
        _dev(sp.pos_total, 'pos_total', torch.int32), qc, gc, jmax, jd, ji, jc,
        int(segments), int(tile), ws_ptr, ws_bytes, _dev(hist, 'hist', torch.int32),
        _stream())))
    return hist


def _gallery_parts(fn, q, gallery):
    """gallery as search takes it -> the list of GalleryIndex segments."""
    if isinstance(gallery, GalleryIndex):
        parts = [gallery]
    elif isinstance(gallery, torch.Tensor):
        g = gallery
        h2ok = g.dim() == 2 and g.shape[1] % 32 == 0
        parts = [GalleryIndex(g if g.is_contiguous() or not h2ok else g.contiguous(),
                              math='h2' if h2ok else None)]
    else:
        parts = list(gallery)
        if not parts or not all(isinstance(p, GalleryIndex) for p in parts):
            raise RuntimeError('%s: gallery must be a tensor, a GalleryIndex or a '
                               'non-empty sequence of GalleryIndex' % fn)
    if q.dim() != 2 or any(p.shape[1] != q.shape[1] for p in parts):
        raise RuntimeError('%s expects [Q, D] queries and [G, D] galleries' % fn)
    return parts


RANK_FUSED_MAX_SEGMENTS = 64   # pps_rank_prepare merges at most 64 lists per query


def rank_eval_fused(q, gallery, qid, qcam, gid, gcam, metric='euclidean', segments=0, tile=0,
                    match_index=None):
    """Per-query (ap float64, valid int32, first_rank int32) -- what
    reid_dataset_evaluator.rank_eval returns on compute_dist(q, gallery,
    math='h2'), bit for bit -- without the [Q, G] matrix: the true matches'
    distances from pps_collect_matches_h2, pps_rank_prepare, the counts from
    the fused distance + count kernel pps_rank_count_h2_tiled, pps_ap_finalize.
    mAP = ap[valid].mean(); first_rank gives the first-match (Market) CMC.

    gallery: what search takes -- a [G, D] tensor (indexed on the fly), a
    GalleryIndex, or a sequence of GalleryIndex objects holding consecutive row
    segments of one logical gallery (GalleryIndex.split).  qid / qcam [Q] and
    gid / gcam [G] are host metadata of the whole logical gallery.  The queries
    are split once.  For a sequence, every segment gets its own MatchIndex and
    one collect with the segment's start as g_offset; pps_rank_prepare merges
    the stacked lists in one call -- more than 64 segments is an error, not
    merged in rounds -- and the merged lists are trimmed to the longest true
    list the ids allow (max_positives); then one count per segment adds into
    the same hist / before.  segments / tile: the count kernel's, as in search.
    match_index: the segments' MatchIndex objects (one, or a sequence in segment
    order) built earlier from the same ids, as rank_eval's `index`; None builds
    them (host, O(G log G)).

    A segment falls back to the materialised path -- compute_dist, then
    collect_matches / rank_count_stream on ITS [Q, rows] block, which is built
    for the collect and again for the count when there are several segments
    (one block lives at a time) -- when the fused kernels do not apply: an
    index holding an x3 split, D % 32 != 0, non-contiguous queries (copied to
    whole rows), or, for the count only, merged lists wider than
    rank_count_h2_max_p().

    Measured against compute_dist + rank_eval it is
    the slower path: 2.5 against 1.1 ms at the Market shape, 32.6 against 15.8
    ms at a 10,000 x 125,000 shard (1.9 / 30.9 ms on clustered features), the
    count kernel alone twice the plain distance GEMM.  The gain is memory -- a
    0.19 GB peak where that path holds the 5.1 GB block -- and a path for a
    gallery split over several indexes, which one compute_dist call cannot
    take."""
    st = _fused_lists('rank_eval_fused', q, gallery, qid, qcam, gid, gcam, metric, match_index)
    dev = q.device
    if st is None:
        return (torch.empty((0,), dtype=torch.float64, device=dev),
                torch.empty((0,), dtype=torch.int32, device=dev),
                torch.empty((0,), dtype=torch.int32, device=dev))
    sp = st.sp
    hist = torch.zeros(tuple(sp.sorted_d.shape), dtype=torch.int32, device=dev)
    before = torch.zeros((q.shape[0],), dtype=torch.int32, device=dev)
    for p, a, mi, junk, fused in st.segments():
        if fused:
            rank_count_h2(st.q_split, p, a, sp, junk, metric, hist, before, segments, tile)
        else:
            dist = st.block(p)
            rank_count_stream(dist, a, sp, junk, hist, before)
            del dist
    return ap_finalize(sp.sorted_d, sp.pos_total, hist, before)


class _FusedLists(object):
    """What _fused_lists leaves for the counts: the gallery segments with their
    start rows, MatchIndex objects and junk lists, the queries' split, the
    merged SortedPositives."""

    def __init__(self, parts, starts, mis, junks, fusable, q_split, sp, block, kept):
        self.parts, self.starts, self.mis, self.junks = parts, starts, mis, junks
        self.fusable, self.q_split, self.sp = fusable, q_split, sp
        self._block, self._kept = block, kept
        self.fits = sp.sorted_d.shape[1] <= rank_count_h2_max_p()

    def segments(self):
        """(segment, its start row, its MatchIndex, its junk lists, whether the
        fused count applies) per gallery segment."""
        for p, a, mi, junk, f in zip(self.parts, self.starts[:-1], self.mis, self.junks,
                                     self.fusable):
            yield p, int(a), mi, junk, f and self.fits

    def block(self, p):
        """The segment's [Q, rows] block (a lone segment's, built for the
        collect, is reused)."""
        return self._kept if self._kept is not None else self._block(p)


def _fused_lists(fn, q, gallery, qid, qcam, gid, gcam, metric, match_index):
    """The front half rank_eval_fused and cmc_eval_fused share: the gallery as
    segments, one MatchIndex and one collect per segment, one rank_prepare over
    the stacked lists, the trim to max_positives.  None when Q == 0."""
    parts = _gallery_parts(fn, q, gallery)
    if len(parts) > RANK_FUSED_MAX_SEGMENTS:
        raise RuntimeError('%s: %d gallery segments, pps_rank_prepare merges at '
                           'most %d lists per query' % (fn, len(parts), RANK_FUSED_MAX_SEGMENTS))
    qid, qcam, gid, gcam = (np.asarray(a).reshape(-1) for a in (qid, qcam, gid, gcam))
    Q, D = q.shape
    starts = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    if len(qid) != Q or len(qcam) != Q or len(gid) != starts[-1] or len(gcam) != starts[-1]:
        raise RuntimeError('%s: %d queries / %d gallery rows, ids and cams of '
                           '%d / %d / %d / %d' % (fn, Q, starts[-1], len(qid), len(qcam),
                                                  len(gid), len(gcam)))
    if starts[-1] >= 2 ** 31:
        raise RuntimeError('%s: gallery indices must fit int32' % fn)
    dev = q.device
    if Q == 0:
        return None
    q_split = None
    if D % 32 == 0 and q.is_contiguous() and any(p.h2 is not None for p in parts):
        q_split = split_h2_tiled(q)   # once, as compute_dist splits them
    qc = q if q.is_contiguous() else q.contiguous()   # compute_dist takes whole rows
    fusable = [q_split is not None and p.h2 is not None for p in parts]
    block = lambda p: compute_dist(qc, p, metric=metric, pad_rows=True)
    keep = len(parts) == 1   # a lone segment's block serves the collect and the count
    if match_index is None:
        mis = [MatchIndex(qid, qcam, gid[int(a):int(b)], gcam[int(a):int(b)], dev)
               for a, b in zip(starts[:-1], starts[1:])]
    else:
        mis = [match_index] if isinstance(match_index, MatchIndex) else list(match_index)
        if [(m.Q, m.G) for m in mis] != [(Q, p.shape[0]) for p in parts]:
            raise RuntimeError('%s: match_index does not fit the queries and '
                               'the gallery segments' % fn)
    pmax = max(mi.capacity for mi in mis)
    lists, junks, kept = [], [], None
    for p, mi, a, f in zip(parts, mis, starts[:-1], fusable):
        if f:
            pd, pi, pc, junk = collect_matches_h2(q_split, p, mi, metric, int(a), pmax)
        else:
            dist = block(p)
            pd, pi, pc, junk = collect_matches(dist, mi, int(a), pmax)
            kept = dist if keep else None
            del dist
        lists.append((pd, pi, pc))
        junks.append(junk)
    sp = rank_prepare(*(torch.stack([l[i] for l in lists]) for i in range(3)))
    del lists
    # one list is as wide as the identity's rows; R stacked ones are R times that
    ptrue = max(1, max_positives(qid, qcam, gid, gcam)) if len(parts) > 1 else pmax
    if ptrue < sp.sorted_d.shape[1]:   # the tail is padding for every query
        sp = SortedPositives(sp.sorted_d[:, :ptrue].contiguous(),
                             sp.sorted_idx[:, :ptrue].contiguous(), sp.pos_total, sp.cells)
    return _FusedLists(parts, starts, mis, junks, fusable, q_split, sp, block, kept)


def cmc_eval_fused(q, gallery, qid, qcam, gid, gcam, topk=100, separate_camera_set=False,
                   first_match_break=False, metric='euclidean', segments=0, tile=0,
                   match_index=None):
    """(ret [Q, topk] float64, valid [Q] int32): the per-query CMC rows of the
    reference's cmc (fractional or first-match, with or without
    separate_camera_set; not single_gallery_shot) -- what cmc_finalize returns
    for cmc_counts on compute_dist(q, gallery, math='h2'), bit for bit --
    without the [Q, G] matrix.  rank_eval_fused's front half (the gallery as
    tensor / GalleryIndex / sequence of segments, one MatchIndex and one
    collect per segment, one rank_prepare, the trim to max_positives), then one
    keyed count per segment (pps_cmc_count_h2_tiled) into one hist and
    pps_cmc_finalize.  Arguments and fallbacks are rank_eval_fused's: a segment
    holding an x3 split, D % 32 != 0, non-contiguous queries or merged lists
    wider than rank_count_h2_max_p() take compute_dist + collect_matches /
    cmc_counts on that segment's block and give the materialised answer."""
    st = _fused_lists('cmc_eval_fused', q, gallery, qid, qcam, gid, gcam, metric, match_index)
    dev = q.device
    if st is None:
        return (torch.empty((0, int(topk)), dtype=torch.float64, device=dev),
                torch.empty((0,), dtype=torch.int32, device=dev))
    sp = st.sp
    hist = torch.zeros(tuple(sp.sorted_d.shape), dtype=torch.int32, device=dev)
    for p, a, mi, junk, fused in st.segments():
        if fused:
            cmc_counts_h2(st.q_split, p, a, sp, junk, mi, separate_camera_set, metric, hist,
                          segments, tile)
        else:
            dist = st.block(p)
            cmc_counts(dist, a, sp, junk, mi, separate_camera_set, hist)
            del dist
    return cmc_finalize(sp.pos_total, hist, topk, first_match_break)


def re_ranking(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3, symmetric=None, whole=False):
    """k-reciprocal re-ranking (reid_dataset_evaluator.py:442-519) -> [Q, G].
    symmetric: q_q and g_g are exactly symmetric (PPS_RERANK_SYMMETRIC: with
    16-byte rows and N >= 16384 the N x N normalised distance is never built,
    pps_re_ranking_ld; else it is built from rows, only q_g^T transposed);
    None = both came from compute_dist's mirrored self-distance (tagged
    `_pps_symmetric`).  Same result either way on symmetric inputs.  Inputs
    may be row-padded views (dist_buffer / compute_dist(pad_rows=True)).
    whole: the three are the blocks of one symmetric [N, N] self-distance
    (self_distance_blocks) -- q_g^T is read in place (PPS_RERANK_WHOLE)."""
    Q, G = q_g.shape
    assert tuple(q_q.shape) == (Q, Q) and tuple(g_g.shape) == (G, G)
    if symmetric is None:
        symmetric = bool(getattr(q_q, '_pps_symmetric', False) and
                         getattr(g_g, '_pps_symmetric', False))
    flags = (RERANK_SYMMETRIC if symmetric else 0) | (RERANK_WHOLE if whole else 0)
    blocks = (_dev_rows(q_g, 'q_g'), _ld(q_g), _dev_rows(q_q, 'q_q'), _ld(q_q),
              _dev_rows(g_g, 'g_g'), _ld(g_g))
    # the size of the path this call takes (in place: no N x N region)
    nbytes = _lib.lib().pps_rerank_workspace_bytes_ld(*blocks, Q, G, k1, k2, flags)
    if nbytes < 0:
        raise RuntimeError('bad re-ranking arguments')
    ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=q_g.device)
    out = torch.empty((Q, G), dtype=torch.float32, device=q_g.device)
    call('pps_re_ranking_ld', *blocks, Q, G, k1, k2, float(lambda_value), flags,
         ws.data_ptr(), int(nbytes), out.data_ptr(), _stream())
    return out


RERANK_SYMMETRIC = 1   # pps_abi.h PPS_RERANK_SYMMETRIC
RERANK_WHOLE = 2       # pps_abi.h PPS_RERANK_WHOLE


def self_distance_blocks(x, Q, metric='euclidean'):
    """Re-ranking's three distance blocks from ONE mirrored self-distance of
    x = [queries; gallery] ([N, D], the first Q rows the queries): -> (M,
    q_g, q_q, g_g), the blocks row-padded views of the exactly symmetric
    [N, N] M (compute_dist(x, x), upper triangle + mirror, one bf16x3 split of
    x).  Pass them to re_ranking(..., whole=True); q_g serves the plain
    ranking as well.  Same values as the three separate compute_dist calls
    on the same tile group."""
    M = compute_dist(x, x, metric=metric, pad_rows=True, symmetric=True)
    return M, M[:Q, Q:], M[:Q, :Q], M[Q:, Q:]


def search_rowmax(q, index, k, metric='euclidean', segments=0, tile=0, workspace=None):
    """search against one h2 GalleryIndex that also returns every query's
    largest squared distance: -> (vals [Q, k], idx [Q, k], rowmax [Q]) with
    vals / idx exactly search's and rowmax the bits of (W * W).amax(1), W =
    compute_dist(q, index, math='h2', symmetric=False) -- over the G real
    columns (pps_search_h2_tiled_rowmax; the matrix is never written).  There
    is no fallback: q must be contiguous with D % 32 == 0 and k <=
    search_max_k()."""
    if not isinstance(index, GalleryIndex) or index.h2 is None:
        raise RuntimeError('search_rowmax: the gallery must be a GalleryIndex holding an h2 split')
    if q.dim() != 2 or q.shape[1] != index.shape[1]:
        raise RuntimeError('search_rowmax expects [Q, D] queries and a [G, D] gallery')
    Q, D = q.shape
    G = index.shape[0]
    k = int(k)
    if D % 32 != 0 or not q.is_contiguous() or not 1 <= k <= search_max_k():
        raise RuntimeError('search_rowmax: needs contiguous queries, D %% 32 == 0 and '
                           '1 <= k <= %d' % search_max_k())
    q_split = split_h2_tiled(q)   # held to the launch: args are its tensors' addresses
    args = _h2_operands('search_rowmax', q_split, index)
    workspace = _search_workspace('search_rowmax', workspace,
                                  search_workspace_bytes(Q, G, k, segments), q.device)
    vals = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    rowmax = torch.empty((Q,), dtype=torch.float32, device=q.device)
    call('pps_search_h2_tiled_rowmax', *(args + (
        METRICS[metric], k, int(segments), int(tile), workspace.data_ptr(),
        workspace.numel() * workspace.element_size(), vals.data_ptr(), idx.data_ptr(),
        rowmax.data_ptr(), _stream())))
    return vals, idx, rowmax


def pair_dist(q, index, lists, counts=None, metric='euclidean'):
    """Distances of listed pairs without the matrix (pps_pair_dist_h2):
    out[r, t] = the distance of query r to gallery row lists[r, t] for t <
    min(counts[r], cap), with the bits compute_dist(q, index, math='h2',
    symmetric=False) holds at that cell; cells past a row's count are 0.
    lists [Q, cap] int32, counts [Q] int32 or None (every entry).  q: the
    [Q, D] queries, or their split_h2_tiled triple.
    index may be a pair (index0, index1) of h2 GalleryIndex that are never
    concatenated (pps_pair_dist_h2_parts): a list index < G0 names that row of
    index0, any other index row (index - G0) of index1; the bits are the same
    kernel's at that cell."""
    q_split = q if isinstance(q, tuple) else split_h2_tiled(q)
    parts = isinstance(index, (tuple, list))
    if parts:
        if len(index) != 2:
            raise RuntimeError('pair_dist: a two-part gallery is (index0, index1)')
        args = _h2_operands('pair_dist', q_split, index[0])
        args1 = _h2_operands('pair_dist', q_split, index[1])
        args = args[:8] + args1[4:]   # ..., B0, b1 planes / norms / scales, B1, D
    else:
        args = _h2_operands('pair_dist', q_split, index)
    Q = args[1]
    if lists.dim() != 2 or lists.shape[0] != Q or lists.shape[1] < 1:
        raise RuntimeError('pair_dist: lists must be [%d, cap >= 1]' % Q)
    cap = lists.shape[1]
    if counts is not None and tuple(counts.shape) != (Q,):
        raise RuntimeError('pair_dist: counts must be [%d]' % Q)
    out = torch.zeros((Q, cap), dtype=torch.float32, device=lists.device)
    call('pps_pair_dist_h2_parts' if parts else 'pps_pair_dist_h2', *(args + (
        METRICS[metric], _dev(lists, 'lists', torch.int32),
        0 if counts is None else _dev(counts, 'counts', torch.int32), cap, out.data_ptr(),
        _stream())))
    return out


def rerank_rows_workspace_bytes(Q, G, k1=20, k2=6, features=False, segments=0):
    """Bytes of workspace of re_ranking_rows (features=False) or
    re_ranking_from_features (host arithmetic, non-decreasing in G): per-row
    structures only, about 27 KB a row at (20, 6), plus the fused search's
    workspace on the features path."""
    L = _lib.lib()
    n = int(L.pps_rerank_features_workspace_bytes(int(Q), int(G), int(k1), int(k2), int(segments))
            if features else L.pps_rerank_rows_workspace_bytes(int(Q), int(G), int(k1), int(k2)))
    if n < 0:
        raise RuntimeError('rerank_rows_workspace_bytes: bad arguments Q=%r G=%r k1=%r k2=%r '
                           'segments=%r' % (Q, G, k1, k2, segments))
    return n


def re_ranking_rows(W, Q, k1=20, k2=6, lambda_value=0.3, g_window=0):
    """Row-form k-reciprocal re-ranking from a materialised [N, N] matrix W of
    x = [queries; gallery] (the first Q rows the queries) -> [Q, G]: the twin
    of re_ranking_from_features (pps_re_ranking_rows).  Row i's
    neighbours are its stable (W[i, j], j) top-(k1 + 1), OD(i, j) =
    W[i, j]^2 / max_j W[i, j]^2; W need not be symmetric (the general h2
    kernel's, compute_dist(x, GalleryIndex(x), symmetric=False), is not).
    g_window: gallery rows per Jaccard workgroup (0 = auto; same bits)."""
    _dev_rows(W, 'W')
    N = W.shape[0]
    if W.shape[1] != N or not 0 < Q < N:
        raise RuntimeError('re_ranking_rows: W must be [N, N] with 0 < Q < N, got %s, Q=%r'
                           % (tuple(W.shape), Q))
    G = N - Q
    nbytes = rerank_rows_workspace_bytes(Q, G, k1, k2)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=W.device)
    out = torch.empty((Q, G), dtype=torch.float32, device=W.device)
    call('pps_re_ranking_rows', W.data_ptr(), _ld(W), Q, G, int(k1), int(k2),
         float(lambda_value), int(g_window), ws.data_ptr(), nbytes, out.data_ptr(), _stream())
    return out


def re_ranking_from_features(x, Q, k1=20, k2=6, lambda_value=0.3, metric='euclidean', segments=0,
                             tile=0, g_window=0):
    """k-reciprocal re-ranking straight from the features x = [queries;
    gallery] ([N, D], the first Q rows the queries) -> [Q, G], without any
    [N, N] buffer and for any gallery size (pps_re_ranking_features; DESIGN
    6.1.4): ranks and row maxima from the fused search of x against itself,
    the weights' distances from the pair kernel, the q x g block computed into
    the result and blended in place.  Bit for bit re_ranking_rows on W =
    compute_dist(x, GalleryIndex(x), symmetric=False).  Holds the planes of x,
    a second copy of the gallery's planes and per-row structures (about 27 KB
    a row at k1 = 20, k2 = 6).  One h2 index only (x's planes under 2 GiB).
    Raises -- it never builds an [N, N] matrix silently -- when x is strided,
    D % 32 != 0 or the distance arithmetic is not h2: use re_ranking_rows on a
    matrix of your own then.  For several query batches against one gallery,
    RerankGallery gives the same bits without repeating the gallery's part."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise RuntimeError('re_ranking_from_features: x must be a [N, D] tensor')
    N, D = x.shape
    if not x.is_contiguous() or D % 32 != 0 or dist_math() != 'h2':
        raise RuntimeError('re_ranking_from_features: needs contiguous features, D %% 32 == 0 '
                           'and h2 distance arithmetic (got stride %s, D=%d, math %r); '
                           're_ranking_rows takes a materialised matrix instead'
                           % (x.stride(), D, dist_math()))
    if not 0 < Q < N:
        raise RuntimeError('re_ranking_from_features: need 0 < Q < N, got Q=%r N=%d' % (Q, N))
    G = N - Q
    x_split, g_split = split_h2_tiled(x), split_h2_tiled(x[Q:])
    nbytes = rerank_rows_workspace_bytes(Q, G, k1, k2, features=True, segments=segments)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    out = torch.empty((Q, G), dtype=torch.float32, device=x.device)
    operands = _h2_split_args(x_split, 'x') + _h2_split_args(g_split, 'g')
    call('pps_re_ranking_features', *(operands + (
        Q, G, D, METRICS[metric], int(k1), int(k2), float(lambda_value), int(segments), int(tile),
        int(g_window), ws.data_ptr(), nbytes, out.data_ptr(), _stream())))
    return out


def rerank_prepared_workspace_bytes(Q, G, k1=20, k2=6, segments=0):
    """Bytes of workspace of one RerankGallery.re_rank call (host arithmetic,
    non-decreasing in Q and in G): re_ranking_rows' per-row structures, the
    merge input and one region the three searches share."""
    n = int(_lib.lib().pps_rerank_prepared_workspace_bytes(int(Q), int(G), int(k1), int(k2),
                                                           int(segments)))
    if n < 0:
        raise RuntimeError('rerank_prepared_workspace_bytes: bad arguments Q=%r G=%r k1=%r k2=%r '
                           'segments=%r' % (Q, G, k1, k2, segments))
    return n


class RerankGallery(object):
    """A gallery prepared once for k-reciprocal re-ranking from the features
    (DESIGN 6.1.6): re_rank(q) gives, bit for bit,
    re_ranking_from_features(cat([q, gallery]), Q) for any number of query
    batches, without repeating the gallery-against-gallery search and without
    the planes of the concatenation.  gallery: a contiguous [G, D] tensor or an
    h2 GalleryIndex.  Holds .index (the GalleryIndex), .k1, .metric and, from
    one search_rowmax of the gallery against itself, .nn_vals / .nn_idx
    ([G, k1 + 1], gallery numbering) and .rowmax ([G]); re_rank only reads
    them.  Raises where re_ranking_from_features raises (strided features,
    D % 32 != 0, distance arithmetic not h2): no matrix is built silently."""

    def __init__(self, gallery, k1=20, metric='euclidean', segments=0, tile=0):
        if isinstance(gallery, GalleryIndex):
            index, ok = gallery, gallery.h2 is not None
        else:
            if not isinstance(gallery, torch.Tensor) or gallery.dim() != 2:
                raise RuntimeError('RerankGallery: gallery must be a [G, D] tensor or a '
                                   'GalleryIndex')
            ok = gallery.is_contiguous() and gallery.shape[1] % 32 == 0
            index = None
        if not ok or dist_math() != 'h2':
            raise RuntimeError('RerankGallery: needs contiguous features, D %% 32 == 0 and h2 '
                               'distance arithmetic (math %r); re_ranking_rows takes a '
                               'materialised matrix instead' % dist_math())
        k1 = int(k1)
        if not 1 <= k1 <= min(63, search_max_k() - 1):
            raise RuntimeError('RerankGallery: k1 + 1 must be <= 64 and <= %d' % search_max_k())
        self.index = index if index is not None else GalleryIndex(gallery, math='h2')
        self.k1, self.metric = k1, metric
        self.nn_vals, self.nn_idx, self.rowmax = search_rowmax(
            self.index.feats, self.index, k1 + 1, metric=metric, segments=segments, tile=tile)

    def re_rank(self, q, k1=None, k2=6, lambda_value=0.3, segments=0, tile=0, g_window=0):
        """[Q, D] queries -> the re-ranked [Q, G] (pps_re_ranking_prepared).
        k1 None = the prepared value; a smaller one reads a prefix of the
        prepared lists, a larger one raises."""
        k1 = self.k1 if k1 is None else int(k1)
        if k1 > self.k1:
            raise RuntimeError('RerankGallery.re_rank: k1=%d above the prepared k1=%d'
                               % (k1, self.k1))
        G, D = self.index.shape
        if (not isinstance(q, torch.Tensor) or q.dim() != 2 or q.shape[1] != D or
                not q.is_contiguous() or q.shape[0] < 1):
            raise RuntimeError('RerankGallery.re_rank: needs contiguous [Q >= 1, %d] queries; '
                               're_ranking_rows takes a materialised matrix instead' % D)
        Q = q.shape[0]
        q_split = split_h2_tiled(q)   # held to the launch
        nbytes = rerank_prepared_workspace_bytes(Q, G, k1, k2, segments)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        out = torch.empty((Q, G), dtype=torch.float32, device=q.device)
        operands = _h2_split_args(q_split, 'q') + _h2_split_args(self.index.h2, 'g')
        call('pps_re_ranking_prepared', *(operands + (
            Q, G, D, METRICS[self.metric], _dev(self.nn_vals, 'nn_vals'),
            _dev(self.nn_idx, 'nn_idx', torch.int32), self.nn_vals.shape[1],
            _dev(self.rowmax, 'g_rowmax'), k1, int(k2), float(lambda_value), int(segments),
            int(tile), int(g_window), ws.data_ptr(), nbytes, out.data_ptr(), _stream())))
        return out


def max_positives(qid, qcam, gid, gcam):
    """Host-side bound on true matches per query (metadata only, exact)."""
    qid = np.asarray(qid, np.int64)
    qcam = np.asarray(qcam, np.int64)
    gid = np.asarray(gid, np.int64)
    gcam = np.asarray(gcam, np.int64)
    if len(qid) == 0 or len(gid) == 0:
        return 0
    ids, inv = np.unique(np.concatenate([qid, gid]), return_inverse=True)
    qi, gi = inv[:len(qid)], inv[len(qid):]
    per_id = np.bincount(gi, minlength=len(ids))
    cams = np.unique(np.concatenate([qcam, gcam]), return_inverse=True)[1]
    qc, gc = cams[:len(qcam)], cams[len(qcam):]
    ncam = int(cams.max()) + 1
    per_idcam = np.bincount(gi * ncam + gc, minlength=len(ids) * ncam)
    cnt = per_id[qi] - per_idcam[qi * ncam + qc]
    return int(cnt.max())


# ---------------------------------------------------------------------------
# Feature extractor
# ---------------------------------------------------------------------------
def _weights(entry, w):
    """f32 weights -> the exact-f32 MFMA entry; int16 (bf16x3 planes from
    split_bf16x3) -> the `_x3` entry (f32 products on bf16 matrix cores)."""
    if isinstance(w, torch.Tensor) and w.dtype == torch.int16:
        return entry + '_x3', _dev(w, 'w', torch.int16)
    return entry, _dev(w, 'w')


def split_bf16x3(x, batched=False):
    """f32 x -> int16 bf16 planes hi, mid, lo with x = hi + mid + lo exactly
    (the weight format of the `_x3` GEMMs): shape (3,) + x.shape, or for
    batched=True (x.shape[0], 3) + x.shape[1:]."""
    nbatch = x.shape[0] if batched else 1
    n = x.numel() // nbatch
    shape = ((nbatch, 3) + tuple(x.shape[1:])) if batched else ((3,) + tuple(x.shape))
    out = torch.empty(shape, dtype=torch.int16, device=x.device)
    call('pps_split_bf16x3', _dev(x, 'x'), n, nbatch, _dev(out, 'out', torch.int16), _stream())
    return out


def conv2d_bn_act(x, cin, w, kpad, k, stride, pad, dil, scale, shift, residual, relu, y,
                  tile=0):
    N, H, W, ldx = x.shape
    _, Ho, Wo, Cout = y.shape
    rp = 0
    if residual is not None:
        if tuple(residual.shape) != tuple(y.shape):
            raise RuntimeError('residual shape %s != output %s'
                               % (tuple(residual.shape), tuple(y.shape)))
        rp = _dev(residual, 'residual')
    fn, wp = _weights('pps_conv2d_bn_act', w)
    call(fn, _dev(x, 'x'), N, H, W, cin, ldx, wp, Cout, kpad,
         k, k, stride, pad, dil, _dev(scale, 'scale'), _dev(shift, 'shift'), rp,
         int(bool(relu)), _dev(y, 'y'), Ho, Wo, Cout, int(tile), _stream())
    return y


def tile_shape(tile, planes=False):
    """(rows, cols) of the tile a pipelined GEMM id launches ((0, 0) if none)."""
    r, c = _lib.ctypes.c_int(0), _lib.ctypes.c_int(0)
    call('pps_x3p_tile_shape', int(tile), int(bool(planes)), _lib.ctypes.addressof(r),
         _lib.ctypes.addressof(c))
    return r.value, c.value


def conv2d_bn_act_pps(x, cin, w3, kpad, k, stride, pad, dil, scale, shift, residual, split,
                      max_ave, pps_out, y=None, tile=0):
    """The last res5 conv (+ BN + residual + ReLU) with the part pooling fused
    into its epilogue (pps_conv2d_bn_act_pps_x3p): pps_out [2^S-1, N, Cout]
    gets what part_power_set would compute from the conv output; y (NHWC, or
    None = not written) the conv output itself.  x: f32 NHWC or bf16x3
    planes (act_planes)."""
    xs = x.shape[1:] if _is_planes(x) else x.shape
    N, H, W, ldx = xs
    nsub, n2, Cout = pps_out.shape
    split = np.ascontiguousarray(split, dtype=np.int32)
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    if nsub != (1 << len(split)) - 1 or n2 != N:
        raise RuntimeError('pps_out must be [2^S - 1, N, Cout]')
    if tuple(residual.shape) != (N, Ho, Wo, Cout) or (y is not None and
                                                       tuple(y.shape) != (N, Ho, Wo, Cout)):
        raise RuntimeError('residual / y must be [N, Ho, Wo, Cout]')
    if _is_planes(x):
        xp, x3, xpl = 0, _dev(x, 'x planes', torch.int16), x[0].numel()
    else:
        xp, x3, xpl = _dev(x, 'x'), 0, 0
    call('pps_conv2d_bn_act_pps_x3p', xp, x3, xpl, N, H, W, cin, ldx,
         _dev(w3, 'w3', torch.int16), Cout, kpad, k, k, stride, pad, dil, _dev(scale, 'scale'),
         _dev(shift, 'shift'), _dev(residual, 'residual'), _dev(y, 'y') if y is not None else 0,
         Ho, Wo, split.ctypes.data_as(_lib.ctypes.c_void_p), len(split), int(bool(max_ave)),
         _dev(pps_out, 'pps_out'), int(tile), _stream())
    return pps_out


def act_planes(shape, device):
    """Buffer for a bf16x3 activation tensor: int16 [3, N, H, W, C] holding
    hi, mid, lo planes with x = hi + mid + lo exactly (split as the x3 GEMMs
    split f32 operands, so a consumer reading the planes gets the bits it
    would have computed from the f32 tensor)."""
    return torch.empty((3,) + tuple(shape), dtype=torch.int16, device=device)


def _is_planes(t):
    return isinstance(t, torch.Tensor) and t.dtype == torch.int16 and t.dim() == 5 \
        and t.shape[0] == 3


def conv2d_bn_act_x3p(x, cin, w3, kpad, k, stride, pad, dil, scale, shift, residual, relu,
                      y, tile=0, splitk=1, part=None, counters=None):
    """conv2d_bn_act on the pipelined bf16x3 GEMM where the input and/or the
    output are bf16x3 activation planes (act_planes) instead of f32 NHWC:
    x / y may each be either.  Same bits as the f32-activation call.
    splitk > 1: K slices with raw partials in `part`, summed in slice order by
    a second pass -- or, with `counters` (int32, zero, >= output tiles), by
    the last slice of each tile in the same launch (same bits)."""
    xs = x.shape[1:] if _is_planes(x) else x.shape
    ys = y.shape[1:] if _is_planes(y) else y.shape
    N, H, W, ldx = xs
    _, Ho, Wo, Cout = ys
    if not (isinstance(w3, torch.Tensor) and w3.dtype == torch.int16):
        raise RuntimeError('activation planes need bf16x3 weights (split_bf16x3)')
    rp = 0
    if residual is not None:
        if tuple(residual.shape) != tuple(ys):
            raise RuntimeError('residual shape %s != output %s'
                               % (tuple(residual.shape), tuple(ys)))
        rp = _dev(residual, 'residual')
    if _is_planes(x):
        xp, x3, xpl = 0, _dev(x, 'x planes', torch.int16), x[0].numel()
    else:
        xp, x3, xpl = _dev(x, 'x'), 0, 0
    if _is_planes(y):
        yp, y3, ypl = 0, _dev(y, 'y planes', torch.int16), y[0].numel()
    else:
        yp, y3, ypl = _dev(y, 'y'), 0, 0
    if splitk > 1:
        M = N * Ho * Wo
        if part is None or part.numel() < splitk * M * Cout:
            raise RuntimeError('split-K needs a partials buffer of >= %d floats'
                               % (splitk * M * Cout))
        if counters is not None:
            call('pps_conv2d_bn_act_x3p_splitk_fused', xp, x3, xpl, N, H, W, cin, ldx,
                 _dev(w3, 'w', torch.int16), Cout, kpad, k, k, stride, pad, dil,
                 _dev(scale, 'scale'), _dev(shift, 'shift'), rp, int(bool(relu)), yp, y3, ypl,
                 Ho, Wo, Cout, int(splitk), _dev(part, 'part'),
                 _dev(counters, 'counters', torch.int32), counters.numel(), int(tile),
                 _stream())
            return y
        call('pps_conv2d_bn_act_x3p_splitk', xp, x3, xpl, N, H, W, cin, ldx,
             _dev(w3, 'w', torch.int16), Cout, kpad, k, k, stride, pad, dil,
             _dev(scale, 'scale'), _dev(shift, 'shift'), rp, int(bool(relu)), yp, y3, ypl, Ho,
             Wo, Cout, int(splitk), _dev(part, 'part'), int(tile), _stream())
        return y
    call('pps_conv2d_bn_act_x3p', xp, x3, xpl, N, H, W, cin, ldx, _dev(w3, 'w', torch.int16),
         Cout, kpad, k, k, stride, pad, dil, _dev(scale, 'scale'), _dev(shift, 'shift'), rp,
         int(bool(relu)), yp, y3, ypl, Ho, Wo, Cout, int(tile), _stream())
    return y


def conv1x1_seam(x, w2c3, scale2c, shift2c, residual, trunk, w2a3, scale2a, shift2a, y):
    """branch2c of an identity bottleneck + branch2a of the next one in one
    launch (pps_conv1x1_seam_x3): trunk = relu(x . w2c * s + t + residual),
    y = relu(trunk . w2a * s + t); x [..., K1], trunk / residual [..., N1],
    y [..., N2] NHWC f32, (K1, N1, N2) = (64, 256, 64) or (128, 512, 128);
    w2c3 / w2a3 bf16x3 planes of the packed [Cout][Kpad] weights.  Same bits
    as the two convolutions on a 16x16x32-block tile."""
    K1, N1, N2 = x.shape[-1], trunk.shape[-1], y.shape[-1]
    M = x.numel() // K1
    if residual.shape != trunk.shape or y.numel() // N2 != M or trunk.numel() // N1 != M:
        raise RuntimeError('seam shapes: x %s, residual %s, trunk %s, y %s'
                           % (tuple(x.shape), tuple(residual.shape), tuple(trunk.shape),
                              tuple(y.shape)))
    call('pps_conv1x1_seam_x3', _dev(x, 'x'), M, K1, _dev(w2c3, 'w2c', torch.int16), N1,
         _dev(scale2c, 'scale2c'), _dev(shift2c, 'shift2c'), _dev(residual, 'residual'),
         _dev(trunk, 'trunk'), _dev(w2a3, 'w2a', torch.int16), N2, _dev(scale2a, 'scale2a'),
         _dev(shift2a, 'shift2a'), _dev(y, 'y'), _stream())
    return trunk, y


def conv2d_dual_bn_act(x, cin, k, stride, pad, x2, stride2, w, kpad1, shift, relu, y,
                       tile=0):
    """relu?(conv_k(x) + conv_1x1/stride2(x2) + shift), BN scales folded in w."""
    N, H, W, ldx = x.shape
    _, H2, W2, C2 = x2.shape
    _, Ho, Wo, Cout = y.shape
    fn, wp = _weights('pps_conv2d_dual_bn_act', w)
    call(fn, _dev(x, 'x'), N, H, W, cin, ldx, k, k, stride, pad,
         _dev(x2, 'x2'), H2, W2, C2, C2, stride2, wp, Cout, kpad1, C2,
         _dev(shift, 'shift'), int(bool(relu)), _dev(y, 'y'), Ho, Wo, Cout, int(tile),
         _stream())
    return y


# ---- f16x2 convolutions (include/pps_abi.h "f16x2 convolutions") ----------
def split_weights_h2(w_packed):
    """Packed [Cout, Kpad] f32 conv weights (Kpad % 32 == 0) -> (w2t, wrs):
    the two chunk-tiled f16 planes [2, Cout16, Kpad] (int16) and the
    per-output-channel inverse scales [Cout] the f16x2 conv entries take."""
    planes, rs, _ = split_h2_tiled(w_packed.contiguous())
    return planes, rs


AMAX_SLOT_FLOATS = 1024   # pps_abi.h PPS_AMAX_SLOT_FLOATS: 16 partial maxima, 64 apart


def amax_slot(device='cuda'):
    """A zeroed activation-max slot (the f16x2 entries' amax_x / amax_y)."""
    return torch.zeros((AMAX_SLOT_FLOATS,), dtype=torch.float32, device=device)


def amax_value(slot):
    """The tensor max a slot holds (max of its partial maxima)."""
    return float(slot[::64].max())


def amax(x, out=None):
    """max |x| into an activation-max slot (pps_amax; the slot is zeroed here)."""
    if out is None:
        out = amax_slot(x.device)
    else:
        _amax_arg(out, 'amax')
        out.zero_()
    call('pps_amax', _dev(x, 'x'), x.numel(), _dev(out, 'amax'), _stream())
    return out


def _amax_arg(a, name):
    if a is None:
        return 0
    if a.dtype != torch.float32 or a.numel() < AMAX_SLOT_FLOATS:
        raise RuntimeError('%s must be an activation-max slot of %d float32 (ops.amax_slot)'
                           % (name, AMAX_SLOT_FLOATS))
    return _dev(a, name)


def split_act_h2(x, amax_x, out=None):
    """f16x2 activation planes [2, *x.shape] (int16 storage) of f32 x with the
    scale of the slot amax_x (pps_split_f16x2_act): what the f16x2 kernels
    split after an f32 fragment read, done once per element."""
    n = x.numel()
    if out is None:
        out = torch.empty((2,) + tuple(x.shape), dtype=torch.int16, device=x.device)
    call('pps_split_f16x2_act', _dev(x, 'x'), n, _amax_arg(amax_x, 'amax_x'),
         _dev(out, 'planes', torch.int16), out[0].numel(), _stream())
    return out


def h2_out_bound(w_packed, scale, shift):
    """(bound_w, bound_b) of a conv whose output is written as f16x2 planes
    (pps_h2_out_bound on the packed f32 weights [Cout, Kpad], BN scale / shift):
    max|y| <= bound_w * max|x| + bound_b."""
    Cout, Kpad = w_packed.shape
    out = (_lib.ctypes.c_float * 2)()
    call('pps_h2_out_bound', _dev(w_packed.contiguous(), 'w'), Cout, Kpad,
         _dev(scale, 'scale') if scale is not None else 0, _dev(shift, 'shift'), out, _stream())
    return float(out[0]), float(out[1])


def conv2d_bn_act_h2out(x, cin, w, wrs, kpad, k, stride, pad, dil, scale, shift, y2, amax_x,
                        bound_in, bound, bound_out, tile=0):
    """Conv + BN + ReLU whose output y2 [2, N, Ho, Wo, Cout] (int16) is f16x2
    planes on the scale of the bound bound[0] * max|x| + bound[1] (max|x| from
    the slot bound_in, `bound` from h2_out_bound), the bound written to the slot
    bound_out (pps_conv2d_bn_act_h2out).  w: bf16x3 planes [3, Cout, Kpad] with
    wrs None, or split_weights_h2 output with its wrs (then x may be f16x2
    planes, and amax_x is the f16x2 input slot)."""
    planes = _h2_planes(x)
    N, H, W, ldx = x.shape[1:] if planes else x.shape
    _, _, Ho, Wo, Cout = y2.shape
    call('pps_conv2d_bn_act_h2out', 0 if planes else _dev(x, 'x'),
         _dev(x, 'x planes', torch.int16) if planes else 0, x.stride(0) if planes else 0,
         N, H, W, cin, ldx, _dev(w, 'w', torch.int16), _dev(wrs, 'wrs') if wrs is not None else 0,
         Cout, kpad, k, k, stride, pad, dil, _dev(scale, 'scale'), _dev(shift, 'shift'),
         _dev(y2, 'y2', torch.int16), y2.stride(0), Ho, Wo, Cout,
         _amax_arg(amax_x, 'amax_x') if amax_x is not None else 0,
         _amax_arg(bound_in, 'bound_in'), float(bound[0]), float(bound[1]),
         _amax_arg(bound_out, 'bound_out'), int(tile), _stream())
    return y2


def _h2_planes(x):
    """x is f16x2 activation planes [2, N, H, W, C] (split_act_h2)?"""
    return x.dtype == torch.int16 and x.dim() == 5 and x.shape[0] == 2


def conv2d_bn_act_h2(x, cin, w2, wrs, kpad, k, stride, pad, dil, scale, shift, residual, relu, y,
                     amax_x, amax_y=None, tile=0):
    """conv2d_bn_act in f16x2 arithmetic (pps_conv2d_bn_act_h2): w2 / wrs from
    split_weights_h2, amax_x = max|x| as a device float (amax() or the
    producer's amax_y), amax_y (optional, zeroed by the caller) receives
    max|y|.  x may be f16x2 activation planes (split_act_h2 with amax_x;
    pps_conv2d_bn_act_h2_planes, same bits)."""
    planes = _h2_planes(x)
    N, H, W, ldx = x.shape[1:] if planes else x.shape
    _, Ho, Wo, Cout = y.shape
    rp = 0
    if residual is not None:
        if tuple(residual.shape) != tuple(y.shape):
            raise RuntimeError('residual shape %s != output %s'
                               % (tuple(residual.shape), tuple(y.shape)))
        rp = _dev(residual, 'residual')
    rest = (N, H, W, cin, ldx, _dev(w2, 'w2t', torch.int16), _dev(wrs, 'wrs'), Cout, kpad, k, k,
            stride, pad, dil, _dev(scale, 'scale'), _dev(shift, 'shift'), rp, int(bool(relu)),
            _dev(y, 'y'), Ho, Wo, Cout, _amax_arg(amax_x, 'amax_x'), _amax_arg(amax_y, 'amax_y'),
            int(tile), _stream())
    if planes:
        call('pps_conv2d_bn_act_h2_planes', _dev(x, 'x planes', torch.int16), x.stride(0), *rest)
    else:
        call('pps_conv2d_bn_act_h2', _dev(x, 'x'), *rest)
    return y


def conv2d_dual_bn_act_h2(x, cin, k, stride, pad, x2, stride2, w2, wrs, kpad1, shift, relu, y,
                          amax_x, amax_x2, amax_y=None, tile=0):
    """conv2d_dual_bn_act in f16x2 arithmetic (pps_conv2d_dual_bn_act_h2)."""
    N, H, W, ldx = x.shape
    _, H2, W2, C2 = x2.shape
    _, Ho, Wo, Cout = y.shape
    call('pps_conv2d_dual_bn_act_h2', _dev(x, 'x'), N, H, W, cin, ldx, k, k, stride, pad,
         _dev(x2, 'x2'), H2, W2, C2, C2, stride2, _dev(w2, 'w2t', torch.int16), _dev(wrs, 'wrs'),
         Cout, kpad1, C2, _dev(shift, 'shift'), int(bool(relu)), _dev(y, 'y'), Ho, Wo, Cout,
         _amax_arg(amax_x, 'amax_x'), _amax_arg(amax_x2, 'amax_x2'), _amax_arg(amax_y, 'amax_y'),
         int(tile), _stream())
    return y


def conv2d_bn_act_pps_h2(x, cin, w2, wrs, kpad, k, stride, pad, dil, scale, shift, residual,
                         split, max_ave, pps_out, amax_x, y=None, tile=0):
    """conv2d_bn_act_pps in f16x2 arithmetic (pps_conv2d_bn_act_pps_h2); x may
    be f16x2 activation planes (pps_conv2d_bn_act_pps_h2_planes)."""
    planes = _h2_planes(x)
    N, H, W, ldx = x.shape[1:] if planes else x.shape
    nsub, n2, Cout = pps_out.shape
    split = np.ascontiguousarray(split, dtype=np.int32)
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    if nsub != (1 << len(split)) - 1 or n2 != N:
        raise RuntimeError('pps_out must be [2^S - 1, N, Cout]')
    rest = (N, H, W, cin, ldx, _dev(w2, 'w2t', torch.int16), _dev(wrs, 'wrs'), Cout, kpad, k, k,
            stride, pad, dil, _dev(scale, 'scale'), _dev(shift, 'shift'),
            _dev(residual, 'residual'), _dev(y, 'y') if y is not None else 0, Ho, Wo,
            split.ctypes.data_as(_lib.ctypes.c_void_p), len(split), int(bool(max_ave)),
            _dev(pps_out, 'pps_out'), _amax_arg(amax_x, 'amax_x'), int(tile), _stream())
    if planes:
        call('pps_conv2d_bn_act_pps_h2_planes', _dev(x, 'x planes', torch.int16), x.stride(0),
             *rest)
    else:
        call('pps_conv2d_bn_act_pps_h2', _dev(x, 'x'), *rest)
    return pps_out


def gemm_bn_act_batched(x, w, scale, shift, relu, y, tile=0):
    """x [B,M,K], w [B,Cout,K] -> y [M, B*Cout] (PPS head convs)."""
    B, M, K = x.shape
    Cout = w.shape[1]
    call('pps_gemm_bn_act_batched', _dev(x, 'x'), M * K, M, K, _dev(w, 'w'), Cout * K,
         Cout, _dev(scale, 'scale'), _dev(shift, 'shift'), int(bool(relu)), _dev(y, 'y'),
         y.stride(0), B, int(tile), _stream())
    return y


def gemm_splitk_batched(x, w, splitk, part, tile=0):
    """x [B,M,K], w [B,Cout,K] (f32) or [B,3,Cout,K] (bf16x3 planes) -> raw
    partials part [splitk, M, B*Cout]."""
    B, M, K = x.shape
    Cout = w.shape[-2]
    fn, wp = _weights('pps_gemm_splitk_batched', w)
    call(fn, _dev(x, 'x'), M, K, wp, Cout, B, splitk, _dev(part, 'part'), int(tile),
         _stream())
    return part


def splitk_bn_act_normalize(part, scale, shift, relu, normalize, y):
    S, M, N = part.shape
    call('pps_splitk_bn_act_normalize', _dev(part, 'part'), S, M, N, _dev(scale, 'scale'),
         _dev(shift, 'shift'), int(bool(relu)), int(bool(normalize)), _dev(y, 'y'), _stream())
    return y


STEM_WIDTH = 128  # input width the fused stem kernel takes (stem.hip kStemW)


def stem_k():
    return _lib.lib().pps_stem_k()


def stem_variant(v=-1):
    """Select the fused stem kernel (0: ring-staged, the default; 1: whole
    tile staged with an LDS epilogue); returns the previous choice, v < 0
    only queries.  Both give identical bits."""
    return _lib.lib().pps_stem_variant(int(v))


def stem_conv_pool_x3(x, w3, scale, shift, y):
    """Fused conv1 7x7/2 + BN + ReLU + maxpool 3x3/2 (pps_stem_conv_pool_x3):
    x NHWC4 [N, H, 128, 4] -> y NHWC [N, Hp, 32, 64]; w3 = split_bf16x3 of
    model.pack_stem_weight."""
    N, H, W, C = x.shape
    _, Hp, Wp, Co = y.shape
    if C != 4 or Co != 64 or tuple(w3.shape) != (3, 64, stem_k()):
        raise RuntimeError('stem: x must be NHWC4, y 64 channels, w3 [3, 64, %d]' % stem_k())
    call('pps_stem_conv_pool_x3', _dev(x, 'x'), N, H, W, _dev(w3, 'w3', torch.int16),
         _dev(scale, 'scale'), _dev(shift, 'shift'), _dev(y, 'y'), Hp, Wp, _stream())
    return y


def stem_split_h2(w):
    """The f16x2 split of the packed stem weight [64, stem_k()] f32
    (pps_stem_split_h2): (w2 [2, 64, stem_k()] f16 planes as int16, w_inv [64]
    the per-channel 2^-s)."""
    if tuple(w.shape) != (64, stem_k()):
        raise RuntimeError('stem weight must be [64, %d]' % stem_k())
    w = w.contiguous()
    w2 = torch.empty((2, 64, stem_k()), dtype=torch.int16, device=w.device)
    winv = torch.empty(64, dtype=torch.float32, device=w.device)
    call('pps_stem_split_h2', _dev(w, 'w'), _dev(w2, 'w2', torch.int16), _dev(winv, 'w_inv'),
         _stream())
    return w2, winv


def stem_conv_pool_h2(x, w2, winv, amax_x, scale, shift, y):
    """The fused stem in f16x2 arithmetic (pps_stem_conv_pool_h2): as
    stem_conv_pool_x3, the input split on the scale of its max (amax_x: an
    activation-max slot, e.g. amax(x)), stem_split_h2 weights."""
    N, H, W, C = x.shape
    _, Hp, Wp, Co = y.shape
    if C != 4 or Co != 64 or tuple(w2.shape) != (2, 64, stem_k()):
        raise RuntimeError('stem: x must be NHWC4, y 64 channels, w2 [2, 64, %d]' % stem_k())
    _amax_arg(amax_x, 'amax_x')
    call('pps_stem_conv_pool_h2', _dev(x, 'x'), N, H, W, _dev(w2, 'w2', torch.int16),
         _dev(winv, 'w_inv'), _dev(amax_x, 'amax_x'), _dev(scale, 'scale'), _dev(shift, 'shift'),
         _dev(y, 'y'), Hp, Wp, _stream())
    return y


def maxpool2d(x, k, stride, pad, y):
    N, H, W, C = x.shape
    _, Ho, Wo, _ = y.shape
    call('pps_maxpool2d', _dev(x, 'x'), N, H, W, C, k, stride, pad, _dev(y, 'y'), Ho, Wo,
         _stream())
    return y


def part_power_set(x, split, max_ave, out):
    N, H, W, C = x.shape
    split = np.ascontiguousarray(split, dtype=np.int32)
    call('pps_part_power_set', _dev(x, 'x'), N, H, W, C,
         split.ctypes.data_as(_lib.ctypes.c_void_p), len(split), int(bool(max_ave)),
         _dev(out, 'out'), _stream())
    return out


def group_mean(x, groups):
    """x [N,D] device; groups: list of index lists -> [len(groups), D] means."""
    N, D = x.shape
    offs = np.zeros(len(groups) + 1, np.int32)
    offs[1:] = np.cumsum([len(g) for g in groups])
    mem = np.concatenate([np.asarray(g, np.int32) for g in groups]) if groups else \
        np.zeros(0, np.int32)
    d_offs = torch.from_numpy(offs).to(x.device)
    d_mem = torch.from_numpy(mem).to(x.device)
    out = torch.empty((len(groups), D), dtype=torch.float32, device=x.device)
    call('pps_group_mean', _dev(x, 'x'), D, d_offs.data_ptr(), d_mem.data_ptr(), len(groups),
         out.data_ptr(), _stream())
    return out


ELTWISE = {'Sum': 0, 'Add': 0, 'Max': 1, 'Mean': 2, 'Relu': 3}


def spatial_bn(x, s, b, rm, riv, eps=1e-5, relu=False, y=None):
    """Caffe2 SpatialBN (is_test) over the last (channel) axis of an NHWC /
    [M, C] tensor (pps_spatial_bn)."""
    C = x.shape[-1]
    if y is None:
        y = torch.empty_like(x)
    call('pps_spatial_bn', _dev(x, 'x'), x.numel() // C, C, _dev(s, 's'), _dev(b, 'b'),
         _dev(rm, 'rm'), _dev(riv, 'riv'), float(eps), int(bool(relu)), _dev(y, 'y'),
         _stream())
    return y


def eltwise(op, xs, y=None):
    """Sum / Add / Max / Mean / Relu of same-shape tensors (pps_eltwise)."""
    xs = list(xs)
    for t in xs[1:]:
        if tuple(t.shape) != tuple(xs[0].shape):
            raise RuntimeError('%s: input shapes differ: %s vs %s'
                               % (op, tuple(xs[0].shape), tuple(t.shape)))
    if y is None:
        y = torch.empty_like(xs[0])
    ptrs = (_lib.ctypes.c_void_p * len(xs))(*[_dev(t, 'input %d' % i) for i, t in enumerate(xs)])
    call('pps_eltwise', ptrs, len(xs), xs[0].numel(), ELTWISE[op], _dev(y, 'y'), _stream())
    return y


def global_pool(x, mode, y=None):
    """AveragePool (mode 'ave') / MaxPool ('max') with global_pooling over an
    NHWC tensor -> [N, C].  x may be an H-slice view of a taller NHWC tensor
    (a Split strip): per-image blocks contiguous, image stride x.stride(0)."""
    N, H, W, C = x.shape
    if x.stride(3) != 1 or x.stride(2) != C or x.stride(1) != W * C:
        raise RuntimeError('global_pool needs per-image contiguous NHWC blocks')
    if y is None:
        y = torch.empty((N, C), dtype=torch.float32, device=x.device)
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError('x must be a float32 device tensor')
    call('pps_global_pool', x.data_ptr(), N, H, W, C, x.stride(0) if N > 1 else H * W * C,
         0 if mode == 'ave' else 1, _dev(y, 'y'), _stream())
    return y


def l2_normalize(x, y=None):
    N, D = x.shape
    if y is None:
        y = torch.empty_like(x)
    call('pps_l2_normalize', _dev(x, 'x'), N, D, _dev(y, 'y'), _stream())
    return y


def preprocess_bgr(img_u8, pixel_means, out_hw, y=None):
    """uint8 BGR [N,Hi,Wi,3] (device) -> NHWC4 float32 [N,Ho,Wo,4]."""
    N, Hi, Wi, C = img_u8.shape
    assert C == 3
    Ho, Wo = out_hw
    if y is None:
        y = torch.empty((N, Ho, Wo, 4), dtype=torch.float32, device=img_u8.device)
    m = np.ascontiguousarray(np.asarray(pixel_means, np.float32).ravel()[:3])
    call('pps_preprocess_bgr', _dev(img_u8, 'img', torch.uint8), N, Hi, Wi,
         m.ctypes.data_as(_lib.ctypes.c_void_p), Ho, Wo, _dev(y, 'y'), _stream())
    return y


# ---------------------------------------------------------------------------
# Operator registry (reference Caffe2 op names): pps_amd/net.py
# ---------------------------------------------------------------------------
def run_op(name, inputs, **args):
    """Look up an operator by its reference (Caffe2) name and run it
    (the registry is net.OPS: every op name of the reference's test net)."""
    from .net import run_op as _run
    return _run(name, inputs, **args)


def preprocess_bgr_ragged(blob_u8, offsets, heights, widths, pixel_means, out_hw, y=None):
    """Ragged batch: blob_u8 flat uint8 device tensor; offsets int64 [N],
    heights/widths int32 [N] device tensors -> NHWC4 float32 [N,Ho,Wo,4]."""
    N = offsets.shape[0]
    Ho, Wo = out_hw
    if y is None:
        y = torch.empty((N, Ho, Wo, 4), dtype=torch.float32, device=blob_u8.device)
    m = np.ascontiguousarray(np.asarray(pixel_means, np.float32).ravel()[:3])
    call('pps_preprocess_bgr_ragged', _dev(blob_u8, 'blob', torch.uint8), N,
         _dev(offsets, 'offsets', torch.int64), _dev(heights, 'heights', torch.int32),
         _dev(widths, 'widths', torch.int32), m.ctypes.data_as(_lib.ctypes.c_void_p), Ho, Wo,
         _dev(y, 'y'), _stream())
    return y
