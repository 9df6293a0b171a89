// The frame of the matrix-free f16x2 kernels: what search_h2_kernel
// (search_h2.hip), rank_count_h2_kernel (rank_h2.hip) and the two listed-pair
// kernels (pair_h2.hip) share, each piece defined once.  A kernel calls the
// pieces in straight-line code around an epilogue of its own; nothing here
// takes a functor or owns a loop over tiles.
//
// Tiled kernels.  Work item = (query panel of BM rows, gallery segment s of
// S); a workgroup strides over the items and walks the BN-column tiles of its
// segment.  Per tile: h2_kloop, then for each of the HB column passes
// fused_park, fused_cols and, per row and column, fused_cell.
// Listed pairs.  pair_dots: one wave, one a-row, up to 64 listed b-rows.
//
// Every distance is h2_finish of an accumulator that h2_kloop or pair_dots
// built from mfma_h2t over the chunks in ascending order -- the bits
// gemm_h2_kernel's h2_dist_epilogue writes at that cell.
#pragma once
#include "gemm_h2_common.hpp"
#include "retrieval.hpp"

namespace pps {

// The one finish outside h2_dist_epilogue: the dot product scaled back by two
// exact power-of-two multiplies, the row's scale first, then dist_value.  The
// order is h2_dist_epilogue's; with it the result has that kernel's bits.
__device__ __forceinline__ float h2_finish(const GemmParams& p, float dot, float ra, float rb,
                                           float qn, float gn) {
  return dist_value(p, (dot * ra) * rb, qn, gn);
}

// ---- work list --------------------------------------------------------------
struct FusedPlan {
  int S, tps, tiles_n;   // segments, gallery tiles per segment, gallery tiles
  int64_t items;         // panels * S
};
// S0: the wanted segment count (fused_segments, under the caller's own clamps)
inline FusedPlan fused_plan(int64_t Q, int64_t G, int64_t S0, int BM, int BN) {
  FusedPlan f;
  f.tiles_n = (int)cdiv(G, BN);
  f.tps = (int)cdiv(f.tiles_n, S0);
  f.S = (int)cdiv(f.tiles_n, f.tps);   // no empty segment
  f.items = cdiv(Q, BM) * f.S;
  return f;
}
inline unsigned fused_grid(const FusedPlan& f) {
  return (unsigned)(f.items < kSearchSlots ? f.items : kSearchSlots);
}

struct FusedItem {
  int s, m0, mrem, t0, t1;   // segment; first row, rows left from it; tiles [t0, t1)
};
__device__ __forceinline__ FusedItem fused_item(const FusedPlan& f, int64_t item, int M, int BM) {
  const int panel = (int)(item / f.S);
  FusedItem it;
  it.s = (int)(item - (int64_t)panel * f.S);
  it.m0 = panel * BM;
  it.mrem = M - it.m0;
  it.t0 = it.s * f.tps;
  it.t1 = min(it.t0 + f.tps, f.tiles_n);
  return it;
}

// ---- the parked tile --------------------------------------------------------
template <int BM, int BN, int WM, int WN, int NS>
struct FusedTile : H2Tile<BM, BN, WM, WN, NS> {
  using T = H2Tile<BM, BN, WM, WN, NS>;
  static constexpr int WCOLS = BN / WN;               // columns of a wave
  static constexpr int BNH = BN / T::HB, LD = BNH + 4;  // columns of a pass, parked row stride
  static constexpr int RPW = BM / T::NW;              // rows a wave finishes
  static constexpr int CS = (BNH + 63) / 64;          // columns per lane and pass
  static constexpr int STATE = T::LDS_BYTES;          // a kernel's row state starts here
  static_assert(BM % T::NW == 0, "rows per wave");
  static_assert(BNH % WCOLS == 0, "a wave's columns fall in one pass");
  static_assert(STATE % 16 == 0, "row state alignment");
};

// Pass hb of a tile: after the barrier that ends every read of the stages (or
// of the previous pass), the waves whose columns fall in the pass write their
// accumulators to t[row][column of the pass]; the second barrier publishes them.
template <class F>
__device__ __forceinline__ void fused_park(float* t, const f32x4 (&acc)[F::TM][F::TN], int hb,
                                           int wm, int wn, int lane) {
  const int r16 = lane & 15, h = lane >> 4;
  const int wc0 = wn * F::WCOLS;
  const int c0h = hb * F::BNH;
  __syncthreads();  // the stages / the previous pass are no longer read
  if (wc0 >= c0h && wc0 < c0h + F::BNH) {
#pragma unroll
    for (int i = 0; i < F::TM; ++i) {
      const int row = wm * (F::TM * 16) + i * 16 + r16;
#pragma unroll
      for (int j = 0; j < F::TN; ++j) {
        const int col = wc0 - c0h + j * 16 + 4 * h;
        *reinterpret_cast<f32x4*>(t + (row * F::LD + col)) = acc[i][j];
      }
    }
  }
  __syncthreads();
}

// This lane's columns of pass hb (column j * 64 + lane of the pass, gallery
// row n0 + hb * BNH + that): inside the pass and the gallery?  norm and scale,
// loaded once for all rows (0 where not ok).  rank_count_h2_kernel writes this
// loop out (its camera load beside it): called from there it costs the
// 192 x 192 instantiations SGPR spills.
template <class F>
__device__ __forceinline__ void fused_cols(const GemmParams& p, int n0, int hb, int lane,
                                           bool (&ok)[F::CS], float (&gn)[F::CS],
                                           float (&rb)[F::CS]) {
  const int c0h = hb * F::BNH;
  const int nrem = p.Ncol - n0;
#pragma unroll
  for (int j = 0; j < F::CS; ++j) {
    const int c = j * 64 + lane;
    ok[j] = c < F::BNH && c0h + c < nrem;
    gn[j] = ok[j] ? p.norm_b[n0 + c0h + c] : 0.f;
    rb[j] = ok[j] ? p.rs_b[n0 + c0h + c] : 0.f;
  }
}

// The distance at parked row `row`, column c of the pass (qn, ra: the row's
// norm and scale; gn, rb: the column's); a column that is not ok finishes a
// zero dot product.
template <class F>
__device__ __forceinline__ float fused_cell(const GemmParams& p, const float* t, int row, int c,
                                            bool ok, float qn, float ra, float gn, float rb) {
  const float dot = ok ? t[row * F::LD + c] : 0.f;
  return h2_finish(p, dot, ra, rb, qn, gn);
}

// ---- listed pairs: two plane operands as those kernels read them --------------
struct PairOperands {
  const unsigned char* q2t;   // planes as bytes
  const unsigned char* g2t;
  int64_t q_plane, g_plane;   // bytes between an operand's two planes
  const float* qsq; const float* qrs;
  const float* gsq; const float* grs;
  int64_t Q;
  int nkc, metric;
};
// the rows of q (a-rows) against the planes of g
inline PairOperands pair_operands(const H2Operand& q, const H2Operand& g, int D, int metric) {
  PairOperands o{};
  o.q2t = reinterpret_cast<const unsigned char*>(q.planes);
  o.g2t = reinterpret_cast<const unsigned char*>(g.planes);
  o.q_plane = h2_plane_elems(q.plane_rows, D) * 2;
  o.g_plane = h2_plane_elems(g.plane_rows, D) * 2;
  o.qsq = q.sq; o.qrs = q.rs; o.gsq = g.sq; o.grs = g.rs;
  o.Q = q.rows;
  o.nkc = D / 32;
  o.metric = metric;
  return o;
}

// this lane's fragment of a-row q, chunk 0 (what pair_dots takes as qa)
__device__ __forceinline__ const unsigned char* pair_a_frag(const PairOperands& a, int q, int lane) {
  return a.q2t + h2_frag_off(q, a.nkc, lane >> 4);
}

// One wave, the a-row of fragment qa, list entries m0 .. min(m0 + 64, end) - 1,
// entry e naming b-row row_of(e): returns lane i's dot product of entry m0 + i (lanes past
// the list: some entry's).  The 64 entries are four blocks of 16 MFMA columns;
// per K chunk each lane loads its 16-byte fragments straight from the tiled
// planes in global memory (the a-row's and its block column's b-row's, slot
// lane >> 4, both planes; no LDS).  All 16 a-rows of the MFMA are the one row,
// so every lane group holds a copy of a block's 16 dot products.  Call with
// all lanes of the wave (MFMA).
//
// PARTS: the b-rows live in two plane sets -- row r < p.B0 is row r of a's b
// operand, any other row is row r - p.B0 of p's -- so a block column carries
// its own base and its own plane stride.  Nothing else differs: same loads,
// same MFMA order, same bits.
struct PairPart {   // the second b operand of the two-part form
  const unsigned char* g2t;
  int64_t g_plane;
  const float* gsq; const float* grs;
  int B0;           // rows of the first b operand
};
template <bool PARTS, class RowOf>
__device__ __forceinline__ float pair_dots_impl(const PairOperands& a, const PairPart& p,
                                                const unsigned char* qa, int m0, int end, int lane,
                                                RowOf row_of) {
  const int r16 = lane & 15, slot = lane >> 4;
  const int nb = min(4, (end - m0 + 15) >> 4);   // blocks with an entry (wave-uniform)
  const unsigned char* ga[4];
  int64_t gp[4];   // PARTS only
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    // columns past the list repeat its last entry (their cells are not read)
    const int mi = min(m0 + 16 * b + r16, end - 1);
    if constexpr (PARTS) {
      const int r = row_of(mi);
      const bool second = r >= p.B0;
      ga[b] = (second ? p.g2t : a.g2t) + h2_frag_off(second ? r - p.B0 : r, a.nkc, slot);
      gp[b] = second ? p.g_plane : a.g_plane;
    } else {
      ga[b] = a.g2t + h2_frag_off(row_of(mi), a.nkc, slot);
    }
  }
  f32x4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < a.nkc; ++kc) {
    const int64_t ko = (int64_t)kc * 1024;
    const f16x8 q0 = *reinterpret_cast<const f16x8*>(qa + ko);
    const f16x8 q1 = *reinterpret_cast<const f16x8*>(qa + a.q_plane + ko);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b < nb) {
        const f16x8 g0 = *reinterpret_cast<const f16x8*>(ga[b] + ko);
        int64_t plane = a.g_plane;
        if constexpr (PARTS) plane = gp[b];
        const f16x8 g1 = *reinterpret_cast<const f16x8*>(ga[b] + plane + ko);
        acc[b] = mfma_h2t(q0, q1, g0, g1, acc[b]);
      }
    }
  }
  // lane i's entry sits in block i >> 4, column i & 15: register i & 3 of the
  // lanes 16 ((i & 15) >> 2) + r, any r.  Every lane picks register
  // (r >> 2, r & 3) of its own; lane i then reads lane
  // 16 ((i & 15) >> 2) + 4 (i >> 4) + (i & 3).
  const int src = 16 * ((lane & 15) >> 2) + 4 * (lane >> 4) + (lane & 3);
  const int rb4 = r16 >> 2, re = lane & 3;
  const f32x4 t = rb4 == 0 ? acc[0] : rb4 == 1 ? acc[1] : rb4 == 2 ? acc[2] : acc[3];
  const float mine = re == 0 ? t[0] : re == 1 ? t[1] : re == 2 ? t[2] : t[3];
  return __shfl(mine, src);
}
template <class RowOf>
__device__ __forceinline__ float pair_dots(const PairOperands& a, const unsigned char* qa, int m0,
                                           int end, int lane, RowOf row_of) {
  return pair_dots_impl<false>(a, PairPart{}, qa, m0, end, lane, row_of);
}
template <class RowOf>
__device__ __forceinline__ float pair_dots_parts(const PairOperands& a, const PairPart& p,
                                                 const unsigned char* qa, int m0, int end,
                                                 int lane, RowOf row_of) {
  return pair_dots_impl<true>(a, p, qa, m0, end, lane, row_of);
}

}  // namespace pps
