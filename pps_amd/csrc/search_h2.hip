// Fused f16x2 distance + stable top-k ("search"): the k nearest gallery rows
// of every query without the [Q, G] distance matrix.
//
// This file holds search_h2_kernel -- the fused frame of h2_fused_common.hpp
// (work item = query panel x gallery segment, h2_kloop per tile, the
// accumulators parked in LDS, fused_cell finishing each distance with the bits
// pps_distmat_h2_tiled would have written) around a top-k filter -- its host
// plan and workspace layout, and the three search entry points.
// Instead of storing the distances, each wave filters its rows of the parked tile:
// a column survives if its packed (float_key(d) << 32 | column) value is not
// above the row's threshold and is appended to the row's candidate buffer;
// when the next pass could overflow the buffer the wave cuts it back to
// between k and k + kTkwSlack entries (wave_cut, the select of
// topk_wave_kernel) and the cut's bound becomes the threshold.  After the
// segment's last tile the row's exact k best are sorted and written to the
// partial list [S][Q][k] (ascending, ties by column, segment-local columns);
// topk_merge joins the S lists on the same stream.  The stable (distance,
// index) top-k is unique, so the result equals topk(distmat) bit for bit for
// every tile and segment count.
//
// EXCL instantiations also drop, in the filter itself, the columns whose
// group equals the row's non-negative group (SearchArgs::q_group / g_group):
// an excluded column never enters a candidate buffer, because cuts and
// thresholds are computed from buffer contents -- let in and removed at the
// end, it could push a member of the true answer out at a cut.  The result is
// the stable top-k of the remaining columns, padded with (+inf, -1).
//
// No workgroup waits on another: a work item touches only its own candidate
// buffers (one set per launched workgroup, reused over the items the
// workgroup strides through) and its own partial list.
//
// LDS: the pipeline stages / the parked tile as in gemm_h2_kernel, plus 16
// bytes of row state (threshold, count) per query row beside them.  The
// candidate buffers live in the caller's workspace.
#include <algorithm>

#include "h2_fused_common.hpp"
#include "topk_wave_common.hpp"

namespace pps {

// tile ids (kSearchNumTiles) and the launch width (kSearchSlots): retrieval.hpp
constexpr int kSearchMaxBM = 256;    // rows of a slot's buffer set
constexpr int kSearchInflow = 256;   // most columns a row can receive between two cut checks
// entries of one row's candidate buffer: what a cut keeps + one pass's inflow
constexpr int search_cap(int k) { return (k + kTkwSlack + kSearchInflow + 63) / 64 * 64; }
constexpr int kSearchJ = search_cap(kTkwMaxK) / 64;   // registers per lane of a cut

struct SearchArgs {
  int k, cap;
  FusedPlan plan;
  unsigned long long* cand;       // [slots][BM][cap]
  float* pvals;                   // [S][Q][k]
  int32_t* pidx;
  // EXCL kernels only: column c is dropped for row r iff
  // q_group[r] >= 0 && g_group[c] == q_group[r] (global row / column)
  const int32_t* q_group;         // [Q]
  const int32_t* g_group;         // [G]
  // ROWMAX kernels only: [Q], zeroed by the entry; receives the bits of
  // max_c fl(d * d) over the real columns by atomicMax (squares are >= 0)
  unsigned* rowmax;
};

// orders a wave's accesses to its candidate buffer in global memory (lane a's
// store, lane b's later load)
__device__ inline void wave_global_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// ascending bitonic sort of buf[0, n2) (LDS), n2 a power of two, by one wave
__device__ inline void wave_bitonic(unsigned long long* buf, int n2) {
  const int lane = threadIdx.x & 63;
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < n2 / 2; t += 64) {
        const int i = 2 * stride * (t / stride) + (t % stride), j = i + stride;
        const bool up = (i & size) == 0;
        const unsigned long long a = buf[i], b = buf[j];
        if ((a > b) == up) { buf[i] = b; buf[j] = a; }
      }
      wave_lds_sync();
    }
}

__device__ inline unsigned long long uniform_u64(unsigned long long x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

template <int BM, int BN, int WM, int WN, int NS, bool EXCL, bool ROWMAX = false>
__global__ void __launch_bounds__(64 * WM * WN)
search_h2_kernel(GemmParams p, SearchArgs a) {
  using F = FusedTile<BM, BN, WM, WN, NS>;
  constexpr int NW = F::NW, TM = F::TM, TN = F::TN, HB = F::HB;
  constexpr int BNH = F::BNH, RPW = F::RPW, CS = F::CS, STATE = F::STATE;
  static_assert(BM <= kSearchMaxBM, "slot rows");
  static_assert(BNH <= kSearchInflow, "a pass's inflow is what search_cap leaves room for");
  static_assert(NW * kTkwMaxK * 8 <= F::LDS_BYTES, "sort scratch of the waves");
  static_assert(STATE + BM * 16 <= kLdsBytesGfx950, "LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[STATE + BM * 16];
  unsigned long long* s_thr = reinterpret_cast<unsigned long long*>(lds + STATE);
  int* s_n = reinterpret_cast<int*>(lds + STATE + BM * 8);
  float* t = reinterpret_cast<float*>(lds);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int k = a.k, cap = a.cap;
  unsigned long long* cand = a.cand + (int64_t)blockIdx.x * BM * cap;
  unsigned long long* sbuf = reinterpret_cast<unsigned long long*>(lds) + wave * kTkwMaxK;

  for (int64_t item = blockIdx.x; item < a.plan.items; item += gridDim.x) {
    const FusedItem it = fused_item(a.plan, item, p.M, BM);
    const int s = it.s, m0 = it.m0, mrem = it.mrem;
    const int cbase = it.t0 * BN;   // the segment's first gallery column
    // the rows of this wave start empty (only this wave touches their state)
    for (int r = lane; r < RPW; r += 64) {
      s_thr[wave * RPW + r] = ~0ull;   // inclusive: entries <= thr stay candidates
      s_n[wave * RPW + r] = 0;
    }

    for (int tn = it.t0; tn < it.t1; ++tn) {
      const int n0 = tn * BN;
      f32x4 acc[TM][TN];
      h2_kloop<BM, BN, WM, WN, NS>(p, lds, m0, n0, wave, lane, wm, wn, acc);

#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        const int c0h = hb * BNH;
        fused_park<F>(t, acc, hb, wm, wn, lane);
        bool ok[CS];
        float gn[CS], rb[CS];
        fused_cols<F>(p, n0, hb, lane, ok, gn, rb);
        for (int i = 0; i < RPW; ++i) {
          const int row = wave * RPW + i;   // wave-uniform
          if (row >= mrem) break;
          const int gr = m0 + row;
          const float qn = p.norm_a[gr];
          const float ra = p.rs_a[gr];
          int qg = -1;   // wave-uniform; negative excludes nothing
          if constexpr (EXCL) qg = __builtin_amdgcn_readfirstlane(a.q_group[gr]);
          unsigned long long thr = uniform_u64(s_thr[row]);
          int n = __builtin_amdgcn_readfirstlane(s_n[row]);
          unsigned long long* buf = cand + (int64_t)row * cap;
          // room for this pass; and once, as soon as a real threshold exists
          if (n + BNH > cap || (thr == ~0ull && n > k + kTkwSlack)) {
            wave_global_sync();
            thr = wave_cut<kSearchJ>(buf, n, k, kTkwSlack);
            wave_global_sync();
          }
          float mx = 0.f;   // ROWMAX: max |d| of this lane's real columns
#pragma unroll
          for (int j = 0; j < CS; ++j) {
            const int c = j * 64 + lane;
            const float d = fused_cell<F>(p, t, row, c, ok[j], qn, ra, gn[j], rb[j]);
            if constexpr (ROWMAX) {
              if (ok[j]) mx = fmaxf(mx, fabsf(d));   // padded columns never count
            }
            const unsigned long long packed =
                ((unsigned long long)float_key(d) << 32) | (uint32_t)(n0 + c0h + c - cbase);
            bool take = ok[j] && packed <= thr;
            // the group is loaded for survivors of the threshold only (no
            // column codes held live over the rows)
            if constexpr (EXCL) {
              if (qg >= 0 && take) take = a.g_group[n0 + c0h + c] != qg;
            }
            const unsigned long long bal = __ballot(take);
            if (take)
              buf[n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = packed;
            n += __popcll(bal);
          }
          if constexpr (ROWMAX) {
            // fl(d * d) is monotone in |d|: one square of the pass's maximum
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            if (lane == 0) atomicMax(a.rowmax + gr, __float_as_uint(mx * mx));
          }
          if (lane == 0) {
            s_thr[row] = thr;
            s_n[row] = n;
          }
        }
      }
      __syncthreads();  // the parked tile is no longer read: the next K loop may stage
    }

    // the segment's list: each row's exact k best, sorted in this wave's LDS scratch
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = 0; i < RPW; ++i) {
      const int row = wave * RPW + i;
      if (row >= mrem) break;
      int n = __builtin_amdgcn_readfirstlane(s_n[row]);
      unsigned long long* buf = cand + (int64_t)row * cap;
      wave_global_sync();
      if (n > k) {
        wave_cut<kSearchJ>(buf, n, k, 0);
        wave_global_sync();
      }
      for (int e = lane; e < n2; e += 64) sbuf[e] = e < n ? buf[e] : ~0ull;
      wave_lds_sync();
      wave_bitonic(sbuf, n2);
      const int64_t o = ((int64_t)s * p.M + (m0 + row)) * k;
      for (int e = lane; e < k; e += 64) {
        const unsigned long long v = sbuf[e];
        a.pvals[o + e] = e < n ? key_float((uint32_t)(v >> 32)) : __builtin_huge_valf();
        a.pidx[o + e] = e < n ? (int32_t)(v & 0xffffffffu) : -1;
      }
      wave_lds_sync();   // sbuf is rewritten for the next row
    }
    __syncthreads();  // the sort scratch is free before the next item stages
  }
}

__global__ void search_fill_pad_kernel(float* vals, int32_t* idx, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    vals[i] = __builtin_huge_valf();
    idx[i] = -1;
  }
}

// ---- host plan ---------------------------------------------------------------
static inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// Segment count before it is rounded to whole tiles per segment:
// fused_segments (the request, 0 = auto, under the segment's tile count) under
// topk_merge's clamps -- kMergeMaxLists lists and kMergeMaxEntries merged
// entries.  Non-decreasing in G.
static int search_segments(int64_t Q, int64_t G, int k, int segments, int BM, int BN) {
  int64_t S = fused_segments(Q, G, segments, BM, BN);
  S = std::min<int64_t>(S, kMergeMaxLists);
  S = std::min<int64_t>(S, kMergeMaxEntries / k);
  return (int)std::max<int64_t>(S, 1);
}

struct SearchLayout {
  int64_t cand_bytes, part_entries, total;
};
// tile-independent (the larger need of the two tile shapes)
static SearchLayout search_layout(int64_t Q, int64_t G, int k, int segments) {
  int S = 1;
  int64_t slots = 1;   // workgroups launched: one buffer set each
  for (int tile = 1; tile < kSearchNumTiles; ++tile) {
    int BM, BN;
    search_tile_shape(tile, BM, BN);
    const int St = search_segments(Q, G, k, segments, BM, BN);
    S = std::max(S, St);
    slots = std::max(slots, std::min<int64_t>(kSearchSlots, cdiv(Q, BM) * St));
  }
  SearchLayout L;
  L.cand_bytes = align256(slots * kSearchMaxBM * search_cap(k) * 8);
  L.part_entries = (int64_t)S * Q * k;
  L.total = L.cand_bytes + 2 * align256(L.part_entries * 4);
  return L;
}

template <int BM, int BN, int WM, int WN, int NS, bool EXCL, bool ROWMAX>
static int launch_search(const GemmParams& p, SearchArgs a, hipStream_t st) {
  hipLaunchKernelGGL((search_h2_kernel<BM, BN, WM, WN, NS, EXCL, ROWMAX>),
                     dim3(fused_grid(a.plan)), dim3(64 * WM * WN), 0, st, p, a);
  PPS_CHECK_LAUNCH("search_h2_kernel");
  return PPS_OK;
}

// the two tile shapes of one filter variant
template <bool EXCL, bool ROWMAX>
static int launch_search_tile(int tile, const GemmParams& p, const SearchArgs& a, hipStream_t st) {
  return tile == 2 ? launch_search<192, 192, 2, 4, 3, EXCL, ROWMAX>(p, a, st)
                   : launch_search<256, 256, 2, 4, 2, EXCL, ROWMAX>(p, a, st);
}

// An upper bound of search_layout(N, N, k, segments).total (a self-search: the
// queries grow with the gallery, and the auto segment count then falls in
// steps) that is non-decreasing in N.  S <= the gallery's tiles and <= the
// request; auto: S <= 2 kSearchSlots / panels <= 512 BM / N, so S * N <= 2^17.
int64_t search_h2_self_workspace_bound(int64_t N, int k, int segments) {
  const int64_t tiles = std::max<int64_t>(cdiv(N, 192), 1);   // the finer tile shape's count
  const int64_t slots = std::min<int64_t>(kSearchSlots, tiles * tiles);
  const int64_t by_req = segments > 0 ? N * std::min<int64_t>(segments, kMergeMaxLists)
                                      : std::max<int64_t>(N, 2 * kSearchSlots * kSearchMaxBM);
  const int64_t entries = k * std::min<int64_t>(by_req, N * tiles);
  return align256(slots * kSearchMaxBM * search_cap(k) * 8) + 2 * align256(entries * 4);
}

// The same bound for Q a-rows against G b-rows: at least
// search_layout(Q, G, k, segments).total and non-decreasing in Q and in G.
// S <= the gallery's tiles, <= kMergeMaxLists and <= the request; auto:
// S <= 2 kSearchSlots / panels, so S * Q <= max(Q, 2^17).  Every term of the
// min below grows with both arguments.
int64_t search_h2_workspace_bound(int64_t Q, int64_t G, int k, int segments) {
  const int64_t tq = std::max<int64_t>(cdiv(Q, 192), 1), tg = std::max<int64_t>(cdiv(G, 192), 1);
  const int64_t slots = std::min<int64_t>(kSearchSlots, tq * tg);
  const int64_t by_req = segments > 0 ? Q * std::min<int64_t>(segments, kMergeMaxLists)
                                      : std::max<int64_t>(Q, 2 * kSearchSlots * kSearchMaxBM);
  const int64_t entries = k * std::min<int64_t>(by_req, Q * std::min<int64_t>(tg, kMergeMaxLists));
  return align256(slots * kSearchMaxBM * search_cap(k) * 8) + 2 * align256(entries * 4);
}

}  // namespace pps

// ---- C ABI ----------------------------------------------------------------
using namespace pps;

int pps_search_max_k(void) { return kTkwMaxK; }

int pps_search_h2_num_tiles(void) { return kSearchNumTiles; }

int64_t pps_search_h2_workspace_bytes(int64_t Q, int64_t G, int k, int segments) {
  if (Q < 0 || G < 0 || k < 1 || k > kTkwMaxK || segments < 0) return -1;
  return search_layout(Q, G, k, segments).total;
}

// pps_search_h2_tiled (excl false), pps_search_h2_tiled_excl (excl true) and
// pps_search_h2_tiled_rowmax (rowmax given, no exclusion)
int pps::search_h2_tiled(const char* fn, bool excl, const H2Operand& q, const H2Operand& g, int D,
                         int metric, int k, int segments, int tile, void* workspace,
                         int64_t ws_bytes, float* vals, int32_t* idx, const int32_t* q_group,
                         const int32_t* g_group, float* rowmax, void* stream) {
  const int64_t Q = q.rows, G = g.rows;
  PPS_ENFORCE_AS(fn, vals && idx, "null pointer");
  PPS_ENFORCE_AS(fn, !excl || (q_group && g_group), "null group pointer");
  PPS_TRY(h2_operands_guard(fn, q, g, D, metric));
  PPS_ENFORCE_AS(fn, k >= 1 && k <= kTkwMaxK,
                 "k must be in [1, " + std::to_string(kTkwMaxK) + "]");
  PPS_TRY(fused_plan_guard(fn, segments, tile));
  if (Q == 0) return PPS_OK;
  hipStream_t st = as_stream(stream);
  if (G == 0) {  // nothing to rank: pad entries only
    if (rowmax) (void)hipMemsetAsync(rowmax, 0, sizeof(float) * Q, st);
    const int64_t n = Q * k;
    hipLaunchKernelGGL(search_fill_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       vals, idx, n);
    PPS_CHECK_LAUNCH("search_fill_pad_kernel");
    return PPS_OK;
  }
  const SearchLayout L = search_layout(Q, G, k, segments);
  if (!workspace || ws_bytes < L.total) {
    set_error(std::string(fn) + ": workspace of " + std::to_string(ws_bytes) + " bytes, need " +
              std::to_string(L.total));
    return PPS_ERR_CAPACITY;
  }
  PPS_ENFORCE_AS(fn, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");

  int BM, BN;
  search_tile_shape(tile, BM, BN);
  SearchArgs a{};
  a.k = k;
  a.cap = search_cap(k);
  a.plan = fused_plan(Q, G, search_segments(Q, G, k, segments, BM, BN), BM, BN);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  a.cand = reinterpret_cast<unsigned long long*>(ws);
  a.pvals = reinterpret_cast<float*>(ws + L.cand_bytes);
  a.pidx = reinterpret_cast<int32_t*>(ws + L.cand_bytes + (L.total - L.cand_bytes) / 2);
  a.q_group = q_group;
  a.g_group = g_group;
  a.rowmax = reinterpret_cast<unsigned*>(rowmax);
  if (rowmax) (void)hipMemsetAsync(rowmax, 0, sizeof(float) * Q, st);   // the atomicMax's zero

  const GemmParams p = h2_params(q, g, D, metric);
  const int rc = excl ? launch_search_tile<true, false>(tile, p, a, st)
                      : (rowmax ? launch_search_tile<false, true>(tile, p, a, st)
                                : launch_search_tile<false, false>(tile, p, a, st));
  if (rc != PPS_OK) return rc;
  MergeOffsets offs{};
  for (int s = 0; s < a.plan.S; ++s) offs.off[s] = (int64_t)s * a.plan.tps * BN;
  return topk_merge(a.pvals, a.pidx, a.plan.S, Q, k, offs, k, vals, idx, st);
}

int pps_search_h2_tiled(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                        const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                        int D, int metric, int k, int segments, int tile, void* workspace,
                        int64_t ws_bytes, float* vals, int32_t* idx, void* stream) {
  return search_h2_tiled("pps_search_h2_tiled", false, h2_operand(q2t, qsq, qrs, Q),
                         h2_operand(g2t, gsq, grs, G), D, metric, k, segments, tile, workspace,
                         ws_bytes, vals, idx, nullptr, nullptr, nullptr, stream);
}

int pps_search_h2_tiled_rowmax(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                               const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                               int D, int metric, int k, int segments, int tile, void* workspace,
                               int64_t ws_bytes, float* vals, int32_t* idx, float* rowmax,
                               void* stream) {
  PPS_ENFORCE(rowmax, "null pointer");
  return search_h2_tiled("pps_search_h2_tiled_rowmax", false, h2_operand(q2t, qsq, qrs, Q),
                         h2_operand(g2t, gsq, grs, G), D, metric, k, segments, tile, workspace,
                         ws_bytes, vals, idx, nullptr, nullptr, rowmax, stream);
}

int pps_search_h2_tiled_excl(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                             const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                             int D, int metric, int k, int segments, int tile, void* workspace,
                             int64_t ws_bytes, float* vals, int32_t* idx,
                             const int32_t* q_group, const int32_t* g_group, void* stream) {
  return search_h2_tiled("pps_search_h2_tiled_excl", true, h2_operand(q2t, qsq, qrs, Q),
                         h2_operand(g2t, gsq, grs, G), D, metric, k, segments, tile, workspace,
                         ws_bytes, vals, idx, q_group, g_group, nullptr, stream);
}
