// Matrix-free rank counts ("fused mAP" and the fractional / separate-camera
// CMC): rank_count_stream's and cmc_count_kernel's twin (eval_counts.hip) that
// computes the f16x2 distances on the fly from the operands' chunk-tiled planes
// instead of reading the [Q, G] matrix.  Every distance has the bits
// pps_distmat_h2_tiled would have written (h2_fused_common.hpp), so the counts
// equal the materialised path's exactly and rank_prepare / ap_finalize /
// cmc_finalize run unchanged around it.  This file holds the count kernel, its
// two junk follow-ups and the two count entry points; the lists the counts are
// taken against come from pps_collect_matches_h2 (pair_h2.hip).
//
// rank_count_h2_kernel: the fused frame of h2_fused_common.hpp (work item =
//    query panel x gallery segment, workgroups striding over the items,
//    h2_kloop per tile, accumulators parked in LDS, each wave finishing BM / 8
//    rows) with a counting epilogue.  A row's first and
//    last positive distance (df, dmax), the first positive's index and its
//    list length sit in 16 B of LDS row state.  A pass none of whose columns
//    has d <= dmax is left after one ballot per 64 columns (the common case:
//    only the entries ranked before the last true match count).  Otherwise
//    the row's sorted positives are staged, 256 at a time, in 1 KiB of LDS the
//    wave owns (four loads a lane from L2; the next row's first block is
//    requested while this row is binned, since hits come in runs of rows), and
//    every lane finds lower_bound(sorted_d[q], d) of its columns with eight
//    branch-free LDS probes -- rank_count_stream's binning, ties between
//    positives included -- and adds 1 to that bin.  A first version counted
//    with one ballot per positive and 64 columns (C_p = #(d <= S_p), S_p by
//    readlane): 82 ms against this one's 28 ms where every column of a
//    10,000 x 125,000 shard is a hit.  `before` is one more ballot,
//    d < df || (d == df && global column < idf).  Counts go out as no-return
//    atomics, one per hit: a hit pass's columns spread over about as many bins
//    as it has columns, so summing per pass first would save nothing, and a
//    per-item staging copy in global memory would cost a load and a store
//    where the atomic costs one operation -- there is no workspace.
//    The junk entries (this gallery segment's, with the pair kernel's
//    distances) are taken back out by a small follow-up kernel on the same
//    stream, as rank_count_stream's chunk 0 does.
//
// Its KEY parameter (kBinDist below) chooses the bins: the distance bins of
//    mAP, or cmc_count_kernel's key bins -- pps_cmc_counts on the h2 matrix,
//    exactly.
//
// No workgroup waits on another; nothing is launched cooperatively.
#include <algorithm>

#include "h2_fused_common.hpp"
#include "topk_wave_common.hpp"

namespace pps {

struct RankH2Args {
  FusedPlan plan;
  int64_t g_offset;
  int Ptot;
  const float* sorted_d;          // [Q][Ptot]
  const int32_t* sorted_idx;
  const int32_t* pos_total;       // [Q]
  int32_t* hist;                  // [Q][Ptot]
  int32_t* before;                // [Q] (distance bins only)
  const int32_t* qcam;            // [Q], this gallery's local [G]: separate-camera key bins
  const int32_t* gcam;
};

// What a valid column adds to hist (the kernel's KEY parameter):
//  kBinDist    rank_count_stream's bins, lower_bound(sorted_d, d), and `before`;
//  kBinKey     cmc_count_kernel's: b = #positives whose (distance, global index)
//              key is below the column's own, counted when b < P; every column
//              is valid (the junk entries are taken back out afterwards);
//  kBinKeyCam  the same bins, a column valid iff gcam[c] != qcam[q]
//              (separate_camera_set; no junk lists).
// The key bin is the distance bin unless d equals a positive's distance
// (s_S[lo] == d): then the column goes past the positives of that tie group
// with a lower global index, found by a binary search on sorted_idx over
// [lo, P) in global memory (L2) -- the tie group may leave the staged block,
// and a second 8 KiB of index blocks would not fit beside the 192 x 192 tile.
// A positive's own column takes that path (b = its own position), so it runs
// at least P times per row, and otherwise only for copied gallery rows.
constexpr int kBinDist = 0, kBinKey = 1, kBinKeyCam = 2;

__device__ inline float uniform_f32(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

template <int BM, int BN, int WM, int WN, int NS, int KEY>
__global__ void __launch_bounds__(64 * WM * WN)
rank_count_h2_kernel(GemmParams p, RankH2Args a) {
  using F = FusedTile<BM, BN, WM, WN, NS>;
  constexpr int NW = F::NW, TM = F::TM, TN = F::TN, HB = F::HB;
  constexpr int BNH = F::BNH, RPW = F::RPW, CS = F::CS, STATE = F::STATE;
  static_assert(RPW <= 64, "a lane per row sets the row state up");
  constexpr int NB = 4, PB = 64 * NB;      // positives binned per round: NB registers a lane
  static_assert(STATE + BM * 16 + NW * PB * 4 <= kLdsBytesGfx950, "LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[STATE + BM * 16 + NW * PB * 4];
  float* s_df = reinterpret_cast<float*>(lds + STATE);   // first positive's distance
  float* s_dmax = s_df + BM;                             // last positive's
  int* s_idf = reinterpret_cast<int*>(s_dmax + BM);      // first positive's global index
  int* s_P = s_idf + BM;                                 // positives (0: the row is skipped)
  float* t = reinterpret_cast<float*>(lds);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int Ptot = a.Ptot;
  // this wave's block of a row's sorted positives, PB floats (+inf past the list)
  float* s_S = reinterpret_cast<float*>(lds + STATE + BM * 16) + wave * PB;
  auto load_block = [&](const float* sd, int P, int p0, float (&S)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int e = p0 + b * 64 + lane;
      S[b] = e < P ? sd[e] : __builtin_huge_valf();
    }
  };

  for (int64_t item = blockIdx.x; item < a.plan.items; item += gridDim.x) {
    const FusedItem it = fused_item(a.plan, item, p.M, BM);
    const int m0 = it.m0, mrem = it.mrem;
    // the state of this wave's rows (only this wave touches it)
    if (lane < RPW) {
      const int row = wave * RPW + lane;
      int P = 0;
      if (row < mrem) {
        const int64_t gr = m0 + row;
        P = min(a.pos_total[gr], Ptot);
        if (P > 0) {
          s_df[row] = a.sorted_d[gr * Ptot];
          s_dmax[row] = a.sorted_d[gr * Ptot + P - 1];
          if (KEY == kBinDist) s_idf[row] = a.sorted_idx[gr * Ptot];
        }
      }
      s_P[row] = P;
    }

    for (int tn = it.t0; tn < it.t1; ++tn) {
      const int n0 = tn * BN;
      f32x4 acc[TM][TN];
      h2_kloop<BM, BN, WM, WN, NS>(p, lds, m0, n0, wave, lane, wm, wn, acc);

#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        const int c0h = hb * BNH;
        fused_park<F>(t, acc, hb, wm, wn, lane);
        // fused_cols written out, with the camera beside the norm and the scale:
        // through the shared piece the 192 x 192 instantiations spill two / one
        // more SGPRs
        bool ok[CS];
        float gn[CS], rb[CS];
        int cam[CS];
        const int nrem = p.Ncol - n0;
#pragma unroll
        for (int j = 0; j < CS; ++j) {
          const int c = j * 64 + lane;
          ok[j] = c < BNH && c0h + c < nrem;
          gn[j] = ok[j] ? p.norm_b[n0 + c0h + c] : 0.f;
          rb[j] = ok[j] ? p.rs_b[n0 + c0h + c] : 0.f;
          if (KEY == kBinKeyCam) cam[j] = ok[j] ? a.gcam[n0 + c0h + c] : 0;
        }
        float Spre[NB];     // row pre_row's first list block, requested a row ahead
        int pre_row = -1;
#pragma unroll
        for (int b = 0; b < NB; ++b) Spre[b] = 0.f;
        for (int i = 0; i < RPW; ++i) {
          const int row = wave * RPW + i;   // wave-uniform
          if (row >= mrem) break;
          const int P = __builtin_amdgcn_readfirstlane(s_P[row]);
          if (P == 0) continue;
          const int64_t gr = m0 + row;
          const float qn = p.norm_a[gr];
          const float ra = p.rs_a[gr];
          const float dmax = uniform_f32(s_dmax[row]);
          const int qc = KEY == kBinKeyCam ? a.qcam[gr] : 0;   // wave-uniform
          float d[CS];
          bool hit[CS];
          int nh = 0;
#pragma unroll
          for (int j = 0; j < CS; ++j) {
            d[j] = fused_cell<F>(p, t, row, j * 64 + lane, ok[j], qn, ra, gn[j], rb[j]);
            hit[j] = ok[j] && d[j] <= dmax;   // d > dmax: ordered after every positive
            if (KEY == kBinKeyCam) hit[j] = hit[j] && cam[j] != qc;
            nh += __popcll(__ballot(hit[j]));
          }
          if (nh == 0) continue;   // nothing of this pass ranks up to the last positive
          if constexpr (KEY == kBinDist) {
            const float df = uniform_f32(s_df[row]);
            const int64_t idf = __builtin_amdgcn_readfirstlane(s_idf[row]);
            int nbef = 0;
#pragma unroll
            for (int j = 0; j < CS; ++j) {
              const int64_t gc = a.g_offset + n0 + c0h + j * 64 + lane;   // global column
              nbef += __popcll(__ballot(hit[j] && (d[j] < df || (d[j] == df && gc < idf))));
            }
            if (nbef && lane == 0) atomicAdd(a.before + gr, nbef);
          }
          const float* sd = a.sorted_d + gr * Ptot;
          int32_t* hq = a.hist + gr * Ptot;
          // the list's first block: requested while the previous row was binned, or now
          float S[NB];
          if (pre_row == row) {
#pragma unroll
            for (int b = 0; b < NB; ++b) S[b] = Spre[b];
          } else {
            load_block(sd, P, 0, S);
          }
          // a row with hits is mostly followed by one (the same columns, the next
          // query): request its first block before this row's rounds
          if (i + 1 < RPW && row + 1 < mrem) {
            const int Pn = __builtin_amdgcn_readfirstlane(s_P[row + 1]);
            if (Pn > 0) {
              load_block(a.sorted_d + (gr + 1) * Ptot, Pn, 0, Spre);
              pre_row = row + 1;
            }
          }
          int done = 0;
          float prev = 0.f;   // the previous block's last distance (p0 > 0)
          for (int p0 = 0;; p0 += PB) {
            if (p0 > 0) load_block(sd, P, p0, S);
#pragma unroll
            for (int b = 0; b < NB; ++b) s_S[b * 64 + lane] = S[b];
            wave_lds_sync();
            const float last = s_S[PB - 1];   // +inf when the list ends inside the block
            int lo[CS];
#pragma unroll
            for (int j = 0; j < CS; ++j) lo[j] = 0;
            // branch-free lower_bound of every column in the block (some entry is
            // >= d for a hit of this block, so the result is below PB)
#pragma unroll
            for (int step = PB / 2; step > 0; step >>= 1)
#pragma unroll
              for (int j = 0; j < CS; ++j)
                if (s_S[lo[j] + step - 1] < d[j]) lo[j] += step;
#pragma unroll
            for (int j = 0; j < CS; ++j) {
              // lower_bound over the whole list falls in [p0, p0 + PB)
              const bool inb = hit[j] && (p0 == 0 || d[j] > prev) && d[j] <= last;
              done += __popcll(__ballot(inb));
              if constexpr (KEY == kBinDist) {
                if (inb) atomicAdd(hq + p0 + lo[j], 1);
              } else if (inb) {
                int b = p0 + lo[j];   // < P: some positive is >= d
                if (s_S[lo[j]] == d[j]) {
                  // the tie group starts at b: go past its members below this column
                  const int gc = (int)(a.g_offset + n0 + c0h + j * 64 + lane);
                  const int32_t* si = a.sorted_idx + gr * Ptot;
                  int hi = P;
                  while (b < hi) {
                    const int mid = (b + hi) >> 1;
                    if (sd[mid] == d[j] && si[mid] < gc) b = mid + 1; else hi = mid;
                  }
                }
                if (b < P) atomicAdd(hq + b, 1);
              }
            }
            prev = last;
            if (done >= nh || p0 + PB >= P) break;
          }
        }
      }
      __syncthreads();  // the parked tile is no longer read: the next K loop may stage
    }
  }
}

// This gallery segment's junk entries were counted like any other column:
// take them back out (rank_count_stream's chunk 0).  One wave per query.
constexpr int kJunkWaves = 4;
__global__ void __launch_bounds__(64 * kJunkWaves)
rank_h2_junk_kernel(int64_t Q, int Ptot, const float* __restrict__ sorted_d,
                    const int32_t* __restrict__ sorted_idx,
                    const int32_t* __restrict__ pos_total, int Jmax,
                    const float* __restrict__ junk_d, const int32_t* __restrict__ junk_idx,
                    const int32_t* __restrict__ junk_cnt, int32_t* __restrict__ hist,
                    int32_t* __restrict__ before) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kJunkWaves + (threadIdx.x >> 6);
  if (q >= Q) return;
  const int P = min(pos_total[q], Ptot);
  if (P <= 0) return;
  const float* sd = sorted_d + q * Ptot;
  const float df = sd[0], dmax = sd[P - 1];
  const int idf = sorted_idx[q * Ptot];
  const int nj = min(junk_cnt[q], Jmax);
  int nb = 0;
  for (int j = lane; j < nj; j += 64) {
    const float d = junk_d[q * Jmax + j];
    if (d <= dmax) {
      int lo = 0, hi = P;   // lower_bound(sd, d) < P
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sd[mid] < d) lo = mid + 1; else hi = mid;
      }
      atomicAdd(hist + q * Ptot + lo, -1);
      nb += (d < df || (d == df && junk_idx[q * Jmax + j] < idf)) ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o);
  if (lane == 0 && nb) atomicAdd(before + q, -nb);
}

// The same for the key bins (cmc_count_kernel's junk loop): an entry leaves
// the bin its own column was counted in, b = #positives with key < (d, index).
__global__ void __launch_bounds__(64 * kJunkWaves)
cmc_h2_junk_kernel(int64_t Q, int Ptot, const float* __restrict__ sorted_d,
                   const int32_t* __restrict__ sorted_idx,
                   const int32_t* __restrict__ pos_total, int Jmax,
                   const float* __restrict__ junk_d, const int32_t* __restrict__ junk_idx,
                   const int32_t* __restrict__ junk_cnt, int32_t* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kJunkWaves + (threadIdx.x >> 6);
  if (q >= Q) return;
  const int P = min(pos_total[q], Ptot);
  if (P <= 0) return;
  const float* sd = sorted_d + q * Ptot;
  const int32_t* si = sorted_idx + q * Ptot;
  const float dmax = sd[P - 1];
  const int nj = min(junk_cnt[q], Jmax);
  for (int j = lane; j < nj; j += 64) {
    const float d = junk_d[q * Jmax + j];
    if (d > dmax) continue;
    const int gi = junk_idx[q * Jmax + j];
    int lo = 0, hi = P;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sd[mid] < d || (sd[mid] == d && si[mid] < gi)) lo = mid + 1; else hi = mid;
    }
    if (lo < P) atomicAdd(hist + q * Ptot + lo, -1);
  }
}

template <int BM, int BN, int WM, int WN, int NS, int KEY>
static int launch_rank_count(const GemmParams& p, const RankH2Args& a, hipStream_t st) {
  hipLaunchKernelGGL((rank_count_h2_kernel<BM, BN, WM, WN, NS, KEY>), dim3(fused_grid(a.plan)),
                     dim3(64 * WM * WN), 0, st, p, a);
  PPS_CHECK_LAUNCH("rank_count_h2_kernel");
  return PPS_OK;
}

// the two tile shapes of one binning mode
template <int KEY>
static int launch_rank_count_tile(int tile, const GemmParams& p, const RankH2Args& a,
                                  hipStream_t st) {
  return tile == 2 ? launch_rank_count<192, 192, 2, 4, 3, KEY>(p, a, st)
                   : launch_rank_count<256, 256, 2, 4, 2, KEY>(p, a, st);
}

// What the two count entries take alike (pps_abi.h), their shared guards and,
// once those passed, the kernel's arguments.
struct CountCall {
  H2Operand q, g;
  int D, metric;
  int64_t g_offset;
  int Ptot;
  const float* sorted_d; const int32_t* sorted_idx; const int32_t* pos_total;
  int segments, tile;
  int32_t* hist;
};
static int rank_count_guards(const char* fn, const CountCall& c) {
  PPS_ENFORCE_AS(fn, c.sorted_d && c.sorted_idx && c.pos_total && c.hist, "null pointer");
  PPS_TRY(h2_operands_guard(fn, c.q, c.g, c.D, c.metric));
  const int Ptot = c.Ptot;
  const int64_t g_offset = c.g_offset, G = c.g.rows;
  PPS_ENFORCE_AS(fn, Ptot > 0, "bad shape");
  PPS_ENFORCE_AS(fn, g_offset >= 0 && g_offset + G < (1ll << 31),
                 "gallery indices must fit int32");
  PPS_TRY(fused_plan_guard(fn, c.segments, c.tile));
  if (c.Ptot > kRankH2MaxP) {
    set_error(std::string(fn) + ": Ptot = " + std::to_string(c.Ptot) +
              " merged positives per query, the fused count takes at most " +
              std::to_string(kRankH2MaxP) + " (pps_rank_count_h2_max_p)");
    return PPS_ERR_CAPACITY;
  }
  return PPS_OK;
}
static void rank_count_plan(const CountCall& c, GemmParams& p, RankH2Args& a) {
  int BM, BN;
  search_tile_shape(c.tile, BM, BN);
  const int64_t Q = c.q.rows, G = c.g.rows;
  a.plan = fused_plan(Q, G, fused_segments(Q, G, c.segments, BM, BN), BM, BN);
  a.g_offset = c.g_offset;
  a.Ptot = c.Ptot;
  a.sorted_d = c.sorted_d; a.sorted_idx = c.sorted_idx; a.pos_total = c.pos_total;
  a.hist = c.hist;
  p = h2_params(c.q, c.g, c.D, c.metric);
}

}  // namespace pps

// ---- C ABI ----------------------------------------------------------------
using namespace pps;

int pps_rank_count_h2_max_p(void) { return kRankH2MaxP; }

int64_t pps_rank_count_h2_workspace_bytes(int64_t Q, int64_t G, int Ptot, int segments) {
  if (Q < 0 || G < 0 || Ptot < 1 || Ptot > kRankH2MaxP || segments < 0) return -1;
  return 0;   // counts go out as atomics: nothing is staged
}

// workspace / ws_bytes: pps_rank_count_h2_workspace_bytes is 0, nothing to check
int pps_rank_count_h2_tiled(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                            const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                            int D, int metric, int64_t g_offset, int Ptot,
                            const float* sorted_d, const int32_t* sorted_idx,
                            const int32_t* pos_total, int Jmax, const float* junk_d,
                            const int32_t* junk_idx, const int32_t* junk_cnt, int segments,
                            int tile, void*, int64_t, int32_t* hist, int32_t* before,
                            void* stream) {
  const CountCall c{h2_operand(q2t, qsq, qrs, Q), h2_operand(g2t, gsq, grs, G), D, metric,
                    g_offset, Ptot, sorted_d, sorted_idx, pos_total, segments, tile, hist};
  PPS_ENFORCE(junk_d && junk_idx && junk_cnt && before, "null pointer");
  PPS_ENFORCE(Jmax > 0, "bad shape");
  PPS_TRY(rank_count_guards(__func__, c));
  if (Q == 0 || G == 0) return PPS_OK;
  hipStream_t st = as_stream(stream);
  GemmParams p{};
  RankH2Args a{};
  rank_count_plan(c, p, a);
  a.before = before;
  PPS_TRY(launch_rank_count_tile<kBinDist>(tile, p, a, st));
  const unsigned grid = (unsigned)((Q + kJunkWaves - 1) / kJunkWaves);
  hipLaunchKernelGGL(rank_h2_junk_kernel, dim3(grid), dim3(64 * kJunkWaves), 0, st, Q, Ptot,
                     sorted_d, sorted_idx, pos_total, Jmax, junk_d, junk_idx, junk_cnt, hist,
                     before);
  PPS_CHECK_LAUNCH("rank_h2_junk_kernel");
  return PPS_OK;
}

int pps_cmc_count_h2_tiled(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                           const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                           int D, int metric, int64_t g_offset, int Ptot,
                           const float* sorted_d, const int32_t* sorted_idx,
                           const int32_t* pos_total, const int32_t* qcam, const int32_t* gcam,
                           int Jmax, const float* junk_d, const int32_t* junk_idx,
                           const int32_t* junk_cnt, int segments, int tile, void*, int64_t,
                           int32_t* hist, void* stream) {
  const CountCall c{h2_operand(q2t, qsq, qrs, Q), h2_operand(g2t, gsq, grs, G), D, metric,
                    g_offset, Ptot, sorted_d, sorted_idx, pos_total, segments, tile, hist};
  PPS_ENFORCE((qcam == nullptr) == (gcam == nullptr),
              "qcam and gcam are given together (separate_camera_set) or not at all");
  PPS_ENFORCE(gcam || (junk_d && junk_idx && junk_cnt && Jmax > 0),
              "without separate_camera_set the junk lists are required");
  PPS_TRY(rank_count_guards(__func__, c));
  if (Q == 0 || G == 0) return PPS_OK;
  hipStream_t st = as_stream(stream);
  GemmParams p{};
  RankH2Args a{};
  rank_count_plan(c, p, a);
  a.qcam = qcam; a.gcam = gcam;
  if (gcam) return launch_rank_count_tile<kBinKeyCam>(tile, p, a, st);
  PPS_TRY(launch_rank_count_tile<kBinKey>(tile, p, a, st));
  const unsigned grid = (unsigned)((Q + kJunkWaves - 1) / kJunkWaves);
  hipLaunchKernelGGL(cmc_h2_junk_kernel, dim3(grid), dim3(64 * kJunkWaves), 0, st, Q, Ptot,
                     sorted_d, sorted_idx, pos_total, Jmax, junk_d, junk_idx, junk_cnt, hist);
  PPS_CHECK_LAUNCH("cmc_h2_junk_kernel");
  return PPS_OK;
}
