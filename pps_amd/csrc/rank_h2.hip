// Matrix-free rank counts ("fused mAP"): the two kernels of the count-based
// evaluation that read the [Q, G] distance matrix (eval_counts.hip:
// collect_matches, rank_count_stream), each with a twin that computes the
// f16x2 distances on the fly from the operands' chunk-tiled planes.  Every
// distance has the bits pps_distmat_h2_tiled would have written -- a cell's
// accumulator depends only on its own query row, its own gallery row and the
// order of the MFMA terms (chunks ascending, mfma_h2t's three terms), and the
// finish is the same expression, dist_value(p, (acc * rs_a) * rs_b, qn, gn) --
// so the lists and counts equal the materialised path's exactly and
// rank_prepare / ap_finalize run unchanged between and after the two.
//
// a) collect_matches_h2: one wave per query.  Its members (the MatchIndex
//    CSR) are taken 64 at a time as four blocks of 16 MFMA columns; per K
//    chunk each lane loads its 16-byte fragments straight from the tiled
//    planes in global memory (the member's row and the query's row, slot
//    lane >> 4, both planes; no LDS staging).  All 16 query rows of the MFMA
//    are the one query, so every lane group holds a copy of the block's 16
//    dot products; one cross-lane move hands lane i member m0 + i's, and the
//    positive / junk split and the compaction are collect_matches'.
//
// b) rank_count_h2: search_h2_kernel's skeleton (work item = query panel x
//    gallery segment, workgroups striding over the items, h2_kloop per tile,
//    accumulators parked in LDS, each wave finishing BM / 8 rows) with a
//    counting epilogue in place of the candidate filter.  A row's first and
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
// c) cmc_count_h2 (the fractional and the separate-camera CMC): b)'s kernel
//    with cmc_count_kernel's key bins in place of the distance bins (its KEY
//    parameter, described at kBinDist below) -- pps_cmc_counts on the h2
//    matrix, exactly; pps_cmc_finalize runs unchanged after it.
//
// No workgroup waits on another; nothing is launched cooperatively.
#include <algorithm>

#include "gemm_h2_common.hpp"
#include "retrieval.hpp"
#include "topk_wave_common.hpp"

namespace pps {

// ---- a) matches' distances ----------------------------------------------------
constexpr int kPairWaves = 4;

struct PairArgs {
  const unsigned char* q2t;   // planes as bytes
  const unsigned char* g2t;
  int64_t q_plane, g_plane;   // bytes between an operand's two planes
  const float* qsq; const float* qrs;
  const float* gsq; const float* grs;
  int64_t Q;
  int nkc, metric;
  const int32_t* qcam; const int32_t* gcam;
  const int32_t* members; const int32_t* q_beg; const int32_t* q_end;
  int64_t g_offset;
  int Pmax, Jmax;
  float* pos_d; int32_t* pos_idx; int32_t* pos_cnt;
  float* junk_d; int32_t* junk_idx; int32_t* junk_cnt;
};

// h2_frag_off (a row's fragment in a chunk-tiled plane): retrieval.hpp

__global__ void __launch_bounds__(64 * kPairWaves)
collect_matches_h2_kernel(PairArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
  if (q >= a.Q) return;   // wave-uniform: every MFMA below runs with all lanes
  const int beg = __builtin_amdgcn_readfirstlane(a.q_beg[q]);
  const int end = __builtin_amdgcn_readfirstlane(a.q_end[q]);
  const int qc = a.qcam[q];
  const int r16 = lane & 15, slot = lane >> 4;
  const unsigned char* qa = a.q2t + h2_frag_off((int)q, a.nkc, slot);
  const float qn = a.qsq[q], ra = a.qrs[q];
  GemmParams p{};
  p.metric = a.metric;
  // lane i's member sits in block i >> 4, column i & 15: register i & 3 of the
  // lanes 16 ((i & 15) >> 2) + r, any r.  Every lane picks register
  // (r >> 2, r & 3) of its own; lane i then reads lane
  // 16 ((i & 15) >> 2) + 4 (i >> 4) + (i & 3).
  const int src = 16 * ((lane & 15) >> 2) + 4 * (lane >> 4) + (lane & 3);
  const unsigned long long below = (1ull << lane) - 1ull;
  int np = 0, nj = 0;
  for (int m0 = beg; m0 < end; m0 += 64) {
    const int nb = min(4, (end - m0 + 15) >> 4);   // blocks with a member (wave-uniform)
    const unsigned char* ga[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      // columns past the list repeat its last member (their cells are not read)
      const int mi = min(m0 + 16 * b + r16, end - 1);
      ga[b] = a.g2t + h2_frag_off(a.members[mi], a.nkc, slot);
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
          const f16x8 g1 = *reinterpret_cast<const f16x8*>(ga[b] + a.g_plane + ko);
          acc[b] = mfma_h2t(q0, q1, g0, g1, acc[b]);
        }
      }
    }
    const int rb4 = r16 >> 2, re = lane & 3;
    const f32x4 t = rb4 == 0 ? acc[0] : rb4 == 1 ? acc[1] : rb4 == 2 ? acc[2] : acc[3];
    const float mine = re == 0 ? t[0] : re == 1 ? t[1] : re == 2 ? t[2] : t[3];
    const float dot = __shfl(mine, src);

    const int m = m0 + lane;
    const bool in = m < end;
    const int idx = in ? a.members[m] : 0;
    const bool pos = in && a.gcam[idx] != qc;
    const bool junk = in && !pos;
    // two exact power-of-two scalings, row scale first (h2_dist_epilogue)
    const float d = in ? dist_value(p, (dot * ra) * a.grs[idx], qn, a.gsq[idx]) : 0.f;
    const unsigned long long bp = __ballot(pos), bj = __ballot(junk);
    const int sp = np + __popcll(bp & below), sj = nj + __popcll(bj & below);
    if (pos && sp < a.Pmax) {
      a.pos_d[q * a.Pmax + sp] = d;
      a.pos_idx[q * a.Pmax + sp] = (int32_t)(a.g_offset + idx);
    }
    if (junk && sj < a.Jmax) {
      a.junk_d[q * a.Jmax + sj] = d;
      a.junk_idx[q * a.Jmax + sj] = (int32_t)(a.g_offset + idx);
    }
    np += __popcll(bp);
    nj += __popcll(bj);
  }
  if (lane == 0) {
    a.pos_cnt[q] = np;
    a.junk_cnt[q] = nj;
  }
}

// ---- b) fused distance + rank counts --------------------------------------------
struct RankH2Args {
  int S, tps, tiles_n;            // segments, gallery tiles per segment, gallery tiles
  int64_t items;                  // panels * S
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
  using T = H2Tile<BM, BN, WM, WN, NS>;
  constexpr int NW = T::NW, TM = T::TM, TN = T::TN, HB = T::HB;
  constexpr int WCOLS = BN / WN;
  constexpr int BNH = BN / HB, LD = BNH + 4;
  constexpr int RPW = BM / NW;             // rows a wave finishes
  constexpr int CS = (BNH + 63) / 64;      // columns per lane and pass
  static_assert(BM % NW == 0 && RPW <= 64, "rows per wave");
  static_assert(BNH % WCOLS == 0, "a wave's columns fall in one pass");
  constexpr int STATE = T::LDS_BYTES;      // row state beside the stages / the parked tile
  constexpr int NB = 4, PB = 64 * NB;      // positives binned per round: NB registers a lane
  static_assert(STATE % 16 == 0 && STATE + BM * 16 + NW * PB * 4 <= kLdsBytesGfx950, "LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[STATE + BM * 16 + NW * PB * 4];
  float* s_df = reinterpret_cast<float*>(lds + STATE);   // first positive's distance
  float* s_dmax = s_df + BM;                             // last positive's
  int* s_idf = reinterpret_cast<int*>(s_dmax + BM);      // first positive's global index
  int* s_P = s_idf + BM;                                 // positives (0: the row is skipped)
  float* t = reinterpret_cast<float*>(lds);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int r16 = lane & 15, h = lane >> 4;
  const int wc0 = wn * WCOLS;
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

  for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int panel = (int)(item / a.S), s = (int)(item - (int64_t)panel * a.S);
    const int m0 = panel * BM;
    const int mrem = p.M - m0;
    const int t0 = s * a.tps, t1 = min(t0 + a.tps, a.tiles_n);
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

    for (int tn = t0; tn < t1; ++tn) {
      const int n0 = tn * BN;
      const int nrem = p.Ncol - n0;
      f32x4 acc[TM][TN];
      h2_kloop<BM, BN, WM, WN, NS>(p, lds, m0, n0, wave, lane, wm, wn, acc);

#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        const int c0h = hb * BNH;
        __syncthreads();  // the stages / the previous pass are no longer read
        if (wc0 >= c0h && wc0 < c0h + BNH) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const int row = wm * (BM / WM) + i * 16 + r16;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const int col = wc0 - c0h + j * 16 + 4 * h;
              *reinterpret_cast<f32x4*>(t + row * LD + col) = acc[i][j];
            }
          }
        }
        __syncthreads();
        // this lane's columns of the pass: norms and scales once for all rows
        bool ok[CS];
        float gn[CS], rb[CS];
        int cam[CS];
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
            const int c = j * 64 + lane;
            // two exact power-of-two scalings, row scale first (h2_dist_epilogue)
            const float dot = ok[j] ? t[row * LD + c] : 0.f;
            d[j] = dist_value(p, (dot * ra) * rb[j], qn, gn[j]);
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
  const int64_t grid = std::min<int64_t>(a.items, kSearchSlots);
  hipLaunchKernelGGL((rank_count_h2_kernel<BM, BN, WM, WN, NS, KEY>), dim3((unsigned)grid),
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

// The plan and the operands the two count entries share (their guards passed).
static void rank_count_plan(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                            const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                            int D, int metric, int64_t g_offset, int Ptot,
                            const float* sorted_d, const int32_t* sorted_idx,
                            const int32_t* pos_total, int segments, int tile, int32_t* hist,
                            GemmParams& p, RankH2Args& a) {
  int BM, BN;
  search_tile_shape(tile, BM, BN);
  const int64_t Qp = (Q + 15) / 16 * 16, Gp = (G + 15) / 16 * 16;
  const int64_t panels = cdiv(Q, BM), tiles_n = cdiv(G, BN);
  const int64_t S0 = fused_segments(Q, G, segments, BM, BN);
  a.tiles_n = (int)tiles_n;
  a.tps = (int)cdiv(tiles_n, S0);
  a.S = (int)cdiv(tiles_n, a.tps);   // no empty segment
  a.items = panels * a.S;
  a.g_offset = g_offset;
  a.Ptot = Ptot;
  a.sorted_d = sorted_d; a.sorted_idx = sorted_idx; a.pos_total = pos_total;
  a.hist = hist;

  p.splitk = 1;
  p.tiled = 3;
  p.a3 = q2t; p.a_plane = Qp * D; p.a_bytes = (uint32_t)(2 * Qp * D * 2);
  p.M = (int)Q;
  p.b3 = g2t; p.b_plane = Gp * D; p.b_bytes = (uint32_t)(2 * Gp * D * 2);
  p.Ncol = (int)G;
  p.Kloop = D;
  p.norm_a = qsq; p.norm_b = gsq;
  p.rs_a = qrs; p.rs_b = grs;
  p.metric = metric;
}

// the checks the planes arguments share with pps_search_h2_tiled (same texts)
#define PPS_ENFORCE_H2_PLANES(Q, G, D, metric)                                              \
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0 && D % 32 == 0, "bad shape (D % 32 == 0)");         \
  PPS_ENFORCE(Q < (1ll << 31), "Q must fit int32");                                         \
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");                                \
  PPS_ENFORCE(2 * ((Q + 15) / 16 * 16) * D * 2 < kMaxBufBytes &&                            \
                  2 * ((G + 15) / 16 * 16) * D * 2 < kMaxBufBytes,                          \
              "planes over 2 GiB")

}  // namespace pps

// ---- C ABI ----------------------------------------------------------------
using namespace pps;

int pps_rank_count_h2_max_p(void) { return kRankH2MaxP; }

int64_t pps_rank_count_h2_workspace_bytes(int64_t Q, int64_t G, int Ptot, int segments) {
  if (Q < 0 || G < 0 || Ptot < 1 || Ptot > kRankH2MaxP || segments < 0) return -1;
  return 0;   // counts go out as atomics: nothing is staged
}

int pps_collect_matches_h2(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                           const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                           int D, int metric, const int32_t* qcam, const int32_t* gcam,
                           const int32_t* members, const int32_t* q_beg, const int32_t* q_end,
                           int64_t g_offset, int Pmax, float* pos_d, int32_t* pos_idx,
                           int32_t* pos_cnt, int Jmax, float* junk_d, int32_t* junk_idx,
                           int32_t* junk_cnt, void* stream) {
  PPS_ENFORCE(qcam && gcam && members && q_beg && q_end && pos_d && pos_idx && pos_cnt &&
                  junk_d && junk_idx && junk_cnt,
              "null pointer");
  PPS_ENFORCE_H2_PLANES(Q, G, D, metric);
  PPS_ENFORCE(Pmax > 0 && Jmax > 0, "bad shape");
  PPS_ENFORCE(g_offset >= 0 && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  if (Q == 0) return PPS_OK;
  PPS_ENFORCE(q2t && qsq && qrs && (G == 0 || (g2t && gsq && grs)), "null pointer");
  PPS_ENFORCE(aligned16(q2t) && aligned16(g2t), "planes must be 16-byte aligned");
  const int64_t Qp = (Q + 15) / 16 * 16, Gp = (G + 15) / 16 * 16;
  PairArgs a{};
  a.q2t = reinterpret_cast<const unsigned char*>(q2t);
  a.g2t = reinterpret_cast<const unsigned char*>(g2t);
  a.q_plane = Qp * D * 2;
  a.g_plane = Gp * D * 2;
  a.qsq = qsq; a.qrs = qrs; a.gsq = gsq; a.grs = grs;
  a.Q = Q;
  a.nkc = D / 32;
  a.metric = metric;
  a.qcam = qcam; a.gcam = gcam; a.members = members; a.q_beg = q_beg; a.q_end = q_end;
  a.g_offset = g_offset;
  a.Pmax = Pmax; a.Jmax = Jmax;
  a.pos_d = pos_d; a.pos_idx = pos_idx; a.pos_cnt = pos_cnt;
  a.junk_d = junk_d; a.junk_idx = junk_idx; a.junk_cnt = junk_cnt;
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)((Q + kPairWaves - 1) / kPairWaves);
  hipLaunchKernelGGL(collect_matches_h2_kernel, dim3(grid), dim3(64 * kPairWaves), 0, st, a);
  PPS_CHECK_LAUNCH("collect_matches_h2_kernel");
  return PPS_OK;
}

int pps_rank_count_h2_tiled(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                            const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                            int D, int metric, int64_t g_offset, int Ptot,
                            const float* sorted_d, const int32_t* sorted_idx,
                            const int32_t* pos_total, int Jmax, const float* junk_d,
                            const int32_t* junk_idx, const int32_t* junk_cnt, int segments,
                            int tile, void* workspace, int64_t ws_bytes, int32_t* hist,
                            int32_t* before, void* stream) {
  PPS_ENFORCE(sorted_d && sorted_idx && pos_total && junk_d && junk_idx && junk_cnt && hist &&
                  before,
              "null pointer");
  PPS_ENFORCE_H2_PLANES(Q, G, D, metric);
  PPS_ENFORCE(Ptot > 0 && Jmax > 0, "bad shape");
  PPS_ENFORCE(g_offset >= 0 && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  PPS_ENFORCE(segments >= 0, "segments must be >= 0 (0 = auto)");
  PPS_ENFORCE(tile >= 0 && tile < kSearchNumTiles,
              "search tile must be 0.." + std::to_string(kSearchNumTiles - 1));
  if (Ptot > kRankH2MaxP) {
    set_error("pps_rank_count_h2_tiled: Ptot = " + std::to_string(Ptot) +
              " merged positives per query, the fused count takes at most " +
              std::to_string(kRankH2MaxP) + " (pps_rank_count_h2_max_p)");
    return PPS_ERR_CAPACITY;
  }
  (void)workspace;   // pps_rank_count_h2_workspace_bytes is 0: nothing to check
  (void)ws_bytes;
  if (Q == 0 || G == 0) return PPS_OK;
  PPS_ENFORCE(q2t && qsq && qrs && g2t && gsq && grs, "null pointer");
  PPS_ENFORCE(aligned16(q2t) && aligned16(g2t), "planes must be 16-byte aligned");
  hipStream_t st = as_stream(stream);

  GemmParams p{};
  RankH2Args a{};
  rank_count_plan(q2t, Q, qsq, qrs, g2t, gsq, grs, G, D, metric, g_offset, Ptot, sorted_d,
                  sorted_idx, pos_total, segments, tile, hist, p, a);
  a.before = before;
  const int rc = launch_rank_count_tile<kBinDist>(tile, p, a, st);
  if (rc != PPS_OK) return rc;
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
                           const int32_t* junk_cnt, int segments, int tile,
                           void* workspace, int64_t ws_bytes, int32_t* hist, void* stream) {
  PPS_ENFORCE(sorted_d && sorted_idx && pos_total && hist, "null pointer");
  PPS_ENFORCE((qcam == nullptr) == (gcam == nullptr),
              "qcam and gcam are given together (separate_camera_set) or not at all");
  PPS_ENFORCE(gcam || (junk_d && junk_idx && junk_cnt && Jmax > 0),
              "without separate_camera_set the junk lists are required");
  PPS_ENFORCE_H2_PLANES(Q, G, D, metric);
  PPS_ENFORCE(Ptot > 0, "bad shape");
  PPS_ENFORCE(g_offset >= 0 && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  PPS_ENFORCE(segments >= 0, "segments must be >= 0 (0 = auto)");
  PPS_ENFORCE(tile >= 0 && tile < kSearchNumTiles,
              "search tile must be 0.." + std::to_string(kSearchNumTiles - 1));
  if (Ptot > kRankH2MaxP) {
    set_error("pps_cmc_count_h2_tiled: Ptot = " + std::to_string(Ptot) +
              " merged positives per query, the fused count takes at most " +
              std::to_string(kRankH2MaxP) + " (pps_rank_count_h2_max_p)");
    return PPS_ERR_CAPACITY;
  }
  (void)workspace;   // pps_rank_count_h2_workspace_bytes is 0: nothing to check
  (void)ws_bytes;
  if (Q == 0 || G == 0) return PPS_OK;
  PPS_ENFORCE(q2t && qsq && qrs && g2t && gsq && grs, "null pointer");
  PPS_ENFORCE(aligned16(q2t) && aligned16(g2t), "planes must be 16-byte aligned");
  hipStream_t st = as_stream(stream);

  GemmParams p{};
  RankH2Args a{};
  rank_count_plan(q2t, Q, qsq, qrs, g2t, gsq, grs, G, D, metric, g_offset, Ptot, sorted_d,
                  sorted_idx, pos_total, segments, tile, hist, p, a);
  a.qcam = qcam; a.gcam = gcam;
  if (gcam) return launch_rank_count_tile<kBinKeyCam>(tile, p, a, st);
  const int rc = launch_rank_count_tile<kBinKey>(tile, p, a, st);
  if (rc != PPS_OK) return rc;
  const unsigned grid = (unsigned)((Q + kJunkWaves - 1) / kJunkWaves);
  hipLaunchKernelGGL(cmc_h2_junk_kernel, dim3(grid), dim3(64 * kJunkWaves), 0, st, Q, Ptot,
                     sorted_d, sorted_idx, pos_total, Jmax, junk_d, junk_idx, junk_cnt, hist);
  PPS_CHECK_LAUNCH("cmc_h2_junk_kernel");
  return PPS_OK;
}
