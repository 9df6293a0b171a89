// Pair distances from the f16x2 planes: out[r][t] = the distance of a-row r to
// b-row lists[r][t] for the listed pairs only, each with the bits
// pps_distmat_h2_tiled would have written at that cell (a cell's accumulator
// depends only on its own two rows and the order of the MFMA terms -- chunks
// ascending, mfma_h2t's three terms -- and the finish is the same expression,
// dist_value(p, (acc * rs_a) * rs_b, qn, gn)).
//
// collect_matches_h2_kernel's scheme (rank_h2.hip) without the positive / junk
// split: one wave per a-row, its list taken 64 entries at a time as four blocks
// of 16 MFMA columns, fragments loaded straight from the tiled planes in
// global memory, one cross-lane move handing lane i entry m0 + i's dot product.
// Re-ranking's V-row weights (rerank.hip) are its first user: the distances of
// every row of x = [queries; gallery] to its few hundred expansion candidates.
#include "gemm_h2_common.hpp"
#include "retrieval.hpp"

namespace pps {

constexpr int kPairDistWaves = 4;

struct PairDistArgs {
  const unsigned char* q2t;   // planes as bytes
  const unsigned char* g2t;
  int64_t q_plane, g_plane;   // bytes between an operand's two planes
  const float* qsq; const float* qrs;
  const float* gsq; const float* grs;
  int64_t Q;
  int G, nkc, metric, cap;
  const int32_t* lists;       // [Q][cap]
  const int32_t* counts;      // [Q] or null (cap entries each)
  float* out;                 // [Q][cap]
};

__global__ void __launch_bounds__(64 * kPairDistWaves)
pair_dist_h2_kernel(PairDistArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kPairDistWaves + (threadIdx.x >> 6);
  if (q >= a.Q) return;   // wave-uniform: every MFMA below runs with all lanes
  int end = a.cap;
  if (a.counts) end = min(max(__builtin_amdgcn_readfirstlane(a.counts[q]), 0), a.cap);
  if (end == 0) return;
  const int32_t* list = a.lists + q * a.cap;
  const int r16 = lane & 15, slot = lane >> 4;
  const unsigned char* qa = a.q2t + h2_frag_off((int)q, a.nkc, slot);
  const float qn = a.qsq[q], ra = a.qrs[q];
  GemmParams p{};
  p.metric = a.metric;
  // an index outside the b operand reads row 0 or G - 1 (no access past the planes)
  auto row_of = [&](int e) { return min(max(list[e], 0), a.G - 1); };
  // lane i's entry sits in block i >> 4, column i & 15: register i & 3 of the
  // lanes 16 ((i & 15) >> 2) + r, any r.  Every lane picks register
  // (r >> 2, r & 3) of its own; lane i then reads lane
  // 16 ((i & 15) >> 2) + 4 (i >> 4) + (i & 3).
  const int src = 16 * ((lane & 15) >> 2) + 4 * (lane >> 4) + (lane & 3);
  for (int m0 = 0; m0 < end; m0 += 64) {
    const int nb = min(4, (end - m0 + 15) >> 4);   // blocks with an entry (wave-uniform)
    const unsigned char* ga[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      // columns past the list repeat its last entry (their cells are not read)
      const int mi = min(m0 + 16 * b + r16, end - 1);
      ga[b] = a.g2t + h2_frag_off(row_of(mi), a.nkc, slot);
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
    if (m < end) {
      const int idx = row_of(m);
      // two exact power-of-two scalings, row scale first (h2_dist_epilogue)
      a.out[q * a.cap + m] = dist_value(p, (dot * ra) * a.grs[idx], qn, a.gsq[idx]);
    }
  }
}

int pair_dist_h2(const uint16_t* q2t, int64_t Q, int64_t Qrows, const float* qsq, const float* qrs,
                 const uint16_t* g2t, const float* gsq, const float* grs, int64_t G, int D,
                 int metric, const int32_t* lists, const int32_t* counts, int cap, float* out,
                 hipStream_t st) {
  if (Q == 0 || G == 0 || cap == 0) return PPS_OK;
  const int64_t Qp = (Qrows + 15) / 16 * 16, Gp = (G + 15) / 16 * 16;
  PairDistArgs a{};
  a.q2t = reinterpret_cast<const unsigned char*>(q2t);
  a.g2t = reinterpret_cast<const unsigned char*>(g2t);
  a.q_plane = Qp * D * 2;
  a.g_plane = Gp * D * 2;
  a.qsq = qsq; a.qrs = qrs; a.gsq = gsq; a.grs = grs;
  a.Q = Q;
  a.G = (int)G;
  a.nkc = D / 32;
  a.metric = metric;
  a.cap = cap;
  a.lists = lists; a.counts = counts; a.out = out;
  const unsigned grid = (unsigned)((Q + kPairDistWaves - 1) / kPairDistWaves);
  hipLaunchKernelGGL(pair_dist_h2_kernel, dim3(grid), dim3(64 * kPairDistWaves), 0, st, a);
  PPS_CHECK_LAUNCH("pair_dist_h2_kernel");
  return PPS_OK;
}

// The [M, G] block of distances of the first M rows of an a operand holding
// Arows rows against a whole b operand: pps_distmat_h2_tiled's launch with the
// a planes' own plane stride (a cell's bits do not depend on the rows around it)
int distmat_h2_head(const uint16_t* a2t, int64_t M, int64_t Arows, const float* asq,
                    const float* ars, const uint16_t* b2t, const float* bsq, const float* brs,
                    int64_t N, int D, int metric, float* out, int64_t ldo, hipStream_t st) {
  if (M == 0 || N == 0) return PPS_OK;
  const int64_t Ap = (Arows + 15) / 16 * 16, Np = (N + 15) / 16 * 16;
  GemmParams p{};
  p.splitk = 1;
  p.tiled = 3;
  p.a3 = a2t; p.a_plane = Ap * D; p.a_bytes = (uint32_t)(2 * Ap * D * 2);
  p.M = (int)M;
  p.b3 = b2t; p.b_plane = Np * D; p.b_bytes = (uint32_t)(2 * Np * D * 2);
  p.Ncol = (int)N;
  p.Kloop = D;
  p.norm_a = asq; p.norm_b = bsq;
  p.rs_a = ars; p.rs_b = brs;
  p.out = out; p.ldo = ldo; p.metric = metric; p.sym = 0;
  return launch_gemm_h2(p, st, 0);
}

}  // namespace pps

// ---- C ABI ----------------------------------------------------------------
using namespace pps;

int pps_pair_dist_h2(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                     const uint16_t* g2t, const float* gsq, const float* grs, int64_t G, int D,
                     int metric, const int32_t* lists, const int32_t* counts, int cap, float* out,
                     void* stream) {
  PPS_ENFORCE(lists && out, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0 && D % 32 == 0, "bad shape (D % 32 == 0)");
  PPS_ENFORCE(Q < (1ll << 31) && G < (1ll << 31), "Q and G must fit int32");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(2 * ((Q + 15) / 16 * 16) * D * 2 < kMaxBufBytes &&
                  2 * ((G + 15) / 16 * 16) * D * 2 < kMaxBufBytes,
              "planes over 2 GiB");
  PPS_ENFORCE(cap >= 1, "cap must be >= 1");
  if (Q == 0) return PPS_OK;
  PPS_ENFORCE(G > 0, "a listed pair needs a b-row (G > 0)");
  PPS_ENFORCE(q2t && qsq && qrs && g2t && gsq && grs, "null pointer");
  PPS_ENFORCE(aligned16(q2t) && aligned16(g2t), "planes must be 16-byte aligned");
  return pair_dist_h2(q2t, Q, Q, qsq, qrs, g2t, gsq, grs, G, D, metric, lists, counts, cap, out,
                      as_stream(stream));
}
