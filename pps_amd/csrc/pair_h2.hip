// Distances of listed pairs from the f16x2 planes, and the [M, N] block of
// the general distance kernel for an a operand that is the head of longer
// planes.  Every distance has the bits pps_distmat_h2_tiled would have written
// at that cell: a cell's accumulator depends only on its own two rows and the
// order of the MFMA terms (chunks ascending, mfma_h2t's three terms), and the
// finish is the same expression (h2_finish, h2_fused_common.hpp).
//
// The kernels give one wave to an a-row and take its list 64 entries at a
// time through pair_dots (h2_fused_common.hpp), which hands lane i entry
// m0 + i's dot product:
//   collect_matches_h2_kernel  the list is the query's members (the MatchIndex
//       CSR); the positive / junk split and the compaction are
//       collect_matches' (eval_counts.hip), so rank_prepare / ap_finalize run
//       unchanged after it;
//   pair_dist_h2_kernel        the list is a row of `lists`, the distances go
//       out in list order.  Re-ranking's V-row weights (rerank.hip) are its
//       first user: the distances of every row of x = [queries; gallery] to
//       its few hundred expansion candidates.
//   pair_dist_h2_parts_kernel  the same with the b-rows in two plane sets
//       (queries' planes then the gallery's, never concatenated): re-ranking
//       against a prepared gallery (rerank_prepared).
#include "h2_fused_common.hpp"

namespace pps {

constexpr int kPairWaves = 4;   // a-rows (waves) per workgroup of both kernels

struct MatchArgs {
  const int32_t* qcam; const int32_t* gcam;
  const int32_t* members; const int32_t* q_beg; const int32_t* q_end;
  int64_t g_offset;
  int Pmax, Jmax;
  float* pos_d; int32_t* pos_idx; int32_t* pos_cnt;
  float* junk_d; int32_t* junk_idx; int32_t* junk_cnt;
};

__global__ void __launch_bounds__(64 * kPairWaves)
collect_matches_h2_kernel(PairOperands o, MatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
  if (q >= o.Q) return;   // wave-uniform: every MFMA below runs with all lanes
  const int beg = __builtin_amdgcn_readfirstlane(a.q_beg[q]);
  const int end = __builtin_amdgcn_readfirstlane(a.q_end[q]);
  const int qc = a.qcam[q];
  const int32_t* members = a.members;
  const unsigned char* qa = pair_a_frag(o, (int)q, lane);
  const float qn = o.qsq[q], ra = o.qrs[q];
  GemmParams p{};
  p.metric = o.metric;
  const unsigned long long below = (1ull << lane) - 1ull;
  int np = 0, nj = 0;
  for (int m0 = beg; m0 < end; m0 += 64) {
    const float dot = pair_dots(o, qa, m0, end, lane, [members](int e) { return members[e]; });
    const int m = m0 + lane;
    const bool in = m < end;
    const int idx = in ? members[m] : 0;
    const bool pos = in && a.gcam[idx] != qc;
    const bool junk = in && !pos;
    const float d = in ? h2_finish(p, dot, ra, o.grs[idx], qn, o.gsq[idx]) : 0.f;
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

struct PairDistArgs {
  int G, cap;
  const int32_t* lists;       // [Q][cap]
  const int32_t* counts;      // [Q] or null (cap entries each)
  float* out;                 // [Q][cap]
};

__global__ void __launch_bounds__(64 * kPairWaves)
pair_dist_h2_kernel(PairOperands o, PairDistArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
  if (q >= o.Q) return;   // wave-uniform: every MFMA below runs with all lanes
  int end = a.cap;
  if (a.counts) end = min(max(__builtin_amdgcn_readfirstlane(a.counts[q]), 0), a.cap);
  if (end == 0) return;
  const int32_t* list = a.lists + q * a.cap;
  const unsigned char* qa = pair_a_frag(o, (int)q, lane);
  const float qn = o.qsq[q], ra = o.qrs[q];
  GemmParams p{};
  p.metric = o.metric;
  // an index outside the b operand reads row 0 or G - 1 (no access past the planes)
  auto row_of = [&](int e) { return min(max(list[e], 0), a.G - 1); };
  for (int m0 = 0; m0 < end; m0 += 64) {
    const float dot = pair_dots(o, qa, m0, end, lane, row_of);
    const int m = m0 + lane;
    if (m < end) {
      const int idx = row_of(m);
      a.out[q * a.cap + m] = h2_finish(p, dot, ra, o.grs[idx], qn, o.gsq[idx]);
    }
  }
}

int pair_dist_h2(const H2Operand& q, const H2Operand& g, int D, int metric, const int32_t* lists,
                 const int32_t* counts, int cap, float* out, hipStream_t st) {
  if (q.rows == 0 || g.rows == 0 || cap == 0) return PPS_OK;
  const PairOperands o = pair_operands(q, g, D, metric);
  const PairDistArgs a{(int)g.rows, cap, lists, counts, out};
  const unsigned grid = (unsigned)((q.rows + kPairWaves - 1) / kPairWaves);
  hipLaunchKernelGGL(pair_dist_h2_kernel, dim3(grid), dim3(64 * kPairWaves), 0, st, o, a);
  PPS_CHECK_LAUNCH("pair_dist_h2_kernel");
  return PPS_OK;
}

// pair_dist_h2_kernel with the b-rows in two plane sets (o's b operand holds
// rows [0, B0), p's rows [B0, a.G)): the same walk, the entry's part choosing
// the fragment base, the plane stride and the norm / scale source.
__global__ void __launch_bounds__(64 * kPairWaves)
pair_dist_h2_parts_kernel(PairOperands o, PairPart p, PairDistArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
  if (q >= o.Q) return;   // wave-uniform: every MFMA below runs with all lanes
  int end = a.cap;
  if (a.counts) end = min(max(__builtin_amdgcn_readfirstlane(a.counts[q]), 0), a.cap);
  if (end == 0) return;
  const int32_t* list = a.lists + q * a.cap;
  const unsigned char* qa = pair_a_frag(o, (int)q, lane);
  const float qn = o.qsq[q], ra = o.qrs[q];
  GemmParams gp{};
  gp.metric = o.metric;
  // an index outside [0, B0 + B1) reads row 0 of the first part or the last of the second
  auto row_of = [&](int e) { return min(max(list[e], 0), a.G - 1); };
  for (int m0 = 0; m0 < end; m0 += 64) {
    const float dot = pair_dots_parts(o, p, qa, m0, end, lane, row_of);
    const int m = m0 + lane;
    if (m < end) {
      const int idx = row_of(m);
      const bool second = idx >= p.B0;
      const float* sq = second ? p.gsq : o.gsq;
      const float* rs = second ? p.grs : o.grs;
      const int r = second ? idx - p.B0 : idx;
      a.out[q * a.cap + m] = h2_finish(gp, dot, ra, rs[r], qn, sq[r]);
    }
  }
}

int pair_dist_h2_parts(const H2Operand& q, const H2Operand& b0, const H2Operand& b1, int D,
                       int metric, const int32_t* lists, const int32_t* counts, int cap,
                       float* out, hipStream_t st) {
  if (q.rows == 0 || b0.rows + b1.rows == 0 || cap == 0) return PPS_OK;
  // an empty part is never addressed: the clamp keeps every index in the other
  const PairOperands o = pair_operands(q, b0, D, metric);
  PairPart p{};
  p.g2t = reinterpret_cast<const unsigned char*>(b1.planes);
  p.g_plane = h2_plane_elems(b1.plane_rows, D) * 2;
  p.gsq = b1.sq; p.grs = b1.rs;
  p.B0 = (int)b0.rows;
  const PairDistArgs a{(int)(b0.rows + b1.rows), cap, lists, counts, out};
  const unsigned grid = (unsigned)((q.rows + kPairWaves - 1) / kPairWaves);
  hipLaunchKernelGGL(pair_dist_h2_parts_kernel, dim3(grid), dim3(64 * kPairWaves), 0, st, o, p, a);
  PPS_CHECK_LAUNCH("pair_dist_h2_parts_kernel");
  return PPS_OK;
}

// pps_distmat_h2_tiled's launch with the a planes' own plane stride
int distmat_h2_head(const H2Operand& a, const H2Operand& b, int D, int metric, float* out,
                    int64_t ldo, hipStream_t st) {
  if (a.rows == 0 || b.rows == 0) return PPS_OK;
  return launch_gemm_h2(h2_params(a, b, D, metric, out, ldo), st, 0);
}

}  // namespace pps

// ---- C ABI ----------------------------------------------------------------
using namespace pps;

int pps_collect_matches_h2(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                           const uint16_t* g2t, const float* gsq, const float* grs, int64_t G,
                           int D, int metric, const int32_t* qcam, const int32_t* gcam,
                           const int32_t* members, const int32_t* q_beg, const int32_t* q_end,
                           int64_t g_offset, int Pmax, float* pos_d, int32_t* pos_idx,
                           int32_t* pos_cnt, int Jmax, float* junk_d, int32_t* junk_idx,
                           int32_t* junk_cnt, void* stream) {
  const H2Operand q = h2_operand(q2t, qsq, qrs, Q), g = h2_operand(g2t, gsq, grs, G);
  PPS_ENFORCE(qcam && gcam && members && q_beg && q_end && pos_d && pos_idx && pos_cnt &&
                  junk_d && junk_idx && junk_cnt,
              "null pointer");
  PPS_TRY(h2_operands_guard(__func__, q, g, D, metric));
  PPS_ENFORCE(Pmax > 0 && Jmax > 0, "bad shape");
  PPS_ENFORCE(g_offset >= 0 && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  if (Q == 0) return PPS_OK;
  // an empty gallery still writes every query's zero counts
  PPS_ENFORCE(q.complete(), "null pointer");
  PPS_ENFORCE(aligned16(q2t) && aligned16(g2t), "planes must be 16-byte aligned");
  const PairOperands o = pair_operands(q, g, D, metric);
  const MatchArgs a{qcam, gcam, members, q_beg, q_end, g_offset, Pmax, Jmax, pos_d, pos_idx,
                    pos_cnt, junk_d, junk_idx, junk_cnt};
  const unsigned grid = (unsigned)((Q + kPairWaves - 1) / kPairWaves);
  hipLaunchKernelGGL(collect_matches_h2_kernel, dim3(grid), dim3(64 * kPairWaves), 0,
                     as_stream(stream), o, a);
  PPS_CHECK_LAUNCH("collect_matches_h2_kernel");
  return PPS_OK;
}

int pps_pair_dist_h2(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                     const uint16_t* g2t, const float* gsq, const float* grs, int64_t G, int D,
                     int metric, const int32_t* lists, const int32_t* counts, int cap, float* out,
                     void* stream) {
  const H2Operand q = h2_operand(q2t, qsq, qrs, Q), g = h2_operand(g2t, gsq, grs, G);
  PPS_ENFORCE(lists && out, "null pointer");
  PPS_TRY(h2_operands_guard(__func__, q, g, D, metric));
  PPS_ENFORCE(G < (1ll << 31), "Q and G must fit int32");
  PPS_ENFORCE(cap >= 1, "cap must be >= 1");
  if (Q == 0) return PPS_OK;
  PPS_ENFORCE(G > 0, "a listed pair needs a b-row (G > 0)");
  return pair_dist_h2(q, g, D, metric, lists, counts, cap, out, as_stream(stream));
}

int pps_pair_dist_h2_parts(const uint16_t* q2t, int64_t Q, const float* qsq, const float* qrs,
                           const uint16_t* b0_2t, const float* b0sq, const float* b0rs, int64_t B0,
                           const uint16_t* b1_2t, const float* b1sq, const float* b1rs, int64_t B1,
                           int D, int metric, const int32_t* lists, const int32_t* counts, int cap,
                           float* out, void* stream) {
  const H2Operand q = h2_operand(q2t, qsq, qrs, Q);
  const H2Operand b0 = h2_operand(b0_2t, b0sq, b0rs, B0), b1 = h2_operand(b1_2t, b1sq, b1rs, B1);
  PPS_ENFORCE(lists && out, "null pointer");
  PPS_TRY(h2_operands_guard(__func__, q, b0, D, metric));
  PPS_TRY(h2_operands_guard(__func__, q, b1, D, metric));
  PPS_ENFORCE(B0 + B1 < (1ll << 31), "B0 + B1 must fit int32");
  PPS_ENFORCE(cap >= 1, "cap must be >= 1");
  if (Q == 0) return PPS_OK;
  PPS_ENFORCE(B0 > 0 && B1 > 0, "a listed pair needs a b-row in each part (B0, B1 > 0)");
  return pair_dist_h2_parts(q, b0, b1, D, metric, lists, counts, cap, out, as_stream(stream));
}
