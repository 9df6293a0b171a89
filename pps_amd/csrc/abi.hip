// extern "C" entry points of libpps_hip.so (declared in include/pps_abi.h).
// Each entry point validates shapes/alignment ENFORCE-style, fills the
// launch parameters and enqueues on the caller's stream.  No allocation, no
// synchronisation: every entry point is hipGraph-capturable.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "retrieval.hpp"

namespace pps {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
bool debug_sync() {
  static const bool on = [] {
    const char* e = getenv("PPS_DEBUG_SYNC");
    return e && e[0] == '1';
  }();
  return on;
}

}  // namespace pps

using namespace pps;

extern "C" {

int pps_abi_version(void) { return 1; }

const char* pps_last_error(void) { return g_last_error.c_str(); }

const char* pps_registered_ops(void) {
  // the reference's Caffe2 op names of the test net (pps_amd/net.py OPS) and
  // the fused / retrieval entry points the product path runs
  return "Conv;SpatialBN;Relu;Sum;Add;Max;Mean;MaxPool;AveragePool;Split;FC;Concat;"
         "Reshape;Normalize;PairWiseDistance;"
         "Conv+SpatialBN+Sum+Relu;PartPowerSet;ComputeDist;RankCounts;CMC;TopK;TopKMerge;"
         "ReRanking;PrepImForBlob";
}

int pps_gemm_num_tiles(void) { return GEMM_NUM_TILES - 1; }

int pps_distmat(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                int64_t ldg, int D, int metric, float* out, int64_t ldo, int tile,
                void* stream) {
  PPS_ENFORCE(q && g && out, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0, "bad shape");
  PPS_ENFORCE(D % 4 == 0, "D must be a multiple of 4, got " + std::to_string(D));
  PPS_ENFORCE(ldq % 4 == 0 && ldg % 4 == 0 && ldq >= D && ldg >= D, "bad leading dims");
  PPS_ENFORCE(ldo >= G, "ldo < G");
  PPS_ENFORCE(aligned16(q) && aligned16(g), "q/g must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(ldq * 4 < kMaxBufBytes && ldg * 4 < kMaxBufBytes, "rows too long");
  // operands are addressed through 32-bit buffer offsets: split Q and G into
  // blocks of < 2 GiB each (one launch per block pair, same results)
  const int64_t qblk = std::min<int64_t>(Q, (kMaxBufBytes - 1) / (ldq * 4));
  const int64_t gblk = std::min<int64_t>(G, (kMaxBufBytes - 1) / (ldg * 4));
  for (int64_t q0 = 0; q0 < Q; q0 += qblk) {
    for (int64_t g0 = 0; g0 < G; g0 += gblk) {
      const int64_t qn = std::min(qblk, Q - q0), gn = std::min(gblk, G - g0);
      GemmParams p{};
  p.splitk = 1;
      p.a = q + q0 * ldq; p.a_bytes = (uint32_t)(qn * ldq * 4);
      p.H = 1; p.W = (int)qn; p.Cin = D; p.lda = (int)ldq;
      p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)qn;
      p.M = (int)qn;
      p.b = g + g0 * ldg; p.b_bytes = (uint32_t)(gn * ldg * 4);
      p.ldb = (int)ldg; p.kb_valid = D; p.Ncol = (int)gn;
      p.Kloop = (D + 15) / 16 * 16;
      p.out = out + q0 * ldo + g0; p.ldo = ldo; p.metric = metric; p.tile = tile;
      const int rc = launch_gemm(p, EPI_DIST, 1, as_stream(stream));
      if (rc != PPS_OK) return rc;
    }
  }
  return PPS_OK;
}

int pps_row_sqnorm(const float* x, int64_t rows, int D, int64_t ld, float* out,
                   void* stream) {
  PPS_ENFORCE(x && out, "null pointer");
  PPS_ENFORCE(rows >= 0 && D > 0 && D % 4 == 0 && ld >= D && ld % 4 == 0, "bad shape");
  PPS_ENFORCE(aligned16(x), "x must be 16-byte aligned");
  return row_sqnorm(x, rows, D, ld, out, as_stream(stream));
}

int pps_split_bf16x3_sqnorm(const float* x, int64_t rows, int D, int64_t ld, uint16_t* out3,
                            float* sqnorm, void* stream) {
  PPS_ENFORCE(x && out3 && sqnorm, "null pointer");
  PPS_ENFORCE(rows >= 0 && D > 0 && D % 4 == 0 && ld >= D && ld % 4 == 0, "bad shape");
  PPS_ENFORCE(aligned16(x), "x must be 16-byte aligned");
  PPS_ENFORCE(((uintptr_t)out3 & 7) == 0, "out3 must be 8-byte aligned");
  return split_sqnorm(x, rows, D, ld, out3, sqnorm, as_stream(stream));
}

int pps_split_bf16x3_sqnorm_tiled(const float* x, int64_t rows, int D, int64_t ld,
                                  uint16_t* out3t, float* sqnorm, void* stream) {
  PPS_ENFORCE(x && out3t && sqnorm, "null pointer");
  PPS_ENFORCE(rows >= 0 && D > 0 && D % 32 == 0 && ld >= D && ld % 4 == 0,
              "bad shape (D % 32 == 0)");
  PPS_ENFORCE(aligned16(x), "x must be 16-byte aligned");
  PPS_ENFORCE(((uintptr_t)out3t & 7) == 0, "out3t must be 8-byte aligned");
  return split_sqnorm_tiled(x, rows, D, ld, out3t, sqnorm, as_stream(stream));
}

int pps_distmat_x3(const float* q, int64_t Q, int64_t ldq, const float* qsq,
                   const uint16_t* g3, const float* gsq, int64_t G, int64_t ldg, int D,
                   int metric, float* out, int64_t ldo, int tile, void* stream) {
  PPS_ENFORCE(q && qsq && g3 && gsq && out, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0, "bad shape");
  PPS_ENFORCE(D % 4 == 0, "D must be a multiple of 4, got " + std::to_string(D));
  PPS_ENFORCE(ldq % 4 == 0 && ldg % 4 == 0 && ldq >= D && ldg >= D, "bad leading dims");
  PPS_ENFORCE(ldo >= G, "ldo < G");
  PPS_ENFORCE(aligned16(q) && aligned16(g3), "q/g3 must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(ldq * 4 < kMaxBufBytes && ldg * 2 < kMaxBufBytes, "rows too long");
  const int64_t qblk = std::min<int64_t>(Q, (kMaxBufBytes - 1) / (ldq * 4));
  const int64_t gblk = std::min<int64_t>(G, (kMaxBufBytes - 1) / (ldg * 2));
  for (int64_t q0 = 0; q0 < Q; q0 += qblk) {
    for (int64_t g0 = 0; g0 < G; g0 += gblk) {
      const int64_t qn = std::min(qblk, Q - q0), gn = std::min(gblk, G - g0);
      GemmParams p{};
      p.splitk = 1;
      p.a = q + q0 * ldq; p.a_bytes = (uint32_t)(qn * ldq * 4);
      p.H = 1; p.W = (int)qn; p.Cin = D; p.lda = (int)ldq;
      p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)qn;
      p.M = (int)qn;
      p.b3 = g3 + g0 * ldg; p.b_plane = G * ldg; p.b_bytes = (uint32_t)(gn * ldg * 2);
      p.ldb = (int)ldg; p.kb_valid = D; p.Ncol = (int)gn;
      p.Kloop = (D + 15) / 16 * 16;
      p.norm_a = qsq + q0; p.norm_b = gsq + g0;
      p.out = out + q0 * ldo + g0; p.ldo = ldo; p.metric = metric; p.tile = tile;
      const int rc = launch_gemm_x3(p, EPI_DIST, 1, as_stream(stream));
      if (rc != PPS_OK) return rc;
    }
  }
  return PPS_OK;
}

int pps_distmat_x3p(const uint16_t* q3, int64_t Q, int64_t ldq, const float* qsq,
                    const uint16_t* g3, const float* gsq, int64_t G, int64_t ldg, int D,
                    int metric, float* out, int64_t ldo, int tile, void* stream) {
  PPS_ENFORCE(q3 && qsq && g3 && gsq && out, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0, "bad shape");
  PPS_ENFORCE(D % 32 == 0, "D must be a multiple of 32, got " + std::to_string(D));
  PPS_ENFORCE(ldq % 8 == 0 && ldg % 8 == 0 && ldq >= D && ldg >= D, "bad leading dims");
  PPS_ENFORCE(ldo >= G, "ldo < G");
  PPS_ENFORCE(aligned16(q3) && aligned16(g3), "q3/g3 must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(tile == 0 || tile >= GEMM_TILE_P_FIRST,
              "query planes need a pipelined tile (0 or >= " +
                  std::to_string((int)GEMM_TILE_P_FIRST) + ")");
  PPS_ENFORCE(ldq * 2 < kMaxBufBytes && ldg * 2 < kMaxBufBytes, "rows too long");
  const int64_t qblk = std::min<int64_t>(Q, (kMaxBufBytes - 1) / (ldq * 2));
  const int64_t gblk = std::min<int64_t>(G, (kMaxBufBytes - 1) / (ldg * 2));
  for (int64_t q0 = 0; q0 < Q; q0 += qblk) {
    for (int64_t g0 = 0; g0 < G; g0 += gblk) {
      const int64_t qn = std::min(qblk, Q - q0), gn = std::min(gblk, G - g0);
      GemmParams p{};
      p.splitk = 1;
      p.a3 = q3 + q0 * ldq; p.a_plane = Q * ldq; p.a_bytes = (uint32_t)(qn * ldq * 2);
      p.H = 1; p.W = (int)qn; p.Cin = D; p.lda = (int)ldq;
      p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)qn;
      p.M = (int)qn;
      p.b3 = g3 + g0 * ldg; p.b_plane = G * ldg; p.b_bytes = (uint32_t)(gn * ldg * 2);
      p.ldb = (int)ldg; p.kb_valid = D; p.Ncol = (int)gn;
      p.Kloop = D;
      p.norm_a = qsq + q0; p.norm_b = gsq + g0;
      p.out = out + q0 * ldo + g0; p.ldo = ldo; p.metric = metric;
      p.tile = tile ? tile : GEMM_TILE_P16_FIRST + 4;  // as pps_distmat_x3's default
      const int rc = launch_gemm_x3(p, EPI_DIST, 1, as_stream(stream));
      if (rc != PPS_OK) return rc;
    }
  }
  return PPS_OK;
}

// Both operands' planes chunk-tiled ([rows16 / 16][D / 32][16][32] per
// plane, rows padded to a multiple of 16 with zeros: pps_tile_planes).
int pps_distmat_x3p_tiled(const uint16_t* q3t, int64_t Q, const float* qsq,
                          const uint16_t* g3t, const float* gsq, int64_t G, int D, int metric,
                          float* out, int64_t ldo, int tile, void* stream) {
  PPS_ENFORCE(q3t && qsq && g3t && gsq && out, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && D > 0 && D % 32 == 0, "bad shape (D % 32 == 0)");
  PPS_ENFORCE(ldo >= G, "ldo < G");
  PPS_ENFORCE(aligned16(q3t) && aligned16(g3t), "planes must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(tile == 0 || (tile >= GEMM_TILE_P_FIRST && tile < GEMM_TILE_WS),
              "tiled planes need a pipelined tile (0 or 29..53)");
  const int64_t Qp = (Q + 15) / 16 * 16, Gp = (G + 15) / 16 * 16;
  PPS_ENFORCE(Qp * D * 2 < kMaxBufBytes && Gp * D * 2 < kMaxBufBytes, "planes over 2 GiB");
  if (Q == 0 || G == 0) return PPS_OK;
  GemmParams p{};
  p.splitk = 1;
  p.tiled = 3;
  p.a3 = q3t; p.a_plane = Qp * D; p.a_bytes = (uint32_t)(Qp * D * 2);
  p.H = 1; p.W = (int)Q; p.Cin = D; p.lda = D;
  p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)Q;
  p.M = (int)Q;
  p.b3 = g3t; p.b_plane = Gp * D; p.b_bytes = (uint32_t)(Gp * D * 2);
  p.ldb = D; p.kb_valid = D; p.Ncol = (int)G;
  p.Kloop = D;
  p.norm_a = qsq; p.norm_b = gsq;
  p.out = out; p.ldo = ldo; p.metric = metric;
  // default 128 x 256 (tile 43): Market 1.81 ms vs 2.05 on 256 x 128, Duke's
  // query x gallery the same either way (scripts/probes/dist_default_tile_probe.py)
  p.tile = tile ? tile : GEMM_TILE_P16_FIRST + 5;
  return launch_gemm_x3(p, EPI_DIST, 1, as_stream(stream));
}

int pps_distmat_x3_self(const float* x, int64_t N, int64_t ld, const float* xsq,
                        const uint16_t* x3, int D, int metric, float* out, int64_t ldo,
                        int tile, void* stream) {
  PPS_ENFORCE(x && xsq && x3 && out, "null pointer");
  PPS_ENFORCE(N >= 0 && D > 0 && D % 32 == 0, "D must be a positive multiple of 32");
  PPS_ENFORCE(ld % 8 == 0 && ld >= D, "bad leading dim");
  PPS_ENFORCE(ldo >= N, "ldo < N");
  PPS_ENFORCE(aligned16(x) && aligned16(x3), "x/x3 must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE(N * ld * 4 < kMaxBufBytes, "self-distance operand larger than 2 GiB");
  PPS_ENFORCE(N * ldo < (1ll << 31), "output larger than 2^31 elements");
  GemmParams p{};
  p.splitk = 1;
  p.a = x; p.a_bytes = (uint32_t)(N * ld * 4);
  p.H = 1; p.W = (int)N; p.Cin = D; p.lda = (int)ld;
  p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)N;
  p.M = (int)N;
  p.b3 = x3; p.b_plane = N * ld; p.b_bytes = (uint32_t)(N * ld * 2);
  p.ldb = (int)ld; p.kb_valid = D; p.Ncol = (int)N;
  p.Kloop = D;
  p.norm_a = xsq; p.norm_b = xsq;
  p.out = out; p.ldo = ldo; p.metric = metric; p.sym = 1; p.tile = tile;
  return launch_gemm_x3(p, EPI_DIST, 1, as_stream(stream));
}

// The same from chunk-tiled planes (pps_split_bf16x3_sqnorm_tiled /
// pps_tile_planes layout): both operands are the one tiled copy, staged by
// pure DMA like pps_distmat_x3p_tiled.
int pps_distmat_x3_self_tiled(const uint16_t* x3t, int64_t N, const float* xsq, int D,
                              int metric, float* out, int64_t ldo, int tile, void* stream) {
  PPS_ENFORCE(x3t && xsq && out, "null pointer");
  PPS_ENFORCE(N >= 0 && D > 0 && D % 32 == 0, "D must be a positive multiple of 32");
  PPS_ENFORCE(ldo >= N, "ldo < N");
  PPS_ENFORCE(aligned16(x3t), "x3t must be 16-byte aligned");
  PPS_ENFORCE(metric >= 0 && metric <= 2, "unknown metric");
  const int64_t Np = (N + 15) / 16 * 16;
  PPS_ENFORCE(Np * D * 2 < kMaxBufBytes, "planes over 2 GiB");
  PPS_ENFORCE(N * ldo < (1ll << 31), "output larger than 2^31 elements");
  PPS_ENFORCE(tile == 0 || (tile >= GEMM_TILE_P_FIRST && tile < GEMM_TILE_C16_FIRST &&
                            tile != GEMM_TILE_WS),
              "tiled self-distance needs a pipelined tile (0, 29..53 or 55)");
  if (N == 0) return PPS_OK;
  GemmParams p{};
  p.splitk = 1;
  p.tiled = 3;
  p.a3 = x3t; p.a_plane = Np * D; p.a_bytes = (uint32_t)(Np * D * 2);
  p.H = 1; p.W = (int)N; p.Cin = D; p.lda = D;
  p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.Ho = 1; p.Wo = (int)N;
  p.M = (int)N;
  p.b3 = x3t; p.b_plane = Np * D; p.b_bytes = (uint32_t)(Np * D * 2);
  p.ldb = D; p.kb_valid = D; p.Ncol = (int)N;
  p.Kloop = D;
  p.norm_a = xsq; p.norm_b = xsq;
  p.out = out; p.ldo = ldo; p.metric = metric; p.sym = 1;
  p.tile = tile ? tile : GEMM_TILE_P16_FIRST + 5;  // 128 x 256 (the distance matrix's)
  return launch_gemm_x3(p, EPI_DIST, 1, as_stream(stream));
}

int pps_pairwise_distance(const float* X, int N, int D, float* Z, void* stream) {
  PPS_ENFORCE(X && Z, "null pointer");
  PPS_ENFORCE(N >= 0 && D > 0 && D % 4 == 0, "X must be 2-D [N][D] with D % 4 == 0");
  PPS_ENFORCE(aligned16(X), "X must be 16-byte aligned");
  GemmParams p{};
  p.splitk = 1;
  PPS_ENFORCE((int64_t)N * D * 4 < kMaxBufBytes, "X larger than 2 GiB");
  p.a = X; p.H = 1; p.W = N; p.Cin = D; p.lda = D; p.a_bytes = (uint32_t)((int64_t)N * D * 4);
  p.KH = p.KW = 1; p.stride = 1; p.dil = 1; p.Ho = 1; p.Wo = N; p.M = N;
  p.b = X; p.ldb = D; p.kb_valid = D; p.Ncol = N; p.b_bytes = p.a_bytes;
  p.Kloop = (D + 15) / 16 * 16;
  p.out = Z; p.ldo = N; p.metric = PPS_METRIC_SQEUCLIDEAN; p.zero_diag = 1;
  return launch_gemm(p, EPI_DIST, 1, as_stream(stream));
}

int pps_collect_matches(const float* dist, int64_t Q, int64_t G, int64_t ldd,
                        const int32_t* qcam, const int32_t* gcam, const int32_t* members,
                        const int32_t* q_beg, const int32_t* q_end, int64_t g_offset,
                        int Pmax, float* pos_d, int32_t* pos_idx, int32_t* pos_cnt, int Jmax,
                        float* junk_d, int32_t* junk_idx, int32_t* junk_cnt, void* stream) {
  PPS_ENFORCE(dist && qcam && gcam && members && q_beg && q_end && pos_d && pos_idx &&
                  pos_cnt && junk_d && junk_idx && junk_cnt,
              "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && ldd >= G && Pmax > 0 && Jmax > 0, "bad shape");
  PPS_ENFORCE(G < (1ll << 31) && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  return collect_matches(dist, Q, ldd, qcam, gcam, members, q_beg, q_end, g_offset, Pmax,
                         pos_d, pos_idx, pos_cnt, Jmax, junk_d, junk_idx, junk_cnt,
                         as_stream(stream));
}

int pps_rank_cells(void) { return kRankCells; }

int pps_rank_prepare(int R, int64_t Q, int Pmax, const float* pos_d, const int32_t* pos_idx,
                     const int32_t* pos_cnt, float* sorted_d, int32_t* sorted_idx,
                     int32_t* pos_total, int32_t* cells, void* stream) {
  PPS_ENFORCE(pos_d && pos_idx && pos_cnt && sorted_d && sorted_idx && pos_total && cells,
              "null pointer");
  PPS_ENFORCE(((uintptr_t)cells & 15) == 0, "cells must be 16-byte aligned");
  PPS_ENFORCE(R >= 1 && R <= kMergeMaxLists,
              "R must be in [1, " + std::to_string(kMergeMaxLists) + "]");
  PPS_ENFORCE(Q >= 0 && Pmax > 0, "bad shape");
  // beyond kRankMergeCap merged positives the lists are sorted in place in
  // global memory (rank_prepare_global_kernel): no capacity limit
  PPS_ENFORCE((int64_t)R * Pmax < (1ll << 30), "R * Pmax must be < 2^30");
  return rank_prepare(R, Q, Pmax, pos_d, pos_idx, pos_cnt, sorted_d, sorted_idx, pos_total,
                      cells, as_stream(stream));
}

int pps_rank_count_stream(const float* dist, int64_t Q, int64_t G, int64_t ldd,
                          int64_t g_offset, int Ptot, const float* sorted_d,
                          const int32_t* sorted_idx, const int32_t* pos_total,
                          const int32_t* cells, int Jmax, const float* junk_d,
                          const int32_t* junk_idx, const int32_t* junk_cnt, int32_t* hist,
                          int32_t* before, void* stream) {
  PPS_ENFORCE(dist && sorted_d && sorted_idx && pos_total && cells && junk_d && junk_idx &&
                  junk_cnt && hist && before,
              "null pointer");
  PPS_ENFORCE(((uintptr_t)cells & 15) == 0, "cells must be 16-byte aligned");
  PPS_ENFORCE(Q >= 0 && G >= 0 && ldd >= G && Ptot > 0 && Jmax > 0, "bad shape");
  PPS_ENFORCE((G + kRankStreamChunk - 1) / kRankStreamChunk <= 65535,
              "G too large for the chunk grid (65535 chunks of " +
                  std::to_string(kRankStreamChunk) + ")");
  return rank_count_stream(dist, Q, G, ldd, g_offset, Ptot, sorted_d, sorted_idx, pos_total,
                           cells, Jmax, junk_d, junk_idx, junk_cnt, hist, before,
                           as_stream(stream));
}

int pps_ap_finalize(int64_t Q, int Ptot, const float* sorted_d, const int32_t* pos_total,
                    const int32_t* hist, const int32_t* before, double* ap,
                    int32_t* valid, int32_t* first_rank, void* stream) {
  PPS_ENFORCE(sorted_d && pos_total && hist && before && ap && valid && first_rank,
              "null pointer");
  PPS_ENFORCE(Q >= 0 && Ptot >= 0, "bad shape");
  return ap_finalize(Q, Ptot, sorted_d, pos_total, hist, before, ap, valid, first_rank,
                     as_stream(stream));
}

int pps_cmc_counts(const float* dist, int64_t Q, int64_t G, int64_t ldd, int64_t g_offset,
                   int Ptot, const float* sorted_d, const int32_t* sorted_idx,
                   const int32_t* pos_total, const int32_t* qcam, const int32_t* gcam, int Jmax,
                   const float* junk_d, const int32_t* junk_idx, const int32_t* junk_cnt,
                   int32_t* hist, void* stream) {
  PPS_ENFORCE(dist && sorted_d && sorted_idx && pos_total && hist, "null pointer");
  PPS_ENFORCE((qcam == nullptr) == (gcam == nullptr),
              "qcam and gcam are given together (separate_camera_set) or not at all");
  PPS_ENFORCE(gcam || (junk_d && junk_idx && junk_cnt && Jmax > 0),
              "without separate_camera_set the junk lists are required");
  PPS_ENFORCE(Q >= 0 && G >= 0 && ldd >= G && Ptot > 0, "bad shape");
  PPS_ENFORCE(G < (1ll << 31) && g_offset + G < (1ll << 31), "gallery indices must fit int32");
  PPS_ENFORCE((G + kRankStreamChunk - 1) / kRankStreamChunk <= 65535,
              "G too large for the chunk grid");
  return cmc_counts(dist, Q, G, ldd, g_offset, Ptot, sorted_d, sorted_idx, pos_total, qcam,
                    gcam, Jmax, junk_d, junk_idx, junk_cnt, hist, as_stream(stream));
}

int pps_cmc_finalize(int64_t Q, int Ptot, const int32_t* pos_total, const int32_t* hist,
                     int topk, int first_match_break, double* ret, int32_t* valid,
                     void* stream) {
  PPS_ENFORCE(pos_total && hist && ret && valid, "null pointer");
  PPS_ENFORCE(Q >= 0 && Ptot > 0 && topk >= 1, "bad shape");
  return cmc_finalize(Q, Ptot, pos_total, hist, topk, first_match_break ? 1 : 0, ret, valid,
                      as_stream(stream));
}

int pps_topk(const float* dist, int64_t Q, int64_t G, int64_t ldd, int k, float* vals,
             int32_t* idx, void* stream) {
  PPS_ENFORCE(dist && vals && idx, "null pointer");
  PPS_ENFORCE(k >= 1 && k <= kTopkCap,
              "k must be in [1, " + std::to_string(kTopkCap) + "], got " + std::to_string(k));
  PPS_ENFORCE(G >= k && ldd >= G, "need G >= k");
  PPS_ENFORCE(G < (1ll << 31), "G must fit int32");
  return topk(dist, Q, G, ldd, k, vals, idx, as_stream(stream));
}

int pps_argsort_rows(const float* dist, int64_t Q, int64_t G, int64_t ldd, int32_t* idx,
                     int64_t ldi, float* vals, int64_t ldv, void* stream) {
  PPS_ENFORCE(dist && idx, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && ldd >= G && ldi >= G && (!vals || ldv >= G), "bad shape");
  PPS_ENFORCE(G <= argsort_rows_cap(), "rows longer than " + std::to_string(argsort_rows_cap()) +
                                           " entries (pps_argsort_rows_cap): use pps_topk");
  return argsort_rows(dist, Q, G, ldd, idx, ldi, vals, ldv, as_stream(stream));
}

int pps_argsort_rows_cap(void) { return argsort_rows_cap(); }

int pps_sgs_keys(const int32_t* order, int64_t Q, int64_t G, int64_t ldo, const int32_t* gid,
                 const int32_t* gcam, const int32_t* qid, const int32_t* qcam,
                 int separate_camera_set, int U, float* keys, void* stream) {
  PPS_ENFORCE(order && gid && gcam && qid && qcam && keys, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 0 && ldo >= G, "bad shape");
  PPS_ENFORCE(U >= 1 && U <= kSgsMaxIds, "U (distinct gallery identities) must be in [1, " +
                                                  std::to_string(kSgsMaxIds) + "]");
  return sgs_keys(order, Q, G, ldo, gid, gcam, qid, qcam, separate_camera_set ? 1 : 0, U, keys,
                  as_stream(stream));
}

int pps_sgs_groups(const float* sorted_keys, const int32_t* perm, int64_t Q, int64_t G, int U,
                   const int32_t* qid, int32_t* gstart, int32_t* glen, int32_t* nids,
                   int32_t* qt, void* stream) {
  PPS_ENFORCE(sorted_keys && perm && qid && gstart && glen && nids && qt, "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 1 && G <= argsort_rows_cap(), "G must be in [1, " +
                                                               std::to_string(argsort_rows_cap()) +
                                                               "]");
  PPS_ENFORCE(U >= 1 && U <= kSgsMaxIds, "U (distinct gallery identities) must be in [1, " +
                                                  std::to_string(kSgsMaxIds) + "]");
  PPS_ENFORCE(sgs_groups_lds_bytes(G, U) <= kLdsBytesGfx950, "groups do not fit in LDS");
  return sgs_groups(sorted_keys, perm, Q, G, U, qid, gstart, glen, nids, qt, as_stream(stream));
}

int pps_sgs_ranks(const int32_t* perm, int64_t Q, int64_t G, const int32_t* rows, int64_t nr,
                  const int32_t* gstart, const int32_t* glen, const int32_t* nids,
                  const int32_t* qt, int U, int repeat, const int32_t* draws, int64_t ldd,
                  int32_t* k, void* stream) {
  PPS_ENFORCE(perm && gstart && glen && nids && qt && k && (nr == 0 || (rows && draws)),
              "null pointer");
  PPS_ENFORCE(Q >= 0 && G >= 1 && nr >= 0 && repeat >= 1 && ldd >= 1, "bad shape");
  PPS_ENFORCE(U >= 1 && U <= kSgsMaxIds && ldd <= U, "ldd must be in [1, U]");
  return sgs_ranks(perm, G, rows, nr, gstart, glen, nids, qt, U, repeat, draws, ldd, k,
                   as_stream(stream));
}

int pps_topk_merge(const float* vals, const int32_t* idx, int R, int64_t Q, int k_in,
                   const int64_t* list_offsets, int k_out, float* out_vals,
                   int32_t* out_idx, void* stream) {
  PPS_ENFORCE(vals && idx && list_offsets && out_vals && out_idx, "null pointer");
  PPS_ENFORCE(R >= 1 && R <= kMergeMaxLists,
              "R must be in [1, " + std::to_string(kMergeMaxLists) + "]");
  PPS_ENFORCE(Q >= 0 && k_in >= 1 && k_out >= 1, "bad shape");
  PPS_ENFORCE((int64_t)R * k_in <= kMergeMaxEntries,
              "R * k_in must be <= " + std::to_string(kMergeMaxEntries) + " (LDS), got " +
                  std::to_string((int64_t)R * k_in));
  MergeOffsets offs{};
  for (int r = 0; r < R; ++r) {
    PPS_ENFORCE(list_offsets[r] >= 0 && list_offsets[r] + k_in <= (int64_t)INT32_MAX,
                "list offset out of the int32 index range");
    offs.off[r] = list_offsets[r];
  }
  return topk_merge(vals, idx, R, Q, k_in, offs, k_out, out_vals, out_idx,
                    as_stream(stream));
}

int64_t pps_rerank_workspace_bytes(int64_t Q, int64_t G, int k1, int k2) {
  if (Q < 0 || G < 0 || k1 < 1 || k2 < 1) return -1;
  return (int64_t)rerank_workspace_bytes(Q, G, k1, k2);
}

int64_t pps_rerank_workspace_bytes_ld(const float* q_g, int64_t ld_qg, const float* q_q,
                                      int64_t ld_qq, const float* g_g, int64_t ld_gg, int64_t Q,
                                      int64_t G, int k1, int k2, int flags) {
  if (Q < 0 || G < 0 || k1 < 1 || k2 < 1) return -1;
  return (int64_t)rerank_workspace_bytes_for(q_g, ld_qg, q_q, ld_qq, g_g, ld_gg, Q, G, k1, k2,
                                             flags);
}

int pps_re_ranking_ld(const float* q_g, int64_t ld_qg, const float* q_q, int64_t ld_qq,
                      const float* g_g, int64_t ld_gg, int64_t Q, int64_t G, int k1, int k2,
                      double lambda_value, int flags, void* workspace, int64_t ws_bytes,
                      float* out, void* stream) {
  PPS_ENFORCE(q_g && q_q && g_g && workspace && out, "null pointer");
  PPS_ENFORCE(Q > 0 && G > 0, "bad shape");
  PPS_ENFORCE(ld_qg >= G && ld_qq >= Q && ld_gg >= G, "leading dims smaller than the rows");
  PPS_ENFORCE(k1 >= 1 && k1 + 1 <= 64, "k1 + 1 must be <= 64");
  PPS_TRY(rr_layout_guard(__func__, k1, k2));
  PPS_ENFORCE(jaccard_lds_bytes(G) + 2048 <= kLdsBytesGfx950,
              "G must be <= 38400 (the Jaccard pass keeps a gallery row in LDS)");
  PPS_ENFORCE((Q + G) >= k1 + 1, "need Q + G >= k1 + 1");
  PPS_ENFORCE((flags & ~(PPS_RERANK_SYMMETRIC | PPS_RERANK_WHOLE)) == 0,
              "unknown re-ranking flags");
  PPS_ENFORCE(!(flags & PPS_RERANK_WHOLE) ||
                  ((flags & PPS_RERANK_SYMMETRIC) && ld_qg == ld_qq && ld_gg == ld_qq &&
                   q_g == q_q + Q && g_g == q_q + Q * ld_qq + Q),
              "PPS_RERANK_WHOLE: q_q, q_g and g_g must be the blocks of one symmetric matrix "
              "(one row stride, q_g = q_q + Q, g_g = q_q + Q * ld + Q) and PPS_RERANK_SYMMETRIC set");
  return rerank(q_g, ld_qg, q_q, ld_qq, g_g, ld_gg, Q, G, k1, k2, lambda_value, workspace,
                (size_t)ws_bytes, out, as_stream(stream), flags);
}

int pps_re_ranking_flags(const float* q_g, const float* q_q, const float* g_g, int64_t Q,
                         int64_t G, int k1, int k2, double lambda_value, int flags,
                         void* workspace, int64_t ws_bytes, float* out, void* stream) {
  return pps_re_ranking_ld(q_g, G, q_q, Q, g_g, G, Q, G, k1, k2, lambda_value, flags, workspace,
                           ws_bytes, out, stream);
}

int pps_re_ranking(const float* q_g, const float* q_q, const float* g_g, int64_t Q,
                   int64_t G, int k1, int k2, double lambda_value, void* workspace,
                   int64_t ws_bytes, float* out, void* stream) {
  return pps_re_ranking_flags(q_g, q_q, g_g, Q, G, k1, k2, lambda_value, 0, workspace,
                              ws_bytes, out, stream);
}

// the (k1, k2, g_window, size) checks the two row-form entries share; every one
// runs before anything is launched
static int rerank_rows_guards(const char* fn, int64_t Q, int64_t G, int k1, int k2,
                              int64_t g_window) {
  PPS_ENFORCE_AS(fn, Q > 0 && G > 0, "bad shape");
  PPS_ENFORCE_AS(fn, Q + G < (1ll << 31), "N = Q + G must fit int32");
  PPS_ENFORCE_AS(fn, k1 >= 1 && k1 + 1 <= 64 && k1 + 1 <= kTkwMaxK,
                 "k1 + 1 must be <= 64 and <= pps_search_max_k()");
  PPS_TRY(rr_layout_guard(fn, k1, k2));
  const int qcap = RrLayout(k1, k2).qcap;
  PPS_ENFORCE_AS(fn, (Q + G) >= k1 + 1, "need Q + G >= k1 + 1");
  PPS_ENFORCE_AS(fn, g_window >= 0 && g_window <= kJacMaxWindow,
                 "g_window must be in [0, " + std::to_string(kJacMaxWindow) + "] (0 = auto)");
  PPS_ENFORCE_AS(fn, g_window == 0 || (G + g_window - 1) / g_window <= 65535,
                 "more than 65535 gallery windows");
  if ((Q + G) * (int64_t)qcap >= (1ll << 31)) {
    set_error(std::string(fn) + ": N * qcap = " + std::to_string(Q + G) + " * " +
              std::to_string(qcap) + " entries of the inverted index do not fit int32");
    return PPS_ERR_CAPACITY;
  }
  return PPS_OK;
}

int64_t pps_rerank_rows_workspace_bytes(int64_t Q, int64_t G, int k1, int k2) {
  if (Q < 0 || G < 0 || k1 < 1 || k1 + 1 > 64 || k2 < 1 || k2 > k1 + 1) return -1;
  return rerank_rows_workspace_bytes(false, Q, G, k1, k2, 0);
}

int pps_re_ranking_rows(const float* W, int64_t ldw, int64_t Q, int64_t G, int k1, int k2,
                        double lambda_value, int64_t g_window, void* workspace, int64_t ws_bytes,
                        float* out, void* stream) {
  PPS_ENFORCE(W && workspace && out, "null pointer");
  PPS_TRY(rerank_rows_guards(__func__, Q, G, k1, k2, g_window));
  PPS_ENFORCE(ldw >= Q + G, "ldw smaller than the rows");
  PPS_ENFORCE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  RrRows src{};
  src.W = W;
  src.ldw = ldw;
  return rerank_rows(src, Q, G, k1, k2, lambda_value, g_window, workspace,
                     ws_bytes < 0 ? 0 : (size_t)ws_bytes, out, as_stream(stream));
}

int64_t pps_rerank_features_workspace_bytes(int64_t Q, int64_t G, int k1, int k2, int segments) {
  if (Q < 0 || G < 0 || k1 < 1 || k1 + 1 > 64 || k1 + 1 > kTkwMaxK || k2 < 1 || k2 > k1 + 1 ||
      segments < 0)
    return -1;
  return rerank_rows_workspace_bytes(true, Q, G, k1, k2, segments);
}

int pps_re_ranking_features(const uint16_t* x2t, const float* xsq, const float* xrs,
                            const uint16_t* g2t, const float* gsq, const float* grs, int64_t Q,
                            int64_t G, int D, int metric, int k1, int k2, double lambda_value,
                            int segments, int tile, int64_t g_window, void* workspace,
                            int64_t ws_bytes, float* out, void* stream) {
  // the operands: x = [queries; gallery] (N rows) and the gallery rows' own planes
  RrRows src{};
  src.x = h2_operand(x2t, xsq, xrs, Q + G);
  src.g = h2_operand(g2t, gsq, grs, G);
  src.D = D; src.metric = metric; src.segments = segments; src.tile = tile;
  PPS_ENFORCE(workspace && out, "null pointer");
  PPS_TRY(rerank_rows_guards(__func__, Q, G, k1, k2, g_window));   // Q, G > 0, N in int32
  PPS_TRY(h2_operands_guard(__func__, src.x, src.g, D, metric));
  PPS_TRY(fused_plan_guard(__func__, segments, tile));
  PPS_ENFORCE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  return rerank_rows(src, Q, G, k1, k2, lambda_value, g_window, workspace,
                     ws_bytes < 0 ? 0 : (size_t)ws_bytes, out, as_stream(stream));
}

int64_t pps_rerank_prepared_workspace_bytes(int64_t Q, int64_t G, int k1, int k2, int segments) {
  if (Q < 0 || G < 0 || k1 < 1 || k1 + 1 > 64 || k1 + 1 > kTkwMaxK || k2 < 1 || k2 > k1 + 1 ||
      segments < 0)
    return -1;
  return rerank_prepared_workspace_bytes(Q, G, k1, k2, segments);
}

int pps_re_ranking_prepared(const uint16_t* q2t, const float* qsq, const float* qrs,
                            const uint16_t* g2t, const float* gsq, const float* grs, int64_t Q,
                            int64_t G, int D, int metric, const float* nn_vals,
                            const int32_t* nn_idx, int nn_ld, const float* g_rowmax, int k1,
                            int k2, double lambda_value, int segments, int tile,
                            int64_t g_window, void* workspace, int64_t ws_bytes, float* out,
                            void* stream) {
  RrPrepared src{};
  src.q = h2_operand(q2t, qsq, qrs, Q);
  src.g = h2_operand(g2t, gsq, grs, G);
  src.nn_vals = nn_vals; src.nn_idx = nn_idx; src.nn_ld = nn_ld; src.g_rowmax = g_rowmax;
  src.D = D; src.metric = metric; src.segments = segments; src.tile = tile;
  PPS_ENFORCE(workspace && out && nn_vals && nn_idx && g_rowmax, "null pointer");
  PPS_TRY(rerank_rows_guards(__func__, Q, G, k1, k2, g_window));   // Q, G > 0, N in int32
  PPS_TRY(h2_operands_guard(__func__, src.q, src.g, D, metric));
  PPS_TRY(fused_plan_guard(__func__, segments, tile));
  PPS_ENFORCE(nn_ld >= k1 + 1, "nn_ld must be >= k1 + 1");
  PPS_ENFORCE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  return rerank_prepared(src, Q, G, k1, k2, lambda_value, g_window, workspace,
                         ws_bytes < 0 ? 0 : (size_t)ws_bytes, out, as_stream(stream));
}

int pps_conv1x1_seam_x3(const float* x, int64_t M, int K1, const uint16_t* w2c, int N1,
                        const float* scale2c, const float* shift2c, const float* residual,
                        float* trunk, const uint16_t* w2a, int N2, const float* scale2a,
                        const float* shift2a, float* y, void* stream) {
  PPS_ENFORCE(x && w2c && scale2c && shift2c && residual && trunk && w2a && scale2a && shift2a &&
                  y,
              "null pointer");
  PPS_ENFORCE(M >= 0 && M * N1 * 4 < kMaxBufBytes, "bad M");
  PPS_ENFORCE(seam_supported(K1, N1, N2),
              "bottleneck seam: (K1, N1, N2) must be (64, 256, 64) or (128, 512, 128), got (" +
                  std::to_string(K1) + ", " + std::to_string(N1) + ", " + std::to_string(N2) + ")");
  PPS_ENFORCE(aligned16(x) && aligned16(w2c) && aligned16(residual) && aligned16(trunk) &&
                  aligned16(w2a) && aligned16(y) && aligned16(scale2c) && aligned16(shift2c) &&
                  aligned16(scale2a) && aligned16(shift2a),
              "seam operands must be 16-byte aligned");
  SeamParams p{x, residual, w2c, scale2c, shift2c, trunk, w2a, scale2a, shift2a, y, (int)M};
  return launch_seam_x3(p, K1, N1, N2, as_stream(stream));
}

// ---- convolutions: the implementations are conv_ops.hip's conv_impl /
// conv_pps_impl / dual_impl; an entry point names what it was given ----------
#define PPS_CONV_SHAPE(a)                                                            \
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.Cout = Cout; a.Kpad = Kpad; \
  a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.dil = dil;                 \
  a.scale = scale; a.shift = shift; a.Ho = Ho; a.Wo = Wo; a.tile = tile; a.stream = stream
#define PPS_DUAL_SHAPE(a)                                                                 \
  a.x = x; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.KH = KH; a.KW = KW;     \
  a.stride = stride; a.pad = pad; a.x2 = x2; a.H2 = H2; a.W2 = W2; a.Cin2 = Cin2;         \
  a.ldx2 = ldx2; a.stride2 = stride2; a.Cout = Cout; a.Kpad = Kpad1; a.Kpad2 = Kpad2;     \
  a.shift = shift; a.relu = relu; a.y = y; a.Ho = Ho; a.Wo = Wo; a.ldy = ldy;             \
  a.tile = tile; a.stream = stream

int pps_conv2d_bn_act(const float* x, int N, int H, int W, int Cin, int ldx,
                      const float* w, int Cout, int Kpad, int KH, int KW, int stride,
                      int pad, int dil, const float* scale, const float* shift,
                      const float* residual, int relu, float* y, int Ho, int Wo, int ldy,
                      int tile, void* stream) {
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.w = w; a.residual = residual; a.relu = relu; a.y = y; a.ldy = ldy;
  return conv_impl(a);
}

int pps_conv2d_bn_act_x3(const float* x, int N, int H, int W, int Cin, int ldx,
                         const uint16_t* w3, int Cout, int Kpad, int KH, int KW, int stride,
                         int pad, int dil, const float* scale, const float* shift,
                         const float* residual, int relu, float* y, int Ho, int Wo, int ldy,
                         int tile, void* stream) {
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.w = w3; a.x3 = 1; a.residual = residual; a.relu = relu; a.y = y; a.ldy = ldy;
  return conv_impl(a);
}

// x3p: bf16x3 activation planes (x3 / y3, plane strides in elements) instead
// of f32 x / y
int pps_conv2d_bn_act_x3p(const float* x, const uint16_t* x3, int64_t x_plane, int N, int H,
                          int W, int Cin, int ldx, const uint16_t* w3, int Cout, int Kpad,
                          int KH, int KW, int stride, int pad, int dil, const float* scale,
                          const float* shift, const float* residual, int relu, float* y,
                          uint16_t* y3, int64_t y_plane, int Ho, int Wo, int ldy, int tile,
                          void* stream) {
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.x_pl = x3; a.x_plane = x_plane; a.w = w3; a.x3 = 1;
  a.residual = residual; a.relu = relu; a.y = y; a.y_pl = y3; a.y_plane = y_plane; a.ldy = ldy;
  return conv_impl(a);
}

int pps_conv2d_bn_act_x3p_splitk(const float* x, const uint16_t* x3, int64_t x_plane, int N,
                                 int H, int W, int Cin, int ldx, const uint16_t* w3, int Cout,
                                 int Kpad, int KH, int KW, int stride, int pad, int dil,
                                 const float* scale, const float* shift, const float* residual,
                                 int relu, float* y, uint16_t* y3, int64_t y_plane, int Ho,
                                 int Wo, int ldy, int splitk, float* part, int tile,
                                 void* stream) {
  PPS_ENFORCE(splitk >= 1 && splitk <= 16, "splitk must be in [1, 16]");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.x_pl = x3; a.x_plane = x_plane; a.w = w3; a.x3 = 1;
  a.residual = residual; a.relu = relu; a.y = y; a.y_pl = y3; a.y_plane = y_plane; a.ldy = ldy;
  a.splitk = splitk; a.part = part;
  return conv_impl(a);
}

int pps_conv2d_bn_act_x3p_splitk_fused(const float* x, const uint16_t* x3, int64_t x_plane,
                                       int N, int H, int W, int Cin, int ldx, const uint16_t* w3,
                                       int Cout, int Kpad, int KH, int KW, int stride, int pad,
                                       int dil, const float* scale, const float* shift,
                                       const float* residual, int relu, float* y, uint16_t* y3,
                                       int64_t y_plane, int Ho, int Wo, int ldy, int splitk,
                                       float* part, int* counters, int64_t n_counters, int tile,
                                       void* stream) {
  PPS_ENFORCE(splitk >= 2 && splitk <= 16, "splitk must be in [2, 16]");
  PPS_ENFORCE(counters != nullptr, "null tile counters");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.x_pl = x3; a.x_plane = x_plane; a.w = w3; a.x3 = 1;
  a.residual = residual; a.relu = relu; a.y = y; a.y_pl = y3; a.y_plane = y_plane; a.ldy = ldy;
  a.splitk = splitk; a.part = part; a.fix_cnt = counters; a.n_cnt = n_counters;
  return conv_impl(a);
}

int pps_x3p_tile_shape(int tile, int planes, int* rows, int* cols) {
  PPS_ENFORCE(rows && cols, "null pointer");
  *rows = x3p_tile_rows(tile, planes != 0);
  *cols = x3p_tile_cols(tile, planes != 0);
  return PPS_OK;
}

// The last res5 conv with the part pooling fused into its epilogue
// (conv_ops.hip conv_pps_impl)
int pps_conv2d_bn_act_pps_x3p(const float* x, const uint16_t* x3, int64_t x_plane, int N,
                              int H, int W, int Cin, int ldx, const uint16_t* w3, int Cout,
                              int Kpad, int KH, int KW, int stride, int pad, int dil,
                              const float* scale, const float* shift, const float* residual,
                              float* y, int Ho, int Wo, const int32_t* splits, int S,
                              int max_ave, float* pps_out, int tile, void* stream) {
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.x_pl = x3; a.x_plane = x_plane; a.w = w3; a.x3 = 1; a.residual = residual; a.y = y;
  a.splits = splits; a.S = S; a.max_ave = max_ave; a.pps_out = pps_out;
  return conv_pps_impl(a);
}

// ---- f16x2 convolutions (include/pps_abi.h "f16x2 convolutions") ----------
int pps_conv2d_bn_act_h2(const float* x, int N, int H, int W, int Cin, int ldx,
                         const uint16_t* w2t, const float* wrs, int Cout, int Kpad, int KH,
                         int KW, int stride, int pad, int dil, const float* scale,
                         const float* shift, const float* residual, int relu, float* y, int Ho,
                         int Wo, int ldy, const float* amax_x, float* amax_y, int tile,
                         void* stream) {
  PPS_ENFORCE(wrs != nullptr, "null weight scales");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.w = w2t; a.x3 = 1; a.w_rs = wrs; a.residual = residual; a.relu = relu;
  a.y = y; a.ldy = ldy; a.amax_in = amax_x; a.amax_out = amax_y;
  return conv_impl(a);
}

int pps_conv2d_dual_bn_act_h2(const float* x, int N, int H, int W, int Cin, int ldx, int KH,
                              int KW, int stride, int pad, const float* x2, int H2, int W2,
                              int Cin2, int ldx2, int stride2, const uint16_t* w2t,
                              const float* wrs, int Cout, int Kpad1, int Kpad2,
                              const float* shift, int relu, float* y, int Ho, int Wo, int ldy,
                              const float* amax_x, const float* amax_x2, float* amax_y, int tile,
                              void* stream) {
  PPS_ENFORCE(wrs != nullptr, "null weight scales");
  DualArgs a;
  PPS_DUAL_SHAPE(a);
  a.w = w2t; a.x3 = 1; a.w_rs = wrs;
  a.amax_in = amax_x; a.amax_in2 = amax_x2; a.amax_out = amax_y;
  return dual_impl(a);
}

int pps_conv2d_bn_act_h2_planes(const uint16_t* x2, int64_t x_plane, int N, int H, int W,
                                int Cin, int ldx, const uint16_t* w2t, const float* wrs, int Cout,
                                int Kpad, int KH, int KW, int stride, int pad, int dil,
                                const float* scale, const float* shift, const float* residual,
                                int relu, float* y, int Ho, int Wo, int ldy, const float* amax_x,
                                float* amax_y, int tile, void* stream) {
  PPS_ENFORCE(wrs != nullptr && x2 != nullptr, "null pointer");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x_pl = x2; a.x_plane = x_plane; a.w = w2t; a.x3 = 1; a.w_rs = wrs;
  a.residual = residual; a.relu = relu; a.y = y; a.ldy = ldy;
  a.amax_in = amax_x; a.amax_out = amax_y;
  return conv_impl(a);
}

int pps_conv2d_bn_act_h2out(const float* x, const uint16_t* x2, int64_t x_plane, int N, int H,
                            int W, int Cin, int ldx, const void* w, const float* wrs, int Cout,
                            int Kpad, int KH, int KW, int stride, int pad, int dil,
                            const float* scale, const float* shift, uint16_t* y2, int64_t y_plane,
                            int Ho, int Wo, int ldy, const float* amax_x, const float* bound_in,
                            float bound_w, float bound_b, float* bound_out, int tile,
                            void* stream) {
  PPS_ENFORCE(w && y2 && bound_in && bound_out, "null pointer");
  PPS_ENFORCE(!x2 || wrs, "f16x2 activation planes in: f16x2 weights (wrs) only");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x2 ? nullptr : x; a.x_pl = x2; a.x_plane = x_plane; a.w = w; a.x3 = 1; a.w_rs = wrs;
  a.relu = 1; a.y_h2 = y2; a.y_h2_plane = y_plane; a.ldy = ldy;
  a.amax_in = wrs ? amax_x : nullptr; a.amax_out = bound_out;
  a.h2o_in = bound_in; a.h2o_bw = bound_w; a.h2o_bb = bound_b;
  return conv_impl(a);
}

int pps_conv2d_bn_act_pps_h2_planes(const uint16_t* x2, int64_t x_plane, int N, int H, int W,
                                    int Cin, int ldx, const uint16_t* w2t, const float* wrs,
                                    int Cout, int Kpad, int KH, int KW, int stride, int pad,
                                    int dil, const float* scale, const float* shift,
                                    const float* residual, float* y, int Ho, int Wo,
                                    const int32_t* splits, int S, int max_ave, float* pps_out,
                                    const float* amax_x, int tile, void* stream) {
  PPS_ENFORCE(wrs != nullptr && x2 != nullptr, "null pointer");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x_pl = x2; a.x_plane = x_plane; a.w = w2t; a.x3 = 1; a.w_rs = wrs; a.residual = residual;
  a.y = y; a.splits = splits; a.S = S; a.max_ave = max_ave; a.pps_out = pps_out;
  a.amax_in = amax_x;
  return conv_pps_impl(a);
}

int pps_conv2d_bn_act_pps_h2(const float* x, int N, int H, int W, int Cin, int ldx,
                             const uint16_t* w2t, const float* wrs, int Cout, int Kpad, int KH,
                             int KW, int stride, int pad, int dil, const float* scale,
                             const float* shift, const float* residual, float* y, int Ho, int Wo,
                             const int32_t* splits, int S, int max_ave, float* pps_out,
                             const float* amax_x, int tile, void* stream) {
  PPS_ENFORCE(wrs != nullptr, "null weight scales");
  ConvArgs a;
  PPS_CONV_SHAPE(a);
  a.x = x; a.w = w2t; a.x3 = 1; a.w_rs = wrs; a.residual = residual;
  a.y = y; a.splits = splits; a.S = S; a.max_ave = max_ave; a.pps_out = pps_out;
  a.amax_in = amax_x;
  return conv_pps_impl(a);
}

int pps_conv2d_dual_bn_act(const float* x, int N, int H, int W, int Cin, int ldx,
                           int KH, int KW, int stride, int pad, const float* x2, int H2,
                           int W2, int Cin2, int ldx2, int stride2, const float* w,
                           int Cout, int Kpad1, int Kpad2, const float* shift, int relu,
                           float* y, int Ho, int Wo, int ldy, int tile, void* stream) {
  DualArgs a;
  PPS_DUAL_SHAPE(a);
  a.w = w;
  return dual_impl(a);
}

int pps_conv2d_dual_bn_act_x3(const float* x, int N, int H, int W, int Cin, int ldx,
                              int KH, int KW, int stride, int pad, const float* x2, int H2,
                              int W2, int Cin2, int ldx2, int stride2, const uint16_t* w3,
                              int Cout, int Kpad1, int Kpad2, const float* shift, int relu,
                              float* y, int Ho, int Wo, int ldy, int tile, void* stream) {
  DualArgs a;
  PPS_DUAL_SHAPE(a);
  a.w = w3; a.x3 = 1;
  return dual_impl(a);
}
#undef PPS_CONV_SHAPE
#undef PPS_DUAL_SHAPE

int pps_gemm_bn_act_batched(const float* x, int64_t x_bstride, int M, int K,
                            const float* w, int64_t w_bstride, int Cout,
                            const float* scale, const float* shift, int relu, float* y,
                            int ldy, int B, int tile, void* stream) {
  PPS_ENFORCE(x && w && scale && shift && y, "null pointer");
  PPS_ENFORCE(M > 0 && K > 0 && Cout > 0 && B > 0, "bad shape");
  PPS_ENFORCE(K % 16 == 0, "K must be a multiple of 16");
  PPS_ENFORCE(x_bstride % 4 == 0 && w_bstride % 4 == 0, "batch strides must be %4");
  PPS_ENFORCE(ldy >= B * Cout, "ldy < B*Cout");
  PPS_ENFORCE(aligned16(x) && aligned16(w), "x/w must be 16-byte aligned");
  GemmParams p{};
  p.splitk = 1;
  PPS_ENFORCE((int64_t)M * K * 4 < kMaxBufBytes && (int64_t)Cout * K * 4 < kMaxBufBytes,
              "operands larger than 2 GiB");
  p.a = x; p.a_bstride = x_bstride; p.H = 1; p.W = M; p.Cin = K; p.lda = K;
  p.a_bytes = (uint32_t)((int64_t)M * K * 4);
  p.b_bytes = (uint32_t)((int64_t)Cout * K * 4);
  p.KH = p.KW = 1; p.stride = 1; p.dil = 1; p.Ho = 1; p.Wo = M; p.M = M;
  p.b = w; p.b_bstride = w_bstride; p.ldb = K; p.kb_valid = K; p.Ncol = Cout;
  p.Kloop = K;
  p.scale = scale; p.shift = shift; p.ss_bstride = Cout;
  p.out = y; p.ldo = ldy; p.out_bstride = Cout; p.relu = relu; p.tile = tile;
  return launch_gemm(p, EPI_CONV, B, as_stream(stream));
}

int pps_gemm_splitk_batched(const float* x, int M, int K, const float* w, int Cout, int B,
                            int splitk, float* part, int tile, void* stream) {
  return splitk_impl(x, M, K, w, 0, Cout, B, splitk, part, tile, stream);
}

int pps_gemm_splitk_batched_x3(const float* x, int M, int K, const uint16_t* w3, int Cout,
                               int B, int splitk, float* part, int tile, void* stream) {
  return splitk_impl(x, M, K, w3, 1, Cout, B, splitk, part, tile, stream);
}

int pps_split_bf16x3(const float* x, int64_t n, int nbatch, uint16_t* out, void* stream) {
  PPS_ENFORCE(x && out, "null pointer");
  PPS_ENFORCE(n > 0 && nbatch > 0, "bad shape");
  return split_bf16x3(x, n, nbatch, out, as_stream(stream));
}

int pps_splitk_bn_act_normalize(const float* part, int splitk, int M, int N,
                                const float* scale, const float* shift, int relu,
                                int normalize, float* y, void* stream) {
  PPS_ENFORCE(part && scale && shift && y, "null pointer");
  PPS_ENFORCE(splitk >= 1 && M >= 0 && N > 0, "bad shape");
  return splitk_bn_act_normalize(part, splitk, (int64_t)M * N, M, N, scale, shift, relu,
                                 normalize, y, as_stream(stream));
}

int pps_maxpool2d(const float* x, int N, int H, int W, int C, int k, int stride, int pad,
                  float* y, int Ho, int Wo, void* stream) {
  PPS_ENFORCE(x && y, "null pointer");
  PPS_ENFORCE(C % 4 == 0, "C must be a multiple of 4");
  PPS_ENFORCE(Ho == (H + 2 * pad - k) / stride + 1 && Wo == (W + 2 * pad - k) / stride + 1,
              "output size does not match pooling arithmetic (floor)");
  PPS_ENFORCE(aligned16(x) && aligned16(y), "x/y must be 16-byte aligned");
  return maxpool2d(x, N, H, W, C, k, stride, pad, y, Ho, Wo, as_stream(stream), nullptr);
}

int pps_part_power_set(const float* x, int N, int H, int W, int C, const int32_t* splits,
                       int nstrip, int max_ave, float* out, void* stream) {
  PPS_ENFORCE(x && splits && out, "null pointer");
  PPS_ENFORCE(nstrip >= 1 && nstrip <= 10, "nstrip must be in [1, 10]");
  int sum = 0;
  for (int j = 0; j < nstrip; ++j) {
    PPS_ENFORCE(splits[j] > 0, "split heights must be positive");
    sum += splits[j];
  }
  PPS_ENFORCE(sum == H, "split heights must sum to H (Split axis=2)");
  return part_power_set(x, N, H, W, C, splits, nstrip, max_ave, out, as_stream(stream));
}

int pps_group_mean(const float* x, int D, const int32_t* offsets, const int32_t* members,
                   int ngroups, float* out, void* stream) {
  PPS_ENFORCE(x && offsets && members && out && D > 0 && ngroups >= 0, "bad arguments");
  return group_mean(x, D, offsets, members, ngroups, out, as_stream(stream));
}

int pps_l2_normalize(const float* x, int64_t N, int D, float* y, void* stream) {
  PPS_ENFORCE(x && y && D > 0 && N >= 0, "bad arguments");
  return l2_normalize(x, N, D, y, as_stream(stream));
}

int pps_preprocess_bgr(const uint8_t* img, int N, int Hi, int Wi, const float* means,
                       int Ho, int Wo, float* y, void* stream) {
  PPS_ENFORCE(img && means && y, "null pointer");
  PPS_ENFORCE(N >= 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "bad shape");
  PPS_ENFORCE(aligned16(y), "y must be 16-byte aligned");
  return preprocess_bgr(img, N, Hi, Wi, nullptr, nullptr, nullptr, means, Ho, Wo, y,
                        as_stream(stream));
}

int pps_preprocess_bgr_ragged(const uint8_t* blob, int N, const int64_t* offsets,
                              const int32_t* heights, const int32_t* widths,
                              const float* means, int Ho, int Wo, float* y, void* stream) {
  PPS_ENFORCE(blob && offsets && heights && widths && means && y, "null pointer");
  PPS_ENFORCE(N >= 0 && Ho > 0 && Wo > 0, "bad shape");
  PPS_ENFORCE(aligned16(y), "y must be 16-byte aligned");
  return preprocess_bgr(blob, N, 0, 0, offsets, heights, widths, means, Ho, Wo, y,
                        as_stream(stream));
}

}  // extern "C"
