// The retrieval side of libpps_hip.so: every internal function one translation
// unit calls in another (evaluation counts, top-k, row argsort, the
// single-gallery-shot CMC, re-ranking) and every capacity limit that both a
// kernel file and an entry-point guard (abi.hip, search_h2.hip) depend on --
// each named once, here.
#pragma once
#include "pps_internal.hpp"

namespace pps {

// ---- limits -------------------------------------------------------------------
// LDS per workgroup (this library is built for gfx950 only)
constexpr int kLdsBytesGfx950 = 160 * 1024;
constexpr int kTopkCap = 1024;       // topk: largest k
constexpr int kTkwMinRow = 16384;    // rows at least this long take topk_wave_kernel
constexpr int kTkwMaxK = 256;        // ... for k up to this (also the fused search's largest k)
constexpr int kMergeMaxLists = 64;   // topk_merge / rank_prepare: lists (shards) per query
// topk_merge keeps the R * k_in packed entries of a query in dynamic LDS (8 B each)
constexpr int kMergeMaxEntries = 8192;
constexpr int kRankCells = 1024;     // bin-lookup cells per query (pps_rank_cells)
// rank_count_stream / cmc_counts: gallery entries per workgroup (grid.y =
// chunks of a row, <= 65535)
constexpr int kRankStreamU = 8;      // float4 per thread in flight in the rank streams
constexpr int kRankStreamChunk = 256 * 4 * kRankStreamU;
// rank_prepare merges R*Pmax positives in dynamic LDS (4 int arrays):
// 16 B per merged positive, 128 KiB at the cap
constexpr int kRankMergeCap = 8192;
static_assert(16 * kRankMergeCap <= kLdsBytesGfx950, "rank_prepare LDS exceeds the CU's LDS");
// fused f16x2 kernels (search_h2.hip, rank_h2.hip): tile ids 0 = default (1),
// 1 = 256 x 256 two-stage, 2 = 192 x 192 three-stage
constexpr int kSearchNumTiles = 3;
constexpr int kSearchSlots = 256;    // workgroups launched at most: one per CU (LDS-bound residency)
// rank_count_h2 / cmc_count_h2: longest merged positive list (Ptot).  The kernel bins a pass
// of columns against the list with one ballot per positive; beyond the cap
// rank_count_stream's binary search on the matrix is the right algorithm
constexpr int kRankH2MaxP = 1024;
// sgs_groups keeps two int32 bounds per gallery identity in LDS (plus G / 4 bytes)
constexpr int kSgsMaxIds = 16384;
static_assert(8 * kSgsMaxIds <= kLdsBytesGfx950, "sgs_groups LDS exceeds the CU's LDS");

// ---- host plan of the fused f16x2 kernels (search_h2.hip, rank_h2.hip) ----------
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline void search_tile_shape(int tile, int& BM, int& BN) {
  if (tile == 2) { BM = 192; BN = 192; } else { BM = 256; BN = 256; }
}
// Gallery segments of a (query panel, gallery segment) work list before they
// are rounded to whole tiles per segment: the request, or (0 = auto) the count
// at which panels x S fills the CUs once or twice, whichever leaves the
// smaller idle tail; never more than the gallery's tiles.  Non-decreasing in G.
inline int64_t fused_segments(int64_t Q, int64_t G, int segments, int BM, int BN) {
  const int64_t panels = cdiv(Q, BM) > 1 ? cdiv(Q, BM) : 1;
  const int64_t tiles_n = cdiv(G, BN) > 1 ? cdiv(G, BN) : 1;
  int64_t S = segments;
  if (S <= 0) {
    const int64_t s1 = kSearchSlots / panels > 1 ? kSearchSlots / panels : 1;
    const int64_t s2 = 2 * kSearchSlots / panels > 1 ? 2 * kSearchSlots / panels : 1;
    auto fill = [&](int64_t s) {
      const int64_t items = panels * s;
      return (double)items / (double)(cdiv(items, kSearchSlots) * kSearchSlots);
    };
    S = fill(s2) > fill(s1) ? s2 : s1;
  }
  return S < tiles_n ? S : tiles_n;
}

// ---- chunk-tiled f16x2 operands: their GemmParams and the entry points' guards ---
// f16 elements of one plane of an operand of `rows` rows (padded to 16), and
// the bytes of its two planes
inline int64_t h2_plane_elems(int64_t rows, int D) { return (rows + 15) / 16 * 16 * D; }
inline int64_t h2_planes_bytes(int64_t rows, int D) { return 2 * h2_plane_elems(rows, D) * 2; }
// One operand: the chunk-tiled f16x2 planes of a row set with the rows' squared
// norms and scales.  head(m) is the first m rows of the same planes (a cell's
// bits do not depend on the rows around it).
struct H2Operand {
  const uint16_t* planes = nullptr;   // [2][plane_rows padded to 16][D]
  const float* sq = nullptr;          // squared norms
  const float* rs = nullptr;          // row scales
  int64_t rows = 0;                   // rows addressed
  int64_t plane_rows = 0;             // rows the planes hold (>= rows): decides the plane stride
  H2Operand head(int64_t m) const { return {planes, sq, rs, m, plane_rows}; }
  bool complete() const { return planes && sq && rs; }
};
// an entry point's (planes, norms, scales, rows): the planes hold exactly those rows
inline H2Operand h2_operand(const uint16_t* planes, const float* sq, const float* rs,
                            int64_t rows) {
  return {planes, sq, rs, rows, rows};
}
// The rows of a against the rows of b
inline GemmParams h2_params(const H2Operand& a, const H2Operand& b, int D, int metric,
                            float* out = nullptr, int64_t ldo = 0, int sym = 0) {
  GemmParams p{};
  p.splitk = 1;
  p.tiled = 3;
  p.a3 = a.planes; p.a_plane = h2_plane_elems(a.plane_rows, D);
  p.a_bytes = (uint32_t)h2_planes_bytes(a.plane_rows, D);
  p.M = (int)a.rows;
  p.b3 = b.planes; p.b_plane = h2_plane_elems(b.plane_rows, D);
  p.b_bytes = (uint32_t)h2_planes_bytes(b.plane_rows, D);
  p.Ncol = (int)b.rows;
  p.Kloop = D;
  p.norm_a = a.sq; p.norm_b = b.sq;
  p.rs_a = a.rs; p.rs_b = b.rs;
  p.out = out; p.ldo = ldo; p.metric = metric; p.sym = sym;
  return p;
}
// The checks of two operands (fn: the entry point's name).  The pointers are
// looked at only when both operands have rows: an entry returns early on an
// empty one, which may come with null pointers.
inline int h2_operands_guard(const char* fn, const H2Operand& q, const H2Operand& g, int D,
                             int metric) {
  const int64_t Q = q.rows, G = g.rows;
  PPS_ENFORCE_AS(fn, Q >= 0 && G >= 0 && D > 0 && D % 32 == 0, "bad shape (D % 32 == 0)");
  PPS_ENFORCE_AS(fn, Q < (1ll << 31), "Q must fit int32");
  PPS_ENFORCE_AS(fn, metric >= 0 && metric <= 2, "unknown metric");
  PPS_ENFORCE_AS(fn, h2_planes_bytes(Q, D) < kMaxBufBytes && h2_planes_bytes(G, D) < kMaxBufBytes,
                 "planes over 2 GiB");
  if (Q == 0 || G == 0) return PPS_OK;
  PPS_ENFORCE_AS(fn, q.complete() && g.complete(), "null pointer");
  PPS_ENFORCE_AS(fn, aligned16(q.planes) && aligned16(g.planes), "planes must be 16-byte aligned");
  return PPS_OK;
}
// segments / tile of the fused kernels' work list
inline int fused_plan_guard(const char* fn, int segments, int tile) {
  PPS_ENFORCE_AS(fn, segments >= 0, "segments must be >= 0 (0 = auto)");
  PPS_ENFORCE_AS(fn, tile >= 0 && tile < kSearchNumTiles,
                 "search tile must be 0.." + std::to_string(kSearchNumTiles - 1));
  return PPS_OK;
}

// ---- fused f16x2 entries other translation units call --------------------------
// byte offset of row r's chunk 0, slot s within a chunk-tiled f16 plane:
// [r / 16][kc][r % 16][32]
__device__ inline int64_t h2_frag_off(int r, int nkc, int slot) {
  return (int64_t)(r >> 4) * nkc * 1024 + (r & 15) * 64 + slot * 16;
}
// search_h2.hip: the body of pps_search_h2_tiled / _excl / _rowmax (guards
// included; fn names the entry in its messages; rowmax null = not wanted)
int search_h2_tiled(const char* fn, bool excl, const H2Operand& q, const H2Operand& g, int D,
                    int metric, int k, int segments, int tile, void* workspace, int64_t ws_bytes,
                    float* vals, int32_t* idx, const int32_t* q_group, const int32_t* g_group,
                    float* rowmax, void* stream);
// bytes that hold the workspace of a search of N rows against themselves, as a
// bound that is non-decreasing in N (host arithmetic)
int64_t search_h2_self_workspace_bound(int64_t N, int k, int segments);
// search_h2.hip: the same for Q a-rows against G b-rows: at least the search's
// workspace, non-decreasing in Q and in G
int64_t search_h2_workspace_bound(int64_t Q, int64_t G, int k, int segments);
// pair_h2.hip: out[r][t] = distance of q's row r to g's row lists[r][t], t <
// min(counts[r], cap) (lists / out rows cap apart; counts null = cap each)
int pair_dist_h2(const H2Operand& q, const H2Operand& g, int D, int metric, const int32_t* lists,
                 const int32_t* counts, int cap, float* out, hipStream_t st);
// pair_h2.hip: pair_dist_h2 with the b-rows in two operands: a list index
// < b0.rows is that row of b0, any other index row (index - b0.rows) of b1;
// indices are clamped to [0, b0.rows + b1.rows)
int pair_dist_h2_parts(const H2Operand& q, const H2Operand& b0, const H2Operand& b1, int D,
                       int metric, const int32_t* lists, const int32_t* counts, int cap,
                       float* out, hipStream_t st);
// pair_h2.hip: the [a.rows, b.rows] block of a (often the head of longer
// planes) against a whole b (pps_distmat_h2_tiled's launch and bits)
int distmat_h2_head(const H2Operand& a, const H2Operand& b, int D, int metric, float* out,
                    int64_t ldo, hipStream_t st);

// ---- evaluation counts (eval_counts.hip) ----------------------------------------
int collect_matches(const float* dist, int64_t Q, int64_t ldd, const int32_t* qcam,
                    const int32_t* gcam, const int32_t* members, const int32_t* q_beg,
                    const int32_t* q_end, int64_t g_offset, int Pmax, float* pos_d,
                    int32_t* pos_idx, int32_t* pos_cnt, int Jmax, float* junk_d,
                    int32_t* junk_idx, int32_t* junk_cnt, hipStream_t st);
int rank_prepare(int R, int64_t Q, int Pmax, const float* pos_d, const int32_t* pos_idx,
                 const int32_t* pos_cnt, float* sorted_d, int32_t* sorted_idx,
                 int32_t* pos_total, int32_t* cells, hipStream_t st);
int rank_count_stream(const float* dist, int64_t Q, int64_t G, int64_t ldd, int64_t g_offset,
                      int Ptot, const float* sorted_d, const int32_t* sorted_idx,
                      const int32_t* pos_total, const int32_t* cells, int Jmax, const float* junk_d,
                      const int32_t* junk_idx, const int32_t* junk_cnt, int32_t* hist,
                      int32_t* before, hipStream_t st);
int ap_finalize(int64_t Q, int Ptot, const float* sorted_d, const int32_t* pos_total,
                const int32_t* hist, const int32_t* before, double* ap, int32_t* valid,
                int32_t* first_rank, hipStream_t st);
int cmc_counts(const float* dist, int64_t Q, int64_t G, int64_t ldd, int64_t g_offset, int Ptot,
               const float* sorted_d, const int32_t* sorted_idx, const int32_t* pos_total,
               const int32_t* qcam, const int32_t* gcam, int Jmax, const float* junk_d,
               const int32_t* junk_idx, const int32_t* junk_cnt, int32_t* hist,
               hipStream_t st);
int cmc_finalize(int64_t Q, int Ptot, const int32_t* pos_total, const int32_t* hist, int topk,
                 int fmb, double* ret, int32_t* valid, hipStream_t st);

// ---- stable top-k (topk.hip) ----------------------------------------------------
int topk(const float* dist, int64_t Q, int64_t G, int64_t ldd, int k, float* vals,
         int32_t* idx, hipStream_t st);
struct MergeOffsets {  // kernel-argument copy of the per-list global offsets
  int64_t off[kMergeMaxLists];
};
int topk_merge(const float* vals, const int32_t* idx, int R, int64_t Q, int kin,
               const MergeOffsets& offs, int kout, float* out_vals, int32_t* out_idx,
               hipStream_t st);

// ---- row argsort (rowsort.hip) --------------------------------------------------
int argsort_rows(const float* dist, int64_t Q, int64_t G, int64_t ldd, int32_t* idx,
                 int64_t ldi, float* vals, int64_t ldv, hipStream_t st);
int argsort_rows_cap();

// ---- CMC with single_gallery_shot (cmc_sgs.hip) ---------------------------------
int sgs_keys(const int32_t* order, int64_t Q, int64_t G, int64_t ldo, const int32_t* gid,
             const int32_t* gcam, const int32_t* qid, const int32_t* qcam, int sep, int U,
             float* keys, hipStream_t st);
int sgs_groups(const float* skeys, const int32_t* perm, int64_t Q, int64_t G, int U,
               const int32_t* qid, int32_t* gstart, int32_t* glen, int32_t* nids, int32_t* qt,
               hipStream_t st);
int sgs_ranks(const int32_t* perm, int64_t G, const int32_t* rows, int64_t nr,
              const int32_t* gstart, const int32_t* glen, const int32_t* nids, const int32_t* qt,
              int U, int repeat, const int32_t* draws, int64_t ldd, int32_t* kout,
              hipStream_t st);
size_t sgs_groups_lds_bytes(int64_t G, int U);

// ---- re-ranking (rerank.hip) -------------------------------------------------
// The row capacities of a (k1, k2) configuration: neighbours kept per row
// (K1), half-size neighbourhoods (Kh), entries of a V row (vcap) and of a V_qe
// row (qcap)
struct RrLayout {
  int K1, Kh, vbound, vcap, qcap;
  RrLayout(int k1, int k2) {
    K1 = k1 + 1;
    Kh = (int)lrint(k1 / 2.0) + 1;  // int(np.around(k1 / 2.)) + 1
    vbound = K1 + K1 * Kh;
    vcap = vbound <= 256 ? 256 : (vbound <= 512 ? 512 : 1024);
    qcap = k2 * vcap;
  }
};
// The limits of that layout (k1 >= 1 checked by the entry, with its own bound)
inline int rr_layout_guard(const char* fn, int k1, int k2) {
  PPS_ENFORCE_AS(fn, k2 >= 1 && k2 <= k1 + 1, "k2 must be in [1, k1 + 1]");
  const RrLayout L(k1, k2);
  PPS_ENFORCE_AS(fn, L.vbound <= 1024, "expansion bound (k1+1)(round(k1/2)+2) must be <= 1024");
  PPS_ENFORCE_AS(fn, L.qcap <= 4096, "k2 * V row capacity must be <= 4096");
  return PPS_OK;
}
int rerank(const float* qg, int64_t ldqg, const float* qq, int64_t ldqq, const float* gg,
           int64_t ldgg, int64_t Q, int64_t G, int k1, int k2, double lambda, void* ws,
           size_t ws_bytes, float* out, hipStream_t st, int flags);
size_t rerank_workspace_bytes(int64_t Q, int64_t G, int k1, int k2);
size_t rerank_workspace_bytes_for(const float* qg, int64_t ldqg, const float* qq, int64_t ldqq,
                                  const float* gg, int64_t ldgg, int64_t Q, int64_t G, int k1,
                                  int k2, int flags);
// dynamic LDS of the Jaccard pass for a gallery of G
size_t jaccard_lds_bytes(int64_t G);
// Row-form re-ranking: OD(i, j) = rr_od(W[i][j], rowmax[i]) with
// W[i][j] the general h2 kernel's value for a-row x_i, b-row x_j.  The OD
// provider: W itself (the materialised twin), or the planes of x = [queries;
// gallery] and of the gallery alone (the features path: no N x N buffer).
constexpr int kJacMaxWindow = 38400;   // gallery rows of one Jaccard window (tm in LDS)
struct RrRows {
  const float* W;            // twin: [N][ldw]; null = the features path
  int64_t ldw;
  H2Operand x;               // features: x = [queries; gallery] (N rows)
  H2Operand g;               // the gallery rows' own planes (rows Q.. of x)
  int D, metric, segments, tile;
};
int rerank_rows(const RrRows& src, int64_t Q, int64_t G, int k1, int k2, double lambda,
                int64_t g_window, void* ws, size_t ws_bytes, float* out, hipStream_t st);
// bytes of the workspace; features: the fused search's workspace included
int64_t rerank_rows_workspace_bytes(bool features, int64_t Q, int64_t G, int k1, int k2,
                                    int segments);

// Row form against a gallery prepared once: the queries' planes
// and the gallery's are separate operands, and the gallery rows' top-(k1 + 1)
// over the gallery columns (nn_vals / nn_idx, rows nn_ld apart, gallery
// numbering) and their row maxima (g_rowmax) come from the caller -- one
// pps_search_h2_tiled_rowmax of the gallery against itself, whatever the
// queries.  Bit for bit rerank_rows on the planes of [queries; gallery].
struct RrPrepared {
  H2Operand q, g;            // Q rows, G rows
  const float* nn_vals; const int32_t* nn_idx; int nn_ld;
  const float* g_rowmax;
  int D, metric, segments, tile;
};
int rerank_prepared(const RrPrepared& src, int64_t Q, int64_t G, int k1, int k2, double lambda,
                    int64_t g_window, void* ws, size_t ws_bytes, float* out, hipStream_t st);
int64_t rerank_prepared_workspace_bytes(int64_t Q, int64_t G, int k1, int k2, int segments);

// OD's arithmetic, float32 as NumPy does it (np.power(M, 2) then / colmax):
// (m * m) / cm, both rounded (a product feeding a division cannot fuse), the
// same expression in every kernel that computes it so that all give the same bits
__device__ inline float rr_od(float m, float cm) { return (m * m) / cm; }

// The concatenated distance matrix M = [[q_q, q_g], [q_g^T, g_g]]
// (reid_dataset_evaluator.py:447-452) read in place from its blocks (row
// strides ld*; qgT = q_g transposed, [G][ldT]), and for a SYMMETRIC M (q_q,
// g_g exactly symmetric) the normalised square of :452-454,
// OD[i][j] = M[j][i]^2 / colmax[i] = M[i][j]^2 / colmax[i], computed on the fly
// with the arithmetic of the OD-building kernels (rr_od).
struct RrMatrix {
  const float* qg;
  const float* qq;
  const float* gg;
  const float* qgT;
  int64_t ldqg, ldqq, ldgg, ldT, Q, G;
  const float* colmax;
  __device__ float m(int64_t r, int64_t c) const {
    if (r < Q) return c < Q ? qq[r * ldqq + c] : qg[r * ldqg + (c - Q)];
    return c < Q ? qgT[(r - Q) * ldT + c] : gg[(r - Q) * ldgg + (c - Q)];
  }
  __device__ float od(int64_t i, int64_t j) const {
    return rr_od(m(i, j), colmax[i]);
  }
};
// stable (value, index) top-k of every row of OD (symmetric M, rows of N =
// Q + G >= kTkwMinRow entries, every block 16-byte aligned): the wave-streaming
// top-k reading M's blocks in place (no N x N OD buffer)
int topk_rr(const RrMatrix& M, int k, float* vals, int32_t* idx, hipStream_t st);
// symmetric M with colmax not yet known: rowmax[q] = max of row q's squares
// (= column q's), and the top-k by (OD, index) through a top-(k+8) on m * m
// (topk.hip); scratch of topk_rr_sq_scratch_bytes(N, k)
int topk_rr_sq(const RrMatrix& M, int k, float* rowmax, void* scratch, size_t scratch_bytes,
               float* vals, int32_t* idx, hipStream_t st);
size_t topk_rr_sq_scratch_bytes(int64_t N, int k);
bool topk_rr_eligible(const RrMatrix& M, int k);

}  // namespace pps
