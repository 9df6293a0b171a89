// Retrieval ranking and evaluation kernels.
//
// The reference sorts every query row (np.argsort, reid_dataset_evaluator.py
// :319,:420) and then walks it in Python.  mAP and CMC only need, for each
// true match p of a query, how many valid gallery entries rank before it, so
// these kernels compute exactly that by counting against the (few) positives'
// distances -- one streaming read of the distance row, no sort.  The result
// equals a stable (distance, gallery index) sort; counts are additive over
// gallery shards, which is what the multi-GPU path all-reduces.
#include "gemm_common.hpp"
#include "retrieval.hpp"

namespace pps {

constexpr int kEvalThreads = 256;

// the stable (distance, global index) order of the positives
__device__ inline bool key_less(float da, int ia, float db, int ib) {
  return da < db || (da == db && ia < ib);
}

// ---- streaming evaluation from a per-identity gallery index ---------------------
// The product path (v2).  A CSR index of the gallery (host-built once from the
// ids: `members` = local gallery indices sorted by (id, index); the query's
// identity occupies members[q_beg[q], q_end[q])) lets every query list its
// true matches directly -- tens of gathers instead of a scan of all G ids and
// cams -- split into positives (other camera) and junk (same camera,
// reid_dataset_evaluator.py:427-428).  The counting pass then needs no ids at
// all: it bins EVERY entry of the distance row against the sorted positives
// and afterwards takes the junk entries (known, few) back out, so the row is
// one pure 16-byte-vector stream of distances.
//
// a) collect_matches: one wave per query.
constexpr int kMatchWaves = 4;
__global__ void __launch_bounds__(64 * kMatchWaves)
collect_matches_kernel(const float* __restrict__ dist, int64_t Q, int64_t ldd,
                       const int32_t* __restrict__ qcam, const int32_t* __restrict__ gcam,
                       const int32_t* __restrict__ members,
                       const int32_t* __restrict__ q_beg, const int32_t* __restrict__ q_end,
                       int64_t g_offset, int Pmax, float* __restrict__ pos_d,
                       int32_t* __restrict__ pos_idx, int32_t* __restrict__ pos_cnt, int Jmax,
                       float* __restrict__ junk_d, int32_t* __restrict__ junk_idx,
                       int32_t* __restrict__ junk_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * kMatchWaves + (threadIdx.x >> 6);
  if (q >= Q) return;
  const int beg = q_beg[q], end = q_end[q], qc = qcam[q];
  const float* row = dist + q * ldd;
  const unsigned long long below = (1ull << lane) - 1ull;
  int np = 0, nj = 0;
  for (int m0 = beg; m0 < end; m0 += 64) {
    const int m = m0 + lane;
    const bool in = m < end;
    const int idx = in ? members[m] : 0;
    const bool pos = in && gcam[idx] != qc;
    const bool junk = in && !pos;
    const float d = in ? row[idx] : 0.f;
    const unsigned long long bp = __ballot(pos), bj = __ballot(junk);
    const int sp = np + __popcll(bp & below), sj = nj + __popcll(bj & below);
    if (pos && sp < Pmax) {
      pos_d[q * Pmax + sp] = d;
      pos_idx[q * Pmax + sp] = (int32_t)(g_offset + idx);
    }
    if (junk && sj < Jmax) {
      junk_d[q * Jmax + sj] = d;
      junk_idx[q * Jmax + sj] = (int32_t)(g_offset + idx);
    }
    np += __popcll(bp);
    nj += __popcll(bj);
  }
  if (lane == 0) {
    pos_cnt[q] = np;
    junk_cnt[q] = nj;
  }
}

int collect_matches(const float* dist, int64_t Q, int64_t ldd, const int32_t* qcam,
                    const int32_t* gcam, const int32_t* members, const int32_t* q_beg,
                    const int32_t* q_end, int64_t g_offset, int Pmax, float* pos_d,
                    int32_t* pos_idx, int32_t* pos_cnt, int Jmax, float* junk_d,
                    int32_t* junk_idx, int32_t* junk_cnt, hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  const unsigned grid = (unsigned)((Q + kMatchWaves - 1) / kMatchWaves);
  hipLaunchKernelGGL(collect_matches_kernel, dim3(grid), dim3(64 * kMatchWaves), 0, st, dist,
                     Q, ldd, qcam, gcam, members, q_beg, q_end, g_offset, Pmax, pos_d, pos_idx,
                     pos_cnt, Jmax, junk_d, junk_idx, junk_cnt);
  PPS_CHECK_LAUNCH("collect_matches_kernel");
  return PPS_OK;
}

// Bin-lookup cells of a query (used by c)): (df, dmax] of its sorted positives
// cut into kStreamCells equal cells by a monotone map; cells[c] = the number
// of positives whose cell is below c, | kCellDirty if a positive lies in c.
constexpr int kStreamCells = kRankCells;
constexpr int kCellDirty = 1 << 30;
__device__ inline float cell_scale(float df, float dmax) {
  const float span = dmax - df;
  const float inv = span > 0.f ? (float)kStreamCells / span : 0.f;
  return isfinite(inv) ? inv : 0.f;  // a denormal span: one cell
}
__device__ inline int cell_of(float d, float df, float inv) {
  const float t = (d - df) * inv;
  const int c = t < (float)(kStreamCells - 1) ? (int)t : kStreamCells - 1;
  return c > 0 ? c : 0;
}

// b) rank_prepare: merge the R shards' positive lists of a query and sort
// them by (distance, global index) -- rank by counting in LDS (one block per
// query; tens of entries on real splits) -- and build its bin-lookup cells.
__global__ void rank_prepare_kernel(int R, int64_t Q, int Pmax, const float* __restrict__ pos_d,
                                    const int32_t* __restrict__ pos_idx,
                                    const int32_t* __restrict__ pos_cnt,
                                    float* __restrict__ sorted_d,
                                    int32_t* __restrict__ sorted_idx,
                                    int32_t* __restrict__ pos_total,
                                    int32_t* __restrict__ cells) {
  const int64_t q = blockIdx.x;
  const int Ptot = R * Pmax;
  extern __shared__ int plds[];
  float* ud = reinterpret_cast<float*>(plds);
  int* ui = plds + Ptot;
  float* sd = reinterpret_cast<float*>(plds + 2 * Ptot);
  int* ct = plds + 3 * Ptot;
  __shared__ int offs[kMergeMaxLists + 1];
  if (threadIdx.x == 0) {
    int o = 0;
    for (int r = 0; r < R; ++r) {
      offs[r] = o;
      const int c = pos_cnt[(int64_t)r * Q + q];
      o += c < Pmax ? c : Pmax;
    }
    offs[R] = o;
  }
  __syncthreads();
  const int P = offs[R];
  for (int r = 0; r < R; ++r) {
    const int n = offs[r + 1] - offs[r];
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
      ud[offs[r] + p] = pos_d[((int64_t)r * Q + q) * Pmax + p];
      ui[offs[r] + p] = pos_idx[((int64_t)r * Q + q) * Pmax + p];
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    const float d = ud[p];
    const int ix = ui[p];
    int rk = 0;
    for (int o = 0; o < P; ++o) rk += key_less(ud[o], ui[o], d, ix) ? 1 : 0;
    sorted_d[q * Ptot + rk] = d;
    sorted_idx[q * Ptot + rk] = ix;
    sd[rk] = d;
  }
  for (int p = P + threadIdx.x; p < Ptot; p += blockDim.x) {
    sorted_d[q * Ptot + p] = INFINITY;
    sorted_idx[q * Ptot + p] = -1;
  }
  if (threadIdx.x == 0) pos_total[q] = P;
  if (P == 0) return;  // uniform: the count pass skips this query
  __syncthreads();
  const float df = sd[0], inv = cell_scale(df, sd[P - 1]);
  for (int p = threadIdx.x; p < P; p += blockDim.x) ct[p] = cell_of(sd[p], df, inv);
  __syncthreads();
  for (int c = threadIdx.x; c < kStreamCells; c += blockDim.x) {
    int lo = 0, hi = P;  // first positive whose cell is >= c (ct is non-decreasing)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ct[mid] < c) lo = mid + 1; else hi = mid;
    }
    cells[q * kStreamCells + c] = lo | ((lo < P && ct[lo] == c) ? kCellDirty : 0);
  }
}

// b') rank_prepare for merged lists longer than the LDS merge holds (R*Pmax
// > kRankMergeCap: an identity with thousands of gallery entries per shard).
// The query's lists are copied into its output row (sorted_d / sorted_idx,
// padding +inf / -1 past P) and sorted there in place by the block: a
// bitonic network for any length -- the first compare of each merge step
// mirrors inside the block (i <-> block end - 1 - i), the rest are half-
// cleaners, every compare puts the smaller (distance, index) key first and
// partners at or past P are skipped (they act as +inf at the end) -- over
// the L2-resident row, one block barrier per stage.  Keys are unique
// (global indices), so the order is the LDS path's.  Then the bin-lookup
// cells from the sorted row (the positive's cell computed on the fly).
__global__ void rank_prepare_global_kernel(int R, int64_t Q, int Pmax,
                                           const float* __restrict__ pos_d,
                                           const int32_t* __restrict__ pos_idx,
                                           const int32_t* __restrict__ pos_cnt,
                                           float* __restrict__ sorted_d,
                                           int32_t* __restrict__ sorted_idx,
                                           int32_t* __restrict__ pos_total,
                                           int32_t* __restrict__ cells) {
  const int64_t q = blockIdx.x;
  const int64_t Ptot = (int64_t)R * Pmax;
  __shared__ int offs[kMergeMaxLists + 1];
  if (threadIdx.x == 0) {
    int o = 0;
    for (int r = 0; r < R; ++r) {
      offs[r] = o;
      const int c = pos_cnt[(int64_t)r * Q + q];
      o += c < Pmax ? c : Pmax;
    }
    offs[R] = o;
  }
  __syncthreads();
  const int P = offs[R];
  float* gd = sorted_d + q * Ptot;
  int32_t* gi = sorted_idx + q * Ptot;
  for (int r = 0; r < R; ++r) {
    const int n = offs[r + 1] - offs[r];
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
      gd[offs[r] + p] = pos_d[((int64_t)r * Q + q) * Pmax + p];
      gi[offs[r] + p] = pos_idx[((int64_t)r * Q + q) * Pmax + p];
    }
  }
  for (int64_t p = P + threadIdx.x; p < Ptot; p += blockDim.x) {
    gd[p] = INFINITY;
    gi[p] = -1;
  }
  if (threadIdx.x == 0) pos_total[q] = P;
  if (P == 0) return;  // uniform
  __syncthreads();
  auto cas = [&](int i, int j) {  // i < j: the smaller key to i
    const float di = gd[i], dj = gd[j];
    const int ii = gi[i], ij = gi[j];
    if (key_less(dj, ij, di, ii)) {
      gd[i] = dj; gi[i] = ij;
      gd[j] = di; gi[j] = ii;
    }
  };
  int n2 = 1;
  while (n2 < P) n2 <<= 1;
  for (int size = 2; size <= n2; size <<= 1) {
    const int half = size >> 1;
    for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {  // mirror step
      const int b = t / half, o = t - b * half;
      const int i = b * size + o, j = b * size + size - 1 - o;
      if (j < P) cas(i, j);
    }
    __syncthreads();
    for (int stride = half >> 1; stride > 0; stride >>= 1) {  // half-cleaners
      for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
        const int b = t / stride, o = t - b * stride;
        const int i = 2 * b * stride + o, j = i + stride;
        if (j < P) cas(i, j);
      }
      __syncthreads();
    }
  }
  const float df = gd[0], inv = cell_scale(df, gd[P - 1]);
  for (int c = threadIdx.x; c < kStreamCells; c += blockDim.x) {
    int lo = 0, hi = P;  // first positive whose cell is >= c (non-decreasing in p)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cell_of(gd[mid], df, inv) < c) lo = mid + 1; else hi = mid;
    }
    cells[q * kStreamCells + c] = lo | ((lo < P && cell_of(gd[lo], df, inv) == c) ? kCellDirty : 0);
  }
}

int rank_prepare(int R, int64_t Q, int Pmax, const float* pos_d, const int32_t* pos_idx,
                 const int32_t* pos_cnt, float* sorted_d, int32_t* sorted_idx,
                 int32_t* pos_total, int32_t* cells, hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  if ((int64_t)R * Pmax > kRankMergeCap) {
    hipLaunchKernelGGL(rank_prepare_global_kernel, dim3((unsigned)Q), dim3(kEvalThreads), 0, st,
                       R, Q, Pmax, pos_d, pos_idx, pos_cnt, sorted_d, sorted_idx, pos_total,
                       cells);
    PPS_CHECK_LAUNCH("rank_prepare_global_kernel");
    return PPS_OK;
  }
  const size_t lds = (size_t)4 * R * Pmax * sizeof(int);
  hipLaunchKernelGGL(rank_prepare_kernel, dim3((unsigned)Q), dim3(kEvalThreads), lds, st, R,
                     Q, Pmax, pos_d, pos_idx, pos_cnt, sorted_d, sorted_idx, pos_total, cells);
  PPS_CHECK_LAUNCH("rank_prepare_kernel");
  return PPS_OK;
}

// c) rank_count_stream: grid (query, row chunk).  Each block streams its chunk
// of the row as 16-byte vectors (kStreamU in flight per thread), bins the
// entries closer than the farthest positive against the sorted positives
// (binary search, LDS histogram), counts the entries ordered before the
// first positive, takes this shard's junk entries back out (chunk 0), and
// adds its counts to hist / before with one global atomic per non-empty bin.
// KLDS = false: positive lists too long for LDS are searched in global memory
// (L2) and binned with global atomics -- no capacity limit.
constexpr int kStreamThreads = 256;
constexpr int kStreamU = kRankStreamU;                       // float4 per thread in flight
constexpr int kStreamChunk = kStreamThreads * kStreamU * 4;  // 8192 entries per block
static_assert(kStreamChunk == kRankStreamChunk, "retrieval.hpp kRankStreamChunk");
constexpr int kStreamLdsCap = 6144;                          // positives held in LDS

template <bool KLDS>
__global__ void __launch_bounds__(kStreamThreads)
rank_count_stream_kernel(const float* __restrict__ dist, int64_t G, int64_t ldd,
                         int64_t g_offset, int Ptot, const float* __restrict__ sorted_d,
                         const int32_t* __restrict__ sorted_idx,
                         const int32_t* __restrict__ pos_total,
                         const int32_t* __restrict__ cells, int Jmax,
                         const float* __restrict__ junk_d,
                         const int32_t* __restrict__ junk_idx,
                         const int32_t* __restrict__ junk_cnt, int32_t* __restrict__ hist,
                         int32_t* __restrict__ before) {
  const int64_t q = blockIdx.x;
  const int P = pos_total[q];
  if (P == 0) return;
  extern __shared__ int slds[];
  const float* gsd = sorted_d + q * Ptot;
  int32_t* ghist = hist + q * Ptot;
  const int Pa = (P + 3) & ~3;  // keeps the cell arrays 16-byte aligned
  float* sd = reinterpret_cast<float*>(slds);
  int* hs = slds + (KLDS ? Pa : 0);
  int* cs = slds + (KLDS ? 2 * Pa : 0);  // bin-lookup cells (rank_prepare)
  int* cc = cs + kStreamCells;          // per-cell entry counts (clean cells)
  __shared__ int red[kStreamThreads / 64];
  const float df = gsd[0], dmax = gsd[P - 1];
  // Binning without a per-entry binary search: a "clean" cell holds no
  // positive, so every entry in it has bin cs[c] exactly and only bumps the
  // cell's counter cc[c] (1024 addresses: a wave's LDS atomics rarely collide;
  // with one counter per positive they serialised).  A cell holding
  // positives finishes the lower_bound with a short forward scan from cs[c].
  // The clean-cell counts are folded into the positives' bins once per block.
  const float inv = cell_scale(df, dmax);
  if (KLDS) {
    for (int p = threadIdx.x; p < P; p += kStreamThreads) {
      sd[p] = gsd[p];
      hs[p] = 0;
    }
    const int4* gc = reinterpret_cast<const int4*>(cells + q * kStreamCells);
    for (int c = threadIdx.x; c < kStreamCells / 4; c += kStreamThreads) {
      reinterpret_cast<int4*>(cs)[c] = gc[c];
      reinterpret_cast<int4*>(cc)[c] = make_int4(0, 0, 0, 0);
    }
    __syncthreads();
  }
  const float* S = KLDS ? sd : gsd;
  const int64_t idf = sorted_idx[q * Ptot];
  auto bin = [&](float d) {  // lower_bound(S, d) for d <= dmax: < P
    int lo = 0, hi = P;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (S[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  auto add = [&](int b, int v) {
    if (KLDS) atomicAdd(&hs[b], v); else atomicAdd(&ghist[b], v);
  };
  int nb = 0;
  auto visit = [&](int64_t i, float d) {
    if (d <= dmax) {
      if (d <= df) {  // bin 0; the only entries that can precede the first positive
        add(0, 1);
        nb += (d < df || g_offset + i < idf) ? 1 : 0;
      } else if (KLDS) {
        const int c = cell_of(d, df, inv);
        const int e = cs[c];
        if (e & kCellDirty) {
          int b = e & (kCellDirty - 1);
          while (S[b] < d) ++b;
          atomicAdd(&hs[b], 1);
        } else {
          atomicAdd(&cc[c], 1);
        }
      } else {
        add(bin(d), 1);
      }
    }
  };
  const int64_t c0 = (int64_t)blockIdx.y * kStreamChunk;
  const int64_t c1 = c0 + kStreamChunk < G ? c0 + kStreamChunk : G;
  const float* row = dist + q * ldd;
  if (((reinterpret_cast<uintptr_t>(row) & 15) == 0)) {
    // 16-byte rows: the chunk [c0, c1) starts on a vector boundary
    const f32x4* v4 = reinterpret_cast<const f32x4*>(row + c0);
    const int nv = (int)((c1 - c0) >> 2);
    f32x4 v[kStreamU];
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) {
      const int j = threadIdx.x + u * kStreamThreads;
      // streamed once: non-temporal, so the row does not evict useful L2 lines
      v[u] = j < nv ? __builtin_nontemporal_load(v4 + j) : f32x4{INFINITY, INFINITY, INFINITY,
                                                                  INFINITY};
    }
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) {
      const int64_t i = c0 + 4 * (int64_t)(threadIdx.x + u * kStreamThreads);
      visit(i, v[u].x);
      visit(i + 1, v[u].y);
      visit(i + 2, v[u].z);
      visit(i + 3, v[u].w);
    }
    const int64_t t = c0 + 4 * (int64_t)nv + threadIdx.x;
    if (t < c1) visit(t, row[t]);
  } else {
    float v[4 * kStreamU];
#pragma unroll
    for (int u = 0; u < 4 * kStreamU; ++u) {
      const int64_t i = c0 + threadIdx.x + (int64_t)u * kStreamThreads;
      v[u] = i < c1 ? row[i] : INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4 * kStreamU; ++u)
      visit(c0 + threadIdx.x + (int64_t)u * kStreamThreads, v[u]);
  }
  if (blockIdx.y == 0) {  // junk entries of this shard were binned above: take them out
    const int nj = junk_cnt[q] < Jmax ? junk_cnt[q] : Jmax;
    for (int j = threadIdx.x; j < nj; j += kStreamThreads) {
      const float d = junk_d[q * Jmax + j];
      if (d <= dmax) {
        add(bin(d), -1);
        nb -= (d < df || (d == df && (int64_t)junk_idx[q * Jmax + j] < idf)) ? 1 : 0;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nb;
  __syncthreads();
  if (KLDS) {
    for (int c = threadIdx.x; c < kStreamCells; c += kStreamThreads)
      if (cc[c]) atomicAdd(&hs[cs[c] & (kCellDirty - 1)], cc[c]);
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += kStreamThreads)
      if (hs[p]) atomicAdd(&ghist[p], hs[p]);
  }
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kStreamThreads / 64; ++w) s += red[w];
    if (s) atomicAdd(&before[q], s);
  }
}

int rank_count_stream(const float* dist, int64_t Q, int64_t G, int64_t ldd, int64_t g_offset,
                      int Ptot, const float* sorted_d, const int32_t* sorted_idx,
                      const int32_t* pos_total, const int32_t* cells, int Jmax, const float* junk_d,
                      const int32_t* junk_idx, const int32_t* junk_cnt, int32_t* hist,
                      int32_t* before, hipStream_t st) {
  if (Q <= 0 || G <= 0) return PPS_OK;
  const int64_t nchunk = (G + kStreamChunk - 1) / kStreamChunk;
  for (int64_t q0 = 0; q0 < Q; q0 += 65535) {  // grid.x limit
    const int64_t qn = Q - q0 < 65535 ? Q - q0 : 65535;
    const dim3 grid((unsigned)qn, (unsigned)nchunk);
    const float* d = dist + q0 * ldd;
    if (Ptot <= kStreamLdsCap) {
      hipLaunchKernelGGL(rank_count_stream_kernel<true>, grid, dim3(kStreamThreads),
                         (size_t)(2 * ((Ptot + 3) & ~3) + 2 * kStreamCells) * sizeof(int), st,
                         d, G, ldd,
                         g_offset, Ptot,
                         sorted_d + q0 * Ptot, sorted_idx + q0 * Ptot, pos_total + q0,
                         cells + q0 * kStreamCells, Jmax, junk_d + q0 * Jmax, junk_idx + q0 * Jmax, junk_cnt + q0,
                         hist + q0 * Ptot, before + q0);
    } else {
      hipLaunchKernelGGL(rank_count_stream_kernel<false>, grid, dim3(kStreamThreads), 0, st, d,
                         G, ldd, g_offset, Ptot, sorted_d + q0 * Ptot, sorted_idx + q0 * Ptot,
                         pos_total + q0, cells + q0 * kStreamCells, Jmax, junk_d + q0 * Jmax, junk_idx + q0 * Jmax,
                         junk_cnt + q0, hist + q0 * Ptot, before + q0);
    }
    PPS_CHECK_LAUNCH("rank_count_stream_kernel");
  }
  return PPS_OK;
}

// ---- 3) AP / first-match finalisation -----------------------------------------
// One wave per query.  le[p] = prefix sum of hist (valid entries with
// d <= d_p); pos_le[p] = #positives with d <= d_p (upper bound, so tied
// positives share the precision at the end of their tie group, as sklearn's
// precision_recall_curve does on distinct thresholds).
__global__ void ap_finalize_kernel(int64_t Q, int Ptot, const float* __restrict__ sorted_d,
                                   const int32_t* __restrict__ pos_total,
                                   const int32_t* __restrict__ hist,
                                   const int32_t* __restrict__ before,
                                   double* __restrict__ ap, int32_t* __restrict__ valid,
                                   int32_t* __restrict__ first_rank) {
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const int P = pos_total[q];
  const float* sd = sorted_d + q * Ptot;
  const int32_t* hq = hist + q * Ptot;
  double acc = 0.0;
  int carry = 0;
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    int v = p < P ? hq[p] : 0;
    // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    const int le = carry + v;
    carry += __shfl(v, 63);
    if (p < P) {
      const float d = sd[p];
      int lo = p, hi = P;  // upper_bound of d in sd[p..P)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sd[mid] <= d) lo = mid + 1; else hi = mid;
      }
      acc += (double)lo / (double)le;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    ap[q] = P > 0 ? acc / (double)P : 0.0;
    valid[q] = P > 0 ? 1 : 0;
    first_rank[q] = P > 0 ? before[q] : -1;
  }
}

int ap_finalize(int64_t Q, int Ptot, const float* sorted_d, const int32_t* pos_total,
                const int32_t* hist, const int32_t* before, double* ap, int32_t* valid,
                int32_t* first_rank, hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  hipLaunchKernelGGL(ap_finalize_kernel, dim3((unsigned)Q), dim3(64), 0, st, Q, Ptot,
                     sorted_d, pos_total, hist, before, ap, valid, first_rank);
  PPS_CHECK_LAUNCH("ap_finalize_kernel");
  return PPS_OK;
}

// ---- 4) CMC beyond the Market protocol (reid_dataset_evaluator.py:283-363) -------
// The reference's cmc defaults to first_match_break=False: for the j-th true
// match (in rank order) at position k among the valid entries it adds
// 1/#matches to ret[k - j], k - j = the number of valid NON-matches ranked
// before it (:349-356); separate_camera_set=True also drops every gallery
// entry from the query's camera (:329-331).  Both need, per positive p, the
// exact count of valid entries ordered before it.  Entry e is binned at
// b(e) = #positives whose (distance, global index) key is below e's, so
// H[p] = sum_{b <= p} hist[b] counts the valid entries ranked before positive
// p plus the positives 0..p: k - j = H[p] - p - 1.  Exact under the stable
// (distance, index) order, ties included; additive over gallery shards.
constexpr int kCmcLdsCap = 4096;

template <bool KLDS, bool SEP>
__global__ void __launch_bounds__(kStreamThreads)
cmc_count_kernel(const float* __restrict__ dist, int64_t G, int64_t ldd, int64_t g_offset,
                 int Ptot, const float* __restrict__ sorted_d,
                 const int32_t* __restrict__ sorted_idx, const int32_t* __restrict__ pos_total,
                 const int32_t* __restrict__ qcam, const int32_t* __restrict__ gcam, int Jmax,
                 const float* __restrict__ junk_d, const int32_t* __restrict__ junk_idx,
                 const int32_t* __restrict__ junk_cnt, int32_t* __restrict__ hist) {
  const int64_t q = blockIdx.x;
  const int P = pos_total[q];
  if (P == 0) return;
  extern __shared__ int slds[];
  float* sd = reinterpret_cast<float*>(slds);
  int* si = slds + (KLDS ? P : 0);
  int* hs = slds + (KLDS ? 2 * P : 0);
  const float* gsd = sorted_d + q * Ptot;
  const int32_t* gsi = sorted_idx + q * Ptot;
  int32_t* ghist = hist + q * Ptot;
  if (KLDS) {
    for (int p = threadIdx.x; p < P; p += kStreamThreads) {
      sd[p] = gsd[p];
      si[p] = gsi[p];
      hs[p] = 0;
    }
    __syncthreads();
  }
  const float* S = KLDS ? sd : gsd;
  const int32_t* I = KLDS ? si : gsi;
  const float dmax = S[P - 1];
  // b = #positives with key < (d, gi); entries ordered after every positive
  // (b == P) do not count
  auto key_bin = [&](float d, int64_t gi) {
    int lo = 0, hi = P;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (S[mid] < d || (S[mid] == d && (int64_t)I[mid] < gi)) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  auto add = [&](int b, int v) {
    if (b < P) {
      if (KLDS) atomicAdd(&hs[b], v); else atomicAdd(&ghist[b], v);
    }
  };
  const int qc = SEP ? qcam[q] : 0;
  const int64_t c0 = (int64_t)blockIdx.y * kStreamChunk;
  const int64_t c1 = c0 + kStreamChunk < G ? c0 + kStreamChunk : G;
  const float* row = dist + q * ldd;
  for (int64_t i = c0 + threadIdx.x; i < c1; i += kStreamThreads) {
    const float d = row[i];
    if (d > dmax) continue;
    if (SEP && gcam[i] == qc) continue;  // same camera: never valid
    add(key_bin(d, g_offset + i), 1);
  }
  if (!SEP && blockIdx.y == 0) {  // this shard's junk (same id, same camera) back out
    const int nj = junk_cnt[q] < Jmax ? junk_cnt[q] : Jmax;
    for (int j = threadIdx.x; j < nj; j += kStreamThreads) {
      const float d = junk_d[q * Jmax + j];
      if (d <= dmax) add(key_bin(d, (int64_t)junk_idx[q * Jmax + j]), -1);
    }
  }
  if (KLDS) {
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += kStreamThreads)
      if (hs[p]) atomicAdd(&ghist[p], hs[p]);
  }
}

int cmc_counts(const float* dist, int64_t Q, int64_t G, int64_t ldd, int64_t g_offset, int Ptot,
               const float* sorted_d, const int32_t* sorted_idx, const int32_t* pos_total,
               const int32_t* qcam, const int32_t* gcam, int Jmax, const float* junk_d,
               const int32_t* junk_idx, const int32_t* junk_cnt, int32_t* hist,
               hipStream_t st) {
  if (Q <= 0 || G <= 0) return PPS_OK;
  const int64_t nchunk = (G + kStreamChunk - 1) / kStreamChunk;
  const bool lds = Ptot <= kCmcLdsCap, sep = gcam != nullptr;
  const size_t shm = lds ? (size_t)3 * Ptot * sizeof(int) : 0;
  for (int64_t q0 = 0; q0 < Q; q0 += 65535) {  // grid.x limit
    const int64_t qn = Q - q0 < 65535 ? Q - q0 : 65535;
    const dim3 grid((unsigned)qn, (unsigned)nchunk);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kStreamThreads), shm, st, dist + q0 * ldd, G, ldd,
                         g_offset, Ptot, sorted_d + q0 * Ptot, sorted_idx + q0 * Ptot,
                         pos_total + q0, sep ? qcam + q0 : nullptr, gcam, Jmax,
                         junk_d + q0 * Jmax, junk_idx + q0 * Jmax, junk_cnt + q0,
                         hist + q0 * Ptot);
    };
    if (lds && sep) launch(cmc_count_kernel<true, true>);
    else if (lds) launch(cmc_count_kernel<true, false>);
    else if (sep) launch(cmc_count_kernel<false, true>);
    else launch(cmc_count_kernel<false, false>);
    PPS_CHECK_LAUNCH("cmc_count_kernel");
  }
  return PPS_OK;
}

// Per query (one wave): ret[q][0..topk) = the reference's CMC row after its
// cumsum (:358-360): for positives p = 0.. in rank order, c = H[p] - p - 1;
// stop at c >= topk; first_match_break adds 1 once, else 1/P each, summed in
// the reference's order (float64, same rounding).  valid[q] = P > 0.
__global__ void cmc_finalize_kernel(int Ptot, const int32_t* __restrict__ pos_total,
                                    const int32_t* __restrict__ hist, int topk, int fmb,
                                    double* __restrict__ ret, int32_t* __restrict__ valid) {
  const int64_t q = blockIdx.x;
  const int P = pos_total[q];
  double* r = ret + q * topk;
  for (int t = threadIdx.x; t < topk; t += 64) r[t] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    valid[q] = P > 0 ? 1 : 0;
    if (P > 0) {
      const int32_t* h = hist + q * Ptot;
      const double delta = 1.0 / (double)P;
      int64_t H = 0;
      for (int p = 0; p < P; ++p) {
        H += h[p];
        const int64_t c = H - p - 1;
        if (c >= topk) break;
        if (fmb) {
          r[c] += 1.0;
          break;
        }
        r[c] += delta;
      }
      for (int t = 1; t < topk; ++t) r[t] += r[t - 1];
    }
  }
}

int cmc_finalize(int64_t Q, int Ptot, const int32_t* pos_total, const int32_t* hist, int topk,
                 int fmb, double* ret, int32_t* valid, hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  hipLaunchKernelGGL(cmc_finalize_kernel, dim3((unsigned)Q), dim3(64), 0, st, Ptot, pos_total,
                     hist, topk, fmb, ret, valid);
  PPS_CHECK_LAUNCH("cmc_finalize_kernel");
  return PPS_OK;
}

}  // namespace pps
