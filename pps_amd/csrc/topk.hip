// Stable per-row top-k: the block kernel, the wave-streaming kernel for long
// rows, re-ranking's in-place variants and the k-way merge of per-shard lists.
#include "gemm_common.hpp"
#include "retrieval.hpp"
#include "topk_wave_common.hpp"

namespace pps {

// ---- stable per-row top-k ---------------------------------------------------------
// Radix select (4 x 8-bit digits of the order-preserving key) finds the k-th
// smallest key K*; entries with key < K*, then entries == K* in index order,
// are compacted into LDS and bitonic-sorted as 64-bit (key << 32 | index)
// (float_key / key_float: topk_wave_common.hpp).
constexpr int kTopkThreads = 256;
constexpr int kTopkBuf = 4096;      // candidate buffer (64-bit entries) in LDS
constexpr int kTopkUnroll = 8;      // row elements per thread per chunk
static_assert(kTopkCap + kTopkThreads * kTopkUnroll <= kTopkBuf,
              "a cut buffer plus one chunk must fit");

// Bitonic sort (ascending) of buf[0, n2), n2 a power of two, by the block.
__device__ inline void block_bitonic(unsigned long long* buf, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
        const int i = 2 * stride * (t / stride) + (t % stride);
        const int j = i + stride;
        const bool up = (i & size) == 0;
        const unsigned long long a = buf[i], b = buf[j];
        if ((a > b) == up) { buf[i] = b; buf[j] = a; }
      }
      __syncthreads();
    }
  }
}

// cut: keep the k best of the n candidates cand[0, n) at the front (block-
// wide).  The k-th best packed key T is found by an 8-pass radix select
// (8-bit digits from the top; packed keys are unique, so exactly k entries
// are <= T) and the k entries are compacted to the front -- a full bitonic
// sort of the buffer (78 LDS-bound stages for 4096 entries, shared by the
// CU's blocks) cost ~150 us per row block on short rows.  Only the final
// cut sorts, and only those k entries.  Returns T (~0 when n <= k).
struct TopkSmem {
  unsigned hist[256];
  unsigned long long pref;
  int rank, cnt;
};
__device__ unsigned long long block_cut(unsigned long long* cand, int n, int k, bool final,
                                        TopkSmem& sm) {
  constexpr int kPerThr = kTopkBuf / kTopkThreads;
  unsigned long long T = ~0ull;
  int keep = n;
  if (n > k) {
    if (threadIdx.x == 0) { sm.pref = 0ull; sm.rank = k; }
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      for (int i = threadIdx.x; i < 256; i += blockDim.x) sm.hist[i] = 0u;
      __syncthreads();
      const unsigned long long pre = sm.pref;
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long v = cand[i];
        if (pass == 0 || (v >> (shift + 8)) == pre)
          atomicAdd(&sm.hist[(unsigned)(v >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 64) {  // one wave: the bin holding rank sm.rank
        const int l = threadIdx.x;
        unsigned h[4], sum = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) { h[b] = sm.hist[4 * l + b]; sum += h[b]; }
        unsigned incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned t = __shfl_up(incl, o);
          if (l >= o) incl += t;
        }
        const unsigned r = (unsigned)sm.rank;
        const unsigned long long hit = __ballot(incl >= r);
        const int hl = __ffsll((long long)hit) - 1;
        if (l == hl) {
          unsigned before = incl - sum;
          int b = 0;
          while (b < 3 && before + h[b] < r) before += h[b++];
          sm.pref = (pre << 8) | (unsigned long long)(4 * l + b);
          sm.rank = (int)(r - before);
        }
      }
      __syncthreads();
    }
    T = sm.pref;  // the k-th best packed key
    unsigned long long mine[kPerThr];
#pragma unroll
    for (int j = 0; j < kPerThr; ++j) {
      const int i = threadIdx.x + j * kTopkThreads;
      mine[j] = i < n ? cand[i] : ~0ull;
    }
    if (threadIdx.x == 0) sm.cnt = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerThr; ++j)
      if (mine[j] <= T) cand[atomicAdd(&sm.cnt, 1)] = mine[j];
    __syncthreads();
    keep = k;
  }
  if (final) {
    int n2 = 1;
    while (n2 < keep) n2 <<= 1;
    for (int i = keep + threadIdx.x; i < n2; i += blockDim.x) cand[i] = ~0ull;
    __syncthreads();
    block_bitonic(cand, n2);
  }
  return T;
}

// One pass over the row.  Entries are packed as (order-preserving key << 32 |
// index), so comparing packed values is the stable (distance, index) order.
// An entry enters the LDS candidate buffer only if it beats the current
// threshold = the k-th best packed value among the candidates kept so far;
// when the buffer could overflow in the next chunk it is cut back to its k
// best (rare after the first chunks: ~k*ln(G/k) insertions per row).
// V4: 16-byte rows -- each thread takes two float4 per chunk (dwordx4 buffer
// loads, 4x fewer load instructions) and the loads run two chunks ahead, so
// a block keeps 16 KB of its row in flight instead of 8 KB (the kernel is
// latency-bound at 5 blocks per CU).  Which thread sees which entry does
// not matter: candidates are ordered by their packed (key, index) value.
template <bool V4>
__global__ void __launch_bounds__(kTopkThreads)
topk_kernel(const float* __restrict__ dist, int64_t G, int64_t ldd, int k,
            float* __restrict__ vals, int32_t* __restrict__ idx) {
  const int64_t q = blockIdx.x;
  const float* row = dist + q * ldd;
  __shared__ unsigned long long cand[kTopkBuf];
  __shared__ int s_n;
  __shared__ unsigned long long s_thr;
  if (threadIdx.x == 0) { s_n = 0; s_thr = ~0ull; }
  __syncthreads();
  const int64_t chunk = (int64_t)blockDim.x * kTopkUnroll;
  __shared__ TopkSmem sm;
  auto cut = [&](int n, bool final) {
    const unsigned long long T = block_cut(cand, n, k, final, sm);
    if (threadIdx.x == 0) {
      s_n = n > k ? k : n;
      if (n > k) s_thr = T;
    }
    __syncthreads();
  };
  // the next chunk's row values are requested before this chunk is
  // processed; the chunk-closing barrier is a raw s_barrier after an LDS-only
  // wait, so those loads stay in flight across it (__syncthreads() would
  // drain them with vmcnt(0))
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  // buffer loads: the row tail past G reads zero without exec-mask branches,
  // which keeps the loads countable (a branchy guard makes hipcc wait vmcnt(0))
  // V4: the vector loop covers the first GV = G & ~3 entries (its descriptor
  // ends there, so no 16-byte load straddles G); the last G - GV entries
  // are taken after the loop by scalar loads.
  const int64_t GV = V4 ? (G & ~(int64_t)3) : G;
  const rsrc_t rrow = make_rsrc(row, (uint32_t)(GV * 4));
  auto ld = [&](int64_t i) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrow, (int)(i * 4), 0, 0));
  };
  // entry u of this thread in the chunk at c0
  auto ent = [&](int64_t c0, int u) -> int64_t {
    return V4 ? c0 + 4 * ((int64_t)(u >> 2) * kTopkThreads + threadIdx.x) + (u & 3)
              : c0 + (int64_t)u * kTopkThreads + threadIdx.x;
  };
  auto load_chunk = [&](int64_t c0, float (&dst)[kTopkUnroll]) {
    if (V4) {
#pragma unroll
      for (int j = 0; j < kTopkUnroll / 4; ++j) {
        const f32x4 v = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrow, (int)(ent(c0, 4 * j) * 4), 0, 0));
        dst[4 * j] = v.x;
        dst[4 * j + 1] = v.y;
        dst[4 * j + 2] = v.z;
        dst[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < kTopkUnroll; ++u) dst[u] = ld(ent(c0, u));
    }
  };
  float d[kTopkUnroll], dn[kTopkUnroll];
  load_chunk(0, d);
  if (V4) load_chunk(chunk, dn);
  for (int64_t c0 = 0; c0 < GV; c0 += chunk) {
    // every wave must take the same cut decision: snapshot the count, then
    // a barrier so that no wave's insertions of this chunk (atomicAdd on
    // s_n) can land before a slower wave has read it
    const int n_now = s_n;
    lds_barrier();
    // the first chunk enters unfiltered: cut it at once (a 2048-entry select
    // instead of a 4096-entry one a chunk later) so the next chunks filter
    if (n_now + chunk > kTopkBuf || (c0 == chunk && n_now > k)) cut(n_now, false);
    const unsigned long long thr = s_thr;
    float dn2[kTopkUnroll];
    load_chunk(c0 + (V4 ? 2 : 1) * chunk, dn2);
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {
      const int64_t i = ent(c0, u);
      const unsigned long long packed =
          ((unsigned long long)float_key(d[u]) << 32) | (uint32_t)i;
      const bool take = i < GV && packed < thr;
      const unsigned long long bal = __ballot(take);  // one LDS atomic per wave
      if (bal) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_n, __popcll(bal));
        base = __shfl(base, 0);
        if (take) cand[base + __popcll(bal & below)] = packed;
      }
    }
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {
      if (V4) {
        d[u] = dn[u];
        dn[u] = dn2[u];
      } else {
        d[u] = dn2[u];
      }
    }
    lds_barrier();
  }
  if (V4 && GV < G) {  // the < 4 entries past the vector loop
    const int n_now = s_n;
    lds_barrier();
    if (n_now + 4 > kTopkBuf) cut(n_now, false);
    const unsigned long long thr = s_thr;
    if (threadIdx.x < G - GV) {
      const int64_t i = GV + threadIdx.x;
      const unsigned long long packed = ((unsigned long long)float_key(row[i]) << 32) | (uint32_t)i;
      if (packed < thr) cand[atomicAdd(&s_n, 1)] = packed;
    }
    __syncthreads();
  }
  cut(s_n, true);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long v = cand[i];
    vals[q * k + i] = key_float((uint32_t)(v >> 32));
    idx[q * k + i] = (int32_t)(v & 0xffffffffu);
  }
}

// Long rows (the 1M-gallery shards: 125k entries per row): every WAVE streams
// its own contiguous quarter of the row with its own threshold and its own
// candidate buffer in LDS, so the streaming loop has no block barrier and no
// LDS atomic (a wave appends at its own uniform count).  When the next
// iteration could overflow the buffer (and once right after the first
// iteration, so the rest of the row is filtered against a real threshold) the
// wave cuts it back to between k and k + kTkwSlack entries; at the end to
// exactly its k best.  Wave 0 then selects the row's k best of the four lists
// and the block sorts them.  Same result as topk_kernel (the stable
// (distance, index) top-k is unique).
//
// Selection is a bisection on the packed value with the buffer held in
// registers: each step is one compare per register, a ballot and a scalar
// popcount -- no LDS atomics.  (A radix select's LDS histogram serialises
// here: after the first cut the buffered keys share their top bytes, so 64
// lanes add into one bin.)
constexpr int kTkwU = 2;                    // float4 per lane per iteration
constexpr int kTkwD = 2;                    // iterations loaded ahead of the one filtering
static_assert(kTkwD == 2, "the streaming loops rotate three named buffers");
constexpr int kTkwIter = 64 * 4 * kTkwU;    // row entries per wave iteration (512)
constexpr int kTkwWaves = kTopkThreads / 64;
// (rows of at least kTkwMinRow entries take this kernel: retrieval.hpp)
// per-wave buffer: what a cut keeps + one iteration's worst-case inflow
__host__ __device__ constexpr int tkw_cap(int k) { return (k + kTkwSlack + kTkwIter + 63) / 64 * 64; }
// registers per lane for a wave's buffer / the four merged lists, for k <= KM
template <int KM> constexpr int tkw_j() { return tkw_cap(KM) / 64; }
template <int KM> constexpr int tkw_merge_j() { return kTkwWaves * KM / 64 + 1; }
// (wave_select / wave_cut: topk_wave_common.hpp)

// RR (re-ranking, rerank.hip): row q is row q of OD for a symmetric M read
// in place -- a virtual row of the M row's first block (Q entries, padded to
// naq = Q rounded up to 4 with +inf, never selected) followed by its second
// block (G entries), each entry transformed to rr_od(m, colmax[q]) before the
// filter; packed indices are the global column (virtual index with the pad
// taken out: a monotone map, so the order is the same).
//
// WPR (waves per row) 1: every wave streams a whole row of its own (a block
// holds four rows) -- for many rows of moderate length (re-ranking's N rows
// of N), where four waves per row would each cut their short segment three or
// four times and then merge: one wave per row cuts ~log(row / 512) times in
// all and sorts its own k, no block barrier.
//
// rows (WPR 1): the rows to process are rows[0, *rows_n) (a device list).
template <int KM, bool RR, int WPR = kTkwWaves>
__global__ void __launch_bounds__(kTopkThreads) __attribute__((amdgpu_waves_per_eu(6)))
topk_wave_kernel(const float* __restrict__ dist, int64_t G, int64_t ldd, int k, int cap,
                 float* __restrict__ vals, int32_t* __restrict__ idx, RrMatrix rr,
                 int64_t nrows, const int32_t* __restrict__ rows = nullptr,
                 const int32_t* __restrict__ rows_n = nullptr) {
  static_assert(WPR == 1 || WPR == kTkwWaves, "one wave or the whole block per row");
  extern __shared__ unsigned long long tkw[];  // [waves][cap] buffers
  // wave-uniform: segment bounds, buffer base and counts live in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  unsigned long long* buf = tkw + wave * cap;
  constexpr int RPB = kTkwWaves / WPR;   // rows per block
  const int wseg = wave % WPR;           // this wave's segment of its row
  int64_t q = (int64_t)blockIdx.x * RPB + wave / WPR;
  if (WPR == 1 && rows) {
    if (q >= *rows_n) return;
    q = rows[q];
  }
  if (WPR == 1 && q >= nrows) return;   // (WPR = 1 has no block barrier)
  const float* row = RR ? nullptr : dist + q * ldd;
  // RR: the two blocks of M's row q
  const int64_t na = RR ? rr.Q : 0, naq = RR ? (rr.Q + 3) / 4 * 4 : 0;
  const float* rowA = RR ? (q < rr.Q ? rr.qq + q * rr.ldqq : rr.qgT + (q - rr.Q) * rr.ldT) : nullptr;
  const float* rowB = RR ? (q < rr.Q ? rr.qg + q * rr.ldqg : rr.gg + (q - rr.Q) * rr.ldgg) : nullptr;
  const float cm = RR ? rr.colmax[q] : 1.f;
  if (RR) G = naq + rr.G;  // virtual row length
  // virtual index -> column of OD
  auto col = [&](uint32_t i) -> uint32_t {
    return RR ? (i < (uint32_t)naq ? i : i - (uint32_t)(naq - na)) : i;
  };
  // one loaded entry -> its OD value (RR) / itself
  auto xf = [&](float m, int64_t i) -> float {
    if (!RR) return m;
    return (i >= na && i < naq) ? __builtin_huge_valf() : rr_od(m, cm);
  };
  // this wave's segment [s0, s1): whole float4s of the 16-byte-aligned row
  const int64_t GV = G & ~(int64_t)3;
  const int64_t per = ((GV / 4 + WPR - 1) / WPR) * 4;
  const int64_t s0 = min(GV, (int64_t)wseg * per), s1 = min(GV, s0 + per);
  const rsrc_t rrow = make_rsrc(RR ? rowA : row, (uint32_t)(GV * 4));  // past GV: reads zero (masked)
  const unsigned long long below = (1ull << lane) - 1ull;
  auto load = [&](int64_t it, f32x4 (&dst)[kTkwU]) {
#pragma unroll
    for (int u = 0; u < kTkwU; ++u) {
      const int64_t i = s0 + it * kTkwIter + 4 * (u * 64 + lane);
      if (RR) {  // per-lane block select; past the segment a harmless in-row address
        const float* a = i >= s1 ? rowA : (i < naq ? rowA + i : rowB + (i - naq));
        dst[u] = *reinterpret_cast<const f32x4*>(a);
      } else {
        dst[u] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrow, (int)(i < s1 ? i * 4 : GV * 4), 0, 0));
      }
    }
  };
  const int64_t niter = (s1 - s0 + kTkwIter - 1) / kTkwIter;
  int n = 0;
  unsigned long long thr = ~0ull;   // inclusive: entries <= thr stay candidates
  // Float pre-filter: an entry can only be <= thr if its distance is not
  // above thr's distance, !(e > thr_f) -- a superset of the exact test (NaN
  // entries and the initial NaN threshold pass it).  One compare per entry;
  // the append runs only for the entry slots where some lane passed.
  float thr_f = key_float((uint32_t)(thr >> 32));
  // one iteration: refill `nxt` (consumed by the previous iteration) with
  // iteration it + kTkwD, then filter `cur`.  Named buffers in a loop
  // unrolled by the rotation length: a rotating a = b, b = c would make the
  // compiler copy the registers at the end of every iteration and so wait for
  // the load it had just issued (vmcnt(0)).
  auto step = [&](int64_t it, const f32x4 (&cur)[kTkwU], f32x4 (&nxt)[kTkwU]) {
    if (n + kTkwIter > cap || (it == 1 && n > k + kTkwSlack)) {
      thr = wave_cut<tkw_j<KM>()>(buf, n, k, kTkwSlack);
      thr_f = key_float((uint32_t)(thr >> 32));
    }
    // keep each step's refill in its step: a load hoisted above the previous
    // step's filter would overlap `nxt` with live buffers, and the loop head
    // would then wait for every load in flight
    asm volatile("" ::: "memory");
    load(it + kTkwD, nxt);
    unsigned long long m[kTkwU][4], any = 0ull;
    float ev[kTkwU][4];
#pragma unroll
    for (int u = 0; u < kTkwU; ++u) {
      const int64_t iv = s0 + it * kTkwIter + 4 * (u * 64 + lane);
      const float e[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ev[u][t] = xf(e[t], iv + t);
        m[u][t] = __ballot(!(ev[u][t] > thr_f));
        any |= m[u][t];
      }
    }
    if (!any) return;
    if ((it + 1) * kTkwIter > s1 - s0) {   // the segment's last iteration: exact, bounded
#pragma unroll
      for (int u = 0; u < kTkwU; ++u) {
        const int64_t i0 = s0 + it * kTkwIter + 4 * (u * 64 + lane);
        const float* e = ev[u];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!m[u][t]) continue;
          const int64_t i = i0 + t;
          const unsigned long long packed = ((unsigned long long)float_key(e[t]) << 32) | col((uint32_t)i);
          const bool take = i < s1 && packed <= thr;
          const unsigned long long bal = __ballot(take);
          if (take) buf[n + __popcll(bal & below)] = packed;
          n += __popcll(bal);
        }
      }
      return;
    }
    // inside the segment every pre-filter passer is appended: an entry with
    // thr's distance but a larger index is a harmless extra candidate (cuts
    // rank packed values), so the slot costs the key, the lane's rank in the
    // pass mask and one LDS store
#pragma unroll
    for (int u = 0; u < kTkwU; ++u) {
      const uint32_t i0 = (uint32_t)(s0 + it * kTkwIter) + 4u * (uint32_t)(u * 64 + lane);
      const float* e = ev[u];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned long long mm = m[u][t];
        if (!mm) continue;
        if (!(e[t] > thr_f)) {
          const uint32_t ub = __float_as_uint(e[t]);
          const uint32_t key = ub ^ ((uint32_t)((int32_t)ub >> 31) | 0x80000000u);
          const int pos = n + (int)__builtin_amdgcn_mbcnt_hi(
                                  (uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
          buf[pos] = ((unsigned long long)key << 32) | col(i0 + (uint32_t)t);
        }
        n += __popcll(mm);
      }
    }
  };
  // Whole rounds: the iterations past the segment read zeros (buffer loads
  // past GV) and take nothing (i >= s1).
  f32x4 a[kTkwU], b[kTkwU], c[kTkwU];
  load(0, a);
  asm volatile("" ::: "memory");   // issue order a, b: the first step waits for a only
  load(1, b);
  for (int64_t it = 0; it < niter; it += 3) {
    step(it, a, c);
    step(it + 1, b, a);
    step(it + 2, c, b);
  }
  if (n > k) wave_cut<tkw_j<KM>()>(buf, n, k, 0);
  // the < 4 entries past the last float4: segment 0 takes them (scalar loads)
  if (wseg == 0 && GV < G) {
    const int64_t i = GV + lane;
    const bool take = i < G;
    const float e = RR ? (take ? xf(rowB[i - naq], i) : 0.f) : row[take ? i : 0];
    const unsigned long long packed =
        take ? (((unsigned long long)float_key(e) << 32) | col((uint32_t)i)) : ~0ull;
    const unsigned long long bal = __ballot(take);
    if (take) buf[n + __popcll(bal & below)] = packed;
    n += __popcll(bal);
  }
  if (WPR == 1) {   // the wave's own list is the row's: exact k, then sorted
    if (n > k) wave_cut<tkw_j<KM>()>(buf, n, k, 0);
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = n + lane; i < n2; i += 64) buf[i] = ~0ull;
    wave_lds_sync();
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
    for (int i = lane; i < k; i += 64) {
      const unsigned long long v = buf[i];
      vals[q * k + i] = key_float((uint32_t)(v >> 32));
      idx[q * k + i] = (int32_t)(v & 0xffffffffu);
    }
    return;
  }
  // merge: wave 0 reads the four lists (<= k + 3 entries each) and keeps the
  // row's k best at the front of the LDS; the block sorts them
  __shared__ int s_cnt[kTkwWaves];
  if (lane == 0) s_cnt[wave] = n;
  __syncthreads();
  if (wave == 0) {
    constexpr int MJ = tkw_merge_j<KM>();
    unsigned long long v[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int p = j * 64 + lane;   // merged position
      int ww = 0, off = p;
      for (; ww < kTkwWaves && off >= s_cnt[ww]; ++ww) off -= s_cnt[ww];
      v[j] = ww < kTkwWaves ? tkw[ww * cap + off] : ~0ull;
    }
    int total = 0;
    for (int ww = 0; ww < kTkwWaves; ++ww) total += s_cnt[ww];
    const unsigned long long T = total > k ? wave_select(v, k, 0) : ~0ull - 1;
    wave_lds_sync();
    int m = 0;
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const bool keep = v[j] <= T;
      const unsigned long long bal = __ballot(keep);
      if (keep) tkw[m + __popcll(bal & below)] = v[j];
      m += __popcll(bal);
    }
    // pad to the sort length
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = m + lane; i < n2; i += 64) tkw[i] = ~0ull;
  }
  __syncthreads();
  int n2 = 1;
  while (n2 < k) n2 <<= 1;
  block_bitonic(tkw, n2);
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long v = tkw[i];
    vals[q * k + i] = key_float((uint32_t)(v >> 32));
    idx[q * k + i] = (int32_t)(v & 0xffffffffu);
  }
}

int topk(const float* dist, int64_t Q, int64_t G, int64_t ldd, int k, float* vals,
         int32_t* idx, hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  const bool v4 = (reinterpret_cast<uintptr_t>(dist) & 15) == 0 && (ldd & 3) == 0;
  if (v4 && G >= kTkwMinRow && k <= kTkwMaxK) {
    const int cap = tkw_cap(k);
    const size_t lds = (size_t)kTkwWaves * cap * 8;
    const RrMatrix none{};
    if (k <= 128)
      hipLaunchKernelGGL((topk_wave_kernel<128, false>), dim3((unsigned)Q), dim3(kTopkThreads),
                         lds, st, dist, G, ldd, k, cap, vals, idx, none, Q, nullptr,
                         nullptr);
    else
      hipLaunchKernelGGL((topk_wave_kernel<kTkwMaxK, false>), dim3((unsigned)Q),
                         dim3(kTopkThreads), lds, st, dist, G, ldd, k, cap, vals, idx, none, Q, nullptr,
                         nullptr);
  } else if (v4)
    hipLaunchKernelGGL(topk_kernel<true>, dim3((unsigned)Q), dim3(kTopkThreads), 0, st, dist, G,
                       ldd, k, vals, idx);
  else
    hipLaunchKernelGGL(topk_kernel<false>, dim3((unsigned)Q), dim3(kTopkThreads), 0, st, dist,
                       G, ldd, k, vals, idx);
  PPS_CHECK_LAUNCH("topk_kernel");
  return PPS_OK;
}

bool topk_rr_eligible(const RrMatrix& M, int k) {
  auto a16 = [](const float* p, int64_t ld) { return aligned16(p) && (ld & 3) == 0; };
  return M.Q + M.G >= kTkwMinRow && k <= kTkwMaxK &&
         a16(M.qq, M.ldqq) && a16(M.qg, M.ldqg) && a16(M.gg, M.ldgg) && a16(M.qgT, M.ldT) &&
         M.ldT >= (M.Q + 3) / 4 * 4 && M.ldqq >= (M.Q + 3) / 4 * 4 && M.Q + M.G < (1ll << 31);
}

int topk_rr(const RrMatrix& M, int k, float* vals, int32_t* idx, hipStream_t st) {
  const int64_t N = M.Q + M.G;
  if (!topk_rr_eligible(M, k)) {
    set_error("topk_rr: needs N >= " + std::to_string(kTkwMinRow) + ", k <= " +
              std::to_string(kTkwMaxK) + " and 16-byte aligned block rows");
    return PPS_ERR_INVALID_ARG;
  }
  const int cap = tkw_cap(k);
  const size_t lds = (size_t)kTkwWaves * cap * 8;
  // one wave per row
  const unsigned rows_grid = (unsigned)((N + kTkwWaves - 1) / kTkwWaves);
  if (k <= 128)
    hipLaunchKernelGGL((topk_wave_kernel<128, true, 1>), dim3(rows_grid), dim3(kTopkThreads),
                       lds, st, nullptr, (int64_t)0, (int64_t)0, k, cap, vals, idx, M, N, nullptr, nullptr);
  else
    hipLaunchKernelGGL((topk_wave_kernel<kTkwMaxK, true, 1>), dim3(rows_grid),
                       dim3(kTopkThreads), lds, st, nullptr, (int64_t)0, (int64_t)0, k, cap,
                       vals, idx, M, N, nullptr, nullptr);
  PPS_CHECK_LAUNCH("topk_wave_kernel<rr>");
  return PPS_OK;
}

// Re-ranking's first pass over a symmetric M (rerank.hip, in place): per row
// q the top-k' by (m * m, index) over M's row -- its first block (qq or
// q_g^T, Q entries) then its second (q_g or g_g, G entries), column = Q +
// position in the second -- and rowmax[q] = the max of the row's squares,
// which for a symmetric M is colmax[q] (:453).  OD = (m * m) / colmax is a
// monotone map of m * m, so rerank_rank_fix_kernel gets the top-k by (OD,
// index) from this list.  One wave per row (four rows per block) streams the
// two blocks as two segments through the same candidate buffer and threshold
// (topk_wave_kernel's filter / cut / select); per entry one product, one
// compare and one max, 32-bit offsets into buffer descriptors.
//
// The list's fix-up runs in the same wave once the row max is known: OD of
// each of the k' = kp entries, and when the kp-th entry's OD is above the
// k-th's (so every entry outside the list has OD above the k-th too) the
// top-k by (OD, index) is the list's k smallest (OD, index) pairs -- written
// to vals (OD) / idx.  Otherwise (an equal-OD run longer than the slack) the
// row goes to fb_rows for the exact OD pass.
template <int KM>
__global__ void __launch_bounds__(kTopkThreads) __attribute__((amdgpu_waves_per_eu(6)))
topk_rr_sq_kernel(RrMatrix rr, int k, int kp, int cap, float* __restrict__ vals,
                  int32_t* __restrict__ idx, float* __restrict__ rowmax,
                  int32_t* __restrict__ fb_rows, int32_t* __restrict__ fb_n) {
  extern __shared__ unsigned long long tkw[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  unsigned long long* buf = tkw + wave * cap;
  const int64_t q = (int64_t)blockIdx.x * kTkwWaves + wave;
  if (q >= rr.Q + rr.G) return;
  const float* rowA = q < rr.Q ? rr.qq + q * rr.ldqq : rr.qgT + (q - rr.Q) * rr.ldT;
  const float* rowB = q < rr.Q ? rr.qg + q * rr.ldqg : rr.gg + (q - rr.Q) * rr.ldgg;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n = 0, cuts = 0;
  unsigned long long thr = ~0ull;
  float thr_f = key_float((uint32_t)(thr >> 32));   // NaN: everything passes
  float mx = 0.f;
  auto cut = [&]() {
    thr = wave_cut<tkw_j<KM>()>(buf, n, kp, kTkwSlack);
    thr_f = key_float((uint32_t)(thr >> 32));
    ++cuts;
  };
  auto segment = [&](const float* base, uint32_t L, uint32_t col0) {
    const uint32_t V = L & ~3u;
    const rsrc_t rs = make_rsrc(base, V * 4u);
    const uint32_t niter = (V + kTkwIter - 1) / kTkwIter;
    auto load = [&](uint32_t it, f32x4 (&dst)[kTkwU]) {
#pragma unroll
      for (int u = 0; u < kTkwU; ++u)
        dst[u] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                       rs, (int)((it * kTkwIter + 4u * (uint32_t)(u * 64 + lane)) * 4u), 0, 0));
    };
    auto step = [&](uint32_t it, const f32x4 (&cur)[kTkwU], f32x4 (&nxt)[kTkwU]) {
      if (n + kTkwIter > cap || (cuts == 0 && n > kp + kTkwSlack)) cut();
      asm volatile("" ::: "memory");
      load(it + kTkwD, nxt);
      const uint32_t i0 = it * kTkwIter;
      const bool last = i0 + kTkwIter > V;   // wave-uniform: the only partial iteration
      float sq[kTkwU][4];
      unsigned long long m[kTkwU][4], any = 0ull;
#pragma unroll
      for (int u = 0; u < kTkwU; ++u) {
        const float e[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
        const uint32_t iv = i0 + 4u * (uint32_t)(u * 64 + lane);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          sq[u][t] = e[t] * e[t];
          const bool valid = !last || iv + t < V;
          mx = valid ? fmaxf(mx, sq[u][t]) : mx;
          m[u][t] = __ballot(valid && !(sq[u][t] > thr_f));
          any |= m[u][t];
        }
      }
      if (!any) return;
#pragma unroll
      for (int u = 0; u < kTkwU; ++u) {
        const uint32_t iv = i0 + 4u * (uint32_t)(u * 64 + lane);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const unsigned long long mm = m[u][t];
          if (!mm) continue;
          if ((mm >> lane) & 1ull) {
            const uint32_t ub = __float_as_uint(sq[u][t]);
            const uint32_t key = ub ^ ((uint32_t)((int32_t)ub >> 31) | 0x80000000u);
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi(
                                    (uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
            buf[pos] = ((unsigned long long)key << 32) | (col0 + iv + (uint32_t)t);
          }
          n += __popcll(mm);
        }
      }
    };
    f32x4 a[kTkwU], b[kTkwU], c[kTkwU];
    load(0, a);
    asm volatile("" ::: "memory");
    load(1, b);
    for (uint32_t it = 0; it < niter; it += 3) {
      step(it, a, c);
      if (it + 1 < niter) step(it + 1, b, a);
      if (it + 2 < niter) step(it + 2, c, b);
    }
    // the < 4 entries past the last float4
    if (V < L) {
      if (n + 4 > cap) cut();
      const bool take = lane < (int)(L - V);
      const float e = take ? base[V + lane] : 0.f;
      const float s2 = e * e;
      if (take) mx = fmaxf(mx, s2);
      const unsigned long long packed =
          ((unsigned long long)float_key(s2) << 32) | (col0 + V + (uint32_t)lane);
      const bool keep = take && packed <= thr;
      const unsigned long long bal = __ballot(keep);
      if (keep) buf[n + __popcll(bal & below)] = packed;
      n += __popcll(bal);
    }
    wave_lds_sync();
  };
  segment(rowA, (uint32_t)rr.Q, 0u);
  segment(rowB, (uint32_t)rr.G, (uint32_t)rr.Q);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) rowmax[q] = mx;
  if (n > kp) wave_cut<tkw_j<KM>()>(buf, n, kp, 0);   // exactly the kp best (row >= kp)
  // fix-up: one list entry per lane (kp <= 64)
  const unsigned long long v = lane < kp ? buf[lane] : ~0ull;
  const float od = key_float((uint32_t)(v >> 32)) / mx;   // rr_od's (m * m) / colmax
  int ps = 0;   // position in (m * m, index) order
  for (int t = 0; t < kp; ++t) ps += __shfl(v, t) < v ? 1 : 0;
  const unsigned long long at_k = __ballot(lane < kp && ps == k - 1);
  const unsigned long long at_l = __ballot(lane < kp && ps == kp - 1);
  const float vk = __shfl(od, (int)__builtin_ctzll(at_k)), vl = __shfl(od, (int)__builtin_ctzll(at_l));
  if (!(vl > vk)) {
    if (lane == 0) fb_rows[atomicAdd(fb_n, 1)] = (int32_t)q;
    return;
  }
  const unsigned long long packed =
      lane < kp ? (((unsigned long long)float_key(od) << 32) | (v & 0xffffffffu)) : ~0ull;
  int pos = 0;
  for (int t = 0; t < kp; ++t) pos += __shfl(packed, t) < packed ? 1 : 0;
  if (lane < kp && pos < k) {
    vals[q * k + pos] = od;
    idx[q * k + pos] = (int32_t)(v & 0xffffffffu);
  }
}

int topk_rr_sq(const RrMatrix& M, int k, float* rowmax, void* scratch, size_t scratch_bytes,
               float* vals, int32_t* idx, hipStream_t st) {
  const int64_t N = M.Q + M.G;
  const int kp = k + 8 < 64 ? k + 8 : 64;
  if (!topk_rr_eligible(M, kp)) {
    set_error("topk_rr_sq: needs N >= " + std::to_string(kTkwMinRow) + ", k <= " +
              std::to_string(kTkwMaxK) + " and 16-byte aligned block rows");
    return PPS_ERR_INVALID_ARG;
  }
  if (scratch_bytes < topk_rr_sq_scratch_bytes(N, k)) {
    set_error("topk_rr_sq: scratch too small");
    return PPS_ERR_CAPACITY;
  }
  int32_t* fb_n = reinterpret_cast<int32_t*>(scratch);
  int32_t* fb_rows = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + 256);
  (void)hipMemsetAsync(fb_n, 0, sizeof(int32_t), st);
  const unsigned grid = (unsigned)((N + kTkwWaves - 1) / kTkwWaves);
  const int capp = tkw_cap(kp);
  hipLaunchKernelGGL(topk_rr_sq_kernel<128>, dim3(grid), dim3(kTopkThreads),
                     (size_t)kTkwWaves * capp * 8, st, M, k, kp, capp, vals, idx, rowmax, fb_rows,
                     fb_n);
  PPS_CHECK_LAUNCH("topk_rr_sq_kernel");
  // the exact OD pass over the rows the list could not settle (grid for all
  // rows; waves past *fb_n return at once)
  RrMatrix Mc = M;
  Mc.colmax = rowmax;
  const int cap = tkw_cap(k);
  hipLaunchKernelGGL((topk_wave_kernel<128, true, 1>), dim3(grid), dim3(kTopkThreads),
                     (size_t)kTkwWaves * cap * 8, st, nullptr, (int64_t)0, (int64_t)0, k, cap,
                     vals, idx, Mc, N, fb_rows, fb_n);
  PPS_CHECK_LAUNCH("topk_wave_kernel<rr, rows>");
  return PPS_OK;
}

size_t topk_rr_sq_scratch_bytes(int64_t N, int) {
  return 256 + (sizeof(int32_t) * N + 255) / 256 * 256;
}

// ---- k-way merge of per-shard top-k lists ------------------------
// R gallery shards each hold a stable ascending top-k_in list per query
// (local indices; list r's global offset off[r]).  The global stable top-k_out
// is their merge by the packed (order-preserving key << 32 | global index)
// value.  Packed values are unique (global indices are), so an entry's output
// position is exactly its position in its own list plus, for every other list,
// the number of that list's entries below it (a binary search in LDS): every
// entry is placed independently, no sort and no serial merge.  Pad entries
// (index < 0, e.g. shards shorter than k_in) pack to ~0 and are never placed;
// output positions past the number of real entries get (+inf, -1).
constexpr int kMergeThreads = 256;
static_assert(kMergeMaxEntries * 8 <= 64 * 1024, "the merge's packed entries in dynamic LDS");

__global__ void topk_merge_kernel(const float* __restrict__ vals,
                                  const int32_t* __restrict__ idx, int R, int64_t Q,
                                  int kin, MergeOffsets offs, int kout,
                                  float* __restrict__ out_vals,
                                  int32_t* __restrict__ out_idx) {
  const int64_t q = blockIdx.x;
  extern __shared__ unsigned long long mkeys[];
  __shared__ int s_real;
  const int n = R * kin;
  if (threadIdx.x == 0) s_real = 0;
  __syncthreads();
  int real = 0;
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const int r = t / kin, p = t - r * kin;
    const int64_t src = ((int64_t)r * Q + q) * kin + p;
    const int32_t li = idx[src];
    unsigned long long key = ~0ull;
    if (li >= 0) {
      key = ((unsigned long long)float_key(vals[src]) << 32) |
            (uint32_t)(offs.off[r] + li);
      ++real;
    }
    mkeys[t] = key;
  }
  atomicAdd(&s_real, real);
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const unsigned long long key = mkeys[t];
    if (key == ~0ull) continue;
    const int r = t / kin;
    int pos = t - r * kin;
    for (int o = 0; o < R && pos < kout; ++o) {
      if (o == r) continue;
      const unsigned long long* L = mkeys + o * kin;
      int lo = 0, hi = kin;  // lower_bound: entries of list o below key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] < key) lo = mid + 1; else hi = mid;
      }
      pos += lo;
    }
    if (pos < kout) {
      out_vals[q * kout + pos] = key_float((uint32_t)(key >> 32));
      out_idx[q * kout + pos] = (int32_t)(key & 0xffffffffu);
    }
  }
  for (int p = s_real + threadIdx.x; p < kout; p += blockDim.x) {
    out_vals[q * kout + p] = INFINITY;
    out_idx[q * kout + p] = -1;
  }
}

int topk_merge(const float* vals, const int32_t* idx, int R, int64_t Q, int kin,
               const MergeOffsets& offs, int kout, float* out_vals, int32_t* out_idx,
               hipStream_t st) {
  if (Q <= 0) return PPS_OK;
  const size_t lds = (size_t)R * kin * sizeof(unsigned long long);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(kMergeThreads), lds, st,
                     vals, idx, R, Q, kin, offs, kout, out_vals, out_idx);
  PPS_CHECK_LAUNCH("topk_merge_kernel");
  return PPS_OK;
}

}  // namespace pps
