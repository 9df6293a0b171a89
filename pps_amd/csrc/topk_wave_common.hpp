// Wave-level pieces of the streaming stable top-k (topk.hip's topk_wave_kernel,
// search_h2.hip's filter epilogue): the order-preserving packing of a distance
// and the bisection select / cut of a wave's candidate buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pps {

// Entries are packed as (order-preserving key << 32 | index), so comparing
// packed values is the stable (distance, index) order.
__device__ inline uint32_t float_key(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// (the largest k, kTkwMaxK: retrieval.hpp)
constexpr int kTkwSlack = 64;               // a streaming cut keeps k .. k + slack entries

__device__ inline void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ inline unsigned long long wave_min_u64(unsigned long long x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}
__device__ inline unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y > x ? y : x;
  }
  return x;
}
template <int J>
__device__ inline int wave_count_le(const unsigned long long (&v)[J], unsigned long long t) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) c += __popcll(__ballot(v[j] <= t));
  return c;
}

// v[j] holds entry j*64 + lane of a wave's n > k unique packed values (~0ull
// past n; no real entry is ~0ull: indices are < 2^31).  Returns a T with
// k <= count(v <= T) <= k + slack; slack 0 gives the k-th smallest value.
// Invariant count(<= lo) < k <= count(<= hi); every value is wave-uniform.
template <int J>
__device__ unsigned long long wave_select(const unsigned long long (&v)[J], int k, int slack) {
  unsigned long long mn = ~0ull, mx = 0ull;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    mn = v[j] < mn ? v[j] : mn;
    mx = (v[j] != ~0ull && v[j] > mx) ? v[j] : mx;
  }
  mn = wave_min_u64(mn);
  mx = wave_max_u64(mx);
  if (k <= 1) return mn;
  unsigned long long lo = mn, hi = mx;   // count(<= mn) = 1 < k
  while (hi - lo > 1) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    const int c = wave_count_le(v, mid);
    if (c >= k && c <= k + slack) return mid;
    if (c < k) lo = mid; else hi = mid;
  }
  return hi;
}

// Cuts a wave's buffer buf[0, n) to the entries <= T of wave_select: reads
// it into registers, selects, writes the kept entries back to the front.
// Returns T; n becomes the kept count.  (The closing wait covers a buffer in
// LDS; a caller with its buffer in global memory fences around the call.)
template <int J>
__device__ unsigned long long wave_cut(unsigned long long* buf, int& n, int k, int slack) {
  const int lane = threadIdx.x & 63;
  unsigned long long v[J];
#pragma unroll
  for (int j = 0; j < J; ++j) v[j] = j * 64 + lane < n ? buf[j * 64 + lane] : ~0ull;
  const unsigned long long T = wave_select(v, k, slack);
  int m = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool keep = v[j] <= T;
    const unsigned long long bal = __ballot(keep);
    if (keep) buf[m + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = v[j];
    m += __popcll(bal);
  }
  wave_lds_sync();
  n = m;
  return T;
}

}  // namespace pps
