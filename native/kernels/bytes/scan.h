#pragma once
// Sum and exclusive scan of one uint32 per thread over a 256-thread workgroup
// (text.hip's and grep.hip's count / write kernel pairs).
#include "../common.h"

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / HBMR_WAVE;   // s_w: one uint32 per wave

__device__ __forceinline__ uint32_t block_reduce_add(uint32_t v, uint32_t* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int i = 0; i < kScanWaves; ++i) t += s_w[i];
  return t;
}

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* s_w) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t v = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < w; ++i) base += s_w[i];
  return base + v - x;
}

}  // namespace
