// Record validation kernels: what SortValidator asks of a SequenceFile split that
// lies in HBM as recsort.hip has it (a byte buffer plus, per record, the offset
// and length of its frame [recordLen][keyLen][key][value] and of its key
// payload).
//
//  1. recvalidate_digest: an order-free digest of the records.  A frame of L
//     bytes is m = ceil(L / 8) little-endian words w_j counted from the frame's
//     first byte (bytes past L are zero), so the digest does not depend on where
//     the frame lies in the buffer.  With mix() the splitmix64 finaliser,
//       s = sum_j mix(w_j + (j + 1) * 0x9E3779B97F4A7C15)
//       h = mix(s ^ (L * 0xD6E8FEB86659FD93))             (all mod 2^64)
//     and the split's digest is (records, sum(L - 8), sum h, sum h^2).  The inner
//     sum is commutative, so the lanes take the words in any order; the outer
//     mix is not linear, so two records cannot trade words unnoticed.  A group
//     of 16 lanes walks a whole record, 16 bytes a lane and 256 bytes a step:
//     a full slot is one 16-byte load at whatever alignment the frame has (four
//     steps' loads at a time while the record has them), the slot that holds the
//     frame's end is cut out of a load of the frame's last 16 bytes (a frame
//     below 16 bytes goes bytewise), so no load leaves the frame and the sync
//     escapes between frames are never read.  The groups
//     stride over the records, the finalise is fused in, and the four totals
//     take one atomic each per workgroup after a block reduction.
//  2. recvalidate_order: the number of records whose key is below their
//     predecessor's (compareBytes on the payload; equal keys are no descent),
//     one thread per adjacent pair, one atomic per workgroup.
//
// The partition check needs no kernel of its own: recsort_hash_part gives the
// partition of every record and the host side counts those off the expected one.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/records.h"
#include "bytes/scan.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kLanes = 16;                    // lanes per record
constexpr int kStep = kLanes * 16;            // bytes a lane group covers in one step
constexpr int kGroups = kThreads / kLanes;    // records a workgroup works on at a time
constexpr int kMaxBlocks = 4096;              // the groups stride over the records beyond
constexpr uint64_t kWordMul = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kLenMul = 0xD6E8FEB86659FD93ull;

__device__ __forceinline__ uint64_t word_hash(uint64_t w, long j) {
  return mix64(w + (uint64_t)(j + 1) * kWordMul);
}

// sum of v over the workgroup, in thread 0; s_w: one uint64 per wave
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
  for (int i = 0; i < kScanWaves; ++i) t += s_w[i];
  return t;
}

__global__ __launch_bounds__(kThreads) void recvalidate_digest_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ foff,
    const int64_t* __restrict__ flen, long n, unsigned long long* __restrict__ out) {
  __shared__ uint64_t s_w[4][kScanWaves];
  const int lane = threadIdx.x % kLanes;
  const long stride = (long)gridDim.x * kGroups;
  uint64_t tot[4] = {0, 0, 0, 0};              // records, bytes, sum h, sum h^2 (lane 0 of a group)
  for (long r = (long)blockIdx.x * kGroups + threadIdx.x / kLanes; r < n; r += stride) {
    const uint8_t* p = data + foff[r];         // a record's 16 lanes stay together
    const long len = flen[r];
    uint64_t s = 0;
    long o = lane * 16L;
    // four steps at a time while all four slots are whole: their loads are in flight together
    for (; o + 3 * kStep + 16 <= len; o += 4 * kStep) {
      uint64_t v[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) __builtin_memcpy(v[u], p + o + u * kStep, 16);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long j = (o + u * kStep) >> 3;
        s += word_hash(v[u][0], j) + word_hash(v[u][1], j + 1);
      }
    }
    for (; o < len; o += kStep) {
      uint64_t w0 = 0, w1 = 0;
      if (o + 16 <= len) {
        uint64_t v[2];
        __builtin_memcpy(v, p + o, 16);
        w0 = v[0];
        w1 = v[1];
      } else if (len >= 16) {
        // the frame ends in this slot: its bytes are the top of the frame's last 16
        uint64_t t[2];
        __builtin_memcpy(t, p + len - 16, 16);
        const int sh = (int)(o + 16 - len);    // 1..15 of those bytes lie before the slot
        if (sh < 8) {
          w0 = (t[0] >> (8 * sh)) | (t[1] << (64 - 8 * sh));
          w1 = t[1] >> (8 * sh);
        } else {
          w0 = t[1] >> (8 * (sh - 8));
        }
      } else {
        for (int b = 0; b < (int)(len - o); ++b) {   // a frame below 16 bytes: bytewise
          const uint64_t x = (uint64_t)p[o + b] << (8 * (b & 7));
          if (b < 8) w0 |= x;
          else w1 |= x;
        }
      }
      s += word_hash(w0, o >> 3);
      if (o + 8 < len) s += word_hash(w1, (o >> 3) + 1);
    }
#pragma unroll
    for (int d = kLanes / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, kLanes);
    if (lane == 0) {
      const uint64_t h = mix64(s ^ ((uint64_t)len * kLenMul));
      tot[0] += 1;
      tot[1] += (uint64_t)(len - 8);
      tot[2] += h;
      tot[3] += h * h;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t t = block_sum_u64(tot[k], s_w[k]);
    if (threadIdx.x == 0) atomicAdd(out + k, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(kThreads) void recvalidate_order_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ koff,
    const int64_t* __restrict__ klen, long n, unsigned long long* __restrict__ unsorted) {
  __shared__ uint32_t s_w[kScanWaves];
  const long stride = (long)gridDim.x * kThreads;
  uint32_t c = 0;                              // n < 2^31
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x + 1; i < n; i += stride)
    if (compare_from(data + koff[i], klen[i], data + koff[i - 1], klen[i - 1], 0) < 0) ++c;
  const uint32_t t = block_reduce_add(c, s_w);
  if (threadIdx.x == 0 && t) atomicAdd(unsorted, (unsigned long long)t);
}

inline unsigned grid_of(long blocks) {
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace

extern "C" {

// out[4] (uint64, set here): the records, sum(flen - 8), sum h and sum h^2 mod
// 2^64 of the n frames data[foff[i] : + flen[i]] (h: the frame digest above).
int hbmr_recvalidate_digest(const uint8_t* data, const int64_t* foff, const int64_t* flen, long n,
                            uint64_t* out, hipStream_t st) {
  const hipError_t rc = hipMemsetAsync(out, 0, 4 * sizeof(uint64_t), st);
  if (rc != hipSuccess) return (int)rc;
  if (n <= 0) return 0;
  if (n >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recvalidate_digest_kernel, dim3(grid_of(ceil_div(n, kGroups))), dim3(kThreads),
                     0, st, data, foff, flen, n, reinterpret_cast<unsigned long long*>(out));
  return (int)hipGetLastError();
}

// *unsorted (uint64, set here): the records i in [1, n) whose key payload is
// below that of record i - 1.
int hbmr_recvalidate_order(const uint8_t* data, const int64_t* koff, const int64_t* klen, long n,
                           uint64_t* unsorted, hipStream_t st) {
  const hipError_t rc = hipMemsetAsync(unsorted, 0, sizeof(uint64_t), st);
  if (rc != hipSuccess) return (int)rc;
  if (n <= 1) return 0;
  if (n >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recvalidate_order_kernel, dim3(grid_of(ceil_div(n - 1, kThreads))),
                     dim3(kThreads), 0, st, data, koff, klen, n,
                     reinterpret_cast<unsigned long long*>(unsorted));
  return (int)hipGetLastError();
}

}  // extern "C"
