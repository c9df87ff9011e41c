#pragma once
// Gathers: 64-bit words and records by a permutation, records of several
// splits by (split, row), and by packed record id in 16-B pieces.
#include "../common.h"
#include "collect.h"   // kNoSplit

namespace {

__global__ __launch_bounds__(256) void gather_u64_kernel(const uint64_t* __restrict__ src,
                                                         const uint32_t* __restrict__ perm, long n,
                                                         uint64_t* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[perm[i]];
}

// dst record i = src record perm[i]; records of `words` 4-byte words
__global__ __launch_bounds__(256) void gather_records_kernel(const uint32_t* __restrict__ src,
                                                             const uint32_t* __restrict__ perm,
                                                             long n, int words,
                                                             uint32_t* __restrict__ dst) {
  const long total = n * words;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / words;
    const int w = (int)(e - r * words);
    dst[e] = src[(long)perm[r] * words + w];
  }
}

// dst record i = record row[k] of split split[k], k = perm ? perm[i] : i, with
// U records per lane in flight: the index loads of all U records are issued,
// then their words, then the stores, so each lane keeps U independent random
// reads outstanding (the v1 loop waited on one record at a time).  Lane t
// moves word t % words of record t / words; iteration j of a block covers
// records r0 + j * stride, so the stores of every j stay coalesced.
template <int U>
__global__ __launch_bounds__(256) void gather_records_multi_v3_kernel(
    const uint32_t* const* __restrict__ bases, const uint32_t* __restrict__ split,
    const uint32_t* __restrict__ row, const uint32_t* __restrict__ perm, long n, int words,
    uint32_t* __restrict__ dst) {
  const int rpb = 256 / words;
  const int t = threadIdx.x;
  if (t >= rpb * words) return;
  const int lr = t / words;
  const int w = t - lr * words;
  const long stride = (long)gridDim.x * rpb;
  for (long r0 = (long)blockIdx.x * rpb + lr; r0 < n; r0 += stride * U) {
    const uint32_t* src[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long r = r0 + j * stride;
      src[j] = nullptr;
      if (r < n) {
        const long k = perm ? (long)perm[r] : r;
        const uint32_t sp = split[k];
        if (sp != kNoSplit) src[j] = bases[sp] + (long)row[k] * words;
      }
    }
    uint32_t v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = src[j] ? src[j][w] : 0u;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long r = r0 + j * stride;
      if (src[j]) dst[r * words + w] = v[j];
    }
  }
}

// The record gather by packed id (gid = split << 24 | row: one dependent index
// load per record), in 16-B pieces: a record of W words is
// moved by L = ceil(W / 4) lanes, lane c the 16 B at word 4c (the last lane
// the remaining 1-4 words) — 7 lanes per 100-B TeraSort record, not a lane per
// word, so a wave keeps 9 records x U in flight per round instead of 2.5 x U, with
// 16-B loads/stores at the record's 4-B alignment (global memory takes
// dword-aligned vector accesses).  The lane holding words 0-3 also writes the
// record's key (hi byte-swapped from words 0-1, lo from word 2's bytes 8-9).
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef u32x4_t __attribute__((aligned(4))) u32x4_a4;
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef u32x2_t __attribute__((aligned(4))) u32x2_a4;

template <int U>
__global__ __launch_bounds__(256) void gather_records_gid16_kernel(
    const uint32_t* const* __restrict__ bases, const uint32_t* __restrict__ gid,
    const uint64_t* packed, long n,
    int words, uint32_t* __restrict__ dst, uint32_t* __restrict__ khi,
    uint64_t* __restrict__ klo, uint32_t* __restrict__ kwin) {
  const int L = (words + 3) >> 2;            // lanes per record
  const int rpw = HBMR_WAVE / L;             // records per wave
  const int lane = threadIdx.x & (HBMR_WAVE - 1), wave = threadIdx.x / HBMR_WAVE;
  if (lane >= rpw * L) return;               // (no barrier in this kernel)
  const int lr = lane / L;
  const int c = lane - lr * L;
  const int w0 = 4 * c;                      // first word of this lane's piece
  const int nw = words - w0 < 4 ? words - w0 : 4;
  const long rpb = (long)rpw * (256 / HBMR_WAVE);
  const long stride = (long)gridDim.x * rpb;
  for (long r0 = (long)blockIdx.x * rpb + wave * rpw + lr; r0 < n; r0 += stride * U) {
    const uint32_t* src[U];
    uint32_t win[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long r = r0 + j * stride;
      src[j] = nullptr;
      win[j] = 0u;
      if (r < n) {
        uint32_t g;
        if (packed) {
          const uint64_t pk = packed[r];
          g = (uint32_t)pk;
          win[j] = (uint32_t)(pk >> 32);
        } else {
          g = gid[r];
        }
        src[j] = bases[g >> 24] + (long)(g & 0xFFFFFFu) * words + w0;
      }
    }
    u32x4_t v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      v[j] = u32x4_t{0u, 0u, 0u, 0u};
      if (!src[j]) continue;
      if (nw == 4) {
        v[j] = *reinterpret_cast<const u32x4_a4*>(src[j]);
      } else if (nw == 2) {
        const u32x2_t t = *reinterpret_cast<const u32x2_a4*>(src[j]);
        v[j].x = t.x;
        v[j].y = t.y;
      } else {
        v[j].x = src[j][0];
        if (nw > 1) v[j].y = src[j][1];
        if (nw > 2) v[j].z = src[j][2];
      }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long r = r0 + j * stride;
      if (r >= n) continue;
      uint32_t* d = dst + r * words + w0;
      if (nw == 4) {
        *reinterpret_cast<u32x4_a4*>(d) = v[j];
      } else if (nw == 2) {
        *reinterpret_cast<u32x2_a4*>(d) = u32x2_t{v[j].x, v[j].y};
      } else {
        d[0] = v[j].x;
        if (nw > 1) d[1] = v[j].y;
        if (nw > 2) d[2] = v[j].z;
      }
      if (khi != nullptr && c == 0) {
        khi[2 * r + 1] = __builtin_bswap32(v[j].x);   // hi = bytes 0-7, big-endian
        khi[2 * r] = __builtin_bswap32(v[j].y);
        klo[r] = ((uint64_t)(v[j].z & 0xFFu) << 8) | ((v[j].z >> 8) & 0xFFu);   // bytes 8-9
        if (kwin != nullptr) kwin[r] = win[j];    // the sort window, for the tie fix
      }
    }
  }
}

}  // namespace
