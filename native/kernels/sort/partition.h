#pragma once
// TeraSort map side: key words, the range partition of every record and the
// scatter into partition order; splitter search of a sorted run; KeyWindow,
// the dense key window the packed reduce sorts by.
#include "../common.h"
#include "radix.h"

namespace {

// hi = key bytes 0..7 big-endian, lo = bytes 8..9 (unsigned lexicographic order
// of the 10-byte key == order of (hi, lo))
__global__ __launch_bounds__(256) void tera_keys_kernel(const uint8_t* __restrict__ rec, long n,
                                                        int stride, uint64_t* __restrict__ hi,
                                                        uint64_t* __restrict__ lo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* r = rec + i * stride;
  uint64_t h = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) h = (h << 8) | r[j];
  hi[i] = h;
  lo[i] = ((uint64_t)r[8] << 8) | r[9];
}

// offsets[p] = first position whose (hi, lo) >= splitter p-1 (p = 1..R-1);
// offsets[0] = 0, offsets[R] = n
__global__ void split_offsets_kernel(const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo,
                                     long n, const uint64_t* __restrict__ shi,
                                     const uint64_t* __restrict__ slo, int nparts,
                                     long* __restrict__ offsets) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > nparts) return;
  if (p == 0) {
    offsets[0] = 0;
    return;
  }
  if (p == nparts) {
    offsets[nparts] = n;
    return;
  }
  const uint64_t kh = shi[p - 1], kl = slo[p - 1];
  long a = 0, b = n;
  while (a < b) {
    const long m = (a + b) >> 1;
    const bool less = hi[m] < kh || (hi[m] == kh && lo[m] < kl);
    if (less) a = m + 1; else b = m;
  }
  offsets[p] = a;
}

// The range partition of a record: pid = number of splitters <= key (partition
// p holds keys in [split[p-1], split[p]), as split_offsets cuts a sorted run).
// The count kernels stage the splitters in LDS once per workgroup; each
// workgroup then walks a grid-stride slice of the records.
constexpr int kMaxSplitters = 4096;

// An order-preserving map of a key's high word to a dense integer: with every
// key byte in [m, m + R) (the job's key alphabet: the maps measure the OR of
// all key bytes, so m = 0 and R = 2^bits — 128 for printable keys),
// v(h) = the 8 bytes of h as base-R digits, and the window (v(h) - vlo) >> sh
// for a group whose keys' v lie in [vlo, vlo + span), sh chosen so the
// window fits in 32 bits.  For printable keys (R = 128) the window keeps ~30
// bits of the group's spread where the raw top 32 bits of h keep ~22 (their
// bytes use 95 of 256 codes and the group fixes most of the first one).
// R = 256, m = 0, vlo = 0 is the plain shift h >> sh.
struct KeyWindow {
  uint64_t vlo;
  uint32_t m, R;
  int sh;
};

__device__ __forceinline__ uint64_t key_window(uint64_t h, const KeyWindow& kw) {
  uint64_t v = 0;
#pragma unroll
  for (int b = 7; b >= 0; --b) v = v * kw.R + (((h >> (8 * b)) & 0xFFu) - kw.m);
  return (v - kw.vlo) >> kw.sh;
}

// running OR of a high word's bytes (folded to one byte at the flush): every
// key byte is at most the OR of all of them, so [0, 2^bits(OR)) is an
// alphabet that holds them; and the key checksum sum(hi + lo) mod 2^64 the
// map reports.  A few VALU per record: this kernel is latency bound (the
// splitter search), and a per-record byte or word min / max cost it 2.4x.
__device__ __forceinline__ void byte_range(uint64_t h, uint32_t l, uint32_t& orb, uint64_t& sum) {
  orb |= (uint32_t)h | (uint32_t)(h >> 32);
  sum += h + l;
}

// the block's (OR of key bytes, key checksum) into parts[blockIdx] — no
// global atomics on one address (across 8 XCDs they serialise at ~0.2 us
// each: 16k blocks cost the kernel 3.5 ms); reduce_pairs_kernel folds them
__device__ __forceinline__ void flush_byte_range(uint32_t orb, uint64_t sum,
                                                 unsigned long long* s_ks,
                                                 unsigned long long* parts) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    orb |= __shfl_xor(orb, o);
    sum += __shfl_xor(sum, o);
  }
  orb |= orb >> 16;
  orb |= orb >> 8;
  if ((threadIdx.x & 63) == 0) {
    atomicOr(&s_ks[0], (unsigned long long)(orb & 0xFFu));
    atomicAdd(&s_ks[1], (unsigned long long)sum);
  }
  __syncthreads();
  if (threadIdx.x == 0 && parts != nullptr) {
    parts[2 * blockIdx.x] = s_ks[0];
    parts[2 * blockIdx.x + 1] = s_ks[1];
  }
}

// ---- TeraSort map v3: partition without a sort ------------------------------
// (A) key words + partition id of every record, and the partition sizes: a
// per-workgroup LDS histogram flushed with one global add per touched bin.
__global__ __launch_bounds__(256) void tera_part_count_kernel(
    const uint8_t* __restrict__ rec, long n, int stride, const uint64_t* __restrict__ shi,
    const uint64_t* __restrict__ slo, int nsplit, uint64_t* __restrict__ hi,
    uint64_t* __restrict__ lo, uint16_t* __restrict__ pid, unsigned int* __restrict__ counts,
    unsigned long long* __restrict__ kmm) {
  __shared__ uint64_t s_hi[kMaxSplitters];
  __shared__ uint16_t s_lo[kMaxSplitters];
  __shared__ unsigned int s_cnt[kMaxSplitters + 1];
  __shared__ unsigned long long s_ks[2];
  uint32_t korb = 0u;
  uint64_t ksum = 0;
  const int nparts = nsplit + 1;
  for (int j = threadIdx.x; j < nsplit; j += 256) {
    s_hi[j] = shi[j];
    s_lo[j] = (uint16_t)slo[j];
  }
  for (int j = threadIdx.x; j < nparts; j += 256) s_cnt[j] = 0u;
  if (threadIdx.x == 0) {
    s_ks[0] = 0ull;
    s_ks[1] = 0ull;
  }
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const uint8_t* r = rec + i * stride;
    uint64_t h = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) h = (h << 8) | r[j];
    const uint32_t l = ((uint32_t)r[8] << 8) | r[9];
    int a = 0, b = nsplit;
    while (a < b) {
      const int m = (a + b) >> 1;
      const bool le = s_hi[m] < h || (s_hi[m] == h && s_lo[m] <= l);
      if (le) a = m + 1; else b = m;
    }
    hi[i] = h;
    lo[i] = l;
    pid[i] = (uint16_t)a;
    atomicAdd(&s_cnt[a], 1u);
    byte_range(h, l, korb, ksum);
  }
  flush_byte_range(korb, ksum, s_ks, kmm);
  for (int j = threadIdx.x; j < nparts; j += 256)
    if (s_cnt[j]) atomicAdd(&counts[j], s_cnt[j]);
}

// exclusive scan of the partition sizes (one workgroup; nparts <= 4097)
__global__ __launch_bounds__(1024) void tera_part_offsets_kernel(
    const unsigned int* __restrict__ counts, int nparts, unsigned int* __restrict__ cursor,
    long* __restrict__ offsets) {
  __shared__ long s_w[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  constexpr int kPer = 5;   // 1024 * 5 >= 4097
  long v[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    v[j] = idx < nparts ? (long)counts[idx] : 0;
    sum += v[j];
  }
  long x = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long u = __shfl_up(x, o);
    if (lane >= o) x += u;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  long run = x - sum;
  for (int i = 0; i < w; ++i) run += s_w[i];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    if (idx < nparts) {
      offsets[idx] = run;
      cursor[idx] = (unsigned int)run;
    }
    run += v[j];
    if (idx == nparts - 1) offsets[nparts] = run;
  }
}

// (B) scatter (hi, lo, row) into partition order.  Each workgroup takes a tile
// of kSortTile records, ranks them per partition in LDS, reserves one range per
// touched partition from the global cursors, and writes.  Order inside a
// partition follows the reservation order (the reduce sorts by key anyway).
__global__ __launch_bounds__(kSortThreads) void tera_part_scatter_kernel(
    const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo,
    const uint16_t* __restrict__ pid, long n, int nparts, unsigned int* __restrict__ cursor,
    uint64_t* __restrict__ ohi, uint64_t* __restrict__ olo, uint32_t* __restrict__ orow) {
  __shared__ unsigned int s_cnt[kMaxSplitters + 1];
  const int t = threadIdx.x;
  const long base = (long)blockIdx.x * kSortTile;
  for (int j = t; j < nparts; j += kSortThreads) s_cnt[j] = 0u;
  __syncthreads();
  unsigned int loc[kSortItems];
  uint16_t p[kSortItems];
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const long e = base + (long)i * kSortThreads + t;
    if (e < n) {
      p[i] = pid[e];
      loc[i] = atomicAdd(&s_cnt[p[i]], 1u);
    }
  }
  __syncthreads();
  for (int j = t; j < nparts; j += kSortThreads) {
    const unsigned int c = s_cnt[j];
    s_cnt[j] = c ? atomicAdd(&cursor[j], c) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const long e = base + (long)i * kSortThreads + t;
    if (e < n) {
      const long d = (long)s_cnt[p[i]] + loc[i];
      ohi[d] = hi[e];
      olo[d] = lo[e];
      orow[d] = (uint32_t)e;
    }
  }
}

// (A') key / partition / count with the key read as 3 dwords (the record
// stride is a multiple of 4: bytes 0-11 of every record are 4-B aligned)
// instead of 10 byte loads per record.
__global__ __launch_bounds__(256) void tera_part_count_w_kernel(
    const uint32_t* __restrict__ rec, long n, int stride_words, const uint64_t* __restrict__ shi,
    const uint64_t* __restrict__ slo, int nsplit, uint64_t* __restrict__ hi,
    uint64_t* __restrict__ lo, uint16_t* __restrict__ pid, unsigned int* __restrict__ counts,
    unsigned long long* __restrict__ kmm) {
  // LDS sized by the splitter count (part_count_w_lds), not a static
  // 4096-entry table (56 KB: two workgroups per CU).  The kernel reads about
  // every sector of the records (a 12-byte key every 100 bytes), so it runs
  // near the copy rate; a 12-bit prefix table that spared 98 % of the
  // splitter searches measured no faster.
  extern __shared__ __align__(16) unsigned char s_dyn[];
  uint64_t* s_hi = reinterpret_cast<uint64_t*>(s_dyn);
  unsigned int* s_cnt = reinterpret_cast<unsigned int*>(s_hi + nsplit);
  uint16_t* s_lo = reinterpret_cast<uint16_t*>(s_cnt + nsplit + 1);
  __shared__ unsigned long long s_ks[2];
  uint32_t korb = 0u;
  uint64_t ksum = 0;
  const int nparts = nsplit + 1;
  for (int j = threadIdx.x; j < nsplit; j += 256) {
    s_hi[j] = shi[j];
    s_lo[j] = (uint16_t)slo[j];
  }
  for (int j = threadIdx.x; j < nparts; j += 256) s_cnt[j] = 0u;
  if (threadIdx.x == 0) {
    s_ks[0] = 0ull;
    s_ks[1] = 0ull;
  }
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const uint32_t* r = rec + i * stride_words;
    const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
    const uint64_t h = ((uint64_t)__builtin_bswap32(w0) << 32) | __builtin_bswap32(w1);
    const uint32_t l = ((w2 & 0xFFu) << 8) | ((w2 >> 8) & 0xFFu);
    int a = 0, b = nsplit;
    while (a < b) {
      const int m = (a + b) >> 1;
      const bool le = s_hi[m] < h || (s_hi[m] == h && s_lo[m] <= l);
      if (le) a = m + 1; else b = m;
    }
    hi[i] = h;
    lo[i] = l;
    pid[i] = (uint16_t)a;
    atomicAdd(&s_cnt[a], 1u);
    byte_range(h, l, korb, ksum);
  }
  flush_byte_range(korb, ksum, s_ks, kmm);
  for (int j = threadIdx.x; j < nparts; j += 256)
    if (s_cnt[j]) atomicAdd(&counts[j], s_cnt[j]);
}

}  // namespace
