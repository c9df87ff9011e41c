// Text map kernels: tokenize → exact hash-aggregate
// (the fused combiner) → Java-hash partition → pack, for GPU WordCount.
//
// The reference's WordCount map (src/examples/.../WordCount.java and the Pipes
// wordcount-simple.cc:34-41) emits (word, 1) per token, and the combiner /
// reducer sums per word after a sort by key.  On the GPU a split is one byte
// buffer in HBM:
//
//  1. wc_tokenize_count / wc_tokenize_write: word starts (a non-space byte
//     whose predecessor is a space or the buffer start; spaces are the ASCII
//     whitespace set of the CPU mapper) compacted in order by a per-tile count,
//     a scan of tile counts and a per-tile rewrite.  Each lane owns 16
//     consecutive bytes read as one 16-byte vector load.
//  2. wc_insert: open-addressing tables of 64-bit keys (32-bit hash tag |
//     representative start + 1) claimed by 64-bit CAS; a tag match is
//     confirmed by comparing the bytes of the representative occurrence, so
//     the aggregation is exact (no hash-only merging).  Each workgroup folds
//     its words into an LDS table first and inserts every distinct word once
//     into the global (HBM) table.  Counts are 64-bit atomics; an optional
//     weight per word makes the same kernel merge partial (word, count) tables.
//  3. wc_compact: occupied slots → (start, len, count, partition), partition =
//     (Text.hashCode() & INT_MAX) % R with hashCode = WritableComparator.
//     hashBytes (31·h + signed byte, h0 = 1), i.e. Hadoop's HashPartitioner.
//  4. wc_pack: words (in a given order) → "word\n" blob for the shuffle.
// Steps 1 to 3 are the templates of bytes/span_table.h, which grep.hip uses
// over match spans; this file says what a word is.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/span_table.h"

namespace {

__device__ __forceinline__ bool is_space(uint8_t c) {
  // bytes.split(): space, \t, \n, \v, \f, \r
  return c == ' ' || (c >= 9 && c <= 13);
}

// this lane's 16 bytes; bytes at or past n read as a space
__device__ __forceinline__ void load16(const uint8_t* __restrict__ buf, long n, long i0,
                                       uint8_t b[kTokBytes]) {
  if (i0 + kTokBytes <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(buf + i0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < kTokBytes; ++j) b[j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
  } else {
#pragma unroll
    for (int j = 0; j < kTokBytes; ++j) b[j] = (i0 + j < n) ? buf[i0 + j] : (uint8_t)' ';
  }
}

// start-of-word bit mask of this lane's 16 bytes
struct WordStarts {
  __device__ __forceinline__ uint32_t operator()(const uint8_t* __restrict__ buf, long n,
                                                 long i0) const {
    uint8_t b[kTokBytes];
    load16(buf, n, i0, b);
    bool prev_space = (i0 == 0) ? true : (i0 - 1 < n ? is_space(buf[i0 - 1]) : true);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kTokBytes; ++j) {
      const bool sp = is_space(b[j]);
      if (!sp && prev_space && i0 + j < n) m |= 1u << j;
      prev_space = sp;
    }
    return m;
  }
};

struct WordEnd {
  static constexpr long kSkip = 1;   // a word's first byte is no space
  __device__ __forceinline__ bool operator()(uint8_t c) const { return is_space(c); }
};

__global__ __launch_bounds__(kTokThreads) void wc_tokenize_count_kernel(
    const uint8_t* __restrict__ buf, long n, uint32_t* __restrict__ tile_counts) {
  tokenize_count(buf, n, tile_counts, WordStarts{});
}

__global__ __launch_bounds__(kTokThreads) void wc_tokenize_write_kernel(
    const uint8_t* __restrict__ buf, long n, const long* __restrict__ tile_base,
    uint32_t* __restrict__ starts, uint32_t* __restrict__ lens) {
  tokenize_write(buf, n, tile_base, starts, lens, WordStarts{}, WordEnd{});
}

// a word is named by its start offset and ends at whitespace
struct WordRep {
  const uint8_t* buf;
  long n;
  const uint32_t* starts;
  const uint32_t* lens;
  __device__ __forceinline__ uint32_t item(long w, const uint8_t*& p, uint32_t& len) const {
    const uint32_t s = starts[w];
    len = lens[w];
    p = buf + s;
    return s;
  }
  __device__ __forceinline__ bool equals(uint32_t rs, const uint8_t* p, uint32_t len) const {
    for (uint32_t i = 0; i < len; ++i)
      if ((long)rs + i >= n || buf[rs + i] != p[i]) return false;
    return !((long)rs + len < n && !is_space(buf[rs + len]));
  }
  template <class F>
  __device__ __forceinline__ long rep(uint32_t rs, uint32_t& s, F each) const {
    s = rs;
    long e = s;
    while (e < n && !is_space(buf[e])) each(buf[e++]);
    return e;
  }
};

__global__ __launch_bounds__(kInsThreads) void wc_insert_kernel(
    const uint8_t* __restrict__ buf, long n, const uint32_t* __restrict__ starts,
    const uint32_t* __restrict__ lens, const int64_t* __restrict__ weights, long nwords,
    unsigned long long* __restrict__ tkeys, unsigned long long* __restrict__ tcounts,
    unsigned long long mask, int* __restrict__ overflow) {
  two_level_insert(WordRep{buf, n, starts, lens}, weights, nwords, tkeys, tcounts, mask, overflow);
}

__global__ __launch_bounds__(256) void wc_compact_kernel(
    const uint8_t* __restrict__ buf, long n, const unsigned long long* __restrict__ tkeys,
    const unsigned long long* __restrict__ tcounts, long cap, int R,
    uint32_t* __restrict__ ustart, uint32_t* __restrict__ ulen, int64_t* __restrict__ ucount,
    int32_t* __restrict__ upart, unsigned int* __restrict__ counter) {
  table_compact(WordRep{buf, n, nullptr, nullptr}, tkeys, tcounts, cap, R, ustart, ulen, ucount,
                upart, counter);
}

__global__ __launch_bounds__(256) void wc_pack_kernel(
    const uint8_t* __restrict__ buf, const uint32_t* __restrict__ ustart,
    const uint32_t* __restrict__ ulen, const int64_t* __restrict__ order, long nu,
    const int64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nu) return;
  const long u = order ? order[i] : i;
  const uint8_t* src = buf + ustart[u];
  const uint32_t len = ulen[u];
  uint8_t* dst = out + out_off[i];
  for (uint32_t j = 0; j < len; ++j) dst[j] = src[j];
  dst[len] = '\n';
}

}  // namespace

extern "C" {

long hbmr_wc_tiles(long n) { return (n + kTokTile - 1) / kTokTile; }

int hbmr_wc_tokenize_count(const uint8_t* buf, long n, uint32_t* tile_counts,
                           hipStream_t stream) {
  const long tiles = hbmr_wc_tiles(n);
  if (tiles == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(buf) & 15u) != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wc_tokenize_count_kernel, dim3((unsigned)tiles), dim3(kTokThreads), 0,
                     stream, buf, n, tile_counts);
  return (int)hipGetLastError();
}

int hbmr_wc_tokenize_write(const uint8_t* buf, long n, const long* tile_base, uint32_t* starts,
                           uint32_t* lens, hipStream_t stream) {
  const long tiles = hbmr_wc_tiles(n);
  if (tiles == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(buf) & 15u) != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wc_tokenize_write_kernel, dim3((unsigned)tiles), dim3(kTokThreads), 0,
                     stream, buf, n, tile_base, starts, lens);
  return (int)hipGetLastError();
}

// cap must be a power of two; tkeys/tcounts zeroed by the caller
int hbmr_wc_insert(const uint8_t* buf, long n, const uint32_t* starts, const uint32_t* lens,
                   const int64_t* weights, long nwords, uint64_t* tkeys, uint64_t* tcounts,
                   long cap, int* overflow, hipStream_t stream) {
  if (nwords == 0) return 0;
  if (cap <= 0 || (cap & (cap - 1)) != 0 || n >= 0xffffffffl) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wc_insert_kernel, dim3(grid_for(nwords, kInsItems)), dim3(kInsThreads), 0,
                     stream, buf, n,
                     starts, lens, weights, nwords,
                     reinterpret_cast<unsigned long long*>(tkeys),
                     reinterpret_cast<unsigned long long*>(tcounts),
                     (unsigned long long)(cap - 1), overflow);
  return (int)hipGetLastError();
}

int hbmr_wc_compact(const uint8_t* buf, long n, const uint64_t* tkeys, const uint64_t* tcounts,
                    long cap, int R, uint32_t* ustart, uint32_t* ulen, int64_t* ucount,
                    int32_t* upart, unsigned int* counter, hipStream_t stream) {
  if (cap == 0) return 0;
  if (R <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wc_compact_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, stream, buf, n,
                     reinterpret_cast<const unsigned long long*>(tkeys),
                     reinterpret_cast<const unsigned long long*>(tcounts), cap, R, ustart, ulen,
                     ucount, upart, counter);
  return (int)hipGetLastError();
}

int hbmr_wc_pack(const uint8_t* buf, const uint32_t* ustart, const uint32_t* ulen,
                 const int64_t* order, long nu, const int64_t* out_off, uint8_t* out,
                 hipStream_t stream) {
  if (nu == 0) return 0;
  hipLaunchKernelGGL(wc_pack_kernel, dim3(grid_for(nu, 256)), dim3(256), 0, stream, buf, ustart,
                     ulen, order, nu, out_off, out);
  return (int)hipGetLastError();
}

}  // extern "C"
