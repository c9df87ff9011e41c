// Grep map kernels: DFA regex match → finditer selection → exact span
// aggregate, for GPU Grep (the RegexMapper + LongSumReducer search job).
//
// The reference's grep map (src/mapred/.../lib/RegexMapper.java) emits
// (match, 1) for each non-overlapping match of a line.  On the GPU a split is
// one byte buffer in HBM and the pattern is a leftmost-first DFA compiled on
// the host (hbmr/ops/grep.py):
//
//  1. grep_cand_count / grep_cand_write: one lane per start byte walks the DFA
//     from that byte and keeps the last accepting position (the leftmost-first
//     match end for that start).  A workgroup stages the transition table and
//     the byte classes into LDS once, then streams 4096-byte tiles: 256 lanes
//     × one 16-byte vector load each into an LDS copy of the tile (+ a halo),
//     16 passes of 256 consecutive start bytes, so lane i reads byte i+t at
//     step t.  A walk ends at the dead state, at the line terminator ('\n',
//     or a '\r' right before '\n' or the buffer end — LineRecordReader's rule)
//     where the synthetic end-of-line class is fed once, or at the buffer end.
//     Starts with a match are compacted in position order by a per-tile count,
//     a scan of tile counts and a per-tile rewrite.
//  2. grep_select_count / grep_select_write: finditer's non-overlapping choice
//     is a greedy chain over the candidates.  A candidate that starts at or
//     after the running maximum of all earlier ends is always chosen (a root);
//     one lane walks the chain of each root up to the next root.
//  3. span_insert / span_compact: the two-level exact hash aggregate of
//     bytes/span_table.h (text.hip's) over explicit (start, len) spans (a
//     match may hold spaces and end anywhere): keys are hash tag << 32 | span
//     index + 1.
//  4. lines_count / lines_write: (start, len) of the '\n'-terminated entries
//     of a match table blob, by the tokenizer pair of the same header.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/span_table.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBytes = 16;                   // per lane and vector load
constexpr int kTile = kThreads * kBytes;     // 4096 bytes per tile
constexpr int kHalo = 256;                   // bytes after the tile kept in LDS
constexpr int kPre = 16;                     // bytes before the tile (1 used; keeps 16-B alignment)
constexpr int kWaves = kThreads / HBMR_WAVE;
constexpr int kMaxTable = 16384;             // uint16 entries: 32 KiB of LDS
constexpr int kMaxGrid = 2048;
constexpr uint16_t kAccept = 0x8000;         // bit 15 of an entry: the target state accepts

// 16 bytes at buf[i0..] into dst (16-byte aligned LDS); bytes at or past n read as '\n'.
// Returns the OR of the bytes read.
__device__ __forceinline__ uint32_t stage16(const uint8_t* __restrict__ buf, long n, long i0,
                                            uint8_t* dst) {
  if (i0 + kBytes <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(buf + i0);
    *reinterpret_cast<uint4*>(dst) = v;
    return v.x | v.y | v.z | v.w;
  }
  uint32_t any = 0;
#pragma unroll
  for (int j = 0; j < kBytes; ++j) {
    const uint8_t c = (i0 + j < n) ? buf[i0 + j] : (uint8_t)'\n';
    dst[j] = c;
    any |= c;
  }
  return any;
}

// byte at tile offset k (k >= -1): the LDS copy, or global memory past the halo
__device__ __forceinline__ uint8_t text_at(const uint8_t* s_text, const uint8_t* __restrict__ buf,
                                           long n, long tile0, long k) {
  if (k < kTile + kHalo) return s_text[kPre + k];
  const long i = tile0 + k;
  return i < n ? buf[i] : (uint8_t)'\n';
}

// length of the leftmost-first match starting at tile offset k (0: none)
__device__ __forceinline__ uint32_t dfa_walk(const uint16_t* s_trans, const uint8_t* s_cls,
                                             const uint8_t* s_text,
                                             const uint8_t* __restrict__ buf, long n, long tile0,
                                             int k, int ncls, int start_bol, int start_mid) {
  uint32_t st = s_text[kPre + k - 1] == '\n' ? (uint32_t)start_bol : (uint32_t)start_mid;
  uint32_t best = 0;
  if (st == 0) return 0;
  for (uint32_t t = 0;; ++t) {
    const long kk = (long)k + t;
    const uint8_t c = text_at(s_text, buf, n, tile0, kk);
    bool term = c == '\n';
    if (c == '\r') term = text_at(s_text, buf, n, tile0, kk + 1) == '\n';
    if (term) {
      if (s_trans[st * ncls + ncls - 1] & kAccept) best = t;
      break;
    }
    const uint16_t e = s_trans[st * ncls + s_cls[c]];
    st = e & 0x7fffu;
    if (st == 0) break;
    if (e & kAccept) best = t + 1;
  }
  return best;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void grep_cand_kernel(
    const uint8_t* __restrict__ buf, long n, const uint16_t* __restrict__ table,
    const uint8_t* __restrict__ byteclass, int nent, int ncls, int start_bol, int start_mid,
    long tiles, uint32_t* __restrict__ tile_counts, const long* __restrict__ tile_base,
    uint32_t* __restrict__ pos, uint32_t* __restrict__ len, int64_t* __restrict__ end,
    int* __restrict__ non_ascii) {
  __shared__ uint16_t s_trans[kMaxTable];
  __shared__ uint8_t s_cls[256];
  __shared__ __align__(16) uint8_t s_text[kPre + kTile + kHalo];
  __shared__ uint32_t s_w[kBytes][kWaves];
  for (int i = threadIdx.x; i < nent; i += kThreads) s_trans[i] = table[i];
  s_cls[threadIdx.x] = byteclass[threadIdx.x];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t hi = 0;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the table is staged; the previous tile's readers are done
    const long tile0 = tile * kTile;
    hi |= stage16(buf, n, tile0 + (long)threadIdx.x * kBytes,
                  s_text + kPre + threadIdx.x * kBytes);
    if (threadIdx.x < kHalo / kBytes)
      stage16(buf, n, tile0 + kTile + (long)threadIdx.x * kBytes,
              s_text + kPre + kTile + threadIdx.x * kBytes);
    if (threadIdx.x == 0) s_text[kPre - 1] = tile0 == 0 ? (uint8_t)'\n' : buf[tile0 - 1];
    __syncthreads();
    uint32_t cnt = 0;   // count kernel: this wave's matches; write kernel: matches before this pass
#pragma unroll 1
    for (int p = 0; p < kBytes; ++p) {
      const int k = p * kThreads + threadIdx.x;
      uint32_t m = 0;
      if (tile0 + k < n)
        m = dfa_walk(s_trans, s_cls, s_text, buf, n, tile0, k, ncls, start_bol, start_mid);
      const unsigned long long b = __ballot(m != 0);
      if (!WRITE) {
        cnt += (uint32_t)__popcll(b);
      } else {
        if (lane == 0) s_w[p][w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int i = 0; i < kWaves; ++i) {
          const uint32_t c = s_w[p][i];
          if (i < w) before += c;
          total += c;
        }
        if (m != 0) {
          const long o = tile_base[tile] + cnt + before +
                         (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
          pos[o] = (uint32_t)(tile0 + k);
          len[o] = m;
          end[o] = (int64_t)(tile0 + k) + (int64_t)m;
        }
        cnt += total;
      }
    }
    if (!WRITE) {
      if (lane == 0) s_w[0][w] = cnt;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < kWaves; ++i) t += s_w[0][i];
        tile_counts[tile] = t;
      }
    }
  }
  if (!WRITE) {
    // one flag store per workgroup at the most
    const int any = __syncthreads_or((hi & 0x80808080u) != 0);
    if (any && threadIdx.x == 0) atomicExch(non_ascii, 1);
  }
}

// Running maximum of the candidates' ends, the idiom of the counts: a maximum
// per block of 256, a scan of the block maxima on the host side of the op,
// then the in-block scan on top of each block's prefix.
__global__ __launch_bounds__(kThreads) void grep_block_max_kernel(
    const int64_t* __restrict__ end, long nc, int64_t* __restrict__ block_max) {
  __shared__ long long s_m[kWaves];
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  long long v = j < nc ? (long long)end[j] : 0ll;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; ++i) v = s_m[i] > v ? s_m[i] : v;
    block_max[blockIdx.x] = (int64_t)v;
  }
}

__global__ __launch_bounds__(kThreads) void grep_prefix_max_kernel(
    const int64_t* __restrict__ end, long nc, const int64_t* __restrict__ block_prefix,
    int64_t* __restrict__ pmax) {
  __shared__ long long s_m[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  long long v = j < nc ? (long long)end[j] : 0ll;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o);
    if (lane >= o && u > v) v = u;
  }
  if (lane == 63) s_m[w] = v;
  __syncthreads();
  long long base = (long long)block_prefix[blockIdx.x];
  for (int i = 0; i < w; ++i) base = s_m[i] > base ? s_m[i] : base;
  if (j < nc) pmax[j] = (int64_t)(base > v ? base : v);
}

__device__ __forceinline__ bool is_root(const uint32_t* __restrict__ pos,
                                        const int64_t* __restrict__ pmax, long j) {
  return j == 0 || (int64_t)pos[j] >= pmax[j - 1];
}

// the chain of root j: take a candidate, skip to the first one at or after its
// end, stop at the next root (its own lane walks on from there)
template <bool WRITE>
__device__ __forceinline__ uint32_t walk_chain(const uint32_t* __restrict__ pos,
                                               const uint32_t* __restrict__ len,
                                               const int64_t* __restrict__ pmax, long nc, long j,
                                               long o, uint32_t* __restrict__ spos,
                                               uint32_t* __restrict__ slen) {
  uint32_t cnt = 0;
  long cur = j;
  for (;;) {
    const uint32_t p = pos[cur], l = len[cur];
    if (WRITE) {
      spos[o + cnt] = p;
      slen[o + cnt] = l;
    }
    ++cnt;
    const uint64_t e = (uint64_t)p + l;
    long nxt = cur + 1;
    while (nxt < nc && (uint64_t)pos[nxt] < e) ++nxt;
    if (nxt >= nc || is_root(pos, pmax, nxt)) break;
    cur = nxt;
  }
  return cnt;
}

__global__ __launch_bounds__(kThreads) void grep_select_count_kernel(
    const uint32_t* __restrict__ pos, const uint32_t* __restrict__ len,
    const int64_t* __restrict__ pmax, long nc, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t s_w[kWaves];
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  uint32_t c = 0;
  if (j < nc && is_root(pos, pmax, j))
    c = walk_chain<false>(pos, len, pmax, nc, j, 0, nullptr, nullptr);
  const uint32_t t = block_reduce_add(c, s_w);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void grep_select_write_kernel(
    const uint32_t* __restrict__ pos, const uint32_t* __restrict__ len,
    const int64_t* __restrict__ pmax, long nc, const long* __restrict__ block_base,
    uint32_t* __restrict__ spos, uint32_t* __restrict__ slen) {
  __shared__ uint32_t s_w[kWaves];
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool root = j < nc && is_root(pos, pmax, j);
  uint32_t c = 0;
  if (root) c = walk_chain<false>(pos, len, pmax, nc, j, 0, nullptr, nullptr);
  const uint32_t off = block_excl_scan(c, s_w);
  if (root) walk_chain<true>(pos, len, pmax, nc, j, block_base[blockIdx.x] + off, spos, slen);
}

// ---------------------------------------------------------------- span aggregate
// a span is named by its index into starts / lens
struct SpanRep {
  const uint8_t* buf;
  const uint32_t* starts;
  const uint32_t* lens;
  __device__ __forceinline__ uint32_t item(long w, const uint8_t*& p, uint32_t& len) const {
    len = lens[w];
    p = buf + starts[w];
    return (uint32_t)w;
  }
  __device__ __forceinline__ bool equals(uint32_t rep, const uint8_t* p, uint32_t len) const {
    if (lens[rep] != len) return false;
    const uint8_t* q = buf + starts[rep];
    for (uint32_t i = 0; i < len; ++i)
      if (q[i] != p[i]) return false;
    return true;
  }
  template <class F>
  __device__ __forceinline__ long rep(uint32_t id, uint32_t& s, F each) const {
    s = starts[id];
    const uint32_t len = lens[id];
    for (uint32_t e = 0; e < len; ++e) each(buf[s + e]);
    return (long)s + len;
  }
};

__global__ __launch_bounds__(kInsThreads) void span_insert_kernel(
    const uint8_t* __restrict__ buf, const uint32_t* __restrict__ starts,
    const uint32_t* __restrict__ lens, const int64_t* __restrict__ weights, long nspans,
    unsigned long long* __restrict__ tkeys, unsigned long long* __restrict__ tcounts,
    unsigned long long mask, int* __restrict__ overflow) {
  two_level_insert(SpanRep{buf, starts, lens}, weights, nspans, tkeys, tcounts, mask, overflow);
}

__global__ __launch_bounds__(256) void span_compact_kernel(
    const uint8_t* __restrict__ buf, const uint32_t* __restrict__ starts,
    const uint32_t* __restrict__ lens, const unsigned long long* __restrict__ tkeys,
    const unsigned long long* __restrict__ tcounts, long cap, int R,
    uint32_t* __restrict__ ustart, uint32_t* __restrict__ ulen, int64_t* __restrict__ ucount,
    int32_t* __restrict__ upart, unsigned int* __restrict__ counter) {
  table_compact(SpanRep{buf, starts, lens}, tkeys, tcounts, cap, R, ustart, ulen, ucount, upart,
                counter);
}

// ---------------------------------------------------------------- newline spans
// entry-start bit mask of this lane's 16 bytes: byte 0, or a byte after '\n'
// (the load is written out here: through text.hip's load16 both lines kernels
// compile differently and grep.lines measured 2 % slower)
struct LineStarts {
  __device__ __forceinline__ uint32_t operator()(const uint8_t* __restrict__ buf, long n,
                                                 long i0) const {
    uint8_t b[kTokBytes];
    if (i0 + kTokBytes <= n) {
      const uint4 v = *reinterpret_cast<const uint4*>(buf + i0);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < kTokBytes; ++j) b[j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
    } else {
#pragma unroll
      for (int j = 0; j < kTokBytes; ++j) b[j] = (i0 + j < n) ? buf[i0 + j] : (uint8_t)'\n';
    }
    bool prev_nl = i0 == 0 ? true : buf[i0 - 1] == '\n';
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kTokBytes; ++j) {
      if (prev_nl && i0 + j < n) m |= 1u << j;
      prev_nl = b[j] == '\n';
    }
    return m;
  }
};

struct LineEnd {
  static constexpr long kSkip = 0;   // an entry may be empty
  __device__ __forceinline__ bool operator()(uint8_t c) const { return c == '\n'; }
};

__global__ __launch_bounds__(kTokThreads) void lines_count_kernel(
    const uint8_t* __restrict__ buf, long n, uint32_t* __restrict__ tile_counts) {
  tokenize_count(buf, n, tile_counts, LineStarts{});
}

__global__ __launch_bounds__(kTokThreads) void lines_write_kernel(
    const uint8_t* __restrict__ buf, long n, const long* __restrict__ tile_base,
    uint32_t* __restrict__ starts, uint32_t* __restrict__ lens) {
  tokenize_write(buf, n, tile_base, starts, lens, LineStarts{}, LineEnd{});
}

inline long tiles_of(long n) { return (n + kTile - 1) / kTile; }
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

inline bool bad_dfa(long n, int nstates, int nclasses, int start_bol, int start_mid) {
  return n >= 0xffffffffl || nstates < 1 || nclasses < 2 || nclasses > 256 ||
         (long)nstates * nclasses > kMaxTable || start_bol < 0 || start_bol >= nstates ||
         start_mid < 0 || start_mid >= nstates;
}

}  // namespace

extern "C" {

int hbmr_grep_cand_count(const uint8_t* buf, long n, const uint16_t* table,
                         const uint8_t* byteclass, int nstates, int nclasses, int start_bol,
                         int start_mid, uint32_t* tile_counts, int* non_ascii,
                         hipStream_t stream) {
  const long tiles = tiles_of(n);
  if (tiles == 0) return 0;
  if (misaligned(buf) || bad_dfa(n, nstates, nclasses, start_bol, start_mid))
    return (int)hipErrorInvalidValue;
  const unsigned grid = (unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid);
  hipLaunchKernelGGL(grep_cand_kernel<false>, dim3(grid), dim3(kThreads), 0, stream, buf, n, table,
                     byteclass, nstates * nclasses, nclasses, start_bol, start_mid, tiles,
                     tile_counts, (const long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                     (int64_t*)nullptr, non_ascii);
  return (int)hipGetLastError();
}

int hbmr_grep_cand_write(const uint8_t* buf, long n, const uint16_t* table,
                         const uint8_t* byteclass, int nstates, int nclasses, int start_bol,
                         int start_mid, const long* tile_base, uint32_t* pos, uint32_t* len,
                         int64_t* end, hipStream_t stream) {
  const long tiles = tiles_of(n);
  if (tiles == 0) return 0;
  if (misaligned(buf) || bad_dfa(n, nstates, nclasses, start_bol, start_mid))
    return (int)hipErrorInvalidValue;
  const unsigned grid = (unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid);
  hipLaunchKernelGGL(grep_cand_kernel<true>, dim3(grid), dim3(kThreads), 0, stream, buf, n, table,
                     byteclass, nstates * nclasses, nclasses, start_bol, start_mid, tiles,
                     (uint32_t*)nullptr, tile_base, pos, len, end, (int*)nullptr);
  return (int)hipGetLastError();
}

long hbmr_grep_select_blocks(long nc) { return (nc + kThreads - 1) / kThreads; }

int hbmr_grep_block_max(const int64_t* end, long nc, int64_t* block_max, hipStream_t stream) {
  if (nc == 0) return 0;
  hipLaunchKernelGGL(grep_block_max_kernel, dim3(grid_for(nc, kThreads)), dim3(kThreads), 0,
                     stream, end, nc, block_max);
  return (int)hipGetLastError();
}

// block_prefix[b] = max end of the blocks before b (0 for the first)
int hbmr_grep_prefix_max(const int64_t* end, long nc, const int64_t* block_prefix, int64_t* pmax,
                         hipStream_t stream) {
  if (nc == 0) return 0;
  hipLaunchKernelGGL(grep_prefix_max_kernel, dim3(grid_for(nc, kThreads)), dim3(kThreads), 0,
                     stream, end, nc, block_prefix, pmax);
  return (int)hipGetLastError();
}

int hbmr_grep_select_count(const uint32_t* pos, const uint32_t* len, const int64_t* pmax, long nc,
                           uint32_t* block_counts, hipStream_t stream) {
  if (nc == 0) return 0;
  hipLaunchKernelGGL(grep_select_count_kernel, dim3(grid_for(nc, kThreads)), dim3(kThreads), 0,
                     stream, pos, len, pmax, nc, block_counts);
  return (int)hipGetLastError();
}

int hbmr_grep_select_write(const uint32_t* pos, const uint32_t* len, const int64_t* pmax, long nc,
                           const long* block_base, uint32_t* spos, uint32_t* slen,
                           hipStream_t stream) {
  if (nc == 0) return 0;
  hipLaunchKernelGGL(grep_select_write_kernel, dim3(grid_for(nc, kThreads)), dim3(kThreads), 0,
                     stream, pos, len, pmax, nc, block_base, spos, slen);
  return (int)hipGetLastError();
}

// cap must be a power of two; tkeys/tcounts zeroed by the caller
int hbmr_span_insert(const uint8_t* buf, long n, const uint32_t* starts, const uint32_t* lens,
                     const int64_t* weights, long nspans, uint64_t* tkeys, uint64_t* tcounts,
                     long cap, int* overflow, hipStream_t stream) {
  if (nspans == 0) return 0;
  if (cap <= 0 || (cap & (cap - 1)) != 0 || n >= 0xffffffffl || nspans >= 0xffffffffl)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(span_insert_kernel, dim3(grid_for(nspans, kInsItems)), dim3(kThreads), 0,
                     stream, buf, starts, lens, weights, nspans,
                     reinterpret_cast<unsigned long long*>(tkeys),
                     reinterpret_cast<unsigned long long*>(tcounts),
                     (unsigned long long)(cap - 1), overflow);
  return (int)hipGetLastError();
}

int hbmr_span_compact(const uint8_t* buf, const uint32_t* starts, const uint32_t* lens,
                      const uint64_t* tkeys, const uint64_t* tcounts, long cap, int R,
                      uint32_t* ustart, uint32_t* ulen, int64_t* ucount, int32_t* upart,
                      unsigned int* counter, hipStream_t stream) {
  if (cap == 0) return 0;
  if (R <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(span_compact_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, stream, buf,
                     starts, lens, reinterpret_cast<const unsigned long long*>(tkeys),
                     reinterpret_cast<const unsigned long long*>(tcounts), cap, R, ustart, ulen,
                     ucount, upart, counter);
  return (int)hipGetLastError();
}

int hbmr_lines_count(const uint8_t* buf, long n, uint32_t* tile_counts, hipStream_t stream) {
  const long tiles = tiles_of(n);
  if (tiles == 0) return 0;
  if (misaligned(buf) || n >= 0xffffffffl) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lines_count_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, stream, buf, n,
                     tile_counts);
  return (int)hipGetLastError();
}

int hbmr_lines_write(const uint8_t* buf, long n, const long* tile_base, uint32_t* starts,
                     uint32_t* lens, hipStream_t stream) {
  const long tiles = tiles_of(n);
  if (tiles == 0) return 0;
  if (misaligned(buf) || n >= 0xffffffffl) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lines_write_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, stream, buf, n,
                     tile_base, starts, lens);
  return (int)hipGetLastError();
}

}  // extern "C"
