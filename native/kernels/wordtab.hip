// Word-table kernels: the reduce side of the word-count family
// (hbmr/ops/wordtab.py holds the definition and the CPU twins;
// hbmr/models/wordtable.py is the job).
//
// A word table is a byte buffer, (start, len) int32 per word and an int64 count
// per word.  A part of the output is the words of one partition in
// compareBytes order, one "word\tcount\n" line each.
//
//  1. wordtab_partition: parts[i] = (h & INT_MAX) % nparts, h =
//     WritableComparator.hashBytes of the word (31 * h + signed byte) started
//     from `seed`: 1 is Text(word)'s partition; hashBytes(prefix) is the
//     partition of Text(prefix + word) without building that key.  One lane per
//     word.
//  2. wordtab_lengths: bytes of the line of record order[i]: the word, '\t', the
//     decimal count (a signed int64: 1-19 digits and the sign), '\n'.
//  3. wordtab_fill: output-tile-centric.  A workgroup owns 4 KiB of the
//     destination, cut at 16-byte boundaries of memory.  It finds the records that
//     overlap its tile by a binary search in the int64 offsets, composes their
//     text into LDS (LDS byte x is a fixed destination byte: lanes run over the
//     records, each writing its count from the back and a word of up to 32 bytes;
//     longer words are queued in LDS in pieces of 1 KiB, and a wave copies a piece
//     with 16-byte loads into aligned LDS slots) and stores the tile as aligned
//     16-byte vectors.  Only the first and last slot of the whole text can be
//     partial: those go bytewise.  A word longer than a tile is copied by several
//     workgroups; no two workgroups write the same 16-byte slot, and no byte
//     outside dst[0, offs[n]) is written.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/scan.h"

namespace {

constexpr int kThreads = kScanThreads;                 // 256
constexpr int kTileBytes = 4096;
constexpr int kTileSlots = kTileBytes / 16;            // one slot per lane
constexpr int kShortWord = 32;                         // longer words are shared by a wave
constexpr int kPieceSlots = 64;                        // slots of a queued piece: one per lane of a wave
// a tile holds at most 4096 / (33 + 3) + 2 queued words and 256 / 64 + 1 extra pieces
constexpr int kQueue = 128;

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

__global__ __launch_bounds__(kThreads) void wordtab_partition_kernel(
    const uint8_t* __restrict__ buf, const int32_t* __restrict__ starts,
    const int32_t* __restrict__ lens, long n, uint32_t seed, uint32_t nparts,
    int32_t* __restrict__ parts) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = buf + starts[i];
  const int len = lens[i];
  uint32_t h = seed;
  for (int j = 0; j < len; ++j) h = h * 31u + (uint32_t)(int32_t)(int8_t)p[j];
  parts[i] = (int32_t)((h & 0x7fffffffu) % nparts);
}

// decimal characters of v, the sign included
__device__ __forceinline__ int count_chars(int64_t v) {
  uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  int d = 1;
  uint64_t p = 10;
#pragma unroll
  for (int k = 1; k < 19; ++k, p *= 10) d += u >= p;   // 10^1 .. 10^18; |v| <= 2^63 < 10^19
  return d + (v < 0);
}

__global__ __launch_bounds__(kThreads) void wordtab_lengths_kernel(
    const int32_t* __restrict__ lens, const int64_t* __restrict__ counts,
    const int32_t* __restrict__ order, long n, int32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const long r = order != nullptr ? (long)order[i] : i;
  out[i] = lens[r] + 2 + count_chars(counts[r]);
}

// the record that holds byte v of the text: the last i with offs[i] <= v
// (offs[0] = 0 <= v < offs[n], offs strictly ascending)
__device__ __forceinline__ long record_of(const int64_t* __restrict__ offs, long n, long v) {
  long lo = 0, hi = n;                                 // offs[lo] <= v < offs[hi]
  while (hi - lo > 1) {
    const long mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void wordtab_fill_kernel(
    const uint8_t* __restrict__ buf, const int32_t* __restrict__ starts,
    const int32_t* __restrict__ lens, const int64_t* __restrict__ counts,
    const int32_t* __restrict__ order, const int64_t* __restrict__ offs, long n,
    uint8_t* __restrict__ dst) {
  __shared__ uint4 s_slots[kTileSlots];
  __shared__ uint32_t s_queue[kQueue];
  __shared__ uint32_t s_queued;
  uint8_t* s = reinterpret_cast<uint8_t*>(s_slots);
  const long total = offs[n];
  const int mis = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
  // LDS byte x is dst[t0 + x]; the tile's bytes of the text are dst[lo, hi)
  const long t0 = (long)blockIdx.x * kTileBytes - mis;
  const long lo = t0 < 0 ? 0 : t0;
  const long hi = t0 + kTileBytes < total ? t0 + kTileBytes : total;
  if (lo >= hi) return;                                // the same in every lane
  if (threadIdx.x == 0) s_queued = 0;
  __syncthreads();
  const long r0 = record_of(offs, n, lo), r1 = record_of(offs, n, hi - 1);
  const int xlo = (int)(lo - t0), xhi = (int)(hi - t0);
  for (long r = r0 + threadIdx.x; r <= r1; r += kThreads) {
    const long id = order != nullptr ? (long)order[r] : r;
    const long o = offs[r], end = offs[r + 1];
    const int wl = lens[id];
    // the count, from the back: '\n', the digits from the least significant, the
    // sign, '\t' (positions relative to the tile; most are inside it)
    long x = end - t0;
    const int64_t c = counts[id];
    uint64_t u = c < 0 ? 0ull - (uint64_t)c : (uint64_t)c;
    --x;
    if (x >= xlo && x < xhi) s[x] = '\n';
    do {
      uint32_t digit;
      if (u >> 32) {
        digit = (uint32_t)(u % 10u);
        u /= 10u;
      } else {
        const uint32_t v = (uint32_t)u;
        digit = v % 10u;
        u = v / 10u;
      }
      --x;
      if (x >= xlo && x < xhi) s[x] = (uint8_t)('0' + digit);
    } while (u != 0);
    if (c < 0) {
      --x;
      if (x >= xlo && x < xhi) s[x] = '-';
    }
    --x;
    if (x >= xlo && x < xhi) s[x] = '\t';
    // the word: dst[o, o + wl), of which [a, e) lies in the tile
    const long a = o > lo ? o : lo, e = o + wl < hi ? o + wl : hi;
    if (a >= e) continue;
    const uint8_t* src = buf + starts[id];
    bool own = wl <= kShortWord;
    if (!own) {
      // pieces of kPieceSlots of the tile's slots, counted from the slot of a
      const int q0 = (int)(a - t0) >> 4, q1 = (int)(e - 1 - t0) >> 4;
      const int pieces = (q1 - q0) / kPieceSlots + 1;
      const uint32_t at = atomicAdd(&s_queued, (uint32_t)pieces);
      if (at + pieces <= kQueue) {
        for (int k = 0; k < pieces; ++k) s_queue[at + k] = (uint32_t)(r - r0) << 8 | (uint32_t)k;
      } else {
        own = true;                                    // (the queue holds every tile's pieces: a guard)
      }
    }
    if (own)
      for (long b = a; b < e; ++b) s[b - t0] = src[b - o];
  }
  __syncthreads();
  const uint32_t queued = s_queued < (uint32_t)kQueue ? s_queued : (uint32_t)kQueue;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t k = wave; k < queued; k += kScanWaves) {
    const uint32_t entry = s_queue[k];
    const long r = r0 + (entry >> 8);
    if (r > r1) continue;                              // (entries come from r0..r1: a guard)
    const long id = order != nullptr ? (long)order[r] : r;
    const long o = offs[r];
    const int wl = lens[id];
    const long a = o > lo ? o : lo, e = o + wl < hi ? o + wl : hi;
    const uint8_t* src = buf + starts[id];
    const int q = ((int)(a - t0) >> 4) + (int)(entry & 0xff) * kPieceSlots + lane;
    // slot q of the tile: dst[t0 + 16 q, + 16), of which [b, f) belongs to the word
    const long slot = t0 + 16L * q;
    const long b = slot > a ? slot : a, f = slot + 16 < e ? slot + 16 : e;
    if (b >= f) continue;
    if (f - b == 16) {
      uint4 v;
      __builtin_memcpy(&v, src + (b - o), 16);         // inside the word, at the source's alignment
      s_slots[q] = v;
    } else {
      for (long y = b; y < f; ++y) s[y - t0] = src[y - o];
    }
  }
  __syncthreads();
  {
    const int q = threadIdx.x;
    const long slot = t0 + 16L * q;
    const long b = slot > lo ? slot : lo, f = slot + 16 < hi ? slot + 16 : hi;
    if (b < f) {
      if (f - b == 16) {
        *reinterpret_cast<uint4*>(dst + slot) = s_slots[q];
      } else {
        for (long y = b; y < f; ++y) dst[y] = s[y - t0];
      }
    }
  }
}

inline bool grid_fits(long blocks) { return blocks < (1L << 31); }

}  // namespace

extern "C" {

int hbmr_wordtab_tile_bytes() { return kTileBytes; }

// parts[n] = (h & INT_MAX) % nparts, h = hashBytes of buf[starts[i], + lens[i])
// started from seed (the caller checks that the words lie in the buffer)
int hbmr_wordtab_partition(const uint8_t* buf, const int32_t* starts, const int32_t* lens, long n,
                           unsigned seed, int nparts, int32_t* parts, hipStream_t st) {
  if (n <= 0) return 0;
  const long blocks = ceil_div(n, kThreads);
  if (nparts <= 0 || !grid_fits(blocks) || buf == nullptr || starts == nullptr ||
      lens == nullptr || parts == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wordtab_partition_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, buf,
                     starts, lens, n, seed, (uint32_t)nparts, parts);
  return (int)hipGetLastError();
}

// out[i] = lens[order[i]] + 1 + chars(counts[order[i]]) + 1 (order null: i)
int hbmr_wordtab_lengths(const int32_t* lens, const int64_t* counts, const int32_t* order, long n,
                         int32_t* out, hipStream_t st) {
  if (n <= 0) return 0;
  const long blocks = ceil_div(n, kThreads);
  if (!grid_fits(blocks) || lens == nullptr || counts == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wordtab_lengths_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, lens,
                     counts, order, n, out);
  return (int)hipGetLastError();
}

// dst[offs[i] : offs[i + 1]) = "word\tcount\n" of record order[i] (null: i); offs[n + 1]
// is the exclusive scan of hbmr_wordtab_lengths over the same records, total =
// offs[n] bytes fit in dst and the words lie in buf (the caller checks).  No other
// byte of dst is written.
int hbmr_wordtab_fill(const uint8_t* buf, const int32_t* starts, const int32_t* lens,
                      const int64_t* counts, const int32_t* order, const int64_t* offs, long n,
                      long total, uint8_t* dst, hipStream_t st) {
  if (n <= 0 || total <= 0) return 0;
  const long mis = (long)(reinterpret_cast<uintptr_t>(dst) & 15);
  const long tiles = ceil_div(mis + total, kTileBytes);
  if (!grid_fits(tiles) || buf == nullptr || starts == nullptr || lens == nullptr ||
      counts == nullptr || offs == nullptr || dst == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wordtab_fill_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, buf, starts,
                     lens, counts, order, offs, n, dst);
  return (int)hipGetLastError();
}

}  // extern "C"
