#pragma once
// Items of a byte buffer and their exact hash aggregate, shared by text.hip
// (words) and grep.hip (match spans, table entries).
//
// Tokenizer pair: each lane owns 16 consecutive bytes read as one 16-byte
// vector load; item starts are compacted in order by a per-tile count, a scan
// of tile counts (the caller's) and a per-tile rewrite.  `Starts` gives the
// start bit mask of a lane's 16 bytes; `End` says whether a byte ends an item
// and has kSkip, the bytes from an item's start that need no look.
//
// Aggregate: open-addressing tables of 64-bit keys (32-bit hash tag | id + 1)
// claimed by 64-bit CAS; a tag match is confirmed by comparing bytes with the
// representative the id names, so the aggregation is exact.  Counts are 64-bit
// atomics; an optional weight per item merges partial tables.  A policy `Rep`
// says how an id names its representative:
//   uint32_t item(long w, const uint8_t*& p, uint32_t& len)  bytes of item w; returns its id
//   bool equals(uint32_t id, const uint8_t* p, uint32_t len) the representative has these bytes
//   long rep(uint32_t id, uint32_t& s, F each)                the representative is buf[s : e];
//                                                             returns e, calls each(byte) in order
// and has the member `buf`.
#include "scan.h"

namespace {

constexpr int kTokThreads = kScanThreads;
constexpr int kTokBytes = 16;                      // per lane
constexpr int kTokTile = kTokThreads * kTokBytes;  // 4096 bytes per workgroup

template <class Starts>
__device__ __forceinline__ void tokenize_count(const uint8_t* __restrict__ buf, long n,
                                               uint32_t* __restrict__ tile_counts, Starts starts) {
  __shared__ uint32_t s_w[kScanWaves];
  const long i0 = (long)blockIdx.x * kTokTile + (long)threadIdx.x * kTokBytes;
  const uint32_t c = i0 < n ? (uint32_t)__popc(starts(buf, n, i0)) : 0u;
  const uint32_t t = block_reduce_add(c, s_w);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = t;
}

template <class Starts, class End>
__device__ __forceinline__ void tokenize_write(const uint8_t* __restrict__ buf, long n,
                                               const long* __restrict__ tile_base,
                                               uint32_t* __restrict__ starts,
                                               uint32_t* __restrict__ lens, Starts mask, End end) {
  __shared__ uint32_t s_w[kScanWaves];
  const long i0 = (long)blockIdx.x * kTokTile + (long)threadIdx.x * kTokBytes;
  uint32_t m = i0 < n ? mask(buf, n, i0) : 0u;
  const uint32_t off = block_excl_scan((uint32_t)__popc(m), s_w);
  long o = tile_base[blockIdx.x] + off;
  while (m) {
    const int j = __ffs(m) - 1;
    m &= m - 1;
    const long s = i0 + j;
    long e = s + End::kSkip;
    while (e < n && !end(buf[e])) ++e;
    starts[o] = (uint32_t)s;
    lens[o] = (uint32_t)(e - s);
    ++o;
  }
}

__device__ __forceinline__ uint64_t bytes_hash64(const uint8_t* p, uint32_t len) {
  uint64_t h = 1469598103934665603ull;  // FNV-1a
  for (uint32_t i = 0; i < len; ++i) h = (h ^ p[i]) * 1099511628211ull;
  h ^= h >> 33;                          // murmur3 fmix64
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// insert (key = tag | id + 1) with weight into the global table
template <class Rep>
__device__ __forceinline__ bool global_insert(const Rep& r, uint64_t h, unsigned long long key,
                                              const uint8_t* p, uint32_t len,
                                              unsigned long long wt,
                                              unsigned long long* __restrict__ tkeys,
                                              unsigned long long* __restrict__ tcounts,
                                              unsigned long long mask) {
  unsigned long long slot = h & mask;
  // a probe run this long means the table is too full: report overflow and let
  // the host retry with a larger table instead of crawling
  const unsigned long long max_probe = mask < 4096ull ? mask : 4096ull;
  for (unsigned long long probe = 0; probe <= max_probe; ++probe) {
    unsigned long long cur = tkeys[slot];
    if (cur == 0ull) {
      cur = atomicCAS(&tkeys[slot], 0ull, key);
      if (cur == 0ull) {
        atomicAdd(&tcounts[slot], wt);
        return true;
      }
    }
    if ((cur >> 32) == (key >> 32) && r.equals((uint32_t)(cur & 0xffffffffull) - 1u, p, len)) {
      atomicAdd(&tcounts[slot], wt);
      return true;
    }
    slot = (slot + 1) & mask;
  }
  return false;
}

constexpr int kInsThreads = 256;
constexpr int kInsPerThread = 16;
constexpr int kInsItems = kInsThreads * kInsPerThread;  // items per workgroup
constexpr int kLdsSlots = 2048;                         // 32 KiB of LDS
constexpr int kLdsProbes = 32;

// Two-level aggregation: a workgroup first folds its 4096 items into an LDS
// table (hot items — the Zipf head of natural text, a frequent match —
// collapse there instead of hammering one global counter), then inserts each
// distinct item once into the global table with its local count.  Items that
// find no LDS slot within kLdsProbes go straight to the global table.
template <class Rep>
__device__ __forceinline__ void two_level_insert(const Rep& r, const int64_t* weights,
                                                 long nitems,
                                                 unsigned long long* tkeys,
                                                 unsigned long long* tcounts,
                                                 unsigned long long mask,
                                                 int* overflow) {
  __shared__ unsigned long long s_keys[kLdsSlots];
  __shared__ unsigned long long s_cnt[kLdsSlots];
  for (int i = threadIdx.x; i < kLdsSlots; i += kInsThreads) {
    s_keys[i] = 0ull;
    s_cnt[i] = 0ull;
  }
  __syncthreads();
  const long w0 = (long)blockIdx.x * kInsItems;
  bool ovf = false;
#pragma unroll 1
  for (int j = 0; j < kInsPerThread; ++j) {
    const long w = w0 + (long)j * kInsThreads + threadIdx.x;
    if (w >= nitems) break;
    const uint8_t* p;
    uint32_t len;
    const uint32_t id = r.item(w, p, len);
    const uint64_t h = bytes_hash64(p, len);
    const unsigned long long key = ((h >> 32) << 32) | (unsigned long long)(id + 1u);
    const unsigned long long wt = weights ? (unsigned long long)weights[w] : 1ull;
    uint32_t slot = (uint32_t)(h >> 7) & (kLdsSlots - 1);
    bool done = false;
    for (int probe = 0; probe < kLdsProbes && !done; ++probe) {
      unsigned long long cur = s_keys[slot];
      if (cur == 0ull) {
        cur = atomicCAS(&s_keys[slot], 0ull, key);
        if (cur == 0ull) {
          atomicAdd(&s_cnt[slot], wt);
          done = true;
          break;
        }
      }
      if ((cur >> 32) == (key >> 32) && r.equals((uint32_t)(cur & 0xffffffffull) - 1u, p, len)) {
        atomicAdd(&s_cnt[slot], wt);
        done = true;
        break;
      }
      slot = (slot + 1) & (kLdsSlots - 1);
    }
    if (!done && !global_insert(r, h, key, p, len, wt, tkeys, tcounts, mask)) ovf = true;
  }
  __syncthreads();
  // flush: each distinct item of this workgroup once into the global table
  for (int i = threadIdx.x; i < kLdsSlots; i += kInsThreads) {
    const unsigned long long key = s_keys[i];
    if (key == 0ull) continue;
    uint32_t s;
    const uint32_t len =
        (uint32_t)(r.rep((uint32_t)(key & 0xffffffffull) - 1u, s, [](uint8_t) {}) - s);
    const uint8_t* p = r.buf + s;
    const uint64_t h = bytes_hash64(p, len);
    if (!global_insert(r, h, key, p, len, s_cnt[i], tkeys, tcounts, mask)) ovf = true;
  }
  if (ovf) atomicExch(overflow, 1);
}

// occupied slots → (start, len, count, partition), partition = (Text.hashCode()
// & INT_MAX) % R with hashCode = WritableComparator.hashBytes (31·h + signed
// byte, h0 = 1), i.e. Hadoop's HashPartitioner
template <class Rep>
__device__ __forceinline__ void table_compact(const Rep& r,
                                              const unsigned long long* __restrict__ tkeys,
                                              const unsigned long long* __restrict__ tcounts,
                                              long cap, int R, uint32_t* __restrict__ ustart,
                                              uint32_t* __restrict__ ulen,
                                              int64_t* __restrict__ ucount,
                                              int32_t* __restrict__ upart,
                                              unsigned int* __restrict__ counter) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const unsigned long long k = tkeys[i];
  if (k == 0ull) return;
  uint32_t s, jh = 1u;
  const long e = r.rep((uint32_t)(k & 0xffffffffull) - 1u, s, [&](uint8_t c) {
    jh = 31u * jh + (uint32_t)(int32_t)(int8_t)c;
  });
  const unsigned int o = atomicAdd(counter, 1u);
  ustart[o] = s;
  ulen[o] = (uint32_t)(e - s);
  ucount[o] = (int64_t)tcounts[i];
  upart[o] = (int32_t)(((int32_t)jh & 0x7fffffff) % R);
}

inline int grid_for(long n, int per) { return (int)((n + per - 1) / per); }

}  // namespace
