#pragma once
// Byte-string records in HBM, shared by recsort.hip, recjoin.hip,
// recvalidate.hip and recgen.hip: the round key and the compare of key payloads
// (WritableComparator.compareBytes: unsigned bytes, a proper prefix first), the
// splitmix64 finaliser, and the destination-aligned slots of the two
// variable-length copies and of the record fill.
#include "../common.h"

namespace {

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// the 64-bit round key of a payload with `left` bytes at p: (p[0 : 7]
// zero-padded, big-endian) << 8 | min(left, 8); 8 = the key continues
__device__ __forceinline__ uint64_t round_key(const uint8_t* p, long left) {
  const int nb = left < 7 ? (int)left : 7;
  uint64_t k = 0;
#pragma unroll
  for (int j = 0; j < 7; ++j) k = (k << 8) | (j < nb ? (uint64_t)p[j] : 0);
  return (k << 8) | (uint64_t)(left < 8 ? left : 8);
}

// compareBytes(a, b) given that the first `from` bytes are equal, 8 bytes a step
__device__ __forceinline__ int compare_from(const uint8_t* a, long la, const uint8_t* b, long lb,
                                            long from) {
  const long n = la < lb ? la : lb;
  long i = from;
  for (; i + 8 <= n; i += 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + i, 8);
    __builtin_memcpy(&y, b + i, 8);
    if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
  }
  for (; i < n; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

// the splitmix64 finaliser: the record digest's word hash and the record
// generator's counter hash
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

constexpr int kCopyLanes = 16;                 // lanes per copy chunk
constexpr int kCopyChunk = kCopyLanes * 16;    // bytes of a chunk: 16 slots of 16 bytes

// The run dst[a, end) is cut into chunks of 16 of its DESTINATION-aligned
// 16-byte slots.  Slot `lane` of chunk c begins at offset `slot` of dst (a
// multiple of 16 in memory; below a for the run's first slot) and holds the
// run's bytes [b, e); false if it holds none.
__device__ __forceinline__ bool slot_span(const uint8_t* dst, long a, long end, long c, int lane,
                                          long& slot, long& b, long& e) {
  const long mis = (long)(reinterpret_cast<uintptr_t>(dst + a) & 15);
  slot = a - mis + c * kCopyChunk + lane * 16L;
  b = slot > a ? slot : a;
  e = slot + 16 < end ? slot + 16 : end;
  return b < e;
}

// Lane `lane` of chunk c of the run dst[a, end) copies its slot: a full slot
// is one 16-byte load (at whatever alignment the source has) and one aligned
// 16-byte store, the partial slots at the run's head and tail go bytewise.
// src_of_a() gives the source address of byte a; it is asked only by a lane
// that has bytes to copy.
template <class Src>
__device__ __forceinline__ void copy_slot(uint8_t* __restrict__ dst, long a, long end, long c,
                                          int lane, Src src_of_a) {
  long slot, b, e;
  if (!slot_span(dst, a, end, c, lane, slot, b, e)) return;
  const uint8_t* q = src_of_a() + (b - a);
  if (e - b == 16) {
    uint4 v;
    __builtin_memcpy(&v, q, 16);
    *reinterpret_cast<uint4*>(dst + b) = v;
  } else {
    for (; b < e; ++b, ++q) dst[b] = *q;
  }
}

}  // namespace
