#pragma once
// TeraGen: Hadoop 1.0.3 TeraGen records bit for bit, generated on the device.
#include "../common.h"

namespace {

// ------------------------------------------------------------------------ TeraSort
// Affine LCG x' = a x + c (mod 2^32): state after `steps` from x0 by squaring.
__device__ __forceinline__ uint32_t lcg_jump(uint64_t steps, uint32_t x) {
  uint32_t ma = 3141592621u, mc = 663896637u;  // the map for 2^i steps
  uint32_t ra = 1u, rc = 0u;                    // accumulated map
  while (steps) {
    if (steps & 1) {
      rc = ma * rc + mc;
      ra = ma * ra;
    }
    mc = ma * mc + mc;
    ma = ma * ma;
    steps >>= 1;
  }
  return ra * x + rc;
}

// Record r (100 B): 10 key bytes (3 LCG draws at iterations 3r+1..3r+3, each
// /52 then 4 base-95 printable digits), the row id right-aligned in 10 chars,
// 78 filler letters starting at 'A' + (8r mod 26), "\r\n".
__global__ __launch_bounds__(256) void teragen_kernel(long first_row, long nrows,
                                                      uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows) return;
  const long row = first_row + i;
  uint8_t rec[100];
  uint32_t s = lcg_jump((uint64_t)row * 3u, 0u);
  uint8_t kb[12];
  for (int q = 0; q < 3; ++q) {
    s = 3141592621u * s + 663896637u;
    uint64_t temp = (uint64_t)s / 52u;
    kb[3 + 4 * q] = (uint8_t)(' ' + temp % 95);
    temp /= 95;
    kb[2 + 4 * q] = (uint8_t)(' ' + temp % 95);
    temp /= 95;
    kb[1 + 4 * q] = (uint8_t)(' ' + temp % 95);
    temp /= 95;
    kb[4 * q] = (uint8_t)(' ' + temp % 95);
  }
  for (int j = 0; j < 10; ++j) rec[j] = kb[j];
  // row id as Java's Integer.toString((int) rowId), right-aligned in 10 chars
  int32_t rid = (int32_t)row;
  char digits[12];
  int nd = 0;
  bool neg = rid < 0;
  uint32_t u = neg ? (uint32_t)(-(int64_t)rid) : (uint32_t)rid;
  do {
    digits[nd++] = (char)('0' + u % 10);
    u /= 10;
  } while (u);
  if (neg) digits[nd++] = '-';
  const int len = nd < 10 ? nd : 10;
  for (int j = 0; j < 10 - len; ++j) rec[10 + j] = ' ';
  for (int j = 0; j < len; ++j) rec[10 + (10 - len) + j] = (uint8_t)digits[nd - 1 - j];
  const int fb = (int)((row * 8) % 26);
  for (int q = 0; q < 7; ++q)
    for (int j = 0; j < 10; ++j) rec[20 + 10 * q + j] = (uint8_t)('A' + (fb + q) % 26);
  for (int j = 0; j < 8; ++j) rec[90 + j] = (uint8_t)('A' + (fb + 7) % 26);
  rec[98] = '\r';
  rec[99] = '\n';
  uint32_t* o = reinterpret_cast<uint32_t*>(out + i * 100);
  for (int j = 0; j < 25; ++j) {
    uint32_t wv;
    __builtin_memcpy(&wv, rec + 4 * j, 4);
    o[j] = wv;
  }
}

}  // namespace
