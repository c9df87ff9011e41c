#pragma once
// Tie fix: after a sort on part of the key, order each run of equal sorted
// prefixes by the rest (lo and the permutation; or keys and records in place).
#include "../common.h"
#include "partition.h"

namespace {

// After a sort by hi only: order each run of equal hi by lo (insertion sort,
// carrying perm).  Runs are rare for TeraSort keys (8 of 10 key bytes in hi);
// a run longer than kTieRun is left alone and flagged, and the caller falls
// back to the full 80-bit sort.
constexpr int kTieRun = 64;

__global__ __launch_bounds__(256) void tera_tie_fix_kernel(const uint64_t* __restrict__ hi,
                                                           uint64_t* __restrict__ lo,
                                                           uint32_t* __restrict__ perm, long n,
                                                           unsigned int* __restrict__ flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n - 1) return;
  const uint64_t h = hi[i];
  if (hi[i + 1] != h || (i > 0 && hi[i - 1] == h)) return;   // not the start of a run
  long e = i + 1;
  while (e < n && hi[e] == h && e - i < kTieRun) ++e;
  if (e < n && hi[e] == h) {
    atomicOr(flag, 1u);
    return;
  }
  for (long a = i + 1; a < e; ++a) {
    const uint64_t kl = lo[a];
    const uint32_t kp = perm[a];
    long b = a - 1;
    while (b >= i && lo[b] > kl) {
      lo[b + 1] = lo[b];
      perm[b + 1] = perm[b];
      --b;
    }
    lo[b + 1] = kl;
    perm[b + 1] = kp;
  }
}

// After the sort on a window of the high key word and the record gather:
// order each run of an equal sorted prefix (hi >> shift) by the full key
// (hi, lo), moving hi, lo and the (already gathered) records themselves.
// Two passes, one thread per record: (1) a record in a run ranks itself
// among the run's members by (hi, lo, position) and, if its place changes,
// copies itself to a compact scratch slot with its destination; (2) every
// scratch slot is written to its destination.  Runs longer than kTieRun (or
// more moved records than the scratch holds) are flagged for the full-key
// path.  A 32-bit window over ~12M keys leaves equal prefixes on a few
// percent of them, in pairs and triples.
__global__ __launch_bounds__(256) void tera_tie_rank_kernel(
    const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo,
    const uint32_t* __restrict__ rec, long n, int words, KeyWindow kw,
    const uint32_t* __restrict__ win, long cap, unsigned int* __restrict__ cnt,
    uint32_t* __restrict__ sdst, uint64_t* __restrict__ shi, uint64_t* __restrict__ slo,
    uint32_t* __restrict__ srec, unsigned int* __restrict__ flag) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  // the records' windows: as the gather stored them, else recomputed from hi
  auto wnd = [&](long x) -> uint64_t { return win ? (uint64_t)win[x] : key_window(hi[x], kw); };
  const uint64_t h = wnd(j);
  const bool prev = j > 0 && wnd(j - 1) == h;
  const bool next = j + 1 < n && wnd(j + 1) == h;
  if (!prev && !next) return;
  const uint64_t hj = hi[j], lj = lo[j];
  long s0 = j, e = j + 1;
  while (s0 > 0 && wnd(s0 - 1) == h && j - s0 < kTieRun) --s0;
  while (e < n && wnd(e) == h && e - j < kTieRun) ++e;
  if ((s0 > 0 && wnd(s0 - 1) == h) || (e < n && wnd(e) == h) || e - s0 > kTieRun) {
    atomicOr(flag, 1u);
    return;
  }
  long rank = 0;
  for (long k = s0; k < e; ++k) {
    const uint64_t hk = hi[k], lk = lo[k];
    rank += hk < hj || (hk == hj && (lk < lj || (lk == lj && k < j)));
  }
  const long d = s0 + rank;
  if (d == j) return;
  const unsigned int slot = atomicAdd(cnt, 1u);
  if ((long)slot >= cap) {
    atomicOr(flag, 1u);
    return;
  }
  sdst[slot] = (uint32_t)d;
  shi[slot] = hj;
  slo[slot] = lj;
  for (int w = 0; w < words; ++w) srec[(long)slot * words + w] = rec[j * words + w];
}

__global__ __launch_bounds__(256) void tera_tie_move_kernel(
    uint64_t* __restrict__ hi, uint64_t* __restrict__ lo, uint32_t* __restrict__ rec, int words,
    long cap, const unsigned int* __restrict__ cnt, const uint32_t* __restrict__ sdst,
    const uint64_t* __restrict__ shi, const uint64_t* __restrict__ slo,
    const uint32_t* __restrict__ srec) {
  const long m = min((long)*cnt, cap);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long)gridDim.x * 256) {
    const long d = sdst[i];
    hi[d] = shi[i];
    lo[d] = slo[i];
    for (int w = 0; w < words; ++w) rec[d * words + w] = srec[i * words + w];
  }
}

}  // namespace
