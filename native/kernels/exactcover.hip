// Pentomino counting (DistributedPentomino's map,
// src/examples/.../dancing/DistributedPentomino.java) as an exact-cover search
// over bit masks.  The search itself is include/hbmr/exactcover_core.h, shared
// with the C++ counter of native/cpu/exactcover.cc, so CPU and GPU slots count
// the same thing the same way.
//
//   exactcover_expand_count_kernel / exactcover_expand_write_kernel
//       one breadth-first level, one lane per state: the children of each state
//       counted, then (after the host's exclusive scan of the counts) written
//       at their offsets.  They turn a map's few prefixes into enough states to
//       fill the device.  The table is read from global memory (it stays in L2).
//   exactcover_count_kernel
//       depth-first count below each frontier state.  A group of kGroup lanes
//       shares one state: every pass of the loop the group tests kGroup rows of
//       the current bucket, one a lane, and takes the first that fits (a
//       ballot), or moves on kGroup rows, or pops when the bucket is exhausted
//       -- ec_step() of exactcover_core.h with the bucket walk split over the
//       group.  One lane per state was the other arm of the A/B: it has kGroup
//       times the states in flight but walks each subtree kGroup times slower,
//       and the longest subtrees of a launch set its end (one-sided 5x18:
//       981 ms at its best depth against 420 ms for groups of 16; 4, 8, 32 and
//       64 lanes were between or behind; profiles/pentomino_1gpu.json).
//       The placement table and the bucket offsets are staged in LDS; a
//       group's stack is one uint16 row index per depth, [depth][group] in
//       LDS (undo is by XOR).  Groups take states from a global work counter
//       (one atomic per wave and fetch), so a group that finishes a subtree
//       takes the next state while its neighbours are still deep in theirs.
//       The loop ends when the counter is past the last state and every
//       group's stack is empty: depth is at most the piece count and every
//       level walks a finite bucket.  No workgroup waits for another.  Counts
//       go to counts[prefix]: a group adds its count when its prefix changes,
//       and what is left at the end is reduced over the wave and added with
//       one 64-bit atomic when the wave ends on one prefix (the usual case:
//       states arrive in prefix order).
#include "../include/hbmr/exactcover_core.h"
#include "common.h"

namespace {

using namespace hbmr_ec;

constexpr int kExpandThreads = 256;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kLdsKeep = 1024;  // left to the runtime
constexpr int kGroup = 16;      // lanes that share a state in the count kernel

template <int W>
__global__ __launch_bounds__(kExpandThreads) void exactcover_expand_count_kernel(
    Table<W> t, const uint64_t* __restrict__ states, long n, int32_t* __restrict__ nchild) {
  const long s = (long)blockIdx.x * kExpandThreads + threadIdx.x;
  if (s >= n) return;
  const Mask<W> full = ec_full<W>(t.ncells);
  nchild[s] = ec_children(t, full, states + s * (W + 1), [](const Mask<W>&, uint64_t) {});
}

template <int W>
__global__ __launch_bounds__(kExpandThreads) void exactcover_expand_write_kernel(
    Table<W> t, const uint64_t* __restrict__ states, long n, const int64_t* __restrict__ child_off,
    long base, long capacity, uint64_t* __restrict__ out) {
  const long s = (long)blockIdx.x * kExpandThreads + threadIdx.x;
  if (s >= n) return;
  const Mask<W> full = ec_full<W>(t.ncells);
  long o = child_off[s] - base;
  ec_children(t, full, states + s * (W + 1), [&](const Mask<W>& occ, uint64_t last) {
    if (o >= 0 && o < capacity) {  // offsets that do not belong to these states write nothing
      for (int k = 0; k < W; ++k) out[o * (W + 1) + k] = occ.w[k];
      out[o * (W + 1) + W] = last;
    }
    ++o;
  });
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = HBMR_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, HBMR_WAVE);
  return v;
}

template <int W>
__global__ __launch_bounds__(1024) void exactcover_count_kernel(
    const uint64_t* __restrict__ gm, const uint32_t* __restrict__ gp,
    const int32_t* __restrict__ goff, int nrows, int ncells, const uint64_t* __restrict__ states,
    long n, long nprefixes, unsigned long long* scratch, unsigned long long* counts,
    unsigned long long* wg_clock) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  uint64_t* s_m = (uint64_t*)s_dyn;
  uint32_t* s_p = (uint32_t*)(s_m + (size_t)W * nrows);
  int32_t* s_off = (int32_t*)(s_p + nrows);
  uint16_t* s_stack = (uint16_t*)(s_off + ncells + 1);  // [kMaxPieces][blockDim.x / G]
  constexpr int G = kGroup;
  const int tid = threadIdx.x, lane = tid & (HBMR_WAVE - 1);
  const int gl = lane % G, gbase = lane - gl;  // place in the group, the group's first lane
  if (wg_clock && tid == 0) wg_clock[2 * blockIdx.x] = wall_clock64();
  for (int i = tid; i < W * nrows; i += blockDim.x) s_m[i] = gm[i];
  for (int i = tid; i < nrows; i += blockDim.x) s_p[i] = gp[i];
  for (int i = tid; i <= ncells; i += blockDim.x) s_off[i] = goff[i];
  __syncthreads();

  const Table<W> t{s_m, s_p, s_off, nrows, ncells};
  const Mask<W> full = ec_full<W>(ncells);
  Lane<W> l;  // the same in every lane of a group
  for (int k = 0; k < W; ++k) l.occ.w[k] = 0;
  l.used = 0;
  l.d = -1;
  l.i = l.e = 0;
  uint16_t* stack = s_stack + tid / G;
  const int stride = blockDim.x / G;
  bool done = false;
  uint32_t src = 0;
  unsigned long long cnt = 0;  // kept by the group's first lane
  uint64_t nodes = 0;
  for (;;) {
    const bool gneed = l.d < 0 && !done;
    const unsigned long long want = __ballot(gneed && gl == 0);
    if (want) {
      const int leader = __builtin_ctzll(want);
      unsigned long long first = 0;
      if (lane == leader) first = atomicAdd(&scratch[0], (unsigned long long)__popcll(want));
      first = __shfl(first, leader, HBMR_WAVE);
      unsigned long long s = first + __popcll(want & ((1ull << lane) - 1));
      s = __shfl(s, gbase, HBMR_WAVE);
      if (gneed) {
        if (s < (unsigned long long)n) {
          const uint64_t* st = states + s * (W + 1);
          const uint32_t from = (uint32_t)(st[W] >> 32);
          if (from < (unsigned long long)nprefixes) {
            if (from != src) {
              if (cnt) atomicAdd(&counts[src], cnt);
              cnt = 0;
              src = from;
            }
            const int c = ec_start(t, full, st, l);
            if (gl == 0) cnt += c;
          }
        } else {
          done = true;
        }
      }
    }
    if (__all(done)) break;
    const bool active = l.d >= 0;
    const int r = l.i + gl;
    Mask<W> m;
    for (int k = 0; k < W; ++k) m.w[k] = 0;
    uint32_t p = 0;
    bool fit = false;
    if (active && r < l.e) {
      m = ec_row(t, r);
      p = t.p[r];
      fit = !ec_meets(m, l.occ) && !(p & l.used);
    }
    const unsigned long long fits = (__ballot(fit) >> gbase) & ((1ull << G) - 1);
    const int f = fits ? __builtin_ctzll(fits) : 0;
    for (int k = 0; k < W; ++k) m.w[k] = __shfl(m.w[k], gbase + f, HBMR_WAVE);
    p = __shfl(p, gbase + f, HBMR_WAVE);
    if (!active) continue;
    if (fits) {
      if (gl == 0) ++nodes;
      Mask<W> occ;
      for (int k = 0; k < W; ++k) occ.w[k] = l.occ.w[k] | m.w[k];
      if (ec_same(occ, full)) {
        if (gl == 0) ++cnt;
        l.i += f + 1;
      } else if (l.d >= kMaxPieces - 1) {
        l.i += f + 1;
      } else {
        l.occ = occ;
        l.used |= p;
        stack[l.d * stride] = (uint16_t)(l.i + f);  // every lane of the group: the same value
        ++l.d;
        const int c = ec_lowest_empty(occ);
        l.i = t.off[c];
        l.e = t.off[c + 1];
      }
    } else {
      l.i += G;
      if (l.i >= l.e && --l.d >= 0) {
        const int back = stack[l.d * stride];
        const Mask<W> bm = ec_row(t, back);
        for (int k = 0; k < W; ++k) l.occ.w[k] ^= bm.w[k];
        l.used ^= t.p[back];
        l.i = back + 1;
        l.e = t.off[ec_lowest_empty(l.occ) + 1];
      }
    }
  }

  const unsigned long long have = __ballot(cnt != 0);
  if (have) {
    const uint32_t s0 = __shfl(src, __builtin_ctzll(have), HBMR_WAVE);
    if (__all(cnt == 0 || src == s0)) {
      const unsigned long long total = wave_sum(cnt);
      if (lane == 0) atomicAdd(&counts[s0], total);
    } else if (cnt) {
      atomicAdd(&counts[src], cnt);
    }
  }
  const unsigned long long wn = wave_sum(nodes);
  if (lane == 0) {
    if (wn) atomicAdd(&scratch[1], wn);
    if (wg_clock) atomicMax(&wg_clock[2 * blockIdx.x + 1], (unsigned long long)wall_clock64());
  }
}

bool table_ok(int words, int nrows, int ncells) {
  return (words == 1 || words == 2) && ncells >= 1 && ncells <= 64 * words && nrows >= 0 &&
         nrows <= kMaxRows;
}

// Threads per workgroup and LDS bytes of the count kernel.  256 threads while
// four workgroups of them fit a CU's LDS, else 1024 so that the one workgroup a
// large table leaves room for still fills the CU's SIMDs.  0 threads: the table
// does not fit.
void count_shape(int words, int nrows, int ncells, int* threads, size_t* lds) {
  const size_t table = (size_t)nrows * (8 * words + 4) + 4 * (size_t)(ncells + 1);
  const size_t room = kLdsBytes - kLdsKeep;
  *threads = 256;
  *lds = table + (size_t)kMaxPieces * 2 * (256 / kGroup);
  if (*lds * 4 <= room) return;
  *threads = 1024;
  *lds = table + (size_t)kMaxPieces * 2 * (1024 / kGroup);
  if (*lds > room) *threads = 0;
}

int device_cus() {
  static int cus = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
      v = 256;
    return v;
  }();
  return cus;
}

int count_blocks(int threads, size_t lds, long n) {
  long per_cu = (long)((kLdsBytes - kLdsKeep) / lds);
  if (per_cu > 2048 / threads) per_cu = 2048 / threads;
  if (per_cu < 1) per_cu = 1;
  const long groups = threads / kGroup;
  long blocks = (n + groups - 1) / groups;
  if (blocks > per_cu * device_cus()) blocks = per_cu * device_cus();
  return (int)(blocks < 1 ? 1 : blocks);
}

template <int W>
int launch_count(const uint64_t* m, const uint32_t* p, const int32_t* off, int nrows, int ncells,
                 const uint64_t* states, long n, long nprefixes, unsigned long long* scratch,
                 unsigned long long* counts, unsigned long long* wg_clock, hipStream_t st) {
  int threads;
  size_t lds;
  count_shape(W, nrows, ncells, &threads, &lds);
  if (!threads) return (int)hipErrorInvalidValue;
  static bool lds_set = false;
  if (!lds_set) {
    HBMR_RETURN_IF_ERROR(hipFuncSetAttribute((const void*)exactcover_count_kernel<W>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             kLdsBytes - kLdsKeep));
    lds_set = true;
  }
  hipLaunchKernelGGL(exactcover_count_kernel<W>, dim3((unsigned)count_blocks(threads, lds, n)),
                     dim3((unsigned)threads), lds, st, m, p, off, nrows, ncells, states, n,
                     nprefixes, scratch, counts, wg_clock);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int hbmr_exactcover_expand_count(int words, const uint64_t* m, const uint32_t* p,
                                 const int32_t* off, int nrows, int ncells,
                                 const uint64_t* states, long n, int32_t* nchild, hipStream_t st) {
  if (!table_ok(words, nrows, ncells) || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long blocks = (n + kExpandThreads - 1) / kExpandThreads;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (words == 1)
    hipLaunchKernelGGL(exactcover_expand_count_kernel<1>, dim3((unsigned)blocks),
                       dim3(kExpandThreads), 0, st, Table<1>{m, p, off, nrows, ncells}, states, n,
                       nchild);
  else
    hipLaunchKernelGGL(exactcover_expand_count_kernel<2>, dim3((unsigned)blocks),
                       dim3(kExpandThreads), 0, st, Table<2>{m, p, off, nrows, ncells}, states, n,
                       nchild);
  return (int)hipGetLastError();
}

int hbmr_exactcover_expand_write(int words, const uint64_t* m, const uint32_t* p,
                                 const int32_t* off, int nrows, int ncells,
                                 const uint64_t* states, long n, const int64_t* child_off,
                                 long base, long capacity, uint64_t* out, hipStream_t st) {
  if (!table_ok(words, nrows, ncells) || n < 0 || capacity < 0) return (int)hipErrorInvalidValue;
  if (n == 0 || capacity == 0) return 0;
  const long blocks = (n + kExpandThreads - 1) / kExpandThreads;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (words == 1)
    hipLaunchKernelGGL(exactcover_expand_write_kernel<1>, dim3((unsigned)blocks),
                       dim3(kExpandThreads), 0, st, Table<1>{m, p, off, nrows, ncells}, states, n,
                       child_off, base, capacity, out);
  else
    hipLaunchKernelGGL(exactcover_expand_write_kernel<2>, dim3((unsigned)blocks),
                       dim3(kExpandThreads), 0, st, Table<2>{m, p, off, nrows, ncells}, states, n,
                       child_off, base, capacity, out);
  return (int)hipGetLastError();
}

// workgroups hbmr_exactcover_count launches for n states (wg_clock holds two
// words for each); 0 when the table does not fit the kernel
int hbmr_exactcover_count_blocks(int words, int nrows, int ncells, long n) {
  if (!table_ok(words, nrows, ncells) || n < 1) return 0;
  int threads;
  size_t lds;
  count_shape(words, nrows, ncells, &threads, &lds);
  return threads ? count_blocks(threads, lds, n) : 0;
}

int hbmr_exactcover_count(int words, const uint64_t* m, const uint32_t* p, const int32_t* off,
                          int nrows, int ncells, const uint64_t* states, long n, long nprefixes,
                          unsigned long long* scratch, unsigned long long* counts,
                          unsigned long long* wg_clock, hipStream_t st) {
  if (!table_ok(words, nrows, ncells) || n < 0 || nprefixes < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  return words == 1 ? launch_count<1>(m, p, off, nrows, ncells, states, n, nprefixes, scratch,
                                      counts, wg_clock, st)
                    : launch_count<2>(m, p, off, nrows, ncells, states, n, nprefixes, scratch,
                                      counts, wg_clock, st);
}

}  // extern "C"
