#pragma once
// K-Means combine and reduce stage: the int64 fixed-point combiners (LDS-
// privatised, sorted, grouped, delta), the centroid update, the cluster padding
// and the fp32 -> bf16 conversion kernels.
#include "../common.h"
#include "grouped.h"

namespace {

// ---------------------------------------------------------------------------
// Combiner: per-cluster sums and counts, LDS-privatised, in 64-bit FIXED POINT.
//
// gfx950 executes ds_add_f32 at ~0.4 lane-ops/clk/CU versus ~14.5 for
// ds_add_u32 (tools/ubench_lds_atomics.hip, profiles/lds_atomics.txt), so the
// partial sums are accumulated as int64 = round(x · 2^shift) with integer LDS
// atomics (ds_add_u64) and flushed with integer global atomics.  Integer sums
// are associative: the combiner output is bitwise identical for any task
// placement, kernel schedule or GPU count (and stays exact through the RCCL
// all-reduce).  bf16 inputs are exact in fixed point whenever |x| ≥ 2^(shift-31)
// ... i.e. every bf16 with ulp ≥ 2^-shift (shift = 24: |x| ≥ 2^-17).
//
// LDS image of the sums: element (row r, dim i) at r*RS + i + (i >> 3) (u64
// units).  A point is handled by D/8 lanes, lane `sub` owning dims
// [8 sub, 8 sub + 8) (one 16-B global load); at step j the 16 lanes of a point
// touch dwords 2(9 sub + j) + {0,1}: all 32 banks exactly once.
typedef unsigned long long u64;

template <int D> struct AccCfg {
  static constexpr int RS = D + D / 8 + 1;  // padded row stride (u64 elements)
  static constexpr int TPP = D / 8;         // lanes per point
};

// Eight consecutive features of one row, as loaded by one lane: bf16 rows
// (the normal path, one 16-B load) or fp32 rows (exact mode, two 16-B loads).
// `ld` is the padded row length in elements.
template <typename T> struct Row8;
template <> struct Row8<__bf16> {
  uint4 v;
  __device__ __forceinline__ void load(const __bf16* X, size_t row, int ld, int sub) {
    v = reinterpret_cast<const uint4*>(X + row * ld)[sub];
  }
  __device__ __forceinline__ void unpack(float f[8]) const { hbmr_unpack8(v, f); }
};
template <> struct Row8<float> {
  uint4 a, b;
  __device__ __forceinline__ void load(const float* X, size_t row, int ld, int sub) {
    const uint4* r = reinterpret_cast<const uint4*>(X + row * ld) + 2 * sub;
    a = r[0];
    b = r[1];
  }
  __device__ __forceinline__ void unpack(float f[8]) const {
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y);
    f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
    f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y);
    f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
  }
};

template <int D, typename T>
__device__ __forceinline__ void lds_add_row(u64* s_rows, int r, int sub, const Row8<T>& v,
                                            float scale) {
  float f[8];
  v.unpack(f);
  u64* dst = s_rows + r * AccCfg<D>::RS + sub * 9;
  long long q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hbmr_fx_accum8(f, scale, q);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (q[j]) atomicAdd(dst + j, (u64)q[j]);
}

template <int D>
__device__ __forceinline__ void flush_rows(const u64* s_rows, const uint32_t* s_cnt, int c0, int cc,
                                           long long* __restrict__ sums,
                                           long long* __restrict__ counts, int tid, int nt) {
  for (int e = tid; e < cc * D; e += nt) {
    const int r = e / D, i = e % D;
    const u64 v = s_rows[r * AccCfg<D>::RS + i + (i >> 3)];
    if (v) atomicAdd(reinterpret_cast<u64*>(sums) + (size_t)(c0 + r) * D + i, v);
  }
  for (int r = tid; r < cc; r += nt) {
    const uint32_t v = s_cnt[r];
    if (v) atomicAdd(reinterpret_cast<u64*>(counts) + c0 + r, (u64)v);
  }
}

// Small k: every workgroup holds all k rows in LDS; grid-stride over points.
// Each lane group keeps U rows (and labels) in flight before its LDS adds.
template <typename T, int D, int U>
__global__ __launch_bounds__(256) void kmeans_accum_lds_kernel(
    const T* __restrict__ X, long n, const int32_t* __restrict__ labels, int k,
    long long* __restrict__ sums, long long* __restrict__ counts, float scale) {
  using A = AccCfg<D>;
  extern __shared__ __attribute__((aligned(16))) u64 s_acc[];  // k*RS sums, then k counts
  const int tid = threadIdx.x;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_acc + k * A::RS);
  for (int i = tid; i < k * A::RS; i += 256) s_acc[i] = 0ull;
  for (int i = tid; i < k; i += 256) s_cnt[i] = 0u;
  __syncthreads();
  constexpr int PPI = 256 / A::TPP;  // point slots per workgroup
  const int sub = tid % A::TPP;
  const int pi = tid / A::TPP;
  const long stride = (long)gridDim.x * PPI;
  long p = (long)blockIdx.x * PPI + pi;
  for (; p + (U - 1) * stride < n; p += U * stride) {
    int lab[U];
    Row8<T> v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      lab[u] = labels[p + u * stride];
      v[u].load(X, p + u * stride, D, sub);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      lds_add_row<D>(s_acc, lab[u], sub, v[u], scale);
      if (sub == 0) atomicAdd(s_cnt + lab[u], 1u);
    }
  }
  for (; p < n; p += stride) {
    const int l0 = labels[p];
    Row8<T> v0;
    v0.load(X, p, D, sub);
    lds_add_row<D>(s_acc, l0, sub, v0, scale);
    if (sub == 0) atomicAdd(s_cnt + l0, 1u);
  }
  __syncthreads();
  flush_rows<D>(s_acc, s_cnt, 0, k, sums, counts, tid, 256);
}

// Large k: grid.y walks cluster chunks of CC clusters.  Each wave scans 256
// labels per step (one int4 per lane), compacts the points whose label falls in
// this workgroup's chunk into a wave-private LDS queue (ballot + prefix count),
// then drains the queue with U rows in flight per lane group.  Every row is
// gathered exactly once over the whole grid; labels are re-read per chunk
// (from L2 / Infinity Cache when the split is small, as map splits are).
constexpr int kAccWaves = 8;
constexpr int kQueue = 256;  // queue entries per wave (one step's worth)

template <typename T, int D, int U>
__global__ __launch_bounds__(512) void kmeans_accum_chunked_kernel(
    const T* __restrict__ X, long n, const int32_t* __restrict__ labels, int k, int CC,
    long pts_per_block, long long* __restrict__ sums, long long* __restrict__ counts,
    float scale) {
  using A = AccCfg<D>;
  extern __shared__ __attribute__((aligned(16))) u64 s_acc[];
  // layout: CC*RS u64 sums | kAccWaves*kQueue u32 queue | CC u32 counts
  constexpr int NT = kAccWaves * HBMR_WAVE;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * CC;
  const int cc = min(CC, k - c0);
  for (int i = tid; i < CC * A::RS; i += NT) s_acc[i] = 0ull;
  uint32_t* s_q = reinterpret_cast<uint32_t*>(s_acc + CC * A::RS);
  uint32_t* s_cnt = s_q + kAccWaves * kQueue;
  for (int i = tid; i < CC; i += NT) s_cnt[i] = 0u;
  __syncthreads();
  const int wave = tid / HBMR_WAVE, lane = tid & 63;
  uint32_t* q = s_q + wave * kQueue;
  constexpr int GPW = HBMR_WAVE / A::TPP;  // points per wave-instruction
  const int grp = lane / A::TPP, sub = lane % A::TPP;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const long pb = (long)blockIdx.x * pts_per_block;
  const long pe = min(n, pb + pts_per_block);
  for (long base = pb + (long)wave * kQueue; base < pe; base += (long)kAccWaves * kQueue) {
    int lab[4];
    const long p4 = base + 4 * lane;
    if (p4 + 3 < pe) {
      const int4 l4 = *reinterpret_cast<const int4*>(labels + p4);
      lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) lab[t] = (p4 + t < pe) ? labels[p4 + t] : -1;
    }
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int rel = lab[t] - c0;
      const bool mine = (unsigned)rel < (unsigned)cc;
      const unsigned long long m = __ballot(mine);
      if (mine) q[cnt + __popcll(m & lt_mask)] = ((uint32_t)(4 * lane + t) << 16) | (uint32_t)rel;
      cnt += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int e = 0; e < cnt; e += U * GPW) {
      Row8<T> v[U];
      uint32_t ent[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = e + u * GPW + grp;
        ent[u] = idx < cnt ? q[idx] : 0xffffffffu;
        if (ent[u] != 0xffffffffu) v[u].load(X, base + (ent[u] >> 16), D, sub);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ent[u] != 0xffffffffu) {
          const int r = (int)(ent[u] & 0xffffu);
          lds_add_row<D>(s_acc, r, sub, v[u], scale);
          if (sub == 0) atomicAdd(s_cnt + r, 1u);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  flush_rows<D>(s_acc, s_cnt, c0, cc, sums, counts, tid, NT);
}

// ---------------------------------------------------------------------------
// Sorted (counting-sort) combiner for large k: no LDS float/int atomics in
// the hot loop at all.
//   1. kmeans_hist      : hist[label]++            (LDS u32 atomics, 1/point)
//   2. kmeans_scan      : offsets = exclusive_scan(hist); cursor = offsets;
//                         counts += hist
//   3. kmeans_scatter   : perm[offsets[l] + rank] = i, rank from a per-block
//                         LDS histogram (ds_add_rtn_u32) + one global atomic
//                         per (block, present label)
//   4. kmeans_segsum    : walk perm in order; each 16-lane group accumulates
//                         whole rows of one cluster in int64 registers and
//                         flushes once per cluster run (global u64 atomics).
// The gather in (4) re-reads each row once; run right after the assign kernel
// on a split of ≤ ~128 MB the rows come from the 256 MiB Infinity Cache.
constexpr int kScatterPts = 4096;  // points per scatter workgroup (16 per thread)

__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels,
                                                          long n, int k,
                                                          uint32_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];
  for (int i = threadIdx.x; i < k; i += 256) s_h[i] = 0u;
  __syncthreads();
  const long n4 = n / 4;
  const int4* l4 = reinterpret_cast<const int4*>(labels);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int4 v = l4[i];
    atomicAdd(s_h + v.x, 1u);
    atomicAdd(s_h + v.y, 1u);
    atomicAdd(s_h + v.z, 1u);
    atomicAdd(s_h + v.w, 1u);
  }
  if (blockIdx.x == 0)
    for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) atomicAdd(s_h + labels[i], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 256)
    if (s_h[i]) atomicAdd(hist + i, s_h[i]);
}

// single workgroup: exclusive scan of hist (k ≤ 1024*64), counts += hist
__global__ __launch_bounds__(1024) void kmeans_scan_kernel(const uint32_t* __restrict__ hist,
                                                           int k, uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ cursor,
                                                           long long* __restrict__ counts) {
  __shared__ uint32_t s_part[1024];
  const int t = threadIdx.x;
  const int per = (k + 1023) / 1024;
  const int lo = min(k, t * per), hi = min(k, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  s_part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = t >= off ? s_part[t - off] : 0u;
    __syncthreads();
    s_part[t] += v;
    __syncthreads();
  }
  uint32_t run = s_part[t] - s;  // exclusive prefix of this thread's range
  for (int i = lo; i < hi; ++i) {
    const uint32_t h = hist[i];
    offsets[i] = run;
    cursor[i] = run;
    if (counts) counts[i] += h;
    run += h;
  }
  if (t == 1023) offsets[k] = s_part[1023];
}

__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const int32_t* __restrict__ labels,
                                                             long n, int k,
                                                             uint32_t* __restrict__ cursor,
                                                             uint32_t* __restrict__ perm) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];  // k counters, then k bases
  uint32_t* s_base = s_h + k;
  const int t = threadIdx.x;
  for (int i = t; i < k; i += 256) s_h[i] = 0u;
  __syncthreads();
  constexpr int PER = kScatterPts / 256;
  const long p0 = (long)blockIdx.x * kScatterPts + (long)t * PER;
  int lab[PER];
  uint32_t rank[PER];
#pragma unroll
  for (int j = 0; j < PER; j += 4) {
    if (p0 + j + 3 < n) {
      const int4 v = *reinterpret_cast<const int4*>(labels + p0 + j);
      lab[j] = v.x; lab[j + 1] = v.y; lab[j + 2] = v.z; lab[j + 3] = v.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) lab[j + q] = (p0 + j + q < n) ? labels[p0 + j + q] : -1;
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) rank[j] = lab[j] >= 0 ? atomicAdd(s_h + lab[j], 1u) : 0u;
  __syncthreads();
  for (int i = t; i < k; i += 256) {
    const uint32_t c = s_h[i];
    s_base[i] = c ? atomicAdd(cursor + i, c) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (lab[j] >= 0) perm[s_base[lab[j]] + rank[j]] = (uint32_t)(p0 + j);
}

// Segmented row sum of the rows perm[s0:e) (sorted by cluster; cluster c owns
// perm[offsets[c]:offsets[c+1])) into out[c] (int64 fixed point).  The wave
// walks its range one cluster segment at a time: the GPW row groups split a
// segment's rows, U rows per group in flight (index load → row gather), and
// at the segment end the groups are reduced with xor-shuffles so each cluster
// costs one 128-value atomic flush per wave — spread over all groups — rather
// than one per group.  Segment bounds are wave-uniform (scalar loads).
// Row indirection of a segsum entry: the plain combiner's perm holds row
// indices; the delta combiner's holds (mover << 1 | sign) — see kmeans_delta_*.
struct IdentityRows {
  __device__ __forceinline__ uint32_t row(uint32_t i) const { return i; }
  __device__ __forceinline__ bool neg(uint32_t) const { return false; }
};

template <typename T, int D, int U, class Rows = IdentityRows>
__device__ __forceinline__ void segsum_range(const T* __restrict__ X,
                                             const uint32_t* __restrict__ pm,
                                             const uint32_t* __restrict__ of, int k, long s0,
                                             long e, u64* __restrict__ out, float scale,
                                             Rows rows = Rows()) {
  constexpr int TPP = D / 8;            // lanes per row
  constexpr int GPW = HBMR_WAVE / TPP;  // row groups per wave
  const int lane = threadIdx.x & 63;
  const int grp = lane / TPP, sub = lane % TPP;
  // first cluster whose segment contains s0: upper_bound(of, s0) - 1
  int lo = 0, hi = k;  // invariant of[lo] <= s0 < of[hi] (of[k] = n)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long)of[mid] <= s0) lo = mid; else hi = mid;
  }
  int cur = __builtin_amdgcn_readfirstlane(lo);
  long p = s0;
  while (p < e) {
    const long segE = min(e, (long)(uint32_t)__builtin_amdgcn_readfirstlane(of[cur + 1]));
    if (segE > p) {
      long long acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0;
      for (long base = p + grp; base < segE; base += (long)U * GPW) {
        uint32_t idx[U];
        Row8<T> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long q = base + (long)u * GPW;
          idx[u] = q < segE ? pm[q] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long q = base + (long)u * GPW;
          if (q < segE) v[u].load(X, rows.row(idx[u]), D, sub);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long q = base + (long)u * GPW;
          if (q < segE) {
            float f[8];
            v[u].unpack(f);
            if (rows.neg(idx[u])) {
              // round-half-even fixed point is odd-symmetric: fx(-x) = -fx(x)
#pragma unroll
              for (int j = 0; j < 8; ++j) f[j] = -f[j];
            }
            hbmr_fx_accum8(f, scale, acc);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int off = TPP; off < HBMR_WAVE; off <<= 1) acc[j] += __shfl_xor(acc[j], off);
      }
      u64* dst = out + (size_t)cur * D + sub * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j % GPW == grp % 8 && acc[j]) atomicAdd(dst + j, (u64)acc[j]);
      p = segE;
    }
    ++cur;
  }
}

template <typename T, int D, int U>
__global__ __launch_bounds__(256) void kmeans_segsum_kernel(
    const T* __restrict__ X, long n, const uint32_t* __restrict__ perm,
    const uint32_t* __restrict__ offsets, int k, long chunk, long long* __restrict__ sums,
    float scale) {
  const long wid = (long)blockIdx.x * (blockDim.x / HBMR_WAVE) + threadIdx.x / HBMR_WAVE;
  const long s = wid * chunk;
  if (s >= n) return;
  segsum_range<T, D, U>(X, perm, offsets, k, s, min(n, s + chunk), reinterpret_cast<u64*>(sums),
                        scale);
}

// ---- grouped sorted combiner ------------------------------------------------------
// hist[s][k] comes from kmeans_hist_grouped_kernel.  Every scatter workgroup
// rebuilds the exclusive scan of its split's histogram in LDS (k ≤ 8192: a few
// µs) so no separate scan launch or grid-wide sync is needed; the workgroup
// with local index 0 of each split also publishes offsets[s] (for the segsum
// launch) and adds the histogram to that task's counts.
__device__ void block_exclusive_scan(const uint32_t* __restrict__ in, int k, uint32_t* out,
                                     uint32_t* total) {
  __shared__ uint32_t s_part[256];
  const int t = threadIdx.x;
  const int per = (k + 255) / 256;
  const int lo = min(k, t * per), hi = min(k, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += in[i];
  // wave-level inclusive scan, then across the 4 waves
  const int lane = t & 63, w = t >> 6;
  uint32_t v = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_part[w] = v;
  __syncthreads();
  uint32_t wbase = 0;
  for (int i = 0; i < w; ++i) wbase += s_part[i];
  uint32_t run = wbase + v - s;
  for (int i = lo; i < hi; ++i) {
    out[i] = run;
    run += in[i];
  }
  if (t == 255) *total = wbase + v;
  __syncthreads();
}

// Per-split label histogram from the labels array: LDS bins, one flush per block.
constexpr long kHistPts = 16384;
__global__ __launch_bounds__(256) void kmeans_hist_grouped_kernel(const SplitTable tbl,
                                                                  const int32_t* __restrict__ labels,
                                                                  uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t s_bins[];
  const int k = tbl.k;
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, blockIdx.x));
  const long local = blockIdx.x - tbl.blk[s];
  const long n = tbl.n[s];
  for (int i = threadIdx.x; i < k; i += 256) s_bins[i] = 0u;
  __syncthreads();
  const int32_t* lab = labels + tbl.off[s];
  const long p1 = min(n, (local + 1) * kHistPts);
  for (long p = local * kHistPts + threadIdx.x; p < p1; p += 256) atomicAdd(s_bins + lab[p], 1u);
  __syncthreads();
  uint32_t* hs = hist + (size_t)s * k;
  for (int i = threadIdx.x; i < k; i += 256)
    if (s_bins[i]) atomicAdd(hs + i, s_bins[i]);
}

__global__ __launch_bounds__(256) void kmeans_scatter_grouped_kernel(
    const SplitTable tbl, const int32_t* __restrict__ labels, const uint32_t* __restrict__ hist,
    uint32_t* __restrict__ cursor, uint32_t* __restrict__ offsets, uint32_t* __restrict__ perm,
    long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];  // off[k] | cnt[k] | base[k]
  const int k = tbl.k;
  uint32_t* s_off = s_h;
  uint32_t* s_cnt = s_h + k;
  uint32_t* s_base = s_h + 2 * k;
  __shared__ uint32_t s_total;
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, blockIdx.x));
  const long local = blockIdx.x - tbl.blk[s];
  const long n = tbl.n[s];
  const uint32_t* hs = hist + (size_t)s * k;
  const int t = threadIdx.x;
  for (int i = t; i < k; i += 256) s_cnt[i] = 0u;
  block_exclusive_scan(hs, k, s_off, &s_total);
  if (local == 0) {
    uint32_t* os = offsets + (size_t)s * (k + 1);
    for (int i = t; i < k; i += 256) {
      os[i] = s_off[i];
      counts[(size_t)s * k + i] += hs[i];
    }
    if (t == 0) os[k] = s_total;
  }
  constexpr int PER = kScatterPts / 256;
  const int32_t* lab_s = labels + tbl.off[s];
  const long p0 = local * kScatterPts + (long)t * PER;
  int lab[PER];
  uint32_t rank[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) lab[j] = (p0 + j < n) ? lab_s[p0 + j] : -1;
#pragma unroll
  for (int j = 0; j < PER; ++j) rank[j] = lab[j] >= 0 ? atomicAdd(s_cnt + lab[j], 1u) : 0u;
  __syncthreads();
  uint32_t* cur_s = cursor + (size_t)s * k;
  for (int i = t; i < k; i += 256) {
    const uint32_t c = s_cnt[i];
    s_base[i] = c ? s_off[i] + atomicAdd(cur_s + i, c) : 0u;
  }
  __syncthreads();
  uint32_t* perm_s = perm + tbl.off[s];
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (lab[j] >= 0) perm_s[s_base[lab[j]] + rank[j]] = (uint32_t)(p0 + j);
}

template <int D, int U>
__global__ __launch_bounds__(256) void kmeans_segsum_grouped_kernel(
    const SplitTable tbl, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ offsets,
    long chunk, long long* __restrict__ sums, float scale) {
  const int k = tbl.k;
  const long wid = (long)blockIdx.x * (blockDim.x / HBMR_WAVE) + threadIdx.x / HBMR_WAVE;
  // tbl.blk holds the prefix sum of WAVES (chunks) per split for this launch
  if (wid >= tbl.blk[tbl.nsplit]) return;
  const int sidx = __builtin_amdgcn_readfirstlane(find_split(tbl, wid));
  const long n = tbl.n[sidx];
  const long s0 = (wid - tbl.blk[sidx]) * chunk;
  segsum_range<__bf16, D, U>(tbl.X[sidx], perm + tbl.off[sidx], offsets + (size_t)sidx * (k + 1), k, s0,
                     min(n, s0 + chunk), reinterpret_cast<u64*>(sums) + (size_t)sidx * k * D,
                     scale);
}

// ---- delta combiner --------------------------------------------------------------
// The combiner output of a split is a function of its points and their labels
// only.  Given a reference partition g of the split (labels of an earlier
// pass) with its exact int64 sums S0[c] = Σ_{g(p)=c} fx(x_p) and counts N0,
// the sums for the new labels l are
//     S[c] = S0[c] + Σ_{l(p)=c, g(p)≠c} fx(x_p) - Σ_{g(p)=c, l(p)≠c} fx(x_p)
// (integer arithmetic: bit-identical to the direct combiner for ANY g).  Only
// the points whose label changed ("movers") are gathered, so once K-Means
// settles the combiner no longer re-reads the split: it is a pass over the
// labels plus a few thousand rows.  Afterwards (S0, N0, g) := (S, N, l), which
// the diff kernel does for g in place.
//
//   kmeans_slab_copy      : sums[t] = S0[t], counts[t] = N0[t]
//   kmeans_delta_diff     : movers (p, new << 16 | old), hist[c] = #entries,
//                           counts[t] += in - out, g[p] = l
//   kmeans_delta_scatter  : entries e = (mover << 1 | sign) sorted by cluster
//                           (+new for sign 0, -old for sign 1)
//   kmeans_delta_segsum   : segmented signed row sums of the entries into sums[t]
struct SlabTable {
  const long long* s[kMaxGroup];
  const long long* c[kMaxGroup];
};
struct GTable {
  int32_t* g[kMaxGroup];
};

__global__ __launch_bounds__(256) void kmeans_slab_copy_kernel(const SlabTable src, long slab,
                                                               int k, long long* __restrict__ sums,
                                                               long long* __restrict__ counts) {
  const int t = blockIdx.y;
  const long long* s = src.s[t];
  long long* d = sums + (size_t)t * slab;
  // slab = k * dp int64 (dp ≥ 64): whole 16-byte pieces
  const long npc = slab / 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npc; i += (long)gridDim.x * 256)
    reinterpret_cast<int4*>(d)[i] = reinterpret_cast<const int4*>(s)[i];
  if (blockIdx.x == 0) {
    const long long* c = src.c[t];
    for (int i = threadIdx.x; i < k; i += 256) counts[(size_t)t * k + i] = c[i];
  }
}

constexpr long kDiffPts = 8192;  // points per diff workgroup
constexpr int kDiffPer = (int)(kDiffPts / 256);  // points per thread

// Every thread loads its 32 (label, reference label) pairs up front (strided
// by the workgroup width, so each load instruction is coalesced) — the loads
// are in flight together instead of one dependent round trip per 64 points —
// then the workgroup reserves room for all of its movers with ONE atomic on
// the split's mover count (a prefix sum over the threads' mover counts places
// each thread's movers).  Mover order is irrelevant downstream: the scatter
// sorts entries by cluster and the row sums are integer.
__global__ __launch_bounds__(256) void kmeans_delta_diff_kernel(
    const SplitTable tbl, const GTable gt, const int32_t* __restrict__ labels,
    uint2* __restrict__ movers, uint32_t* __restrict__ mcount, uint32_t* __restrict__ hist,
    long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_bins[];  // in[k] | out[k]
  __shared__ uint32_t s_wsum[4];
  __shared__ uint32_t s_first;
  const int k = tbl.k;
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, blockIdx.x));
  const long local = blockIdx.x - tbl.blk[s];
  const long n = tbl.n[s];
  const int t = threadIdx.x;
  for (int i = t; i < 2 * k; i += 256) s_bins[i] = 0u;
  const int32_t* lab = labels + tbl.off[s];
  int32_t* g = gt.g[s];
  uint2* mv = movers + tbl.off[s];
  const int lane = t & 63, wave = t >> 6;
  const long p0 = local * kDiffPts + t;
  const long p1 = min(n, (local + 1) * kDiffPts);
  int32_t l[kDiffPer], o[kDiffPer];
  // branch-free: every load is issued (index clamped into the workgroup's
  // range, which holds at least one point) and out-of-range pairs zeroed by a
  // select, so all 64 loads of a thread are in flight together
#pragma unroll
  for (int j = 0; j < kDiffPer; ++j) {
    const long p = p0 + (long)j * 256;
    const bool in = p < p1;
    const long pc = in ? p : p1 - 1;
    const int32_t a = lab[pc], b = g[pc];
    l[j] = in ? a : 0;
    o[j] = in ? b : 0;
  }
  // (a label outside [0, k) would index past the bins and the slabs: such a
  // point is never a mover — the bit-exactness tests catch it)
  uint32_t chm = 0u;
  uint32_t pk[kDiffPer];  // new << 16 | old (k <= 8192)
#pragma unroll
  for (int j = 0; j < kDiffPer; ++j) {
    const bool ch = l[j] != o[j] && (unsigned)l[j] < (unsigned)k && (unsigned)o[j] < (unsigned)k;
    chm |= (uint32_t)ch << j;
    pk[j] = ((uint32_t)l[j] << 16) | ((uint32_t)o[j] & 0xffffu);
  }
  const uint32_t cnt = (uint32_t)__popc(chm);
  uint32_t x = cnt;  // inclusive prefix over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_wsum[wave] = x;
  __syncthreads();
  if (t == 0) {
    const uint32_t tot = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    s_first = tot ? atomicAdd(mcount + s, tot) : 0u;
  }
  __syncthreads();
  if (chm) {
    uint32_t i = s_first + x - cnt;
    for (int w = 0; w < wave; ++w) i += s_wsum[w];
#pragma unroll
    for (int j = 0; j < kDiffPer; ++j) {
      if ((chm >> j) & 1u) {
        const uint32_t p = (uint32_t)(p0 + (long)j * 256);
        const uint32_t nl = pk[j] >> 16, ol = pk[j] & 0xffffu;
        mv[i++] = make_uint2(p, pk[j]);
        g[p] = (int32_t)nl;
        atomicAdd(s_bins + nl, 1u);
        atomicAdd(s_bins + k + ol, 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* hs = hist + (size_t)s * k;
  u64* cs = reinterpret_cast<u64*>(counts) + (size_t)s * k;
  for (int c = t; c < k; c += 256) {
    const uint32_t in = s_bins[c], out = s_bins[k + c];
    if (in | out) {
      atomicAdd(hs + c, in + out);
      if (in != out) atomicAdd(cs + c, (u64)((long long)in - (long long)out));
    }
  }
}

// tbl.blk: prefix of scatter workgroups per split sized for the worst case
// (every point moved: 2n entries); surplus workgroups leave after the scan.
__global__ __launch_bounds__(256) void kmeans_delta_scatter_kernel(
    const SplitTable tbl, const uint2* __restrict__ movers, const uint32_t* __restrict__ mcount,
    const uint32_t* __restrict__ hist, uint32_t* __restrict__ cursor,
    uint32_t* __restrict__ offsets, uint32_t* __restrict__ perm) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_h[];  // off[k] | cnt[k] | base[k]
  const int k = tbl.k;
  __shared__ uint32_t s_total;
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, blockIdx.x));
  const long local = blockIdx.x - tbl.blk[s];
  const long ne = 2L * (long)__builtin_amdgcn_readfirstlane(mcount[s]);
  if (local > 0 && local * kScatterPts >= ne) return;   // uniform: nothing for this block
  uint32_t* s_off = s_h;
  uint32_t* s_cnt = s_h + k;
  uint32_t* s_base = s_h + 2 * k;
  const int t = threadIdx.x;
  for (int i = t; i < k; i += 256) s_cnt[i] = 0u;
  block_exclusive_scan(hist + (size_t)s * k, k, s_off, &s_total);
  if (local == 0) {
    uint32_t* os = offsets + (size_t)s * (k + 1);
    for (int i = t; i < k; i += 256) os[i] = s_off[i];
    if (t == 0) os[k] = s_total;
  }
  constexpr int PER = kScatterPts / 256;
  const uint2* mv = movers + tbl.off[s];
  const long e0 = local * kScatterPts + (long)t * PER;
  int cl[PER];
  uint32_t rank[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const long e = e0 + j;
    cl[j] = -1;
    if (e < ne) {
      const uint32_t y = mv[e >> 1].y;
      cl[j] = (e & 1) ? (int)(y & 0xffffu) : (int)(y >> 16);
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) rank[j] = cl[j] >= 0 ? atomicAdd(s_cnt + cl[j], 1u) : 0u;
  __syncthreads();
  uint32_t* cur_s = cursor + (size_t)s * k;
  for (int i = t; i < k; i += 256) {
    const uint32_t c = s_cnt[i];
    s_base[i] = c ? s_off[i] + atomicAdd(cur_s + i, c) : 0u;
  }
  __syncthreads();
  uint32_t* perm_s = perm + 2 * tbl.off[s];
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (cl[j] >= 0) perm_s[s_base[cl[j]] + rank[j]] = (uint32_t)(e0 + j);
}

struct MoverRows {
  const uint2* mv;
  __device__ __forceinline__ uint32_t row(uint32_t e) const { return mv[e >> 1].x; }
  __device__ __forceinline__ bool neg(uint32_t e) const { return (e & 1u) != 0u; }
};

// Persistent grid: wave items (split, chunk of `chunk` entries) in split order,
// counted from the device-side mover counts.
template <typename T, int D, int U>
__global__ __launch_bounds__(256) void kmeans_delta_segsum_kernel(
    const SplitTable tbl, const uint2* __restrict__ movers, const uint32_t* __restrict__ mcount,
    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ offsets, long chunk,
    long long* __restrict__ sums, float scale) {
  const int k = tbl.k;
  const long nw = (long)gridDim.x * (blockDim.x / HBMR_WAVE);
  long wid = (long)blockIdx.x * (blockDim.x / HBMR_WAVE) + threadIdx.x / HBMR_WAVE;
  int s = 0;
  long sbase = 0;
  long items = (2L * (long)__builtin_amdgcn_readfirstlane(mcount[0]) + chunk - 1) / chunk;
  for (; ; wid += nw) {
    while (wid >= sbase + items) {
      sbase += items;
      if (++s >= tbl.nsplit) return;
      items = (2L * (long)__builtin_amdgcn_readfirstlane(mcount[s]) + chunk - 1) / chunk;
    }
    const long ne = 2L * (long)__builtin_amdgcn_readfirstlane(mcount[s]);
    const long e0 = (wid - sbase) * chunk;
    segsum_range<T, D, U, MoverRows>(
        reinterpret_cast<const T*>(tbl.X[s]), perm + 2 * tbl.off[s],
        offsets + (size_t)s * (k + 1), k, e0, min(ne, e0 + chunk),
        reinterpret_cast<u64*>(sums) + (size_t)s * k * D, scale, MoverRows{movers + tbl.off[s]});
  }
}

// Reduce side + next-iteration prep.  One workgroup per cluster.
// sums are fixed-point int64 [k, dp], counts int64 [k].
__global__ __launch_bounds__(128) void kmeans_update_kernel(
    const long long* __restrict__ sums, const long long* __restrict__ counts, int k, int d,
    int dp, float inv_scale, float* __restrict__ cen, __bf16* __restrict__ cbf,
    float* __restrict__ chalf, float* __restrict__ shift2) {
  const int j = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ float red[2][128];
  const long long cnt = counts ? counts[j] : 0;
  const double inv = cnt > 0 ? (double)inv_scale / (double)cnt : 0.0;
  float nrm = 0.f, dsq = 0.f;
  uint16_t* cb = reinterpret_cast<uint16_t*>(cbf) + (size_t)j * dp;
  for (int i = tid; i < dp; i += 128) {
    float v = 0.f;
    if (i < d) {
      const float old = cen[(size_t)j * d + i];
      v = cnt > 0 ? (float)((double)sums[(size_t)j * dp + i] * inv) : old;
      dsq += (v - old) * (v - old);
      cen[(size_t)j * d + i] = v;
    }
    const uint16_t b = hbmr_f32_to_bf16(v);
    cb[i] = b;
    const float vb = hbmr_bf16_to_f32(b);
    nrm += vb * vb;
  }
  red[0][tid] = nrm;
  red[1][tid] = dsq;
  __syncthreads();
  for (int s = 64; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    chalf[j] = -0.5f * red[0][0];
    if (shift2) shift2[j] = red[1][0];
  }
}

__global__ __launch_bounds__(256) void f32_to_bf16_pad_kernel(const float* __restrict__ src,
                                                              long n, int d, int dp,
                                                              uint16_t* __restrict__ dst) {
  const long total = n * dp;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / dp;
    const int c = (int)(e - r * dp);
    dst[e] = c < d ? hbmr_f32_to_bf16(src[r * d + c]) : (uint16_t)0;
  }
}

__global__ void kmeans_pad_clusters_kernel(__bf16* cbf, float* chalf, int k, int k_pad, int dp) {
  const int j = k + blockIdx.x;
  if (j >= k_pad) return;
  uint16_t* cb = reinterpret_cast<uint16_t*>(cbf) + (size_t)j * dp;
  for (int i = threadIdx.x; i < dp; i += blockDim.x) cb[i] = 0;
  if (threadIdx.x == 0) chalf[j] = -1.0e30f;
}

}  // namespace
