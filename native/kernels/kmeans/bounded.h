#pragma once
// Exact K-Means, bounded pass: centroid shifts, the sweep over the stored
// per-point bounds and the v3 fused assign over the rows the sweep lists.
#include "../common.h"
#include "fused.h"

namespace {

// ---------------------------------------------------------------------------
// The bounded pass (hbmr_kmeans_assign_top3_q1_bounded).  A split's reference
// partition keeps, beside its labels g, a certified lower bound gap[p] of
// min_{j != g(p)} |x_p - c_j| - |x_p - c_g(p)| (distances over the fp32 data)
// against the centroids `ref`.  For centroids c' the triangle inequality gives
//   |x - c'_g| <= |x - ref_g| + shift[g],  |x - c'_j| >= |x - ref_j| - shift[j],
// shift[j] = |c'_j - ref_j|, so the bound against c' is at least
// gap - shift[g] - max_j shift[j]; where that stays > 0 the exact arg-min is
// still g (uniquely) and the point needs no distance at all (Hamerly's test).
//   shift : shift[j] per distinct ref of the batch, fp64, rounded up;
//   sweep : decays every gap, keeps the label of a point whose bound holds and
//           lists the other rows per split (device-side counts);
//   assign: the v3 fused assign over the lists (row indirection), whose
//           epilogue leaves a fresh gap for the points it certifies.
constexpr int kSweepPer = 8;                         // points per thread in the sweep
constexpr int kBoundHdr = 512;                       // list counts | max shifts (u32 / f32 [64])

struct ShiftTable {
  const float* ref[kMaxGroup];
};

// shift[r][j] = |cen_j - ref[r]_j| (>=), smax[r] = max_j (as bits: floats >= 0)
__global__ __launch_bounds__(64) void kmeans_bound_shift_kernel(
    const ShiftTable tbl, const float* __restrict__ cen, int k, int d, float* __restrict__ shift,
    uint32_t* __restrict__ smax) {
  const int j = blockIdx.x, r = blockIdx.y;
  const float* a = cen + (size_t)j * d;
  const float* b = tbl.ref[r] + (size_t)j * d;
  double acc = 0.0;
  for (int i = threadIdx.x; i < d; i += 64) {
    const double e = (double)a[i] - (double)b[i];
    acc = fma(e, e, acc);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
  if (threadIdx.x == 0) {
    const float s = __double2float_ru(sqrt(acc) * (1.0 + 0x1p-40));
    shift[(size_t)r * k + j] = s;
    atomicMax(smax + r, __float_as_uint(s));
  }
}

// a - b rounded toward -inf where that is positive (else some value <= 0), for
// b >= 0: the rounding error of the fp32 difference is itself an fp32 number
// (Knuth's two-sum); results too small for it to be one count as 0
__device__ __forceinline__ float sub_rd_pos(float a, float b) {
  const float t = a - b;
  if (!(t > 0x1p-100f)) return 0.f;
  const float bb = t - a;
  const float err = (a - (t - bb)) - (b + bb);
  return err < 0.f ? __uint_as_float(__float_as_uint(t) - 1u) : t;
}

struct SweepTable {
  int nsplit;
  const int32_t* g[kMaxGroup];     // the reference partition's labels
  float* gap[kMaxGroup];           // its bounds (null: none yet, every row is listed)
  int rid[kMaxGroup];              // which shift row the gaps refer to
  long n[kMaxGroup];
  long off[kMaxGroup];
  long blk[kMaxGroup + 1];
};

__global__ __launch_bounds__(256) void kmeans_bound_sweep_kernel(
    const SweepTable tbl, int k, const float* __restrict__ shift,
    const float* __restrict__ smax, int32_t* __restrict__ labels, uint32_t* __restrict__ cnt,
    uint32_t* __restrict__ idx) {
  const long b = blockIdx.x;
  int lo = 0, hi = tbl.nsplit;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl.blk[mid] <= b) lo = mid; else hi = mid;
  }
  const int s = __builtin_amdgcn_readfirstlane(lo);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = tbl.n[s], o = tbl.off[s];
  const int32_t* __restrict__ g = tbl.g[s];
  float* __restrict__ gap = tbl.gap[s];
  const float* __restrict__ sh = shift + (size_t)tbl.rid[s] * k;
  const float sm = gap ? smax[tbl.rid[s]] : 0.f;
  const long p0 = (b - tbl.blk[s]) * (256 * kSweepPer);
  __shared__ uint32_t wcnt[4][kSweepPer];
  __shared__ uint32_t base_s;
  bool list[kSweepPer];
  uint32_t rank[kSweepPer];
#pragma unroll
  for (int i = 0; i < kSweepPer; ++i) {
    const long p = p0 + i * 256 + tid;
    list[i] = false;
    if (p < n) {
      list[i] = true;
      if (gap) {
        const int32_t c = g[p];
        // rounded toward -inf: the stored bound never exceeds the true one
        const float v =
            (uint32_t)c < (uint32_t)k ? sub_rd_pos(sub_rd_pos(gap[p], sh[c]), sm) : 0.f;
        if (v > 0.f) {
          list[i] = false;
          labels[o + p] = c;
          gap[p] = v;
        }
      }
    }
    const unsigned long long m = __ballot(list[i]);
    rank[i] = lane_rank(m);
    if (lane == 0) wcnt[wave][i] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int i = 0; i < kSweepPer; ++i) {
        const uint32_t c = wcnt[w][i];
        wcnt[w][i] = tot;
        tot += c;
      }
    base_s = tot ? atomicAdd(cnt + s, tot) : 0u;
  }
  __syncthreads();
  uint32_t* out = idx + o + base_s;
#pragma unroll
  for (int i = 0; i < kSweepPer; ++i)
    if (list[i]) out[wcnt[wave][i] + rank[i]] = (uint32_t)(p0 + i * 256 + tid);
}

struct GapTable {
  float* gap[kMaxGroup];
};

// The v3 fused assign over each split's list: the grid is the full batch's
// (the list lengths live on the device); a workgroup past its split's list
// leaves before it stages anything.
template <int D, bool F16>
__global__ __launch_bounds__(256, kExactMinB) void kmeans_assign_top3_q1_bounded_kernel(
    const TopQ1Table tbl, const GapTable gt, const __bf16* __restrict__ Ct,
    const float* __restrict__ chalf, int ntiles, int32_t* __restrict__ labels, FusedQ1Fin fin,
    const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ idx,
    unsigned long long* __restrict__ skipped) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (blockIdx.x == 0 && threadIdx.x == 0 && skipped != nullptr) {
    unsigned long long sk = 0;
    for (int i = 0; i < tbl.nsplit; ++i)
      sk += (unsigned long long)(tbl.off[i + 1] - tbl.off[i]) - cnt[i];
    if (sk) atomicAdd(skipped, sk);
  }
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  int lo = 0, hi = tbl.nsplit;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl.blk[mid] <= b) lo = mid; else hi = mid;
  }
  const int s = __builtin_amdgcn_readfirstlane(lo);
  const long nl = (long)__builtin_amdgcn_readfirstlane(cnt[s]);
  const long lb = b - tbl.blk[s];
  if (lb * 256 >= nl) return;
  const long o = tbl.off[s];
  fin.xnorm = tbl.xnorm[s];
  fin.xbn2 = tbl.xbn2[s];
  fin.xerr = tbl.xerr[s];
  fin.sidx = s;
  fin.idx = idx + o;
  fin.gap = gt.gap[s];
  assign_tile_v3<D, F16, true>(tbl.X[s], nl, Ct, chalf, ntiles, labels + o, lb, smem, fin);
}

// 16 features of a row per lane of an 8-lane group: 128m + 32h + 4sub + (0..3)
// (0 past d; d % 4 == 0): each float4 load of the group reads 128 contiguous
// bytes of the row

}  // namespace
