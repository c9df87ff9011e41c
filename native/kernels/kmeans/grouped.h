#pragma once
// K-Means assign stage, batched: SplitTable and the grouped assign kernels,
// one launch for every split of a batch of map tasks.
#include "../common.h"
#include "assign.h"

namespace {

// ---------------------------------------------------------------------------
// Grouped (batched) map kernels: one launch covers every split of a batch of
// map tasks.  Each workgroup finds its split in a small table passed by value.
constexpr int kMaxGroup = 64;

struct SplitTable {
  int nsplit;
  int k;
  const __bf16* X[kMaxGroup];
  long n[kMaxGroup];
  long off[kMaxGroup];        // offset of the split's points in the batch arrays
  long blk[kMaxGroup + 1];    // prefix sum of workgroups per split (per kernel)
};

__device__ __forceinline__ int find_split(const SplitTable& t, long b) {
  int lo = 0, hi = t.nsplit;  // t.blk[lo] <= b < t.blk[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.blk[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

template <int D>
__global__ __launch_bounds__(kThreads, 2) void kmeans_assign_grouped_kernel(
    const SplitTable tbl, const __bf16* __restrict__ C, const float* __restrict__ chalf,
    int nchunks, int32_t* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, b));
  assign_tile<D>(tbl.X[s], tbl.n[s], C, chalf, nchunks, labels + tbl.off[s], nullptr,
                 b - tbl.blk[s], smem);
}

template <int D, int PB>
__global__ __launch_bounds__(AssignV2<D>::THREADS, AssignV2<D>::MINB) void kmeans_assign_grouped_v2_kernel(
    const SplitTable tbl, const __bf16* __restrict__ C, const float* __restrict__ chalf,
    int ntiles, int32_t* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, b));
  assign_tile_v2<D, PB>(tbl.X[s], tbl.n[s], C, chalf, ntiles, labels + tbl.off[s], nullptr,
                    b - tbl.blk[s], smem);
}

// Exact mode over a batch of splits in ONE launch (a per-split launch of the
// top-3 assign ran at 57 % MFMA busy against 67 % for a long dispatch): the
// batch's labels / scores and the two-row cand / margin arrays are indexed by
// the batch position (split offset + row), second rows at stride tbl.off[nsplit]
template <int D, int PB, bool F16>
__global__ __launch_bounds__(AssignV2<D>::THREADS, kExactMinB) void
kmeans_assign_top3_grouped_v2_kernel(const SplitTable tbl, const __bf16* __restrict__ C,
                                     const float* __restrict__ chalf, int ntiles,
                                     int32_t* __restrict__ labels, int32_t* __restrict__ cand,
                                     float* __restrict__ scores, float* __restrict__ margin,
                                     long total) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  const int s = __builtin_amdgcn_readfirstlane(find_split(tbl, b));
  const long o = tbl.off[s];
  assign_tile_v2<D, PB, true, F16>(tbl.X[s], tbl.n[s], C, chalf, ntiles, labels + o, scores + o,
                                   b - tbl.blk[s], smem, cand + o, margin + o, total);
}

}  // namespace
