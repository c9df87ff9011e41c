#pragma once
// K8: merge of two sorted runs (merge path).
#include "../common.h"

namespace {

// ---- K8: merge of sorted runs (merge path) -----------------------------------
// Merge two sorted runs A[0,na) and B[0,nb) of (hi, lo) keys with u32 payloads
// (stable: A before B on equal keys).  Thread t owns output [t*kMergeItems,
// (t+1)*kMergeItems): it finds where that diagonal crosses the merge path by
// binary search, then merges its items sequentially.  Runs are bound by HBM
// bandwidth (each element read once, written once; the search touches
// log2(n) elements per thread).
constexpr int kMergeItems = 16;

__device__ __forceinline__ bool key_lt(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) {
  return ah < bh || (ah == bh && al < bl);
}

__global__ __launch_bounds__(256) void merge_path_kernel(
    const uint64_t* __restrict__ ahi, const uint64_t* __restrict__ alo,
    const uint32_t* __restrict__ av, long na, const uint64_t* __restrict__ bhi,
    const uint64_t* __restrict__ blo, const uint32_t* __restrict__ bv, long nb,
    uint64_t* __restrict__ ohi, uint64_t* __restrict__ olo, uint32_t* __restrict__ ov) {
  const long n = na + nb;
  const long d = ((long)blockIdx.x * 256 + threadIdx.x) * kMergeItems;
  if (d >= n) return;
  // largest i in [max(0, d-nb), min(d, na)] with A[i-1] <= B[d-i] (A wins ties)
  long lo_i = d > nb ? d - nb : 0, hi_i = d < na ? d : na;
  while (lo_i < hi_i) {
    const long i = (lo_i + hi_i + 1) >> 1;
    const long j = d - i;
    // i is feasible iff A[i-1] <= B[j] (j < nb) — i.e. not B[j] < A[i-1]
    if (j >= nb || !key_lt(bhi[j], blo[j], ahi[i - 1], alo[i - 1])) lo_i = i;
    else hi_i = i - 1;
  }
  long i = lo_i, j = d - lo_i;
  const long end = d + kMergeItems < n ? d + kMergeItems : n;
  for (long o = d; o < end; ++o) {
    bool take_a;
    if (i >= na) take_a = false;
    else if (j >= nb) take_a = true;
    else take_a = !key_lt(bhi[j], blo[j], ahi[i], alo[i]);
    if (take_a) {
      ohi[o] = ahi[i];
      olo[o] = alo[i];
      ov[o] = av[i];
      ++i;
    } else {
      ohi[o] = bhi[j];
      olo[o] = blo[j];
      ov[o] = bv[j];
      ++j;
    }
  }
}

}  // namespace
