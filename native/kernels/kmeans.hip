// K-Means map-side kernels for MI355X (gfx950).
//
// These are the GPU "map function + combiner" of a K-Means MapReduce
// iteration.  In the reference the GPU map task is an external Pipes binary
// launched per task (hadoop-1.0.3/src/mapred/org/apache/hadoop/mapred/pipes/
// Application.java:162-181, PipesGPUMapRunner.java:66-118) and the combiner is
// the C++ CombineRunner (src/c++/pipes/impl/HadoopPipes.cc:660-705); there is no
// GPU code in the reference, so these kernels are designed from scratch
// (SURVEY.md §2.11 K1-K3).
//
//  kmeans_assign   : labels[i] = argmin_j ||x_i - c_j||^2 computed as an MFMA
//                    GEMM  S = C · Xᵀ  (v_mfma_f32_32x32x16_bf16, fp32 accum)
//                    with the centroid tiles staged in LDS by global_load_lds
//                    and a fused running-argmax epilogue on
//                    score = x·c - ||c||²/2 (the -||c||²/2 term is loaded as
//                    the MFMA's initial accumulator, so no subtraction).
//                    Points sit on the MFMA *column* (lane) axis so each
//                    lane's arg-max is register-local: no cross-lane
//                    reduction until the very end.
//  kmeans_accum_*  : per-cluster partial sums / counts (the combiner) with
//                    LDS-privatised accumulators; one global atomic flush per
//                    workgroup instead of one per point (global f32 atomics
//                    run at ≈1.3 TB/s chip-wide: MI355X_MICROARCH.md).
//  kmeans_update   : reduce side: c_j = sum_j / count_j, emits the bf16
//                    centroid image + -||c||²/2 for the next iteration.
//
// This file is the translation unit and holds the extern "C" entry points;
// the kernels and their launch templates are in the sections under kmeans/,
// one stage of the pipeline each:
//  assign.h       : MFMA assign (v1 chunked, v2 pipelined), arg-max epilogues
//  grouped.h      : SplitTable, the grouped (batched) assign kernels
//  combine.h      : combiners (LDS, sorted, grouped, delta), update, pad, convert
//  refine.h       : exact mode, refine v1 / v2 (certify + fp64 re-score)
//  image.h        : exact mode staging, 16-bit images, centroid neighbour table
//  refine_queue.h : exact mode, refine v3 (q1 / q2 / q3 queues, stats)
//  fused.h        : exact mode, top-3 assign with step 1 fused (v2, v3)
//  bounded.h      : exact mode, shift / sweep / bounded assign
//  launch.h       : host launch templates
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "kmeans/assign.h"
#include "kmeans/grouped.h"
#include "kmeans/combine.h"
#include "kmeans/refine.h"
#include "kmeans/image.h"
#include "kmeans/refine_queue.h"
#include "kmeans/fused.h"
#include "kmeans/bounded.h"
#include "kmeans/launch.h"

extern "C" {

int hbmr_kmeans_assign_bf16(const void* X, long n, int dp, const void* C, const float* chalf,
                            int k_pad, int32_t* labels, float* scores, hipStream_t st) {
  return dispatch_dp(dp, [&](auto D) {
    return launch_assign<D()>(X, n, C, chalf, k_pad, labels, scores, st);
  });
}

// Workspace of the sorted combiner: hist[k] | offsets[k+1] | cursor[k] | perm[n]
// (u32 each, regions 256-B aligned).
long hbmr_kmeans_accum_workspace_bytes(long n, int k) {
  return (long)(3 * ws_align(((size_t)k + 1) * 4) + ws_align((size_t)n * 4));
}

int hbmr_kmeans_accum_bf16(const void* X, long n, int dp, const int32_t* labels, int k,
                           long long* sums, long long* counts, int fx_shift, void* ws,
                           long ws_bytes, int mode, hipStream_t st) {
  return accum_impl<__bf16>(X, n, dp, labels, k, sums, counts, fx_shift, ws, ws_bytes, mode, st);
}

// Exact mode: the combiner over the fp32 points (rows of dp floats), so the
// partial sums are the int64 fixed point of the fp32 data, not of its bf16 copy.
int hbmr_kmeans_accum_f32(const float* X, long n, int dp, const int32_t* labels, int k,
                          long long* sums, long long* counts, int fx_shift, void* ws,
                          long ws_bytes, int mode, hipStream_t st) {
  return accum_impl<float>(X, n, dp, labels, k, sums, counts, fx_shift, ws, ws_bytes, mode, st);
}

int hbmr_kmeans_update(const long long* sums, const long long* counts, int fx_shift, int k, int d,
                       int dp, int k_pad, float* cen, void* cbf, float* chalf, float* shift2,
                       hipStream_t st) {
  if (k <= 0) return 0;
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(k), dim3(128), 0, st, sums, counts, k, d, dp,
                     ldexpf(1.0f, -fx_shift), cen, reinterpret_cast<__bf16*>(cbf), chalf, shift2);
  if (k_pad > k)
    hipLaunchKernelGGL(kmeans_pad_clusters_kernel, dim3(k_pad - k), dim3(64), 0, st,
                       reinterpret_cast<__bf16*>(cbf), chalf, k, k_pad, dp);
  return (int)hipGetLastError();
}

int hbmr_kmeans_padded_k(int k) { return ((k + kCK - 1) / kCK) * kCK; }

int hbmr_kmeans_padded_dim(int d) {
  for (int dp : {64, 128, 256})
    if (d <= dp) return dp;
  return -1;
}

int hbmr_f32_to_bf16_pad(const float* src, long n, int d, int dp, void* dst, hipStream_t st) {
  if (n <= 0) return 0;
  if (d > dp) return (int)hipErrorInvalidValue;
  const long total = n * dp;
  const long grid = std::min<long>((total + 255) / 256, 1L << 20);
  hipLaunchKernelGGL(f32_to_bf16_pad_kernel, dim3((unsigned)grid), dim3(256), 0, st, src, n, d,
                     dp, reinterpret_cast<uint16_t*>(dst));
  return (int)hipGetLastError();
}

// A batch of K-Means map tasks (one per split) launched from C++ in one call:
// assign + combine per split into its own output slab sums[t] / counts[t]
// (zeroed here).  Removes the per-task host overhead of the runtime's launch
// path; each task still gets its own map output (attempt isolation).
long hbmr_kmeans_batch_workspace_bytes(long total_n, int ntasks, int k) {
  return (long)(ws_align((size_t)ntasks * k * 4) * 2 + ws_align((size_t)ntasks * (k + 1) * 4) +
                ws_align((size_t)total_n * 4));
}

int hbmr_kmeans_map_batch(int ntasks, const void* const* X, const long* n, int dp,
                          const void* C, const float* chalf, int k_pad, int k, int32_t* labels,
                          void* ws, long ws_bytes, long long* sums, long long* counts,
                          int fx_shift, int zero_outputs, hipStream_t st) {
  if (ntasks <= 0) return 0;
  if (zero_outputs) {
    HBMR_RETURN_IF_ERROR(hipMemsetAsync(sums, 0, (size_t)ntasks * k * dp * 8, st));
    HBMR_RETURN_IF_ERROR(hipMemsetAsync(counts, 0, (size_t)ntasks * k * 8, st));
  }
  long total = 0;
  for (int t = 0; t < ntasks; ++t) total += n[t];
  const bool small = ((size_t)k * AccCfg<128>::RS * 8 + (size_t)k * 4) <= 76 * 1024 && dp <= 128;
  if (!small && ntasks <= kMaxGroup && k <= 8192 &&
      ws_bytes >= hbmr_kmeans_batch_workspace_bytes(total, ntasks, k)) {
    set_lds_limits();
    return map_batch_grouped(ntasks, X, n, dp, C, chalf, k_pad, k, labels, ws, sums, counts,
                             fx_shift, st, cu_count());
  }
  // every task's labels at its offset in `labels` (as the grouped path lays
  // them out): callers keep them, e.g. as the delta combiner's reference partition
  long off = 0;
  for (int t = 0; t < ntasks; ++t) {
    int rc = hbmr_kmeans_assign_bf16(X[t], n[t], dp, C, chalf, k_pad, labels + off, nullptr, st);
    if (rc) return rc;
    rc = hbmr_kmeans_accum_bf16(X[t], n[t], dp, labels + off, k, sums + (size_t)t * k * dp,
                                counts + (size_t)t * k, fx_shift, ws, ws_bytes, 0, st);
    if (rc) return rc;
    off += n[t];
  }
  return 0;
}

// ---- delta combiner (see kmeans_delta_* above) ------------------------------------
// workspace: hist[B*k] | cursor[B*k] | offsets[B*(k+1)] | mcount[B] | movers[total]
// (uint2) | perm[2*total] (u32), regions 256-B aligned.
long hbmr_kmeans_delta_workspace_bytes(long total_n, int ntasks, int k) {
  return (long)(2 * ws_align((size_t)ntasks * k * 4) + ws_align((size_t)ntasks * (k + 1) * 4) +
                ws_align((size_t)ntasks * 4) + 2 * ws_align((size_t)total_n * 8));
}

int hbmr_kmeans_delta_combine(int ntasks, const void* const* X, const long* n, int dp, int x_f32,
                              int k, const int32_t* labels, void* ws, long ws_bytes,
                              long long* sums, long long* counts, int fx_shift,
                              int32_t* const* g, const long long* const* S0,
                              const long long* const* N0, hipStream_t st) {
  if (ntasks <= 0) return 0;
  if (ntasks > kMaxGroup || k <= 0 || k > 8192 || (dp != 64 && dp != 128 && dp != 256))
    return (int)hipErrorInvalidValue;
  long total = 0;
  for (int i = 0; i < ntasks; ++i) {
    if (n[i] < 0 || n[i] >= (1L << 31)) return (int)hipErrorInvalidValue;
    total += n[i];
  }
  if (ws == nullptr || ws_bytes < hbmr_kmeans_delta_workspace_bytes(total, ntasks, k))
    return (int)hipErrorInvalidValue;
  set_lds_limits();
  return x_f32 ? delta_combine_impl<float>(ntasks, X, n, dp, k, labels, ws, sums, counts,
                                           fx_shift, g, S0, N0, st)
               : delta_combine_impl<__bf16>(ntasks, X, n, dp, k, labels, ws, sums, counts,
                                            fx_shift, g, S0, N0, st);
}

// A batch of map tasks against reference partitions: grouped MFMA assign of
// every split into `labels`, then the delta combiner.
int hbmr_kmeans_map_batch_delta(int ntasks, const void* const* X, const long* n, int dp,
                                const void* C, const float* chalf, int k_pad, int k,
                                int32_t* labels, void* ws, long ws_bytes, long long* sums,
                                long long* counts, int fx_shift, int32_t* const* g,
                                const long long* const* S0, const long long* const* N0,
                                hipStream_t st) {
  if (ntasks <= 0) return 0;
  if (ntasks > kMaxGroup || k_pad % kCK) return (int)hipErrorInvalidValue;
  const int pts = assign_pts_of(dp);
  if (!pts) return (int)hipErrorInvalidValue;
  SplitTable t;
  make_split_table(t, ntasks, k, X, n);
  const long nb = split_blocks(t, [&](long m) { return (m + pts - 1) / pts; });
  if (nb > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (nb > 0) {
    launch_grouped_assign(dp, nb, t, C, chalf, k_pad, labels, st);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
  }
  return hbmr_kmeans_delta_combine(ntasks, X, n, dp, 0, k, labels, ws, ws_bytes, sums, counts,
                                   fx_shift, g, S0, N0, st);
}

int hbmr_kmeans_assign_top3_bf16(const void* X, long n, int dp, const void* C, const float* chalf,
                                 int k_pad, int32_t* labels, int32_t* cand, float* scores,
                                 float* margin, hipStream_t st) {
  if (!labels || !cand || !scores || !margin) return (int)hipErrorInvalidValue;
  return dispatch_dp(dp, [&](auto D) {
    return launch_assign_top3<D(), false>(X, n, C, chalf, k_pad, labels, cand, scores, margin, st);
  });
}

// exact mode's default: fp16 operands (rows of fp16 bit patterns, C the fp16
// centroid image of hbmr_kmeans_image_f16, chalf its -|c~|^2/2)
int hbmr_kmeans_assign_top3_f16(const void* X, long n, int dp, const void* C, const float* chalf,
                                int k_pad, int32_t* labels, int32_t* cand, float* scores,
                                float* margin, hipStream_t st) {
  if (!labels || !cand || !scores || !margin) return (int)hipErrorInvalidValue;
  return dispatch_dp(dp, [&](auto D) {
    return launch_assign_top3<D(), true>(X, n, C, chalf, k_pad, labels, cand, scores, margin, st);
  });
}

// the top-3 assign of a batch of splits in one launch (dp <= 128; else
// hipErrorNotSupported): labels / scores [N], cand / margin [2N] of the batch,
// N = sum n, split i at offset n[0] + ... + n[i-1]
int hbmr_kmeans_assign_top3_grouped(int nsplit, const void* const* X, const long* n, int dp,
                                    int f16, const void* C, const float* chalf, int k_pad,
                                    int32_t* labels, int32_t* cand, float* scores, float* margin,
                                    hipStream_t st) {
  if (!labels || !cand || !scores || !margin) return (int)hipErrorInvalidValue;
  return dispatch_dp(dp, [&](auto D) {
    return f16 ? launch_assign_top3_grouped<D(), true>(nsplit, X, n, C, chalf, k_pad, labels,
                                                       cand, scores, margin, st)
               : launch_assign_top3_grouped<D(), false>(nsplit, X, n, C, chalf, k_pad, labels,
                                                        cand, scores, margin, st);
  });
}

// Exact mode, one batch: top-3 assign with step 1 fused (FusedQ1Fin): labels
// of every point, the batch's step-2 queue and flagged count in ws (as
// hbmr_kmeans_refine_batch_q1g leaves them); dp <= 128
int hbmr_kmeans_assign_top3_q1_grouped(int nsplit, const void* const* X, const long* n, int dp,
                                       int f16, const void* C, const void* Ct,
                                       const float* chalf, int k_pad,
                                       int32_t* labels, const float* const* xnorm,
                                       const float* const* xbn2, const float* const* xerr,
                                       int d, int k, const float* cnorm, const float* cmax,
                                       const float* cerr, const float* cerrmax, void* ws,
                                       long ws_bytes, const float* dcc, hipStream_t st) {
  if (nsplit <= 0 || nsplit > kMaxGroup || k_pad % 32 || k <= 0 || k_pad < k ||
      d > kRefineMaxDp || !labels || ((uintptr_t)ws & 255) || (dp != 64 && dp != 128))
    return (int)hipErrorInvalidValue;
  TopQ1Table t;
  memset(&t, 0, sizeof(t));
  t.nsplit = nsplit;
  long total = 0, nb = 0;
  for (int i = 0; i < nsplit; ++i) {
    if (n[i] < 0 || n[i] > 0x7fffffffL) return (int)hipErrorInvalidValue;
    fill_topq1(t, i, X, xnorm, xbn2, xerr, total, nb);
    total += n[i];
    nb += ceil_div(n[i], kFusedPts);
  }
  t.off[nsplit] = total;
  t.blk[nsplit] = nb;
  const RefineLayout Ly = refine_layout(nsplit, n);
  if (ws_bytes < (long)Ly.bytes) return (int)hipErrorInvalidValue;
  char* w = static_cast<char*>(ws);
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(w, 0, kHdrClear, st));
  if (nb == 0) return 0;
  if (nb > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const FusedQ1Fin fin = make_fused_fin(k, d, k_pad, cnorm, cerr, dcc, cmax, cerrmax, w, Ly);
  // the v3 kernel (default; needs the tiled image Ct), or v2
  // (hbmr_kmeans_set_exact_kernel(2) / HBMR_EXACT_V3=v2, read once)
  if (exact_kernel() == 3) {
    if (!Ct) return (int)hipErrorInvalidValue;
    const auto [kern, lds] = fused_kernel(dp, f16, [](auto D, auto F) {
      return &kmeans_assign_top3_q1_v3_kernel<D(), F()>;
    });
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, st, t,
                       reinterpret_cast<const __bf16*>(Ct), chalf, k_pad / 32, labels, fin);
    return (int)hipGetLastError();
  }
  const auto [kern, lds] = fused_kernel(dp, f16, [](auto D, auto F) {
    return &kmeans_assign_top3_q1_grouped_kernel<D(), F()>;
  });
  hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(AssignV2<64>::THREADS), lds, st, t,
                     reinterpret_cast<const __bf16*>(C), chalf, k_pad / 32, labels, fin);
  return (int)hipGetLastError();
}

// workspace of the bounded pass: list counts and max shifts (kBoundHdr), a
// shift row per split (at most one distinct ref each), the splits' row lists
long hbmr_kmeans_bound_workspace_bytes(long total, int nsplit, int k) {
  if (total < 0 || nsplit <= 0 || nsplit > kMaxGroup || k <= 0) return -1;
  const size_t sh = ((size_t)nsplit * k * sizeof(float) + 255) & ~(size_t)255;
  return (long)(kBoundHdr + sh + (size_t)total * sizeof(uint32_t));
}

// hbmr_kmeans_assign_top3_q1_grouped for splits that keep per-point bounds
// (see kmeans_bound_shift_kernel): g[i] the split's reference labels, gap[i]
// its bounds [n_i] against the centroids ref[i] ([k, d] fp32; null: gap[i]
// holds nothing yet and every row is assigned), cen the current centroids
// [k, d].  Leaves what the grouped call leaves (labels of every point, the
// step-2 queue and flagged count in ws), gap[i] valid against cen, and adds
// the number of points it did not assign to *skipped (device, may be null).
// The list lengths stay on the device: no synchronisation, no read-back.
// Always the v3 kernel: there is no bounded v2, so a caller that honours the
// v2 selection (hbmr_kmeans_get_exact_kernel() == 2) uses the grouped call.
int hbmr_kmeans_assign_top3_q1_bounded(int nsplit, const void* const* X, const long* n, int dp,
                                       int f16, const void* Ct, const float* chalf, int k_pad,
                                       int32_t* labels, const float* const* xnorm,
                                       const float* const* xbn2, const float* const* xerr,
                                       int d, int k, const float* cnorm, const float* cmax,
                                       const float* cerr, const float* cerrmax, void* ws,
                                       long ws_bytes, const float* dcc,
                                       const int32_t* const* g, float* const* gap,
                                       const float* const* ref, const float* cen, void* bws,
                                       long bws_bytes, unsigned long long* skipped,
                                       hipStream_t st) {
  if (nsplit <= 0 || nsplit > kMaxGroup || k_pad % 32 || k <= 0 || k_pad < k || d <= 0 ||
      d > kRefineMaxDp || !labels || ((uintptr_t)ws & 255) || (dp != 64 && dp != 128) || !Ct ||
      !g || !gap || !ref || !cen || !bws || ((uintptr_t)bws & 255))
    return (int)hipErrorInvalidValue;
  TopQ1Table t;
  SweepTable sw;
  GapTable gt;
  ShiftTable sh;
  memset(&t, 0, sizeof(t));
  memset(&sw, 0, sizeof(sw));
  memset(&gt, 0, sizeof(gt));
  memset(&sh, 0, sizeof(sh));
  t.nsplit = sw.nsplit = nsplit;
  long total = 0, nb = 0, nsb = 0;
  int nref = 0;
  for (int i = 0; i < nsplit; ++i) {
    // (an empty split has no rows to bound: its g / gap may be null)
    if (n[i] < 0 || n[i] > 0x7fffffffL || (n[i] > 0 && (!gap[i] || (ref[i] && !g[i]))))
      return (int)hipErrorInvalidValue;
    fill_topq1(t, i, X, xnorm, xbn2, xerr, total, nb);
    sw.off[i] = total;
    sw.blk[i] = nsb;
    sw.n[i] = n[i];
    sw.g[i] = g[i];
    gt.gap[i] = gap[i];
    if (ref[i]) {
      int r = 0;
      while (r < nref && sh.ref[r] != ref[i]) ++r;
      if (r == nref) sh.ref[nref++] = ref[i];
      sw.rid[i] = r;
      sw.gap[i] = gap[i];
    }
    total += n[i];
    nb += ceil_div(n[i], kFusedPts);
    nsb += ceil_div(n[i], 256 * kSweepPer);
  }
  t.off[nsplit] = total;
  t.blk[nsplit] = nb;
  sw.blk[nsplit] = nsb;
  const RefineLayout Ly = refine_layout(nsplit, n);
  if (ws_bytes < (long)Ly.bytes ||
      bws_bytes < hbmr_kmeans_bound_workspace_bytes(total, nsplit, k))
    return (int)hipErrorInvalidValue;
  char* w = static_cast<char*>(ws);
  char* bw = static_cast<char*>(bws);
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(w, 0, kHdrClear, st));
  if (nb == 0) return 0;
  if (nb > 0x7fffffffL) return (int)hipErrorInvalidValue;
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(bw, 0, kBoundHdr, st));
  uint32_t* cnt = reinterpret_cast<uint32_t*>(bw);
  uint32_t* smax = cnt + kMaxGroup;
  float* shift = reinterpret_cast<float*>(bw + kBoundHdr);
  uint32_t* idx = reinterpret_cast<uint32_t*>(
      bw + kBoundHdr + (((size_t)nsplit * k * sizeof(float) + 255) & ~(size_t)255));
  if (nref > 0) {
    hipLaunchKernelGGL(kmeans_bound_shift_kernel, dim3((unsigned)k, (unsigned)nref), dim3(64), 0,
                       st, sh, cen, k, d, shift, smax);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
  }
  hipLaunchKernelGGL(kmeans_bound_sweep_kernel, dim3((unsigned)nsb), dim3(256), 0, st, sw, k,
                     shift, reinterpret_cast<const float*>(smax), labels, cnt, idx);
  HBMR_RETURN_IF_ERROR(hipGetLastError());
  const FusedQ1Fin fin = make_fused_fin(k, d, k_pad, cnorm, cerr, dcc, cmax, cerrmax, w, Ly);
  const auto [kern, lds] = fused_kernel(dp, f16, [](auto D, auto F) {
    return &kmeans_assign_top3_q1_bounded_kernel<D(), F()>;
  });
  hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, st, t, gt,
                     reinterpret_cast<const __bf16*>(Ct), chalf, k_pad / 32, labels, fin,
                     (const uint32_t*)cnt, (const uint32_t*)idx, skipped);
  return (int)hipGetLastError();
}

int hbmr_kmeans_refine_f32(const float* X32, long n, int d, int ldx, const float* xnorm,
                           const float* xbn2, const float* xerr, const float* C32, int k,
                           int k_pad, const float* cnorm, const float* cmax, const float* cerr,
                           const float* cerrmax, const int32_t* nbr_idx,
                           const float* nbr_dist, int L, int32_t* labels, const int32_t* cand,
                           const float* scores, const float* margin, unsigned long long* stats,
                           int nstats, hipStream_t st) {
  if (n <= 0) return 0;
  if (d > ldx || d > kRefineMaxDp || k <= 0 || k_pad < k || L < 1 || L > k)
    return (int)hipErrorInvalidValue;
  const double pack_rel = pack_rel_of(k_pad);
  const long blocks = (n + 255) / 256;
  // v2 wants whole 8-feature lane slices and 16-byte aligned rows
  const bool v2_ok = d % 8 == 0 && ldx % 4 == 0 && ((uintptr_t)X32 & 15) == 0 &&
                     ((uintptr_t)C32 & 15) == 0;
  if (v2_ok) {
    auto kern = d <= 128 ? kmeans_refine_v2_kernel<1> : kmeans_refine_v2_kernel<2>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, st, X32, n, d, ldx, xnorm,
                       xbn2, xerr, C32, k, cnorm, cmax, cerr, cerrmax, pack_rel, nbr_idx,
                       nbr_dist, L, labels, cand, scores, margin, stats, nstats);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(kmeans_refine_kernel, dim3((unsigned)blocks), dim3(256), 0, st, X32, n, d,
                     ldx, xnorm, xbn2, xerr, C32, k, cnorm, cmax, cerr, cerrmax, pack_rel,
                     nbr_idx, nbr_dist, L,
                     labels, cand, scores, margin, stats, nstats);
  return (int)hipGetLastError();
}


int hbmr_kmeans_exact_prep(const float* x, long n, int d, int ldx, int dp, int f16, void* x16,
                           float* xnorm, float* xn2, float* xerr, hipStream_t st) {
  if (n <= 0) return 0;
  if (d > ldx || d > dp || dp % 8 || !x16 || !xnorm || !xn2 || !xerr)
    return (int)hipErrorInvalidValue;
  const long blocks = (n + 15) / 16;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kmeans_exact_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, d,
                     ldx, dp, f16, reinterpret_cast<uint16_t*>(x16), xnorm, xn2, xerr);
  return (int)hipGetLastError();
}

// the fused exact top-3 kernel: 3 (v3, the default) or 2 (v2); -1 restores the
// default (HBMR_EXACT_V3=v2 selects v2).  Returns the previous setting.
int hbmr_kmeans_set_exact_kernel(int v) {
  const int old = g_exact_kernel;
  g_exact_kernel = v == 2 || v == 3 ? v : -1;
  return old;
}

// the fused exact top-3 kernel in effect: 3 or 2
int hbmr_kmeans_get_exact_kernel(void) { return exact_kernel(); }

int hbmr_kmeans_image16_tiled(const void* c16, int k_pad, int dp, void* c16t, hipStream_t st) {
  if (k_pad <= 0 || k_pad % 32 || (dp != 64 && dp != 128) || !c16 || !c16t)
    return (int)hipErrorInvalidValue;
  const long pieces = (long)k_pad * dp / 8;
  hipLaunchKernelGGL(kmeans_image16_tiled_kernel, dim3((unsigned)((pieces + 255) / 256)),
                     dim3(256), 0, st, reinterpret_cast<const uint4*>(c16), k_pad, dp,
                     reinterpret_cast<uint4*>(c16t));
  return (int)hipGetLastError();
}

// maxima: float [2] = (max |c_j|, max |c_j - c~_j|), written by the kernel
int hbmr_kmeans_image16(const float* cen, int k, int d, int dp, int k_pad, int f16, void* c16,
                        float* chalf, float* cnorm, float* cerr, float* maxima, hipStream_t st) {
  if (k <= 0 || k_pad < k || d > dp) return (int)hipErrorInvalidValue;
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(maxima, 0, 2 * sizeof(float), st));
  hipLaunchKernelGGL(kmeans_image16_kernel, dim3((unsigned)k_pad), dim3(128), 0, st, cen, k, d,
                     dp, f16, reinterpret_cast<uint16_t*>(c16), chalf, cnorm, cerr,
                     reinterpret_cast<unsigned*>(maxima));
  return (int)hipGetLastError();
}

int hbmr_kmeans_centroid_nbr(const float* cen, int k, int d, int L, int32_t* di, float* dv,
                             float* pd, hipStream_t st) {
  if (k <= 0 || k > kNbrMaxK || d <= 0 || d > kNbrMaxD || L <= 0 || L > k)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)cen & 15) != 0) return (int)hipErrorInvalidValue;
  int kp2 = 1;
  while (kp2 < k) kp2 <<= 1;
  const size_t lds = (size_t)kp2 * sizeof(unsigned long long);
  static bool lds_set = false;
  if (!lds_set) {
    HBMR_RETURN_IF_ERROR(hipFuncSetAttribute((const void*)kmeans_centroid_nbr_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kNbrMaxK * sizeof(unsigned long long))));
    lds_set = true;
  }
  const double rel = (double)(d + 4) * 0x1p-53 * 1.01;
  hipLaunchKernelGGL(kmeans_centroid_nbr_kernel, dim3((unsigned)k), dim3(kNbrThreads), lds, st,
                     cen, k, d, L, kp2, rel, di, dv, pd);
  return (int)hipGetLastError();
}


// Refine v3 over a batch of splits (ns[nsplit]; at most 64): per split, right
// after its top-3 assign, hbmr_kmeans_refine_batch_q1 (reset = 1 for the
// first split); then hbmr_kmeans_refine_batch_finish once.  The workspace
// holds the two sharded queues (hbmr_kmeans_refine_batch_bytes).
long hbmr_kmeans_refine_batch_bytes(int nsplit, const long* ns) {
  if (nsplit <= 0 || nsplit > kMaxGroup) return -1;
  return (long)refine_layout(nsplit, ns).bytes;
}

int hbmr_kmeans_refine_batch_q1(int nsplit, const long* ns, int s, int d, int k, int k_pad,
                                const float* xnorm, const float* xbn2, const float* xerr,
                                const float* cnorm, const float* cmax, const float* cerr,
                                const float* cerrmax, const int32_t* labels, const int32_t* cand,
                                const float* scores, const float* margin,
                                unsigned long long* stats, void* ws, long ws_bytes, int reset,
                                const float* dcc, hipStream_t st) {
  if (nsplit <= 0 || nsplit > kMaxGroup || s < 0 || s >= nsplit || k <= 0 || k_pad < k ||
      d > kRefineMaxDp || ((uintptr_t)ws & 255))
    return (int)hipErrorInvalidValue;
  for (int i = 0; i < nsplit; ++i)
    if (ns[i] < 0 || ns[i] > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const RefineLayout Ly = refine_layout(nsplit, ns);
  if (ws_bytes < (long)Ly.bytes) return (int)hipErrorInvalidValue;
  char* w = static_cast<char*>(ws);
  uint32_t* c1 = reinterpret_cast<uint32_t*>(w);
  if (reset) HBMR_RETURN_IF_ERROR(hipMemsetAsync(c1, 0, kHdrClear, st));
  const long n = ns[s];
  if (n == 0) return 0;
  const double pack_rel = pack_rel_of(k_pad);
  const long b1 = ceil_div(n, 256 * kQ1Per);
  hipLaunchKernelGGL(kmeans_refine_q1_kernel, dim3((unsigned)b1), dim3(256), 0, st, n, s, d, k,
                     xnorm, xbn2, xerr, cnorm, cmax, cerr, cerrmax, pack_rel, labels, cand,
                     scores, margin, c1, reinterpret_cast<ExactQ1*>(w + Ly.off1), Ly.cap1,
                     reinterpret_cast<unsigned long long*>(w + kStatsOff), dcc);
  return (int)hipGetLastError();
}

// step 1 of a whole batch after hbmr_kmeans_assign_top3_grouped (resets the
// batch's queues): the batch arrays as that call wrote them
int hbmr_kmeans_refine_batch_q1g(int nsplit, const long* ns, int d, int k, int k_pad,
                                 const float* const* xnorm, const float* const* xbn2,
                                 const float* const* xerr, const float* cnorm, const float* cmax,
                                 const float* cerr, const float* cerrmax, const int32_t* labels,
                                 const int32_t* cand, const float* scores, const float* margin,
                                 void* ws, long ws_bytes, const float* dcc, hipStream_t st) {
  if (nsplit <= 0 || nsplit > kMaxGroup || k <= 0 || k_pad < k || d > kRefineMaxDp ||
      ((uintptr_t)ws & 255))
    return (int)hipErrorInvalidValue;
  Q1Table t;
  memset(&t, 0, sizeof(t));
  t.nsplit = nsplit;
  long total = 0, nb = 0;
  for (int i = 0; i < nsplit; ++i) {
    if (ns[i] < 0 || ns[i] > 0x7fffffffL) return (int)hipErrorInvalidValue;
    t.n[i] = ns[i];
    fill_topq1(t, i, nullptr, xnorm, xbn2, xerr, total, nb);
    total += ns[i];
    nb += ceil_div(ns[i], 256 * kQ1Per);
  }
  t.blk[nsplit] = nb;
  t.total = total;
  const RefineLayout Ly = refine_layout(nsplit, ns);
  if (ws_bytes < (long)Ly.bytes) return (int)hipErrorInvalidValue;
  char* w = static_cast<char*>(ws);
  uint32_t* c1 = reinterpret_cast<uint32_t*>(w);
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(c1, 0, kHdrClear, st));
  if (nb == 0) return 0;
  const double pack_rel = pack_rel_of(k_pad);
  hipLaunchKernelGGL(kmeans_refine_q1_grouped_kernel, dim3((unsigned)nb), dim3(256), 0, st, t, d,
                     k, cnorm, cmax, cerr, cerrmax, pack_rel, labels, cand, scores, margin, c1,
                     reinterpret_cast<ExactQ1*>(w + Ly.off1), Ly.cap1,
                     reinterpret_cast<unsigned long long*>(w + kStatsOff), dcc);
  return (int)hipGetLastError();
}

int hbmr_kmeans_refine_batch_finish(int nsplit, const long* ns, const float* const* x32,
                                    int32_t* const* labels, int d, int ldx, const float* C32,
                                    int k, int k_pad, const float* cmax, const float* cerrmax,
                                    const int32_t* nbr_idx, const float* nbr_dist, int L,
                                    unsigned long long* stats, int nstats, void* ws,
                                    long ws_bytes, hipStream_t st) {
  if (nsplit <= 0 || nsplit > kMaxGroup || d > ldx || d > kRefineMaxDp || d % 8 || ldx % 4 ||
      k <= 0 || k_pad < k || L < 1 || L > k || nstats < 3 || ((uintptr_t)C32 & 15) ||
      ((uintptr_t)ws & 255))
    return (int)hipErrorInvalidValue;
  const RefineLayout Ly = refine_layout(nsplit, ns);
  if (ws_bytes < (long)Ly.bytes) return (int)hipErrorInvalidValue;
  RefineTable tbl;
  std::memset(&tbl, 0, sizeof(tbl));
  tbl.nsplit = nsplit;
  for (int i = 0; i < nsplit; ++i) {
    if ((uintptr_t)x32[i] & 15) return (int)hipErrorInvalidValue;
    tbl.x32[i] = x32[i];
    tbl.labels[i] = labels[i];
  }
  const double pack_rel = pack_rel_of(k_pad);
  char* w = static_cast<char*>(ws);
  uint32_t* c1 = reinterpret_cast<uint32_t*>(w);
  uint32_t* c2 = c1 + kQShards;
  const ExactQ1* q1 = reinterpret_cast<const ExactQ1*>(w + Ly.off1);
  ExactQ2* q2 = reinterpret_cast<ExactQ2*>(w + Ly.off2);
  unsigned long long* ss = reinterpret_cast<unsigned long long*>(w + kStatsOff);
  // (q3 walks each point's neighbours through a chain of dependent loads:
  // a full grid keeps 4x more points in flight than the quarter grid did)
  const unsigned g3 = std::max(1u, Ly.g2);
  if (d <= 128) {
    hipLaunchKernelGGL(kmeans_refine_q2_kernel<1>, dim3(Ly.g2), dim3(256), 0, st, tbl, d, ldx,
                       C32, k, cmax, cerrmax, pack_rel, c1, q1, Ly.cap1, c2, q2, Ly.cap2, ss);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
    hipLaunchKernelGGL(kmeans_refine_q3_kernel<1>, dim3(g3), dim3(256), 0, st, tbl, d, ldx, C32,
                       k, nbr_idx, nbr_dist, L, c2, q2, Ly.cap2, ss, nstats);
  } else {
    hipLaunchKernelGGL(kmeans_refine_q2_kernel<2>, dim3(Ly.g2), dim3(256), 0, st, tbl, d, ldx,
                       C32, k, cmax, cerrmax, pack_rel, c1, q1, Ly.cap1, c2, q2, Ly.cap2, ss);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
    hipLaunchKernelGGL(kmeans_refine_q3_kernel<2>, dim3(g3), dim3(256), 0, st, tbl, d, ldx, C32,
                       k, nbr_idx, nbr_dist, L, c2, q2, Ly.cap2, ss, nstats);
  }
  HBMR_RETURN_IF_ERROR(hipGetLastError());
  hipLaunchKernelGGL(kmeans_refine_stats_kernel, dim3(1), dim3(64), 0, st, ss, stats, nstats);
  return (int)hipGetLastError();
}

}  // extern "C"
