#pragma once
// K-Means host side: the launch templates behind the extern "C" entry points
// of kmeans.hip (kernel choice by row width, grids, workspaces, LDS opt-in).
#include "../common.h"
#include "../../include/hbmr/hbmr.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>
#include "assign.h"
#include "grouped.h"
#include "combine.h"
#include "fused.h"

namespace {

// f(std::integral_constant<int, D>{}) for the row width dp among Ds (none
// given: 64, 128, 256); hipErrorInvalidValue for a width with no kernel
template <int... Ds, class F>
int dispatch_dp(int dp, F&& f) {
  if constexpr (sizeof...(Ds) == 0) {
    return dispatch_dp<64, 128, 256>(dp, f);
  } else {
    int rc = (int)hipErrorInvalidValue;
    (void)((dp == Ds && (rc = f(std::integral_constant<int, Ds>{}), true)) || ...);
    return rc;
  }
}

// assign_pts<dp>(); 0 for a width with no kernel
inline int assign_pts_of(int dp) {
  int pts = 0;
  dispatch_dp(dp, [&](auto D) { return pts = assign_pts<D()>(); });
  return pts;
}

// points per workgroup of the fused top-3 kernels, at either width
constexpr int kFusedPts = AssignV2<64>::PTS;
static_assert(kFusedPts == AssignV2<128>::PTS && AssignV2<64>::THREADS == AssignV2<128>::THREADS,
              "the fused launches size one grid and block for dp = 64 and 128");

// {instantiation, dynamic LDS bytes} of a fused top-3 kernel template for
// (dp in {64, 128}, f16): pick(D, F16) names the template's <D, F16>
template <class Pick>
auto fused_kernel(int dp, int f16, Pick pick) {
  std::pair<decltype(pick(std::integral_constant<int, 64>{}, std::true_type{})), size_t> r{};
  dispatch_dp<64, 128>(dp, [&](auto D) {
    r = {f16 ? pick(D, std::true_type{}) : pick(D, std::false_type{}), AssignV2<D()>::LDS_BYTES};
    return 0;
  });
  return r;
}

// relative truncation of the packed arg-max codes: lb = 4 + ceil(log2(k_pad / 32)) bits
inline double pack_rel_of(int k_pad) {
  int tb = 0;
  while ((1 << tb) < k_pad / 32) ++tb;
  return ldexp(1.0, 4 + tb - 23);
}

// the fused epilogue's batch-wide arguments: step-1 queue, counters and stats
// in the workspace w laid out by Ly.  cmax / cerrmax are device values: the
// kernel reads them through the pointers and folds them itself
inline FusedQ1Fin make_fused_fin(int k, int d, int k_pad, const float* cnorm, const float* cerr,
                                 const float* dcc, const float* cmax, const float* cerrmax,
                                 char* w, const RefineLayout& Ly) {
  FusedQ1Fin fin;
  memset(&fin, 0, sizeof(fin));
  fin.k = k;
  fin.gam = (double)(d + 2) * 0x1p-23 * 1.01;
  fin.pack_rel = pack_rel_of(k_pad);
  fin.cnorm = cnorm;
  fin.cerr = cerr;
  fin.dcc = dcc;
  fin.qcount = reinterpret_cast<uint32_t*>(w);
  fin.q1 = reinterpret_cast<ExactQ1*>(w + Ly.off1);
  fin.cap1 = Ly.cap1;
  fin.stats = reinterpret_cast<unsigned long long*>(w + kStatsOff);
  fin.cmax_p = cmax;
  fin.cerrmax_p = cerrmax;
  return fin;
}

// split i of a batch table: its rows (TopQ1Table only), per-point norms, offset
// in the batch's arrays and first workgroup
template <class Table>
void fill_topq1(Table& t, int i, const void* const* X, const float* const* xnorm,
                const float* const* xbn2, const float* const* xerr, long total, long nb) {
  if constexpr (std::is_same<Table, TopQ1Table>::value)
    t.X[i] = reinterpret_cast<const __bf16*>(X[i]);
  t.xnorm[i] = xnorm[i];
  t.xbn2[i] = xbn2[i];
  t.xerr[i] = xerr[i];
  t.off[i] = total;
  t.blk[i] = nb;
}

// a batch's splits as a SplitTable (rows, sizes, offsets; blk by split_blocks);
// returns the batch's number of points
inline long make_split_table(SplitTable& t, int nsplit, int k, const void* const* X,
                             const long* n) {
  memset(&t, 0, sizeof(t));
  t.nsplit = nsplit;
  t.k = k;
  long total = 0;
  for (int i = 0; i < nsplit; ++i) {
    t.X[i] = reinterpret_cast<const __bf16*>(X[i]);
    t.n[i] = n[i];
    t.off[i] = total;
    total += n[i];
  }
  return total;
}

// t.blk for a launch that gives a split of n points per(n) workgroups (or
// waves); returns their number over the batch
template <class F>
long split_blocks(SplitTable& t, F per) {
  long nb = 0;
  for (int i = 0; i < t.nsplit; ++i) {
    t.blk[i] = nb;
    nb += per(t.n[i]);
  }
  t.blk[t.nsplit] = nb;
  return nb;
}

template <int D>
int launch_assign(const void* X, long n, const void* C, const float* chalf, int k_pad,
                  int32_t* labels, float* scores, hipStream_t st) {
  using Cfg = AssignCfg<D>;
  if (n <= 0) return 0;
  if (k_pad % kCK) return (int)hipErrorInvalidValue;
  constexpr int pts = assign_pts<D>();
  const long nblk = (n + pts - 1) / pts;
  if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if constexpr (D <= 128) {
    hipLaunchKernelGGL((kmeans_assign_v2_kernel<D, kV2PB>), dim3((unsigned)nblk),
                       dim3(AssignV2<D>::THREADS), AssignV2<D>::LDS_BYTES, st,
                       reinterpret_cast<const __bf16*>(X), n, reinterpret_cast<const __bf16*>(C),
                       chalf, k_pad / 32, labels, scores);
  } else {
    hipLaunchKernelGGL(kmeans_assign_kernel<D>, dim3((unsigned)nblk), dim3(kThreads),
                       Cfg::LDS_BYTES, st, reinterpret_cast<const __bf16*>(X), n,
                       reinterpret_cast<const __bf16*>(C), chalf, k_pad / kCK, labels, scores);
  }
  return (int)hipGetLastError();
}

template <int D>
void launch_grouped_assign(long nb, const SplitTable& t, const void* C, const float* chalf,
                           int k_pad, int32_t* labels, hipStream_t st) {
  if constexpr (D <= 128) {
    hipLaunchKernelGGL((kmeans_assign_grouped_v2_kernel<D, kV2PB>), dim3((unsigned)nb),
                       dim3(AssignV2<D>::THREADS), AssignV2<D>::LDS_BYTES, st, t,
                       reinterpret_cast<const __bf16*>(C), chalf, k_pad / 32, labels);
  } else {
    hipLaunchKernelGGL(kmeans_assign_grouped_kernel<D>, dim3((unsigned)nb), dim3(kThreads),
                       AssignCfg<D>::LDS_BYTES, st, t, reinterpret_cast<const __bf16*>(C), chalf,
                       k_pad / kCK, labels);
  }
}

inline void launch_grouped_assign(int dp, long nb, const SplitTable& t, const void* C,
                                  const float* chalf, int k_pad, int32_t* labels, hipStream_t st) {
  dispatch_dp(dp, [&](auto D) {
    launch_grouped_assign<D()>(nb, t, C, chalf, k_pad, labels, st);
    return 0;
  });
}

template <typename T, int D>
int launch_accum(const void* Xv, long n, const int32_t* labels, int k, long long* sums,
                 long long* counts, float scale, int num_cu, hipStream_t st) {
  using A = AccCfg<D>;
  if (n <= 0) return 0;
  const T* X = reinterpret_cast<const T*>(Xv);
  const size_t small_bytes = (size_t)k * A::RS * 8 + (size_t)k * 4;
  if (small_bytes <= 76 * 1024) {
    constexpr int U = 8;
    const long per_block = 256 / A::TPP * U;
    long grid = std::min<long>((n + per_block - 1) / per_block, (long)num_cu * 2);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((kmeans_accum_lds_kernel<T, D, U>), dim3((unsigned)grid), dim3(256),
                       small_bytes, st, X, n, labels, k, sums, counts, scale);
  } else {
    // one workgroup per CU: CC u64 rows + queues + counts within ~150 KiB
    constexpr int U = 8;
    const size_t qbytes = (size_t)kAccWaves * kQueue * 4;
    int CC = (int)((150 * 1024 - qbytes) / ((size_t)A::RS * 8 + 4));
    CC = (CC / 8) * 8;
    if (CC > k) CC = k;
    const int nchunk = (k + CC - 1) / CC;
    long nb = ((long)num_cu + nchunk - 1) / nchunk;
    long ppb = (n + nb - 1) / nb;
    ppb = ((ppb + 2047) / 2048) * 2048;
    nb = (n + ppb - 1) / ppb;
    const size_t lds = (size_t)CC * A::RS * 8 + qbytes + (size_t)CC * 4;
    hipLaunchKernelGGL((kmeans_accum_chunked_kernel<T, D, U>), dim3((unsigned)nb, (unsigned)nchunk),
                       dim3(kAccWaves * HBMR_WAVE), lds, st, X, n, labels, k, CC, ppb, sums,
                       counts, scale);
  }
  return (int)hipGetLastError();
}

int cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  return cus;
}

bool set_lds_limits() {
  // Opt every kernel that asks for >64 KiB of dynamic LDS into the full 160 KiB.
  // The limit is static + dynamic, so a kernel with static __shared__ arrays
  // may ask for less; a refused opt-in must not leave a sticky error behind
  // for the next launch's hipGetLastError.
  static bool done = false;
  if (!done) {
    auto optin = [](const void* fn) {
      hipFuncAttributes at{};
      size_t stat = 0;
      if (hipFuncGetAttributes(&at, fn) == hipSuccess) stat = at.sharedSizeBytes;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(160 * 1024 - stat)) != hipSuccess)
        (void)hipGetLastError();
    };
#define HBMR_LDS_OPTIN(fn) optin((const void*)(fn))
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<__bf16, 64, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<__bf16, 128, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<__bf16, 256, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<__bf16, 64, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<__bf16, 128, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<__bf16, 256, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<float, 64, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<float, 128, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_lds_kernel<float, 256, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<float, 64, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<float, 128, 8>));
    HBMR_LDS_OPTIN((kmeans_accum_chunked_kernel<float, 256, 8>));
    HBMR_LDS_OPTIN(kmeans_scatter_grouped_kernel);
    HBMR_LDS_OPTIN(kmeans_delta_scatter_kernel);
    HBMR_LDS_OPTIN(kmeans_delta_diff_kernel);
#undef HBMR_LDS_OPTIN
    done = true;
  }
  return done;
}

template <int D, bool F16>
int launch_assign_top3_grouped(int nsplit, const void* const* X, const long* n, const void* C,
                               const float* chalf, int k_pad, int32_t* labels, int32_t* cand,
                               float* scores, float* margin, hipStream_t st) {
  if constexpr (D > 128) {
    return (int)hipErrorNotSupported;      // the caller launches per split
  } else {
    if (nsplit <= 0 || nsplit > kMaxGroup || k_pad % 32) return (int)hipErrorInvalidValue;
    for (int i = 0; i < nsplit; ++i)
      if (n[i] < 0) return (int)hipErrorInvalidValue;
    SplitTable t;
    const long total = make_split_table(t, nsplit, 0, X, n);
    constexpr int pts = AssignV2<D>::PTS;
    const long nb = split_blocks(t, [](long m) { return (m + pts - 1) / pts; });
    if (nb == 0) return 0;
    if (nb > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((kmeans_assign_top3_grouped_v2_kernel<D, kV2PB, F16>), dim3((unsigned)nb),
                       dim3(AssignV2<D>::THREADS), AssignV2<D>::LDS_BYTES, st, t,
                       reinterpret_cast<const __bf16*>(C), chalf, k_pad / 32, labels, cand, scores,
                       margin, total);
    return (int)hipGetLastError();
  }
}

template <int D, bool F16>
int launch_assign_top3(const void* X, long n, const void* C, const float* chalf, int k_pad,
                       int32_t* labels, int32_t* cand, float* scores, float* margin,
                       hipStream_t st) {
  if (n <= 0) return 0;
  if (k_pad % kCK) return (int)hipErrorInvalidValue;
  constexpr int pts = assign_pts<D>();
  const long nblk = (n + pts - 1) / pts;
  if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if constexpr (D <= 128) {
    hipLaunchKernelGGL((kmeans_assign_top3_v2_kernel<D, kV2PB, F16>), dim3((unsigned)nblk),
                       dim3(AssignV2<D>::THREADS), AssignV2<D>::LDS_BYTES, st,
                       reinterpret_cast<const __bf16*>(X), n, reinterpret_cast<const __bf16*>(C),
                       chalf, k_pad / 32, labels, cand, scores, margin);
  } else {
    hipLaunchKernelGGL((kmeans_assign_top3_kernel<D, F16>), dim3((unsigned)nblk), dim3(kThreads),
                       AssignCfg<D>::LDS_BYTES, st, reinterpret_cast<const __bf16*>(X), n,
                       reinterpret_cast<const __bf16*>(C), chalf, k_pad / kCK, labels, cand,
                       scores, margin);
  }
  return (int)hipGetLastError();
}

static size_t ws_align(size_t b) { return (b + 255) & ~(size_t)255; }

template <typename T>
static int accum_impl(const void* X, long n, int dp, const int32_t* labels, int k,
                      long long* sums, long long* counts, int fx_shift, void* ws, long ws_bytes,
                      int mode, hipStream_t st) {
  set_lds_limits();
  const int cus = cu_count();
  const float scale = ldexpf(1.0f, fx_shift);
  if (n <= 0) return 0;
  // mode: 0 = auto, 1 = LDS-privatised (small k / chunked), 2 = sorted
  const bool small = ((size_t)k * AccCfg<128>::RS * 8 + (size_t)k * 4) <= 76 * 1024 && dp <= 128;
  const bool sorted = mode == 2 || (mode == 0 && !small && ws != nullptr &&
                                    ws_bytes >= hbmr_kmeans_accum_workspace_bytes(n, k));
  if (sorted) {
    if (ws == nullptr || ws_bytes < hbmr_kmeans_accum_workspace_bytes(n, k) || n >= (1L << 32))
      return (int)hipErrorInvalidValue;
    char* w = reinterpret_cast<char*>(ws);
    const size_t kb = ws_align(((size_t)k + 1) * 4);
    uint32_t* hist = reinterpret_cast<uint32_t*>(w);
    uint32_t* offsets = reinterpret_cast<uint32_t*>(w + kb);
    uint32_t* cursor = reinterpret_cast<uint32_t*>(w + 2 * kb);
    uint32_t* perm = reinterpret_cast<uint32_t*>(w + 3 * kb);
    HBMR_RETURN_IF_ERROR(hipMemsetAsync(hist, 0, (size_t)k * 4, st));
    const size_t hlds = (size_t)k * 4;
    long hgrid = std::min<long>((n / 4 + 255) / 256 + 1, (long)cus * 2);
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)hgrid), dim3(256), hlds, st, labels, n,
                       k, hist);
    hipLaunchKernelGGL(kmeans_scan_kernel, dim3(1), dim3(1024), 0, st, hist, k, offsets, cursor,
                       counts);
    const long sgrid = (n + kScatterPts - 1) / kScatterPts;
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((unsigned)sgrid), dim3(256), 2 * hlds, st,
                       labels, n, k, cursor, perm);
    // segsum: one chunk per wave, ~8 waves per CU worth of chunks at least
    // short chunks keep the per-wave dependent-load chain short for small
    // splits; long chunks amortise flush atomics for big ones
    long chunk = (n + (long)cus * 16 - 1) / ((long)cus * 16);
    chunk = std::min<long>(4096, std::max<long>(128, ((chunk + 63) / 64) * 64));
    const long nw = (n + chunk - 1) / chunk;
    const long sblocks = (nw + 3) / 4;
    return dispatch_dp(dp, [&](auto D) {
      hipLaunchKernelGGL((kmeans_segsum_kernel<T, D(), 8>), dim3((unsigned)sblocks), dim3(256),
                         0, st, reinterpret_cast<const T*>(X), n, perm, offsets, k, chunk, sums,
                         scale);
      return (int)hipGetLastError();
    });
  }
  return dispatch_dp(dp, [&](auto D) {
    return launch_accum<T, D()>(X, n, labels, k, sums, counts, scale, cus, st);
  });
}

// Grouped path: 1 memset + 4 launches for the whole batch (assign, histogram,
// scan+scatter, segmented sum).  labels must hold Σ n[t] entries.
static int map_batch_grouped(int ntasks, const void* const* X, const long* n, int dp,
                             const void* C, const float* chalf, int k_pad, int k,
                             int32_t* labels, void* ws, long long* sums, long long* counts,
                             int fx_shift, hipStream_t st, int cus) {
  SplitTable t;
  const long total = make_split_table(t, ntasks, k, X, n);
  char* w = reinterpret_cast<char*>(ws);
  const size_t hb = ws_align((size_t)ntasks * k * 4);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w);
  uint32_t* cursor = reinterpret_cast<uint32_t*>(w + hb);
  uint32_t* offsets = reinterpret_cast<uint32_t*>(w + 2 * hb);
  uint32_t* perm = reinterpret_cast<uint32_t*>(w + 2 * hb + ws_align((size_t)ntasks * (k + 1) * 4));
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(hist, 0, 2 * hb, st));  // hist + cursor
  // 1. assign, then the histogram as an LDS-binned pass over the labels
  const int pts = assign_pts_of(dp);
  if (!pts) return (int)hipErrorInvalidValue;
  long nb = split_blocks(t, [&](long m) { return (m + pts - 1) / pts; });
  if (nb > 0) {
    launch_grouped_assign(dp, nb, t, C, chalf, k_pad, labels, st);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
  }
  const long hb_blocks = split_blocks(t, [](long m) { return (m + kHistPts - 1) / kHistPts; });
  if (hb_blocks > 0) {
    hipLaunchKernelGGL(kmeans_hist_grouped_kernel, dim3((unsigned)hb_blocks), dim3(256),
                       (size_t)k * 4, st, t, labels, hist);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
  }
  // 2. scan + scatter (+ counts, offsets)
  nb = split_blocks(t, [](long m) {
    return std::max<long>(1, (m + kScatterPts - 1) / kScatterPts);
  });
  hipLaunchKernelGGL(kmeans_scatter_grouped_kernel, dim3((unsigned)nb), dim3(256),
                     (size_t)3 * k * 4, st, t, labels, hist, cursor, offsets, perm, counts);
  HBMR_RETURN_IF_ERROR(hipGetLastError());
  // 3. segmented row sums: chunks sized so the batch yields ≥ 16 waves per CU
  long chunk = (total + (long)cus * 16 - 1) / ((long)cus * 16);
  chunk = std::min<long>(4096, std::max<long>(128, ((chunk + 63) / 64) * 64));
  const long nw = split_blocks(t, [&](long m) { return (m + chunk - 1) / chunk; });
  const float scale = ldexpf(1.0f, fx_shift);
  if (nw > 0) {
    const long blocks = (nw + 3) / 4;
    dispatch_dp(dp, [&](auto D) {
      hipLaunchKernelGGL((kmeans_segsum_grouped_kernel<D(), 8>), dim3((unsigned)blocks),
                         dim3(256), 0, st, t, perm, offsets, chunk, sums, scale);
      return 0;
    });
  }
  return (int)hipGetLastError();
}

template <typename T>
static int delta_combine_impl(int ntasks, const void* const* X, const long* n, int dp, int k,
                              const int32_t* labels, void* ws, long long* sums,
                              long long* counts, int fx_shift, int32_t* const* g,
                              const long long* const* S0, const long long* const* N0,
                              hipStream_t st) {
  SplitTable t;
  const long total = make_split_table(t, ntasks, k, X, n);
  char* w = reinterpret_cast<char*>(ws);
  const size_t hb = ws_align((size_t)ntasks * k * 4);
  const size_t ob = ws_align((size_t)ntasks * (k + 1) * 4);
  const size_t mb = ws_align((size_t)ntasks * 4);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w);
  uint32_t* cursor = reinterpret_cast<uint32_t*>(w + hb);
  uint32_t* offsets = reinterpret_cast<uint32_t*>(w + 2 * hb);
  uint32_t* mcount = reinterpret_cast<uint32_t*>(w + 2 * hb + ob);
  uint2* movers = reinterpret_cast<uint2*>(w + 2 * hb + ob + mb);
  uint32_t* perm = reinterpret_cast<uint32_t*>(w + 2 * hb + ob + mb + ws_align((size_t)total * 8));
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(hist, 0, 2 * hb, st));   // hist + cursor
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(mcount, 0, mb, st));
  // 0. outputs start from the reference partition's sums and counts
  SlabTable src;
  memset(&src, 0, sizeof(src));
  for (int i = 0; i < ntasks; ++i) {
    src.s[i] = S0[i];
    src.c[i] = N0[i];
  }
  const long slab = (long)k * dp;
  const unsigned gx = (unsigned)std::max<long>(1, std::min<long>((slab / 2 + 255) / 256, 64));
  hipLaunchKernelGGL(kmeans_slab_copy_kernel, dim3(gx, (unsigned)ntasks), dim3(256), 0, st, src,
                     slab, k, sums, counts);
  HBMR_RETURN_IF_ERROR(hipGetLastError());
  // 1. movers, entry histogram, count deltas, g := labels
  long nb = split_blocks(t, [](long m) { return (m + kDiffPts - 1) / kDiffPts; });
  GTable gt;
  memset(&gt, 0, sizeof(gt));
  for (int i = 0; i < ntasks; ++i) gt.g[i] = g[i];
  if (nb > 0) {
    hipLaunchKernelGGL(kmeans_delta_diff_kernel, dim3((unsigned)nb), dim3(256), (size_t)2 * k * 4,
                       st, t, gt, labels, movers, mcount, hist, counts);
    HBMR_RETURN_IF_ERROR(hipGetLastError());
  }
  // 2. entries sorted by cluster (grid for the worst case, 2n entries per split)
  nb = split_blocks(t, [](long m) {
    return std::max<long>(1, (2 * m + kScatterPts - 1) / kScatterPts);
  });
  hipLaunchKernelGGL(kmeans_delta_scatter_kernel, dim3((unsigned)nb), dim3(256),
                     (size_t)3 * k * 4, st, t, movers, mcount, hist, cursor, offsets, perm);
  HBMR_RETURN_IF_ERROR(hipGetLastError());
  // 3. signed segmented row sums (persistent waves over the device-side counts)
  const float scale = ldexpf(1.0f, fx_shift);
  const unsigned blocks = (unsigned)cu_count() * 4;
  return dispatch_dp(dp, [&](auto D) {
    hipLaunchKernelGGL((kmeans_delta_segsum_kernel<T, D(), 8>), dim3(blocks), dim3(256), 0, st,
                       t, movers, mcount, perm, offsets, 256L, sums, scale);
    return (int)hipGetLastError();
  });
}

}  // namespace
