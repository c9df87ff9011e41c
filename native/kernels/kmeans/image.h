#pragma once
// Exact K-Means staging: the 16-bit copy and norms of a split's points, the
// 16-bit centroid images (row-major and tiled) and the centroid neighbour table
// of the Elkan scan.
#include "../common.h"
#include "refine.h"

namespace {

// ---------------------------------------------------------------------------
// Exact mode staging.  A split's fp32 rows become the 16-bit MFMA copy (fp16 by
// default, saturated at ±65504; or bf16) plus, per point, |x| (fp64 → fp32),
// |x~|^2 (fp64 → fp32) and the rounding error |x - x~| (fp64, rounded UP):
// the certification's inputs.  16 lanes per row, 8 features per lane.
__device__ __forceinline__ uint16_t hbmr_f32_to_f16_sat(float v) {
  const _Float16 h = (_Float16)fminf(fmaxf(v, -65504.f), 65504.f);
  return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float hbmr_f16_to_f32(uint16_t b) {
  return (float)__builtin_bit_cast(_Float16, b);
}

__global__ __launch_bounds__(256) void kmeans_exact_prep_kernel(
    const float* __restrict__ x, long n, int d, int ldx, int dp, int f16,
    uint16_t* __restrict__ x16, float* __restrict__ xnorm, float* __restrict__ xn2,
    float* __restrict__ xerr) {
  const long row = (long)blockIdx.x * 16 + threadIdx.x / kRefineGroup;
  const int sub = threadIdx.x % kRefineGroup;
  const bool ok = row < n;
  const long r = ok ? row : n - 1;
  double a = 0.0, q = 0.0, e = 0.0;
  for (int i0 = 8 * sub; i0 < dp; i0 += 8 * kRefineGroup) {
    uint16_t hb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + j;
      const float v = i < d ? x[r * ldx + i] : 0.f;
      const uint16_t b = f16 ? hbmr_f32_to_f16_sat(v) : hbmr_f32_to_bf16(v);
      const float vt = f16 ? hbmr_f16_to_f32(b) : hbmr_bf16_to_f32(b);
      hb[j] = b;
      a = fma((double)v, (double)v, a);
      q = fma((double)vt, (double)vt, q);
      const double df = (double)v - (double)vt;
      e = fma(df, df, e);
    }
    if (ok) {
      uint4 w;
      w.x = hb[0] | ((uint32_t)hb[1] << 16);
      w.y = hb[2] | ((uint32_t)hb[3] << 16);
      w.z = hb[4] | ((uint32_t)hb[5] << 16);
      w.w = hb[6] | ((uint32_t)hb[7] << 16);
      *reinterpret_cast<uint4*>(x16 + r * dp + i0) = w;
    }
  }
  a = row_sum16(a);
  q = row_sum16(q);
  e = row_sum16(e);
  if (ok && sub == 0) {
    xnorm[r] = (float)sqrt(a);
    xn2[r] = (float)q;
    xerr[r] = __double2float_ru(sqrt(e) * (1.0 + 0x1p-50));
  }
}

// Tiled copy of a 16-bit image [k_pad, dp] (dp = 64 / 128) for the v3 assign:
// tile T (32 rows) holds its 16-byte pieces piece-major, (q, r) at
// T * 32 * dp * 2 + q * 512 + r * 16 bytes (q = piece in the row, r = row).
__global__ __launch_bounds__(256) void kmeans_image16_tiled_kernel(const uint4* __restrict__ c16,
                                                                   int k_pad, int dp,
                                                                   uint4* __restrict__ c16t) {
  const long P = (long)blockIdx.x * 256 + threadIdx.x;
  const int cpr = dp / 8;
  if (P >= (long)k_pad * cpr) return;
  const long T = P / (32 * cpr);
  const int w = (int)(P % (32 * cpr));
  const int q = w / 32, r = w % 32;
  c16t[P] = c16[(T * 32 + r) * cpr + q];
}

// The 16-bit image of the fp32 centroids for exact mode (fp16 by default):
// c16 [k_pad, dp], chalf = -|c~|^2/2 (fp32, summed as kmeans_update sums the
// bf16 image's), |c| and |c - c~| (fp64, rounded up) and their maxima (as
// float bits: non-negative floats order as unsigned).  One workgroup per row.
__global__ __launch_bounds__(128) void kmeans_image16_kernel(
    const float* __restrict__ cen, int k, int d, int dp, int f16, uint16_t* __restrict__ c16,
    float* __restrict__ chalf, float* __restrict__ cnorm, float* __restrict__ cerr,
    unsigned* __restrict__ maxbits) {
  const int j = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ float red[128];
  __shared__ double red64[2][128];
  float nrm = 0.f;
  double a = 0.0, e = 0.0;
  for (int i = tid; i < dp; i += 128) {
    const float v = (j < k && i < d) ? cen[(size_t)j * d + i] : 0.f;
    const uint16_t b = f16 ? hbmr_f32_to_f16_sat(v) : hbmr_f32_to_bf16(v);
    const float vt = f16 ? hbmr_f16_to_f32(b) : hbmr_bf16_to_f32(b);
    c16[(size_t)j * dp + i] = b;
    nrm += vt * vt;
    a = fma((double)v, (double)v, a);
    const double df = (double)v - (double)vt;
    e = fma(df, df, e);
  }
  red[tid] = nrm;
  red64[0][tid] = a;
  red64[1][tid] = e;
  __syncthreads();
  for (int s = 64; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red64[0][tid] += red64[0][tid + s];
      red64[1][tid] += red64[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    chalf[j] = j < k ? -0.5f * red[0] : -1.0e30f;
    if (j < k) {
      const float cn = __double2float_ru(sqrt(red64[0][0]) * (1.0 + 0x1p-50));
      const float ce = __double2float_ru(sqrt(red64[1][0]) * (1.0 + 0x1p-50));
      cnorm[j] = cn;
      cerr[j] = ce;
      atomicMax(maxbits + 0, __float_as_uint(cn));
      atomicMax(maxbits + 1, __float_as_uint(ce));
    }
  }
}

// One workgroup per centroid a: D(a, b) = sum_i (c_ai - c_bi)^2 in fp64 — one
// rounded difference and d fused square-adds, |D~ - D| <= (d + 2) 2^-53 D —
// then the lower bound sqrt(D~ (1 - rel)) rounded DOWN to fp32 and the upper
// bound sqrt(D~ (1 + rel)) rounded UP (rel = (d + 4) 2^-53 * 1.01 also covers
// the product and sqrt roundings).  The (lower bound, b) keys of the row are
// bitonic-sorted in LDS — ties by index, i.e. a stable sort — and the L
// first kept (di, dv: the scan order and its stop rule); pd[a][b] gets the
// upper bounds.  The pairwise form (not the Gram form) bounds the error by D
// itself, so near centroids keep tight bounds.
constexpr int kNbrThreads = 256;
constexpr int kNbrMaxD = 256;
constexpr int kNbrMaxK = 8192;

__global__ __launch_bounds__(kNbrThreads) void kmeans_centroid_nbr_kernel(
    const float* __restrict__ cen, int k, int d, int L, int kp2, double rel,
    int32_t* __restrict__ di, float* __restrict__ dv, float* __restrict__ pd) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];   // kp2
  __shared__ double s_ca[kNbrMaxD];
  const int a = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < d; i += kNbrThreads) s_ca[i] = (double)cen[(long)a * d + i];
  __syncthreads();
  const bool vec4 = (d & 3) == 0;
  for (int b = t; b < kp2; b += kNbrThreads) {
    unsigned long long key = ~0ull;
    if (b < k) {
      float lo_f = 0.f, hi_f = 0.f;
      if (b != a) {
        const float* cb = cen + (long)b * d;
        double acc = 0.0;
        if (vec4) {
          for (int i = 0; i < d; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(cb + i);
            double e = s_ca[i] - (double)v.x;
            acc = fma(e, e, acc);
            e = s_ca[i + 1] - (double)v.y;
            acc = fma(e, e, acc);
            e = s_ca[i + 2] - (double)v.z;
            acc = fma(e, e, acc);
            e = s_ca[i + 3] - (double)v.w;
            acc = fma(e, e, acc);
          }
        } else {
          for (int i = 0; i < d; ++i) {
            const double e = s_ca[i] - (double)cb[i];
            acc = fma(e, e, acc);
          }
        }
        const double lo = sqrt(fmax(0.0, acc * (1.0 - rel)));
        const double hi = sqrt(acc * (1.0 + rel));
        lo_f = (float)lo;
        if ((double)lo_f > lo) lo_f = nextafterf(lo_f, 0.f);
        hi_f = (float)hi;
        if ((double)hi_f < hi) hi_f = nextafterf(hi_f, __builtin_inff());
      }
      if (pd) pd[(long)a * k + b] = hi_f;
      key = ((unsigned long long)__float_as_uint(lo_f) << 32) | (unsigned)b;
    }
    s_key[b] = key;
  }
  __syncthreads();
  for (int size = 2; size <= kp2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < kp2 / 2; i += kNbrThreads) {
        const int pos = 2 * i - (i & (stride - 1));
        const int q = pos + stride;
        const bool up = (pos & size) == 0;
        const unsigned long long x = s_key[pos], y = s_key[q];
        if ((x > y) == up) {
          s_key[pos] = y;
          s_key[q] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int j = t; j < L; j += kNbrThreads) {
    const unsigned long long key = s_key[j];
    di[(long)a * L + j] = (int32_t)(uint32_t)(key & 0xffffffffull);
    dv[(long)a * L + j] = __uint_as_float((uint32_t)(key >> 32));
  }
}

}  // namespace
