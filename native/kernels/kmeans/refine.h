#pragma once
// Exact K-Means, certification per split: the error bounds of the 16-bit scores
// and the refine v1 / v2 kernels that certify each point's arg-max against the
// fp32 data and re-score the uncertain points in fp64.
#include "../common.h"

namespace {

// ---------------------------------------------------------------------------
// Exact mode, step 2: certify each point's bf16 arg-max against its fp32 data
// and re-score the uncertain points in fp64.
//
// The assign kernel ranks s~_j = x~.c~_j - |c~_j|^2/2 (x~, c~ = bf16 of the fp32
// x, c; fp32 accumulation), i.e. the bf16 distances D~_j = |x~ - c~_j|^2.  With
// the rounding errors themselves, e_x = |x - x~| and e_j = |c_j - c~_j| (fp64,
// rounded up; the worst case u = 2^-8 of bf16's 8 significant bits would give
// u|x|, u|c_j| — about 3.5x looser for round-to-nearest data, and the flagged
// fraction scales with it)
// |(x~ - c~_j) - (x - c_j)| <= a_j = e_x + e_j, so
// |D~_j - D_j| <= a_j (2 sqrt(D~_j) + a_j).  In score units (D/2), adding the
// fp32 accumulation error e_acc and the arg-max packing truncation e_pack:
//     E_j = a_j (2 sqrt(D~_j) + a_j) / 2 + e_acc_j + e_pack_j,   |s~_j - s_j| <= E_j.
// Any cluster t ranked below a cluster r by the kernel (s~_t <= s~_r, so
// D~_t >= D~_r) has  s_t <= s~_r + E_max(r)  (E with |c_t| <= cmax and
// e_t <= e_max; the score falls faster than E_t grows once sqrt(D~_r) >= 2 a_max).  Hence, with the
// kernel's top three b, s, t:
//   1. margin(b, s) > E_b + E_max(s)                 -> b is the exact winner;
//   2. else D_b, D_s, D_t in fp64 from the fp32 rows; the winner w of the three
//      (ties to the lower index) is exact if (|x|^2 - D_w)/2 > s~_t + E_max(t);
//   3. else an Elkan scan: |x - c_j| >= |c_w - c_j| - |x - c_w|, so walking w's
//      centroid neighbours in ascending |c_w - c_j| (nbr_idx / nbr_dist, L per
//      centroid, distances rounded down) can stop at |c_w - c_j| > r_w + r_best;
//      a point that outruns its L neighbours scans every centroid.
// Steps 2-3 run on groups of 16 lanes (8 features per lane, fp64, the point
// held in registers), four flagged points per wave at a time.
// stats += (flagged, relabelled, points that needed step 3).
constexpr int kRefineGroup = 16;
constexpr int kRefineMaxDp = 256;
constexpr int kRefinePer = kRefineMaxDp / kRefineGroup;  // features per lane

// Error bound E of a kernel score sc (point norm xn, |x~|^2 = x2) against a
// centroid of norm cn whose distance vector carries rounding error <= a, and a
// lower bound of sqrt(D~) for the monotonicity test.
__device__ __forceinline__ void exact_bound(double sc, double ct, double xt, double x2, double a,
                                            double gam, double pack_rel, double& e,
                                            double& dlo) {
  // ct, xt: upper bounds of |c~| and |x~| (|c| + |c - c~|, |x| + |x - x~|: no
  // relative-rounding assumption, so fp16 subnormals and saturation are covered)
  const double eacc = gam * (xt * ct + 0.5 * ct * ct);
  const double epack = fabs(sc) * pack_rel;
  const double slack = 2.0 * (eacc + epack) + x2 * 0x1p-22;
  const double dhi = fmax(0.0, x2 - 2.0 * sc) + slack;
  dlo = sqrt(fmax(0.0, x2 - 2.0 * sc - slack));
  e = a * (2.0 * sqrt(dhi) + a) * 0.5 + eacc + epack;
}

// Error of a kernel score sc against the exact rounded-operand score
// (accumulation + packing, eap) and an upper bound of sqrt(D~) (rdhi), for a
// centroid with |c~| <= ct and |x~| <= xt (see exact_bound).
__device__ __forceinline__ void score_err(double sc, double ct, double xt, double x2, double gam,
                                          double pack_rel, double& eap, double& rdhi) {
  const double eacc = gam * (xt * ct + 0.5 * ct * ct);
  eap = eacc + fabs(sc) * pack_rel;
  rdhi = sqrt(fmax(0.0, x2 - 2.0 * sc) + 2.0 * eap + x2 * 0x1p-22);
}

__device__ __forceinline__ double group_sum16(double v) {
#pragma unroll
  for (int off = 1; off < kRefineGroup; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

// |x - c_j|^2 in fp64; xv holds this lane's features 8*sub + 128*m + (0..7)
__device__ __forceinline__ double group_dist2(const double (&xv)[kRefinePer],
                                              const float* __restrict__ c, int d, int sub) {
  double acc = 0.0;
#pragma unroll
  for (int m = 0; m < kRefinePer / 8; ++m) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int i = 8 * sub + 8 * kRefineGroup * m + jj;
      if (i < d) {
        const double e = xv[8 * m + jj] - (double)c[i];
        acc = fma(e, e, acc);
      }
    }
  }
  return group_sum16(acc);
}

// Four distances at once (the Elkan scan's candidates): the loads and FMA
// chains of four centroid rows interleave, and so do the four reductions —
// a scan step otherwise waits out one row's L2 latency and one shuffle chain.
__device__ __forceinline__ void group_dist2x4(const double (&xv)[kRefinePer],
                                              const float* __restrict__ c0,
                                              const float* __restrict__ c1,
                                              const float* __restrict__ c2,
                                              const float* __restrict__ c3, int d, int sub,
                                              double (&out)[4]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int m = 0; m < kRefinePer / 8; ++m) {
    const int b = 8 * sub + 8 * kRefineGroup * m;
    if (b + 8 <= d) {
      float v0[8], v1[8], v2[8], v3[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        v0[jj] = c0[b + jj];
        v1[jj] = c1[b + jj];
        v2[jj] = c2[b + jj];
        v3[jj] = c3[b + jj];
      }
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const double x = xv[8 * m + jj];
        const double e0 = x - (double)v0[jj], e1 = x - (double)v1[jj];
        const double e2 = x - (double)v2[jj], e3 = x - (double)v3[jj];
        a0 = fma(e0, e0, a0);
        a1 = fma(e1, e1, a1);
        a2 = fma(e2, e2, a2);
        a3 = fma(e3, e3, a3);
      }
    } else {
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        if (b + jj < d) {
          const double x = xv[8 * m + jj];
          const double e0 = x - (double)c0[b + jj], e1 = x - (double)c1[b + jj];
          const double e2 = x - (double)c2[b + jj], e3 = x - (double)c3[b + jj];
          a0 = fma(e0, e0, a0);
          a1 = fma(e1, e1, a1);
          a2 = fma(e2, e2, a2);
          a3 = fma(e3, e3, a3);
        }
      }
    }
  }
#pragma unroll
  for (int off = 1; off < kRefineGroup; off <<= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
    a3 += __shfl_xor(a3, off);
  }
  out[0] = a0;
  out[1] = a1;
  out[2] = a2;
  out[3] = a3;
}

__global__ __launch_bounds__(256) void kmeans_refine_kernel(
    const float* __restrict__ X32, long n, int d, int ldx, const float* __restrict__ xnorm,
    const float* __restrict__ xbn2, const float* __restrict__ xerr,
    const float* __restrict__ C32, int k, const float* __restrict__ cnorm,
    const float* __restrict__ cmax, const float* __restrict__ cerr,
    const float* __restrict__ cerrmax, double pack_rel,
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_dist, int L,
    int32_t* __restrict__ labels, const int32_t* __restrict__ cand,
    const float* __restrict__ score, const float* __restrict__ margin,
    unsigned long long* __restrict__ stats, int nstats) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // the counters gather in LDS, one global atomic per counter and block: one
  // per event on a single address serialised ~10^6 atomics per 12.5M points
  __shared__ unsigned long long cnt[5];
  if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
  __syncthreads();
  const double inflate = 1.0 + 0x1p-20;
  const double gam = (double)(d + 2) * 0x1p-23 * 1.01;
  const double cem = (double)cerrmax[0] * inflate;
  const double cm = (double)cmax[0] * inflate + cem;  // bound of |c~_j| for every j
  bool flag = false;
  int b = 0, s2 = 0, s3 = 0;
  double xn = 0.0, x2 = 0.0, sb = 0.0, m3 = 0.0, amax = 0.0;
  if (p < n) {
    b = labels[p];
    s2 = cand[p];
    s3 = cand[n + p];
    if (s2 < k) {  // a padded runner-up (-1e30) is never close: k == 1
      xn = ((double)xnorm[p] + (double)xerr[p]) * inflate;  // bound of |x~|
      x2 = (double)xbn2[p];
      sb = score[p];
      const double m2 = margin[p];
      m3 = margin[n + p];
      const double xe = (double)xerr[p];
      amax = (xe + cem) * inflate;
      double eb, es, dl_b, dl_s;
      exact_bound(sb, ((double)cnorm[b] + (double)cerr[b]) * inflate, xn, x2, (xe + (double)cerr[b]) * inflate,
                  gam, pack_rel, eb, dl_b);
      exact_bound(sb - m2, cm, xn, x2, amax, gam, pack_rel, es, dl_s);
      flag = !(m2 > eb + es && dl_s >= 2.0 * amax);
    }
  }
  unsigned long long mask = __ballot(flag);
  if (lane == 0 && mask) atomicAdd(&cnt[0], (unsigned long long)__popcll(mask));
  const int grp = lane / kRefineGroup, sub = lane % kRefineGroup;
  // four groups take the flagged points of this wave in turn
  while (mask) {
    unsigned long long m = mask;  // the grp-th set bit of mask (or none)
    for (int i = 0; i < grp && m; ++i) m &= m - 1;
    const bool have = m != 0;
    const int src = have ? __ffsll((long long)m) - 1 : 0;
    for (int i = 0; i < 4 && mask; ++i) mask &= mask - 1;
    const long q = __shfl(p, src);
    const int qb = __shfl(b, src), qs = __shfl(s2, src), qt = __shfl(s3, src);
    const double qsb = __shfl(sb, src), qm3 = __shfl(m3, src);
    const double qxn = __shfl(xn, src), qx2 = __shfl(x2, src), qamax = __shfl(amax, src);
    if (!have) continue;
    const float* xr = X32 + (size_t)q * ldx;
    double xv[kRefinePer];
#pragma unroll
    for (int mm = 0; mm < kRefinePer / 8; ++mm)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int i = 8 * sub + 8 * kRefineGroup * mm + jj;
        xv[8 * mm + jj] = i < d ? (double)xr[i] : 0.0;
      }
    const bool t_real = qt < k;
    const double db = group_dist2(xv, C32 + (size_t)qb * d, d, sub);
    const double ds = group_dist2(xv, C32 + (size_t)qs * d, d, sub);
    const double dt = t_real ? group_dist2(xv, C32 + (size_t)qt * d, d, sub) : 0.0;
    int w = qb;
    double dw = db;
    if (ds < dw || (ds == dw && qs < w)) { w = qs; dw = ds; }
    if (t_real && (dt < dw || (dt == dw && qt < w))) { w = qt; dw = dt; }
    bool certified = !t_real;
    if (t_real) {
      double et, dl_t;
      exact_bound(qsb - qm3, cm, qxn, qx2, qamax, gam, pack_rel, et, dl_t);
      // scores are on the bf16 point's baseline: s_t = (|x~|^2 - D_t)/2 with
      // exact D; |x~|^2 (qx2) was stored in fp32, hence the 2^-23 margin.
      // (|x|^2 of the fp32 row would differ by ~|x| e_x, a shift the bound
      // does not carry)
      certified = 0.5 * (qx2 - dw) - qx2 * 0x1p-23 > (qsb - qm3) + et &&
                  dl_t >= 2.0 * qamax;
    }
    if (!certified) {
      if (sub == 0) atomicAdd(&cnt[2], 1ull);
      // step 3: Elkan scan around w0 = w (exact distance r0)
      const int w0 = w;
      const double r0 = sqrt(dw);
      bool done = false;
      const int32_t* ni = nbr_idx + (size_t)w0 * L;
      const float* nd = nbr_dist + (size_t)w0 * L;
      // four neighbours per step: the exit bound r0 + r_best is taken at the
      // step's start (r_best only shrinks, so it admits a superset of the
      // candidates the one-at-a-time walk would visit; the minimum over a
      // superset is the same exact winner)
      const float* cw0 = C32 + (size_t)w0 * d;
      int evals = 0;
      for (int jj = 0; jj < L; jj += 4) {
        const double lim = (r0 + sqrt(dw)) * (1.0 + 0x1p-40);
        if ((double)nd[jj] > lim) {
          done = true;
          break;
        }
        int jv[4];
        const float* cp[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool ok = jj + u < L && (double)nd[jj + u] <= lim;
          jv[u] = ok ? ni[jj + u] : -1;
          cp[u] = ok ? C32 + (size_t)jv[u] * d : cw0;
        }
        double dj[4];
        group_dist2x4(xv, cp[0], cp[1], cp[2], cp[3], d, sub, dj);
        evals += 4;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (jv[u] >= 0 && (dj[u] < dw || (dj[u] == dw && jv[u] < w))) { w = jv[u]; dw = dj[u]; }
      }
      if (sub == 0) {
        atomicAdd(&cnt[3], (unsigned long long)evals);
        if (!done && L < k) atomicAdd(&cnt[4], 1ull);
      }
      if (!done && L < k) {
        for (int j = 0; j < k; j += 4) {  // outran the neighbour list: every centroid
          const float* cp[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) cp[u] = C32 + (size_t)(j + u < k ? j + u : j) * d;
          double dj[4];
          group_dist2x4(xv, cp[0], cp[1], cp[2], cp[3], d, sub, dj);
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (j + u < k && (dj[u] < dw || (dj[u] == dw && j + u < w))) { w = j + u; dw = dj[u]; }
        }
      }
    }
    if (sub == 0 && w != qb) {
      labels[q] = w;
      atomicAdd(&cnt[1], 1ull);
    }
  }
  __syncthreads();
  if (threadIdx.x < (nstats < 5 ? 3 : 5) && cnt[threadIdx.x])
    atomicAdd(stats + threadIdx.x, cnt[threadIdx.x]);
}

// Refine v2: the same certification and the same fp64 sums, bit for bit, laid
// out for latency.  v1 (above) reads rows with 211 scalar dword loads and
// reduces with ds_bpermute shuffles at 163 VGPRs (3 waves per SIMD), so a
// flagged point waits out one L2 round trip per row.  v2 takes NM = ceil(d/128)
// chunks at compile time, loads every row as 16-byte vectors (d % 8 == 0,
// 16-byte aligned rows), issues the point row and all candidate rows before
// the first FMA, and reduces over the 16-lane group with DPP row operations
// (quad_perm, row_half_mirror, row_mirror — one DPP row is 16 lanes), which
// add in the same pairwise order as v1's xor butterfly.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double row_sum16(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]: xor 1
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]: xor 2
  v += dpp_f64<0x141>(v);  // row_half_mirror: the other quad of the half-row
  v += dpp_f64<0x140>(v);  // row_mirror: the other half of the row
  return v;
}

template <int NM>
__device__ __forceinline__ void load_row8(const float* __restrict__ r, int d, int sub,
                                          float (&v)[8 * NM]) {
  // branch-free (see load_row16): clamped address + select, no per-load wait.
  // Lane sub of the 16-lane group owns features 128m + 64h + 4sub + (0..3):
  // each float4 load of the group reads 256 contiguous bytes of the row
#pragma unroll
  for (int m = 0; m < NM; ++m) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int b = 128 * m + 64 * h + 4 * sub;
      const bool ok = b < d;
      const float4 a = *reinterpret_cast<const float4*>(r + (ok ? b : 0));
      float* o = v + 8 * m + 4 * h;
      o[0] = ok ? a.x : 0.f; o[1] = ok ? a.y : 0.f; o[2] = ok ? a.z : 0.f; o[3] = ok ? a.w : 0.f;
    }
  }
}

// R rows' |x - c|^2 (features past d are zero on both sides: fma(0, 0, acc) = acc)
template <int NM, int R>
__device__ __forceinline__ void rows_dist2(const double (&xv)[8 * NM],
                                           const float* const (&rows)[R], int d, int sub,
                                           double (&out)[R]) {
  float cv[R][8 * NM];
#pragma unroll
  for (int r = 0; r < R; ++r) load_row8<NM>(rows[r], d, sub, cv[r]);
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
#pragma unroll
  for (int i = 0; i < 8 * NM; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double e = xv[i] - (double)cv[r][i];
      acc[r] = fma(e, e, acc[r]);
    }
#pragma unroll
  for (int r = 0; r < R; ++r) out[r] = row_sum16(acc[r]);
}

// neighbours per Elkan step: 2 keeps v2 at 128 VGPRs (4 waves per SIMD; 4 rows
// in flight take 134, 3 waves).  The exit bound refreshes every step, and the
// minimum over any superset of the one-at-a-time walk is the same winner.
constexpr int kElkanStep = 2;

template <int NM>
__global__ __launch_bounds__(256) void kmeans_refine_v2_kernel(
    const float* __restrict__ X32, long n, int d, int ldx, const float* __restrict__ xnorm,
    const float* __restrict__ xbn2, const float* __restrict__ xerr,
    const float* __restrict__ C32, int k, const float* __restrict__ cnorm,
    const float* __restrict__ cmax, const float* __restrict__ cerr,
    const float* __restrict__ cerrmax, double pack_rel,
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_dist, int L,
    int32_t* __restrict__ labels, const int32_t* __restrict__ cand,
    const float* __restrict__ score, const float* __restrict__ margin,
    unsigned long long* __restrict__ stats, int nstats) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  __shared__ unsigned long long cnt[5];
  if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
  __syncthreads();
  const double inflate = 1.0 + 0x1p-20;
  const double gam = (double)(d + 2) * 0x1p-23 * 1.01;
  const double cem = (double)cerrmax[0] * inflate;
  const double cm = (double)cmax[0] * inflate + cem;  // bound of |c~_j| for every j
  bool flag = false;
  int b = 0, s2 = 0, s3 = 0;
  double xn = 0.0, x2 = 0.0, sb = 0.0, m3 = 0.0, amax = 0.0;
  if (p < n) {
    b = labels[p];
    s2 = cand[p];
    s3 = cand[n + p];
    if (s2 < k) {
      xn = ((double)xnorm[p] + (double)xerr[p]) * inflate;  // bound of |x~|
      x2 = (double)xbn2[p];
      sb = score[p];
      const double m2 = margin[p];
      m3 = margin[n + p];
      const double xe = (double)xerr[p];
      amax = (xe + cem) * inflate;
      double eb, es, dl_b, dl_s;
      exact_bound(sb, ((double)cnorm[b] + (double)cerr[b]) * inflate, xn, x2, (xe + (double)cerr[b]) * inflate,
                  gam, pack_rel, eb, dl_b);
      exact_bound(sb - m2, cm, xn, x2, amax, gam, pack_rel, es, dl_s);
      flag = !(m2 > eb + es && dl_s >= 2.0 * amax);
    }
  }
  unsigned long long mask = __ballot(flag);
  if (lane == 0 && mask) atomicAdd(&cnt[0], (unsigned long long)__popcll(mask));
  const int grp = lane / kRefineGroup, sub = lane % kRefineGroup;
  while (mask) {
    unsigned long long m = mask;
    for (int i = 0; i < grp && m; ++i) m &= m - 1;
    const bool have = m != 0;
    const int src = have ? __ffsll((long long)m) - 1 : 0;
    for (int i = 0; i < 4 && mask; ++i) mask &= mask - 1;
    const long q = __shfl(p, src);
    const int qb = __shfl(b, src), qs = __shfl(s2, src), qt = __shfl(s3, src);
    const double qsb = __shfl(sb, src), qm3 = __shfl(m3, src);
    const double qxn = __shfl(xn, src), qx2 = __shfl(x2, src), qamax = __shfl(amax, src);
    if (!have) continue;
    const bool t_real = qt < k;
    double xv[8 * NM];
    {
      float xf[8 * NM];
      load_row8<NM>(X32 + (size_t)q * ldx, d, sub, xf);
#pragma unroll
      for (int i = 0; i < 8 * NM; ++i) xv[i] = (double)xf[i];
    }
    double d3[3];
    {
      const float* const rows[3] = {C32 + (size_t)qb * d, C32 + (size_t)qs * d,
                                    C32 + (size_t)(t_real ? qt : qb) * d};
      rows_dist2<NM, 3>(xv, rows, d, sub, d3);
    }
    int w = qb;
    double dw = d3[0];
    if (d3[1] < dw || (d3[1] == dw && qs < w)) { w = qs; dw = d3[1]; }
    if (t_real && (d3[2] < dw || (d3[2] == dw && qt < w))) { w = qt; dw = d3[2]; }
    bool certified = !t_real;
    if (t_real) {
      double et, dl_t;
      exact_bound(qsb - qm3, cm, qxn, qx2, qamax, gam, pack_rel, et, dl_t);
      certified = 0.5 * (qx2 - dw) - qx2 * 0x1p-23 > (qsb - qm3) + et &&
                  dl_t >= 2.0 * qamax;
    }
    if (!certified) {
      if (sub == 0) atomicAdd(&cnt[2], 1ull);
      const int w0 = w;
      const double r0 = sqrt(dw);
      bool done = false;
      const int32_t* ni = nbr_idx + (size_t)w0 * L;
      const float* nd = nbr_dist + (size_t)w0 * L;
      const float* cw0 = C32 + (size_t)w0 * d;
      int evals = 0;
      for (int jj = 0; jj < L; jj += kElkanStep) {
        const double lim = (r0 + sqrt(dw)) * (1.0 + 0x1p-40);
        if ((double)nd[jj] > lim) {
          done = true;
          break;
        }
        int jv[kElkanStep];
        const float* cp[kElkanStep];
#pragma unroll
        for (int v = 0; v < kElkanStep; ++v) {
          const bool ok = jj + v < L && (double)nd[jj + v] <= lim;
          jv[v] = ok ? ni[jj + v] : -1;
          cp[v] = ok ? C32 + (size_t)jv[v] * d : cw0;
        }
        double dj[kElkanStep];
        rows_dist2<NM, kElkanStep>(xv, cp, d, sub, dj);
        evals += kElkanStep;
#pragma unroll
        for (int v = 0; v < kElkanStep; ++v)
          if (jv[v] >= 0 && (dj[v] < dw || (dj[v] == dw && jv[v] < w))) { w = jv[v]; dw = dj[v]; }
      }
      if (sub == 0) {
        atomicAdd(&cnt[3], (unsigned long long)evals);
        if (!done && L < k) atomicAdd(&cnt[4], 1ull);
      }
      if (!done && L < k) {
        for (int j = 0; j < k; j += 4) {
          const float* cp[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) cp[v] = C32 + (size_t)(j + v < k ? j + v : j) * d;
          double dj[4];
          rows_dist2<NM, 4>(xv, cp, d, sub, dj);
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (j + v < k && (dj[v] < dw || (dj[v] == dw && j + v < w))) { w = j + v; dw = dj[v]; }
        }
      }
    }
    if (sub == 0 && w != qb) {
      labels[q] = w;
      atomicAdd(&cnt[1], 1ull);
    }
  }
  __syncthreads();
  if (threadIdx.x < (nstats < 5 ? 3 : 5) && cnt[threadIdx.x])
    atomicAdd(stats + threadIdx.x, cnt[threadIdx.x]);
}

}  // namespace
