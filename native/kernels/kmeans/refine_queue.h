#pragma once
// Exact K-Means, certification per batch (refine v3): the sharded queues and
// their layout, step 1 (q1, plain and grouped), steps 2 and 3 (q2, q3) on a
// persistent grid, and the statistics kernel.
#include "../common.h"
#include <algorithm>
#include "grouped.h"
#include "refine.h"

namespace {

// ---------------------------------------------------------------------------
// Refine v3: the certification as a compacted queue pipeline over a BATCH of
// splits.  v2 certifies each point in the thread that scanned it and then walks
// the wave's flagged points four at a time, each round a dependent row-load
// chain, so a wave waits out several L2/HBM round trips serially.  v3 splits
// the work by what each step needs:
//   q1 (per split, right after its top-3 assign): step 1 (margins vs bounds)
//       streams every point; the flagged ones are compacted into queue Q1;
//   q2 (once per batch): step 2 over Q1 on a persistent grid, 8 lanes per entry
//       (16 features each), 8 entries per wave, the next entries prefetched and
//       every row load issued before the first FMA; winners that the top three
//       cannot certify go to queue Q2;
//   q3 (once per batch): the Elkan neighbour scan over Q2 (≈1 % of points with
//       fp16 operands).
// The batch pays q2/q3's latency chains once instead of once per split.  Same
// bounds and ties as v1/v2; the fp64 distance sums differ only in summation
// order (labels can differ only on exact fp64 ties).
// Both queues are sharded 8 ways (by blockIdx % 8, i.e. per XCD under the
// round-robin placement): one counter word takes ≈88 atomics/µs
// (MI355X_MICROARCH.md, dequeue row).  Shard j holds its entries contiguously
// at [j * cap, j * cap + count_j).
struct ExactQ1 {
  uint32_t row, split;
  int32_t b, s, t;
  float sb, m3, x2, xn, xe, pad0, pad1;
};
struct ExactQ2 {
  uint32_t row, split;
  int32_t w, pad;
  double dw;
};
static_assert(sizeof(ExactQ1) == 48 && sizeof(ExactQ2) == 24, "queue entry layout");

constexpr int kQShards = 8;
constexpr int kQ1Per = 4;            // points per thread in the step-1 scan
constexpr int kQ2Lanes = 8;          // lanes per Q1 entry in step 2
constexpr int kQ2Per = HBMR_WAVE / kQ2Lanes;
constexpr int kRefineGrid = 2048;    // persistent grid of q2 and q3
// workspace header: Q1 / Q2 shard counts (8 + 8 u32) and the sharded stats
// (8 shards x 4 u64 at kStatsOff): one word per stat took every block's
// atomic at the kernels' tails; kmeans_refine_stats_kernel folds them
constexpr int kStatsOff = 64;
constexpr int kRefineHdr = 512;
constexpr int kHdrClear = kStatsOff + kQShards * 4 * 8;

struct RefineTable {                 // the batch's splits, by value
  int nsplit;
  const float* x32[kMaxGroup];
  int32_t* labels[kMaxGroup];
};

__host__ __device__ inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

struct RefineLayout {
  long cap1, cap2;                   // entries per shard
  unsigned g2;
  size_t off1, off2, bytes;
};
inline RefineLayout refine_layout(int nsplit, const long* ns) {
  RefineLayout L;
  long total = 0, cap1 = 0, nb_fused = 0;
  for (int i = 0; i < nsplit; ++i) {
    total += ns[i];
    cap1 += ceil_div(ceil_div(ns[i], 256 * kQ1Per), kQShards) * 256 * kQ1Per;
    nb_fused += ceil_div(ns[i], 256);
  }
  // the fused top-3 epilogue appends from 256-point workgroups, shard =
  // blockIdx % kQShards: at most ceil(nb / kQShards) workgroups per shard
  L.cap1 = std::max<long>(cap1, ceil_div(nb_fused, kQShards) * 256);
  L.g2 = (unsigned)std::max<long>(1, std::min<long>(kRefineGrid, ceil_div(total, 4 * kQ2Per)));
  const long per_iter = (long)L.g2 * 4 * kQ2Per;           // Q1 entries per grid iteration
  L.cap2 = ceil_div(L.g2, kQShards) * 4 * kQ2Per * std::max<long>(1, ceil_div(total, per_iter));
  L.off1 = kRefineHdr;
  L.off2 = L.off1 + ((kQShards * (size_t)L.cap1 * sizeof(ExactQ1) + 255) & ~(size_t)255);
  L.bytes = L.off2 + kQShards * (size_t)L.cap2 * sizeof(ExactQ2);
  return L;
}

// item i of the flattened sharded queue → its slot (counts of the 8 shards)
__device__ __forceinline__ long shard_slot(const uint32_t (&c)[kQShards], long cap, uint32_t i) {
  uint32_t acc = 0;
  long slot = 0;
#pragma unroll
  for (int j = 0; j < kQShards; ++j) {
    if (i >= acc && i < acc + c[j]) slot = (long)j * cap + (i - acc);
    acc += c[j];
  }
  return slot;
}

__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Step 1's certification of one point (its kernel top-3 in e, best - second
// margin m2, cnb / ceb = |c_b|, |c_b - c~_b|): true = not certified, the point
// goes to step 2.  Shared by the step-1 scan and the fused top-3 epilogue.
//
// GAP: also the point's bound for the next passes (see kmeans_bound_sweep_kernel),
// a lower bound of min_{j != b} |x - c_j| - |x - c_b| over the fp32 data
// (distances, not squared), 0 for a flagged point.  The rule that certified
// the point established D_j - D_b >= delta for every j != b: the generic rule
// s_b >= s~_b - E_b and s_j <= s~_s + E_max(s), i.e. delta = 2 (mm - eb - es);
// the pair rule the smaller of its s term 2 (mm - ep) and its t term
// 2 (m3 - eb - et).  With sqrt(D_b) <= R = sqrt(dhi_b) + a_b (exact_bound's
// upper bound of D~_b and the operands' rounding error) and sqrt(D + delta) -
// sqrt(D) falling in D:  |x - c_j| - |x - c_b| >= delta / (sqrt(R^2 + delta) + R),
// evaluated in fp64, shaved by 2^-30 twice for its own rounding, rounded down.
template <bool GAP>
__device__ __forceinline__ bool q1_certify(const ExactQ1& e, float m2, float cnb, float ceb, int k,
                                           double gam, double cm, double cem, double pack_rel,
                                           const float* __restrict__ cnorm,
                                           const float* __restrict__ cerr,
                                           const float* __restrict__ dcc, float& gap) {
  const double inflate = 1.0 + 0x1p-20;
  const double xn = ((double)e.xn + (double)e.xe) * inflate;
  const double x2 = (double)e.x2;
  const double sb = e.sb;
  const double mm = m2;
  const double amax = ((double)e.xe + cem) * inflate;
  double eb, es, dl_b, dl_s;
  exact_bound(sb, ((double)cnb + (double)ceb) * inflate, xn, x2,
              ((double)e.xe + (double)ceb) * inflate, gam, pack_rel, eb, dl_b);
  exact_bound(sb - mm, cm, xn, x2, amax, gam, pack_rel, es, dl_s);
  bool flag = !(mm > eb + es && dl_s >= 2.0 * amax);
  // GAP: certified margin, score units (D / 2).  The generic rule's, whether
  // or not that rule held: it is read only once `flag` is false, and a point
  // that only the pair rule certifies replaces it below.
  double marg = mm - (eb + es);
  const int b = e.b, sc = e.s, t = e.t;
  if (flag && dcc != nullptr && t < k && t != b) {
    // Pair rule: D_s - D_b >= (D~_s - D~_b) - 2|c~_b - c~_s| e_x
    //   - 2 sqrt(D~_s) e_s - 2 sqrt(D~_b) e_b - (e_x + e_b)^2
    // (x - c_j = (x~ - c~_j) + (dx - dc_j); the dx terms of b and s
    // cancel up to (c~_b - c~_s).dx), with |c~_b - c~_s| <= |c_b - c_s|
    // + e_b + e_s — tighter than E_b + E_s where the two centroids are
    // close and the point is not.  Everything ranked at or below t is
    // beaten by the generic rule at t (margin b-t against E_b + E_max(t)).
    const double ex = (double)e.xe * inflate;
    const double ebb = (double)ceb * inflate;
    const double ess = (double)cerr[sc] * inflate;
    const double dbs = ((double)dcc[(size_t)b * k + sc] + (double)ceb + (double)cerr[sc]) *
                       inflate;
    double eap_b, rb, eap_s, rs;
    score_err(sb, ((double)cnb + (double)ceb) * inflate, xn, x2, gam, pack_rel, eap_b, rb);
    score_err(sb - mm, ((double)cnorm[sc] + (double)cerr[sc]) * inflate, xn, x2, gam,
              pack_rel, eap_s, rs);
    const double ep = dbs * ex + rs * ess + rb * ebb + 0.5 * (ex + ebb) * (ex + ebb) +
                      eap_b + eap_s;
    double et, dl_t;
    const double m3 = e.m3;
    exact_bound(sb - m3, cm, xn, x2, amax, gam, pack_rel, et, dl_t);
    if (mm > ep && m3 > eb + et && dl_t >= 2.0 * amax) {
      flag = false;
      if constexpr (GAP) marg = fmin(mm - ep, m3 - (eb + et));
    }
  }
  if constexpr (GAP) {
    gap = 0.f;
    if (!flag && marg > 0.0) {
      const double ctb = ((double)cnb + (double)ceb) * inflate;
      const double eacc = gam * (xn * ctb + 0.5 * ctb * ctb);
      const double slack = 2.0 * (eacc + fabs(sb) * pack_rel) + x2 * 0x1p-22;
      const double r = sqrt(fmax(0.0, x2 - 2.0 * sb) + slack) * (1.0 + 0x1p-40) +
                       ((double)e.xe + (double)ceb) * inflate;
      const double delta = 2.0 * marg * (1.0 - 0x1p-30);
      const double g = delta / (sqrt(r * r + delta) * (1.0 + 0x1p-40) + r) * (1.0 - 0x1p-30);
      gap = fmaxf(0.f, __double2float_rd(g));
    }
  }
  return flag;
}

__device__ __forceinline__ bool q1_flagged(const ExactQ1& e, float m2, float cnb, float ceb, int k,
                                           double gam, double cm, double cem, double pack_rel,
                                           const float* __restrict__ cnorm,
                                           const float* __restrict__ cerr,
                                           const float* __restrict__ dcc) {
  float unused;
  return q1_certify<false>(e, m2, cnb, ceb, k, gam, cm, cem, pack_rel, cnorm, cerr, dcc, unused);
}

// Step 1 over one block of 256 * kQ1Per points of split sidx (block index blk
// within the split); cand / margin second rows at stride cs.
__device__ __forceinline__ void refine_q1_block(
    long n, int sidx, long blk, int d, int k, const float* __restrict__ xnorm,
    const float* __restrict__ xbn2, const float* __restrict__ xerr,
    const float* __restrict__ cnorm, const float* __restrict__ cmax,
    const float* __restrict__ cerr, const float* __restrict__ cerrmax, double pack_rel,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ cand,
    const float* __restrict__ score, const float* __restrict__ margin, long cs,
    uint32_t* __restrict__ qcount, ExactQ1* __restrict__ q1, long cap1,
    unsigned long long* __restrict__ stats, const float* __restrict__ dcc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int shard = blockIdx.x % kQShards;
  __shared__ uint32_t wcnt[4][kQ1Per];
  __shared__ uint32_t base_s;
  const double inflate = 1.0 + 0x1p-20;
  const double gam = (double)(d + 2) * 0x1p-23 * 1.01;
  const double cem = (double)cerrmax[0] * inflate;
  const double cm = (double)cmax[0] * inflate + cem;
  // every load of the four points first, then the dependent gathers, then math
  ExactQ1 e[kQ1Per];
  bool in[kQ1Per];
  float m2[kQ1Per];
#pragma unroll
  for (int i = 0; i < kQ1Per; ++i) {
    const long p = blk * (256 * kQ1Per) + i * 256 + tid;
    in[i] = p < n;
    const long q = in[i] ? p : n - 1;
    e[i].row = (uint32_t)q;
    e[i].split = (uint32_t)sidx;
    e[i].b = labels[q];
    e[i].s = cand[q];
    e[i].t = cand[cs + q];
    e[i].sb = score[q];
    m2[i] = margin[q];
    e[i].m3 = margin[cs + q];
    e[i].x2 = xbn2[q];
    e[i].xn = xnorm[q];
    e[i].xe = xerr[q];
  }
  float cnb[kQ1Per], ceb[kQ1Per];
#pragma unroll
  for (int i = 0; i < kQ1Per; ++i) {
    cnb[i] = cnorm[e[i].b];
    ceb[i] = cerr[e[i].b];
  }
  bool flag[kQ1Per];
  uint32_t rank[kQ1Per];
#pragma unroll
  for (int i = 0; i < kQ1Per; ++i) {
    flag[i] = in[i] && e[i].s < k &&
              q1_flagged(e[i], m2[i], cnb[i], ceb[i], k, gam, cm, cem, pack_rel, cnorm, cerr, dcc);
    const unsigned long long m = __ballot(flag[i]);
    rank[i] = lane_rank(m);
    if (lane == 0) wcnt[wave][i] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int i = 0; i < kQ1Per; ++i) {
        const uint32_t c = wcnt[w][i];
        wcnt[w][i] = tot;
        tot += c;
      }
    base_s = tot ? atomicAdd(qcount + shard, tot) : 0u;
    if (tot) atomicAdd(stats + 4 * shard, (unsigned long long)tot);
  }
  __syncthreads();
  ExactQ1* out = q1 + (long)shard * cap1 + base_s;
#pragma unroll
  for (int i = 0; i < kQ1Per; ++i)
    if (flag[i]) out[wcnt[wave][i] + rank[i]] = e[i];
}

__global__ __launch_bounds__(256) void kmeans_refine_q1_kernel(
    long n, int sidx, int d, int k, const float* __restrict__ xnorm,
    const float* __restrict__ xbn2, const float* __restrict__ xerr,
    const float* __restrict__ cnorm, const float* __restrict__ cmax,
    const float* __restrict__ cerr, const float* __restrict__ cerrmax, double pack_rel,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ cand,
    const float* __restrict__ score, const float* __restrict__ margin,
    uint32_t* __restrict__ qcount, ExactQ1* __restrict__ q1, long cap1,
    unsigned long long* __restrict__ stats, const float* __restrict__ dcc) {
  refine_q1_block(n, sidx, blockIdx.x, d, k, xnorm, xbn2, xerr, cnorm, cmax, cerr, cerrmax,
                  pack_rel, labels, cand, score, margin, n, qcount, q1, cap1, stats, dcc);
}

// the splits of a batch in one launch (after the grouped top-3 assign): the
// batch arrays hold split s at offset off[s], second rows at stride total
struct Q1Table {
  int nsplit;
  long total;
  long n[kMaxGroup];
  long off[kMaxGroup];
  long blk[kMaxGroup + 1];
  const float* xnorm[kMaxGroup];
  const float* xbn2[kMaxGroup];
  const float* xerr[kMaxGroup];
};

__global__ __launch_bounds__(256) void kmeans_refine_q1_grouped_kernel(
    const Q1Table tbl, int d, int k, const float* __restrict__ cnorm,
    const float* __restrict__ cmax, const float* __restrict__ cerr,
    const float* __restrict__ cerrmax, double pack_rel, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ cand, const float* __restrict__ score,
    const float* __restrict__ margin, uint32_t* __restrict__ qcount, ExactQ1* __restrict__ q1,
    long cap1, unsigned long long* __restrict__ stats, const float* __restrict__ dcc) {
  const long b = blockIdx.x;
  int lo = 0, hi = tbl.nsplit;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl.blk[mid] <= b) lo = mid; else hi = mid;
  }
  const int s = __builtin_amdgcn_readfirstlane(lo);
  const long o = tbl.off[s];
  refine_q1_block(tbl.n[s], s, b - tbl.blk[s], d, k, tbl.xnorm[s], tbl.xbn2[s], tbl.xerr[s],
                  cnorm, cmax, cerr, cerrmax, pack_rel, labels + o, cand + o, score + o,
                  margin + o, tbl.total, qcount, q1, cap1, stats, dcc);
}

template <int NM>
__device__ __forceinline__ void load_row16(const float* __restrict__ r, int d, int sub,
                                           float (&v)[16 * NM]) {
  // branch-free: every load is issued (address clamped into the row) and the
  // features past d are zeroed by a select, so all of a round's loads stay in
  // flight together (a guarded load made hipcc wait on each one in turn)
#pragma unroll
  for (int m = 0; m < NM; ++m) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int b = 128 * m + 32 * h + 4 * sub;
      const bool ok = b < d;
      const float4 a = *reinterpret_cast<const float4*>(r + (ok ? b : 0));
      float* o = v + 16 * m + 4 * h;
      o[0] = ok ? a.x : 0.f; o[1] = ok ? a.y : 0.f; o[2] = ok ? a.z : 0.f; o[3] = ok ? a.w : 0.f;
    }
  }
}

__device__ __forceinline__ float row_sum8f(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

__device__ __forceinline__ double row_sum8(double v) {
  v += dpp_f64<0xB1>(v);   // xor 1
  v += dpp_f64<0x4E>(v);   // xor 2
  v += dpp_f64<0x141>(v);  // row_half_mirror: the other quad of the 8-lane group
  return v;
}

template <int NM>
__global__ __launch_bounds__(256) void kmeans_refine_q2_kernel(
    const RefineTable tbl, int d, int ldx, const float* __restrict__ C32, int k,
    const float* __restrict__ cmax, const float* __restrict__ cerrmax, double pack_rel,
    const uint32_t* __restrict__ qcount, const ExactQ1* __restrict__ q1, long cap1,
    uint32_t* __restrict__ q2count, ExactQ2* __restrict__ q2, long cap2,
    unsigned long long* __restrict__ sstats) {
  // Q2 entries are staged in LDS and written out with ONE global atomic per
  // block (at the end, or when the buffer nears full): an atomic-with-return
  // per wave and round on the 8 shard counters, whose latency every spilling
  // wave waited out, was half of this kernel's time (diagnostic variant
  // without it: refine 1.71 -> 0.82 ms per 12.5M points)
  constexpr uint32_t kPerBlk = 4 * kQ2Per;        // entries per block round
  constexpr uint32_t kBuf = 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane / kQ2Lanes, sub = lane % kQ2Lanes;
  __shared__ ExactQ2 sbuf[kBuf];
  __shared__ uint32_t sn, sbase;
  __shared__ unsigned long long cnt[2];
  if (tid < 2) cnt[tid] = 0;
  if (tid == 0) sn = 0;
  __syncthreads();
  const double inflate = 1.0 + 0x1p-20;
  const double gam = (double)(d + 2) * 0x1p-23 * 1.01;
  const double cem = (double)cerrmax[0] * inflate;
  const double cm = (double)cmax[0] * inflate + cem;
  uint32_t c1[kQShards];
  uint32_t total = 0;
#pragma unroll
  for (int j = 0; j < kQShards; ++j) {
    c1[j] = qcount[j];
    total += c1[j];
  }
  const int shard = blockIdx.x % kQShards;
  const uint32_t stride = gridDim.x * kPerBlk;
  const uint32_t off = wave * kQ2Per + grp;
  auto flush = [&]() {            // block-uniform call sites only
    if (tid == 0) {
      sbase = atomicAdd(q2count + shard, sn);
      cnt[1] += sn;
    }
    __syncthreads();
    const uint32_t m = sn;
    for (uint32_t i = tid; i < m; i += 256) q2[(long)shard * cap2 + sbase + i] = sbuf[i];
    __syncthreads();
    if (tid == 0) sn = 0;
    __syncthreads();
  };
  uint32_t bb = blockIdx.x * kPerBlk;
  ExactQ1 e;
  if (bb < total) e = q1[shard_slot(c1, cap1, min(bb + off, total - 1))];
  for (; bb < total; bb += stride) {             // same trip count in every wave
    const ExactQ1 q = e;
    const bool have = bb + off < total;
    // prefetch the next round's entry while this round's rows are in flight
    const uint32_t nb = bb + stride;
    if (nb < total) e = q1[shard_slot(c1, cap1, min(nb + off, total - 1))];
    const bool t_real = q.t < k;
    const float* xr = tbl.x32[q.split] + (size_t)q.row * ldx;
    float xf[16 * NM], c0[16 * NM], c1r[16 * NM], c2[16 * NM];
    load_row16<NM>(xr, d, sub, xf);
    load_row16<NM>(C32 + (size_t)q.b * d, d, sub, c0);
    load_row16<NM>(C32 + (size_t)q.s * d, d, sub, c1r);
    load_row16<NM>(C32 + (size_t)(t_real ? q.t : q.b) * d, d, sub, c2);
    // fp32 distances (a third of the fp64 form's VALU work, which bound this
    // kernel): every term goes through at most 16*NM + 3 roundings (lane fma
    // chain + the 8-lane tree), so |D^ - D| <= rel * D + abs_eps; the winner is
    // decided only where the three bands do not overlap, else the point goes
    // to the neighbour scan, which restarts from w's exact fp64 distance
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16 * NM; ++i) {
      const float e0 = xf[i] - c0[i], e1 = xf[i] - c1r[i], e2 = xf[i] - c2[i];
      f0 = fmaf(e0, e0, f0);
      f1 = fmaf(e1, e1, f1);
      f2 = fmaf(e2, e2, f2);
    }
    f0 = row_sum8f(f0);
    f1 = row_sum8f(f1);
    f2 = row_sum8f(f2);
    const double rel = (double)(16 * NM + 8) * 0x1p-24 * 1.01, aeps = 0x1p-120;
    int w = q.b;
    double dw = f0;
    if ((double)f1 < dw || ((double)f1 == dw && q.s < w)) { w = q.s; dw = f1; }
    if (t_real && ((double)f2 < dw || ((double)f2 == dw && q.t < w))) { w = q.t; dw = f2; }
    const double whi = dw * (1.0 + rel) + aeps;            // >= D_w
    auto beats = [&](double dj) { return dj * (1.0 - rel) - aeps > whi; };
    bool separated = isfinite(whi) &&
                     (w == q.b || beats(f0)) && (w == q.s || beats(f1)) &&
                     (!t_real || w == q.t || beats(f2));
    dw = whi;
    bool certified = !t_real && separated;
    if (t_real && separated) {
      const double xn = ((double)q.xn + (double)q.xe) * inflate;
      const double x2 = (double)q.x2;
      const double amax = ((double)q.xe + cem) * inflate;
      const double st = (double)q.sb - (double)q.m3;
      double et, dl_t;
      exact_bound(st, cm, xn, x2, amax, gam, pack_rel, et, dl_t);
      certified = 0.5 * (x2 - dw) - x2 * 0x1p-23 > st + et && dl_t >= 2.0 * amax;
    }
    if (have && sub == 0 && certified && w != q.b) {
      tbl.labels[q.split][q.row] = w;
      atomicAdd(&cnt[0], 1ull);
    }
    const bool spill = have && sub == 0 && !certified;
    const unsigned long long m = __ballot(spill);
    if (m) {
      uint32_t b2 = 0;
      if (lane == 0) b2 = atomicAdd(&sn, (uint32_t)__popcll(m));    // LDS
      b2 = __shfl(b2, 0);
      if (spill) {
        ExactQ2 o;
        o.row = q.row;
        o.split = q.split;
        o.w = w;
        o.pad = 0;
        o.dw = dw;
        sbuf[b2 + lane_rank(m)] = o;
      }
    }
    __syncthreads();
    if (sn > kBuf - kPerBlk) flush();
  }
  __syncthreads();
  if (sn) flush();
  if (tid < 2 && cnt[tid]) atomicAdd(sstats + 4 * shard + 1 + tid, cnt[tid]);
}

template <int NM>
__global__ __launch_bounds__(256) void kmeans_refine_q3_kernel(
    const RefineTable tbl, int d, int ldx, const float* __restrict__ C32, int k,
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_dist, int L,
    const uint32_t* __restrict__ q2count, const ExactQ2* __restrict__ q2, long cap2,
    unsigned long long* __restrict__ sstats, int nstats) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = lane / kRefineGroup, sub = lane % kRefineGroup;
  __shared__ unsigned long long cnt[3];
  if (tid < 3) cnt[tid] = 0;
  __syncthreads();
  uint32_t c2[kQShards];
  uint32_t total = 0;
#pragma unroll
  for (int j = 0; j < kQShards; ++j) {
    c2[j] = q2count[j];
    total += c2[j];
  }
  const uint32_t nwaves = gridDim.x * 4;
  const uint32_t gw = blockIdx.x * 4 + (tid >> 6);
  for (uint32_t base = gw * 4; base < total; base += nwaves * 4) {
    const uint32_t idx = base + grp;
    const bool have = idx < total;
    const ExactQ2 q = q2[shard_slot(c2, cap2, have ? idx : base)];
    int32_t* lab = tbl.labels[q.split];
    const int b0 = lab[q.row];   // the MFMA pick: step 2 left it in place
    double xv[8 * NM];
    {
      float xf[8 * NM];
      load_row8<NM>(tbl.x32[q.split] + (size_t)q.row * ldx, d, sub, xf);
#pragma unroll
      for (int i = 0; i < 8 * NM; ++i) xv[i] = (double)xf[i];
    }
    const int w0 = q.w;
    int w = w0;
    // step 2 hands over its winner with an fp32 distance (an upper bound):
    // the scan starts from w0's exact fp64 distance
    double dw;
    {
      const float* c0p[1] = {C32 + (size_t)w0 * d};
      double d0[1];
      rows_dist2<NM, 1>(xv, c0p, d, sub, d0);
      dw = d0[0];
    }
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
    const bool full = !done && L < k;
    if (full) {
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
    if (have && sub == 0) {
      atomicAdd(&cnt[1], (unsigned long long)evals);
      if (full) atomicAdd(&cnt[2], 1ull);
      if (w != b0) atomicAdd(&cnt[0], 1ull);
      lab[q.row] = w;
    }
  }
  __syncthreads();
  // sharded stats (kmeans_refine_stats_kernel folds them): word 1 of a shard
  // counts relabels; word 3 counts the scan's neighbour distances in shards
  // 0-3 and its full scans in shards 4-7
  const int sh = blockIdx.x % (kQShards / 2);
  if (tid == 0 && cnt[0]) atomicAdd(sstats + 4 * sh + 1, cnt[0]);
  if (tid == 1 && cnt[1]) atomicAdd(sstats + 4 * sh + 3, cnt[1]);
  if (tid == 2 && cnt[2]) atomicAdd(sstats + 4 * (sh + kQShards / 2) + 3, cnt[2]);
}

// stats[0..2] (+3, 4 when nstats >= 5) += the shards of a refine batch
__global__ void kmeans_refine_stats_kernel(const unsigned long long* __restrict__ ss,
                                           unsigned long long* __restrict__ stats, int nstats) {
  const int t = threadIdx.x;
  if (t >= 5 || (t >= 3 && nstats < 5)) return;
  unsigned long long v = 0;
  if (t < 3) {
    for (int j = 0; j < kQShards; ++j) v += ss[4 * j + t];
  } else {
    for (int j = 0; j < kQShards / 2; ++j) v += ss[4 * (j + (t - 3) * (kQShards / 2)) + 3];
  }
  if (v) stats[t] += v;
}

}  // namespace
