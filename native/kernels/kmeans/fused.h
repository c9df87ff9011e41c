#pragma once
// Exact K-Means, fused assign: the top-3 assign whose epilogue runs step 1 of
// the certification (FusedQ1Fin), as the v2 and the v3 kernel.
#include "../common.h"
#include "assign.h"
#include "grouped.h"
#include "refine_queue.h"

namespace {

// ---------------------------------------------------------------------------
// Top-3 assign with step 1 fused into its epilogue (HBMR_EXACT_FUSED_Q1, the
// default): the lane that finishes a point holds its kernel top 3 and
// margins in registers, certifies it there (q1_flagged) and appends only an
// uncertain point to the step-2 queue — one atomic per workgroup — so the
// candidate / score / margin arrays (20 B per point written, then read back
// with the labels by the step-1 scan) are never materialised.
struct FusedQ1Fin {
  const float* xnorm;
  const float* xbn2;
  const float* xerr;
  int sidx;
  int k;
  double gam, pack_rel;
  const float* cmax_p;       // max |c_j| and max |c_j - c~_j| (device, 1 float each)
  const float* cerrmax_p;
  const float* cnorm;
  const float* cerr;
  const float* dcc;
  uint32_t* qcount;
  ExactQ1* q1;
  long cap1;
  unsigned long long* stats;
  // the bounded pass (BND): entry p of the split's list is point row idx[p]
  // (n = the list's length); a certified point's bound goes to gap[row]
  const uint32_t* idx;
  float* gap;

  template <class AM, int PB, bool BND = false>
  __device__ __forceinline__ void operator()(const AM (&am)[PB], int h, long p0, int col, long n,
                                             int32_t* __restrict__ labels) const {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ uint32_t fq_cnt[4 * PB];
    __shared__ uint32_t fq_base;
    const int shard = blockIdx.x % kQShards;
    const double inflate = 1.0 + 0x1p-20;
    const double cem = (double)cerrmax_p[0] * inflate;
    const double cm = (double)cmax_p[0] * inflate + cem;
    ExactQ1 e[PB];
    bool flag[PB];
    uint32_t rank[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
      float v[3];
      int c[3];
      am[pb].top3(v[0], v[1], v[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) c[i] = am[pb].cluster(v[i], h);
      float ov[3];
      int oc[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        ov[i] = __shfl_xor(v[i], 32);
        oc[i] = __shfl_xor(c[i], 32);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) insert3(v, c, ov[i], oc[i]);
      if (((c[0] ^ c[1]) & AM::TMASK) == 0) {
        v[2] = v[0];
        c[2] = c[0];
      }
      const long p = p0 + pb * 32 + col;
      flag[pb] = false;
      if (h == 0 && p < n) {
        long row = p;
        if constexpr (BND) row = idx[p];
        labels[row] = c[0];
        const float bs = am[pb].score(v[0]);
        const float m2 = bs - am[pb].score(v[1]);
        ExactQ1& q = e[pb];
        q.row = (uint32_t)row;
        q.split = (uint32_t)sidx;
        q.b = c[0];
        q.s = c[1];
        q.t = c[2];
        q.sb = bs;
        q.m3 = bs - am[pb].score(v[2]);
        q.x2 = xbn2[row];
        q.xn = xnorm[row];
        q.xe = xerr[row];
        q.pad0 = q.pad1 = 0.f;
        if constexpr (BND) {
          float gp = 0.f;     // fewer than two clusters: no bound
          flag[pb] = q.s < k && q1_certify<true>(q, m2, cnorm[q.b], cerr[q.b], k, gam, cm, cem,
                                                 pack_rel, cnorm, cerr, dcc, gp);
          gap[row] = gp;
        } else {
          flag[pb] = q.s < k && q1_flagged(q, m2, cnorm[q.b], cerr[q.b], k, gam, cm, cem,
                                           pack_rel, cnorm, cerr, dcc);
        }
      }
      const unsigned long long m = __ballot(flag[pb]);
      rank[pb] = lane_rank(m);
      if (lane == 0) fq_cnt[wave * PB + pb] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t tot = 0;
#pragma unroll
      for (int i = 0; i < 4 * PB; ++i) {
        const uint32_t c = fq_cnt[i];
        fq_cnt[i] = tot;
        tot += c;
      }
      fq_base = tot ? atomicAdd(qcount + shard, tot) : 0u;
      if (tot) atomicAdd(stats + 4 * shard, (unsigned long long)tot);
    }
    __syncthreads();
    ExactQ1* out = q1 + (long)shard * cap1 + fq_base;
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
      if (flag[pb]) out[fq_cnt[wave * PB + pb] + rank[pb]] = e[pb];
  }
};

// ---------------------------------------------------------------------------
// v3 of the fused exact assign (PB = 2 point blocks per wave, D <= 128).  v2
// issues ~100 VALU and ~48 SALU per 32-cluster tile and wave beside its 16
// MFMAs (PMC: MFMA pipes 51 % busy, 40 % of wave cycles issue-stalled;
// profiles/r04_exact_pipe_ab.json).  v3 trims that stream and the registers:
//  * the 16 (tile, register) codes of a tile are made once, in SGPRs, and
//    shared by both point blocks (v2 re-derived them per block: 39 s_add);
//  * -|c|^2/2 is read from LDS straight into the accumulators (v2 kept a bias
//    register set and copied it: 16 v_mov per tile);
//  * the centroid image is tiled (piece-major, hbmr_kmeans_image16_tiled): a
//    tile's DMA is lane-linear on both sides and a lane's k-step s is at a
//    fixed immediate offset (s * 1 KiB) from one base register — no
//    XOR-swizzle offsets (8 VGPRs) or per-read address VALU; 16 lanes of one
//    k-step read 256 contiguous bytes (conflict-free).
// Measured negatives, removed in round 6 (profiles/r05_exact_v3_ab.json):
// just-in-time A reads at 4 waves per SIMD, s_setprio over the MFMA chain,
// epilogue pipelining (two accumulator sets), a half-tile pipeline, two tiles
// per barrier step, a 6-slot ring and DMA reordering; so was v4, which keeps
// the centroids stationary in registers and streams the points
// (profiles/r06_exact_v4_ab.json): its per-block cross-wave merge makes it
// VALU-issue bound; and v5, which takes the barrier out by giving each wave a
// private one-tile slot refilled chunk by chunk (profiles/r06_exact_v5_ab.json):
// 4x the L2->LDS bytes and DMA issues cost more than the barrier (+13 %).
// tiled image: tile t is 32 * D * 2 contiguous bytes already in LDS order
template <int D>
__device__ __forceinline__ void stage_tile32t(char* buf, const __bf16* __restrict__ Ct,
                                              const float* __restrict__ chalf, int tile, int wave,
                                              int lane) {
  using V = AssignV2<D>;
  // wave-uniform bases + a 32-bit lane offset: the saddr form of the DMA (one
  // VGPR of address, not a 64-bit pair per instruction)
  const uint32_t loff = (uint32_t)lane * 16u;
#pragma unroll
  for (int i = 0; i < V::P; ++i) {
    const int base = (i * V::WAVES + wave) * HBMR_WAVE;
    const char* g = reinterpret_cast<const char*>(Ct) + (size_t)tile * V::TILE_BYTES +
                    (size_t)base * 16;
    __builtin_amdgcn_global_load_lds((const void*)(g + loff), (void*)(buf + base * 16), 16, 0, 0);
  }
  if (wave == 0 && lane < 32) {
    const char* g = reinterpret_cast<const char*>(chalf + (size_t)tile * 32);
    __builtin_amdgcn_global_load_lds((const void*)(g + loff / 4u), (void*)(buf + V::TILE_BYTES),
                                     4, 0, 0);
  }
}

// (tile, register) codes of tile t in SGPRs (see PackedArgMax)
__device__ __forceinline__ void tile_codes(uint32_t top, int t, uint32_t (&code)[16]) {
  const uint32_t base = top - ((uint32_t)t << 4);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    code[r] = base | (15u - r);
    asm("" : "+s"(code[r]));
  }
}

// PackedTop2x8::update with precomputed codes (pair insertion, NT tracks)
__device__ __forceinline__ void top2_insert(PackedTop2x8& am, const f32x16& acc,
                                            const uint32_t (&code)[16], uint32_t vmask) {
  constexpr int NT = PackedTop2x8::NT;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if ((r / NT) % 2) continue;
    const float u = __uint_as_float((__float_as_uint(acc[r]) & vmask) | code[r]);
    const float v = __uint_as_float((__float_as_uint(acc[r + NT]) & vmask) | code[r + NT]);
    const float m = vmed3(am.tb[r % NT], u, v);
    am.ts[r % NT] = vmax3(m, am.ts[r % NT], am.ts[r % NT]);
    am.tb[r % NT] = vmax3(am.tb[r % NT], u, v);
  }
}

// BND (the bounded pass): entry p of the workgroup is point row fin.idx[p], n
// the length of the split's list
template <int D, bool F16, bool BND = false>
__device__ __forceinline__ void assign_tile_v3(const __bf16* __restrict__ X, long n,
                                               const __bf16* __restrict__ Ct,
                                               const float* __restrict__ chalf, int ntiles,
                                               int32_t* __restrict__ labels, long blk, char* smem,
                                               const FusedQ1Fin& fin) {
  static_assert(D <= 128, "v3 keeps two 32-point blocks of D <= 128 in registers");
  constexpr int PB = 2, NS = 4;
  using V = AssignV2<D, NS>;
  static_assert(V::WAVES == 4, "v3: 4 waves per workgroup");
  constexpr int KS = V::KS;
  // the bias sits right after the tile's rows whatever D is
  static_assert(V::TILE_BYTES == 32 * D * 2, "tile layout");
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / HBMR_WAVE);
  const int lane = tid & (HBMR_WAVE - 1);
  const int h = lane >> 5;
  const int col = lane & 31;
  const long p0 = blk * (V::WAVES * PB * 32) + (long)wave * PB * 32;
  // a tile buffer + rowoff: this lane's k-step s at s KiB (tiled layout)
  const int rowoff = h * 512 + col * 16;
  auto frag = [&](const char* row, int s) __attribute__((always_inline)) {
    return *reinterpret_cast<const bf16x8*>(row + s * 1024);
  };
  // (load_bias of assign.h, kept as a lambda: calling the helper here reorders
  // the instructions of 28 kernels, tools/kernel_isa_diff.py)
  auto bias = [&](const char* buf, f32x16& acc) __attribute__((always_inline)) {
    const float* ch = reinterpret_cast<const float*>(buf + V::TILE_BYTES);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(ch + 8 * g + 4 * h);
      acc[4 * g + 0] = v[0];
      acc[4 * g + 1] = v[1];
      acc[4 * g + 2] = v[2];
      acc[4 * g + 3] = v[3];
    }
  };

#pragma unroll
  for (int i = 0; i < NS; ++i)
    if (i < ntiles) stage_tile32t<D>(smem + i * V::BUF, Ct, chalf, i, wave, lane);

  bf16x8 bfrag[PB][KS];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    long p = p0 + pb * 32 + col;
    if (p >= n) p = n - 1;
    if constexpr (BND) p = fin.idx[p];
    const uint4* row = reinterpret_cast<const uint4*>(X + p * D);
#pragma unroll
    for (int s = 0; s < KS; ++s) bfrag[pb][s] = __builtin_bit_cast(bf16x8, row[2 * s + h]);
  }
  PackedTop2x8 am[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) am[pb].init(ntiles);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(bfrag[pb][s]));
  __syncthreads();
  const bool w0 = wave == 0;
  const uint32_t top = am[0].top;
  const uint32_t vmask = am[0].vmask;   // one copy for both blocks

  // v2's ring (tile t+1's A read during tile t), codes shared, bias into acc
  bf16x8 a[KS];
  f32x16 bz;
  {
    const char* row = smem + rowoff;
#pragma unroll
    for (int s = 0; s < KS; ++s) a[s] = frag(row, s);
    bias(smem, bz);
  }
  int slot = 0;
  for (int t = 0; t < ntiles; ++t) {
    wait_tile_dmas<V::P, NS - 2>(max(0, min(NS - 2, ntiles - 2 - t)), w0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    char* rbuf = smem + slot * V::BUF;
    if (t + NS < ntiles) stage_tile32t<D>(rbuf, Ct, chalf, t + NS, wave, lane);
    slot = slot + 1 == NS ? 0 : slot + 1;
    const char* nbuf = smem + slot * V::BUF;
    const char* nrow = nbuf + rowoff;
    f32x16 acc[PB];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
        acc[pb] = mfma32x32x16<F16>(a[s], bfrag[pb][s], s == 0 ? bz : acc[pb]);
      a[s] = frag(nrow, s);
    }
    uint32_t code[16];
    tile_codes(top, t, code);
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) top2_insert(am[pb], acc[pb], code, vmask);
    bias(nbuf, bz);
  }
  fin.template operator()<PackedTop2x8, PB, BND>(am, h, p0, col, n, labels);
}

struct TopQ1Table {       // the batch's splits, by value (X, per-point norms)
  int nsplit;
  const __bf16* X[kMaxGroup];
  const float* xnorm[kMaxGroup];
  const float* xbn2[kMaxGroup];
  const float* xerr[kMaxGroup];
  long off[kMaxGroup + 1];
  long blk[kMaxGroup + 1];
};

template <int D, bool F16>
__global__ __launch_bounds__(AssignV2<D>::THREADS, kExactMinB) void
kmeans_assign_top3_q1_grouped_kernel(const TopQ1Table tbl, const __bf16* __restrict__ C,
                                     const float* __restrict__ chalf, int ntiles,
                                     int32_t* __restrict__ labels, FusedQ1Fin fin) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  int lo = 0, hi = tbl.nsplit;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl.blk[mid] <= b) lo = mid; else hi = mid;
  }
  const int s = __builtin_amdgcn_readfirstlane(lo);
  const long o = tbl.off[s];
  fin.xnorm = tbl.xnorm[s];
  fin.xbn2 = tbl.xbn2[s];
  fin.xerr = tbl.xerr[s];
  fin.sidx = s;
  assign_tile_v2<D, 2, true, F16, FusedQ1Fin>(tbl.X[s], tbl.off[s + 1] - o, C, chalf, ntiles,
                                              labels + o, nullptr, b - tbl.blk[s], smem, nullptr,
                                              nullptr, -1, &fin);
}

// v3 (see assign_tile_v3): kExactMinB workgroups of 4 waves per CU
template <int D, bool F16>
__global__ __launch_bounds__(256, kExactMinB) void kmeans_assign_top3_q1_v3_kernel(
    const TopQ1Table tbl, const __bf16* __restrict__ Ct, const float* __restrict__ chalf,
    int ntiles, int32_t* __restrict__ labels, FusedQ1Fin fin) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long b = hbmr_xcd_remap(blockIdx.x, gridDim.x);
  int lo = 0, hi = tbl.nsplit;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl.blk[mid] <= b) lo = mid; else hi = mid;
  }
  const int s = __builtin_amdgcn_readfirstlane(lo);
  const long o = tbl.off[s];
  fin.xnorm = tbl.xnorm[s];
  fin.xbn2 = tbl.xbn2[s];
  fin.xerr = tbl.xerr[s];
  fin.sidx = s;
  assign_tile_v3<D, F16>(tbl.X[s], tbl.off[s + 1] - o, Ct, chalf, ntiles, labels + o,
                         b - tbl.blk[s], smem, fin);
}

}  // namespace
