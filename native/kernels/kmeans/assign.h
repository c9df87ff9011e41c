#pragma once
// K-Means assign stage: the MFMA wrapper, the tile geometry (AssignCfg,
// AssignV2), the arg-max epilogues, the chunked v1 tile loop (D = 256), the
// software-pipelined v2 tile loop (D <= 128) and the four plain assign kernels.
#include "../common.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * HBMR_WAVE;
constexpr int kCK = 64;  // clusters per LDS chunk (two 32-row MFMA blocks)

// One 32x32x16 MFMA on 16-bit operands held as bf16x8 bit patterns: bf16, or
// fp16 (F16) — exact mode's default, whose 11 significant bits round the
// points and centroids 8x closer than bf16's 8 at the same matrix-core rate,
// so 8x fewer points fail the certification (kmeans_refine_*).
template <bool F16>
__device__ __forceinline__ f32x16 mfma32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <int D> struct AssignCfg {
  static constexpr int KS = D / 16;             // MFMA k-steps (K=16 each)
  static constexpr int CPR = D / 8;             // 16-byte pieces per row
  static constexpr int SWZ = CPR >= 16 ? 15 : CPR - 1;
  static constexpr int PB = D <= 128 ? 2 : 1;   // 32-point blocks per wave
  static constexpr int PTS = kWaves * PB * 32;  // points per workgroup
  static constexpr int CHUNK_BYTES = kCK * D * 2;
  static constexpr int BUF_BYTES = CHUNK_BYTES + kCK * 4;
  static constexpr int LDS_BYTES = 2 * BUF_BYTES;
};

// Stage centroid chunk `chunk` (kCK rows × D bf16) plus its -||c||²/2 values
// into LDS buffer `buf`.  The LDS image is lane-linear (global_load_lds writes
// base + lane*16) so the bank-conflict XOR swizzle is applied to the SOURCE
// address: LDS piece (row, p) holds global piece (row, p ^ (row & SWZ))
// (cdna_hip_programming.md §5.4 rule 21).
template <int D>
__device__ __forceinline__ void stage_chunk(char* buf, const __bf16* __restrict__ C,
                                            const float* __restrict__ chalf, int chunk,
                                            int wave, int lane) {
  using Cfg = AssignCfg<D>;
  constexpr int PIECES = kCK * Cfg::CPR;  // 16-B pieces in the chunk
  constexpr int ROUNDS = PIECES / kThreads;
  static_assert(PIECES % kThreads == 0, "chunk must tile the workgroup");
  const char* gbase = reinterpret_cast<const char*>(C) + (size_t)chunk * Cfg::CHUNK_BYTES;
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i) {
    const int base = (i * kWaves + wave) * HBMR_WAVE;
    const int p = base + lane;
    const int row = p / Cfg::CPR;
    const int cpos = p % Cfg::CPR;
    const int src = cpos ^ (row & Cfg::SWZ);
    const char* g = gbase + row * (D * 2) + src * 16;
    __builtin_amdgcn_global_load_lds((const void*)g, (void*)(buf + base * 16), 16, 0, 0);
  }
  if (wave == 0) {
    const float* g = chalf + (size_t)chunk * kCK + lane;
    __builtin_amdgcn_global_load_lds((const void*)g, (void*)(buf + Cfg::CHUNK_BYTES), 4, 0, 0);
  }
}

__device__ __forceinline__ float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Packed running arg-max of one lane over 32-row MFMA tiles (points on lanes,
// clusters on the 16 accumulator registers).  The low lb = 4 + log2(tiles)
// mantissa bits of every score are overwritten with a (tile, register) code,
// so the running maximum needs no index registers: per tile and 32-point block
// it costs 16 v_and_or_b32 + 8 v_max3_f32 into two partial maxima.  lb ≤ 12,
// i.e. ≤ 2^-12 relative perturbation — below the bf16 operand rounding (2^-8).
// v_max3_f32 goes through asm because __builtin_fmaxf canonicalises both
// operands in IEEE mode (an extra v_max_f32 x,x,x per input, which made the
// epilogue as long as the MFMA chain); the and_or stays compiler-visible so
// MFMA→VALU read hazards are still padded.
struct PackedArgMax {
  uint32_t vmask;  // VGPR copy of ~((1 << lb) - 1): VOP3 reads only one SGPR
  uint32_t top;    // (2^tb - 1) << 4
  float b0, b1;

  __device__ __forceinline__ void init(int ntiles) {
    int tb = 0;
    while ((1 << tb) < ntiles) ++tb;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmask) : "s"(~((1u << (tb + 4)) - 1u)));
    top = ((1u << tb) - 1u) << 4;
    b0 = b1 = -3.0e38f;
  }
  __device__ __forceinline__ void update(const f32x16& acc, int t) {
    const uint32_t base = top - ((uint32_t)t << 4);
    // per-register codes laundered into opaque SGPRs, else the or-constant is
    // folded into a v_and + v_or3 pair instead of one v_and_or_b32.  (The asm
    // is empty: a real s_or_b32 in it would clobber SCC under the loop branch.)
    uint32_t code[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      code[r] = base | (15u - r);
      asm("" : "+s"(code[r]));
    }
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      const float u0 = __uint_as_float((__float_as_uint(acc[r + 0]) & vmask) | code[r + 0]);
      const float u1 = __uint_as_float((__float_as_uint(acc[r + 1]) & vmask) | code[r + 1]);
      const float u2 = __uint_as_float((__float_as_uint(acc[r + 2]) & vmask) | code[r + 2]);
      const float u3 = __uint_as_float((__float_as_uint(acc[r + 3]) & vmask) | code[r + 3]);
      b0 = vmax3(b0, u0, u1);
      b1 = vmax3(b1, u2, u3);
    }
  }
  // best packed score of this lane and its cluster (lane half h)
  __device__ __forceinline__ float best() const { return fmaxf(b0, b1); }
  __device__ __forceinline__ int cluster(float bv, int h) const {
    const uint32_t code = __float_as_uint(bv) & ~vmask;
    const int tile = (int)(top >> 4) - (int)(code >> 4);
    const int r = 15 - (int)(code & 15u);
    return tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
  }
  __device__ __forceinline__ float score(float bv) const {
    return __uint_as_float(__float_as_uint(bv) & vmask);
  }
};

__device__ __forceinline__ float vmed3(float a, float b, float c) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Insert packed score u into the sorted triple b >= s >= t: t = med3(s, t, u),
// s = med3(b, s, u), b = max(b, u) (the middle of a sorted pair and u is the
// new lower member).
__device__ __forceinline__ void packed_insert3(float& b, float& s, float& t, float u) {
  t = vmed3(s, t, u);
  s = vmed3(b, s, u);
  b = vmax3(b, u, u);
}

// Packed running TOP-2 per TRACK (exact mode, hbmr.kmeans.exact): same (tile,
// register) codes as PackedArgMax.  The 16 accumulator registers of a lane
// form NT = 4 tracks (register r -> track r & 3), each keeping its best two.
// A full running top-3 (3 VALU ops per score) did not fit beside the MFMAs:
// with K = 128 one 32x32 output tile is 8 MFMAs (256 MFMA cycles per SIMD, 64
// of them blocking vector issue), and its 4 issue slots per score overran the
// remaining 192 cycles (top-3 assign ran 20 % behind the plain arg-max).
// Together with the lane half h, a cluster's track is its index bits 0-2:
// cluster = tile*32 + (r&3) + 8(r>>2) + 4h.  The top 3 of a point are the
// top 3 of the 16 track candidates; every cluster that is not a candidate
// scores <= its track's second, which is <= the third — unless the best and
// the second share a track, which finish_point flags (t = b, margin 0: step 2
// of the certification then defers the point to the neighbour scan).
// workgroups per CU the exact (top-3) assign kernels are built for: 3 keeps
// them at <= 168 VGPRs, i.e. 3 waves per SIMD like the plain arg-max kernel
constexpr int kExactMinB = 3;
struct PackedTop2x8 : PackedArgMax {
  static constexpr int NT = 4;             // register tracks per lane (r & 3)
  static constexpr uint32_t TMASK = 7u;    // cluster bits of a track
  float tb[NT], ts[NT];
  __device__ __forceinline__ void init(int ntiles) {
    PackedArgMax::init(ntiles);
#pragma unroll
    for (int i = 0; i < NT; ++i) tb[i] = ts[i] = -3.0e38f;
  }
  __device__ __forceinline__ void update(const f32x16& acc, int tt) {
    const uint32_t base = top - ((uint32_t)tt << 4);
    uint32_t code[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      code[r] = base | (15u - r);
      asm("" : "+s"(code[r]));
    }
    // registers r and r + NT belong to one track: both are inserted at once —
    // the second of {b >= s, u, v} is max(med3(b, u, v), s) — 3 VALU ops per
    // two scores instead of 4 (the epilogue is what bounds this kernel)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if ((r / NT) % 2) continue;
      const float u = __uint_as_float((__float_as_uint(acc[r]) & vmask) | code[r]);
      const float v = __uint_as_float((__float_as_uint(acc[r + NT]) & vmask) | code[r + NT]);
      const float m = vmed3(tb[r % NT], u, v);
      ts[r % NT] = vmax3(m, ts[r % NT], ts[r % NT]);
      tb[r % NT] = vmax3(tb[r % NT], u, v);
    }
  }
  __device__ __forceinline__ void top3(float& b, float& s, float& t) const {
    b = s = t = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      packed_insert3(b, s, t, tb[i]);
      packed_insert3(b, s, t, ts[i]);
    }
  }
};

template <bool EXACT>
using ArgMaxT = typename std::conditional<EXACT, PackedTop2x8, PackedArgMax>::type;

// (score, cluster) insertion into a sorted triple; ties to the lower cluster
__device__ __forceinline__ void insert3(float (&v)[3], int (&c)[3], float u, int cu) {
  auto gt = [](float a, int ca, float b, int cb) { return a > b || (a == b && ca < cb); };
  if (gt(u, cu, v[2], c[2])) {
    v[2] = u; c[2] = cu;
    if (gt(v[2], c[2], v[1], c[1])) {
      float tv = v[1]; v[1] = v[2]; v[2] = tv;
      int tc = c[1]; c[1] = c[2]; c[2] = tc;
      if (gt(v[1], c[1], v[0], c[0])) {
        tv = v[0]; v[0] = v[1]; v[1] = tv;
        tc = c[0]; c[0] = c[1]; c[1] = tc;
      }
    }
  }
}

// Finish one point: lane-local arg-max (exact mode: top 3), then across the
// two lane halves (each half saw a different set of cluster rows).  Exact mode
// writes the runner-ups cand[p], cand[n+p] and the score margins best-second,
// best-third (masked scores) to margin[p], margin[n+p].
template <bool EXACT, class AM>
__device__ __forceinline__ void finish_point(const AM& am, int h, long p, long n,
                                             int32_t* __restrict__ labels,
                                             int32_t* __restrict__ cand,
                                             float* __restrict__ scores,
                                             float* __restrict__ margin, long cs = -1) {
  // cs: stride of the second candidate / margin (n for one split; the batch
  // size when a grouped launch writes a batch's arrays)
  if (cs < 0) cs = n;
  if constexpr (!EXACT) {
    float bv = am.best();
    int cluster = am.cluster(bv, h);
    const float ov = __shfl_xor(bv, 32);
    const int oc = __shfl_xor(cluster, 32);
    if (ov > bv || (ov == bv && oc < cluster)) { bv = ov; cluster = oc; }
    if (h == 0 && p < n) {
      labels[p] = cluster;
      if (scores) scores[p] = am.score(bv);
    }
  } else {
    float v[3];
    int c[3];
    am.top3(v[0], v[1], v[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = am.cluster(v[i], h);
    float ov[3];
    int oc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ov[i] = __shfl_xor(v[i], 32);
      oc[i] = __shfl_xor(c[i], 32);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) insert3(v, c, ov[i], oc[i]);
    // best and second in one track: the rest is bounded only by the second
    if (((c[0] ^ c[1]) & AM::TMASK) == 0) {
      v[2] = v[0];
      c[2] = c[0];
    }
    if (h == 0 && p < n) {
      labels[p] = c[0];
      cand[p] = c[1];
      cand[cs + p] = c[2];
      const float bs = am.score(v[0]);
      scores[p] = bs;
      margin[p] = bs - am.score(v[1]);
      margin[cs + p] = bs - am.score(v[2]);
    }
  }
}

// v1, the chunked form (launched at D = 256 only; D <= 128 takes v2 below):
// one workgroup's tile of points [blk*PTS, (blk+1)*PTS) of one split.
template <int D, bool EXACT = false, bool F16 = false>
__device__ __forceinline__ void assign_tile(const __bf16* __restrict__ X, long n,
                                            const __bf16* __restrict__ C,
                                            const float* __restrict__ chalf, int nchunks,
                                            int32_t* __restrict__ labels,
                                            float* __restrict__ scores, long blk, char* smem,
                                            int32_t* __restrict__ cand = nullptr,
                                            float* __restrict__ margin = nullptr) {
  using Cfg = AssignCfg<D>;
  constexpr int KS = Cfg::KS, PB = Cfg::PB;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / HBMR_WAVE);
  const int lane = tid & (HBMR_WAVE - 1);
  const int h = lane >> 5;   // lane half: selects k-offset 8h in A/B fragments
  const int col = lane & 31;
  const long p0 = blk * Cfg::PTS + (long)wave * PB * 32;

  // Kick off chunk 0 first so it overlaps the point-fragment loads.
  stage_chunk<D>(smem, C, chalf, 0, wave, lane);

  // B operand = points: lane holds X[p][16s + 8h .. +7] for its column p.
  bf16x8 bfrag[PB][KS];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    long p = p0 + pb * 32 + col;
    if (p >= n) p = n - 1;
    const uint4* row = reinterpret_cast<const uint4*>(X + p * D);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 v = row[2 * s + h];
      bfrag[pb][s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  ArgMaxT<EXACT> am[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) am[pb].init(nchunks * (kCK / 32));

  // Retire the fragment loads here and launder the registers through an asm
  // so hipcc's waitcnt pass does not see them as pending inside the chunk loop
  // (it would otherwise emit vmcnt(0) at the first MFMA and drain the next
  // chunk's global_load_lds prefetch every iteration).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(bfrag[pb][s]));
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    char* cur = smem + (c & 1) * Cfg::BUF_BYTES;
    if (c + 1 < nchunks)
      stage_chunk<D>(smem + ((c + 1) & 1) * Cfg::BUF_BYTES, C, chalf, c + 1, wave, lane);
    const float* ch = reinterpret_cast<const float*>(cur + Cfg::CHUNK_BYTES);
#pragma unroll
    for (int cb = 0; cb < kCK / 32; ++cb) {
      f32x16 acc[PB];
      // Initial accumulator = -||c||²/2 of the cluster on this register's row:
      // row(reg, lane) = (reg & 3) + 8 * (reg >> 2) + 4 * h.
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ch + cb * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
          acc[pb][4 * g + 0] = v[0];
          acc[pb][4 * g + 1] = v[1];
          acc[pb][4 * g + 2] = v[2];
          acc[pb][4 * g + 3] = v[3];
        }
      }
      const int arow = cb * 32 + col;
      const char* abase = cur + arow * (D * 2);
      const int aswz = arow & Cfg::SWZ;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int q = 2 * s + h;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(abase + ((q ^ aswz) << 4));
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
          acc[pb] = mfma32x32x16<F16>(a, bfrag[pb][s], acc[pb]);
      }
#pragma unroll
      for (int pb = 0; pb < PB; ++pb) am[pb].update(acc[pb], c * (kCK / 32) + cb);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
    finish_point<EXACT>(am[pb], h, p0 + pb * 32 + col, n, labels, cand, scores, margin);
}

// ---------------------------------------------------------------------------
// v2: software-pipelined variant for D ≤ 128 (PB = 2).
// The centroid stream advances in 32-cluster tiles through an NS-deep LDS
// ring; the A fragments (and -|c|²/2) of tile t+1 are read into registers
// while tile t's 16 MFMAs run, so the MFMA chain never waits on an LDS read,
// and there is ONE barrier per tile:
//   wait own DMA(t+1) + lgkmcnt(0) → barrier → DMA(t+NS) into tile t's slot
//   (its LDS→register reads retired by the lgkmcnt) → ds_read tile t+1 →
//   MFMAs + arg-max epilogue of tile t.
// A DMA thus has NS-1 tiles (≈(NS-1)·512 MFMA cycles) to land: with NS = 2 the
// L2 latency under full-chip load was exposed every tile.
// waves per v2 workgroup sharing one centroid stream; 8 (2 per SIMD, half the
// L2→LDS traffic per FLOP) measured 16–19 % slower than 4 at 100M×1024×128
// (profiles/kmeans_assign_tuning.md)
constexpr int kV2Waves = 4;
constexpr int kV2PB = 2;  // 32-point blocks per wave in every v2 launch

template <int D, int NSV = 4> struct AssignV2 {
  static constexpr int KS = D / 16;
  static constexpr int NS = NSV;                         // ring depth
  static constexpr int TILE_BYTES = 32 * D * 2;          // 32 clusters
  static constexpr int BUF = TILE_BYTES + 32 * 4;        // + -|c|²/2
  static constexpr int LDS_BYTES = NS * BUF;
  static constexpr int PIECES = 32 * (D / 8);            // 16-B pieces per tile
  static constexpr int WAVES = kV2Waves;
  static constexpr int THREADS = WAVES * HBMR_WAVE;
  static constexpr int MINB = 2;                         // → ≤ 256 VGPRs
  static constexpr int P = PIECES / THREADS;             // DMAs per lane per tile
  static constexpr int PTS = WAVES * kV2PB * 32;         // points per workgroup
  static_assert(PIECES % THREADS == 0, "a tile's pieces must tile the workgroup");
};

template <int N> __device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Wait until at most `y` tile-DMAs of this wave are outstanding (wave 0 issues
// one extra DMA per tile for -|c|²/2).  y is wave-uniform, ≤ Y.
template <int P, int Y>
__device__ __forceinline__ void wait_tile_dmas(int y, bool w0) {
  if constexpr (Y > 0) {
    if (y == Y) {
      if (w0) vm_wait<Y * (P + 1)>(); else vm_wait<Y * P>();
      return;
    }
    wait_tile_dmas<P, Y - 1>(y, w0);
  } else {
    vm_wait<0>();
  }
}

template <int D>
__device__ __forceinline__ void stage_tile32(char* buf, const __bf16* __restrict__ C,
                                             const float* __restrict__ chalf, int tile, int wave,
                                             int lane) {
  using V = AssignV2<D>;
  constexpr int CPR = D / 8;
  constexpr int SWZ = AssignCfg<D>::SWZ;
  const char* gbase = reinterpret_cast<const char*>(C) + (size_t)tile * V::TILE_BYTES;
#pragma unroll
  for (int i = 0; i < V::P; ++i) {
    const int base = (i * V::WAVES + wave) * HBMR_WAVE;
    const int p = base + lane;
    const int row = p / CPR, cpos = p % CPR;
    const char* g = gbase + row * (D * 2) + ((cpos ^ (row & SWZ)) * 16);
    __builtin_amdgcn_global_load_lds((const void*)g, (void*)(buf + base * 16), 16, 0, 0);
  }
  if (wave == 0 && lane < 32) {
    const float* g = chalf + (size_t)tile * 32 + lane;
    __builtin_amdgcn_global_load_lds((const void*)g, (void*)(buf + V::TILE_BYTES), 4, 0, 0);
  }
}

// -|c|²/2 of the tile in tile_buf (behind its TILE_BYTES of rows) into `bias`, the
// MFMA's initial accumulator: this lane's rows 8g + 4h .. 8g + 4h + 3, g = 0..3
template <int D>
__device__ __forceinline__ void load_bias(const char* tile_buf, int h, f32x16& bias) {
  const float* ch = reinterpret_cast<const float*>(tile_buf + AssignV2<D>::TILE_BYTES);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(ch + 8 * g + 4 * h);
    bias[4 * g + 0] = v[0];
    bias[4 * g + 1] = v[1];
    bias[4 * g + 2] = v[2];
    bias[4 * g + 3] = v[3];
  }
}

template <int D>
__device__ __forceinline__ void read_tile32(const char* buf, int col, int h, bf16x8 (&a)[D / 16],
                                            f32x16& bias) {
  constexpr int SWZ = AssignCfg<D>::SWZ;
  const char* abase = buf + col * (D * 2);
  const int aswz = col & SWZ;
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    a[s] = *reinterpret_cast<const bf16x8*>(abase + (((2 * s + h) ^ aswz) << 4));
  load_bias<D>(buf, h, bias);
}

struct NoFin {};   // assign_tile_v2's default finish (finish_point)

// the fused exact kernel: 3 = v3 (default), 2 = v2 (HBMR_EXACT_V3=v2, read once;
// hbmr_kmeans_set_exact_kernel overrides it in-process)
int g_exact_kernel = -1;
inline int exact_kernel() {
  static const int env = [] {
    const char* e = getenv("HBMR_EXACT_V3");
    return e && strcmp(e, "v2") == 0 ? 2 : 3;
  }();
  return g_exact_kernel > 0 ? g_exact_kernel : env;
}

template <int D, int PB, bool EXACT = false, bool F16 = false, class Fin = NoFin>
__device__ __forceinline__ void assign_tile_v2(const __bf16* __restrict__ X, long n,
                                               const __bf16* __restrict__ C,
                                               const float* __restrict__ chalf, int ntiles,
                                               int32_t* __restrict__ labels,
                                               float* __restrict__ scores, long blk, char* smem,
                                               int32_t* __restrict__ cand = nullptr,
                                               float* __restrict__ margin = nullptr,
                                               long cs = -1, const Fin* fin = nullptr) {
  static_assert(D <= 128, "v2 keeps PB point blocks of D ≤ 128 in registers");
  using V = AssignV2<D>;
  constexpr int KS = V::KS;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / HBMR_WAVE);
  const int lane = tid & (HBMR_WAVE - 1);
  const int h = lane >> 5;
  const int col = lane & 31;
  const long p0 = blk * (V::WAVES * PB * 32) + (long)wave * PB * 32;

#pragma unroll
  for (int i = 0; i < V::NS; ++i)
    if (i < ntiles) stage_tile32<D>(smem + i * V::BUF, C, chalf, i, wave, lane);

  bf16x8 bfrag[PB][KS];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    long p = p0 + pb * 32 + col;
    if (p >= n) p = n - 1;
    const uint4* row = reinterpret_cast<const uint4*>(X + p * D);
#pragma unroll
    for (int s = 0; s < KS; ++s) bfrag[pb][s] = __builtin_bit_cast(bf16x8, row[2 * s + h]);
  }
  ArgMaxT<EXACT> am[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) am[pb].init(ntiles);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(bfrag[pb][s]));
  __syncthreads();

  // Rolling register prefetch: right after the two MFMAs that consume k-step s
  // of tile t, fragment s of tile t+1 is read into the same registers, so each
  // LDS read has the rest of the tile's MFMAs to land and only one register
  // set of A (and of -|c|²/2) is live.
  bf16x8 a[KS];
  f32x16 bias;
  read_tile32<D>(smem, col, h, a, bias);
  constexpr int SWZ = AssignCfg<D>::SWZ;
  const int aswz = col & SWZ;

  const bool w0 = wave == 0;
  int slot = 0;  // t % NS
  for (int t = 0; t < ntiles; ++t) {
    // tile t+1's DMA has landed for every wave (younger DMAs in flight: tiles
    // t+2 .. min(t+NS-1, ntiles-1)), and this wave's reads of tile t have
    // retired → tile t's slot is free
    wait_tile_dmas<V::P, V::NS - 2>(max(0, min(V::NS - 2, ntiles - 2 - t)), w0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + V::NS < ntiles) stage_tile32<D>(smem + slot * V::BUF, C, chalf, t + V::NS, wave, lane);
    slot = slot + 1 == V::NS ? 0 : slot + 1;
    // (past the last tile the reads hit a stale slot: harmless and branch-free)
    const char* nbuf = smem + slot * V::BUF;
    const char* nrow = nbuf + col * (D * 2);
    f32x16 acc[PB];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
        acc[pb] = mfma32x32x16<F16>(a[s], bfrag[pb][s], s == 0 ? bias : acc[pb]);
      a[s] = *reinterpret_cast<const bf16x8*>(nrow + (((2 * s + h) ^ aswz) << 4));
    }
    load_bias<D>(nbuf, h, bias);
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) am[pb].update(acc[pb], t);
  }

  if constexpr (!std::is_same<Fin, NoFin>::value) {
    (*fin)(am, h, p0, col, n, labels);        // e.g. the fused step-1 certification
  } else {
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
      finish_point<EXACT>(am[pb], h, p0 + pb * 32 + col, n, labels, cand, scores, margin, cs);
  }
}

template <int D>
__global__ __launch_bounds__(kThreads, 2) void kmeans_assign_kernel(
    const __bf16* __restrict__ X, long n, const __bf16* __restrict__ C,
    const float* __restrict__ chalf, int nchunks, int32_t* __restrict__ labels,
    float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  assign_tile<D>(X, n, C, chalf, nchunks, labels, scores,
                 hbmr_xcd_remap(blockIdx.x, gridDim.x), smem);
}

template <int D, int PB>
__global__ __launch_bounds__(AssignV2<D>::THREADS, AssignV2<D>::MINB) void kmeans_assign_v2_kernel(
    const __bf16* __restrict__ X, long n, const __bf16* __restrict__ C,
    const float* __restrict__ chalf, int ntiles, int32_t* __restrict__ labels,
    float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  assign_tile_v2<D, PB>(X, n, C, chalf, ntiles, labels, scores,
                    hbmr_xcd_remap(blockIdx.x, gridDim.x), smem);
}

// Exact mode: the same kernels with the top-3 epilogue (bf16 or fp16 operands;
// the 16-bit rows travel as bf16 bit patterns either way).
template <int D, bool F16>
__global__ __launch_bounds__(kThreads, 2) void kmeans_assign_top3_kernel(
    const __bf16* __restrict__ X, long n, const __bf16* __restrict__ C,
    const float* __restrict__ chalf, int nchunks, int32_t* __restrict__ labels,
    int32_t* __restrict__ cand, float* __restrict__ scores, float* __restrict__ margin) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  assign_tile<D, true, F16>(X, n, C, chalf, nchunks, labels, scores,
                            hbmr_xcd_remap(blockIdx.x, gridDim.x), smem, cand, margin);
}

template <int D, int PB, bool F16>
__global__ __launch_bounds__(AssignV2<D>::THREADS, kExactMinB) void kmeans_assign_top3_v2_kernel(
    const __bf16* __restrict__ X, long n, const __bf16* __restrict__ C,
    const float* __restrict__ chalf, int ntiles, int32_t* __restrict__ labels,
    int32_t* __restrict__ cand, float* __restrict__ scores, float* __restrict__ margin) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  assign_tile_v2<D, PB, true, F16>(X, n, C, chalf, ntiles, labels, scores,
                                   hbmr_xcd_remap(blockIdx.x, gridDim.x), smem, cand, margin);
}

// points per workgroup of the assign kernel launch_*assign picks: the
// pipelined v2 for D ≤ 128, the chunked v1 for D = 256
template <int D> constexpr int assign_pts() {
  if constexpr (D <= 128) return AssignV2<D>::PTS;
  else return AssignCfg<D>::PTS;
}

}  // namespace
