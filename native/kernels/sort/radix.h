#pragma once
// LSD radix sorts of uint64 keys, 8-bit digits, stable (so multi-word keys sort
// by successive passes, least-significant word first).
// * (key, uint32 value) pairs.  Per pass: (1) per-tile digit histograms, (2)
//   one workgroup per digit scans its column of tile counts, (3) a stable
//   scatter: each 64-lane wave ranks its keys with 8 ballots (multi-split),
//   the tile is regrouped by digit in LDS and written out in digit runs.
// * keys only: onesweep, below.
// The tile constants here also size the TeraSort partition scatter.
#include "../common.h"

namespace {

constexpr int kSortThreads = 256;
constexpr int kSortItems = 16;
constexpr int kSortTile = kSortThreads * kSortItems;  // 4096 keys per workgroup
constexpr int kRadix = 256;
constexpr int kSortWaves = kSortThreads / HBMR_WAVE;

__device__ __forceinline__ uint32_t digit_of(uint64_t k, int shift) {
  return (uint32_t)(k >> shift) & 0xFFu;
}

// Block-wide exclusive scan of one value per thread (256 threads).
__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t x, uint32_t* s_w) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t v = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < w; ++i) base += s_w[i];
  __syncthreads();
  return base + v - x;
}

// (2) one workgroup per digit: exclusive scan over tiles in place, column total
__global__ __launch_bounds__(1024) void radix_scan_kernel(uint32_t* __restrict__ hist, long ntiles,
                                                          uint32_t* __restrict__ totals) {
  __shared__ uint32_t s_w[16];
  __shared__ uint32_t s_carry;
  uint32_t* h = hist + (long)blockIdx.x * ntiles;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (long c = 0; c < ntiles; c += 4096) {
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long idx = c + (long)t * 4 + j;
      v[j] = idx < ntiles ? h[idx] : 0u;
      sum += v[j];
    }
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(x, o);
      if (lane >= o) x += u;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t wbase = s_carry;
    for (int i = 0; i < w; ++i) wbase += s_w[i];
    uint32_t run = wbase + x - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long idx = c + (long)t * 4 + j;
      if (idx < ntiles) h[idx] = run;
      run += v[j];
    }
    __syncthreads();
    if (t == 1023) s_carry = run;
    __syncthreads();
  }
  if (t == 0) totals[blockIdx.x] = s_carry;
}

// (3') stable scatter with wave-private ranking.  Each wave owns a contiguous
// 1024-key quarter of the tile (loads stay 512 B per wave instruction), ranks
// its keys among equal digits with 8 ballots and a wave-private LDS counter per
// digit — no workgroup barrier inside the per-key loop (radix_scatter_kernel
// takes three per key) — then one digit-major scan over the 4 waves' counts
// places every key.  Order (wave, item, lane) is index order, so stable.
__global__ __launch_bounds__(kSortThreads) void radix_scatter_v2_kernel(
    const uint64_t* __restrict__ kin, const uint32_t* __restrict__ vin, uint64_t* __restrict__ kout,
    uint32_t* __restrict__ vout, long n, int shift, long ntiles, const uint32_t* __restrict__ hist,
    const uint32_t* __restrict__ totals) {
  __shared__ uint64_t s_k[kSortTile];
  __shared__ uint32_t s_v[kSortTile];
  __shared__ uint32_t s_wh[kSortWaves][kRadix];  // per-wave digit counts, then wave offsets
  __shared__ uint32_t s_toff[kRadix];
  __shared__ uint32_t s_gbase[kRadix];
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long tile = blockIdx.x;
  const long base = tile * kSortTile;
  const int tile_n = (int)min((long)kSortTile, n - base);
  constexpr int kWaveSpan = kSortTile / kSortWaves;  // 1024 keys per wave

#pragma unroll
  for (int i = 0; i < kSortWaves; ++i) s_wh[i][t] = 0u;
  uint64_t k[kSortItems];
  uint32_t v[kSortItems];
  const long wbase = base + (long)w * kWaveSpan;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const long e = wbase + i * HBMR_WAVE + lane;
    if (e < n) {
      k[i] = kin[e];
      v[i] = vin ? vin[e] : (uint32_t)e;
    }
  }
  __syncthreads();
  const uint64_t lt = __lanemask_lt();
  uint32_t rank[kSortItems];
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const bool valid = w * kWaveSpan + i * HBMR_WAVE + lane < tile_n;
    const uint32_t d = valid ? digit_of(k[i], shift) : 0u;
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1u);
      m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t pre = __popcll(m & lt);
    uint32_t old = 0u;
    if (valid) old = s_wh[w][d];
    __builtin_amdgcn_wave_barrier();
    rank[i] = old + pre;
    if (valid && pre == 0) s_wh[w][d] = old + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // thread t = digit t: tile offset of the digit, each wave's offset within it,
  // and the digit's global start for this tile
  {
    uint32_t c[kSortWaves], cnt = 0;
#pragma unroll
    for (int i = 0; i < kSortWaves; ++i) {
      c[i] = s_wh[i][t];
      cnt += c[i];
    }
    const uint32_t gb = block_excl_scan256(totals[t], s_w);
    s_gbase[t] = gb + hist[(long)t * ntiles + tile];
    const uint32_t toff = block_excl_scan256(cnt, s_w);
    s_toff[t] = toff;
    uint32_t run = toff;
#pragma unroll
    for (int i = 0; i < kSortWaves; ++i) {
      s_wh[i][t] = run;
      run += c[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    if (w * kWaveSpan + i * HBMR_WAVE + lane < tile_n) {
      const uint32_t local = s_wh[w][digit_of(k[i], shift)] + rank[i];
      s_k[local] = k[i];
      s_v[local] = v[i];
    }
  }
  __syncthreads();
  for (int j = t; j < tile_n; j += kSortThreads) {
    const uint64_t key = s_k[j];
    const uint32_t d = digit_of(key, shift);
    const long dst = (long)s_gbase[d] + (j - (long)s_toff[d]);
    kout[dst] = key;
    vout[dst] = s_v[j];
  }
}

// (1') digit histogram per tile with one LDS add per (wave, digit) group:
// 8 ballots find the lanes sharing a digit and its leader adds their count
// (radix_hist_kernel issues one contended LDS atomic per key)
__global__ __launch_bounds__(kSortThreads) void radix_hist_v2_kernel(const uint64_t* __restrict__ keys,
                                                                     long n, int shift, long ntiles,
                                                                     uint32_t* __restrict__ hist) {
  __shared__ uint32_t s[kSortWaves][kRadix];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int i = 0; i < kSortWaves; ++i) s[i][t] = 0u;
  __syncthreads();
  constexpr int kWaveSpan = kSortTile / kSortWaves;
  const long wbase = (long)blockIdx.x * kSortTile + (long)w * kWaveSpan;
  const uint64_t lt = __lanemask_lt();
  uint64_t k[kSortItems];
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const long e = wbase + i * HBMR_WAVE + lane;
    k[i] = e < n ? keys[e] : 0ull;
  }
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const bool valid = wbase + i * HBMR_WAVE + lane < n;
    const uint32_t d = digit_of(k[i], shift);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1u);
      m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    if (valid && __popcll(m & lt) == 0) s[w][d] += (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  hist[(long)t * ntiles + blockIdx.x] = s[0][t] + s[1][t] + s[2][t] + s[3][t];
}

// ---------------------------------------------------------------- onesweep (keys only)
// LSD radix sort of uint64 keys by bits [begin, begin + 8·passes) with ONE read
// of the keys for every digit's histogram and one scatter pass per digit whose
// tile offsets come from a decoupled look-back instead of a per-pass
// histogram + scan (radix_hist_v2 + radix_scan: one more read of the keys and
// two more launches per pass).  Tiles take their index from an atomic ticket,
// so every tile a tile waits on was scheduled before it.  Status words per
// (tile, digit), 64-bit: bits 63-48 the pass's epoch, 47-46 the kind (0
// empty, 1 aggregate = this tile's count, 2 inclusive prefix through this
// tile), 31-0 the value.  A word from another epoch reads as empty, so the
// status array is zeroed once when allocated, not before every pass.
// A look-back that sees nothing for kSpinLimit polls sets *err and moves on
// (the output is then wrong and the caller's order check sees it): every wave
// reaches the kernel's end.
constexpr uint64_t kStAgg = 1ull << 46, kStInc = 2ull << 46, kStKind = 3ull << 46;
constexpr int kSpinLimit = 1 << 22;
constexpr int kMaxPasses = 8;

__global__ __launch_bounds__(kSortThreads) void radix_hist_all_kernel(
    const uint64_t* __restrict__ keys, long n, int begin, int end, int passes,
    uint32_t* __restrict__ ghist) {
  __shared__ uint32_t s[kMaxPasses][kRadix];
  const int t = threadIdx.x;
  for (int p = 0; p < passes; ++p) s[p][t] = 0u;
  __syncthreads();
  for (long base = (long)blockIdx.x * kSortTile; base < n; base += (long)gridDim.x * kSortTile) {
#pragma unroll 4
    for (int i = 0; i < kSortItems; ++i) {
      const long e = base + (long)i * kSortThreads + t;
      if (e < n) {
        const uint64_t k = keys[e];
        for (int p = 0; p < passes; ++p) {
          const int sh = begin + 8 * p;
          atomicAdd(&s[p][(uint32_t)(k >> sh) & ((1u << min(8, end - sh)) - 1u)], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int p = 0; p < passes; ++p)
    if (s[p][t]) atomicAdd(&ghist[p * kRadix + t], s[p][t]);
}

// one workgroup per pass: exclusive scan of the digit counts in place
__global__ __launch_bounds__(kSortThreads) void radix_bases_kernel(uint32_t* __restrict__ ghist) {
  __shared__ uint32_t s_w[4];
  uint32_t* h = ghist + blockIdx.x * kRadix;
  const uint32_t x = h[threadIdx.x];
  const uint32_t e = block_excl_scan256(x, s_w);
  h[threadIdx.x] = e;
}

// WAVES waves of 64 lanes, 16 keys per lane: a tile of WAVES·1024 keys.  More
// keys per tile make longer digit runs for the scatter's writes (8 waves:
// 32 keys = 256 B per digit on average) and fewer look-backs.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void radix_onesweep_kernel(
    const uint64_t* __restrict__ kin, uint64_t* __restrict__ kout, long n, int shift,
    uint32_t dmask, const uint32_t* __restrict__ gbase, uint64_t* __restrict__ status,
    uint64_t epoch, uint32_t* __restrict__ ticket, uint32_t* __restrict__ err) {
  constexpr int kThreads = WAVES * 64;
  constexpr int kTile = kThreads * kSortItems;
  constexpr int kWaveSpan = kSortItems * 64;
  static_assert(WAVES >= 4, "one thread per digit");
  __shared__ uint64_t s_k[kTile];
  __shared__ uint32_t s_wh[WAVES][kRadix];
  __shared__ uint32_t s_cnt[kRadix];
  __shared__ uint32_t s_toff[kRadix];
  __shared__ uint32_t s_g[kRadix];
  __shared__ uint32_t s_tile;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) s_tile = atomicAdd(ticket, 1u);
  for (int i = t; i < WAVES * kRadix; i += kThreads) (&s_wh[0][0])[i] = 0u;
  __syncthreads();
  const long tile = s_tile;
  const long base = tile * kTile;
  const int tile_n = (int)min((long)kTile, n - base);
  uint64_t k[kSortItems];
  const long wbase = base + (long)w * kWaveSpan;
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const long e = wbase + i * HBMR_WAVE + lane;
    k[i] = e < n ? kin[e] : 0ull;
  }
  const uint64_t lt = __lanemask_lt();
  uint32_t rank[kSortItems];
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const bool valid = w * kWaveSpan + i * HBMR_WAVE + lane < tile_n;
    const uint32_t d = valid ? ((uint32_t)(k[i] >> shift) & dmask) : 0u;
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1u);
      m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t pre = __popcll(m & lt);
    uint32_t old = 0u;
    if (valid) old = s_wh[w][d];
    __builtin_amdgcn_wave_barrier();
    rank[i] = old + pre;
    if (valid && pre == 0) s_wh[w][d] = old + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (t < kRadix) {
    // thread t = digit t: publish the tile's count, look back for its prefix
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) cnt += s_wh[i][t];
    uint64_t* st = status + tile * kRadix + t;
    const uint64_t ep = epoch << 48;
    uint32_t excl = 0;
    if (tile == 0) {
      __hip_atomic_store(st, ep | kStInc | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __hip_atomic_store(st, ep | kStAgg | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (long p = tile - 1; p >= 0; --p) {
        const uint64_t* q = status + p * kRadix + t;
        uint64_t v = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (((v >> 48) != epoch || (v & kStKind) == 0u) && ++spins < kSpinLimit) {
          __builtin_amdgcn_s_sleep(1);
          v = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if ((v >> 48) != epoch || (v & kStKind) == 0u) {
          atomicOr(err, 1u);
          break;
        }
        excl += (uint32_t)v;
        if ((v & kStKind) == kStInc) break;
      }
      __hip_atomic_store(st, ep | kStInc | (excl + cnt), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    s_g[t] = gbase[t] + excl;
    s_cnt[t] = cnt;
  }
  __syncthreads();
  if (w == 0) {
    // the tile's digit offsets: exclusive scan of 256 counts, 4 per lane
    const uint32_t a0 = s_cnt[4 * lane], a1 = s_cnt[4 * lane + 1], a2 = s_cnt[4 * lane + 2],
                   a3 = s_cnt[4 * lane + 3];
    const uint32_t sum = a0 + a1 + a2 + a3;
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(x, o);
      if (lane >= o) x += u;
    }
    const uint32_t e0 = x - sum;
    s_toff[4 * lane] = e0;
    s_toff[4 * lane + 1] = e0 + a0;
    s_toff[4 * lane + 2] = e0 + a0 + a1;
    s_toff[4 * lane + 3] = e0 + a0 + a1 + a2;
  }
  __syncthreads();
  if (t < kRadix) {
    // each wave's start inside the digit's run
    uint32_t run = s_toff[t];
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
      const uint32_t c = s_wh[i][t];
      s_wh[i][t] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    if (w * kWaveSpan + i * HBMR_WAVE + lane < tile_n)
      s_k[s_wh[w][((uint32_t)(k[i] >> shift) & dmask)] + rank[i]] = k[i];
  }
  __syncthreads();
  for (int j = t; j < tile_n; j += kThreads) {
    const uint64_t key = s_k[j];
    const uint32_t d = ((uint32_t)(key >> shift) & dmask);
    kout[(long)s_g[d] + (j - (long)s_toff[d])] = key;
  }
}

}  // namespace
