#pragma once
// TeraSort reduce side, before the sort: collect the pieces every map produced
// (plain, shuffle slots, packed record ids); after it: the order check and
// the per-group statistics, with the fold of per-block partial pairs.
#include "../common.h"
#include "partition.h"

namespace {

__global__ __launch_bounds__(256) void check_sorted_kernel(const uint64_t* __restrict__ hi,
                                                           const uint64_t* __restrict__ lo, long n,
                                                           unsigned long long* __restrict__ bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x + 1;
  bool b = false;
  if (i < n) b = hi[i - 1] > hi[i] || (hi[i - 1] == hi[i] && lo[i - 1] > lo[i]);
  const uint64_t m = __ballot(b);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(bad, (unsigned long long)__popcll(m));
}

// One group of the one-rank reduce, after its sort: acc[0] += the records out
// of order (against the previous record; record 0 against the previous
// group's last key *ph / *pl when given), acc[1] += sum(hi + lo) mod 2^64 (the
// order-independent key checksum) — one pass, one atomic per wave, in place
// of an order check, two reductions and the elementwise seam check.
__global__ __launch_bounds__(256) void tera_group_stats_kernel(
    const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, long n,
    const uint64_t* __restrict__ ph, const uint64_t* __restrict__ pl,
    unsigned long long* __restrict__ parts) {
  __shared__ unsigned long long s[2][4];
  uint64_t sum = 0, bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const uint64_t h = hi[i], l = lo[i];
    sum += h + l;
    if (i > 0) {
      const uint64_t h0 = hi[i - 1], l0 = lo[i - 1];
      bad += h0 > h || (h0 == h && l0 > l);
    } else if (ph != nullptr) {
      bad += *ph > h || (*ph == h && *pl > l);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    bad += __shfl_xor(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = bad;
    s[1][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    parts[2 * blockIdx.x] = s[0][0] + s[0][1] + s[0][2] + s[0][3];
    parts[2 * blockIdx.x + 1] = s[1][0] + s[1][1] + s[1][2] + s[1][3];
  }
}

// one workgroup: out[0] (|= or +=, by or0) and out[1] += over nparts pairs
__global__ __launch_bounds__(256) void reduce_pairs_kernel(const unsigned long long* __restrict__ parts,
                                                           long nparts, int or0,
                                                           unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s[2][4];
  unsigned long long a = 0, b = 0;
  for (long i = threadIdx.x; i < nparts; i += 256) {
    a = or0 ? (a | parts[2 * i]) : a + parts[2 * i];
    b += parts[2 * i + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(a, o);
    a = or0 ? (a | x) : a + x;
    b += __shfl_xor(b, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = a;
    s[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long x = out[0], y = out[1];
    for (int w = 0; w < 4; ++w) {
      x = or0 ? (x | s[0][w]) : x + s[0][w];
      y += s[1][w];
    }
    out[0] = x;
    out[1] = y;
  }
}

// Concatenate S pieces: piece s is [starts[s], starts[s] + len_s) of its split's
// (hi, lo, row) arrays, placed at [prefix[s], prefix[s+1]) of the output; the
// output also records which split each element came from.  hi/lo (in and out)
// may be null (records-only collection for the shuffle).
__global__ __launch_bounds__(256) void tera_collect_kernel(
    const uint64_t* const* __restrict__ his, const uint64_t* const* __restrict__ los,
    const uint32_t* const* __restrict__ rows, const long* __restrict__ starts,
    const long* __restrict__ prefix, int S, long n, uint64_t* __restrict__ ohi,
    uint64_t* __restrict__ olo, uint32_t* __restrict__ osplit, uint32_t* __restrict__ orow) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    int a = 0, b = S;          // largest s with prefix[s] <= i
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (prefix[m] <= i) a = m; else b = m;
    }
    const long j = starts[a] + (i - prefix[a]);
    if (ohi) ohi[i] = his[a][j];
    if (olo) olo[i] = los[a][j];
    osplit[i] = (uint32_t)a;
    orow[i] = rows[a][j];
  }
}

// Static-shape shuffle send layout (the TeraSort shuffle waves): W destination
// slots of C entries.  Entry j of slot d is element j of destination d's pieces
// — piece s is [starts[s*W + d], +len) of split s's partition-ordered rows,
// placed at [pre[d*(S+1) + s], pre[d*(S+1) + s + 1]) — while j < min(pre[d*(S+1)
// + S], C); entries past the count get split = kNoSplit (the gather skips them).
// Every offset is read on the device: no host round trip between the maps'
// partition offsets and the all-to-all that sends the slots.
constexpr uint32_t kNoSplit = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void tera_collect_slots_kernel(
    const uint32_t* const* __restrict__ rows, const long* __restrict__ starts,
    const long* __restrict__ pre, int S, int W, long C, uint32_t* __restrict__ osplit,
    uint32_t* __restrict__ orow) {
  const long n = (long)W * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int d = (int)(i / C);
    const long j = i - (long)d * C;
    const long* pd = pre + (long)d * (S + 1);
    if (j >= pd[S]) {
      osplit[i] = kNoSplit;
      orow[i] = 0u;
      continue;
    }
    int a = 0, b = S;          // largest s with pd[s] <= j
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (pd[m] <= j) a = m; else b = m;
    }
    osplit[i] = (uint32_t)a;
    orow[i] = rows[a][starts[(long)a * W + d] + (j - pd[a])];
  }
}

// ---- TeraSort reduce v4: packed record ids ------------------------------------
// A group's records are named by a 32-bit gid = split << 24 | row (splits < 256,
// rows < 2^24): the key sort carries the gid itself, so the record gather makes
// ONE dependent index load per record (v3: perm, then split and row).
__global__ __launch_bounds__(256) void tera_collect_gid_kernel(
    const uint64_t* const* __restrict__ his, const uint32_t* const* __restrict__ rows,
    const long* __restrict__ starts, const long* __restrict__ prefix, int S, long n, int pack,
    KeyWindow kw, uint64_t* __restrict__ ohi, uint32_t* __restrict__ ogid) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    int a = 0, b = S;          // largest s with prefix[s] <= i
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (prefix[m] <= i) a = m; else b = m;
    }
    const long j = starts[a] + (i - prefix[a]);
    const uint32_t g = ((uint32_t)a << 24) | rows[a][j];
    if (pack) {
      // one sortable word: the key's 32-bit window above the record id
      ohi[i] = ((key_window(his[a][j], kw) & 0xFFFFFFFFull) << 32) | g;
    } else {
      ohi[i] = his[a][j];
      ogid[i] = g;
    }
  }
}

}  // namespace
