// Record join kernels: the map-side join of sorted SequenceFile splits
// (CompositeInputFormat's inner / outer / override over tbl sources) on splits
// that lie in HBM as recsort.hip has them: a byte buffer plus, per record, the
// offset and length of its frame and of its key payload.  Order is compareBytes
// on the payload, as in recsort.hip.
//
//  1. recjoin_heads: a record opens a group when its key is above its
//     predecessor's; a key below its predecessor's is unsorted input and the
//     smallest such record is reported (vector atomic min).  Adjacent keys are
//     compared by a group of 16 lanes, 16 bytes a lane and 256 bytes a step (keys
//     run to 1000 bytes); the first differing byte is a min over the group.
//  2. recjoin_rank: for every group head of a source, the lower bound of its
//     key among another source's group heads and whether the key there is
//     equal.  Two levels: a search over the dense round keys 0 of the other
//     source's heads (recsort's 64-bit key: 7 bytes and min(len, 8)), then,
//     only if the key goes on beyond 7 bytes, full compares from byte 7 inside
//     the run of equal round key (against full compares over all heads: 0.15
//     vs 0.36 ms on RandomWriter keys, level on text keys; tools/bench_join.py,
//     profiles/join_1gpu.json).
//  3. recjoin_expand: one thread per output tuple of a tuple range finds its key
//     by a search over the keys' first tuples, takes its odometer digits (last
//     source fastest) and gives the record of every slot and the frame length.
//  4. recjoin_frames: once the host has laid the frames out in the file body,
//     16 lanes per tuple write [recordLen][keyLen] and the TupleWritable header
//     of the tuple's mask, and list the pieces to copy: the serialized key and
//     one value per written slot (override: the whole frame of the record).
//  5. recjoin_copy: the piece copy, recsort_gather's scheme (16 lanes per chunk
//     of 16 destination-aligned 16-byte slots) over pieces that name their
//     source by address, so the pieces of all sources go in one launch (against
//     hbmr_recsort_gather once per source for the values and once per owner for
//     the keys: 0.45 vs 0.97 ms and 1.06 vs 1.33 ms, same profile).
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/records.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 16;                    // lanes per key pair, per tuple, per copy chunk
constexpr int kStep = kLanes * 16;            // bytes a lane group covers in one step
int g_two_level = 1;                          // hbmr_recjoin_set_two_level (A/B)

// per source the addresses of data, foff, flen, koff, klen (a device table: the
// source of a tuple varies per thread)
struct Sources {
  const int64_t* tab;
  __device__ const uint8_t* data(int s) const {
    return reinterpret_cast<const uint8_t*>(tab[5 * s]);
  }
  __device__ const int64_t* row(int s, int r) const {
    return reinterpret_cast<const int64_t*>(tab[5 * s + 1 + r]);
  }
  __device__ long foff(int s, long i) const { return row(s, 0)[i]; }
  __device__ long flen(int s, long i) const { return row(s, 1)[i]; }
  // end of the serialized key = start of the value
  __device__ long kend(int s, long i) const { return row(s, 2)[i] + row(s, 3)[i]; }
};

// compareBytes(a, b) by the 16 lanes of a group; every lane returns the result
__device__ __forceinline__ int group_compare(const uint8_t* a, long la, const uint8_t* b, long lb,
                                             int lane) {
  const long n = la < lb ? la : lb;
  for (long base = 0; base < n; base += kStep) {
    const long o = base + lane * 16L;
    int d = 16;                                // first differing byte of this lane's piece
    if (o + 16 <= n) {
      uint4 x, y;
      __builtin_memcpy(&x, a + o, 16);         // both have whatever alignment they have
      __builtin_memcpy(&y, b + o, 16);
      const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
      if (d3) d = 12 + (__builtin_ctz(d3) >> 3);
      if (d2) d = 8 + (__builtin_ctz(d2) >> 3);
      if (d1) d = 4 + (__builtin_ctz(d1) >> 3);
      if (d0) d = __builtin_ctz(d0) >> 3;
    } else {
      for (long i = o; i < n; ++i)
        if (a[i] != b[i]) {
          d = (int)(i - o);
          break;
        }
    }
    int pos = d < 16 ? lane * 16 + d : kStep;
#pragma unroll
    for (int w = kLanes / 2; w > 0; w >>= 1) {
      const int other = __shfl_xor(pos, w, kLanes);
      pos = other < pos ? other : pos;
    }
    if (pos < kStep) return a[base + pos] < b[base + pos] ? -1 : 1;
  }
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

__global__ __launch_bounds__(kThreads) void recjoin_heads_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ koff,
    const int64_t* __restrict__ klen, long n, int32_t* __restrict__ head,
    uint32_t* __restrict__ bad) {
  const long i = (long)blockIdx.x * (kThreads / kLanes) + threadIdx.x / kLanes;
  const int lane = threadIdx.x % kLanes;
  if (i >= n) return;                          // a pair's 16 lanes leave together
  int c = -1;
  if (i > 0) c = group_compare(data + koff[i - 1], klen[i - 1], data + koff[i], klen[i], lane);
  if (lane == 0) {
    head[i] = c < 0 ? 1 : 0;
    if (c > 0) atomicMin(bad, (uint32_t)i);
  }
}

struct Heads {             // the group heads of one source
  const uint8_t* data;
  const int64_t* koff;
  const int64_t* klen;
  const int32_t* rec;      // record of each head
  long n;
};

__global__ __launch_bounds__(kThreads) void recjoin_rank_kernel(
    Heads p, Heads t, const uint64_t* __restrict__ thk, int two_level, int32_t* __restrict__ lb,
    int32_t* __restrict__ eq) {
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= p.n) return;
  const long r = p.rec[g];
  const uint8_t* q = p.data + p.koff[r];
  const long ql = p.klen[r];
  long lo = 0, hi = t.n, from = 0;
  bool full = true;                            // a full compare decides inside [lo, hi)
  if (two_level) {
    const uint64_t rk = round_key(q, ql);
    long a = 0, b = t.n;                       // first head whose round key is >= rk
    while (a < b) {
      const long mid = (a + b) >> 1;
      if (thk[mid] < rk) a = mid + 1;
      else b = mid;
    }
    lo = a;
    b = t.n;                                   // first head whose round key is > rk
    while (a < b) {
      const long mid = (a + b) >> 1;
      if (thk[mid] <= rk) a = mid + 1;
      else b = mid;
    }
    hi = a;
    from = 7;
    full = (rk & 0xff) > 7;                    // <= 7: the key ended, equal round keys = equal keys
  }
  int e;
  if (full) {
    const long end = hi;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      const long m = t.rec[mid];
      if (compare_from(t.data + t.koff[m], t.klen[m], q, ql, from) < 0) lo = mid + 1;
      else hi = mid;
    }
    e = 0;
    if (lo < end) {
      const long m = t.rec[lo];
      e = compare_from(t.data + t.koff[m], t.klen[m], q, ql, from) == 0;
    }
  } else {
    e = hi > lo;
  }
  lb[g] = (int32_t)lo;
  eq[g] = e;
}

struct Keys {              // the K output keys in key order
  const int64_t* base;     // [K + 1] first tuple of each key
  const int32_t* mask;     // [K] sources that have the key
  const int32_t* first;    // [S, K] first record of the key in each source
  const int32_t* cnt;      // [S, K] its records there (0: absent)
  const int32_t* osrc;     // [K] the source whose records give the key bytes (override: the output)
  const int32_t* orec;     // [K] its first record of the key
  long K;
};

__global__ __launch_bounds__(kThreads) void recjoin_expand_kernel(
    Sources src, int S, Keys keys, int override_op, const int32_t* __restrict__ hdr_len, long lo,
    long T, int32_t* __restrict__ tkey, int32_t* __restrict__ trec, int64_t* __restrict__ tlen) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= T) return;
  const long t = lo + j;
  long a = 0, b = keys.K;                      // base[a] <= t < base[a + 1]
  while (b - a > 1) {
    const long mid = (a + b) >> 1;
    if (keys.base[mid] <= t) a = mid;
    else b = mid;
  }
  const long k = a;
  long r = t - keys.base[k];
  tkey[j] = (int32_t)k;
  const int o = keys.osrc[k];
  if (override_op) {
    const long rec = keys.first[o * keys.K + k] + r;
    for (int s = 0; s < S; ++s) trec[s * T + j] = s == o ? (int32_t)rec : -1;
    tlen[j] = src.flen(o, rec);
    return;
  }
  const long orec = keys.orec[k];
  long len = src.kend(o, orec) - src.foff(o, orec) + hdr_len[keys.mask[k]];   // 8 + key + header
  for (int s = S - 1; s >= 0; --s) {
    const long c = keys.cnt[s * keys.K + k];
    int32_t rec = -1;
    if (c > 0) {
      rec = (int32_t)(keys.first[s * keys.K + k] + r % c);
      r /= c;
      len += src.foff(s, rec) + src.flen(s, rec) - src.kend(s, rec);
    }
    trec[s * T + j] = rec;
  }
  tlen[j] = len;
}

__global__ __launch_bounds__(kThreads) void recjoin_frames_kernel(
    Sources src, int S, Keys keys, int override_op, const int32_t* __restrict__ hdr_len,
    const int32_t* __restrict__ hdr_off, const uint8_t* __restrict__ hdr_bytes, long T,
    const int32_t* __restrict__ tkey, const int32_t* __restrict__ trec,
    const int64_t* __restrict__ tlen, const int64_t* __restrict__ dst_off,
    uint8_t* __restrict__ dst, int64_t* __restrict__ psrc, int64_t* __restrict__ plen,
    int64_t* __restrict__ pdst) {
  const long j = (long)blockIdx.x * (kThreads / kLanes) + threadIdx.x / kLanes;
  const int lane = threadIdx.x % kLanes;
  if (j >= T) return;
  const long k = tkey[j];
  const long d = dst_off[j];
  const int o = keys.osrc[k];
  const long p0 = j * (S + 1);
  if (override_op) {
    if (lane <= S) {
      const long rec = trec[o * T + j];
      psrc[p0 + lane] = (int64_t)reinterpret_cast<uintptr_t>(src.data(o) + src.foff(o, rec));
      plen[p0 + lane] = lane == 0 ? tlen[j] : 0;
      pdst[p0 + lane] = d;
    }
    return;
  }
  const long orec = keys.orec[k];
  const long kstart = src.foff(o, orec) + 8;
  const long kser = src.kend(o, orec) - kstart;
  const int m = keys.mask[k];
  const int hl = hdr_len[m];
  const uint8_t* hb = hdr_bytes + hdr_off[m];
  const uint32_t reclen = (uint32_t)(tlen[j] - 8);
  for (int i = lane; i < 8 + hl; i += kLanes) {
    if (i < 4) dst[d + i] = (uint8_t)(reclen >> (8 * (3 - i)));
    else if (i < 8) dst[d + i] = (uint8_t)((uint32_t)kser >> (8 * (7 - i)));
    else dst[d + kser + i] = hb[i - 8];
  }
  if (lane == 0) {
    psrc[p0] = (int64_t)reinterpret_cast<uintptr_t>(src.data(o) + kstart);
    plen[p0] = kser;
    pdst[p0] = d + 8;
    long at = d + 8 + kser + hl;
    for (int s = 0; s < S; ++s) {
      const long rec = trec[s * T + j];
      long vl = 0, vs = 0;
      if (rec >= 0) {
        vs = src.kend(s, rec);
        vl = src.foff(s, rec) + src.flen(s, rec) - vs;
      }
      psrc[p0 + 1 + s] = (int64_t)reinterpret_cast<uintptr_t>(src.data(s) + vs);
      plen[p0 + 1 + s] = vl;
      pdst[p0 + 1 + s] = at;
      at += vl;
    }
  }
}

// 16 consecutive lanes copy one chunk of 16 destination-aligned 16-byte slots of a piece
__global__ __launch_bounds__(kThreads) void recjoin_copy_kernel(
    const int64_t* __restrict__ psrc, const int64_t* __restrict__ plen,
    const int64_t* __restrict__ pdst, const int64_t* __restrict__ chunk_base,
    const uint32_t* __restrict__ chunk_entry, long nchunks, uint8_t* __restrict__ dst) {
  const long g = (long)blockIdx.x * (kThreads / kLanes) + threadIdx.x / kLanes;
  if (g >= nchunks) return;
  const int lane = threadIdx.x % kLanes;
  const long p = chunk_entry[g];
  const long c = g - chunk_base[p];
  const long a = pdst[p];
  copy_slot(dst, a, a + plen[p], c, lane,
            [&] { return reinterpret_cast<const uint8_t*>((uintptr_t)psrc[p]); });
}

}  // namespace

extern "C" {

// head[i] = 1 if record i opens a group (i = 0, or its key is above its
// predecessor's), else 0; *bad = the first record whose key is below its
// predecessor's, 0xffffffff if the keys are sorted.
int hbmr_recjoin_heads(const uint8_t* data, const int64_t* koff, const int64_t* klen, long n,
                       int32_t* head, uint32_t* bad, hipStream_t st) {
  const hipError_t rc = hipMemsetAsync(bad, 0xff, 4, st);
  if (rc != hipSuccess) return (int)rc;
  if (n <= 0) return 0;
  if (n >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recjoin_heads_kernel, dim3((unsigned)ceil_div(n, kThreads / kLanes)),
                     dim3(kThreads), 0, st, data, koff, klen, n, head, bad);
  return (int)hipGetLastError();
}

// the rank kernel searches the round keys first (1, the default) or runs full
// compares over all heads (0): an A/B knob of tools/bench_join.py
int hbmr_recjoin_set_two_level(int on) {
  g_two_level = on ? 1 : 0;
  return 0;
}

// For head g < np of the probe source (record prec[g]): lb[g] = the number of the
// nt heads of the other source (records trec, ascending keys, round keys 0 in
// thk) whose key is below its key, eq[g] = 1 if head lb[g] has its key.
int hbmr_recjoin_rank(const uint8_t* pdata, const int64_t* pkoff, const int64_t* pklen,
                      const int32_t* prec, long np, const uint8_t* tdata, const int64_t* tkoff,
                      const int64_t* tklen, const int32_t* trec, const uint64_t* thk, long nt,
                      int32_t* lb, int32_t* eq, hipStream_t st) {
  if (np <= 0) return 0;
  if (np >= (1L << 31) || nt >= (1L << 31) || nt < 0) return (int)hipErrorInvalidValue;
  const Heads p{pdata, pkoff, pklen, prec, np}, t{tdata, tkoff, tklen, trec, nt};
  hipLaunchKernelGGL(recjoin_rank_kernel, dim3((unsigned)ceil_div(np, kThreads)), dim3(kThreads), 0,
                     st, p, t, thk, g_two_level, lb, eq);
  return (int)hipGetLastError();
}

// Tuples [lo, lo + T) of the join of S sources (tab: int64[5 * S], per source
// the addresses of data, foff, flen, koff, klen) over K keys: tkey[T] the key,
// trec[S, T] the record of each slot (-1: unwritten), tlen[T] the frame length.
int hbmr_recjoin_expand(const int64_t* tab, int S, const int64_t* base, const int32_t* mask,
                        const int32_t* first, const int32_t* cnt, const int32_t* osrc,
                        const int32_t* orec, long K, int override_op, const int32_t* hdr_len,
                        long lo, long T, int32_t* tkey, int32_t* trec, int64_t* tlen,
                        hipStream_t st) {
  if (T <= 0) return 0;
  if (S < 1 || S > 8 || K <= 0 || K >= (1L << 31) || T >= (1L << 31) || lo < 0)
    return (int)hipErrorInvalidValue;
  const Keys keys{base, mask, first, cnt, osrc, orec, K};
  hipLaunchKernelGGL(recjoin_expand_kernel, dim3((unsigned)ceil_div(T, kThreads)), dim3(kThreads),
                     0, st, Sources{tab}, S, keys, override_op, hdr_len, lo, T, tkey, trec, tlen);
  return (int)hipGetLastError();
}

// The frames of the T expanded tuples at dst_off[T] in dst: writes the record
// header and the tuple header (hdr_bytes[hdr_off[mask] : + hdr_len[mask]]) and
// lists the S + 1 pieces of each tuple (psrc address, plen, pdst offset in dst)
// for hbmr_recjoin_copy.
int hbmr_recjoin_frames(const int64_t* tab, int S, const int32_t* mask, const int32_t* osrc,
                        const int32_t* orec, int override_op, const int32_t* hdr_len,
                        const int32_t* hdr_off, const uint8_t* hdr_bytes, long T,
                        const int32_t* tkey, const int32_t* trec, const int64_t* tlen,
                        const int64_t* dst_off, uint8_t* dst, int64_t* psrc, int64_t* plen,
                        int64_t* pdst, hipStream_t st) {
  if (T <= 0) return 0;
  if (S < 1 || S > 8 || T >= (1L << 31)) return (int)hipErrorInvalidValue;
  const Keys keys{nullptr, mask, nullptr, nullptr, osrc, orec, 0};
  hipLaunchKernelGGL(recjoin_frames_kernel, dim3((unsigned)ceil_div(T, kThreads / kLanes)),
                     dim3(kThreads), 0, st, Sources{tab}, S, keys, override_op, hdr_len, hdr_off,
                     hdr_bytes, T, tkey, trec, tlen, dst_off, dst, psrc, plen, pdst);
  return (int)hipGetLastError();
}

// dst[pdst[p] : + plen[p]] = the plen[p] bytes at address psrc[p].  chunk_base:
// the exclusive scan of each piece's chunk count (0 for an empty piece, else
// ((dst address + pdst) & 15) + plen + 255) / 256); chunk_entry[nchunks]: the
// piece of each chunk.
int hbmr_recjoin_copy(const int64_t* psrc, const int64_t* plen, const int64_t* pdst,
                      const int64_t* chunk_base, const uint32_t* chunk_entry, long nchunks,
                      uint8_t* dst, hipStream_t st) {
  if (nchunks <= 0) return 0;
  const long grid = ceil_div(nchunks, kThreads / kLanes);
  if (grid >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recjoin_copy_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, psrc, plen,
                     pdst, chunk_base, chunk_entry, nchunks, dst);
  return (int)hipGetLastError();
}

}  // extern "C"
