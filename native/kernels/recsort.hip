// Record sort kernels: variable-length byte-string keys carrying variable-length
// values (SURVEY.md K4 "sort records by (partition, key bytes)" and K9 "gather
// that permutes variable-size records", general form; sort.hip holds TeraSort's
// fixed 10/100-byte forms).
//
// A split is one byte buffer in HBM plus a per-record index: frame offset and
// length ([recordLen][keyLen][key][value], copied verbatim) and the offset and
// length of the key payload (behind BytesWritable's 4-byte length or Text's
// vint).  Order is WritableComparator.compareBytes on the payload: unsigned
// bytes, a proper prefix first.
//
//  1. recsort_hash_part: (hashBytes(payload) & INT_MAX) % R.  A key is spread
//     over 16 lanes (keys run to 1000 bytes): lane l folds bytes l, l+16, ...
//     with Horner steps of 31^16, scales by the power of 31 its last byte still
//     lacks, and the 16 partial sums are added (all mod 2^32); 31^len is h0 = 1.
//  2. String sort by rounds.  Round d gives an active record the 64-bit key
//     (payload[7d : 7d+7] zero-padded, big-endian) << 8 | min(len - 7d, 8); the
//     sequence of round keys orders byte strings like compareBytes (the low
//     byte puts "ab" < "ab\0" < "ab\0\0"; 8 = the key continues).  The active
//     records (those in a segment of more than one record whose key has not
//     ended; a segment = equal partition and equal round keys so far, so it is
//     active as a whole and its positions are consecutive) are sorted stably
//     by (segment, round key) with two calls of the LSD pairs sort of sort.hip
//     — the active list is in position order, hence already in segment order —
//     and written back into the positions they occupy.  One pass then flags
//     the heads of the new segments, scans the head index (the new segment id)
//     and compacts the next round's active set: recsort_flags_reduce (block
//     aggregates), recsort_scan_blocks, recsort_apply (write-back scatter +
//     compaction).
//  3. recsort_cuts: total order — lower bound of each split point over the
//     sorted keys by full-key compares (a key equal to a split point goes to
//     the upper partition: TotalOrderPartitioner's bisect_right over points).
//  4. recsort_gather: the variable-length record gather.  A record's frame is
//     cut into chunks of 16 of its DESTINATION-aligned 16-byte slots; 16 lanes
//     copy a chunk, lane l the slot l: full slots are one 16-byte load (at
//     whatever alignment the source has) and one aligned 16-byte store, the
//     partial slots at the frame's head and tail are copied bytewise.  The
//     chunks of a frame are consecutive, so a wave still moves 1 KiB of a
//     large frame in one piece and a 20 KB value spreads over 5 workgroups,
//     while the lanes of a wave are not idle on a 300-byte record.  A chunk
//     finds its record in a chunk → entry table (one load; a binary search
//     over the chunk offsets per chunk cost as much as the copy itself:
//     profiles/sort_1gpu.json).  The slot copy is bytes/records.h's, shared
//     with recjoin.hip's piece copy.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/records.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kKeyLanes = 16;                 // lanes per key in the hash kernel
constexpr uint64_t kContinues = 8;            // low byte of a round key: more bytes follow

inline long align_up(long a, long b) { return ceil_div(a, b) * b; }

__host__ __device__ constexpr uint32_t pow31(uint32_t e) {
  uint32_t r = 1, b = 31;
  while (e) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__global__ __launch_bounds__(kThreads) void recsort_hash_part_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ koff,
    const int64_t* __restrict__ klen, long n, uint32_t nparts, uint32_t* __restrict__ part) {
  const long key = (long)blockIdx.x * (kThreads / kKeyLanes) + (threadIdx.x / kKeyLanes);
  const int l = threadIdx.x % kKeyLanes;
  if (key >= n) return;              // a key's 16 lanes leave together
  const uint8_t* p = data + koff[key];
  const long len = klen[key];
  constexpr uint32_t kStep = pow31(kKeyLanes);
  uint32_t acc = 0;
  long last = -1;
  for (long i = l; i < len; i += kKeyLanes) {
    acc = acc * kStep + (uint32_t)(int32_t)(int8_t)p[i];
    last = i;
  }
  if (last >= 0) acc *= pow31((uint32_t)(len - 1 - last));
#pragma unroll
  for (int o = kKeyLanes / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kKeyLanes);
  if (l == 0) {
    const uint32_t h = acc + pow31((uint32_t)len);
    part[key] = (h & 0x7fffffffu) % nparts;
  }
}

__global__ __launch_bounds__(kThreads) void recsort_round_keys_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ koff,
    const int64_t* __restrict__ klen, const uint32_t* __restrict__ rec, long m, int d,
    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t r = rec[i];
  long left = klen[r] - 7L * d;
  if (left < 0) left = 0;
  const uint8_t* p = data + koff[r] + 7L * d;
  keys[i] = round_key(p, left);
  vals[i] = (uint32_t)i;
}

// after the round-key sort: the segment of each sorted entry as the key of the
// second (stable, narrow) sort, carrying the entry's rank in the first
__global__ __launch_bounds__(kThreads) void recsort_seg_keys_kernel(
    const uint32_t* __restrict__ seg, const uint32_t* __restrict__ vals, long m,
    uint64_t* __restrict__ skeys, uint32_t* __restrict__ rank) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  skeys[j] = seg[vals[j]];
  rank[j] = (uint32_t)j;
}

struct Sorted {            // the (segment, round key) order of a round
  const uint64_t* keys;    // round keys in round-key order
  const uint64_t* skeys;   // segments in (segment, round key) order
  const uint32_t* rank;    // rank in round-key order of entry i of the final order
  long m;
  __device__ bool head(long i) const {
    if (i == 0) return true;
    return skeys[i] != skeys[i - 1] || keys[rank[i]] != keys[rank[i - 1]];
  }
  // entry i is sorted again next round: its key goes on and its segment has company
  __device__ bool active(long i, bool head_i) const {
    if ((keys[rank[i]] & 0xff) != kContinues) return false;
    return !(head_i && (i == m - 1 || head(i + 1)));
  }
};

// inclusive scans over the 256 entries of a block: max of x, sum of y
__device__ __forceinline__ void block_scan_max_add(uint32_t& x, uint32_t& y, uint32_t* s_x,
                                                   uint32_t* s_y) {
  const int t = threadIdx.x;
  s_x[t] = x;
  s_y[t] = y;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < kThreads; o <<= 1) {
    const uint32_t ux = t >= o ? s_x[t - o] : 0, uy = t >= o ? s_y[t - o] : 0;
    __syncthreads();
    x = x > ux ? x : ux;
    y += uy;
    s_x[t] = x;
    s_y[t] = y;
    __syncthreads();
  }
}

// bmax[b]: 1 + the last head index in block b (0: none); bsum[b]: its active entries
__global__ __launch_bounds__(kThreads) void recsort_flags_reduce_kernel(
    Sorted s, uint32_t* __restrict__ bmax, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_x[kThreads], s_y[kThreads];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  uint32_t x = 0, y = 0;
  if (i < s.m) {
    const bool h = s.head(i);
    x = h ? (uint32_t)i + 1 : 0;
    y = s.active(i, h) ? 1 : 0;
  }
  block_scan_max_add(x, y, s_x, s_y);
  if (threadIdx.x == kThreads - 1) {
    bmax[blockIdx.x] = x;
    bsum[blockIdx.x] = y;
  }
}

// exclusive scans of the block aggregates in place (one workgroup); *count = active total
__global__ __launch_bounds__(kThreads) void recsort_scan_blocks_kernel(
    uint32_t* __restrict__ bmax, uint32_t* __restrict__ bsum, long nb,
    uint32_t* __restrict__ count) {
  __shared__ uint32_t s_x[kThreads], s_y[kThreads];
  uint32_t cx = 0, cy = 0;
  for (long base = 0; base < nb; base += kThreads) {
    const long b = base + threadIdx.x;
    const uint32_t x0 = b < nb ? bmax[b] : 0, y0 = b < nb ? bsum[b] : 0;
    uint32_t x = x0, y = y0;
    block_scan_max_add(x, y, s_x, s_y);
    const uint32_t tx = s_x[kThreads - 1], ty = s_y[kThreads - 1];
    if (b < nb) {
      // exclusive: the entries before b (the max scan has no inverse: take the neighbour's)
      const uint32_t px = threadIdx.x ? s_x[threadIdx.x - 1] : 0;
      bmax[b] = cx > px ? cx : px;
      bsum[b] = cy + y - y0;
    }
    cx = cx > tx ? cx : tx;
    cy += ty;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = cy;
}

// write-back scatter + compaction of the next round's active set
__global__ __launch_bounds__(kThreads) void recsort_apply_kernel(
    Sorted s, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ bmax,
    const uint32_t* __restrict__ bsum, const uint32_t* __restrict__ act_pos,
    const uint32_t* __restrict__ act_rec, uint32_t* __restrict__ perm,
    uint32_t* __restrict__ new_pos, uint32_t* __restrict__ new_rec,
    uint32_t* __restrict__ new_seg) {
  __shared__ uint32_t s_x[kThreads], s_y[kThreads];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  uint32_t x = 0, y = 0;
  bool act = false;
  if (i < s.m) {
    const bool h = s.head(i);
    act = s.active(i, h);
    x = h ? (uint32_t)i + 1 : 0;
    y = act ? 1 : 0;
  }
  block_scan_max_add(x, y, s_x, s_y);
  if (i >= s.m) return;
  const uint32_t rec = act_rec[vals[s.rank[i]]];
  const uint32_t pos = act_pos[i];
  perm[pos] = rec;
  if (act) {
    const uint32_t before = bmax[blockIdx.x];
    const uint32_t head = (x > before ? x : before) - 1;   // entry 0 is a head: never 0 - 1
    const uint32_t slot = bsum[blockIdx.x] + y - 1;
    new_pos[slot] = pos;
    new_rec[slot] = rec;
    new_seg[slot] = act_pos[head];
  }
}

__global__ void recsort_cuts_kernel(const uint8_t* __restrict__ data,
                                    const int64_t* __restrict__ koff,
                                    const int64_t* __restrict__ klen,
                                    const uint32_t* __restrict__ perm, long n,
                                    const uint8_t* __restrict__ sp,
                                    const int64_t* __restrict__ sp_off,
                                    const int64_t* __restrict__ sp_len, int nsplit,
                                    int64_t* __restrict__ cuts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsplit) return;
  const uint8_t* q = sp + sp_off[s];
  const long ql = sp_len[s];
  long lo = 0, hi = n;               // first sorted position whose key is >= the point
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    const uint32_t r = perm[mid];
    if (compare_from(data + koff[r], klen[r], q, ql, 0) < 0) lo = mid + 1;
    else hi = mid;
  }
  cuts[s] = lo;
}

// kCopyLanes consecutive lanes copy one chunk of a frame
__global__ __launch_bounds__(kThreads) void recsort_gather_kernel(
    const uint8_t* __restrict__ src, const uint32_t* __restrict__ perm,
    const int64_t* __restrict__ foff, const int64_t* __restrict__ flen,
    const int64_t* __restrict__ dst_off, const int64_t* __restrict__ chunk_base,
    const uint32_t* __restrict__ chunk_entry, long n, long nchunks, uint8_t* __restrict__ dst) {
  const long g = (long)blockIdx.x * (kThreads / kCopyLanes) + (threadIdx.x / kCopyLanes);
  if (g >= nchunks) return;
  const int lane = threadIdx.x % kCopyLanes;
  const long lo = chunk_entry[g];    // chunk g's entry: chunk_base[lo] <= g < chunk_base[lo + 1]
  const long c = g - chunk_base[lo];
  const long rec = perm ? (long)perm[lo] : lo;
  const long len = flen[rec];
  const long a = dst_off[lo];        // offset into dst: the frame is [a, a + len)
  copy_slot(dst, a, a + len, c, lane, [&] { return src + foff[rec]; });
}

}  // namespace

extern "C" {

int hbmr_recsort_hash_partition(const uint8_t* data, const int64_t* koff, const int64_t* klen,
                                long n, int nparts, uint32_t* part, hipStream_t st) {
  if (n <= 0) return 0;
  if (nparts <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recsort_hash_part_kernel,
                     dim3((unsigned)ceil_div(n, kThreads / kKeyLanes)), dim3(kThreads), 0, st,
                     data, koff, klen, n, (uint32_t)nparts, part);
  return (int)hipGetLastError();
}

int hbmr_recsort_round_keys(const uint8_t* data, const int64_t* koff, const int64_t* klen,
                            const uint32_t* rec, long m, int d, uint64_t* keys, uint32_t* vals,
                            hipStream_t st) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(recsort_round_keys_kernel, dim3((unsigned)ceil_div(m, kThreads)),
                     dim3(kThreads), 0, st, data, koff, klen, rec, m, d, keys, vals);
  return (int)hipGetLastError();
}

long hbmr_recsort_round_workspace_bytes(long m) {
  const long mm = std::max(1L, m), nb = ceil_div(mm, kThreads);
  return 3 * align_up(mm * 8, 256) + 3 * align_up(mm * 4, 256) + 2 * align_up(nb * 4, 256) +
         align_up(hbmr_radix_sort_workspace_bytes(mm), 256);
}

// One round of the string sort over the m active entries (act_pos ascending,
// act_rec the records there, act_seg their segments: non-decreasing, below
// 2^seg_bits).  Sorts them by (segment, round key d), writes the records back
// into perm at act_pos, and compacts the next round's active entries into
// new_pos / new_rec / new_seg (segment = position of the segment's head);
// *count (device) receives their number.
int hbmr_recsort_round(const uint8_t* data, const int64_t* koff, const int64_t* klen, int d,
                       long m, int seg_bits, const uint32_t* act_pos, const uint32_t* act_rec,
                       const uint32_t* act_seg, uint32_t* perm, uint32_t* new_pos,
                       uint32_t* new_rec, uint32_t* new_seg, uint32_t* count, void* ws,
                       long ws_bytes, hipStream_t st) {
  if (m <= 0) return (int)hipMemsetAsync(count, 0, 4, st);
  if (m >= (1L << 31) || seg_bits < 1 || seg_bits > 32 ||
      ws_bytes < hbmr_recsort_round_workspace_bytes(m))
    return (int)hipErrorInvalidValue;
  const long nb = ceil_div(m, kThreads);
  char* p = static_cast<char*>(ws);
  auto take = [&](long bytes) {
    char* q = p;
    p += align_up(bytes, 256);
    return q;
  };
  uint64_t* keys = reinterpret_cast<uint64_t*>(take(m * 8));
  uint64_t* tkeys = reinterpret_cast<uint64_t*>(take(m * 8));
  uint64_t* skeys = reinterpret_cast<uint64_t*>(take(m * 8));
  uint32_t* vals = reinterpret_cast<uint32_t*>(take(m * 4));
  uint32_t* tvals = reinterpret_cast<uint32_t*>(take(m * 4));
  uint32_t* rank = reinterpret_cast<uint32_t*>(take(m * 4));
  uint32_t* bmax = reinterpret_cast<uint32_t*>(take(nb * 4));
  uint32_t* bsum = reinterpret_cast<uint32_t*>(take(nb * 4));
  const long rws = hbmr_radix_sort_workspace_bytes(m);
  void* radix = take(rws);
  const dim3 grid((unsigned)nb), block(kThreads);
  hipLaunchKernelGGL(recsort_round_keys_kernel, grid, block, 0, st, data, koff, klen, act_rec, m,
                     d, keys, vals);
  int rc = hbmr_radix_sort_pairs_u64(keys, vals, tkeys, tvals, m, 0, 64, radix, rws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(recsort_seg_keys_kernel, grid, block, 0, st, act_seg, vals, m, skeys, rank);
  rc = hbmr_radix_sort_pairs_u64(skeys, rank, tkeys, tvals, m, 0, seg_bits, radix, rws, st);
  if (rc) return rc;
  const Sorted s{keys, skeys, rank, m};
  hipLaunchKernelGGL(recsort_flags_reduce_kernel, grid, block, 0, st, s, bmax, bsum);
  hipLaunchKernelGGL(recsort_scan_blocks_kernel, dim3(1), block, 0, st, bmax, bsum, nb, count);
  hipLaunchKernelGGL(recsort_apply_kernel, grid, block, 0, st, s, vals, bmax, bsum, act_pos,
                     act_rec, perm, new_pos, new_rec, new_seg);
  return (int)hipGetLastError();
}

// cuts[s]: the first of the n sorted positions whose key is >= split point s
int hbmr_recsort_cuts(const uint8_t* data, const int64_t* koff, const int64_t* klen,
                      const uint32_t* perm, long n, const uint8_t* sp, const int64_t* sp_off,
                      const int64_t* sp_len, int nsplit, int64_t* cuts, hipStream_t st) {
  if (nsplit <= 0) return 0;
  hipLaunchKernelGGL(recsort_cuts_kernel, dim3((unsigned)ceil_div(nsplit, 64)), dim3(64), 0, st,
                     data, koff, klen, perm, n, sp, sp_off, sp_len, nsplit, cuts);
  return (int)hipGetLastError();
}

int hbmr_recsort_chunk_bytes(void) { return kCopyChunk; }

// dst[dst_off[i] : + flen[r]] = src[foff[r] : + flen[r]] with r = perm[i] (perm
// null: r = i), i < n.  chunk_base[n + 1]: the exclusive scan of each entry's
// chunk count ((dst address & 15) + flen[r] + chunk - 1) / chunk, chunk =
// hbmr_recsort_chunk_bytes().  chunk_entry[nchunks]: the entry each chunk belongs to.
int hbmr_recsort_gather(const uint8_t* src, const uint32_t* perm, const int64_t* foff,
                        const int64_t* flen, const int64_t* dst_off, const int64_t* chunk_base,
                        const uint32_t* chunk_entry, long n, long nchunks, uint8_t* dst,
                        hipStream_t st) {
  if (n <= 0 || nchunks <= 0) return 0;
  const long grid = ceil_div(nchunks, kThreads / kCopyLanes);
  if (grid >= (1L << 31) || chunk_entry == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recsort_gather_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, src, perm,
                     foff, flen, dst_off, chunk_base, chunk_entry, n, nchunks, dst);
  return (int)hipGetLastError();
}

}  // extern "C"
