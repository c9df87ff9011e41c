// GPU sort / shuffle kernels for MI355X.
//
// The radix sorts replace MapOutputBuffer's QuickSort over (partition, key)
// (hadoop-1.0.3 MapTask.java:1119-1130, 1415; util/QuickSort.java:57-131);
// the rest is TeraSort (BASELINE config 5): the map range-partitions its split
// without sorting it (TeraSort.java:57-211's trie partitioner), the reduce
// collects each group of partitions from every map, sorts a window of the
// key packed above a 32-bit record id (or (key, id) pairs), gathers the
// 100-byte records once, orders the runs the window left tied and checks the
// order (TeraValidate).
//
// This file is the translation unit and holds the two A/B tunables and the
// extern "C" entry points; the kernels are in the sections under sort/:
//  radix.h     : pairs sort (tile histogram, scan, stable scatter), onesweep
//  teragen.h   : TeraGen records, bit for bit, with an O(log n) LCG jump
//  partition.h : key words, partition count / offsets / scatter (the map),
//                splitter search of a sorted run, KeyWindow
//  collect.h   : collect (plain, shuffle slots, packed ids), order check,
//                group statistics, fold of per-block partial pairs
//  gather.h    : u64 and record gathers: by permutation, by (split, row), by
//                packed id in 16-B pieces
//  tie_fix.h   : order runs of an equal sorted prefix (keys, or records in place)
//  merge.h     : merge path of two sorted runs (K8)
#include "common.h"
#include "../include/hbmr/hbmr.h"

#include <algorithm>
#include "sort/radix.h"
#include "sort/teragen.h"
#include "sort/partition.h"
#include "sort/collect.h"
#include "sort/gather.h"
#include "sort/tie_fix.h"
#include "sort/merge.h"

namespace {

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

int g_onesweep_waves = 8;  // waves per onesweep tile (hbmr_radix_set_onesweep_waves, A/B)
int g_gather_unroll = 2;   // records in flight per lane group (hbmr_gather_set_unroll, A/B)

}  // namespace

extern "C" {

long hbmr_radix_sort_workspace_bytes(long n) {
  const long ntiles = std::max(1L, ceil_div(n, kSortTile));
  return (long)(kRadix * ntiles + kRadix) * 4;
}

// Sort (keys, vals) by key bits [begin_bit, end_bit) (8-bit digits, LSD, stable).
// keys/vals hold the input and receive the output; tkeys/tvals are scratch of
// the same size.  vals == nullptr sorts (key, original index) into tvals-free
// mode is not supported: pass a values array (e.g. iota) — see hbmr.ops.sort.
int hbmr_radix_sort_pairs_u64(uint64_t* keys, uint32_t* vals, uint64_t* tkeys, uint32_t* tvals,
                              long n, int begin_bit, int end_bit, void* ws, long ws_bytes,
                              hipStream_t st) {
  if (n <= 1) return 0;
  if (n >= (1L << 32) || begin_bit < 0 || end_bit > 64 || begin_bit >= end_bit)
    return (int)hipErrorInvalidValue;
  const long ntiles = ceil_div(n, kSortTile);
  if (ws_bytes < hbmr_radix_sort_workspace_bytes(n)) return (int)hipErrorInvalidValue;
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
  uint32_t* totals = hist + (long)kRadix * ntiles;
  uint64_t* ka = keys;
  uint32_t* va = vals;
  uint64_t* kb = tkeys;
  uint32_t* vb = tvals;
  int passes = 0;
  for (int shift = begin_bit; shift < end_bit; shift += 8, ++passes) {
    hipLaunchKernelGGL(radix_hist_v2_kernel, dim3((unsigned)ntiles), dim3(kSortThreads), 0, st,
                       ka, n, shift, ntiles, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(kRadix), dim3(1024), 0, st, hist, ntiles, totals);
    hipLaunchKernelGGL(radix_scatter_v2_kernel, dim3((unsigned)ntiles), dim3(kSortThreads), 0, st,
                       ka, va, kb, vb, n, shift, ntiles, hist, totals);
    std::swap(ka, kb);
    std::swap(va, vb);
  }
  if (passes & 1) {
    HBMR_RETURN_IF_ERROR(hipMemcpyAsync(keys, ka, n * 8, hipMemcpyDeviceToDevice, st));
    HBMR_RETURN_IF_ERROR(hipMemcpyAsync(vals, va, n * 4, hipMemcpyDeviceToDevice, st));
  }
  return (int)hipGetLastError();
}

long hbmr_radix_onesweep_workspace_bytes(long n) {
  return (long)(kMaxPasses * kRadix + kMaxPasses + 1) * 4;
}

long hbmr_radix_onesweep_status_bytes(long n) {
  return std::max(1L, ceil_div(n, kSortTile)) * kRadix * 8;   // tiles of >= 4096 keys
}

// Sort uint64 keys by bits [begin_bit, end_bit) (8-bit digits, LSD, stable),
// keys only, onesweep: one histogram read for all digits, then per digit one
// look-back scatter.  keys holds the input and receives the output; tkeys is
// scratch of the same size; *err (device) is set if a look-back timed out.
// status (hbmr_radix_onesweep_status_bytes) is reused across calls on one
// stream: each pass tags its words with a fresh epoch from *epoch (a host
// counter; at 0 or 0xFFFF the status is zeroed first and the count restarts).
// copy_back = 0 leaves an odd pass count's result in tkeys.
int hbmr_radix_sort_keys_u64(uint64_t* keys, uint64_t* tkeys, long n, int begin_bit, int end_bit,
                             void* ws, long ws_bytes, void* status, long status_bytes,
                             unsigned int* epoch, uint32_t* err, int copy_back, hipStream_t st) {
  if (n <= 1) return 0;
  const int passes = (end_bit - begin_bit + 7) / 8;
  if (n >= (1L << 30) || begin_bit < 0 || end_bit > 64 || begin_bit >= end_bit ||
      passes > kMaxPasses || epoch == nullptr)
    return (int)hipErrorInvalidValue;
  if (ws_bytes < hbmr_radix_onesweep_workspace_bytes(n) ||
      status_bytes < hbmr_radix_onesweep_status_bytes(n))
    return (int)hipErrorInvalidValue;
  const long ntiles = ceil_div(n, kSortTile);
  uint32_t* ghist = reinterpret_cast<uint32_t*>(ws);
  uint32_t* tickets = ghist + kMaxPasses * kRadix;
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(ghist, 0, (kMaxPasses * kRadix + kMaxPasses) * 4, st));
  const long hgrid = std::min<long>(ntiles, 2048);
  hipLaunchKernelGGL(radix_hist_all_kernel, dim3((unsigned)hgrid), dim3(kSortThreads), 0, st,
                     keys, n, begin_bit, end_bit, passes, ghist);
  hipLaunchKernelGGL(radix_bases_kernel, dim3((unsigned)passes), dim3(kSortThreads), 0, st, ghist);
  uint64_t* ka = keys;
  uint64_t* kb = tkeys;
  const int waves = g_onesweep_waves;
  const long tiles = ceil_div(n, (long)waves * 64 * kSortItems);
  for (int p = 0; p < passes; ++p) {
    if (*epoch == 0 || *epoch >= 0xFFFFu) {
      HBMR_RETURN_IF_ERROR(hipMemsetAsync(status, 0, status_bytes, st));
      *epoch = 0;
    }
    const uint64_t ep = ++*epoch;
    const int sh = begin_bit + 8 * p;
    const uint32_t dm = (1u << std::min(8, end_bit - begin_bit - 8 * p)) - 1u;
    if (waves == 16)
      hipLaunchKernelGGL(radix_onesweep_kernel<16>, dim3((unsigned)tiles), dim3(1024), 0, st, ka,
                         kb, n, sh, dm, ghist + p * kRadix, reinterpret_cast<uint64_t*>(status),
                         ep, tickets + p, err);
    else if (waves == 8)
      hipLaunchKernelGGL(radix_onesweep_kernel<8>, dim3((unsigned)tiles), dim3(512), 0, st, ka, kb,
                         n, sh, dm, ghist + p * kRadix, reinterpret_cast<uint64_t*>(status), ep,
                         tickets + p, err);
    else
      hipLaunchKernelGGL(radix_onesweep_kernel<4>, dim3((unsigned)tiles), dim3(256), 0, st, ka, kb,
                         n, sh, dm, ghist + p * kRadix, reinterpret_cast<uint64_t*>(status), ep,
                         tickets + p, err);
    std::swap(ka, kb);
  }
  if ((passes & 1) && copy_back)
    HBMR_RETURN_IF_ERROR(hipMemcpyAsync(keys, ka, n * 8, hipMemcpyDeviceToDevice, st));
  return (int)hipGetLastError();
}

int hbmr_teragen(long first_row, long nrows, void* out, hipStream_t st) {
  if (nrows <= 0) return 0;
  hipLaunchKernelGGL(teragen_kernel, dim3((unsigned)ceil_div(nrows, 256)), dim3(256), 0, st,
                     first_row, nrows, reinterpret_cast<uint8_t*>(out));
  return (int)hipGetLastError();
}

int hbmr_tera_keys(const void* records, long n, int stride, uint64_t* hi, uint64_t* lo,
                   hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(tera_keys_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint8_t*>(records), n, stride, hi, lo);
  return (int)hipGetLastError();
}

int hbmr_gather_u64(const uint64_t* src, const uint32_t* perm, long n, uint64_t* dst,
                    hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(gather_u64_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, src,
                     perm, n, dst);
  return (int)hipGetLastError();
}

int hbmr_gather_records(const void* src, const uint32_t* perm, long n, int record_bytes, void* dst,
                        hipStream_t st) {
  if (n <= 0) return 0;
  if (record_bytes % 4) return (int)hipErrorInvalidValue;
  const int words = record_bytes / 4;
  const long grid = std::min<long>(ceil_div(n * words, 256), 1L << 20);
  hipLaunchKernelGGL(gather_records_kernel, dim3((unsigned)grid), dim3(256), 0, st,
                     reinterpret_cast<const uint32_t*>(src), perm, n, words,
                     reinterpret_cast<uint32_t*>(dst));
  return (int)hipGetLastError();
}

int hbmr_split_offsets(const uint64_t* hi, const uint64_t* lo, long n, const uint64_t* shi,
                       const uint64_t* slo, int nparts, long* offsets, hipStream_t st) {
  hipLaunchKernelGGL(split_offsets_kernel, dim3((unsigned)ceil_div(nparts + 1, 256)), dim3(256), 0,
                     st, hi, lo, n, shi, slo, nparts, offsets);
  return (int)hipGetLastError();
}

int hbmr_check_sorted(const uint64_t* hi, const uint64_t* lo, long n, unsigned long long* bad,
                      hipStream_t st) {
  if (n <= 1) return 0;
  hipLaunchKernelGGL(check_sorted_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, hi,
                     lo, n, bad);
  return (int)hipGetLastError();
}

// acc: device u64[2 + 2 * 1024]: (out of order, checksum) accumulators, then
// the per-block partials
int hbmr_tera_group_stats(const uint64_t* hi, const uint64_t* lo, long n, const uint64_t* ph,
                          const uint64_t* pl, unsigned long long* acc, hipStream_t st) {
  if (n <= 0) return 0;
  if ((ph == nullptr) != (pl == nullptr)) return (int)hipErrorInvalidValue;
  const long grid = std::min<long>(ceil_div(n, 256 * 4), 1024);
  hipLaunchKernelGGL(tera_group_stats_kernel, dim3((unsigned)grid), dim3(256), 0, st, hi, lo, n,
                     ph, pl, acc + 2);
  hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(256), 0, st, acc + 2, grid, 0, acc);
  return (int)hipGetLastError();
}

int hbmr_tera_collect_slots(const uint32_t* const* rows, const long* starts, const long* pre,
                            int S, int W, long C, uint32_t* osplit, uint32_t* orow,
                            hipStream_t st) {
  if (W <= 0 || C <= 0) return 0;
  if (S <= 0) return (int)hipErrorInvalidValue;
  const long grid = std::min<long>(ceil_div((long)W * C, 256), 256L * 256);
  hipLaunchKernelGGL(tera_collect_slots_kernel, dim3((unsigned)grid), dim3(256), 0, st, rows,
                     starts, pre, S, W, C, osplit, orow);
  return (int)hipGetLastError();
}

int hbmr_tera_collect(const uint64_t* const* his, const uint64_t* const* los,
                      const uint32_t* const* rows, const long* starts, const long* prefix, int S,
                      long n, uint64_t* ohi, uint64_t* olo, uint32_t* osplit, uint32_t* orow,
                      hipStream_t st) {
  if (n <= 0) return 0;
  if (S <= 0) return (int)hipErrorInvalidValue;
  const long grid = std::min<long>(ceil_div(n, 256), 256L * 256);
  hipLaunchKernelGGL(tera_collect_kernel, dim3((unsigned)grid), dim3(256), 0, st, his, los, rows,
                     starts, prefix, S, n, ohi, olo, osplit, orow);
  return (int)hipGetLastError();
}

// TeraSort map v3: (hi, lo, row) of n records in partition order and the
// partition boundaries offsets[0..nparts] (int64, device).  ws: device scratch
// of hbmr_tera_partition_workspace_bytes(n, nparts) bytes.
constexpr long kPartGridMax = 256L * 64;

inline size_t part_count_w_lds(int nsplit) {
  return (size_t)nsplit * 8 + (size_t)(nsplit + 1) * 4 + (size_t)nsplit * 2 + 16;
}

long hbmr_tera_partition_workspace_bytes(long n, int nparts) {
  return n * 8 * 2 + n * 2 + 2L * (nparts + 1) * 4 + 64 + kPartGridMax * 16;
}

// kst (nullable, device uint64[2] the caller zeroes): [0] |= every key's
// high-word bytes, [1] += sum(hi + lo) over the split (its key checksum)
int hbmr_tera_partition(const void* records, long n, int stride, const uint64_t* shi,
                        const uint64_t* slo, int nsplit, uint64_t* ohi, uint64_t* olo,
                        uint32_t* orow, long* offsets, unsigned long long* kmm, void* ws,
                        long ws_bytes, hipStream_t st) {
  const int nparts = nsplit + 1;
  if (nsplit < 0 || nsplit > kMaxSplitters) return (int)hipErrorInvalidValue;
  if (n < 0 || n >= (1L << 32)) return (int)hipErrorInvalidValue;
  if (ws_bytes < hbmr_tera_partition_workspace_bytes(n, nparts)) return (int)hipErrorInvalidValue;
  uint8_t* p = reinterpret_cast<uint8_t*>(ws);
  uint64_t* hi = reinterpret_cast<uint64_t*>(p);
  uint64_t* lo = hi + n;
  uint16_t* pid = reinterpret_cast<uint16_t*>(lo + n);
  unsigned int* counts = reinterpret_cast<unsigned int*>(
      (reinterpret_cast<uintptr_t>(pid + n) + 15) & ~uintptr_t(15));
  unsigned int* cursor = counts + (nparts + 1);
  unsigned long long* kparts = reinterpret_cast<unsigned long long*>(
      (reinterpret_cast<uintptr_t>(cursor + (nparts + 1)) + 15) & ~uintptr_t(15));
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(counts, 0, (size_t)(nparts + 1) * 4, st));
  // word loads of the key when the records allow them, else byte loads
  const bool words = stride % 4 == 0 && stride >= 12 &&
                     reinterpret_cast<uintptr_t>(records) % 4 == 0;
  if (n > 0) {
    const long grid = std::min<long>(ceil_div(n, 256), kPartGridMax);
    unsigned long long* kp = kmm != nullptr ? kparts : nullptr;
    if (words)
      hipLaunchKernelGGL(tera_part_count_w_kernel, dim3((unsigned)grid), dim3(256),
                         part_count_w_lds(nsplit), st,
                         reinterpret_cast<const uint32_t*>(records), n, stride / 4, shi, slo,
                         nsplit, hi, lo, pid, counts, kp);
    else
      hipLaunchKernelGGL(tera_part_count_kernel, dim3((unsigned)grid), dim3(256), 0, st,
                         reinterpret_cast<const uint8_t*>(records), n, stride, shi, slo, nsplit,
                         hi, lo, pid, counts, kp);
    if (kmm != nullptr)
      hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(256), 0, st, kparts, grid, 1, kmm);
  }
  hipLaunchKernelGGL(tera_part_offsets_kernel, dim3(1), dim3(1024), 0, st, counts, nparts, cursor,
                     offsets);
  // (an LDS-staged scatter writing contiguous per-partition runs measured 2.4x
  // slower than this item-wise one: 19.1 vs 8.1 ms per 20 GB, twice the tiles'
  // scans, barriers and cursor atomics for writes that were already
  // ~85-record runs per partition and tile)
  if (n > 0)
    hipLaunchKernelGGL(tera_part_scatter_kernel, dim3((unsigned)ceil_div(n, kSortTile)),
                       dim3(kSortThreads), 0, st, hi, lo, pid, n, nparts, cursor, ohi, olo, orow);
  return (int)hipGetLastError();
}

int hbmr_tera_tie_fix(const uint64_t* hi, uint64_t* lo, uint32_t* perm, long n,
                      unsigned int* flag, hipStream_t st) {
  if (n <= 1) return 0;
  hipLaunchKernelGGL(tera_tie_fix_kernel, dim3((unsigned)ceil_div(n - 1, 256)), dim3(256), 0, st,
                     hi, lo, perm, n, flag);
  return (int)hipGetLastError();
}

int hbmr_merge_path(const uint64_t* ahi, const uint64_t* alo, const uint32_t* av, long na,
                    const uint64_t* bhi, const uint64_t* blo, const uint32_t* bv, long nb,
                    uint64_t* ohi, uint64_t* olo, uint32_t* ov, hipStream_t st) {
  const long n = na + nb;
  if (n <= 0) return 0;
  if (na < 0 || nb < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(merge_path_kernel, dim3((unsigned)ceil_div(ceil_div(n, kMergeItems), 256)),
                     dim3(256), 0, st, ahi, alo, av, na, bhi, blo, bv, nb, ohi, olo, ov);
  return (int)hipGetLastError();
}

// pack != 0: ohi = window << 32 | gid with the window of key_window(vlo, m,
// R, sh) (< 2^32 for the group's keys), ogid unused
int hbmr_tera_collect_gid(const uint64_t* const* his, const uint32_t* const* rows,
                          const long* starts, const long* prefix, int S, long n, int pack,
                          uint64_t vlo, unsigned int m, unsigned int R, int sh, uint64_t* ohi,
                          uint32_t* ogid, hipStream_t st) {
  if (n <= 0) return 0;
  if (S <= 0 || S > 256 || (!pack && ogid == nullptr) || R < 2 || R > 256 || m + R > 256 ||
      sh < 0 || sh > 63)
    return (int)hipErrorInvalidValue;
  const KeyWindow kw{vlo, m, R, sh};
  const long grid = std::min<long>(ceil_div(n, 256), 256L * 256);
  hipLaunchKernelGGL(tera_collect_gid_kernel, dim3((unsigned)grid), dim3(256), 0, st, his, rows,
                     starts, prefix, S, n, pack, kw, ohi, ogid);
  return (int)hipGetLastError();
}

// gid: the record ids (split << 24 | row), or nullptr and packed: sorted keys
// whose low 32 bits are the ids (hi may be packed itself: each record's id is
// read before its key is written over it, by the same lanes)
int hbmr_gather_records_gid(const void* const* bases, const uint32_t* gid, const uint64_t* packed,
                            long n, int record_bytes, void* dst, uint64_t* hi, uint64_t* lo,
                            uint32_t* win, hipStream_t st) {
  if (n <= 0) return 0;
  if (record_bytes % 4 || record_bytes > 4 * 64 || (gid == nullptr) == (packed == nullptr))
    return (int)hipErrorInvalidValue;
  if ((hi == nullptr) != (lo == nullptr) || (hi != nullptr && record_bytes < 12))
    return (int)hipErrorInvalidValue;
  const int words = record_bytes / 4;
  const int u = g_gather_unroll;
  const long rpb = (long)(HBMR_WAVE / ((words + 3) / 4)) * (256 / HBMR_WAVE);
  const long grid16 = std::min<long>(ceil_div(n, rpb * u), 1L << 18);
  auto k = u == 1 ? gather_records_gid16_kernel<1>
         : u == 4 ? gather_records_gid16_kernel<4>
         : u == 8 ? gather_records_gid16_kernel<8> : gather_records_gid16_kernel<2>;
  hipLaunchKernelGGL(k, dim3((unsigned)grid16), dim3(256), 0, st,
                     reinterpret_cast<const uint32_t* const*>(bases), gid, packed, n, words,
                     reinterpret_cast<uint32_t*>(dst), reinterpret_cast<uint32_t*>(hi), lo,
                     packed != nullptr ? win : nullptr);
  return (int)hipGetLastError();
}

// waves per onesweep scatter tile: 4 (4096 keys), 8 (default: 80M keys in
// 2.02 ms against 2.54 for 4 — longer digit runs per write, fewer look-backs)
// or 16 (1.98 ms, one workgroup per CU);
// returns the previous setting
int hbmr_radix_set_onesweep_waves(int w) {
  const int old = g_onesweep_waves;
  g_onesweep_waves = w == 4 || w == 16 ? w : 8;
  return old;
}

// records each lane group of the packed-id gather keeps in flight: 1, 2
// (default: 0.81 ms per 12.5M records against 0.91 for 4 and 1.39 for 8 —
// more random lines in flight per CU thrash it), 4 or 8; returns the previous
// setting
int hbmr_gather_set_unroll(int u) {
  const int old = g_gather_unroll;
  g_gather_unroll = u == 1 || u == 4 || u == 8 ? u : 2;
  return old;
}

long hbmr_tera_tie_fix_scratch_bytes(long cap, int record_bytes) {
  return 16 + cap * (4 + 8 + 8 + (long)record_bytes);
}

// scratch: hbmr_tera_tie_fix_scratch_bytes(cap, record_bytes) for at most cap
// moved records (more are flagged)
// runs: equal key_window(vlo, m, R, sh) of hi (m = 0, R = 256, vlo = 0: hi >> sh),
// read from win (the gather's copy of each record's window) when given
int hbmr_tera_tie_fix_records(uint64_t* hi, uint64_t* lo, void* rec, long n, int record_bytes,
                              uint64_t vlo, unsigned int m, unsigned int R, int sh,
                              const uint32_t* win, unsigned int* flag, void* scratch, long cap,
                              hipStream_t st) {
  if (n <= 1) return 0;
  if (record_bytes % 4 || record_bytes > 4 * 64 || sh < 0 || sh > 63 || cap < 1 ||
      n >= (1L << 32) || R < 2 || R > 256 || m + R > 256)
    return (int)hipErrorInvalidValue;
  const KeyWindow kw{vlo, m, R, sh};
  char* sc = reinterpret_cast<char*>(scratch);
  unsigned int* cnt = reinterpret_cast<unsigned int*>(sc);
  uint64_t* shi = reinterpret_cast<uint64_t*>(sc + 16);
  uint64_t* slo = shi + cap;
  uint32_t* sdst = reinterpret_cast<uint32_t*>(slo + cap);
  uint32_t* srec = sdst + cap;
  const int words = record_bytes / 4;
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(cnt, 0, 4, st));
  hipLaunchKernelGGL(tera_tie_rank_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, hi,
                     lo, reinterpret_cast<const uint32_t*>(rec), n, words, kw, win, cap, cnt, sdst,
                     shi, slo, srec, flag);
  const long grid = std::min<long>(ceil_div(cap, 256), 4096);
  hipLaunchKernelGGL(tera_tie_move_kernel, dim3((unsigned)grid), dim3(256), 0, st, hi, lo,
                     reinterpret_cast<uint32_t*>(rec), words, cap, cnt, sdst, shi, slo, srec);
  return (int)hipGetLastError();
}

int hbmr_gather_records_multi(const void* const* bases, const uint32_t* split, const uint32_t* row,
                              const uint32_t* perm, long n, int record_bytes, void* dst,
                              hipStream_t st) {
  if (n <= 0) return 0;
  if (record_bytes % 4 || record_bytes > 4 * 256) return (int)hipErrorInvalidValue;
  const int words = record_bytes / 4;
  constexpr int U = 4;
  const long grid = std::min<long>(ceil_div(n, (256 / words) * U), 1L << 18);
  hipLaunchKernelGGL(gather_records_multi_v3_kernel<U>, dim3((unsigned)grid), dim3(256), 0, st,
                     reinterpret_cast<const uint32_t* const*>(bases), split, row, perm, n, words,
                     reinterpret_cast<uint32_t*>(dst));
  return (int)hipGetLastError();
}

}  // extern "C"
