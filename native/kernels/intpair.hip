// Int-pair text kernels: the map and the reduce of SecondarySort
// (hbmr/ops/intpair.py holds the definition and the CPU twin;
// hbmr/models/secondarysort.py is the job).  The first device code here that
// reads numbers out of text and writes them back.
//
// A line is a '\n'-terminated entry of the split (the last may lack its '\n');
// white space is str.split()'s ASCII set: 9-13, 28-31, 32.  A line with fewer than
// two tokens is skipped; otherwise its first two tokens must have the device
// form [+-]?[0-9]+ with a value in int32, else the line is irregular and the
// host redoes the split with Python's own int().  A record's key is the word of
// IntPair.serialize, (first + 2^31) << 32 | (second + 2^31): unsigned order of
// the word is the job's sort order, the high word alone its grouping.
//
//  1. intpair_lines_count / intpair_lines_write: the kernel's own newline pass,
//     16 bytes a lane at whatever alignment the buffer has (a split of another
//     job's cache need not be aligned).  count leaves the newlines per 4 KiB tile
//     and raises the non-ASCII flag; the host scans the tile counts; write ranks
//     the newlines of a tile with the block scan of bytes/scan.h and stores the
//     line starts.
//  2. intpair_parse: one lane per line.  The bytes of a workgroup's 256 lines are
//     one run of the buffer: up to 16 KiB they are staged in LDS with aligned
//     16-byte loads (nothing outside the buffer is read), longer runs are read
//     from memory.  A lane walks its line once, never past the line's end (known
//     on entry), and stops after the second token; digits
//     accumulate in 64 bits and saturate, so a long token cannot wrap back into
//     range.  (status, key) per line, the records per workgroup for the
//     compaction, and the irregular flag.
//  3. intpair_compact: the keys of the record lines, in line order, by the block
//     scan over the statuses and the host's scan of the workgroup counts.
//  4. intpair_partition: abs(first * 127) % R in 64 bits (INT_MIN * 127 fits).
//  5. intpair_lengths: bytes of "<first>\t<second>\n" per sorted record, plus the
//     49 bytes of the separator line where the high word differs from the
//     predecessor's (a group head; record 0 is one).
//  6. intpair_fill: a workgroup takes 256 consecutive records, whose text is one
//     run of the output.  A lane composes its record in three 64-bit registers
//     (pushed from the back: '\n', the digits of second from the least
//     significant, ...) and puts it into LDS at the run's own misalignment, so an
//     LDS slot is a destination slot; the run then leaves as aligned 16-byte
//     stores, its partial head and tail slots bytewise.  No byte outside the run
//     is written.
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/scan.h"

namespace {

constexpr int kThreads = kScanThreads;                 // 256
constexpr int kLaneBytes = 16;
constexpr int kTile = kThreads * kLaneBytes;           // bytes of a newline tile
constexpr int kRecMax = 24;                            // "-2147483648\t-2147483648\n" is 24 bytes
constexpr int kSepLen = 49;                            // 48 dashes and '\n'
constexpr int kRunMax = kThreads * (kRecMax + kSepLen);
constexpr int kRunSlots = (kRunMax + 15 + 15) / 16;    // + the run's misalignment
constexpr int kStageBytes = 16384;                     // bytes of 256 lines the parse stages in LDS
constexpr int kStageSlots = (kStageBytes + 15 + 15) / 16;

enum : uint8_t { kSkip = 0, kRecord = 1, kIrregular = 2 };

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

__device__ __forceinline__ bool is_space(uint8_t c) {
  return (uint32_t)c - 9u <= 4u || (uint32_t)c - 28u <= 4u;      // 9-13, 28-32
}

// 0x80 in each byte of w that equals '\n' (exact: no borrow across bytes)
__device__ __forceinline__ uint32_t newline_bytes(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// bit j set: byte i0 + j of buf[0, n) is '\n'; *high: some byte is >= 0x80
__device__ __forceinline__ uint32_t newline_mask(const uint8_t* __restrict__ buf, long n, long i0,
                                                 bool* high) {
  uint32_t m = 0;
  *high = false;
  if (i0 + kLaneBytes <= n) {
    uint4 v;
    __builtin_memcpy(&v, buf + i0, 16);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t t = newline_bytes(w[k]);
      m |= (((t >> 7) & 1) | ((t >> 14) & 2) | ((t >> 21) & 4) | ((t >> 28) & 8)) << (4 * k);
      *high |= (w[k] & 0x80808080u) != 0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kLaneBytes; ++j) {
      if (i0 + j < n) {
        const uint8_t c = buf[i0 + j];
        m |= (uint32_t)(c == '\n') << j;
        *high |= c >= 0x80;
      }
    }
  }
  return m;
}

__global__ __launch_bounds__(kThreads) void intpair_lines_count_kernel(
    const uint8_t* __restrict__ buf, long n, uint32_t* __restrict__ tile_counts,
    int* __restrict__ non_ascii) {
  __shared__ uint32_t s_w[kScanWaves];
  bool high = false;
  const long i0 = (long)blockIdx.x * kTile + (long)threadIdx.x * kLaneBytes;
  const uint32_t m = i0 < n ? newline_mask(buf, n, i0, &high) : 0u;
  if (high) atomicOr(non_ascii, 1);
  const uint32_t total = block_reduce_add(__popc(m), s_w);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// starts[0] = 0; newline k of the buffer, at byte i, begins line k + 1 if i + 1 < n
__global__ __launch_bounds__(kThreads) void intpair_lines_write_kernel(
    const uint8_t* __restrict__ buf, long n, const long* __restrict__ tile_base, long nlines,
    int32_t* __restrict__ starts) {
  __shared__ uint32_t s_w[kScanWaves];
  bool high = false;
  const long i0 = (long)blockIdx.x * kTile + (long)threadIdx.x * kLaneBytes;
  uint32_t m = i0 < n ? newline_mask(buf, n, i0, &high) : 0u;
  long line = tile_base[blockIdx.x] + block_excl_scan(__popc(m), s_w) + 1;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nlines > 0) starts[0] = 0;
  for (int k = 0; k < kLaneBytes && m; ++k) {          // at most 16 bits are set
    const int j = __ffs(m) - 1;
    m &= m - 1;
    if (i0 + j + 1 < n && line < nlines) starts[line] = (int32_t)(i0 + j + 1);
    ++line;
  }
}

// One token of buf[pos, end): pos moves past it.  false: no token left.  *bad:
// not of the form [+-]?[0-9]+ or outside int32.  (Positions are ints: a split has
// fewer than 2^31 bytes.)
__device__ __forceinline__ bool next_int(const uint8_t* __restrict__ buf, int& pos, int end,
                                         int32_t* value, bool* bad) {
  while (pos < end && is_space(buf[pos])) ++pos;
  if (pos >= end) return false;
  bool neg = false, junk = false;
  uint8_t c = buf[pos];
  if (c == '+' || c == '-') {
    neg = c == '-';
    ++pos;
  }
  uint64_t acc = 0;
  const int first_digit = pos;
  for (; pos < end; ++pos) {
    c = buf[pos];
    if (is_space(c)) break;
    const uint32_t d = (uint32_t)c - '0';
    junk |= d > 9u;
    // 64 bits hold acc * 10 + 9 for any acc < 2^32; at 2^32 and above acc is
    // saturated and stays: out of range.  (One 32 x 32 -> 64 multiply-add a
    // digit: a full 64-bit multiply is three quarter-rate multiplies.)
    if (acc < (1ull << 32)) acc = (uint64_t)(uint32_t)acc * 10u + (d > 9u ? 0u : d);
  }
  const uint64_t limit = neg ? (1ull << 31) : (1ull << 31) - 1;
  *bad = junk || pos == first_digit || acc > limit;
  *value = neg ? (int32_t)(0u - (uint32_t)acc) : (int32_t)(uint32_t)acc;
  return true;
}

__device__ __forceinline__ uint64_t pair_key(int32_t first, int32_t second) {
  return (uint64_t)((uint32_t)first ^ 0x80000000u) << 32 | ((uint32_t)second ^ 0x80000000u);
}

// the line src[pos, end): its status, and a record's two values
__device__ __forceinline__ uint8_t parse_line(const uint8_t* __restrict__ src, int pos, int end,
                                              int32_t* a, int32_t* b) {
  bool bad_a = false, bad_b = false;
  if (!next_int(src, pos, end, a, &bad_a) || !next_int(src, pos, end, b, &bad_b)) return kSkip;
  return (bad_a || bad_b) ? kIrregular : kRecord;
}

__global__ __launch_bounds__(kThreads) void intpair_parse_kernel(
    const uint8_t* __restrict__ buf, long n, const int32_t* __restrict__ starts, long nlines,
    uint8_t* __restrict__ status, int64_t* __restrict__ keys, uint32_t* __restrict__ block_counts,
    int* __restrict__ irregular) {
  __shared__ uint32_t s_w[kScanWaves];
  __shared__ uint4 s_slots[kStageSlots];
  uint8_t* s = reinterpret_cast<uint8_t*>(s_slots);
  // the bytes of the workgroup's lines are one run buf[lo, hi): staged in LDS in
  // 16-byte pieces when they fit (LDS byte x is buf[lo - mis + x]), else each lane
  // reads its line from memory
  const long b0 = (long)blockIdx.x * kThreads;
  const long b1 = b0 + kThreads < nlines ? b0 + kThreads : nlines;
  long lo = starts[b0], hi = b1 < nlines ? (long)starts[b1] : n;
  // the lane's own line, asked for now: the loads run beside the staging
  const long i = b0 + threadIdx.x;
  long pos = 0, end = 0;
  if (i < nlines) {
    pos = starts[i];
    // the line's end: its '\n' (the byte before the next line), or the buffer's
    end = i + 1 < nlines ? (long)starts[i + 1] - 1 : (buf[n - 1] == '\n' ? n - 1 : n);
  }
  if (lo < 0) lo = 0;
  if (hi > n) hi = n;
  if (hi < lo) hi = lo;
  const bool staged = hi - lo <= kStageBytes;          // the same in every lane
  const int mis = (int)(reinterpret_cast<uintptr_t>(buf + lo) & 15);
  if (staged) {
    const long nslots = (mis + (hi - lo) + 15) >> 4;
    for (long q = threadIdx.x; q < nslots; q += kThreads) {
      const long g0 = lo - mis + q * 16;               // buf + g0 is 16-byte aligned
      if (g0 >= 0 && g0 + 16 <= n) {
        s_slots[q] = *reinterpret_cast<const uint4*>(buf + g0);
      } else {
        for (int j = 0; j < 16; ++j) s[q * 16 + j] = (g0 + j >= 0 && g0 + j < n) ? buf[g0 + j] : 0;
      }
    }
    __syncthreads();
  }
  uint8_t st = kSkip;
  if (i < nlines) {
    if (pos < lo) pos = lo;
    if (end > hi) end = hi;
    int32_t a = 0, b = 0;
    if (staged) {
      st = parse_line(s, (int)(pos - lo + mis), (int)(end - lo + mis), &a, &b);
    } else {
      st = parse_line(buf, (int)pos, (int)end, &a, &b);
    }
    status[i] = st;
    keys[i] = st == kRecord ? (int64_t)pair_key(a, b) : 0;
    if (st == kIrregular) atomicOr(irregular, 1);
  }
  const uint32_t total = block_reduce_add(st == kRecord ? 1u : 0u, s_w);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void intpair_compact_kernel(
    const uint8_t* __restrict__ status, const int64_t* __restrict__ keys, long nlines,
    const long* __restrict__ block_base, long nrecords, int64_t* __restrict__ out) {
  __shared__ uint32_t s_w[kScanWaves];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool rec = i < nlines && status[i] == kRecord;
  const long at = block_base[blockIdx.x] + block_excl_scan(rec ? 1u : 0u, s_w);
  if (rec && at < nrecords) out[at] = keys[i];
}

__device__ __forceinline__ int32_t first_of(uint64_t key) {
  return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
}

__device__ __forceinline__ int32_t second_of(uint64_t key) {
  return (int32_t)((uint32_t)key ^ 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void intpair_partition_kernel(
    const int64_t* __restrict__ keys, long n, long nparts, int64_t* __restrict__ parts) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  long v = (long)first_of((uint64_t)keys[i]) * 127;    // |v| < 2^38
  if (v < 0) v = -v;
  parts[i] = v % nparts;
}

// decimal characters of v, the sign included
__device__ __forceinline__ int int_chars(int32_t v) {
  const uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  int d = 1;
  d += u >= 10u;
  d += u >= 100u;
  d += u >= 1000u;
  d += u >= 10000u;
  d += u >= 100000u;
  d += u >= 1000000u;
  d += u >= 10000000u;
  d += u >= 100000000u;
  d += u >= 1000000000u;
  return d + (v < 0);
}

__device__ __forceinline__ bool is_head(const int64_t* __restrict__ keys, long i) {
  return i == 0 || (uint32_t)((uint64_t)keys[i] >> 32) != (uint32_t)((uint64_t)keys[i - 1] >> 32);
}

__global__ __launch_bounds__(kThreads) void intpair_lengths_kernel(
    const int64_t* __restrict__ keys, long n, int32_t* __restrict__ lens) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = (uint64_t)keys[i];
  lens[i] = int_chars(first_of(k)) + int_chars(second_of(k)) + 2 + (is_head(keys, i) ? kSepLen : 0);
}

// A record's text in registers, little-endian: byte j of the text is byte j of
// (w0, w1, w2).  Characters are pushed in front.
struct Text24 {
  uint64_t w0 = 0, w1 = 0, w2 = 0;
  int len = 0;
  __device__ __forceinline__ void push(uint8_t c) {
    w2 = (w2 << 8) | (w1 >> 56);
    w1 = (w1 << 8) | (w0 >> 56);
    w0 = (w0 << 8) | c;
    ++len;
  }
  __device__ __forceinline__ void push_int(int32_t v) {
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
#pragma unroll
    for (int d = 0; d < 10; ++d) {                     // an int32 has at most 10 digits
      push((uint8_t)('0' + u % 10u));
      u /= 10u;
      if (u == 0) break;
    }
    if (v < 0) push('-');
  }
  __device__ __forceinline__ uint8_t at(int j) const {
    return (uint8_t)(j < 8 ? w0 >> (8 * j) : j < 16 ? w1 >> (8 * (j - 8)) : w2 >> (8 * (j - 16)));
  }
};

// offs[n + 1]: the exclusive scan of intpair_lengths
__global__ __launch_bounds__(kThreads) void intpair_fill_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ offs, long n,
    uint8_t* __restrict__ dst) {
  __shared__ uint4 s_slots[kRunSlots];
  uint8_t* s = reinterpret_cast<uint8_t*>(s_slots);
  const long r0 = (long)blockIdx.x * kThreads;
  const long r1 = r0 + kThreads < n ? r0 + kThreads : n;
  const long o0 = offs[r0];
  long span = offs[r1] - o0;
  if (span < 0) span = 0;
  if (span > kRunMax) span = kRunMax;                  // (lengths from intpair_lengths never exceed it)
  const int mis = (int)(reinterpret_cast<uintptr_t>(dst + o0) & 15);
  const long total = mis + span;                       // LDS byte x is dst[o0 - mis + x]
  const long i = r0 + threadIdx.x;
  if (i < r1) {
    const uint64_t k = (uint64_t)keys[i];
    Text24 t;
    t.push('\n');
    t.push_int(second_of(k));
    t.push('\t');
    t.push_int(first_of(k));
    long x = offs[i] - o0 + mis;
    if (is_head(keys, i)) {
      for (int j = 0; j < kSepLen; ++j, ++x)
        if (x >= mis && x < total) s[x] = j < kSepLen - 1 ? '-' : '\n';
    }
    for (int j = 0; j < t.len; ++j, ++x)
      if (x >= mis && x < total) s[x] = t.at(j);
  }
  __syncthreads();
  uint8_t* base = dst + o0 - mis;                      // 16-byte aligned
  const long nslots = (total + 15) >> 4;
  for (long q = threadIdx.x; q < nslots; q += kThreads) {
    const long b = q * 16 < mis ? mis : q * 16;
    const long e = q * 16 + 16 < total ? q * 16 + 16 : total;
    if (e - b == 16) {
      *reinterpret_cast<uint4*>(base + q * 16) = s_slots[q];
    } else {
      for (long x = b; x < e; ++x) base[x] = s[x];
    }
  }
}

inline bool grid_fits(long blocks) { return blocks < (1L << 31); }

}  // namespace

extern "C" {

long hbmr_intpair_tiles(long n) { return n <= 0 ? 0 : ceil_div(n, kTile); }

// tile_counts[hbmr_intpair_tiles(n)]: the '\n' bytes of each tile of buf[0, n)
// (any alignment, n < 2^31); *non_ascii |= 1 if a byte is >= 0x80
int hbmr_intpair_lines_count(const uint8_t* buf, long n, uint32_t* tile_counts, int* non_ascii,
                             hipStream_t st) {
  const long tiles = hbmr_intpair_tiles(n);
  if (tiles == 0) return 0;
  if (n >= (1L << 31) || buf == nullptr || tile_counts == nullptr || non_ascii == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_lines_count_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, buf,
                     n, tile_counts, non_ascii);
  return (int)hipGetLastError();
}

// starts[nlines]: the first byte of each line; tile_base: the exclusive scan of
// tile_counts; nlines = newlines + (the last byte is not '\n')
int hbmr_intpair_lines_write(const uint8_t* buf, long n, const long* tile_base, long nlines,
                             int32_t* starts, hipStream_t st) {
  const long tiles = hbmr_intpair_tiles(n);
  if (tiles == 0 || nlines <= 0) return 0;
  if (n >= (1L << 31) || nlines > n || buf == nullptr || tile_base == nullptr || starts == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_lines_write_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, buf,
                     n, tile_base, nlines, starts);
  return (int)hipGetLastError();
}

long hbmr_intpair_blocks(long n) { return n <= 0 ? 0 : ceil_div(n, kThreads); }

// Per line of buf[0, n) (starts[nlines], ascending, inside the buffer): status 0
// skip, 1 record, 2 irregular, and the record's key (else 0).
// block_counts[hbmr_intpair_blocks(nlines)]: the records of each 256 lines.
// *irregular |= 1 if a line is irregular.
int hbmr_intpair_parse(const uint8_t* buf, long n, const int32_t* starts, long nlines,
                       uint8_t* status, int64_t* keys, uint32_t* block_counts, int* irregular,
                       hipStream_t st) {
  if (nlines <= 0) return 0;
  if (n <= 0 || n >= (1L << 31) || nlines > n || buf == nullptr || starts == nullptr ||
      status == nullptr || keys == nullptr || block_counts == nullptr || irregular == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_parse_kernel, dim3((unsigned)hbmr_intpair_blocks(nlines)),
                     dim3(kThreads), 0, st, buf, n, starts, nlines, status, keys, block_counts,
                     irregular);
  return (int)hipGetLastError();
}

// out[nrecords]: the keys of the lines of status 1, in line order; block_base:
// the exclusive scan of intpair_parse's block_counts
int hbmr_intpair_compact(const uint8_t* status, const int64_t* keys, long nlines,
                         const long* block_base, long nrecords, int64_t* out, hipStream_t st) {
  if (nlines <= 0 || nrecords <= 0) return 0;
  if (nlines >= (1L << 31) || nrecords > nlines || block_base == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_compact_kernel, dim3((unsigned)hbmr_intpair_blocks(nlines)),
                     dim3(kThreads), 0, st, status, keys, nlines, block_base, nrecords, out);
  return (int)hipGetLastError();
}

// parts[n] = abs(first * 127) % nparts of each key (FirstPartitioner, in 64 bits)
int hbmr_intpair_partition(const int64_t* keys, long n, long nparts, int64_t* parts,
                           hipStream_t st) {
  if (n <= 0) return 0;
  if (nparts <= 0 || !grid_fits(hbmr_intpair_blocks(n))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_partition_kernel, dim3((unsigned)hbmr_intpair_blocks(n)),
                     dim3(kThreads), 0, st, keys, n, nparts, parts);
  return (int)hipGetLastError();
}

// lens[n]: the output bytes of each record of a part (keys sorted): its line,
// and in front of a group head the separator line
int hbmr_intpair_lengths(const int64_t* keys, long n, int32_t* lens, hipStream_t st) {
  if (n <= 0) return 0;
  if (!grid_fits(hbmr_intpair_blocks(n))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_lengths_kernel, dim3((unsigned)hbmr_intpair_blocks(n)),
                     dim3(kThreads), 0, st, keys, n, lens);
  return (int)hipGetLastError();
}

// dst[offs[i] : offs[i + 1]) = the text of record i; offs[n + 1] is the exclusive
// scan of hbmr_intpair_lengths over the same keys and dst holds offs[n] bytes
// (the caller checks).  No other byte of dst is written.
int hbmr_intpair_fill(const int64_t* keys, const int64_t* offs, long n, uint8_t* dst,
                      hipStream_t st) {
  if (n <= 0) return 0;
  if (!grid_fits(hbmr_intpair_blocks(n)) || offs == nullptr || dst == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(intpair_fill_kernel, dim3((unsigned)hbmr_intpair_blocks(n)), dim3(kThreads),
                     0, st, keys, offs, n, dst);
  return (int)hipGetLastError();
}

}  // extern "C"
