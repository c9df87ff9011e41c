// Snappy-compressed SequenceFile splits on the device (hbmr/ops/seqz.py): what
// turns the columns of BLOCK-compressed blocks, decoded by snappydec.hip into a
// scratch "columns" buffer, and the in-place decoded values of RECORD-compressed
// records into the (data, index) of an uncompressed split: frames
// [recordLen][keyLen][key][value] back to back and, per record, the offset and
// length of its frame and of its key payload.
//
// The host (native/io/seqzindex.cc) lists per block (int64[10, nb], row-major)
// the record count, the record base and the offset and decoded length of the
// four columns — key lengths, keys, value lengths, values — in the columns
// buffer, and has checked those ranges.  Everything read OUT of a column is
// checked here before it is used as a length or an offset.
//
//  1. seqblock_vint: the two length columns of every block (n Hadoop vints
//     each) into per-record key and value lengths at the block's record base,
//     with a per-block status.
//  2. seqblock_index: per record the four index rows from its lengths and its
//     offsets (scans on the caller's side); the key payload from the key's
//     first bytes as recindex.cc takes it from a frame.
//  3. seqblock_assemble: per record the 8-byte header, the key piece and the
//     value piece at the frame's offset, in the destination-aligned 16-byte
//     slots of bytes/records.h.  Without a value source it writes header and
//     key only (RECORD mode, whose values the decoder wrote in place).
#include "bytes/records.h"

namespace {

constexpr int kThreads = 256;

// status bits of a block
enum : int {
  kMidVint = 1,     // a length column ends inside a vint
  kCount = 2,       // fewer or more than n vints, or column bytes left over
  kRange = 4,       // a length negative or >= 2^31
  kSum = 8,         // the lengths do not add up to the decoded keys / values column
  kKeyPrefix = 16,  // a BytesWritable / Text prefix inconsistent with the key's length
};

struct Blocks {
  const int64_t* t;
  long nb;
  __device__ long n(long b) const { return t[b]; }
  __device__ long base(long b) const { return t[nb + b]; }
  __device__ long off(long b, int col) const { return t[(2 + 2 * col) * nb + b]; }
  __device__ long len(long b, int col) const { return t[(3 + 2 * col) * nb + b]; }
};

// bytes of the vint whose first byte is fb (1..9)
__device__ __forceinline__ int vint_size(int fb) {
  return fb >= -112 ? 1 : (fb < -120 ? 1 - (fb + 120) : 1 - (fb + 112));
}

// The value of the vint at p (its `size` bytes lie inside the column): -1 for a
// negative one or one of 2^31 and above.
__device__ __forceinline__ long vint_length(const uint8_t* p, int fb, int size) {
  if (size == 1) return fb < 0 ? -1 : fb;
  if (fb < -120) return -1;
  uint64_t v = 0;
  for (int i = 1; i < size; ++i) v = (v << 8) | p[i];
  return v > 0x7fffffffull ? -1 : (long)v;
}

// One wave per (block, length column).  The wave holds a window of 64 column
// bytes that begins at a vint: every lane takes its byte as a candidate first
// byte and knows where the vint after it would begin; the true chain from lane
// 0 is marked by pointer jumping (six doublings over a 64-byte LDS row), a
// marked lane's rank among the marked is its record, and the chain's exit is
// the next window's start.
__global__ __launch_bounds__(64) void seqblock_vint_kernel(const uint8_t* __restrict__ cols,
                                                           Blocks blk, int64_t* __restrict__ klen,
                                                           int64_t* __restrict__ vlen,
                                                           int* __restrict__ status) {
  __shared__ uint8_t s_mark[64];
  const long b = blockIdx.x >> 1;
  const int which = blockIdx.x & 1;              // 0: key lengths, 1: value lengths
  const int lane = threadIdx.x;
  const uint8_t* col = cols + blk.off(b, 2 * which);
  const long len = blk.len(b, 2 * which);
  const long n = blk.n(b);
  int64_t* out = (which ? vlen : klen) + blk.base(b);

  long pos = 0, rec = 0;
  unsigned long long sum = 0;
  int err = 0;
  while (pos < len) {
    const long i = pos + lane;
    const int fb = i < len ? (int)(int8_t)col[i] : 0;
    const int size = vint_size(fb);
    int jump = lane + size < 64 ? lane + size : 64;
    s_mark[lane] = lane == 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const bool m = s_mark[lane];
      __syncthreads();
      if (m && jump < 64) s_mark[jump] = 1;
      const int j2 = __shfl(jump, jump & 63);
      jump = jump < 64 ? j2 : 64;
      __syncthreads();
    }
    const bool mark = s_mark[lane] && i < len;
    __syncthreads();
    const unsigned long long marks = __ballot(mark);       // lane 0 is in it: pos < len
    const long r = rec + __popcll(marks & ((1ull << lane) - 1));
    if (mark) {
      if (i + size > len) {
        err |= kMidVint;
      } else if (r >= n) {
        err |= kCount;
      } else {
        const long v = vint_length(col + i, fb, size);
        if (v < 0) err |= kRange;
        out[r] = v < 0 ? 0 : v;
        sum += v < 0 ? 0 : (unsigned long long)v;
      }
    }
    const int last = 63 - __builtin_clzll(marks);
    pos += __shfl(lane + size, last);
    rec += __popcll(marks);
    if (__any(err)) break;
  }
  if (rec != n) err |= kCount;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (!err && sum != (unsigned long long)blk.len(b, 2 * which + 1)) err |= kSum;
  if (err) atomicOr(&status[b], err);
}

// Index rows of record r from its frame offset and lengths; the key payload
// from the first bytes of the key at cols[ksrc[r]].  prefix 4: BytesWritable, 0:
// Text.  A key outside the columns buffer or with a bad prefix sets its block's
// status and gets an empty payload.
__global__ __launch_bounds__(kThreads) void seqblock_index_kernel(
    const uint8_t* __restrict__ cols, long cols_bytes, const int64_t* __restrict__ foff,
    const int64_t* __restrict__ klen, const int64_t* __restrict__ vlen,
    const int64_t* __restrict__ ksrc, const int64_t* __restrict__ rec_block, long n, int prefix,
    int64_t* __restrict__ index, int* __restrict__ status) {
  const long r = (long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const long a = foff[r], kl = klen[r], vl = vlen[r], ks = ksrc[r];
  long poff = 0, plen = -1;
  if (kl >= 0 && ks >= 0 && ks + kl <= cols_bytes) {
    const uint8_t* k = cols + ks;
    if (prefix) {
      if (kl >= 4) {
        poff = 4;
        plen = (long)(((uint32_t)k[0] << 24) | ((uint32_t)k[1] << 16) | ((uint32_t)k[2] << 8) | k[3]);
      }
    } else if (kl >= 1) {
      const int fb = (int)(int8_t)k[0];
      poff = vint_size(fb);
      if (poff <= kl) plen = vint_length(k, fb, (int)poff);
    }
    if (plen < 0 || poff + plen != kl) plen = -1;
  }
  if (plen < 0) {
    atomicOr(&status[rec_block[r]], kKeyPrefix);
    poff = plen = 0;
  }
  index[r] = a;
  index[n + r] = 8 + kl + vl;
  index[2 * n + r] = a + 8 + poff;
  index[3 * n + r] = plen;
}

struct Piece {
  const uint8_t* base;      // nullptr: no such piece
  long bytes;               // of the buffer at base
  const int64_t* off;       // per record, in that buffer
};

// 16 lanes per record: lane 0 writes [recordLen][keyLen] big-endian, then the
// lanes copy the key and the value, a chunk of 16 destination-aligned slots a
// step (copy_slot).  A record whose frame or sources do not lie inside their
// buffers is left out.
__global__ __launch_bounds__(kThreads) void seqblock_assemble_kernel(
    Piece key, Piece val, const int64_t* __restrict__ foff, const int64_t* __restrict__ klen,
    const int64_t* __restrict__ vlen, long n, uint8_t* __restrict__ dst, long dst_bytes) {
  const long r = (long)blockIdx.x * (kThreads / kCopyLanes) + threadIdx.x / kCopyLanes;
  if (r >= n) return;
  const int lane = threadIdx.x % kCopyLanes;
  const long a = foff[r], kl = klen[r], vl = vlen[r];
  if (a < 0 || kl < 0 || vl < 0 || kl + vl > 0x7fffffffL - 8 || a + 8 + kl + vl > dst_bytes) return;
  const long ks = key.off[r], vs = val.base != nullptr ? val.off[r] : 0;
  if (ks < 0 || ks + kl > key.bytes) return;
  if (val.base != nullptr && (vs < 0 || vs + vl > val.bytes)) return;
  if (lane == 0) {
    const uint32_t h0 = (uint32_t)(kl + vl), h1 = (uint32_t)kl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dst[a + j] = (uint8_t)(h0 >> (24 - 8 * j));
      dst[a + 4 + j] = (uint8_t)(h1 >> (24 - 8 * j));
    }
  }
  const long k0 = a + 8, v0 = k0 + kl;
  const long kch = ((long)(reinterpret_cast<uintptr_t>(dst + k0) & 15) + kl + kCopyChunk - 1) / kCopyChunk;
  for (long c = 0; c < kch; ++c) copy_slot(dst, k0, k0 + kl, c, lane, [&] { return key.base + ks; });
  if (val.base == nullptr) return;
  const long vch = ((long)(reinterpret_cast<uintptr_t>(dst + v0) & 15) + vl + kCopyChunk - 1) / kCopyChunk;
  for (long c = 0; c < vch; ++c) copy_slot(dst, v0, v0 + vl, c, lane, [&] { return val.base + vs; });
}

int launch_assemble(Piece key, Piece val, const int64_t* foff, const int64_t* klen,
                    const int64_t* vlen, long n, uint8_t* dst, long dst_bytes, hipStream_t st) {
  if (n <= 0) return 0;
  if (n >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(seqblock_assemble_kernel, dim3((unsigned)ceil_div(n, kThreads / kCopyLanes)),
                     dim3(kThreads), 0, st, key, val, foff, klen, vlen, n, dst, dst_bytes);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// klen / vlen (int64, one slot per record of all blocks) from the length
// columns of the nb blocks of `blocks` (int64[10, nb], see the top) in cols;
// status[nb] (int32) is cleared, then gets each block's bits.  A block writes
// only its own n slots.
int hbmr_seqblock_vint(const uint8_t* cols, const int64_t* blocks, long nb, int64_t* klen,
                       int64_t* vlen, int* status, hipStream_t st) {
  if (nb <= 0) return 0;
  if (nb >= (1L << 30)) return (int)hipErrorInvalidValue;
  HBMR_RETURN_IF_ERROR(hipMemsetAsync(status, 0, 4 * (size_t)nb, st));
  hipLaunchKernelGGL(seqblock_vint_kernel, dim3((unsigned)(2 * nb)), dim3(64), 0, st, cols,
                     Blocks{blocks, nb}, klen, vlen, status);
  return (int)hipGetLastError();
}

// index (int64[4, n]) of n records from foff, klen, vlen and ksrc (the key's
// offset in cols, a buffer of cols_bytes); rec_block[r]: the status slot of
// record r's block.
int hbmr_seqblock_index(const uint8_t* cols, long cols_bytes, const int64_t* foff,
                        const int64_t* klen, const int64_t* vlen, const int64_t* ksrc,
                        const int64_t* rec_block, long n, int prefix, int64_t* index, int* status,
                        hipStream_t st) {
  if (n <= 0) return 0;
  if (n >= (1L << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(seqblock_index_kernel, dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads),
                     0, st, cols, cols_bytes, foff, klen, vlen, ksrc, rec_block, n, prefix, index,
                     status);
  return (int)hipGetLastError();
}

// The frames of n records into dst[0, dst_bytes): header, key (kbase[ksrc[r]],
// klen[r] bytes of a buffer of kbytes) and value (vbase[vsrc[r]], vlen[r] bytes
// of a buffer of vbytes) at foff[r].
int hbmr_seqblock_assemble(const uint8_t* kbase, long kbytes, const int64_t* ksrc,
                           const uint8_t* vbase, long vbytes, const int64_t* vsrc,
                           const int64_t* foff, const int64_t* klen, const int64_t* vlen, long n,
                           uint8_t* dst, long dst_bytes, hipStream_t st) {
  if (n > 0 && (kbase == nullptr || vbase == nullptr)) return (int)hipErrorInvalidValue;
  return launch_assemble(Piece{kbase, kbytes, ksrc}, Piece{vbase, vbytes, vsrc}, foff, klen, vlen,
                         n, dst, dst_bytes, st);
}

// The same without the value piece: header and key only; vlen goes into the
// header (RECORD mode: the values are in place already).
int hbmr_seqblock_heads(const uint8_t* kbase, long kbytes, const int64_t* ksrc,
                        const int64_t* foff, const int64_t* klen, const int64_t* vlen, long n,
                        uint8_t* dst, long dst_bytes, hipStream_t st) {
  if (n > 0 && kbase == nullptr) return (int)hipErrorInvalidValue;
  return launch_assemble(Piece{kbase, kbytes, ksrc}, Piece{nullptr, 0, nullptr}, foff, klen, vlen,
                         n, dst, dst_bytes, st);
}

}  // extern "C"
