// Raw Snappy decode on the device: one wave per raw stream ("chunk") of a
// Hadoop-framed Snappy file.  The host lists the chunks from the framing's
// headers (native/io/snappyindex.cc); chunk c of the int64[4, n] table is
// (offset of the raw stream in src, its compressed length, offset of its
// output in dst, its uncompressed length).  The decoder is the twin of
// hbmr_snappy_decompress (native/io/snappy.cc): it takes any valid stream
// (every literal and copy form, copies reaching back across 64 KiB fragments,
// overlapping runs) and rejects what the host decoder rejects, with a nonzero
// code in status[c] and no access outside the chunk's two ranges.
//
// Shape of a wave's work.  The stream position is wave-uniform.  The wave
// holds 512 bytes of the compressed stream in two registers a lane (a
// sliding window, refilled a half at a time, every load checked against the
// chunk's end); tags, lengths and offsets are read out of it with v_readlane,
// so the whole parse is scalar work and touches no memory.  The 64 lanes move
// the bytes, one element a step: an element of up to 64 bytes is one byte a
// lane, a longer literal goes in destination-aligned 16-byte slots
// (bytes/records.h).  (A second shape was measured against this one and
// deleted: up to 8 short elements parsed ahead, then one load and one store of
// the whole batch with lane i taking the batch's byte i.  It saved no time on
// int-pair lines and lost 20 % on word text — profiles/snappy_1gpu.json, "ab":
// the per-lane choice among 8 sources costs more than the stores it merges,
// and what bounds a wave is the load-to-store round trip of each step, which
// a batch of copies that read recent output does not shorten.)
#include "bytes/records.h"

namespace {

constexpr int kHalf = 256;   // bytes of the stream one window register holds across the wave

enum : int {
  kBadPreamble = 1,   // no varint, or not the table's uncompressed length
  kTruncated = 2,     // an element's operand or literal runs past the stream
  kBadOffset = 3,     // a copy with offset 0 or past the bytes produced
  kOverrun = 4,       // an element would write past the uncompressed length
  kShort = 5,         // the stream ends before the uncompressed length
};

// Four bytes of the stream at [a, a + 4) for the window; bytes at or past the
// chunk's end `hi` are not read and stand as 0 (a >= 0: the window only moves
// forward from the chunk's start).
__device__ __forceinline__ uint32_t window_dword(const uint8_t* in, long a, long hi) {
  uint32_t v = 0;
  if (a + 4 <= hi) {
    __builtin_memcpy(&v, in + a, 4);
  } else {
    for (int j = 0; j < 4; ++j)
      if (a + j < hi) v |= (uint32_t)in[a + j] << (8 * j);
  }
  return v;
}

// At least five bytes of the window from byte idx on (idx wave-uniform, in
// [0, kHalf)), lowest first.
__device__ __forceinline__ uint64_t window_bits(uint32_t w0, uint32_t w1, int idx) {
  const int d = idx >> 2;
  const uint32_t lo = __builtin_amdgcn_readlane(w0, d);
  const uint32_t hi = d + 1 < 64 ? __builtin_amdgcn_readlane(w0, (d + 1) & 63)
                                 : __builtin_amdgcn_readlane(w1, 0);
  return (((uint64_t)hi << 32) | lo) >> (8 * (idx & 3));
}

struct Elem {
  int err;      // 0, or the violation
  bool lit;
  int hdr;      // tag and operand bytes
  long len;     // bytes produced
  long off;     // a copy's offset
};

// One element from its first five bytes, checked against what is left of the
// stream (in_left >= 1, counted from the tag), the bytes produced so far (op)
// and the uncompressed length: the checks of hbmr_snappy_decompress, all before
// any byte moves.
__device__ __forceinline__ Elem parse_element(uint64_t bits, long in_left, long op, long ulen) {
  Elem e;
  e.err = 0;
  e.off = 0;
  const uint32_t tag = (uint32_t)bits & 0xff;
  const int kind = tag & 3;
  e.lit = kind == 0;
  if (e.lit) {
    long len = tag >> 2;
    int nb = 0;
    if (len >= 60) {
      nb = (int)len - 59;
      if (in_left - 1 < nb) {
        e.err = kTruncated;
        return e;
      }
      len = (long)((bits >> 8) & (0xffffffffull >> (8 * (4 - nb))));
    }
    e.hdr = 1 + nb;
    e.len = len + 1;
    if (in_left - e.hdr < e.len) e.err = kTruncated;
    else if (ulen - op < e.len) e.err = kOverrun;
    return e;
  }
  const int nb = kind == 1 ? 1 : kind == 2 ? 2 : 4;
  e.hdr = 1 + nb;
  if (in_left - 1 < nb) {
    e.err = kTruncated;
    return e;
  }
  if (kind == 1) {
    e.len = 4 + ((tag >> 2) & 7);
    e.off = (long)(((tag >> 5) << 8) | ((uint32_t)(bits >> 8) & 0xff));
  } else {
    e.len = 1 + (tag >> 2);
    e.off = kind == 2 ? (long)((bits >> 8) & 0xffff) : (long)((bits >> 8) & 0xffffffffull);
  }
  if (e.off == 0 || e.off > op) e.err = kBadOffset;
  else if (ulen - op < e.len) e.err = kOverrun;
  return e;
}

// A copy element reads bytes of `out` that other lanes of this wave stored while
// executing earlier elements, possibly the one just before.  Program order
// orders a lane's accesses against its own only: lane i's load of a byte lane j
// stored is ordered by nothing, and a wave's vector stores and loads complete
// out of order with one another.  So before such a load the wave waits until
// every store it has issued is complete (vmcnt(0): on gfx9 a store leaves the
// counter when the write is acknowledged), as a workgroup-scope release, and
// takes a workgroup-scope acquire after it.  That is the hand-off between two
// waves of a workgroup, here between two lanes of one wave: both sit on one CU
// and share its write-through vector L1, which is coherent for the CU's own
// stores, so no cache invalidate is needed at this scope.  The wave-scope
// fences that would cost nothing emit no wait at all and are not enough.
// Everything read from `out` is a per-lane vector load (global_load_ubyte); the
// scalar cache is not coherent with vector stores, and nothing of `out` goes
// through it.  The caller tracks how far the output is drained and comes here
// only when a source reaches past that.
__device__ __forceinline__ void drain_stores() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Decode the raw stream in[0, clen) into out[0, ulen).  Returns 0, or the first
// violation; then the bytes of out are unspecified, and nothing outside either
// range was read or written.
__device__ __forceinline__ int decode_chunk(const uint8_t* in, long clen, uint8_t* out, long ulen,
                                            int lane) {
  long wb = 0;                                   // stream offset of the window
  uint32_t w0 = window_dword(in, 4L * lane, clen);
  uint32_t w1 = window_dword(in, kHalf + 4L * lane, clen);

  // the varint preamble
  long ip = -1;
  {
    const uint64_t bits = window_bits(w0, w1, 0);
    uint32_t want = 0;
    for (int i = 0; i < 5 && i < clen; ++i) {
      const uint32_t b = (uint32_t)(bits >> (8 * i)) & 0xff;
      want |= (b & 0x7f) << (7 * i);
      if (!(b & 0x80)) {
        if (!(i == 4 && b > 0x0f)) ip = i + 1;
        break;
      }
    }
    if (ip < 0 || (long)want != ulen) return kBadPreamble;
  }

  long op = 0;        // bytes produced
  long drained = 0;   // out[0, drained) is complete in memory: drain_stores() ran at op == drained
  while (ip < clen) {
    if (ip - wb >= kHalf) {                      // slide the window: ip - wb < kHalf after it
      if (ip - wb < 2 * kHalf) {
        w0 = w1;
        wb += kHalf;
      } else {                                   // a long literal jumped past it
        wb = ip;
        w0 = window_dword(in, wb + 4L * lane, clen);
      }
      w1 = window_dword(in, wb + kHalf + 4L * lane, clen);
    }

    const Elem e = parse_element(window_bits(w0, w1, (int)(ip - wb)), clen - ip, op, ulen);
    if (e.err) return e.err;
    ip += e.hdr;
    if (e.lit) {
      if (e.len <= 64) {
        if (lane < e.len) out[op + lane] = in[ip + lane];
      } else {
        // destination-aligned 16-byte slots, four 256-byte chunks of them a step
        const long mis = (long)(reinterpret_cast<uintptr_t>(out + op) & 15);
        const long nchunk = (mis + e.len + kCopyChunk - 1) / kCopyChunk;
        const uint8_t* s = in + ip;
        for (long c = lane / kCopyLanes; c < nchunk; c += 64 / kCopyLanes)
          copy_slot(out, op, op + e.len, c, lane % kCopyLanes, [&] { return s; });
      }
      ip += e.len;
    } else {
      // (e.len <= 64: one byte a lane.)  A run, off < len, repeats its off
      // source bytes; all of them were stored before this element began.
      const long first = op - e.off;
      const long last = first + (e.off < e.len ? e.off : e.len);
      if (last > drained) {
        drain_stores();
        drained = op;
      }
      if (lane < e.len) {
        const long j = e.off >= e.len ? lane : lane % (int)e.off;
        out[op + lane] = out[first + j];
      }
    }
    op += e.len;
  }
  return op == ulen ? 0 : kShort;
}

__global__ __launch_bounds__(64) void snappy_decode_kernel(const uint8_t* src,
                                                           const long* __restrict__ table, long n,
                                                           uint8_t* dst, int* __restrict__ status) {
  const long c = blockIdx.x;
  const int lane = threadIdx.x;
  const int err = decode_chunk(src + table[c], table[n + c], dst + table[2 * n + c],
                               table[3 * n + c], lane);
  if (lane == 0) status[c] = err;
}

}  // namespace

extern "C" {

// Decode n_chunks raw Snappy streams of src into dst by the int64[4, n_chunks]
// table (see the top); status[c] (int32) gets 0 or chunk c's violation.  The
// caller has checked the table's ranges against both buffers: the kernel keeps
// every access inside a chunk's ranges, whatever the stream holds.
int hbmr_snappy_decode(const void* src, const void* table, long n_chunks, void* dst, void* status,
                       void* stream) {
  if (n_chunks <= 0) return 0;
  if (n_chunks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_chunks), block(64);
  hipLaunchKernelGGL(snappy_decode_kernel, grid, block, 0, st, (const uint8_t*)src,
                     (const long*)table, n_chunks, (uint8_t*)dst, (int*)status);
  return (int)hipGetLastError();
}

}  // extern "C"
