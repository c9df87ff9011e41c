// Record generator kernels: RandomWriter's and RandomTextWriter's records written
// straight into a SequenceFile body in HBM (hbmr/ops/recgen.py holds the
// definition and the CPU twin; hbmr/models/randomwrite.py is the job).  The
// mirror image of recsort_gather and recvalidate_digest: a write-only fill of
// variable-length frames at arbitrary byte alignment, headers and payload
// interleaved, the 20-byte sync holes between frames left alone.
//
// Counter-based, so any byte is computable alone.  With mix64 the splitmix64
// finaliser, lo32/hi32 the halves of a word and mulhi32(x, r) = (x * r) >> 32:
//   S      = mix64(seed + (map + 1) * 0x9E3779B97F4A7C15)     (the host passes S)
//   R(i)   = mix64(S + (i + 1) * 0xD6E8FEB86659FD93)          i: record of the map
//   B(i,t) = mix64(R(i) + (t + 1) * 0x94D049BB133111EB)       t: 0 key, 1 value
//   w32(j) = word j of stream t from a = lo32(B), b = hi32(B): two 32-bit multiplies
// Bytes records: lengths min + mulhi32(lo32/hi32(R), range); payload bytes
// 4j..4j+3 are w32(j) little-endian; frame [8+kl+vl][4+kl][kl][key][vl][value],
// integers big-endian.  Text records: word counts from R the same way, word k
// of a stream is vocabulary[mulhi32(w32(k), V)], the words joined by one space;
// frame [recLen][keyLen][vint(kl)][key][vint(vl)][value].
//
//  1. recgen_lengths: one thread per record.  Bytes: the two mulhi32.  Text: the
//     word counts and the payload lengths as a sum over the words' lengths, from a
//     word-offset table in LDS.
//  2. recgen_fill_bytes: recsort_gather's scheme.  A frame is cut into chunks of
//     its DESTINATION-aligned 16-byte slots (bytes/records.h), 16 lanes take a
//     chunk, a chunk -> record table replaces any search.  A slot is composed in
//     registers from whichever of the four big-endian header integers and the two
//     payload streams it covers (a payload slot is five w32 words shifted by the
//     payload's offset within the slot) and goes out as one aligned 16-byte
//     store (a slot inside one payload, which most are, skips the masks and the
//     header); the partial slots at a frame's head and tail are written bytewise,
//     never past the frame.  A lane takes kGenSlots slots of its chunk, 256 bytes
//     apart, so the three mix64 of a record (R and the two B) are paid once per
//     four slots: per slot they cost more multiplies than the slot's five w32.
//  3. recgen_fill_text: the vocabulary lies in LDS as a byte blob plus word
//     offsets.  16 lanes take a record; 16 words a step, a lane computes its
//     word's id from w32 (ids are recomputed, never stored), the group scans the
//     word lengths for the payload offsets, and each lane writes its word and the
//     space in front of it bytewise.  The header integers and the two vint
//     prefixes go bytewise too.  Every store is checked against the frame's end.
//     (Frames composed in LDS and copied out in aligned 16-byte slots ran at half
//     this kernel's rate, the 2 KiB per record of LDS costing the occupancy that
//     hides the word lookups: profiles/randomwriter_1gpu.json.)
#include "common.h"
#include "../include/hbmr/hbmr.h"
#include "bytes/records.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGenSlots = 4;                          // slots a lane fills of its chunk
constexpr int kGenChunk = kGenSlots * kCopyChunk;     // bytes of a fill chunk
constexpr int kTextLanes = 16;                        // lanes per text record
constexpr int kTextGroups = kThreads / kTextLanes;
constexpr int kMaxWords = 1024;                       // vocabulary limits (LDS)
constexpr int kMaxVocabBytes = 16384;
constexpr int kMaxBlocks = 2048;                      // the text groups stride over the records beyond
constexpr uint64_t kRecMul = 0xD6E8FEB86659FD93ull;
constexpr uint64_t kStreamMul = 0x94D049BB133111EBull;

__device__ __forceinline__ uint64_t rec_word(uint64_t S, long i) {
  return mix64(S + (uint64_t)(i + 1) * kRecMul);
}

__device__ __forceinline__ uint64_t stream_word(uint64_t R, int t) {
  return mix64(R + (uint64_t)(t + 1) * kStreamMul);
}

__device__ __forceinline__ uint32_t w32(uint32_t a, uint32_t b, uint32_t j) {
  uint32_t x = a + j;
  x ^= x >> 16;
  x *= 0x21F0AAADu;
  x ^= b;
  x ^= x >> 15;
  x *= 0x735A2D97u;
  x ^= x >> 15;
  return x;
}

// ---------------------------------------------------------------- slot composition
// A slot as two little-endian words (lo: bytes 0-7, hi: bytes 8-15); the parts
// of a slot are OR-ed together.
struct Slot {
  uint64_t lo, hi;
};

__device__ __forceinline__ Slot operator|(Slot x, Slot y) { return Slot{x.lo | y.lo, x.hi | y.hi}; }

// 0xff in the bytes [from, to) of a word, clipped to the word
__device__ __forceinline__ uint64_t byte_mask(int from, int to) {
  from = from < 0 ? 0 : from;
  to = to > 8 ? 8 : to;
  if (from >= to) return 0;
  const uint64_t below_to = to == 8 ? ~0ull : (1ull << (8 * to)) - 1;
  return below_to & ~((1ull << (8 * from)) - 1);       // from < to <= 8
}

// what the slot at frame offset p holds of the big-endian int v at frame offset h
__device__ __forceinline__ Slot be32_part(uint32_t v, long p, long h) {
  const long d = h - p;                                // slot byte of the int's first byte
  if (d <= -4 || d >= 16) return Slot{0, 0};
  const uint64_t x = __builtin_bswap32(v);             // memory order in a little-endian word
  const int sd = 8 * (int)d;
  return Slot{d < 0 ? x >> -sd : d < 8 ? x << sd : 0,
              d >= 8 ? x << (sd - 64) : d > 4 ? x >> (64 - sd) : 0};   // past the slot: shifted out
}

// what the slot at frame offset p holds of the payload stream (a, b) that lies
// at the frame offsets [s0, s0 + len)
__device__ __forceinline__ Slot stream_part(uint32_t a, uint32_t b, long p, long s0, long len) {
  const long q = p - s0;                               // stream offset of the slot's byte 0
  if (q + 16 <= 0 || q >= len) return Slot{0, 0};
  const int from = q < 0 ? (int)-q : 0;
  const int to = len - q < 16 ? (int)(len - q) : 16;
  const uint32_t j0 = (uint32_t)(q >> 2);              // floor; words outside the stream are masked
  const int sh = 8 * (int)(q & 3);
  const uint32_t w0 = w32(a, b, j0), w1 = w32(a, b, j0 + 1), w2 = w32(a, b, j0 + 2),
                 w3 = w32(a, b, j0 + 3);
  uint64_t x0 = w0 | (uint64_t)w1 << 32, x1 = w2 | (uint64_t)w3 << 32;
  if (sh) {
    const uint64_t x2 = w32(a, b, j0 + 4);
    x0 = (x0 >> sh) | (x1 << (64 - sh));
    x1 = (x1 >> sh) | (x2 << (64 - sh));
  }
  return Slot{x0 & byte_mask(from, to), x1 & byte_mask(from - 8, to - 8)};
}

// the 16 bytes at offset q of the payload stream (a, b): five words, shifted
__device__ __forceinline__ uint4 stream_slot(uint32_t a, uint32_t b, long q) {
  const uint32_t j0 = (uint32_t)(q >> 2), sh = (uint32_t)(q & 3);
  const uint32_t w0 = w32(a, b, j0), w1 = w32(a, b, j0 + 1), w2 = w32(a, b, j0 + 2),
                 w3 = w32(a, b, j0 + 3), w4 = w32(a, b, j0 + 4);
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                    __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// ---------------------------------------------------------------- bytes records
__global__ __launch_bounds__(kThreads) void recgen_fill_bytes_kernel(
    uint64_t S, long first, const int64_t* __restrict__ foff, const int64_t* __restrict__ flen,
    const int64_t* __restrict__ klen, const int64_t* __restrict__ chunk_base,
    const uint32_t* __restrict__ chunk_entry, long nchunks, uint8_t* __restrict__ dst) {
  const long g = (long)blockIdx.x * (kThreads / kCopyLanes) + (threadIdx.x / kCopyLanes);
  if (g >= nchunks) return;
  const int lane = threadIdx.x % kCopyLanes;
  const long rec = chunk_entry[g];   // chunk g's record: chunk_base[rec] <= g < chunk_base[rec + 1]
  const long c = g - chunk_base[rec];
  const long a = foff[rec], len = flen[rec], kl = klen[rec];
  const long vl = len - 16 - kl;     // the host checked 0 <= kl, 16 + kl <= len
  const uint64_t R = rec_word(S, first + rec);
  const uint64_t bk = stream_word(R, 0), bv = stream_word(R, 1);
#pragma unroll
  for (int u = 0; u < kGenSlots; ++u) {
    long slot, b, e;
    if (!slot_span(dst, a, a + len, c * kGenSlots + u, lane, slot, b, e)) continue;
    const long p = slot - a;         // frame offset of the slot's byte 0: -15 and up
    // a slot inside one payload, which most are: no header, nothing to mask
    const long qv = p - (16 + kl), qk = p - 12;
    if (qv >= 0 && qv + 16 <= vl) {
      *reinterpret_cast<uint4*>(dst + slot) = stream_slot((uint32_t)bv, (uint32_t)(bv >> 32), qv);
      continue;
    }
    if (qk >= 0 && qk + 16 <= kl) {
      *reinterpret_cast<uint4*>(dst + slot) = stream_slot((uint32_t)bk, (uint32_t)(bk >> 32), qk);
      continue;
    }
    const Slot v = be32_part((uint32_t)(8 + kl + vl), p, 0) | be32_part((uint32_t)(4 + kl), p, 4) |
                   be32_part((uint32_t)kl, p, 8) | be32_part((uint32_t)vl, p, 12 + kl) |
                   stream_part((uint32_t)bk, (uint32_t)(bk >> 32), p, 12, kl) |
                   stream_part((uint32_t)bv, (uint32_t)(bv >> 32), p, 16 + kl, vl);
    if (e - b == 16) {
      *reinterpret_cast<ulonglong2*>(dst + slot) = make_ulonglong2(v.lo, v.hi);
    } else {
      for (long x = b; x < e; ++x) {
        const int i = (int)(x - slot);
        dst[x] = (uint8_t)(i < 8 ? v.lo >> (8 * i) : v.hi >> (8 * (i - 8)));
      }
    }
  }
}

// ---------------------------------------------------------------- text records
struct TextParams {
  uint32_t lo_k, range_k, lo_v, range_v;   // word counts: lo + mulhi32(half of R, range)
};

// the word offsets into LDS (nwords + 1 of them; at most kMaxVocabBytes fits 16 bits)
__device__ __forceinline__ void load_offsets(const int32_t* __restrict__ woff, int nwords,
                                             uint16_t* s_off) {
  for (int i = threadIdx.x; i <= nwords; i += kThreads) s_off[i] = (uint16_t)woff[i];
}

__device__ __forceinline__ uint32_t word_id(uint32_t a, uint32_t b, uint32_t k, uint32_t nwords) {
  return __umulhi(w32(a, b, k), nwords);
}

// bytes of the payload of n words of stream B: the words and the spaces between them
__device__ __forceinline__ long words_len(uint64_t B, uint32_t n, const uint16_t* s_off,
                                          uint32_t nwords) {
  const uint32_t a = (uint32_t)B, b = (uint32_t)(B >> 32);
  long s = n ? (long)n - 1 : 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t id = word_id(a, b, k, nwords);
    s += s_off[id + 1] - s_off[id];
  }
  return s;
}

__device__ __forceinline__ int vint_size(long v) {
  return v <= 127 ? 1 : v < 256 ? 2 : v < 65536 ? 3 : v < (1L << 24) ? 4 : 5;
}

// byte i of Hadoop's VInt of v (0 <= v < 2^31)
__device__ __forceinline__ uint8_t vint_byte(long v, int i) {
  const int n = vint_size(v);
  if (n == 1) return (uint8_t)v;
  if (i == 0) return (uint8_t)(0x90 - (n - 1));        // -112 - (data bytes)
  return (uint8_t)(v >> (8 * (n - 1 - i)));
}

// v from vint_size(v) + v
__device__ __forceinline__ long unvint(long rest) {
  if (rest - 1 <= 127) return rest - 1;
  if (rest - 2 < 256) return rest - 2;
  if (rest - 3 < 65536) return rest - 3;
  if (rest - 4 < (1L << 24)) return rest - 4;
  return rest - 5;
}

// out[0..4)[count]: key and value payload lengths, and for text the word counts
__global__ __launch_bounds__(kThreads) void recgen_lengths_kernel(
    uint64_t S, long first, long count, int text, TextParams pr,
    const int32_t* __restrict__ woff, int nwords, int64_t* __restrict__ out) {
  __shared__ uint16_t s_off[kMaxWords + 1];
  if (text) {
    load_offsets(woff, nwords, s_off);
    __syncthreads();
  }
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const uint64_t R = rec_word(S, first + i);
  const uint32_t nk = pr.lo_k + __umulhi((uint32_t)R, pr.range_k);
  const uint32_t nv = pr.lo_v + __umulhi((uint32_t)(R >> 32), pr.range_v);
  if (!text) {
    out[i] = nk;
    out[count + i] = nv;
    out[2 * count + i] = 0;
    out[3 * count + i] = 0;
    return;
  }
  out[i] = words_len(stream_word(R, 0), nk, s_off, (uint32_t)nwords);
  out[count + i] = words_len(stream_word(R, 1), nv, s_off, (uint32_t)nwords);
  out[2 * count + i] = nk;
  out[3 * count + i] = nv;
}

// The 16 lanes of a record write the n words of stream B, joined by spaces, to
// dst[at, ...), nothing at or past `end`.
__device__ __forceinline__ void write_words(uint64_t B, uint32_t n, long at, long end, int lane,
                                            const uint8_t* s_blob, const uint16_t* s_off,
                                            uint32_t nwords, uint8_t* __restrict__ dst) {
  const uint32_t a = (uint32_t)B, b = (uint32_t)(B >> 32);
  uint32_t run = 0;                                    // payload bytes of the words before k0
  for (uint32_t k0 = 0; k0 < n; k0 += kTextLanes) {    // n is the same in the record's lanes
    const uint32_t k = k0 + lane;
    uint32_t from = 0, wl = 0, item = 0;
    if (k < n) {
      const uint32_t id = word_id(a, b, k, nwords);
      from = s_off[id];
      wl = s_off[id + 1] - from;
      item = wl + (k ? 1 : 0);                         // the space goes in front
    }
    uint32_t incl = item;
#pragma unroll
    for (int o = 1; o < kTextLanes; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, kTextLanes);
      if (lane >= o) incl += t;
    }
    long x = at + run + (incl - item);
    run += __shfl(incl, kTextLanes - 1, kTextLanes);
    if (k < n) {
      if (k) {
        if (x < end) dst[x] = ' ';
        ++x;
      }
      for (uint32_t j = 0; j < wl && x + j < end; ++j) dst[x + j] = s_blob[from + j];
    }
  }
}

__global__ __launch_bounds__(kThreads) void recgen_fill_text_kernel(
    uint64_t S, long first, long n, TextParams pr, const uint8_t* __restrict__ blob,
    const int32_t* __restrict__ woff, int nwords, int nbytes,
    const int64_t* __restrict__ foff, const int64_t* __restrict__ flen,
    const int64_t* __restrict__ klen, uint8_t* __restrict__ dst) {
  __shared__ uint8_t s_blob[kMaxVocabBytes];
  __shared__ uint16_t s_off[kMaxWords + 1];
  load_offsets(woff, nwords, s_off);
  for (int i = threadIdx.x; i < nbytes; i += kThreads) s_blob[i] = blob[i];
  __syncthreads();
  const int lane = threadIdx.x % kTextLanes;
  const long stride = (long)gridDim.x * kTextGroups;
  for (long r = (long)blockIdx.x * kTextGroups + threadIdx.x / kTextLanes; r < n; r += stride) {
    const uint64_t R = rec_word(S, first + r);         // a record's 16 lanes stay together
    const uint32_t nk = pr.lo_k + __umulhi((uint32_t)R, pr.range_k);
    const uint32_t nv = pr.lo_v + __umulhi((uint32_t)(R >> 32), pr.range_v);
    const long a = foff[r], len = flen[r], kl = klen[r], end = a + len;
    const int ks = vint_size(kl);
    const long rest = len - 8 - ks - kl;               // vint(vl) and the value payload
    const long vl = unvint(rest);
    const int vs = (int)(rest - vl);
    for (int i = lane; i < 8 + ks; i += kTextLanes) {
      uint8_t v;
      if (i < 4) v = (uint8_t)((uint32_t)(len - 8) >> (8 * (3 - i)));
      else if (i < 8) v = (uint8_t)((uint32_t)(ks + kl) >> (8 * (7 - i)));
      else v = vint_byte(kl, i - 8);
      if (a + i < end) dst[a + i] = v;
    }
    const long vat = a + 8 + ks + kl;                  // the value's vint
    for (int i = lane; i < vs; i += kTextLanes)
      if (vat + i < end) dst[vat + i] = vint_byte(vl, i);
    write_words(stream_word(R, 0), nk, a + 8 + ks, end, lane, s_blob, s_off, (uint32_t)nwords,
                dst);
    write_words(stream_word(R, 1), nv, vat + vs, end, lane, s_blob, s_off, (uint32_t)nwords, dst);
  }
}

inline bool vocabulary_fits(const void* blob, const void* woff, int nwords, int nbytes) {
  return blob != nullptr && woff != nullptr && nwords >= 1 && nwords <= kMaxWords &&
         nbytes >= 0 && nbytes <= kMaxVocabBytes;
}

}  // namespace

extern "C" {

int hbmr_recgen_chunk_bytes(void) { return kGenChunk; }

// out[4][count] (int64): key payload length, value payload length, key words,
// value words (0 for bytes records) of the records first .. first + count - 1
// of the map whose split word is S.  The two lengths (text: word counts) are
// lo + mulhi32(half of R, range).  Text: woff[nwords + 1], the byte offset of
// each word of the vocabulary (device).
int hbmr_recgen_lengths(uint64_t S, long first, long count, int text, uint32_t lo_k,
                        uint32_t range_k, uint32_t lo_v, uint32_t range_v, const int32_t* woff,
                        int nwords, int64_t* out, hipStream_t st) {
  if (count <= 0) return 0;
  if (count >= (1L << 31) || first < 0) return (int)hipErrorInvalidValue;
  if (text && (woff == nullptr || nwords < 1 || nwords > kMaxWords))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recgen_lengths_kernel, dim3((unsigned)ceil_div(count, kThreads)),
                     dim3(kThreads), 0, st, S, first, count, text,
                     TextParams{lo_k, range_k, lo_v, range_v}, woff, nwords, out);
  return (int)hipGetLastError();
}

// Writes the bytes-record frames of the records first .. first + n - 1 to
// dst[foff[i] : + flen[i]] with key payloads of klen[i] bytes (0 <= klen[i],
// 16 + klen[i] <= flen[i], every frame inside dst: the caller checks).
// chunk_base[n + 1]: the exclusive scan of each frame's chunk count ((dst address
// & 15) + flen[i] + chunk - 1) / chunk, chunk = hbmr_recgen_chunk_bytes();
// chunk_entry[nchunks]: the record each chunk belongs to.
int hbmr_recgen_fill_bytes(uint64_t S, long first, const int64_t* foff, const int64_t* flen,
                           const int64_t* klen, const int64_t* chunk_base,
                           const uint32_t* chunk_entry, long n, long nchunks, uint8_t* dst,
                           hipStream_t st) {
  if (n <= 0 || nchunks <= 0) return 0;
  const long grid = ceil_div(nchunks, kThreads / kCopyLanes);
  if (grid >= (1L << 31) || chunk_entry == nullptr || first < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(recgen_fill_bytes_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, S,
                     first, foff, flen, klen, chunk_base, chunk_entry, nchunks, dst);
  return (int)hipGetLastError();
}

// Writes the text-record frames of the records first .. first + n - 1 to
// dst[foff[i] : + flen[i]] (key payloads of klen[i] bytes; every frame inside
// dst: the caller checks; no byte outside a frame is written).  blob[nbytes]
// and woff[nwords + 1]: the vocabulary's bytes and word offsets (device).
int hbmr_recgen_fill_text(uint64_t S, long first, long n, uint32_t lo_k, uint32_t range_k,
                          uint32_t lo_v, uint32_t range_v, const uint8_t* blob,
                          const int32_t* woff, int nwords, int nbytes, const int64_t* foff,
                          const int64_t* flen, const int64_t* klen, uint8_t* dst, hipStream_t st) {
  if (n <= 0) return 0;
  if (n >= (1L << 31) || first < 0 || !vocabulary_fits(blob, woff, nwords, nbytes))
    return (int)hipErrorInvalidValue;
  const long blocks = ceil_div(n, kTextGroups);
  hipLaunchKernelGGL(recgen_fill_text_kernel,
                     dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(kThreads),
                     0, st, S, first, n, TextParams{lo_k, range_k, lo_v, range_v}, blob, woff,
                     nwords, nbytes, foff, flen, klen, dst);
  return (int)hipGetLastError();
}

}  // extern "C"
