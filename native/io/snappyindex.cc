// Chunk table of a Hadoop-framed Snappy stream (what a `.snappy` file holds):
// the independent raw streams a device decoder takes in parallel
// (native/kernels/snappydec.hip), listed from the headers alone.
//
// The framing is snappy.cc's (BlockCompressorStream.java:76-153): per block a
// big-endian int of the uncompressed length, then big-endian int-length-
// prefixed raw Snappy chunks until their preambles add up to it.  The checks
// are those of hbmr_snappy_hadoop_uncompressed_length: a truncated header, a
// chunk length <= 0 or past the end, chunk lengths that do not add up to the
// block's header, a preamble over 22*n + 64.
//
// C ABI (ctypes from hbmr/ops/snappydec.py, libhbmr_cpu.so).
#include <cstdint>

extern "C" long hbmr_snappy_uncompressed_length(const uint8_t* in, long n);

namespace {

inline long get_be32(const uint8_t* p) {
  return (long)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]);
}

}  // namespace

extern "C" {

// Walk in[0:n].  Returns the number of chunks, or -1 on bad framing; *total
// gets the uncompressed size.  With table != nullptr (int64[4, cap], row-major)
// chunk i < cap gets column i: the raw stream's offset in `in`, its compressed
// length, its offset in the output and its uncompressed length.  Call once with
// table == nullptr for the count, then with a table of that many columns.
long hbmr_snappy_index(const uint8_t* in, long n, int64_t* table, long cap, long* total) {
  long pos = 0, out = 0, chunks = 0;
  while (pos < n) {
    if (n - pos < 4) return -1;
    const long orig = get_be32(in + pos);
    pos += 4;
    long got = 0;
    while (got < orig) {
      if (n - pos < 4) return -1;
      const long c = get_be32(in + pos);
      pos += 4;
      if (c <= 0 || c > 0x7fffffffL || n - pos < c) return -1;
      const long u = hbmr_snappy_uncompressed_length(in + pos, c);
      if (u < 0) return -1;
      if (table != nullptr && chunks < cap) {
        table[chunks] = pos;
        table[cap + chunks] = c;
        table[2 * cap + chunks] = out + got;
        table[3 * cap + chunks] = u;
      }
      ++chunks;
      got += u;
      pos += c;
    }
    if (got != orig) return -1;
    out += orig;
  }
  if (total != nullptr) *total = out;
  return chunks;
}

}  // extern "C"
