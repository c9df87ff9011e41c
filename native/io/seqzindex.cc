// Plan of a split of a Snappy RECORD- or BLOCK-compressed SequenceFile for the
// device loader (hbmr/ops/seqz.py, native/kernels/seqblock.hip): the file byte
// range to load and, relative to it, the raw Snappy streams the decode kernel
// (native/kernels/snappydec.hip) takes, in its int64[4, c] table form.
//
//   RECORD  frames are [recLen][keyLen][key][framed Snappy value] with sync
//           escapes as in an uncompressed file.  The headers give every length,
//           so the whole record index is built here: recs is int64[7, n] — the
//           four index rows of recindex.cc over the FINAL frames (back to back,
//           [8 + klen + vlen]), then the key's offset in the loaded range, its
//           length and the value's uncompressed length.  A value's chunks have
//           their destination inside the final frame (foff + 8 + klen).
//   BLOCK   blocks are [escape + sync][vint n] and four columns (key lengths,
//           keys, value lengths, values), each [vint compressedLen][framed
//           Snappy stream].  The chunks decode into a scratch "columns" buffer;
//           blocks is int64[10, b]: the record count, the record base and the
//           offset and decoded length of each column there.  The records'
//           lengths are known only on the device.
//
// The framing of a stream is snappyindex.cc's.  The split rule is
// SequenceFileRecordReader's: sync to the first marker at or after `start`, then
// take records (blocks) until one begins at or after the end behind a marker.
// The file's header is parsed by the caller (hbmr/io/sequencefile.py).
//
// C ABI (ctypes, libhbmr_cpu.so).  Two calls: with null tables for the counts
// in dims, then with tables of those sizes.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

extern "C" long hbmr_snappy_uncompressed_length(const uint8_t* in, long n);

namespace {

thread_local std::string g_err;

constexpr int64_t kSyncSize = 20;

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

struct Plan {
  const char* name;
  const uint8_t* b;     // the file
  int64_t flen;
  const uint8_t* sync;
  int prefix;           // 4: BytesWritable, 0: Text (vint)
  int64_t lo = 0;       // start of the range to load
  int64_t* chunks;
  long chunk_cap;
  int64_t* recs;
  long rec_cap;
  int64_t* blocks;
  long block_cap;
  long nchunks = 0, nrecs = 0, nblocks = 0;
  int64_t out = 0;      // bytes of the final data (RECORD), of the columns buffer (BLOCK)
  int64_t kv = 0;       // BLOCK: decoded bytes of the keys and values columns

  bool in_block = false;   // walking blocks: every error names the current one

  [[noreturn]] void fail(const std::string& what) const {
    throw std::runtime_error(std::string(name) + ": " +
                             (in_block ? "block " + std::to_string(nblocks) + ": " : "") + what);
  }

  // A Hadoop vint at pos, inside [pos, end); advances pos.
  int64_t vint(int64_t& pos, int64_t end, const char* what) const {
    if (pos >= end) fail(std::string(what) + ": a vint runs off the file");
    const int8_t first = (int8_t)b[pos++];
    if (first >= -112) return first;
    const bool neg = first < -120;
    const int len = neg ? -(first + 120) : -(first + 112);
    if (end - pos < len) fail(std::string(what) + ": a vint runs off the file");
    uint64_t v = 0;
    for (int i = 0; i < len; ++i) v = (v << 8) | b[pos++];
    return neg ? (int64_t)~v : (int64_t)v;
  }

  // The chunks of the framed stream b[pos, end) with output from dst on; returns
  // its uncompressed size.
  int64_t stream(int64_t pos, int64_t end, int64_t dst, const std::string& what) {
    int64_t done = 0;
    while (pos < end) {
      if (end - pos < 4) fail(what + ": truncated snappy block header");
      const int64_t orig = be32(b + pos);
      pos += 4;
      int64_t got = 0;
      while (got < orig) {
        if (end - pos < 4) fail(what + ": truncated snappy chunk header");
        const int64_t c = be32(b + pos);
        pos += 4;
        if (c <= 0 || c > 0x7fffffffL || end - pos < c)
          fail(what + ": snappy chunk length past the end");
        const int64_t u = hbmr_snappy_uncompressed_length(b + pos, c);
        if (u < 0) fail(what + ": malformed snappy chunk preamble");
        if (chunks != nullptr) {
          if (nchunks >= chunk_cap) fail("chunk capacity exceeded");
          chunks[nchunks] = pos - lo;
          chunks[chunk_cap + nchunks] = c;
          chunks[2 * chunk_cap + nchunks] = dst + done + got;
          chunks[3 * chunk_cap + nchunks] = u;
        }
        ++nchunks;
        got += u;
        pos += c;
      }
      if (got != orig) fail(what + ": snappy chunk lengths do not add up to their block's header");
      done += orig;
    }
    return done;
  }

  // Reader.sync_to + SequenceFileRecordReader's start
  int64_t first_position(int64_t header_end, int64_t start) const {
    if (start <= header_end) return header_end;
    if (start + kSyncSize >= flen) return flen;
    for (int64_t p = start + 4; p + 16 <= flen; ++p)
      if (memcmp(b + p, sync, 16) == 0) return p - 4;
    return flen;
  }

  void check_sync(int64_t pos) const {
    if (pos + kSyncSize > flen || memcmp(b + pos + 4, sync, 16) != 0) fail("sync check failure");
  }

  // returns the end of the range
  int64_t walk_records(int64_t pos, int64_t end) {
    int64_t hi = pos;
    while (pos + 4 <= flen) {
      const int64_t rec_pos = pos;
      bool sync_seen = false;
      int32_t len = (int32_t)be32(b + pos);
      if (len == -1) {
        check_sync(pos);
        sync_seen = true;
        pos += kSyncSize;
        if (pos + 4 > flen) break;
        len = (int32_t)be32(b + pos);
      }
      if (rec_pos >= end && sync_seen) break;
      if (pos + 8 > flen) fail("truncated record");
      const int32_t klen = (int32_t)be32(b + pos + 4);
      if (len < 0 || klen < 0 || klen > len || pos + 8 + len > flen) fail("corrupt record");
      const int64_t key = pos + 8;
      int64_t poff, plen;     // the payload, relative to the key
      if (prefix) {
        if (klen < 4) fail("corrupt BytesWritable key");
        poff = 4;
        plen = (int32_t)be32(b + key);
        if (plen != klen - 4) fail("corrupt BytesWritable key");
      } else {
        int64_t q = key;
        plen = vint(q, key + klen, "Text key");
        poff = q - key;
        if (plen < 0 || poff + plen != klen) fail("corrupt Text key");
      }
      const int64_t foff = out;
      const int64_t vlen = stream(key + klen, pos + 8 + len, foff + 8 + klen,
                                  "record " + std::to_string(nrecs));
      if (8 + (int64_t)klen + vlen > 0x7fffffffL) fail("record too long");
      if (recs != nullptr) {
        if (nrecs >= rec_cap) fail("record capacity exceeded");
        int64_t* r = recs + nrecs;
        r[0] = foff;
        r[rec_cap] = 8 + klen + vlen;
        r[2 * rec_cap] = foff + 8 + poff;
        r[3 * rec_cap] = plen;
        r[4 * rec_cap] = key - lo;
        r[5 * rec_cap] = klen;
        r[6 * rec_cap] = vlen;
      }
      ++nrecs;
      out = foff + 8 + klen + vlen;
      pos += 8 + (int64_t)len;
      hi = pos;
    }
    return hi;
  }

  int64_t walk_blocks(int64_t pos, int64_t end) {
    int64_t hi = pos;
    in_block = true;
    while (pos + 4 <= flen && pos < end) {
      if ((int32_t)be32(b + pos) != -1) fail("expected sync before block");
      check_sync(pos);
      pos += kSyncSize;
      const int64_t n = vint(pos, flen, "block header");
      if (n < 0 || n > 0x7fffffffL) fail("bad record count");
      int64_t col[8];
      for (int c = 0; c < 4; ++c) {
        if (pos >= flen) fail("truncated block");
        const int64_t clen = vint(pos, flen, "column header");
        if (clen < 0 || flen - pos < clen) fail("column's compressed length past the end");
        col[2 * c] = out;
        col[2 * c + 1] = stream(pos, pos + clen, out, "column " + std::to_string(c));
        out += col[2 * c + 1];
        pos += clen;
      }
      // a vint is at least a byte: n of them do not fit a shorter length column
      if (col[1] < n || col[5] < n) fail("record count above what its length columns hold");
      kv += col[3] + col[7];
      if (blocks != nullptr) {
        if (nblocks >= block_cap) fail("block capacity exceeded");
        int64_t* r = blocks + nblocks;
        r[0] = n;
        r[block_cap] = nrecs;
        for (int j = 0; j < 8; ++j) r[(2 + j) * block_cap] = col[j];
      }
      ++nblocks;
      nrecs += n;
      hi = pos;
    }
    return hi;
  }
};

struct Map {
  int fd = -1;
  void* p = MAP_FAILED;
  size_t n = 0;
  ~Map() {
    if (p != MAP_FAILED) munmap(p, n);
    if (fd >= 0) close(fd);
  }
};

}  // namespace

extern "C" {

const char* hbmr_seqz_last_error() { return g_err.c_str(); }

// The plan of the split (start, length) of the file image file[0, flen) whose
// header ends at header_end with the 16 sync bytes `sync`.  mode 1: RECORD, 2:
// BLOCK; prefix 4: BytesWritable keys, 0: Text keys.  dims[0..7): the range to
// load [lo, hi), records, chunks, blocks, bytes of the final data (RECORD; BLOCK:
// 8 a record plus the keys and values columns) and of the columns buffer.
// chunks int64[4, chunk_cap], recs int64[7, rec_cap] (RECORD), blocks
// int64[10, block_cap] (BLOCK), or null for the counts alone.  Returns 0, or
// -1 (hbmr_seqz_last_error names the file and the block).
long hbmr_seqz_index_mem(const char* name, const uint8_t* file, long flen, long header_end,
                         const uint8_t* sync, int mode, int prefix, long start, long length,
                         int64_t* dims, int64_t* chunks, long chunk_cap, int64_t* recs,
                         long rec_cap, int64_t* blocks, long block_cap) {
  try {
    Plan p{name, file, flen, sync, prefix};
    p.chunks = chunks;
    p.chunk_cap = chunk_cap;
    p.recs = recs;
    p.rec_cap = rec_cap;
    p.blocks = blocks;
    p.block_cap = block_cap;
    if (mode != 1 && mode != 2) p.fail("not a RECORD- or BLOCK-compressed file");
    if (header_end < 16 || header_end > flen) p.fail("truncated SequenceFile header");
    const int64_t end = (int64_t)start + length;
    const int64_t pos0 = p.first_position(header_end, start);
    p.lo = pos0;
    int64_t hi = pos0;
    if (pos0 < end && pos0 < flen) hi = mode == 1 ? p.walk_records(pos0, end) : p.walk_blocks(pos0, end);
    const int64_t data_bytes = mode == 2 ? 8 * (int64_t)p.nrecs + p.kv : p.out;
    dims[0] = pos0;
    dims[1] = hi;
    dims[2] = p.nrecs;
    dims[3] = p.nchunks;
    dims[4] = p.nblocks;
    dims[5] = data_bytes;
    dims[6] = mode == 2 ? p.out : 0;
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

long hbmr_seqz_index(const char* path, long header_end, const uint8_t* sync, int mode, int prefix,
                     long start, long length, int64_t* dims, int64_t* chunks, long chunk_cap,
                     int64_t* recs, long rec_cap, int64_t* blocks, long block_cap) {
  Map m;
  m.fd = open(path, O_RDONLY);
  struct stat st;
  if (m.fd < 0 || fstat(m.fd, &st) != 0) {
    g_err = std::string("cannot open ") + path;
    return -1;
  }
  m.n = (size_t)st.st_size;
  if (m.n) {
    m.p = mmap(nullptr, m.n, PROT_READ, MAP_PRIVATE, m.fd, 0);
    if (m.p == MAP_FAILED) {
      g_err = std::string("mmap failed for ") + path;
      return -1;
    }
  }
  return hbmr_seqz_index_mem(path, m.n ? static_cast<const uint8_t*>(m.p) : nullptr, (long)m.n,
                             header_end, sync, mode, prefix, start, length, dims, chunks, chunk_cap,
                             recs, rec_cap, blocks, block_cap);
}

}  // extern "C"
