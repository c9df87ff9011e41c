// Record index of a SequenceFile byte range, and the layout of a part written
// from gathered frames (the host pieces of GPU Sort: hbmr/ops/recsort.py).
//
//   hbmr_seq_index_records — one pass over the records of a FileSplit of an
//                            uncompressed SequenceFile<BytesWritable|Text, *>:
//                            per record the offset and length of its frame
//                            ([recordLen][keyLen][key][value]) and of its key
//                            payload (behind BytesWritable's 4-byte length or
//                            Text's vint), relative to the start of the raw
//                            range that holds them.  Same boundary rule as
//                            SequenceFileRecordReader; sync escapes lie inside
//                            the range and are not indexed.
//   hbmr_seq_layout        — from frame lengths, each frame's offset in a file
//                            body that starts at `pos`, leaving the 20-byte
//                            sync escapes where Writer's check-and-write-sync
//                            rule (an escape before a record once 2000 bytes
//                            lie behind the last one) puts them.
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "sequencefile.h"

namespace {

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

thread_local std::string g_err;

constexpr int64_t kSyncSize = 20;
constexpr int64_t kSyncInterval = 100 * kSyncSize;

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

const char* hbmr_seq_index_last_error() { return g_err.c_str(); }

// idx == nullptr: count only.  Else idx[0..n), idx[cap..cap+n), idx[2cap..), idx[3cap..):
// frame offset, frame length, key payload offset, key payload length.  range[0..2):
// the file offsets [first record or its sync escape, end of the last record).
// Returns the number of records, or -1 (hbmr_seq_index_last_error).
long hbmr_seq_index_records(const char* path, long start, long length, long* range, int64_t* idx,
                            long cap) {
  try {
    hbmr::io::SeqReader r(path);
    if (r.compression() != hbmr::io::Compression::NONE)
      throw std::runtime_error(std::string(path) + ": compressed SequenceFile");
    int prefix;     // 4: BytesWritable, 0: Text (vint)
    if (r.key_class() == "org.apache.hadoop.io.BytesWritable") prefix = 4;
    else if (r.key_class() == "org.apache.hadoop.io.Text") prefix = 0;
    else throw std::runtime_error(std::string(path) + ": key class " + r.key_class());
    const int64_t flen = r.file_length();
    const int64_t end = (int64_t)start + length;
    if (start > r.position()) r.sync_to(start);
    const int64_t pos0 = r.position();
    range[0] = range[1] = pos0;
    if (pos0 >= end || pos0 >= flen) return 0;
    Map m;
    m.fd = open(path, O_RDONLY);
    if (m.fd < 0) throw std::runtime_error(std::string("cannot open ") + path);
    m.n = (size_t)flen;
    m.p = mmap(nullptr, m.n, PROT_READ, MAP_PRIVATE, m.fd, 0);
    if (m.p == MAP_FAILED) throw std::runtime_error(std::string("mmap failed for ") + path);
    const uint8_t* b = static_cast<const uint8_t*>(m.p);
    const uint8_t* sync = r.sync_bytes();
    int64_t pos = pos0;
    long n = 0;
    while (pos + 4 <= flen) {
      const int64_t rec_pos = pos;
      bool sync_seen = false;
      int32_t len = (int32_t)be32(b + pos);
      if (len == -1) {
        if (pos + kSyncSize > flen || memcmp(b + pos + 4, sync, 16) != 0)
          throw std::runtime_error(std::string(path) + ": sync check failure");
        sync_seen = true;
        pos += kSyncSize;
        if (pos + 4 > flen) break;
        len = (int32_t)be32(b + pos);
      }
      if (rec_pos >= end && sync_seen) break;
      if (pos + 8 > flen) throw std::runtime_error("truncated record");
      const int32_t klen = (int32_t)be32(b + pos + 4);
      if (len < 0 || klen < 0 || klen > len || pos + 8 + len > flen)
        throw std::runtime_error("corrupt record");
      int64_t poff, plen;
      if (prefix) {
        if (klen < 4) throw std::runtime_error("corrupt BytesWritable key");
        poff = pos + 12;
        plen = (int32_t)be32(b + pos + 8);
        if (plen != klen - 4) throw std::runtime_error("corrupt BytesWritable key");
      } else {
        const uint8_t* q = b + pos + 8;
        plen = hbmr::io::read_vlong(q, b + pos + 8 + klen);
        poff = q - b;
        if (plen < 0 || poff + plen != pos + 8 + klen)
          throw std::runtime_error("corrupt Text key");
      }
      if (idx != nullptr) {
        if (n >= cap) throw std::runtime_error("index capacity exceeded");
        idx[n] = pos - pos0;
        idx[cap + n] = 8 + (int64_t)len;
        idx[2 * cap + n] = poff - pos0;
        idx[3 * cap + n] = plen;
      }
      pos += 8 + len;
      range[1] = pos;
      ++n;
    }
    return n;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// pos: file position of the body's first byte; last_sync: Writer's last sync
// position.  dst[i]: offset of frame i in the body; gaps[0..return): body
// offsets of the sync escapes (at most one per frame); *total: body bytes.
long hbmr_seq_layout(const int64_t* flen, long n, long pos, long last_sync, int64_t* dst,
                     int64_t* gaps, int64_t* total) {
  const int64_t pos0 = pos;
  int64_t p = pos, ls = last_sync;
  long g = 0;
  for (long i = 0; i < n; ++i) {
    if (p >= ls + kSyncInterval && ls != p) {
      gaps[g++] = p - pos0;
      p += kSyncSize;
      ls = p;
    }
    dst[i] = p - pos0;
    p += flen[i];
  }
  *total = p - pos0;
  return g;
}

}  // extern "C"
