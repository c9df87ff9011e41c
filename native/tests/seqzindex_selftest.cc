// Stand-alone run of the compressed-SequenceFile split plan
// (native/io/seqzindex.cc), built under ASAN+UBSAN by
// `python native/build.py sanitize asan` (tests/test_seqz.py).  argv holds six
// words per case: a file, its header's end, the mode (1 RECORD, 2 BLOCK), the
// key prefix (4 BytesWritable, 0 Text), the split's start and its length.  The
// file, well formed or not, is read into a heap block of exactly its size, so a
// read past a header, a column or a chunk is a sanitizer report.  Prints per
// case `bad`, or the seven dims and every word of the tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" long hbmr_seqz_index_mem(const char* name, const uint8_t* file, long flen,
                                    long header_end, const uint8_t* sync, int mode, int prefix,
                                    long start, long length, int64_t* dims, int64_t* chunks,
                                    long chunk_cap, int64_t* recs, long rec_cap, int64_t* blocks,
                                    long block_cap);

int main(int argc, char** argv) {
  for (int a = 1; a + 5 < argc; a += 6) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::perror(argv[a]);
      return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t* data = static_cast<uint8_t*>(std::malloc(n > 0 ? n : 1));
    if (n > 0 && std::fread(data, 1, n, f) != (size_t)n) {
      std::fprintf(stderr, "%s: short read\n", argv[a]);
      return 2;
    }
    std::fclose(f);
    const long header_end = std::atol(argv[a + 1]);
    const int mode = std::atoi(argv[a + 2]), prefix = std::atoi(argv[a + 3]);
    const long start = std::atol(argv[a + 4]), length = std::atol(argv[a + 5]);
    if (header_end < 16 || header_end > n) {
      std::fprintf(stderr, "%s: header end outside the file\n", argv[a]);
      return 2;
    }
    const uint8_t* sync = data + header_end - 16;
    int64_t dims[7], dims2[7];
    if (hbmr_seqz_index_mem(argv[a], data, n, header_end, sync, mode, prefix, start, length, dims,
                            nullptr, 0, nullptr, 0, nullptr, 0) != 0) {
      std::printf("bad\n");
    } else {
      const long nrec = (long)dims[2], nch = (long)dims[3], nb = (long)dims[4];
      std::vector<int64_t> chunks(4 * (size_t)nch + 1), recs(7 * (size_t)nrec + 1),
          blocks(10 * (size_t)nb + 1);
      if (hbmr_seqz_index_mem(argv[a], data, n, header_end, sync, mode, prefix, start, length,
                              dims2, chunks.data(), nch, mode == 1 ? recs.data() : nullptr, nrec,
                              mode == 2 ? blocks.data() : nullptr, nb) != 0) {
        std::fprintf(stderr, "%s: the second walk failed\n", argv[a]);
        return 1;
      }
      for (int i = 0; i < 7; ++i)
        if (dims[i] != dims2[i]) {
          std::fprintf(stderr, "%s: the two walks disagree\n", argv[a]);
          return 1;
        }
      for (int i = 0; i < 7; ++i) std::printf("%s%lld", i ? " " : "", (long long)dims[i]);
      for (size_t i = 0; i < 4 * (size_t)nch; ++i) std::printf(" %lld", (long long)chunks[i]);
      if (mode == 1)
        for (size_t i = 0; i < 7 * (size_t)nrec; ++i) std::printf(" %lld", (long long)recs[i]);
      else
        for (size_t i = 0; i < 10 * (size_t)nb; ++i) std::printf(" %lld", (long long)blocks[i]);
      std::printf("\n");
    }
    std::free(data);
  }
  return 0;
}
