// Stand-alone run of the Snappy chunk-table walk (native/io/snappyindex.cc),
// built under ASAN+UBSAN by `python native/build.py sanitize asan`
// (tests/test_snappy_gpu.py).  argv[1..]: framed Snappy files, well formed or
// not.  Each is read into a heap block of exactly its size, so a read past a
// header or a chunk is a sanitizer report.  Prints per file `bad`, or the
// chunk count, the output size and the table's columns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" long hbmr_snappy_index(const uint8_t* in, long n, int64_t* table, long cap, long* total);

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
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
    long total = -1;
    const long chunks = hbmr_snappy_index(data, n, nullptr, 0, &total);
    if (chunks < 0) {
      std::printf("bad\n");
    } else {
      std::vector<int64_t> table(4 * (size_t)chunks + 1);
      long total2 = -1;
      if (hbmr_snappy_index(data, n, table.data(), chunks, &total2) != chunks || total2 != total) {
        std::fprintf(stderr, "%s: the two walks disagree\n", argv[a]);
        return 1;
      }
      std::printf("%ld %ld", chunks, total);
      for (long i = 0; i < chunks; ++i)
        std::printf(" %lld:%lld:%lld:%lld", (long long)table[i], (long long)table[chunks + i],
                    (long long)table[2 * chunks + i], (long long)table[3 * chunks + i]);
      std::printf("\n");
    }
    std::free(data);
  }
  return 0;
}
