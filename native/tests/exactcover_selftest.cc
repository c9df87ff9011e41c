// Stand-alone run of the exact-cover counter (native/cpu/exactcover.cc), built
// under ASAN+UBSAN or TSAN by `python native/build.py sanitize asan|tsan`
// (tests/test_pentomino_gpu.py).  argv[1]: a table and states as
// hbmr/ops/exactcover.py dumps them; argv[2]: threads.  Prints one count per
// prefix, then the placements made.
//
//   int32 words, nrows, ncells, nstates, nprefixes
//   uint64 m[words][nrows]; uint32 p[nrows]; int32 off[ncells + 1]
//   uint64 states[nstates][words + 1]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hbmr/hbmr.h"

template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: exactcover_selftest TABLE [THREADS]\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t h[5];
  std::vector<uint64_t> m, states;
  std::vector<uint32_t> p;
  std::vector<int32_t> off;
  bool ok = std::fread(h, sizeof(int32_t), 5, f) == 5 && h[0] >= 1 && h[0] <= 2 && h[1] >= 0 &&
            h[2] >= 1 && h[3] >= 0 && h[4] >= 0;
  ok = ok && read_vec(f, m, (size_t)h[0] * h[1]) && read_vec(f, p, (size_t)h[1]) &&
       read_vec(f, off, (size_t)h[2] + 1) && read_vec(f, states, (size_t)h[3] * (h[0] + 1));
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "exactcover_selftest: short or malformed table file\n");
    return 2;
  }
  std::vector<int64_t> counts((size_t)h[4], 0);
  uint64_t nodes = 0;
  const int rc = hbmr_exactcover_count_cpu(h[0], m.data(), p.data(), off.data(), h[1], h[2],
                                           states.data(), h[3], h[4], counts.data(), &nodes,
                                           argc > 2 ? std::atoi(argv[2]) : 1);
  if (rc != 0) {
    std::fprintf(stderr, "exactcover_selftest: counter returned %d\n", rc);
    return 1;
  }
  for (int64_t c : counts) std::printf("%lld\n", (long long)c);
  std::printf("nodes %llu\n", (unsigned long long)nodes);
  return 0;
}
