// Exact-cover counter for CPU slots (Pentomino map): the search of
// include/hbmr/exactcover_core.h below each state, states handed out to the
// threads from one atomic counter, counts summed per prefix.
#include <atomic>
#include <cerrno>
#include <mutex>
#include <thread>
#include <vector>

#include "../include/hbmr/exactcover_core.h"
#include "../include/hbmr/hbmr.h"

namespace {

using namespace hbmr_ec;

template <int W>
void count_range(const Table<W>& t, const uint64_t* states, long n, long nprefixes,
                 std::atomic<long>& next, std::vector<int64_t>& counts, uint64_t& nodes) {
  const Mask<W> full = ec_full<W>(t.ncells);
  uint16_t stack[kMaxPieces];
  for (long s = next.fetch_add(1); s < n; s = next.fetch_add(1)) {
    const uint64_t* st = states + s * (W + 1);
    const uint64_t src = st[W] >> 32;
    if (src >= (uint64_t)nprefixes) continue;  // checked by the caller: never taken
    Lane<W> l;
    int64_t c = ec_start(t, full, st, l);
    while (l.d >= 0) c += ec_step(t, full, l, stack, 1, nodes);
    counts[src] += c;
  }
}

template <int W>
int count_cpu(const uint64_t* m, const uint32_t* p, const int32_t* off, int nrows, int ncells,
              const uint64_t* states, long n, long nprefixes, int64_t* counts, uint64_t* nodes,
              int threads) {
  const Table<W> t{m, p, off, nrows, ncells};
  std::atomic<long> next{0};
  if (threads < 1) threads = 1;
  if ((long)threads > n) threads = n > 0 ? (int)n : 1;
  std::mutex mu;
  auto work = [&] {
    std::vector<int64_t> mine((size_t)nprefixes, 0);
    uint64_t my_nodes = 0;
    count_range<W>(t, states, n, nprefixes, next, mine, my_nodes);
    std::lock_guard<std::mutex> g(mu);
    for (long i = 0; i < nprefixes; ++i) counts[i] += mine[i];
    if (nodes) *nodes += my_nodes;
  };
  if (threads == 1) {
    work();
    return 0;
  }
  std::vector<std::thread> pool;
  for (int i = 0; i < threads; ++i) pool.emplace_back(work);
  for (auto& th : pool) th.join();
  return 0;
}

}  // namespace

// counts[nprefixes] and *nodes are added to.  -EINVAL for a table or a state
// the search cannot hold.
extern "C" int hbmr_exactcover_count_cpu(int words, const uint64_t* m, const uint32_t* p,
                                         const int32_t* off, int nrows, int ncells,
                                         const uint64_t* states, long n, long nprefixes,
                                         int64_t* counts, uint64_t* nodes, int threads) {
  if ((words != 1 && words != 2) || ncells < 1 || ncells > 64 * words || nrows < 0 ||
      nrows > kMaxRows || n < 0 || nprefixes < 0)
    return -EINVAL;
  for (int c = 0; c <= ncells; ++c)
    if (off[c] < 0 || off[c] > nrows || (c && off[c] < off[c - 1])) return -EINVAL;
  for (long s = 0; s < n; ++s)
    if ((states[s * (words + 1) + words] >> 32) >= (uint64_t)nprefixes) return -EINVAL;
  return words == 1 ? count_cpu<1>(m, p, off, nrows, ncells, states, n, nprefixes, counts, nodes,
                                   threads)
                    : count_cpu<2>(m, p, off, nrows, ncells, states, n, nprefixes, counts, nodes,
                                   threads);
}
