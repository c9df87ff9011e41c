// Exact-cover counting over a bit-mask placement table: the one search both the
// C++ counter (native/cpu/exactcover.cc) and the HIP kernels
// (native/kernels/exactcover.hip) run, so CPU and GPU slots count alike.
//
// The table is hbmr/ops/exactcover.py's: every placement is a mask over the
// board's cells (W 64-bit words) and one piece bit; the placements are bucketed
// by their lowest cell, bucket c at rows [off[c], off[c + 1]).  A state is
// (occupied cells, used pieces).  The search takes the lowest empty cell and
// tries every placement of its bucket whose piece is unused and whose mask is
// clear of the occupied cells; a state with every cell covered counts 1.  Every
// exact cover is reached exactly once, depth is at most the piece count and
// every level walks a finite bucket.
//
// A lane advances by ec_step(): scan the current bucket to the next placement
// that fits, then push it (or count it, if it completes the board), or pop
// when the bucket is exhausted.  Undo is by XOR, so a stack entry is only the
// row index; the bucket end is found again from the lowest empty cell.  The
// count kernel makes the same moves with the bucket walk split over a group of
// lanes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HBMR_EC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HBMR_EC_HD inline
#endif

namespace hbmr_ec {

constexpr int kMaxPieces = 24;   // stack entries per lane; the host refuses more pieces
constexpr int kMaxRows = 65535;  // row indices are kept as uint16

template <int W>
struct Mask {
  uint64_t w[W];
};

template <int W>
HBMR_EC_HD bool ec_meets(const Mask<W>& a, const Mask<W>& b) {
  uint64_t x = 0;
  for (int k = 0; k < W; ++k) x |= a.w[k] & b.w[k];
  return x != 0;
}

template <int W>
HBMR_EC_HD bool ec_same(const Mask<W>& a, const Mask<W>& b) {
  uint64_t x = 0;
  for (int k = 0; k < W; ++k) x |= a.w[k] ^ b.w[k];
  return x == 0;
}

template <int W>
HBMR_EC_HD Mask<W> ec_full(int ncells) {
  Mask<W> f;
  for (int k = 0; k < W; ++k) {
    const int left = ncells - 64 * k;
    f.w[k] = left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
  }
  return f;
}

// lowest clear bit of a mask that is not full
template <int W>
HBMR_EC_HD int ec_lowest_empty(const Mask<W>& occ) {
  for (int k = 0; k < W - 1; ++k)
    if (~occ.w[k]) return 64 * k + __builtin_ctzll(~occ.w[k]);
  return 64 * (W - 1) + __builtin_ctzll(~occ.w[W - 1]);
}

// m is planar: word k of row r at m[k * nrows + r]; p holds 1 << piece
template <int W>
struct Table {
  const uint64_t* m;
  const uint32_t* p;
  const int32_t* off;
  int nrows;
  int ncells;
};

template <int W>
HBMR_EC_HD Mask<W> ec_row(const Table<W>& t, int r) {
  Mask<W> m;
  for (int k = 0; k < W; ++k) m.w[k] = t.m[k * t.nrows + r];
  return m;
}

template <int W>
struct Lane {
  Mask<W> occ;
  uint32_t used;
  int d;     // rows pushed below the start state; -1: no state in hand
  int i, e;  // next row to try and the end of the current bucket
};

// Take the state (words: occ[W], then used in the low half of the last word).
// Returns what the state counts by itself: 1 if it is a full cover (the lane
// stays free), else 0.  A state with cells outside the board has no completion.
template <int W>
HBMR_EC_HD int ec_start(const Table<W>& t, const Mask<W>& full, const uint64_t* st, Lane<W>& l) {
  uint64_t out = 0;
  for (int k = 0; k < W; ++k) {
    l.occ.w[k] = st[k];
    out |= st[k] & ~full.w[k];
  }
  l.used = (uint32_t)st[W];
  l.d = -1;
  if (out) return 0;
  if (ec_same(l.occ, full)) return 1;
  const int c = ec_lowest_empty(l.occ);
  l.d = 0;
  l.i = t.off[c];
  l.e = t.off[c + 1];
  return 0;
}

// One move of a lane that holds a state (l.d >= 0).  stack[d * stride] is the
// lane's entry for depth d.  Returns the covers completed by this move (0 or 1)
// and adds 1 to nodes for every placement made.
template <int W>
HBMR_EC_HD int ec_step(const Table<W>& t, const Mask<W>& full, Lane<W>& l, uint16_t* stack,
                       int stride, uint64_t& nodes) {
  Mask<W> m;
  uint32_t p = 0;
  while (l.i < l.e) {
    m = ec_row(t, l.i);
    p = t.p[l.i];
    if (!ec_meets(m, l.occ) && !(p & l.used)) break;
    ++l.i;
  }
  if (l.i < l.e) {
    ++nodes;
    Mask<W> occ;
    for (int k = 0; k < W; ++k) occ.w[k] = l.occ.w[k] | m.w[k];
    if (ec_same(occ, full)) {  // a leaf: counted, nothing to push
      ++l.i;
      return 1;
    }
    if (l.d >= kMaxPieces - 1) {  // never with a table the host built
      ++l.i;
      return 0;
    }
    l.occ = occ;
    l.used |= p;
    stack[l.d * stride] = (uint16_t)l.i;
    ++l.d;
    const int c = ec_lowest_empty(occ);
    l.i = t.off[c];
    l.e = t.off[c + 1];
    return 0;
  }
  if (--l.d >= 0) {  // bucket exhausted: take the parent's row back
    const int r = stack[l.d * stride];
    m = ec_row(t, r);
    for (int k = 0; k < W; ++k) l.occ.w[k] ^= m.w[k];
    l.used ^= t.p[r];
    l.i = r + 1;
    l.e = t.off[ec_lowest_empty(l.occ) + 1];
  }
  return 0;
}

// Children of one state, in bucket order: `emit(child words)` for each.  A full
// cover passes through as its own only child, so a level loses no count.
template <int W, class Emit>
HBMR_EC_HD int ec_children(const Table<W>& t, const Mask<W>& full, const uint64_t* st, Emit emit) {
  Lane<W> l;
  if (ec_start(t, full, st, l)) {
    emit(l.occ, st[W]);
    return 1;
  }
  if (l.d < 0) return 0;
  int n = 0;
  for (int r = l.i; r < l.e; ++r) {
    const Mask<W> m = ec_row(t, r);
    const uint32_t p = t.p[r];
    if (ec_meets(m, l.occ) || (p & l.used)) continue;
    Mask<W> occ;
    for (int k = 0; k < W; ++k) occ.w[k] = l.occ.w[k] | m.w[k];
    emit(occ, st[W] | p);
    ++n;
  }
  return n;
}

}  // namespace hbmr_ec
