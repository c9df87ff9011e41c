"""Pentomino counting as an exact-cover search over bit masks: the placement
table, the numpy/Python twin, and the bindings of the C++ counter
(native/cpu/exactcover.cc) and the HIP kernels (native/kernels/exactcover.hip).

The table is built from the ``DancingLinks`` rows of a
:class:`~hbmr.examples.dancing.Pentomino`, same rows in the same order (the
X-piece restriction included), so a row index means what it means in the
classic job's prefix lines.  Each row is a bit mask over the board's cells and
a piece bit; rows are bucketed by their lowest cell.

**Cells are numbered along the board's shorter side**: ``bit = x * h + y`` when
``h <= w``, else ``y * w + x``.  This is part of the table's definition, not a
detail: the search fills the lowest empty cell, so the filled region advances
as a front as wide as the short side, and a front that wide closes off dead
regions early.  Numbered along the long side, 3×20 does not finish in minutes;
numbered this way it takes 68 thousand placements.

A state is ``(occupied cells, used pieces)``, held as ``W + 1`` uint64 words:
the cell mask (``W`` = 1 up to 64 cells, 2 up to 128), then the used pieces in
the low half of the last word and the index of the prefix the state descends
from in the high half.  The search takes the lowest empty cell and tries every
row of that cell's bucket whose piece is unused and whose mask is clear of the
occupied cells; a state with every cell covered counts 1.  Every exact cover is
reached exactly once, and the number of completions of a prefix does not
depend on the order of the search, so per-prefix counts equal the classic
mapper's although the classic splitter picks its columns by the fewest-rows
rule.  A fully covered state passes through :func:`expand` as its own child.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

MAX_PIECES = 24          # kMaxPieces of native/include/hbmr/exactcover_core.h
MAX_ROWS = 65535
#: breadth-first levels below the prefixes before the depth-first count, and
#: the most states one level chunk may hold (profiles/pentomino_1gpu.json)
DEFAULT_LEVELS = 8
DEFAULT_CAPACITY = 1 << 20

_CPU_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib",
                         "libhbmr_cpu.so")
_CPU = None


class Table:
    """The placement table of one board (see the module docstring)."""

    def __init__(self, w, h, npieces, rows):
        """``rows``: (piece index, [(y, x), ...]) per DancingLinks row, in order."""
        self.w, self.h, self.npieces = w, h, npieces
        self.ncells = w * h
        if not 1 <= self.ncells <= 128:
            raise ValueError(f"a {w}x{h} board does not fit a 128-bit cell mask")
        if npieces > MAX_PIECES:
            raise ValueError(f"{npieces} pieces: the search holds at most {MAX_PIECES}")
        if len(rows) > MAX_ROWS:
            raise ValueError(f"{len(rows)} placements: the search holds at most {MAX_ROWS}")
        self.words = 1 if self.ncells <= 64 else 2
        self.full = (1 << self.ncells) - 1
        #: no cover exists unless the pieces' cells are the board's: counts are 0
        self.solvable = self.ncells == 5 * npieces
        self.row_mask = [sum(1 << self.bit(y, x) for y, x in cells) for _, cells in rows]
        self.row_pbit = [1 << p for p, _ in rows]
        low = [(m & -m).bit_length() - 1 for m in self.row_mask]
        #: bucket order -> DancingLinks row (stable: rows of a bucket keep their order)
        self.order = sorted(range(len(rows)), key=lambda r: low[r])
        self.buckets = [[] for _ in range(self.ncells)]
        for r in self.order:
            self.buckets[low[r]].append((self.row_mask[r], self.row_pbit[r]))
        off = np.zeros(self.ncells + 1, dtype=np.int32)
        np.cumsum([len(b) for b in self.buckets], out=off[1:])
        self.off = off
        n = len(rows)
        self.nrows = n
        # planar: word k of (bucket-ordered) row r at m[k, r]
        self.m = np.zeros((self.words, n), dtype=np.uint64)
        for i, r in enumerate(self.order):
            for k in range(self.words):
                self.m[k, i] = (self.row_mask[r] >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        self.p = np.array([self.row_pbit[r] for r in self.order], dtype=np.uint32)
        self._device = {}

    def bit(self, y, x):
        """The cell's bit: numbered along the shorter side."""
        return x * self.h + y if self.h <= self.w else y * self.w + x

    def widened(self):
        """The same table with 128-bit masks (a 60-cell board through the
        two-word instantiation counts what the one-word one counts)."""
        t = Table.__new__(Table)
        t.__dict__.update(self.__dict__)
        if self.words == 1:
            t.words = 2
            t.m = np.concatenate([self.m, np.zeros_like(self.m)], axis=0)
            t._device = {}
        return t

    def on(self, device):
        """(m, p, off) as tensors on ``device``, made once."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.m.view(np.int64)).to(device),
                                 torch.from_numpy(self.p.view(np.int32)).to(device),
                                 torch.from_numpy(self.off).to(device))
        return self._device[key]


def table(pentomino) -> Table:
    """The placement table of a Pentomino (or OneSidedPentomino)."""
    npieces = len(pentomino.names)
    rows = []
    for cols in pentomino.dl.rows:
        cells = [divmod(c - npieces, pentomino.w) for c in cols[1:]]
        rows.append((cols[0], cells))
    return Table(pentomino.w, pentomino.h, npieces, rows)


# ------------------------------------------------------------------------------ states
def _pack(tab, states):
    """[(occ, used, src)] as uint64[n, W + 1]."""
    out = np.zeros((len(states), tab.words + 1), dtype=np.uint64)
    for i, (occ, used, src) in enumerate(states):
        for k in range(tab.words):
            out[i, k] = (occ >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        out[i, tab.words] = used | (src << 32)
    return out


def _unpack(tab, words):
    words = np.asarray(words, dtype=np.uint64).reshape(-1, tab.words + 1)
    out = []
    for row in words.tolist():
        occ = sum(row[k] << (64 * k) for k in range(tab.words))
        out.append((occ, row[tab.words] & 0xFFFFFFFF, row[tab.words] >> 32))
    return out


def states(tab, prefixes) -> np.ndarray:
    """uint64[n, W + 1]: the state each prefix (a list of DancingLinks row
    indices, as ``split`` gives them) leaves, tagged with the prefix's index."""
    out = []
    for src, prefix in enumerate(prefixes):
        occ = used = 0
        for r in prefix:
            m, p = tab.row_mask[r], tab.row_pbit[r]
            if occ & m or used & p:
                raise ValueError(f"prefix {list(prefix)}: row {r} meets an earlier row")
            occ |= m
            used |= p
        out.append((occ, used, src))
    return _pack(tab, out)


def _children(tab, occ, used):
    if occ == tab.full:
        return [(occ, used)]
    c = (~occ & (occ + 1)).bit_length() - 1
    return [(occ | m, used | p) for m, p in tab.buckets[c] if not (m & occ) and not (p & used)]


def expand(tab, words) -> np.ndarray:
    """One breadth-first level: the children of every state, in state order
    and within a state in bucket order.  A full cover is its own only child."""
    out = []
    for occ, used, src in _unpack(tab, words):
        out.extend((o, u, src) for o, u in _children(tab, occ, used))
    return _pack(tab, out)


def count_states(tab, words, nprefixes, nodes=None) -> np.ndarray:
    """int64[nprefixes]: the covers below the states, summed by prefix.
    ``nodes``: a one-element list the placements made are added to."""
    counts = np.zeros(nprefixes, dtype=np.int64)
    if not tab.solvable:
        return counts
    full, buckets = tab.full, tab.buckets
    made = 0

    def below(occ, used):
        nonlocal made
        if occ == full:
            return 1
        c = (~occ & (occ + 1)).bit_length() - 1
        total = 0
        for m, p in buckets[c]:
            if not (m & occ) and not (p & used):
                made += 1
                total += below(occ | m, used | p)
        return total

    for occ, used, src in _unpack(tab, words):
        counts[src] += below(occ, used)
    if nodes is not None:
        nodes[0] += made
    return counts


def count(tab, prefixes, nodes=None) -> np.ndarray:
    """The twin: covers that extend each prefix, in plain Python."""
    return count_states(tab, states(tab, prefixes), len(prefixes), nodes)


# ------------------------------------------------------------------------------ C++ counter
def _cpu_lib():
    global _CPU
    if _CPU is None:
        if not os.path.exists(_CPU_PATH):
            raise RuntimeError(f"{_CPU_PATH} missing: run native/build.py")
        L = ctypes.CDLL(_CPU_PATH)
        P, L64, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
        L.hbmr_exactcover_count_cpu.argtypes = [I, P, P, P, I, I, P, L64, L64, P, P, I]
        L.hbmr_exactcover_count_cpu.restype = I
        _CPU = L
    return _CPU


def count_states_cpu(tab, words, nprefixes, threads=1, nodes=None) -> np.ndarray:
    counts = np.zeros(nprefixes, dtype=np.int64)
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, tab.words + 1)
    if not tab.solvable or not len(words):
        return counts
    made = np.zeros(1, dtype=np.uint64)
    m = np.ascontiguousarray(tab.m)
    rc = _cpu_lib().hbmr_exactcover_count_cpu(
        tab.words, m.ctypes.data, tab.p.ctypes.data, tab.off.ctypes.data, tab.nrows, tab.ncells,
        words.ctypes.data, len(words), nprefixes, counts.ctypes.data, made.ctypes.data,
        max(1, int(threads)))
    if rc != 0:
        raise RuntimeError(f"hbmr_exactcover_count_cpu failed with code {rc}")
    if nodes is not None:
        nodes[0] += int(made[0])
    return counts


def count_cpu(tab, prefixes, threads=1, nodes=None) -> np.ndarray:
    """int64 per prefix from the C++ counter, bit-equal to :func:`count`."""
    return count_states_cpu(tab, states(tab, prefixes), len(prefixes), threads, nodes)


def dump(tab, words, nprefixes, path):
    """The table and the states as native/tests/exactcover_selftest.cc reads them."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, tab.words + 1)
    with open(path, "wb") as f:
        f.write(np.array([tab.words, tab.nrows, tab.ncells, len(words), nprefixes],
                         dtype=np.int32).tobytes())
        for a in (np.ascontiguousarray(tab.m), tab.p, tab.off, words):
            f.write(a.tobytes())


# ------------------------------------------------------------------------------ GPU
def _table_args(tab, device):
    from . import _lib
    m, p, off = tab.on(device)
    return (tab.words, _lib.ptr(m), _lib.ptr(p), _lib.ptr(off), tab.nrows, tab.ncells)


def _check_capacity(tab, capacity):
    longest = int(np.diff(tab.off).max()) if tab.nrows else 1
    if capacity < max(1, longest):
        raise ValueError(f"capacity {capacity} is under the longest bucket ({longest}): "
                         "one state's children would not fit")


def expand_gpu(tab, words, capacity=DEFAULT_CAPACITY):
    """One level on the device: yields the children of ``words`` (a device
    int64[n, W + 1]) in order, as tensors of at most ``capacity`` states.  A
    level whose children would not fit one tensor is cut between states and
    written in parts.  Runs on the current stream."""
    import torch

    from . import _lib
    lib = _lib.load()
    _check_capacity(tab, capacity)
    n = int(words.shape[0])
    if n == 0:
        return
    args = _table_args(tab, words.device)
    st = _lib.stream_handle()
    nchild = torch.empty(n, dtype=torch.int32, device=words.device)
    _lib.check(lib.hbmr_exactcover_expand_count(*args, _lib.ptr(words), n, _lib.ptr(nchild), st),
               "hbmr_exactcover_expand_count")
    ends = torch.cumsum(nchild, 0, dtype=torch.int64)
    offs = ends - nchild
    ends_h = ends.cpu().numpy()
    a = 0
    while a < n:
        base = int(ends_h[a - 1]) if a else 0
        # the most states from a whose children fit
        b = int(np.searchsorted(ends_h, base + capacity, side="right"))
        b = min(max(b, a + 1), n)
        total = int(ends_h[b - 1]) - base
        if total:
            out = torch.empty((total, tab.words + 1), dtype=torch.int64, device=words.device)
            _lib.check(lib.hbmr_exactcover_expand_write(
                *args, _lib.ptr(words[a:]), b - a, _lib.ptr(offs[a:]), base, total,
                _lib.ptr(out), st), "hbmr_exactcover_expand_write")
            yield out
        a = b


def count_states_gpu(tab, words, counts, scratch=None, wg_clock=None):
    """The depth-first count below the device states ``words``, added to the
    device int64 ``counts`` (one per prefix).  ``scratch``: int64[2], the work
    counter (zeroed here) and the placements made (added to).  Runs on the
    current stream."""
    import torch

    from . import _lib
    lib = _lib.load()
    n = int(words.shape[0])
    if n == 0:
        return counts
    if scratch is None:
        scratch = torch.zeros(2, dtype=torch.int64, device=words.device)
    else:
        scratch[0] = 0
    _lib.check(lib.hbmr_exactcover_count(
        *_table_args(tab, words.device), _lib.ptr(words), n, int(counts.shape[0]),
        _lib.ptr(scratch), _lib.ptr(counts), _lib.ptr(wg_clock), _lib.stream_handle()),
        "hbmr_exactcover_count")
    return counts


def count_blocks(tab, n) -> int:
    """Workgroups the count kernel launches for ``n`` states."""
    from . import _lib
    return int(_lib.load().hbmr_exactcover_count_blocks(tab.words, tab.nrows, tab.ncells, n))


def count_gpu(tab, prefixes, stream=None, levels=DEFAULT_LEVELS, capacity=DEFAULT_CAPACITY,
              device=None, on_launch=None, stats=None):
    """Device int64 per prefix: the covers that extend it.  The prefixes'
    states are expanded ``levels`` levels breadth-first, a chunk of at most
    ``capacity`` states at a time (so frontier memory is bounded by
    ``levels * capacity`` states), and each last-level chunk is counted depth
    first.  Launches go to ``stream`` (the current stream by default).
    ``on_launch(kind, level, nstates)`` is called before each kernel group;
    ``stats``: a dict that gets ``placements``, the tree nodes the count
    kernel made (a device synchronise)."""
    import torch

    from . import _lib
    device = torch.device("cuda" if device is None else device)
    counts = torch.zeros(len(prefixes), dtype=torch.int64, device=device)
    if not tab.solvable or not len(prefixes):
        return counts                     # no cover exists: nothing is launched
    _check_capacity(tab, capacity)
    first = states(tab, prefixes).view(np.int64)
    scratch = torch.zeros(2, dtype=torch.int64, device=device)

    def descend(words, level):
        if level == levels:
            if on_launch:
                on_launch("count", level, int(words.shape[0]))
            count_states_gpu(tab, words, counts, scratch)
            return
        if on_launch:
            on_launch("expand", level, int(words.shape[0]))
        for part in expand_gpu(tab, words, capacity):
            descend(part, level + 1)

    with _lib.stream_ctx(stream):
        start = torch.from_numpy(first).to(device)
        for a in range(0, len(prefixes), capacity):
            descend(start[a:a + capacity], 0)
        if stats is not None:
            stats["placements"] = int(scratch[1])
    return counts
