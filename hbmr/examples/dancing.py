"""Dancing links (Knuth's Algorithm X) with Sudoku and pentomino tilings, and a
distributed pentomino job (src/examples/org/apache/hadoop/examples/dancing/
{DancingLinks,Sudoku,Pentomino,DistributedPentomino}.java).

The distributed job enumerates the search tree to a fixed depth on the client,
writes one prefix per input line (NLineInputFormat, one line per map) and each
map counts the solutions below its prefix; a reducer sums them.

``pentomino -gpu`` runs the count as the split-level job of
hbmr/models/pentomino.py (exact-cover kernels on the GPU map slots, the same
search in C++ on CPU slots) over the same prefixes, with the same
``part-00000``; ``-onesided`` takes the 18 one-sided pentominoes
(:class:`OneSidedPentomino`), on either path.
"""
from __future__ import annotations

import argparse
import logging
import os
import tempfile

from ..io.writable import LongWritable, Text
from ..mapred import FileInputFormat, FileOutputFormat, JobClient, JobConf, Mapper, Reducer
from ..mapred.formats import NLineInputFormat

log = logging.getLogger("hbmr.examples.pentomino")


class DancingLinks:
    """Exact cover over ``ncols`` columns (the first ``primary`` must be covered
    exactly once; the rest at most once).  Rows are lists of column indices."""

    def __init__(self, ncols, primary=None):
        self.ncols = ncols
        self.primary = ncols if primary is None else primary
        self.rows: list[list[int]] = []
        self.row_names: list = []

    def add_row(self, cols, name=None):
        self.rows.append(sorted(set(cols)))
        self.row_names.append(name if name is not None else len(self.rows) - 1)

    # A compact set-based Algorithm X (the column choice heuristic: fewest rows)
    def _prepare(self):
        cols = {c: set() for c in range(self.ncols)}
        for i, r in enumerate(self.rows):
            for c in r:
                cols[c].add(i)
        return cols

    @staticmethod
    def _select(cols, rows, r):
        removed = []
        for j in rows[r]:
            for i in cols[j]:
                for k in rows[i]:
                    if k != j:
                        cols[k].discard(i)
            removed.append(cols.pop(j))
        return removed

    @staticmethod
    def _deselect(cols, rows, r, removed):
        for j in reversed(rows[r]):
            cols[j] = removed.pop()
            for i in cols[j]:
                for k in rows[i]:
                    if k != j:
                        cols[k].add(i)

    def _search(self, cols, partial, on_solution, limit=None, prefix_depth=None, prefixes=None):
        primary = [c for c in cols if c < self.primary]
        if not primary:
            if prefixes is not None:
                prefixes.append(list(partial))
                return 1
            on_solution([self.row_names[r] for r in partial])
            return 1
        if prefix_depth is not None and len(partial) == prefix_depth:
            prefixes.append(list(partial))
            return 0
        c = min(primary, key=lambda x: len(cols[x]))
        count = 0
        for r in sorted(cols[c]):
            partial.append(r)
            removed = self._select(cols, self.rows, r)
            count += self._search(cols, partial, on_solution, limit, prefix_depth, prefixes)
            self._deselect(cols, self.rows, r, removed)
            partial.pop()
            if limit is not None and count >= limit:
                break
        return count

    def solve(self, on_solution=lambda s: None, limit=None, prefix=()):
        cols = self._prepare()
        for r in prefix:
            self._select(cols, self.rows, r)
        return self._search(cols, list(prefix), on_solution, limit)

    def split(self, depth):
        """All partial solutions (row index lists) of the given depth."""
        prefixes: list = []
        self._search(self._prepare(), [], lambda s: None, None, depth, prefixes)
        return prefixes


# ------------------------------------------------------------------------ Sudoku
class Sudoku:
    """9×9 (or n²×n²) Sudoku as exact cover: cell, row-digit, col-digit, box-digit."""

    def __init__(self, grid):
        self.grid = [list(r) for r in grid]
        self.n = len(grid)
        self.b = int(round(self.n ** 0.5))

    @classmethod
    def parse(cls, text):
        rows = []
        for line in text.strip().splitlines():
            toks = line.replace(",", " ").split()
            if toks:
                rows.append([0 if t in ("?", ".", "0") else int(t) for t in toks])
        return cls(rows)

    def _dlx(self):
        n, b = self.n, self.b
        dl = DancingLinks(4 * n * n)
        for r in range(n):
            for c in range(n):
                given = self.grid[r][c]
                for d in range(1, n + 1):
                    if given and d != given:
                        continue
                    box = (r // b) * b + c // b
                    dl.add_row([r * n + c, n * n + r * n + d - 1, 2 * n * n + c * n + d - 1,
                                3 * n * n + box * n + d - 1], (r, c, d))
        return dl

    def solve(self, limit=None):
        out = []

        def emit(rows):
            g = [[0] * self.n for _ in range(self.n)]
            for r, c, d in rows:
                g[r][c] = d
            out.append(g)
        self._dlx().solve(emit, limit=limit)
        return out


# ------------------------------------------------------------------------ Pentomino
_PIECES = {  # cells of each pentomino in one orientation
    "F": [(0, 1), (0, 2), (1, 0), (1, 1), (2, 1)], "I": [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)],
    "L": [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1)], "N": [(0, 1), (1, 1), (2, 0), (2, 1), (3, 0)],
    "P": [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)], "T": [(0, 0), (0, 1), (0, 2), (1, 1), (2, 1)],
    "U": [(0, 0), (0, 2), (1, 0), (1, 1), (1, 2)], "V": [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)],
    "W": [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)], "X": [(0, 1), (1, 0), (1, 1), (1, 2), (2, 1)],
    "Y": [(0, 1), (1, 0), (1, 1), (2, 1), (3, 1)], "Z": [(0, 0), (0, 1), (1, 1), (2, 1), (2, 2)],
}


def _orientations(cells, fixed=False):
    outs = set()
    pts = cells
    for flip in ((False,) if fixed else (False, True)):
        p = [(r, -c) for r, c in pts] if flip else list(pts)
        for _ in range(4):
            p = [(c, -r) for r, c in p]
            mr, mc = min(r for r, _ in p), min(c for _, c in p)
            outs.add(tuple(sorted((r - mr, c - mc) for r, c in p)))
    return sorted(outs)


class Pentomino:
    """Tile a width×height board with the 12 pentominoes.  To count each
    distinct solution once, the X piece is restricted to the board's lower-left
    quadrant (removes the rotations/reflections of symmetric boards)."""

    pieces = _PIECES
    fixed = False          # True: rotations only (a mirror image is another piece)

    def __init__(self, width=10, height=6):
        self.w, self.h = width, height
        names = sorted(self.pieces)
        self.names = names
        ncols = len(names) + width * height
        self.dl = DancingLinks(ncols)
        for pi, name in enumerate(names):
            for shape in _orientations(self.pieces[name], fixed=self.fixed):
                ph = max(r for r, _ in shape) + 1
                pw = max(c for _, c in shape) + 1
                for y in range(height - ph + 1):
                    for x in range(width - pw + 1):
                        if name == "X" and not (x + 1 <= (width - 1) / 2 and
                                                y + 1 <= (height - 1) / 2):
                            continue
                        cells = [len(names) + (y + r) * width + (x + c) for r, c in shape]
                        self.dl.add_row([pi] + cells, (name, tuple((y + r, x + c)
                                                                  for r, c in shape)))

    def solve(self, on_solution=lambda s: None, prefix=()):
        return self.dl.solve(on_solution, prefix=prefix)

    def split(self, depth):
        return self.dl.split(depth)


_CHIRAL = "FLNPYZ"      # the shapes no rotation turns into their mirror image


class OneSidedPentomino(Pentomino):
    """The 18 one-sided pentominoes (pieces may be turned but not flipped over,
    so each chiral shape comes in both mirror forms, ``F`` and ``F'``) on a
    width×height board of 90 cells, e.g. 9×10.  Board columns and the X-piece
    restriction are Pentomino's: the piece set is closed under reflection, so
    the board's symmetries act on the solutions as they do there."""

    pieces = dict(_PIECES, **{n + "'": [(r, -c) for r, c in _PIECES[n]] for n in _CHIRAL})
    fixed = True

    def __init__(self, width=9, height=10):
        super().__init__(width, height)


def make_pentomino(width, height, onesided=False):
    return (OneSidedPentomino if onesided else Pentomino)(width, height)


# ------------------------------------------------------------------------ distributed
class PentominoMapper(Mapper):
    def configure(self, job):
        self.p = make_pentomino(job.get_int("pent.width", 10), job.get_int("pent.height", 6),
                                job.get_boolean("pent.onesided", False))

    def map(self, key, value, output, reporter):
        prefix = [int(t) for t in str(value).split(",") if t]
        n = self.p.solve(prefix=prefix)
        output.collect(Text("solutions"), LongWritable(n))


class SumReducer(Reducer):
    def reduce(self, key, values, output, reporter):
        output.collect(key, LongWritable(sum(v.get() for v in values)))


def distributed_pentomino(out, width=10, height=6, depth=2, conf=None, cluster=None,
                          verbose=False, onesided=False):
    p = make_pentomino(width, height, onesided)
    prefixes = p.split(depth)
    tmp = tempfile.mkdtemp(prefix="pent-")
    with open(os.path.join(tmp, "prefixes.txt"), "w") as f:
        for pre in prefixes:
            f.write(",".join(map(str, pre)) + "\n")
    job = JobConf(conf)
    job.set_job_name("dancingElephant")
    job.set_int("pent.width", width)
    job.set_int("pent.height", height)
    job.set_boolean("pent.onesided", bool(onesided))
    job.set_input_format(NLineInputFormat)
    job.set_int("mapred.line.input.format.linespermap", max(1, len(prefixes) // 16))
    job.set_mapper_class(PentominoMapper)
    job.set_combiner_class(SumReducer)
    job.set_reducer_class(SumReducer)
    job.set_output_key_class(Text)
    job.set_output_value_class(LongWritable)
    job.set_num_reduce_tasks(1)
    FileInputFormat.setInputPaths(job, tmp)
    FileOutputFormat.setOutputPath(job, out)
    JobClient.runJob(job, cluster=cluster, verbose=verbose)
    total = 0
    for fn in os.listdir(out):
        if fn.startswith("part-"):
            for line in open(os.path.join(out, fn)):
                total += int(line.split("\t")[1])
    return total


def main_sudoku(argv=None, cluster=None):
    ap = argparse.ArgumentParser(prog="hbmr sudoku")
    ap.add_argument("puzzle")
    a = ap.parse_args(argv)
    sols = Sudoku.parse(open(a.puzzle).read()).solve()
    for s in sols:
        print("\n".join(" ".join(map(str, r)) for r in s) + "\n")
    print(f"Found {len(sols)} solutions")
    return 0


def run_pentomino(out, width=10, height=6, depth=2, onesided=False, maps=None, conf=None,
                  cluster=None, gpu=False, verbose=False):
    """Count the tilings into ``out``; ``gpu``: as the split-level job of
    hbmr/models/pentomino.py, the classic job if the output is not eligible
    (the reason is logged).  Returns the count."""
    if gpu:
        from ..models import pentomino as P
        from ._gpu import run_gpu_job
        rj = run_gpu_job(lambda: P.gpu_job(out, width, height, depth, onesided, maps, base=conf),
                         "pentomino", conf, cluster, log)
        if rj is not None:
            return int(rj._impl.jip.result[0]["solutions"])
    return distributed_pentomino(out, width, height, depth, conf=conf, cluster=cluster,
                                 verbose=verbose, onesided=onesided)


def main_pentomino(argv=None, cluster=None):
    ap = argparse.ArgumentParser(prog="hbmr pentomino")
    ap.add_argument("output")
    ap.add_argument("-width", type=int, default=None)
    ap.add_argument("-height", type=int, default=None)
    ap.add_argument("-depth", type=int, default=2)
    ap.add_argument("-onesided", action="store_true",
                    help="the 18 one-sided pentominoes (default board 9x10)")
    ap.add_argument("-m", type=int, default=None, help="maps (with -gpu)")
    ap.add_argument("-gpu", action="store_true",
                    help="run as a split-level job (exact-cover kernels on GPU slots)")
    a = ap.parse_args(argv)
    width = a.width if a.width is not None else (9 if a.onesided else 10)
    height = a.height if a.height is not None else (10 if a.onesided else 6)
    n = run_pentomino(a.output, width, height, a.depth, a.onesided, a.m, cluster=cluster,
                      gpu=a.gpu, verbose=True)
    print(f"{n} solutions")
    return 0
