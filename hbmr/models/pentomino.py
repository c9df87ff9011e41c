"""GPU Pentomino — DistributedPentomino (examples/dancing/DistributedPentomino.java)
as a split-level job.

The classic job writes one search prefix per input line and each map runs
Algorithm X below its lines.  Here the prefixes are the same ``split(depth)``
list, a map is a contiguous range of them, and it counts the tilings below its
range with the exact-cover kernels (native/kernels/exactcover.hip) on a GPU
slot or the C++ counter (native/cpu/exactcover.cc) on a CPU slot — one search,
bit-equal, so the hybrid scheduler may mix the two.  The reduce is a collective
sum, and rank 0 writes the classic job's ``part-00000``: ``solutions\\t<N>``.
"""
from __future__ import annotations

import functools

from ..gpu.splitjob import SplitJob, SplitSpec
from ..mapred import JobConf
from . import records, splits

WIDTH_KEY, HEIGHT_KEY, DEPTH_KEY = "pent.width", "pent.height", "pent.depth"
ONESIDED_KEY = "pent.onesided"
LEVELS_KEY = "hbmr.pentomino.gpu.levels"
CAPACITY_KEY = "hbmr.pentomino.gpu.capacity"


@functools.lru_cache(maxsize=4)
def problem(width, height, depth, onesided=False):
    """(placement table, prefixes) of a board: what every task of a job needs."""
    from ..examples.dancing import make_pentomino
    from ..ops import exactcover
    p = make_pentomino(width, height, onesided)
    return exactcover.table(p), p.split(depth)


def classic_maps(nprefixes):
    """The number of maps the classic job makes of so many prefix lines."""
    per = max(1, nprefixes // 16)
    return max(1, -(-nprefixes // per))


class PentominoSplitJob(splits.FinishesOutput, SplitJob):
    collective_reduce = True
    needs_reduce = True
    cache_inputs = False           # a split is its own spec: nothing to keep

    def configure(self, conf):
        from ..ops import exactcover
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.shape = (conf.get_int(WIDTH_KEY, 10), conf.get_int(HEIGHT_KEY, 6),
                      conf.get_int(DEPTH_KEY, 2), conf.get_boolean(ONESIDED_KEY, False))
        self.levels = conf.get_int(LEVELS_KEY, exactcover.DEFAULT_LEVELS)
        self.capacity = conf.get_int(CAPACITY_KEY, exactcover.DEFAULT_CAPACITY)

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        n = len(problem(*self.shape)[1])
        maps = max(1, min(n, conf.get_num_map_tasks()))
        out = []
        for i in range(maps):
            lo, hi = i * n // maps, (i + 1) * n // maps
            out.append(SplitSpec(i, f"pentomino:{self.shape}:{lo}:{hi}", "range",
                                 {"lo": lo, "hi": hi}, splits.place(i, maps, trackers), 0))
        return out

    def load_split(self, spec, device):
        return (spec.params["lo"], spec.params["hi"])

    def load_split_sample(self, spec, device, fraction):
        lo, hi = spec.params["lo"], spec.params["hi"]
        return (lo, lo + max(1, int((hi - lo) * fraction)))

    def split_nbytes(self, data):
        return 0

    # -- map --------------------------------------------------------------------------
    def map_gpu(self, ctx, data):
        from ..ops import exactcover
        tab, prefixes = problem(*self.shape)
        counts = exactcover.count_gpu(tab, prefixes[data[0]:data[1]],
                                      stream=getattr(ctx, "stream", None), levels=self.levels,
                                      capacity=self.capacity, device=ctx.device)
        return counts.sum()

    def map_cpu(self, ctx, data):
        from ..ops import exactcover
        tab, prefixes = problem(*self.shape)
        return int(exactcover.count_cpu(tab, prefixes[data[0]:data[1]]).sum())

    # -- reduce -----------------------------------------------------------------------
    def combine(self, ctx, outputs):
        import torch
        return torch.tensor([sum(int(o) for o in outputs)], dtype=torch.int64)

    def reduce(self, ctx, combined):
        t = combined
        if ctx.device is not None and ctx.device.type == "cuda":
            t = t.to(ctx.device)
        ctx.comm.all_reduce(t)
        total = int(t.cpu()[0])
        if self.out and ctx.rank == 0:
            with records.part_writer(self.out, "part-00000") as f:
                # no prefix, no map output: the classic reducer writes nothing
                if problem(*self.shape)[1]:
                    f.write(b"solutions\t%d\n" % total)
        return {"solutions": total}


def why_ineligible(out, base=None):
    """None if GPU Pentomino takes this job, else the reason it does not."""
    return splits.local_output_reason(out, base)


def gpu_job(out, width=10, height=6, depth=2, onesided=False, maps=None, base=None) -> JobConf:
    """Pentomino as a split-level job of ``maps`` maps (default: as many as the
    classic job makes of its prefix lines).  Raises ValueError, with the
    reason, for compressed output, an output directory that is not local, or a
    board the placement table does not hold."""
    from ..fs import strip_scheme
    why = why_ineligible(out, base)
    if why is not None:
        raise ValueError(f"pentomino into {out!r} is not eligible for the GPU: {why}")
    try:
        _, prefixes = problem(width, height, depth, bool(onesided))
    except ValueError as e:
        raise ValueError(f"pentomino {width}x{height} is not eligible for the GPU: {e}") from e
    job = splits.file_job(base, "dancingElephant-gpu", "hbmr.models.pentomino:PentominoSplitJob",
                          output=strip_scheme(str(out)),
                          maps=max(1, maps or classic_maps(len(prefixes))))
    job.set_int(WIDTH_KEY, width)
    job.set_int(HEIGHT_KEY, height)
    job.set_int(DEPTH_KEY, depth)
    job.set_boolean(ONESIDED_KEY, bool(onesided))
    job.set_num_reduce_tasks(1)
    return job
