"""GPU SortValidator — the checks of benchmarks/sortvalidator.py as a map-only
split-level job.

The classic job calls a Python ``map()`` per record: a keyed hash, four counter
increments, a key compare and a key deserialisation.  Here every file of the
sort's input and output directories is one split, indexed in one native pass
(native/io/recindex.cc) and held in HBM as raw bytes + index — the same split,
under the same cache key, that GPU Sort loads for a file it reads as one split,
so validating right after ``sort -gpu`` on the same cluster finds the input
resident (the key names a file by path and size, as Sort's does: a file
rewritten in place to the same size on a live cluster is checked as loaded).
A map is the record digest, the count of descents and the partition check of
native/kernels/recvalidate.hip over the split; its results go into the classic
job's ``SortValidator`` counters.  The record hash differs from the
classic job's, which only ever compares its own two sums.
"""
from __future__ import annotations

import os

from ..gpu.splitjob import SplitJob
from ..mapred import JobConf
from . import records, splits

GROUP = "SortValidator"
SORTED_DIR_KEY = "sortvalidate.sorted.dir"
REDUCES_KEY = "sortvalidate.reduces"
TOTAL_ORDER_KEY = "sortvalidate.total.order"
JOB_NAME = "sortvalidate-gpu"


class ValidateSplitJob(splits.BothSlots, splits.RecordSplits, SplitJob):
    collective_reduce = True
    needs_reduce = False

    def configure(self, conf):
        self.conf = conf
        self.sorted_dir = os.path.abspath(conf.get(SORTED_DIR_KEY))
        self.reduces = conf.get_int(REDUCES_KEY, 1)
        self.total_order = conf.get_boolean(TOTAL_ORDER_KEY, False)

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        """One split per file, the whole file: GPU Sort's key and value for it."""
        from ..mapred.formats import SequenceFileInputFormat
        files = SequenceFileInputFormat().list_status(JobConf(conf))
        return [splits.file_spec(i, splits.whole_file_key(f.path, f.length), f.path, 0, f.length,
                                 splits.place(i, len(files), trackers))
                for i, f in enumerate(files)]

    # -- map --------------------------------------------------------------------------
    def side_of(self, path):
        """("IN" | "OUT", part number or None) of a file, as ValidateMapper.configure
        takes them."""
        if not os.path.abspath(path).startswith(self.sorted_dir):
            return "IN", None
        name = os.path.basename(path)
        return "OUT", int(name.split("-")[1]) if name.startswith("part-") else None

    def _map(self, ctx, split):
        from ..mapred import counters as C
        from ..ops import recvalidate
        data, index = split["data"], split["index"]
        side, part = self.side_of(ctx.spec.split["params"]["path"])
        if self.total_order:
            part = None
        n, nbytes, hs, hq, unsorted, mis = recvalidate.validate_records(
            data, index, side == "OUT", self.reduces, part, getattr(ctx, "stream", None))
        rep = ctx.reporter
        rep.incrCounter(C.TASK_GROUP, C.MAP_INPUT_RECORDS, n)
        rep.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        splits.count_snappy_decoded(self, ctx)
        rep.incrCounter(GROUP, f"{side}_RECORDS", n)
        rep.incrCounter(GROUP, f"{side}_BYTES", nbytes)
        rep.incrCounter(GROUP, f"{side}_HASH_SUM", hs)
        rep.incrCounter(GROUP, f"{side}_HASH_SQ_SUM", hq)
        if side == "OUT":
            rep.incrCounter(GROUP, "UNSORTED_RECORDS", unsorted)
            if part is not None:
                rep.incrCounter(GROUP, "MISPARTITIONED_RECORDS", mis)
        return {"records": n}


def why_ineligible(sort_input, sort_output):
    """None if GPU SortValidator takes the two directories, else the reason."""
    sides = []
    for d in (sort_input, sort_output):
        classes = set()
        for f in records.input_files(d):
            why = records.file_reason(f, classes)
            if why is not None:
                return why
        sides.append(classes)
    if len(sides[0] | sides[1]) > 1:
        return "sort input and output of different key/value classes"
    return None


def gpu_job(sort_input, sort_output, total_order=False, base=None) -> JobConf:
    """SortValidator over the sort's input and output directories as a map-only
    split-level job.  Raises ValueError, with the reason, when a file of either
    is not eligible (compressed, a key class other than BytesWritable or Text,
    not a local file) or the two sides differ in their classes."""
    why = why_ineligible(sort_input, sort_output)
    if why is not None:
        raise ValueError(f"validation of {sort_output!r} against {sort_input!r} is not eligible "
                         f"for the GPU: {why}")
    job = splits.file_job(base, JOB_NAME, "hbmr.models.sortvalidate:ValidateSplitJob",
                          [sort_input, sort_output])
    outs = [p for p in os.listdir(sort_output) if p.startswith("part-")]
    job.set(SORTED_DIR_KEY, sort_output)
    job.set_int(REDUCES_KEY, len(outs))
    job.set_boolean(TOTAL_ORDER_KEY, total_order)
    job.set_num_reduce_tasks(0)
    return job


def range_overlaps(sort_output, outs):
    """The adjacent non-empty parts (``outs``, in order) whose key ranges overlap:
    the first and last key payload of each from the native record index, of a
    compressed part from the split loader's."""
    from ..ops import recsort
    bounds = []
    for p in outs:
        path = os.path.join(sort_output, p)
        data, index = (t.numpy() for t in records.load_record_split(
            path, 0, os.path.getsize(path), "cpu"))
        if index.shape[1]:
            koff, klen = index[recsort.KOFF], index[recsort.KLEN]
            bounds.append(tuple(data[koff[i]:koff[i] + klen[i]].tobytes() for i in (0, -1)))
    return sum(1 for a, b in zip(bounds, bounds[1:]) if a[1] > b[0])
