"""GPU SecondarySort — the job of examples/SecondarySort.java as a split-level job.

The classic job parses "a b" lines in a Python mapper, sorts IntPair keys
through the generic sort buffer, partitions and groups by ``a`` alone and writes
a separator line per group, then "a\\tb" lines.  Here a text split is read into
HBM with LineRecordReader's boundary rule (the loader of GPU WordCount and GPU
Grep, under the same cache key), native/kernels/intpair.hip parses the lines
into 64-bit key words and the map sorts them by (partition, key).  Partition
``p`` of ``R = mapred.reduce.tasks`` belongs to rank ``p*W//R`` as in GPU Sort:
the keys travel there by all-to-all-v, the owner sorts what it received again
(a re-sort beats a merge on the GPU: SURVEY.md K8), formats each part on the
device and writes ``part-NNNNN``.  Equal keys cannot be told apart in the
output, so the parts are the classic job's byte for byte.

A split the device does not take — a byte >= 0x80, or a first or second token
that is not a plain int32 decimal — is mapped again by the classic expression
over the decoded text (hbmr.ops.intpair.parse_slow) and counted in
``SECONDARYSORT_CPU_FALLBACK_SPLITS``; a line the classic map fails on fails
this map too.
"""
from __future__ import annotations

import os

from ..gpu.splitjob import SplitJob
from ..mapred import FileInputFormat, FileOutputFormat, JobConf
from . import records
from .sort import _owned
from .wordcount import WordCountSplitJob, compressed_input_reason, count_snappy_decoded

SECONDARYSORT_GROUP = "hbmr.SecondarySortCounters"
SECONDARYSORT_CPU_FALLBACK_SPLITS = "SECONDARYSORT_CPU_FALLBACK_SPLITS"
SEPARATOR_KEY = "mapred.textoutputformat.separator"


class SecondarySortSplitJob(SplitJob):
    collective_reduce = True
    needs_reduce = True

    get_splits = WordCountSplitJob.get_splits
    load_split = WordCountSplitJob.load_split

    def configure(self, conf):
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.nparts = max(1, conf.get_num_reduce_tasks())

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, data):
        """The same on both kinds of slot: the ops take the twin for a host
        tensor, and the irregular flag has one definition."""
        from ..mapred import counters as C
        from ..ops import intpair
        stream = getattr(ctx, "stream", None)
        count_snappy_decoded(self, ctx)
        parsed = intpair.parse(data, stream)
        keys = parsed.keys
        if parsed.irregular:
            ctx.reporter.incrCounter(SECONDARYSORT_GROUP, SECONDARYSORT_CPU_FALLBACK_SPLITS, 1)
            keys = intpair.parse_slow(bytes(data.cpu().numpy())).to(data.device)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_RECORDS, parsed.lines)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_OUTPUT_RECORDS, int(keys.numel()))
        keys, nrec = intpair.sort_keys(keys, self.nparts, stream)
        return {"keys": keys, "records": nrec}

    def map_gpu(self, ctx, data):
        return self._map(ctx, data)

    def map_cpu(self, ctx, data):
        return self._map(ctx, data)

    # -- shuffle + reduce -------------------------------------------------------------
    def combine(self, ctx, outputs):
        """The tracker's map outputs regrouped by destination rank: each output
        is ordered by partition and a rank owns consecutive partitions, so a
        destination's share of an output is one slice."""
        import torch
        dev = ctx.device if ctx.device is not None else torch.device("cpu")
        W = max(1, ctx.world_size)
        pieces, send = [], []
        for j in range(W):
            pa, pb = _owned(j, W, self.nparts)
            nr = 0
            for o in outputs:
                r0, r1 = sum(o["records"][:pa]), sum(o["records"][:pb])
                pieces.append(o["keys"][r0:r1].to(dev))
                nr += r1 - r0
            send.append(nr)
        keys = torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.int64, device=dev)
        return keys, send

    def reduce(self, ctx, combined):
        from ..mapred import counters as C
        from ..ops import intpair
        keys, send = combined
        got = ctx.comm.all_to_all_v(keys, send)[0].contiguous()
        got, nrec = intpair.sort_keys(got, self.nparts)
        pa, pb = _owned(ctx.rank, max(1, ctx.world_size), self.nparts)
        if sum(nrec[:pa]) or sum(nrec[pb:]):
            raise RuntimeError("records of a partition this rank does not own arrived here")
        groups, r0 = 0, sum(nrec[:pa])
        for p in range(pa, pb):
            text, g = intpair.format_part(got[r0:r0 + nrec[p]])
            groups += g
            r0 += nrec[p]
            if self.out:
                with records.part_writer(self.out, f"part-{p:05d}") as f:
                    f.write(text.cpu().numpy().tobytes())
        n = int(got.numel())
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_INPUT_GROUPS, groups)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_INPUT_RECORDS, n)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_OUTPUT_RECORDS, n + groups)
        return {"records": n, "groups": groups, "parts": pb - pa}

    def job_succeeded(self, jip):
        if self.out:
            records.finish_output(self.out)


def why_ineligible(inputs, base=None):
    """None if GPU SecondarySort takes this job, else the reason it does not."""
    if base is not None and base.get_boolean("mapred.output.compress", False):
        return "compressed output"
    if base is not None and base.get(SEPARATOR_KEY, "\t") != "\t":
        return f"{SEPARATOR_KEY} is not a tab"
    for f in records.input_files(inputs):
        if not os.path.isfile(f):
            return f"input {f} is not a local file"
        if compressed_input_reason(f) is not None:
            return compressed_input_reason(f)
    return None


def gpu_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    """SecondarySort as a split-level job (GPU map slots, CPU slots per the
    hybrid cost model).  Raises ValueError, with the reason, for anything not
    eligible: an input that is not a local file or carries the extension of
    a compression codec other than Snappy, compressed output, an output separator other than tab."""
    why = why_ineligible(inputs, base)
    if why is not None:
        raise ValueError(f"secondarysort of {inputs!r} is not eligible for the GPU: {why}")
    job = JobConf(base)
    job.set_job_name("secondary sort-gpu")
    job.set("hbmr.splitjob.class", "hbmr.models.secondarysort:SecondarySortSplitJob")
    job.set_num_reduce_tasks(max(1, reduces))
    FileInputFormat.setInputPaths(job, *([inputs] if isinstance(inputs, str) else inputs))
    FileOutputFormat.setOutputPath(job, output)
    if maps:
        job.set_num_map_tasks(maps)
    return job
