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

from ..gpu.splitjob import SplitJob
from ..mapred import JobConf
from . import records, splits

SECONDARYSORT_GROUP = "hbmr.SecondarySortCounters"
SECONDARYSORT_CPU_FALLBACK_SPLITS = "SECONDARYSORT_CPU_FALLBACK_SPLITS"


class SecondarySortSplitJob(splits.BothSlots, splits.FinishesOutput, splits.TextSplits, SplitJob):
    collective_reduce = True
    needs_reduce = True

    def configure(self, conf):
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.nparts = max(1, conf.get_num_reduce_tasks())

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, data):
        """The same on both kinds of slot: the irregular flag has one definition."""
        from ..mapred import counters as C
        from ..ops import intpair
        stream = getattr(ctx, "stream", None)
        splits.count_snappy_decoded(self, ctx)
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

    # -- shuffle + reduce -------------------------------------------------------------
    def combine(self, ctx, outputs):
        """(keys, keys per rank): the map outputs regrouped by destination rank."""
        import torch
        return splits.by_destination(outputs, max(1, ctx.world_size), self.nparts,
                                     [splits.Field("keys", "records", torch.int64)],
                                     splits.device_of(ctx))[0]

    def reduce(self, ctx, combined):
        from ..mapred import counters as C
        from ..ops import intpair
        keys, send = combined
        got = ctx.comm.all_to_all_v(keys, send)[0].contiguous()
        got, nrec = intpair.sort_keys(got, self.nparts)
        pa, pb = splits.owned(ctx.rank, max(1, ctx.world_size), self.nparts)
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


def why_ineligible(inputs, base=None):
    """None if GPU SecondarySort takes this job, else the reason it does not."""
    return splits.text_output_reason(base) or splits.text_input_reason(inputs)


def gpu_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    """SecondarySort as a split-level job (GPU map slots, CPU slots per the
    hybrid cost model).  Raises ValueError, with the reason, for anything not
    eligible: an input that is not a local file or carries the extension of
    a compression codec other than Snappy, compressed output, an output separator other than tab."""
    why = why_ineligible(inputs, base)
    if why is not None:
        raise ValueError(f"secondarysort of {inputs!r} is not eligible for the GPU: {why}")
    job = splits.file_job(base, "secondary sort-gpu",
                          "hbmr.models.secondarysort:SecondarySortSplitJob", inputs, output, maps)
    job.set_num_reduce_tasks(max(1, reduces))
    return job
