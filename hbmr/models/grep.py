"""GPU Grep — the grep-search job of examples/Grep.java as a split-level job.

The classic job is RegexMapper + LongSumReducer (combiner and reducer) into a
temp ``SequenceFile<Text, LongWritable>`` that the grep-sort job reads.  Here a
text split is read into HBM with LineRecordReader's boundary rule (the loader
of GPU WordCount), the pattern is compiled once per job into a leftmost-first
DFA (hbmr/ops/grep.py) and native/kernels/grep.hip matches, selects
finditer's non-overlapping matches and counts them exactly (the fused
combiner).  The per-tracker match tables are merged and hash-partitioned like
HashPartitioner, shuffled like the word tables, and each tracker writes its
partition sorted by Text key order as ``part-NNNNN``.

A split that holds a byte ≥ 0x80 is mapped with the CPU twin (``re`` over the
decoded text differs from byte semantics there) and counted in
``GREP_CPU_FALLBACK_SPLITS``.
"""
from __future__ import annotations

from ..gpu.splitjob import SplitJob
from ..io.writable import LongWritable, Text
from ..mapred import JobConf
from . import records, splits

REGEX_KEY = "mapred.mapper.regex"
GROUP_KEY = "mapred.mapper.regex.group"
GREP_GROUP = "hbmr.GrepCounters"
GREP_CPU_FALLBACK_SPLITS = "GREP_CPU_FALLBACK_SPLITS"


class GrepSplitJob(splits.FinishesOutput, splits.TextSplits, SplitJob):
    collective_reduce = True
    needs_reduce = True

    def configure(self, conf):
        from ..ops import grep
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.regex = conf.get(REGEX_KEY, ".*")
        self.group = conf.get_int(GROUP_KEY, 0)
        # compiled once per job; None: every split takes the CPU map
        self.prog = grep.compile_pattern(
            self.regex, self.group, conf.get_int(grep.MAX_STATES_KEY, grep.MAX_STATES))

    def _input(self, ctx, data):
        from ..mapred import counters as C
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        splits.count_snappy_decoded(self, ctx)

    def map_gpu(self, ctx, data):
        from ..ops import grep
        self._input(ctx, data)
        if self.prog is None:
            raise ValueError(f"pattern {self.regex!r} is not eligible for the GPU: "
                             f"{grep.why_ineligible(self.regex, self.group)}")
        blob, counts, non_ascii = grep.count_matches(data, self.prog, getattr(ctx, "stream", None))
        if non_ascii:
            ctx.reporter.incrCounter(GREP_GROUP, GREP_CPU_FALLBACK_SPLITS, 1)
            blob, counts = grep.count_matches_cpu(bytes(data.cpu().numpy()), self.regex,
                                                  self.group)
            blob, counts = blob.to(data.device), counts.to(data.device)
        return blob, counts

    def map_cpu(self, ctx, data):
        from ..ops import grep
        self._input(ctx, data)
        raw = bytes(data.cpu().numpy())
        if max(raw, default=0) >= 0x80:     # a GPU slot would have fallen back here
            ctx.reporter.incrCounter(GREP_GROUP, GREP_CPU_FALLBACK_SPLITS, 1)
        return grep.count_matches_cpu(raw, self.regex, self.group)

    def combine(self, ctx, outputs):
        from ..ops import grep
        blob, cnt = splits.cat_tables(outputs, splits.device_of(ctx))
        return grep.merge_tables(blob, cnt, max(1, ctx.world_size))

    def reduce(self, ctx, combined):
        from ..mapred import counters as C
        from ..ops import grep, text
        blob, counts, part_bytes, part_words = combined
        rblob, rcounts = splits.shuffle_tables(ctx, blob, counts, part_bytes, part_words)
        mblob, mcounts, _, _ = grep.merge_tables(rblob, rcounts, 1)
        items = text.sorted_items(mblob, mcounts)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_INPUT_GROUPS, len(items))
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_OUTPUT_RECORDS, len(items))
        if self.out:
            with records.part_writer(self.out, f"part-{ctx.rank:05d}", Text, LongWritable) as w:
                for m, n in items:
                    w.append(Text(m), LongWritable(n))
        return {"distinct": len(items), "matches": sum(n for _, n in items)}


def gpu_job(inputs, output, regex, group=0, base=None, maps=None) -> JobConf:
    """The grep-search job as a split-level job (GPU map slots, CPU slots per
    the hybrid cost model).  Raises ValueError, with the reason, for a pattern
    the GPU matcher does not take, and for an input that is not a local file or
    carries the extension of a compression codec other than Snappy."""
    from ..ops import grep
    why = grep.why_ineligible(regex, group,
                              JobConf(base).get_int(grep.MAX_STATES_KEY, grep.MAX_STATES))
    if why is not None:
        raise ValueError(f"pattern {regex!r} is not eligible for the GPU: {why}")
    why = splits.text_input_reason(inputs)
    if why is not None:
        raise ValueError(f"grep of {inputs!r} is not eligible for the GPU: {why}")
    job = splits.file_job(base, "grep-search-gpu", "hbmr.models.grep:GrepSplitJob", inputs,
                          output, maps)
    job.set(REGEX_KEY, regex)
    job.set_int(GROUP_KEY, group)
    return job
