"""Grep: count regex matches, then sort by count descending
(src/examples/org/apache/hadoop/examples/Grep.java: a RegexMapper +
LongSumReducer job into a temp SequenceFile, then an InverseMapper sort job
with LongWritable.DecreasingComparator and one reducer).

``-gpu`` runs the search job as the split-level job of hbmr/models/grep.py
(DFA regex kernels on the GPU map slots); the sort job is the same.  A pattern
the GPU matcher does not take, or an input it does not read (not a local file,
or compressed with a codec other than Snappy), logs the reason and runs the
classic search."""
from __future__ import annotations

import argparse
import logging
import os
import shutil
import tempfile

from ..io.writable import LongWritable, Text
from ..mapred import FileInputFormat, FileOutputFormat, JobClient, JobConf
from ..mapred.formats import SequenceFileInputFormat, SequenceFileOutputFormat
from ..mapred.lib.basic import InverseMapper, LongSumReducer, RegexMapper
from ._gpu import run_gpu_job

log = logging.getLogger("hbmr.examples.grep")


class DecreasingLong:
    """LongWritable.DecreasingComparator as a sort key over serialised keys."""

    def sort_key(self, kb):
        return -int.from_bytes(kb[:8], "big", signed=True)


def _search_gpu(inp, out, regex, group, conf, cluster):
    """The search job as a split job; None if the pattern or an input is not eligible."""
    from ..models import grep as G
    return run_gpu_job(lambda: G.gpu_job(inp, out, regex, group, base=conf), "search", conf,
                       cluster, log)


def run(inp, out, regex, group=0, conf=None, cluster=None, verbose=False, gpu=False):
    tmp = tempfile.mkdtemp(prefix="grep-temp-")
    try:
        if not gpu or _search_gpu(inp, os.path.join(tmp, "out"), regex, group, conf,
                                  cluster) is None:
            _search(inp, os.path.join(tmp, "out"), regex, group, conf, cluster, verbose)
        return _sort(os.path.join(tmp, "out"), out, conf, cluster, verbose)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _search(inp, out, regex, group, conf, cluster, verbose):
    grep = JobConf(conf)
    grep.set_job_name("grep-search")
    FileInputFormat.setInputPaths(grep, *([inp] if isinstance(inp, str) else inp))
    grep.set_mapper_class(RegexMapper)
    grep.set("mapred.mapper.regex", regex)
    grep.set_int("mapred.mapper.regex.group", group)
    grep.set_combiner_class(LongSumReducer)
    grep.set_reducer_class(LongSumReducer)
    FileOutputFormat.setOutputPath(grep, out)
    grep.set_output_format(SequenceFileOutputFormat)
    grep.set_output_key_class(Text)
    grep.set_output_value_class(LongWritable)
    JobClient.runJob(grep, cluster=cluster, verbose=verbose)


def _sort(inp, out, conf, cluster, verbose):
    sort = JobConf(conf)
    sort.set_job_name("grep-sort")
    FileInputFormat.setInputPaths(sort, inp)
    sort.set_input_format(SequenceFileInputFormat)
    sort.set_mapper_class(InverseMapper)
    sort.set_num_reduce_tasks(1)
    FileOutputFormat.setOutputPath(sort, out)
    sort.set_map_output_key_class(LongWritable)
    sort.set_map_output_value_class(Text)
    sort.set_output_key_class(LongWritable)
    sort.set_output_value_class(Text)
    sort.set_output_key_comparator_class(DecreasingLong)
    return JobClient.runJob(sort, cluster=cluster, verbose=verbose)


def main(argv=None, cluster=None):
    ap = argparse.ArgumentParser(prog="hbmr grep")
    ap.add_argument("indir")
    ap.add_argument("outdir")
    ap.add_argument("regex")
    ap.add_argument("group", nargs="?", type=int, default=0)
    ap.add_argument("-gpu", action="store_true",
                    help="run the search as a split-level job (DFA regex kernels on GPU slots)")
    a = ap.parse_args(argv)
    rj = run(a.indir, a.outdir, a.regex, a.group, cluster=cluster, verbose=True, gpu=a.gpu)
    return 0 if rj.isSuccessful() else 1
