"""MultiFileWordCount (src/examples/org/apache/hadoop/examples/MultiFileWordCount.java):
word count where each map reads several whole files (MultiFileInputFormat).

``-gpu`` runs the job as the split-level job of hbmr/models/wordtable.py (the
files of a map concatenated in HBM, text and word-table kernels on the GPU map
slots) with the same output, byte for byte.  An input the GPU job does not take
logs the reason and runs the classic job."""
from __future__ import annotations

import argparse
import logging

from ..io.writable import LongWritable, Text
from ..mapred import FileInputFormat, FileOutputFormat, JobClient, JobConf
from ..mapred.lib.basic import LongSumReducer, TokenCountMapper
from ..mapred.lib.combine import MultiFileInputFormat
from ._gpu import run_gpu_job

log = logging.getLogger("hbmr.examples.multifilewc")


def make_job(inp, out, maps=2, conf=None, reduces=None) -> JobConf:
    job = JobConf(conf)
    job.set_job_name("MultiFileWordCount")
    job.set_input_format(MultiFileInputFormat)
    job.set_num_map_tasks(maps)
    job.set_mapper_class(TokenCountMapper)
    job.set_combiner_class(LongSumReducer)
    job.set_reducer_class(LongSumReducer)
    job.set_output_key_class(Text)
    job.set_output_value_class(LongWritable)
    if reduces is not None:
        job.set_num_reduce_tasks(reduces)
    FileInputFormat.setInputPaths(job, *([inp] if isinstance(inp, str) else inp))
    FileOutputFormat.setOutputPath(job, out)
    return job


def run(inp, out, maps=2, reduces=None, conf=None, cluster=None, gpu=False):
    """Run the job; ``gpu``: as the split-level job of hbmr/models/wordtable.py,
    the classic job if it is not eligible (the reason is logged)."""
    rj = None
    if gpu:
        from ..models import wordtable
        r = JobConf(conf).get_num_reduce_tasks() if reduces is None else reduces
        rj = run_gpu_job(lambda: wordtable.multifilewc_job(inp, out, r, conf, maps),
                         "multifilewc", conf, cluster, log)
    if rj is not None:
        return rj
    return JobClient.runJob(make_job(inp, out, maps, conf, reduces), cluster=cluster)


def main(argv=None, cluster=None):
    ap = argparse.ArgumentParser(prog="hbmr multifilewc")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-m", type=int, default=2, help="maps")
    ap.add_argument("-r", type=int, default=None, help="reduces")
    ap.add_argument("-gpu", action="store_true",
                    help="run as a split-level job (text and word-table kernels on GPU slots)")
    a = ap.parse_args(argv)
    rj = run(a.input, a.output, a.m, a.r, cluster=cluster, gpu=a.gpu)
    return 0 if rj.isSuccessful() else 1
