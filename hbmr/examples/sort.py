"""Sort: identity map/reduce over SequenceFiles, optionally totally ordered
(src/examples/org/apache/hadoop/examples/Sort.java: -inFormat/-outFormat,
-outKey/-outValue, -r reduces, -totalOrder pcnt numSamples maxSplits →
InputSampler.RandomSampler + TotalOrderPartitioner).

``-gpu`` runs the job as the split-level job of hbmr/models/sort.py (record
sort kernels on the GPU map slots); with ``-totalOrder`` the partition file is
sampled as always and its keys are the split points.  An input the GPU sort
does not take logs the reason and runs the classic job."""
from __future__ import annotations

import argparse
import logging
import os

from ..io import sequencefile as seqf
from ..mapred import FileInputFormat, FileOutputFormat, JobClient, JobConf
from ..mapred.formats import SequenceFileInputFormat, SequenceFileOutputFormat
from ..mapred.lib.basic import IdentityMapper, IdentityReducer, InputSampler, TotalOrderPartitioner
from ..utils.reflection import load_class
from ._gpu import run_gpu_job

log = logging.getLogger("hbmr.examples.sort")


def make_job(inp, out, reduces=1, total_order=None, conf=None, in_format=None,
             out_format=None) -> JobConf:
    job = JobConf(conf)
    job.set_job_name("sorter")
    FileInputFormat.setInputPaths(job, *([inp] if isinstance(inp, str) else inp))
    FileOutputFormat.setOutputPath(job, out)
    job.set_input_format(in_format or SequenceFileInputFormat)
    job.set_output_format(out_format or SequenceFileOutputFormat)
    job.set_mapper_class(IdentityMapper)
    job.set_reducer_class(IdentityReducer)
    job.set_num_reduce_tasks(reduces)
    # key/value classes of the (first) input file
    first = _first_file(inp)
    if first and (in_format is None or in_format is SequenceFileInputFormat):
        with seqf.Reader(first) as r:
            job.set_output_key_class(r.key_class)
            job.set_output_value_class(r.value_class)
    if total_order is not None and reduces > 1:
        pcnt, num_samples, max_splits = total_order
        sampler = InputSampler(pcnt, num_samples, max_splits)
        fmt = (in_format or SequenceFileInputFormat)()
        path = os.path.join(os.path.dirname(os.path.abspath(out)),
                            f"_sortPartitioning-{os.path.basename(out)}")
        sampler.write_partition_file(fmt, job, path)
        job.set_partitioner_class(TotalOrderPartitioner)
    return job


def _sort_gpu(job, inp, out, reduces, conf, cluster, in_format, out_format):
    """The sort as a split job (partition file and split points of ``job``, the
    classic job already made); None if the input is not eligible."""
    from ..models import sort as S
    return run_gpu_job(
        lambda: S.gpu_job(inp, out, reduces, job.get("total.order.partitioner.path"), base=conf,
                          in_format=in_format, out_format=out_format), "sort", conf, cluster, log)


def run(inp, out, reduces=1, total_order=None, conf=None, cluster=None, in_format=None,
        out_format=None, gpu=False):
    """Run the sort; ``gpu``: as the split-level job of hbmr/models/sort.py
    (record sort kernels on the GPU map slots), the classic job if the input
    is not eligible (the reason is logged)."""
    job = make_job(inp, out, reduces, total_order, conf, in_format, out_format)
    rj = _sort_gpu(job, inp, out, reduces, conf, cluster, in_format, out_format) if gpu else None
    return rj if rj is not None else JobClient.runJob(job, cluster=cluster)


def _first_file(inp):
    p = inp if isinstance(inp, str) else inp[0]
    if os.path.isdir(p):
        fs = sorted(f for f in os.listdir(p) if not f.startswith(("_", ".")))
        return os.path.join(p, fs[0]) if fs else None
    return p if os.path.exists(p) else None


def main(argv=None, cluster=None):
    ap = argparse.ArgumentParser(prog="hbmr sort")
    ap.add_argument("indir")
    ap.add_argument("outdir")
    ap.add_argument("-r", type=int, default=1)
    ap.add_argument("-inFormat")
    ap.add_argument("-outFormat")
    ap.add_argument("-totalOrder", nargs=3, metavar=("pcnt", "numSamples", "maxSplits"))
    ap.add_argument("-gpu", action="store_true",
                    help="run as a split-level job (record sort kernels on GPU slots)")
    a = ap.parse_args(argv)
    to = None
    if a.totalOrder:
        to = (float(a.totalOrder[0]), int(a.totalOrder[1]), int(a.totalOrder[2]))
    rj = run(a.indir, a.outdir, a.r, to, cluster=cluster,
             in_format=load_class(a.inFormat) if a.inFormat else None,
             out_format=load_class(a.outFormat) if a.outFormat else None, gpu=a.gpu)
    return 0 if rj.isSuccessful() else 1
