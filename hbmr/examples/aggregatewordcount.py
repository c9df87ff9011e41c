"""AggregateWordCount / AggregateWordHistogram (src/examples/org/apache/hadoop/
examples/AggregateWord{Count,Histogram}.java) on the aggregate framework.

``-gpu`` runs either program as the split-level job of
hbmr/models/wordtable.py (text and word-table kernels on the GPU map slots)
with the same output, byte for byte.  An input the GPU job does not take logs
the reason and runs the classic job."""
from __future__ import annotations

import argparse
import logging

from ..io.writable import Text
from ..mapred import JobClient
from ..mapred.lib.aggregate import ValueAggregatorBaseDescriptor, ValueAggregatorJob
from ._gpu import run_gpu_job

log = logging.getLogger("hbmr.examples.aggregatewordcount")


class WordCountPlugIn(ValueAggregatorBaseDescriptor):
    def generateKeyValPairs(self, key, val):  # noqa: N802
        one = Text("1")
        return [self.generateEntry(self.LONG_VALUE_SUM, w, one) for w in str(val).split()]


class WordHistogramPlugIn(ValueAggregatorBaseDescriptor):
    def generateKeyValPairs(self, key, val):  # noqa: N802
        return [self.generateEntry(self.VALUE_HISTOGRAM, "WORD_HISTOGRAM", Text(f"{w}\t1"))
                for w in str(val).split()]


def run(inp, out, reduces=1, conf=None, cluster=None, histogram=False, gpu=False):
    """Run the job; ``gpu``: as the split-level job of hbmr/models/wordtable.py,
    the classic job if it is not eligible (the reason is logged)."""
    name = "aggregatewordhist" if histogram else "aggregatewordcount"
    rj = None
    if gpu:
        from ..models import wordtable
        rj = run_gpu_job(lambda: wordtable.gpu_job(name, inp, out, reduces, conf), name, conf,
                         cluster, log)
    if rj is not None:
        return rj
    job = ValueAggregatorJob.createValueAggregatorJob(
        inp, out, [WordHistogramPlugIn if histogram else WordCountPlugIn], reduces, conf)
    return JobClient.runJob(job, cluster=cluster)


def main(argv=None, cluster=None, histogram=False):
    ap = argparse.ArgumentParser(prog="hbmr aggregatewordcount")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("reduces", nargs="?", type=int, default=1)
    ap.add_argument("-gpu", action="store_true",
                    help="run as a split-level job (text and word-table kernels on GPU slots)")
    a = ap.parse_args(argv)
    rj = run(a.input, a.output, a.reduces, cluster=cluster, histogram=histogram, gpu=a.gpu)
    return 0 if rj.isSuccessful() else 1


def main_histogram(argv=None, cluster=None):
    return main(argv, cluster, histogram=True)
