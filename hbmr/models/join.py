"""GPU Join — the map-side join of examples/Join.java as a map-only split-level
job.

The classic job reads the i-th file of every source through
CompositeRecordReader: a heap of readers, one TupleWritable per output record.
Here map ``i`` indexes those files in one native pass each
(native/io/recindex.cc), joins them on the device (native/kernels/recjoin.hip:
group heads, cross ranks, tuple expansion, frame copy) and writes
``part-0000i`` through the layout path of ``sequencefile.Writer``.  The parts
hold the records of the classic job's parts, in the same order.  A join needs
no shuffle and no reduce: the job has maps only.
"""
from __future__ import annotations

import os
import re

from ..gpu.splitjob import SplitJob, SplitSpec
from ..mapred import JobConf
from . import records, splits

OP_KEY = "hbmr.join.op"
OUT_KEY_CLASS_KEY = "hbmr.join.output.key.class"
OUT_VALUE_CLASS_KEY = "hbmr.join.output.value.class"
JOB_NAME = "join-gpu"


class JoinSplitJob(splits.BothSlots, splits.FinishesOutput, SplitJob):
    collective_reduce = True
    needs_reduce = False

    def configure(self, conf):
        from ..io.writable import class_for_java_name
        from ..mapred.join import TupleWritable  # noqa: F401  (registers the class name)
        from ..ops import recjoin
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.op = conf.get(OP_KEY, "inner")
        self.chunk_bytes = conf.get_long(recjoin.CHUNK_BYTES_KEY, recjoin.CHUNK_BYTES_DEFAULT)
        self.key_class = class_for_java_name(conf.get(OUT_KEY_CLASS_KEY))
        self.value_class = class_for_java_name(conf.get(OUT_VALUE_CLASS_KEY))

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        """One split per partition: the i-th file of every source, in the order
        CompositeInputFormat.getSplits gives them."""
        from ..mapred.join import CompositeInputFormat
        found = CompositeInputFormat().getSplits(JobConf(conf), 1)
        out = []
        for i, cs in enumerate(found):
            files = [{"path": s.path, "start": s.start, "length": s.length} for s in cs.splits]
            key = "join:" + "|".join(f"{f['path']}:{f['start']}:{f['length']}" for f in files)
            out.append(SplitSpec(i, key, "file", {"files": files, "part": i},
                                 splits.place(i, len(found), trackers),
                                 sum(f["length"] for f in files)))
        return out

    def load_split(self, spec: SplitSpec, device):
        sources, vclasses = [], []
        for f in spec.params["files"]:
            sources.append(splits.load_job_split(self, spec.key, f["path"], f["start"],
                                                  f["length"], device))
            vclasses.append(records.first_classes([f["path"]])[1])
        return {"sources": sources, "value_classes": vclasses, "part": spec.params["part"],
                "files": [f["path"] for f in spec.params["files"]]}

    def load_split_sample(self, spec, device, fraction):
        split = self.load_split(spec, device)
        split["sources"] = [(d, i[:, :max(1, int(i.shape[1] * fraction))].contiguous())
                            for d, i in split["sources"]]
        split["probe"] = True            # joined, not written
        return split

    def split_nbytes(self, split) -> int:
        return int(sum(d.numel() + i.numel() * 8 for d, i in split["sources"]))

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, split):
        from ..io.writable import class_for_java_name
        from ..mapred import counters as C
        from ..ops import recjoin
        sources = split["sources"]
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_RECORDS,
                                 sum(int(i.shape[1]) for _, i in sources))
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES,
                                 sum(int(d.numel()) for d, _ in sources))
        splits.count_snappy_decoded(self, ctx)
        headers = None
        if self.op != "override":
            headers = recjoin.tuple_headers([class_for_java_name(v)
                                             for v in split["value_classes"]])
        stream = getattr(ctx, "stream", None)
        try:
            if split.get("probe") or not self.out:
                n = sum(int(ch.flen.size) for ch in recjoin.join_chunks(
                    sources, self.op, headers, self.chunk_bytes, stream))
                return {"records": n}
            with records.part_writer(self.out, f"part-{split['part']:05d}", self.key_class,
                                     self.value_class) as w:
                n = recjoin.write_join(w, sources, self.op, headers, self.chunk_bytes, stream)
        except recjoin.UnsortedInput as e:
            raise IOError(f"{split['files'][e.source]} is not sorted: the key of record "
                          f"{e.record} is below its predecessor's") from e
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_OUTPUT_RECORDS, n)
        return {"records": n}

    def job_succeeded(self, jip):
        if self.out:
            os.makedirs(self.out, exist_ok=True)
        super().job_succeeded(jip)


def _flat_sources(expr, base):
    """(op, [path]) of a flat ``op(tbl(SequenceFileInputFormat, path), ...)``
    over the built-in operators, else the reason as a string."""
    from ..mapred.formats import SequenceFileInputFormat
    from ..mapred.join.parser import COMPOSITE_TYPES, CNode, WNode, parse
    from ..utils.reflection import load_class
    root = parse(expr, None)
    if not isinstance(root, CNode) or root.ident not in COMPOSITE_TYPES:
        return f"join expression {expr!r} is not inner, outer or override over tables"
    paths = []
    for k in root.kids:
        if not isinstance(k, WNode):
            return f"nested join expression {k}"
        fmt = k.fmt_cls if isinstance(k.fmt_cls, type) else load_class(k.fmt_cls)
        if fmt is not SequenceFileInputFormat:
            return f"custom input format {fmt.__name__}"
        paths.append(k.indir)
    if not 2 <= len(paths) <= 8:
        return f"{len(paths)} join sources (2 to 8)"
    return root.ident, paths


def why_ineligible(inputs, join_type="inner", base=None, reduces=0, in_format=None,
                   out_format=None, expr=None):
    """None if GPU Join takes this job, else the reason it does not."""
    from ..mapred.formats import SequenceFileInputFormat, SequenceFileOutputFormat
    from ..mapred.join import CompositeInputFormat
    if base is not None:
        if base.get("mapred.join.keycomparator"):
            return f"custom key comparator {base.get('mapred.join.keycomparator')}"
        for k, v in base:
            if re.match(r"^mapred\.join\.define\.", k):
                return f"custom join operator {k} = {v}"
    if expr is None:
        if join_type not in ("inner", "outer", "override"):
            return f"join operator {join_type!r} (inner, outer or override only)"
        if in_format is not None and in_format is not SequenceFileInputFormat:
            return f"custom input format {in_format.__name__}"
        expr = CompositeInputFormat.compose(join_type, SequenceFileInputFormat, *inputs)
    try:
        flat = _flat_sources(expr, base)
    except ValueError as e:
        return str(e)
    if isinstance(flat, str):
        return flat
    op, paths = flat
    if reduces != 0:
        return f"{reduces} reduces (the GPU join is map-only)"
    if out_format is not None and out_format is not SequenceFileOutputFormat:
        return f"custom output format {out_format.__name__}"
    if base is not None and base.get_boolean("mapred.output.compress", False):
        return "compressed output"
    classes = set()
    for p in paths:
        if not os.path.exists(p):
            return f"input {p} is not a local path"
        for f in records.input_files(p):
            why = records.file_reason(f, classes)
            if why is not None:
                return why
    if len({k for k, _ in classes}) > 1:
        return "sources of different key classes"
    if op == "override" and len({v for _, v in classes}) > 1:
        return "override over sources of different value classes"
    return None


def gpu_job(inputs, output, join_type="inner", reduces=0, base=None, in_format=None,
            out_format=None, out_key=None, out_value=None, expr=None) -> JobConf:
    """The join of ``inputs`` (sorted, identically partitioned SequenceFile
    directories) as a map-only split-level job.  Raises ValueError, with the
    reason, for anything not eligible (:func:`why_ineligible`)."""
    from ..mapred.formats import SequenceFileInputFormat
    from ..mapred.join import CompositeInputFormat, TupleWritable
    from ..utils.reflection import class_name
    why = why_ineligible(inputs, join_type, base, reduces, in_format, out_format, expr)
    if why is not None:
        raise ValueError(f"join of {list(inputs)!r} is not eligible for the GPU: {why}")
    if expr is None:
        expr = CompositeInputFormat.compose(join_type, SequenceFileInputFormat, *inputs)
    op, paths = _flat_sources(expr, base)
    kc, vc = records.first_classes([f for p in paths for f in records.input_files(p)])
    if op != "override":
        vc = TupleWritable.JAVA_NAME
    job = splits.file_job(base, JOB_NAME, "hbmr.models.join:JoinSplitJob", output=output)
    job.set("mapred.join.expr", expr)
    job.set(OP_KEY, op)
    job.set(OUT_KEY_CLASS_KEY, class_name(out_key) if out_key is not None else kc)
    job.set(OUT_VALUE_CLASS_KEY, class_name(out_value) if out_value is not None else vc)
    job.set_num_reduce_tasks(0)
    return job
