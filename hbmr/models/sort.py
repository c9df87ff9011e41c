"""GPU Sort — the identity-map/identity-reduce job of examples/Sort.java as a
split-level job.

The classic job runs IdentityMapper/IdentityReducer through the generic sort
buffer, record by record.  Here a split of a
``SequenceFile<BytesWritable|Text, *>`` lies in HBM as bytes + index: an
uncompressed one is indexed in one native pass (native/io/recindex.cc), a
Snappy RECORD- or BLOCK-compressed one is decoded and assembled into the same
frames on the device (hbmr/ops/seqz.py); the map
partitions (HashPartitioner over the key payload, or TotalOrderPartitioner's
split points), sorts by (partition, key bytes) and gathers the frames into one
blob per split (native/kernels/recsort.hip).  Partition ``p`` of
``R = mapred.reduce.tasks`` belongs to rank ``p*W//R``: the frames and their
lengths travel there by all-to-all-v, the owner sorts what it received with
the same device sort (a re-sort beats a merge on the GPU: SURVEY.md K8) and
writes ``part-NNNNN`` through the layout path of ``sequencefile.Writer``.

Per part the key order is the classic job's; among equal keys the values come
in (source rank, map, record) order — Hadoop does not fix their order across
maps either.
"""
from __future__ import annotations

from ..gpu.splitjob import SplitJob
from ..mapred import JobConf
from . import records, splits

KEY_CLASS_KEY = "hbmr.sort.key.class"
VALUE_CLASS_KEY = "hbmr.sort.value.class"
PARTITION_FILE_KEY = "hbmr.sort.partition.file"


def read_split_points(path, key_class):
    """The key payloads of a TotalOrderPartitioner partition file, in order."""
    from ..io import sequencefile as seqf
    pts = []
    with seqf.Reader(path) as r:
        while True:
            raw = r.next_raw()
            if raw is None:
                break
            pts.append(key_class.raw_sort_key(raw[0]))
    return pts


class SortSplitJob(splits.BothSlots, splits.FinishesOutput, splits.RecordSplits, SplitJob):
    collective_reduce = True
    needs_reduce = True

    def configure(self, conf):
        from ..io.writable import class_for_java_name
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.nparts = max(1, conf.get_num_reduce_tasks())
        self.key_class = class_for_java_name(conf.get(KEY_CLASS_KEY))
        self.value_class = class_for_java_name(conf.get(VALUE_CLASS_KEY))
        path = conf.get(PARTITION_FILE_KEY)
        self.split_points = None
        if path and self.nparts > 1:
            self.split_points = read_split_points(path, self.key_class)
            if len(self.split_points) != self.nparts - 1:
                raise ValueError(f"{path}: {len(self.split_points)} split points for "
                                 f"{self.nparts} partitions")

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        from ..mapred.formats import SequenceFileInputFormat
        found = SequenceFileInputFormat().getSplits(JobConf(conf),
                                                    max(1, conf.get_num_map_tasks()))
        return [splits.file_spec(i, splits.record_key(s.path, s.start, s.length), s.path, s.start,
                                 s.length, splits.place(i, len(found), trackers))
                for i, s in enumerate(found)]

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, split):
        from ..mapred import counters as C
        from ..ops import recsort
        data, index = split["data"], split["index"]
        n = int(index.shape[1])
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_RECORDS, n)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        splits.count_snappy_decoded(self, ctx)
        perm, nrec, nbytes, blob = recsort.sort_records(
            data, index, self.nparts, self.split_points, getattr(ctx, "stream", None))
        meta = _meta(index)[perm.to(index.device).long()]
        return {"blob": blob, "meta": meta, "records": nrec, "bytes": nbytes}

    # -- shuffle + reduce -------------------------------------------------------------
    def combine(self, ctx, outputs):
        """(blob, meta, bytes per rank, records per rank): the map outputs
        regrouped by destination rank."""
        import torch
        (blob, send_bytes), (meta, send_recs) = splits.by_destination(
            outputs, max(1, ctx.world_size), self.nparts,
            [splits.Field("blob", "bytes", torch.uint8),
             splits.Field("meta", "records", torch.int64, (3,))], splits.device_of(ctx))
        return blob, meta, send_bytes, send_recs

    def reduce(self, ctx, combined):
        import torch

        from ..mapred import counters as C
        from ..ops import recsort
        blob, meta, send_bytes, send_recs = combined
        comm = ctx.comm
        rblob = comm.all_to_all_v(blob, send_bytes)[0]
        rmeta = comm.all_to_all_v(meta, send_recs)[0]
        flen = rmeta[:, 0].contiguous()
        foff = torch.cumsum(flen, 0) - flen
        index = torch.stack([foff, flen, foff + rmeta[:, 1], rmeta[:, 2]]).contiguous()
        perm, nrec = recsort.sort_perm(rblob, index, self.nparts, self.split_points)
        pa, pb = splits.owned(ctx.rank, max(1, ctx.world_size), self.nparts)
        if sum(nrec[:pa]) or sum(nrec[pb:]):
            raise RuntimeError("records of a partition this rank does not own arrived here")
        written = 0
        if self.out:
            r0 = 0
            for p in range(pa, pb):
                with records.part_writer(self.out, f"part-{p:05d}", self.key_class,
                                         self.value_class) as w:
                    written += recsort.write_part(w, rblob, index, perm[r0:r0 + nrec[p]])
                r0 += nrec[p]
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_INPUT_RECORDS, int(perm.numel()))
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_OUTPUT_RECORDS, written)
        return {"records": written, "parts": pb - pa}


def _meta(index):
    """int64[n, 3] per record: frame length, key payload offset in the frame,
    key payload length — what rebuilds an index over frames laid back to back."""
    import torch
    return torch.stack([index[1], index[2] - index[0], index[3]], dim=1)


def why_ineligible(inputs, base=None, in_format=None, out_format=None):
    """None if GPU Sort takes this job, else the reason it does not."""
    from ..mapred.formats import SequenceFileInputFormat, SequenceFileOutputFormat
    if in_format is not None and in_format is not SequenceFileInputFormat:
        return f"custom input format {in_format.__name__}"
    if out_format is not None and out_format is not SequenceFileOutputFormat:
        return f"custom output format {out_format.__name__}"
    if base is not None and base.get("mapred.output.key.comparator.class"):
        return f"custom key comparator {base.get('mapred.output.key.comparator.class')}"
    if base is not None and base.get_boolean("mapred.output.compress", False):
        return "compressed output"
    classes = set()
    for f in records.input_files(inputs):
        why = records.file_reason(f, classes)
        if why is not None:
            return why
    if len(classes) > 1:
        return "inputs of different key/value classes"
    return None


def gpu_job(inputs, output, reduces=1, partition_file=None, base=None, maps=None, in_format=None,
            out_format=None) -> JobConf:
    """Sort as a split-level job (GPU map slots, CPU slots per the hybrid cost
    model).  ``partition_file``: a TotalOrderPartitioner partition file whose
    keys become the split points.  Raises ValueError, with the reason, for
    anything not eligible: RECORD- or BLOCK-compressed input of a codec other
    than SnappyCodec, a key class other
    than BytesWritable or Text, a custom input/output format or comparator."""
    why = why_ineligible(inputs, base, in_format, out_format)
    if why is not None:
        raise ValueError(f"sort of {inputs!r} is not eligible for the GPU: {why}")
    job = splits.file_job(base, "sorter-gpu", "hbmr.models.sort:SortSplitJob", inputs, output, maps)
    kc, vc = records.first_classes(records.input_files(inputs))
    job.set(KEY_CLASS_KEY, kc)
    job.set(VALUE_CLASS_KEY, vc)
    job.set_num_reduce_tasks(max(1, reduces))
    if partition_file and reduces > 1:
        job.set(PARTITION_FILE_KEY, partition_file)
    return job
