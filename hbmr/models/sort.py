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

from ..gpu.splitjob import SplitJob, SplitSpec
from ..mapred import FileInputFormat, FileOutputFormat, JobConf
from . import records
from .wordcount import count_snappy_decoded

KEY_CLASS_KEY = "hbmr.sort.key.class"
VALUE_CLASS_KEY = "hbmr.sort.value.class"
PARTITION_FILE_KEY = "hbmr.sort.partition.file"


def owner_of(p, world, nparts):
    """The rank that sorts and writes partition ``p`` of ``nparts``."""
    return p * world // nparts


def _owned(rank, world, nparts):
    ps = [p for p in range(nparts) if owner_of(p, world, nparts) == rank]
    return (ps[0], ps[-1] + 1) if ps else (0, 0)


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


class SortSplitJob(SplitJob):
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
        splits = SequenceFileInputFormat().getSplits(JobConf(conf),
                                                     max(1, conf.get_num_map_tasks()))
        out = []
        for i, s in enumerate(splits):
            loc = [trackers[i * len(trackers) // len(splits)]] if trackers else []
            key = f"sort:{s.path}:{s.start}:{s.length}"
            out.append(SplitSpec(i, key, "file", {"path": s.path, "start": s.start,
                                                  "length": s.length}, loc, s.length))
        return out

    def load_split(self, spec: SplitSpec, device):
        p = spec.params
        data, index = records.load_job_split(self, spec.key, p["path"], p["start"], p["length"],
                                             device)
        return {"data": data, "index": index}

    def load_split_sample(self, spec, device, fraction):
        split = self.load_split(spec, device)
        n = max(1, int(split["index"].shape[1] * fraction))
        return {"data": split["data"], "index": split["index"][:, :n].contiguous()}

    def split_nbytes(self, split) -> int:
        return int(split["data"].numel() + split["index"].numel() * 8)

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, split):
        import torch

        from ..mapred import counters as C
        from ..ops import recsort
        data, index = split["data"], split["index"]
        n = int(index.shape[1])
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_RECORDS, n)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        count_snappy_decoded(self, ctx)
        perm, nrec, nbytes, blob = recsort.sort_records(
            data, index, self.nparts, self.split_points, getattr(ctx, "stream", None))
        meta = _meta(index)[perm.to(index.device).long()]
        return {"blob": blob, "meta": meta, "records": nrec, "bytes": nbytes}

    def map_gpu(self, ctx, split):
        return self._map(ctx, split)

    def map_cpu(self, ctx, split):
        return self._map(ctx, split)

    # -- shuffle + reduce -------------------------------------------------------------
    def combine(self, ctx, outputs):
        """The tracker's map outputs regrouped by destination rank: each output
        is ordered by partition and a rank owns consecutive partitions, so a
        destination's share of an output is one slice."""
        import torch
        dev = ctx.device if ctx.device is not None else torch.device("cpu")
        W = max(1, ctx.world_size)
        blobs, metas, send_bytes, send_recs = [], [], [], []
        for j in range(W):
            pa, pb = _owned(j, W, self.nparts)
            nb = nr = 0
            for o in outputs:
                b0, b1 = sum(o["bytes"][:pa]), sum(o["bytes"][:pb])
                r0, r1 = sum(o["records"][:pa]), sum(o["records"][:pb])
                blobs.append(o["blob"][b0:b1].to(dev))
                metas.append(o["meta"][r0:r1].to(dev))
                nb += b1 - b0
                nr += r1 - r0
            send_bytes.append(nb)
            send_recs.append(nr)
        blob = torch.cat(blobs) if blobs else torch.empty(0, dtype=torch.uint8, device=dev)
        meta = torch.cat(metas) if metas else torch.empty((0, 3), dtype=torch.int64, device=dev)
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
        pa, pb = _owned(ctx.rank, max(1, ctx.world_size), self.nparts)
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

    def job_succeeded(self, jip):
        if self.out:
            records.finish_output(self.out)


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
    job = JobConf(base)
    job.set_job_name("sorter-gpu")
    job.set("hbmr.splitjob.class", "hbmr.models.sort:SortSplitJob")
    kc, vc = records.first_classes(records.input_files(inputs))
    job.set(KEY_CLASS_KEY, kc)
    job.set(VALUE_CLASS_KEY, vc)
    job.set_num_reduce_tasks(max(1, reduces))
    if partition_file and reduces > 1:
        job.set(PARTITION_FILE_KEY, partition_file)
    FileInputFormat.setInputPaths(job, *([inputs] if isinstance(inputs, str) else inputs))
    FileOutputFormat.setOutputPath(job, output)
    if maps:
        job.set_num_map_tasks(maps)
    return job
