"""GPU RandomWriter and RandomTextWriter — the generators of the Sort benchmark
chain (examples/RandomWriter.java, RandomTextWriter.java) as a map-only
split-level job.

The classic mappers draw every record from ``random.Random`` and append it to a
``SequenceFile.Writer`` one at a time.  Here a map plans its records on the
device (lengths, the stop rule, the file layout), fills the whole file body
with the record generator kernels (native/kernels/recgen.hip; the CPU twin on
CPU slots) and writes ``part-NNNNN`` in one piece through the layout path of
``sequencefile.Writer``.  The records are those of :mod:`hbmr.ops.recgen`: the
classic mapper's shape, stop rule and counters, bytes that depend only on
(``hbmr.randomwrite.seed``, map, record, offset) — the classic job seeds
itself from Python's per-process string hash, so its bytes are its own.

A map that produced its file in one chunk leaves the body and its record index
in the tracker's split cache under the key GPU Sort and GPU SortValidator give
a file they read as one split, as what ``records.load_record_split`` would
load from the finished file: ``randomwriter -gpu``, ``sort -gpu`` and
``sortvalidate -gpu`` on one cluster read no input from disk.
"""
from __future__ import annotations

import os
import struct

from ..gpu.splitjob import SplitJob, SplitSpec
from ..mapred import JobConf
from . import records, splits

SEED_KEY = "hbmr.randomwrite.seed"
RESIDENT_KEY = "hbmr.randomwrite.gpu.resident"
CHUNK_KEY = "hbmr.randomwrite.gpu.chunk.bytes"
TEXT_KEY = "hbmr.randomwrite.text"
BYTES_CLASS = "org.apache.hadoop.io.BytesWritable"
TEXT_CLASS = "org.apache.hadoop.io.Text"


def record_params(conf, text):
    """(bytes per map, (min key, max key, min value, max value)) of the
    ``test.randomwrite.*`` / ``test.randomtextwrite.*`` keys, with the classic
    mappers' defaults."""
    if text:
        p = "test.randomtextwrite."
        return conf.get_long(p + "bytes_per_map", 1 << 20), (
            conf.get_int(p + "min_words_key", 5), conf.get_int(p + "max_words_key", 10),
            conf.get_int(p + "min_words_value", 10), conf.get_int(p + "max_words_value", 100))
    p = "test.randomwrite."
    return conf.get_long(p + "bytes_per_map", 1 << 20), (
        conf.get_int(p + "min_key", 10), conf.get_int(p + "max_key", 1000),
        conf.get_int(p + "min_value", 0), conf.get_int(p + "max_value", 20000))


def vocabulary():
    """RandomTextWriter's words."""
    from ..examples import randomwriter
    return randomwriter._WORDS


class RandomWriteSplitJob(splits.BothSlots, splits.FinishesOutput, SplitJob):
    collective_reduce = True
    needs_reduce = False
    cache_inputs = False           # a split is its own spec: nothing to keep

    def configure(self, conf):
        from ..io.writable import class_for_java_name
        from ..ops import recgen
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.text = conf.get_boolean(TEXT_KEY, False)
        self.kind = recgen.TEXT if self.text else recgen.BYTES
        self.total, params = record_params(conf, self.text)
        self.params = recgen.check_params(self.kind, params)
        self.vocabulary = recgen.Vocabulary(vocabulary()) if self.text else None
        self.seed = conf.get_long(SEED_KEY, 0)
        self.resident = conf.get_boolean(RESIDENT_KEY, True)
        self.chunk_bytes = max(1, conf.get_long(CHUNK_KEY, 1 << 30))
        self.record_class = class_for_java_name(TEXT_CLASS if self.text else BYTES_CLASS)

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        maps = max(1, conf.get_num_map_tasks())
        return [SplitSpec(i, f"randomwrite:{self.out}:{self.seed}:{i}", "synthetic", {"map": i},
                          splits.place(i, maps, trackers), max(0, self.total))
                for i in range(maps)]

    def load_split(self, spec, device):
        return spec

    def load_split_sample(self, spec, device, fraction):
        return spec

    def split_nbytes(self, data):
        return 0

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, spec):
        from ..io import sequencefile as seqf
        from ..mapred import counters as C
        from ..ops import recgen
        m = int(spec.params["map"])
        dev = ctx.device if ctx.device is not None else "cpu"
        stream = getattr(ctx, "stream", None)
        name = f"part-{m:05d}"
        left, first, chunks, kept = self.total, 0, 0, None
        with records.part_writer(self.out, name, self.record_class, self.record_class) as w:
            escape = struct.pack(">i", seqf.SYNC_ESCAPE) + w.sync
            while left > 0:
                # the layout continues at the writer's position from chunk to chunk
                data, p = recgen.generate(self.kind, self.seed, m, first, left, self.params, dev,
                                          w.out.tell(), w.last_sync_pos, self.vocabulary,
                                          self.chunk_bytes, escape, stream)
                w.append_frames(data.cpu().numpy(), p.gaps)
                n = int(p.index.shape[1])
                first += n
                left -= p.payload
                chunks += 1
                kept = (data, p.index) if chunks == 1 else None
            size = w.out.tell()
        rep = ctx.reporter
        rep.incrCounter(C.TASK_GROUP, C.MAP_OUTPUT_RECORDS, first)
        if self.text:
            rep.incrCounter("RandomTextWriter", "BYTES_WRITTEN", self.total - left)
        else:
            rep.incrCounter("RandomWriter", "RECORDS_WRITTEN", first)
            rep.incrCounter("RandomWriter", "BYTES_WRITTEN", self.total - left)
        if self.resident and kept is not None:
            self._keep(ctx, name, size, kept, dev)
        return {"records": first, "bytes": size}

    def _keep(self, ctx, name, size, kept, dev):
        """The finished file's split, as ``records.load_record_split`` would
        load it, into the tracker's split cache for the device the map ran on.
        The path is spelled as SequenceFileInputFormat.list_status reports it."""
        import torch

        from ..fs import strip_scheme
        cache = getattr(ctx, "split_cache", None)
        if cache is None:
            return
        data, index = kept
        where = dev.index if isinstance(dev, torch.device) and dev.type == "cuda" else "cpu"
        key = splits.whole_file_key(os.path.join(strip_scheme(self.out), name), size)
        split = {"data": data, "index": index}
        try:
            cache.put(key, where, split, int(data.numel() + index.numel() * 8))
        except Exception:  # noqa: BLE001  (a cache that turns the entry away: the file stands)
            pass


def why_ineligible(out, text=False, base=None):
    """None if GPU RandomWriter takes this job, else the reason it does not."""
    from ..ops import recgen
    why = splits.local_output_reason(out, base)
    if why is None and text:
        why = recgen.vocabulary_reason(vocabulary())
    return why


def gpu_job(out, maps=2, bytes_per_map=1 << 20, text=False, seed=0, base=None) -> JobConf:
    """RandomWriter (``text``: RandomTextWriter) as a map-only split-level job
    of ``maps`` maps.  Raises ValueError, with the reason, for anything it does
    not take: compressed output, an output directory that is not local, a
    vocabulary beyond what the text kernels hold in LDS, record bounds under
    which no record ever adds a byte."""
    from ..ops import recgen
    why = why_ineligible(out, text, base)
    if why is not None:
        name = "randomtextwriter" if text else "randomwriter"
        raise ValueError(f"{name} into {out!r} is not eligible for the GPU: {why}")
    job = splits.file_job(base, "random-text-writer-gpu" if text else "random-writer-gpu",
                          "hbmr.models.randomwrite:RandomWriteSplitJob", output=out,
                          maps=max(1, maps))
    job.set_boolean(TEXT_KEY, bool(text))
    job.set_long("test.randomtextwrite.bytes_per_map" if text else
                 "test.randomwrite.bytes_per_map", bytes_per_map)
    job.set_long(SEED_KEY, seed)
    job.set_num_reduce_tasks(0)
    recgen.check_params(recgen.TEXT if text else recgen.BYTES, record_params(job, text)[1])
    return job
