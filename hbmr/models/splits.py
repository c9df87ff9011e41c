"""What the split-level jobs share above the kernels: where a split is placed,
how a text or a SequenceFile split is named, keyed and loaded, which rank owns
a partition and how map outputs are regrouped for it, the word tables'
shuffle, and the eligibility checks and the tail of the job builders.  A new
job is a map plus a reduce on top of these (``records.py`` beside it holds the
SequenceFile loader and the part writer)."""
from __future__ import annotations

import collections
import os

from ..gpu.splitjob import SplitSpec
from ..mapred import FileInputFormat, FileOutputFormat, JobConf
from . import records

COMPRESSED_INPUT_GROUP = "hbmr.CompressedInputCounters"
SNAPPY_DECODED_BYTES = "SNAPPY_DECODED_BYTES"
SEPARATOR_KEY = "mapred.textoutputformat.separator"


# ----------------------------------------------------------------------------- placement
def place(i, n, trackers):
    """The preferred locations of split ``i`` of ``n``: the trackers take
    consecutive runs of splits, as even as they come."""
    return [trackers[i * len(trackers) // n]] if trackers else []


def file_spec(i, key, path, start, length, locations):
    """The SplitSpec of the byte range (start, length) of a file."""
    return SplitSpec(i, key, "file", {"path": path, "start": start, "length": length},
                     locations, length)


def device_of(ctx):
    """The device a tracker combines and reduces on: its GPU, else the host."""
    import torch
    return ctx.device if ctx.device is not None else torch.device("cpu")


# ----------------------------------------------------------------------------- the slots
class BothSlots:
    """One ``_map(ctx, data)`` for both kinds of slot: the ops take the CPU twin
    for a host tensor."""

    def map_gpu(self, ctx, data):
        return self._map(ctx, data)

    def map_cpu(self, ctx, data):
        return self._map(ctx, data)


class FinishesOutput:
    """Completes ``self.out`` (``mapred.output.dir``) when the job succeeds."""

    def job_succeeded(self, jip):
        if self.out:
            records.finish_output(self.out)


# ----------------------------------------------------------------------------- decoded bytes
def note_decoded(job, key, nbytes):
    """Notes that the load of the split ``key`` of ``job`` decoded ``nbytes``
    of Snappy input, for the map's counter."""
    notes = job.__dict__.setdefault("_snappy_decoded", {})
    notes[key] = notes.get(key, 0) + int(nbytes)


def count_snappy_decoded(job, ctx):
    """SNAPPY_DECODED_BYTES of a map: what its own load decoded, on the device
    or in the twin — nothing for a split found resident."""
    key = (getattr(ctx.spec, "split", None) or {}).get("key")
    n = job.__dict__.get("_snappy_decoded", {}).pop(key, 0)
    if n:
        ctx.reporter.incrCounter(COMPRESSED_INPUT_GROUP, SNAPPY_DECODED_BYTES, n)


def load_job_split(job, key, path, start, length, device):
    """``records.load_record_split`` for the split ``key`` of ``job``; the
    bytes a compressed file decoded to are noted for the map's
    SNAPPY_DECODED_BYTES (nothing for a split found resident)."""
    data, index, compressed = records.load_split_flagged(path, start, length, device)
    if compressed:
        note_decoded(job, key, data.numel())
    return data, index


# ----------------------------------------------------------------------------- text input
def read_text_split(path, start, length, chunk=1 << 16) -> bytes:
    """Bytes of the lines a LineRecordReader over (path, start, length) returns,
    newlines included: the first partial line is skipped unless start == 0, and
    the line running through the split end is read to its end."""
    from ..fs import strip_scheme
    end = start + length
    with open(strip_scheme(path), "rb") as f:
        f.seek(start)
        begin = start
        if start != 0:
            while True:
                buf = f.read(chunk)
                if not buf:
                    return b""
                i = buf.find(b"\n")
                if i >= 0:
                    begin += i + 1
                    break
                begin += len(buf)
        if begin > end:
            return b""
        f.seek(begin)
        body = f.read(end - begin)
        # finish the line that contains offset `end` (it starts at or before end)
        tail = []
        while True:
            buf = f.read(chunk)
            if not buf:
                break
            i = buf.find(b"\n")
            if i >= 0:
                tail.append(buf[:i + 1])
                break
            tail.append(buf)
        return body + b"".join(tail)


def is_snappy(path) -> bool:
    """Whether ``path`` carries SnappyCodec's extension: the one codec whose
    files the split-level text jobs take (decoded by hbmr/ops/snappydec.py)."""
    from ..io.compress import SnappyCodec, codec_for_path
    return isinstance(codec_for_path(path), SnappyCodec)


def compressed_input_reason(path):
    """``compressed input <path>`` for a file of any codec but Snappy, else None."""
    from ..io.compress import codec_for_path
    if codec_for_path(path) is not None and not is_snappy(path):
        return f"compressed input {path}"
    return None


def load_text_file(job, key, path, device):
    """The decoded bytes of the ``.snappy`` file ``path`` on ``device``.  The
    split ``key`` of ``job`` is noted as decoded here, for the map's counter."""
    from ..ops import snappydec
    t = snappydec.decode_file(path, device)
    note_decoded(job, key, t.numel())
    return t


def text_key(path, start, length):
    """The split-cache key of a text split."""
    return f"wc:{path}:{start}:{length}"


class TextSplits:
    """Text input of a split-level job: TextInputFormat's splits, read into
    device memory with LineRecordReader's boundary rule.  A `.snappy` file is
    one whole split: it is decoded on the device (hbmr/ops/snappydec.py) and
    the decoded text is what stays resident.  The jobs that inherit this share
    the splits they leave in the cache."""

    def get_splits(self, conf, trackers):
        from ..mapred.formats import TextInputFormat
        splits = TextInputFormat().getSplits(JobConf(conf), max(1, conf.get_num_map_tasks()))
        return [file_spec(i, text_key(s.path, s.start, s.length), s.path, s.start, s.length,
                          place(i, len(splits), trackers)) for i, s in enumerate(splits)]

    def load_split(self, spec: SplitSpec, device):
        import torch
        p = spec.params
        if is_snappy(p["path"]):
            # a compressed file is one whole split (TextInputFormat.is_splitable):
            # no first-line skip; what stays resident under the key is the text
            return load_text_file(self, spec.key, p["path"], device)
        data = read_text_split(p["path"], p["start"], p["length"])
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else \
            torch.empty(0, dtype=torch.uint8)
        return t if str(device) == "cpu" else t.to(device)


# ----------------------------------------------------------------------------- record input
def record_key(path, start, length):
    """The split-cache key of a SequenceFile split."""
    return f"sort:{path}:{start}:{length}"


def whole_file_key(path, size):
    """The split-cache key of the whole file ``path`` of ``size`` bytes: what
    GPU Sort gives a file it takes as one split, what GPU SortValidator reads
    and what GPU RandomWriter leaves behind, so the chain reads nothing from
    disk."""
    return record_key(path, 0, size)


class RecordSplits:
    """SequenceFile input of a split-level job: a split lies in device memory
    as ``{"data": uint8[bytes], "index": int64[4, n]}`` (records.py)."""

    def load_split(self, spec: SplitSpec, device):
        p = spec.params
        data, index = load_job_split(self, spec.key, p["path"], p["start"], p["length"],
                                             device)
        return {"data": data, "index": index}

    def load_split_sample(self, spec, device, fraction):
        split = self.load_split(spec, device)
        n = max(1, int(split["index"].shape[1] * fraction))
        return {"data": split["data"], "index": split["index"][:, :n].contiguous()}

    def split_nbytes(self, split) -> int:
        return int(split["data"].numel() + split["index"].numel() * 8)


# ----------------------------------------------------------------------------- ownership
def owner_of(p, world, nparts):
    """The rank that reduces and writes partition ``p`` of ``nparts``."""
    return p * world // nparts


def owned(rank, world, nparts):
    """The half-open range of partitions ``rank`` owns: consecutive ones,
    (0, 0) for a rank that owns none."""
    ps = [p for p in range(nparts) if owner_of(p, world, nparts) == rank]
    return (ps[0], ps[-1] + 1) if ps else (0, 0)


#: a tensor of a map output (a dict) and the key of its per-partition counts;
#: dtype and trailing shape are those of the tensor (for a tracker without maps)
Field = collections.namedtuple("Field", "tensor counts dtype shape", defaults=((),))


def by_destination(outputs, world, nparts, fields, device):
    """A tracker's map outputs regrouped by destination rank: each output is
    ordered by partition and a rank owns consecutive partitions, so a
    destination's share of an output is one slice.  Per field: (the slices
    back to back in (rank, output) order on ``device``, the count per rank)."""
    import torch
    ranges = [owned(j, world, nparts) for j in range(world)]
    regrouped = []
    for f in fields:
        pieces, send = [], []
        for pa, pb in ranges:
            n = 0
            for o in outputs:
                assert o[f.tensor].dtype == f.dtype and tuple(o[f.tensor].shape[1:]) == f.shape
                a, b = sum(o[f.counts][:pa]), sum(o[f.counts][:pb])
                pieces.append(o[f.tensor][a:b].to(device))
                n += b - a
            send.append(n)
        regrouped.append((torch.cat(pieces) if pieces else
                          torch.empty((0, *f.shape), dtype=f.dtype, device=device), send))
    return regrouped


# ----------------------------------------------------------------------------- word tables
def cat_tables(outputs, device):
    """The (blob, counts) tables of a tracker's map outputs back to back on
    ``device``."""
    import torch
    blobs = [b.to(device) for b, _ in outputs]
    counts = [c.to(device) for _, c in outputs]
    return (torch.cat(blobs) if blobs else torch.empty(0, dtype=torch.uint8, device=device),
            torch.cat(counts) if counts else torch.empty(0, dtype=torch.int64, device=device))


def shuffle_tables(ctx, blob, counts, part_bytes, part_words):
    """The word tables' shuffle: two static-shape all-to-alls (bytes, then
    counts) whose slot sizes every rank agrees on through a HOST all-reduce
    of the largest per-destination sizes (the sizes are host values
    already: merge_tables returns them), so no collective here waits for
    the device; the one host read is the compaction after both exchanges
    are enqueued.  An overflowing slot (impossible with exact maxima, kept
    as a guard) sends every rank to all_to_all_v (an all-reduced flag)."""
    import torch

    from ..parallel.collectives import compact_static
    comm = ctx.comm
    W = comm.world_size
    if W <= 1 or not hasattr(comm, "all_to_all_v_static"):
        return comm.all_to_all_v(blob, part_bytes)[0], comm.all_to_all_v(counts, part_words)[0]
    mx = torch.tensor([max(part_bytes or [0]), max(part_words or [0])], dtype=torch.int64)
    mx = comm.all_reduce_max(mx) if hasattr(comm, "all_reduce_max") else mx
    cap_b, cap_w = max(1, int(mx[0])), max(1, int(mx[1]))
    rb, rcb = comm.all_to_all_v_static(blob, part_bytes, cap_b)
    rc, rcw = comm.all_to_all_v_static(counts, part_words, cap_w)
    got_b = compact_static(rb, rcb, cap_b)
    got_w = compact_static(rc, rcw, cap_w)
    # the fallback is a collective: every rank must take it or none (one
    # rank entering all_to_all_v alone would hang the gang), so the
    # overflow flags are all-reduced first
    over = torch.tensor([int(got_b is None or got_w is None)], dtype=torch.int64)
    if hasattr(comm, "all_reduce_max"):
        over = comm.all_reduce_max(over)
    if int(over[0]):
        return comm.all_to_all_v(blob, part_bytes)[0], comm.all_to_all_v(counts, part_words)[0]
    return got_b[0], got_w[0]


# ----------------------------------------------------------------------------- eligibility
def text_input_reason(inputs):
    """None if the text loader reads these inputs (local files, no codec but
    Snappy), else the reason it does not."""
    for f in records.input_files(inputs):
        if not os.path.isfile(f):
            return f"input {f} is not a local file"
        why = compressed_input_reason(f)
        if why is not None:
            return why
    return None


def text_output_reason(base):
    """None if the device formats this job's text parts (uncompressed,
    ``key\\tvalue`` lines), else the reason it does not."""
    if base is not None and base.get_boolean("mapred.output.compress", False):
        return "compressed output"
    if base is not None and base.get(SEPARATOR_KEY, "\t") != "\t":
        return f"{SEPARATOR_KEY} is not a tab"
    return None


def local_output_reason(out, base):
    """None if a map may write its part into ``out`` itself (a local
    directory, uncompressed output), else the reason it may not."""
    if base is not None and base.get_boolean("mapred.output.compress", False):
        return "compressed output"
    if "://" in str(out) and not str(out).startswith("file://"):
        return f"output directory {out} is not a local one"
    return None


# ----------------------------------------------------------------------------- builders
def file_job(base, name, split_class, inputs=None, output=None, maps=None) -> JobConf:
    """The JobConf of the split-level job ``split_class`` (``module:Class``)
    over ``base``: its name, its input paths and output directory where it has
    them, ``maps`` map tasks if given."""
    job = JobConf(base)
    job.set_job_name(name)
    job.set("hbmr.splitjob.class", split_class)
    if inputs is not None:
        FileInputFormat.setInputPaths(job, *([inputs] if isinstance(inputs, str) else inputs))
    if output is not None:
        FileOutputFormat.setOutputPath(job, output)
    if maps:
        job.set_num_map_tasks(maps)
    return job
