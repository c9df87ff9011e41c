"""The word-count family as split-level jobs with a device reduce: ``wordcount``,
``multifilewc``, ``aggregatewordcount`` and ``aggregatewordhist``.

The four classic jobs are one job with a different input format, key prefix or
final aggregator: tokenise, sum per word, partition by the hash of the shuffle
key, sort each partition by key and write ``word\\tcount`` lines.  Here the map
is GPU WordCount's (native/kernels/text.hip: tokenise and aggregate a split in
HBM); :class:`WordTableSplitJob` differs from ``WordCountSplitJob`` after it:

* there are ``R = mapred.reduce.tasks`` parts, and partition ``p`` belongs to
  rank ``p*W//R`` as in GPU Sort;
* ``combine`` sums the tracker's tables, partitions the words with the job's
  hash seed (native/kernels/wordtab.hip: seed 1 for ``Text(word)``, the hash of
  ``LongValueSum:`` for the aggregate framework's key, without building it) and
  groups them by owning rank for the all-to-all-v;
* ``reduce`` merges what it received, sorts by (partition, word) on the device
  (hbmr/ops/recsort.py), formats each owned partition on the device and makes
  one device-to-host copy per part.

``aggregatewordhist`` shuffles the words for balance only, sorts and
run-lengths each rank's counts, sends the runs to the owner of the partition
of ``ValueHistogram:WORD_HISTOGRAM`` and writes the one report line there.

The mappers of the last three programs tokenise with ``str(value).split()``,
the device with ``bytes.split()``.  The two agree unless a split holds a byte
>= 0x80 or in 0x1c-0x1f; such a split is counted on the host by the classic
mapper's own expression and adds 1 to ``WORDTABLE_CPU_FALLBACK_SPLITS``.
"""
from __future__ import annotations

import collections

from ..gpu.splitjob import SplitJob, SplitSpec
from ..io.writable import hash_bytes
from ..mapred import JobConf
from . import records, splits

PROGRAM_KEY = "hbmr.wordtable.program"
WORDTABLE_GROUP = "hbmr.WordTableCounters"
WORDTABLE_CPU_FALLBACK_SPLITS = "WORDTABLE_CPU_FALLBACK_SPLITS"
HISTOGRAM_ID = b"WORD_HISTOGRAM"
HISTOGRAM_KEY = b"ValueHistogram:" + HISTOGRAM_ID

# program -> (job name, the shuffle key's prefix, whether the classic mapper
# tokenises the decoded text)
PROGRAMS = {
    "wordcount": ("wordcount-gpu", b"", False),
    "multifilewc": ("MultiFileWordCount-gpu", b"", True),
    "aggregatewordcount": ("ValueAggregatorJob-gpu", b"LongValueSum:", True),
    "aggregatewordhist": ("ValueAggregatorJob-gpu", b"", True),
}


def classic_words(raw: bytes):
    """The words TokenCountMapper and the aggregate plug-ins emit for the lines
    of ``raw``: ``str(Text(line)).split()``, each as ``Text(word)``'s bytes."""
    c = collections.Counter()
    for line in raw.split(b"\n"):
        c.update(w.encode("utf-8") for w in line.decode("utf-8", errors="replace").split())
    return c


def read_files(paths) -> bytes:
    """The lines of whole files back to back: a file that does not end in a
    newline gets one, an empty file contributes nothing."""
    from ..fs import strip_scheme
    out = []
    for p in paths:
        with open(strip_scheme(p), "rb") as f:
            data = f.read()
        if data:
            out.append(data if data.endswith(b"\n") else data + b"\n")
    return b"".join(out)


class WordTableSplitJob(splits.BothSlots, splits.FinishesOutput, splits.TextSplits, SplitJob):
    collective_reduce = True
    needs_reduce = True

    def configure(self, conf):
        self.conf = conf
        self.out = conf.get("mapred.output.dir")
        self.nparts = max(1, conf.get_num_reduce_tasks())
        self.program = conf.get(PROGRAM_KEY, "wordcount")
        if self.program not in PROGRAMS:
            raise ValueError(f"{PROGRAM_KEY}: unknown program {self.program!r}")
        _, prefix, self.decoded = PROGRAMS[self.program]
        self.seed = hash_bytes(prefix) & 0xFFFFFFFF
        self.histogram = self.program == "aggregatewordhist"

    # -- input ------------------------------------------------------------------------
    def get_splits(self, conf, trackers):
        if conf.get(PROGRAM_KEY, "wordcount") != "multifilewc":
            return super().get_splits(conf, trackers)
        from ..mapred.lib.combine import MultiFileInputFormat
        found = MultiFileInputFormat().getSplits(JobConf(conf), max(1, conf.get_num_map_tasks()))
        out = []
        for i, s in enumerate(found):
            paths = [str(p) for p in s.paths]
            key = "mfwc:" + "|".join(f"{p}:{n}" for p, n in zip(paths, s.lengths))
            out.append(SplitSpec(i, key, "file", {"paths": paths},
                                 splits.place(i, len(found), trackers),
                                 sum(int(n) for n in s.lengths)))
        return out

    def load_split(self, spec: SplitSpec, device):
        if "paths" not in spec.params:
            return super().load_split(spec, device)
        import torch
        paths = spec.params["paths"]
        if any(splits.is_snappy(p) for p in paths):
            return self._load_files_decoded(spec, device)
        data = read_files(paths)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else \
            torch.empty(0, dtype=torch.uint8)
        return t if str(device) == "cpu" else t.to(device)

    def _load_files_decoded(self, spec, device):
        """:func:`read_files` where some files are ``.snappy``: those are decoded
        on ``device``, the plain ones copied there, and the join rule is the
        same — a newline after any file that lacks one (one host read of the
        files' last bytes for the split)."""
        import torch
        dev = torch.device(device)
        pieces = []
        for p in spec.params["paths"]:
            if splits.is_snappy(p):
                t = splits.load_text_file(self, spec.key, p, device)
            else:
                raw = read_files([p])
                t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev) if raw else None
            if t is not None and t.numel():
                pieces.append(t)
        if not pieces:
            return torch.empty(0, dtype=torch.uint8, device=dev)
        last = torch.stack([t[-1] for t in pieces]).tolist()
        newline = torch.tensor([10], dtype=torch.uint8, device=dev)
        out = []
        for t, b in zip(pieces, last):
            out.append(t)
            if b != 10:
                out.append(newline)
        return torch.cat(out) if len(out) > 1 else out[0]

    # -- map --------------------------------------------------------------------------
    def _map(self, ctx, data):
        """The same on both kinds of slot: the flag has one definition."""
        from ..mapred import counters as C
        from ..ops import text, wordtab
        ctx.reporter.incrCounter(C.TASK_GROUP, C.MAP_INPUT_BYTES, int(data.numel()))
        splits.count_snappy_decoded(self, ctx)
        if self.decoded and wordtab.flag_nonclassic(data):
            ctx.reporter.incrCounter(WORDTABLE_GROUP, WORDTABLE_CPU_FALLBACK_SPLITS, 1)
            blob, counts = text._table_from(classic_words(bytes(data.cpu().numpy())))
            return blob.to(data.device), counts.to(data.device)
        return text.count_words(data, getattr(ctx, "stream", None))

    # -- shuffle + reduce -------------------------------------------------------------
    def _dest(self, parts, world):
        """The rank each word travels to: the owner of its partition (words of
        the histogram job: the partition itself, one per rank)."""
        if self.histogram:
            return parts
        return parts * world // self.nparts

    def combine(self, ctx, outputs):
        """The tracker's tables summed, the words grouped by destination rank:
        (blob, counts, bytes per rank, words per rank)."""
        import torch
        from ..ops import text, wordtab
        W = max(1, ctx.world_size)
        buf, us, ul, uc = merge_table(*splits.cat_tables(outputs, splits.device_of(ctx)))
        parts = wordtab.partition(buf, us, ul, W if self.histogram else self.nparts,
                                  1 if self.histogram else self.seed)
        dest = self._dest(parts.to(torch.int64), W)
        order = torch.argsort(dest, stable=True)
        dest_o = dest[order]
        send_words = torch.bincount(dest_o, minlength=W)
        send_bytes = torch.bincount(dest_o, weights=ul[order].to(torch.float64) + 1,
                                    minlength=W).to(torch.int64)
        return (pack_words(buf, us, ul, order), uc[order].contiguous(), send_bytes.tolist(),
                send_words.tolist())

    def reduce(self, ctx, combined):
        from ..mapred import counters as C
        from ..ops import wordtab
        blob, counts, send_bytes, send_words = combined
        W = max(1, ctx.world_size)
        rblob, rcounts = splits.shuffle_tables(ctx, blob, counts, send_bytes, send_words)
        buf, us, ul, uc = merge_table(rblob, rcounts)
        n = int(us.numel())
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_INPUT_GROUPS, n)
        if self.histogram:
            return self._reduce_histogram(ctx, uc, W)
        parts = wordtab.partition(buf, us, ul, self.nparts, self.seed)
        order, nrec = wordtab.sort_table(buf, us, ul, parts, self.nparts)
        pa, pb = splits.owned(ctx.rank, W, self.nparts)
        if sum(nrec) != sum(nrec[pa:pb]):
            raise RuntimeError("words of a partition this rank does not own arrived here")
        r0 = 0
        for p in range(self.nparts):
            if pa <= p < pb and self.out:
                text = wordtab.format_part(buf, us, ul, uc, order[r0:r0 + nrec[p]].contiguous())
                with records.part_writer(self.out, f"part-{p:05d}") as f:
                    f.write(text.cpu().numpy().tobytes())       # the part's one copy to the host
            r0 += nrec[p]
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_OUTPUT_RECORDS, n)
        return {"distinct": n, "words": int(uc.sum()) if n else 0, "parts": pb - pa}

    def _reduce_histogram(self, ctx, counts, world):
        import torch
        from ..mapred import counters as C
        from ..ops import wordtab
        values, mult = wordtab.count_runs(wordtab.sort_counts(counts))
        target = (hash_bytes(HISTOGRAM_KEY) & 0x7FFFFFFF) % self.nparts
        owner = splits.owner_of(target, world, self.nparts)
        runs = torch.stack([values, mult], dim=1).contiguous()
        send = [int(runs.shape[0]) if j == owner else 0 for j in range(world)]
        got = ctx.comm.all_to_all_v(runs, send)[0]
        pa, pb = splits.owned(ctx.rank, world, self.nparts)
        written = 0
        for p in range(pa, pb):
            line = b""
            if p == target and got.shape[0]:
                report = wordtab.histogram_report(got[:, 0], got[:, 1])
                line = HISTOGRAM_ID + b"\t" + report.encode() + b"\n"
                written = 1
            if self.out:
                with records.part_writer(self.out, f"part-{p:05d}") as f:
                    f.write(line)
        ctx.reporter.incrCounter(C.TASK_GROUP, C.REDUCE_OUTPUT_RECORDS, written)
        return {"distinct": int(counts.numel()), "parts": pb - pa}


def merge_table(blob, counts):
    """A concatenation of ``b"word\\n"`` tables summed per word: (buf, starts
    int32, lens int32, counts int64), the words unordered."""
    import torch
    from ..ops import text
    if blob.device.type != "cuda":
        c = collections.Counter()
        for w, n in text.parse_table(bytes(blob.numpy()), counts):
            c[w] += int(n)
        words = list(c)
        lens = [len(w) for w in words]
        starts = [0] * len(words)
        for i in range(1, len(words)):
            starts[i] = starts[i - 1] + lens[i - 1] + 1
        raw = b"".join(w + b"\n" for w in words)
        return (torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else
                torch.empty(0, dtype=torch.uint8),
                torch.tensor(starts, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32),
                torch.tensor([c[w] for w in words], dtype=torch.int64))
    buf = text._aligned(blob.contiguous())
    starts, lens = text.tokenize(buf)
    if starts.numel() != counts.numel():
        raise ValueError(f"word table mismatch: {starts.numel()} words, {counts.numel()} counts")
    us, ul, uc, _ = text.aggregate(buf, starts, lens, counts.contiguous(), 1)
    return buf, us.contiguous(), ul.contiguous(), uc.contiguous()


def pack_words(buf, starts, lens, order):
    """The ``b"word\\n"`` blob of the words ``order`` (int64 ids)."""
    import torch
    from ..ops import text
    if buf.device.type == "cuda":
        return text.pack(buf, starts, lens, order)
    raw = buf.numpy().tobytes()
    s, n = starts.tolist(), lens.tolist()
    out = b"".join(raw[s[i]:s[i] + n[i]] + b"\n" for i in order.tolist())
    return torch.frombuffer(bytearray(out), dtype=torch.uint8) if out else \
        torch.empty(0, dtype=torch.uint8)


# ----------------------------------------------------------------------------- builders
def why_ineligible(inputs, reduces, base=None):
    """None if the word-table job takes this job, else the reason it does not."""
    if reduces < 1:
        return f"{reduces} reduces: the map output itself is the job's output"
    return splits.text_output_reason(base) or splits.text_input_reason(inputs)


def gpu_job(program, inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    """``program`` (a key of PROGRAMS) as a split-level job (GPU map slots, CPU
    slots per the hybrid cost model).  Raises ValueError, with the reason, for
    anything not eligible: no reduces, an input that is not a local file or
    carries the extension of a compression codec other than Snappy, compressed output, an output
    separator other than tab."""
    if program not in PROGRAMS:
        raise KeyError(program)
    why = why_ineligible(inputs, reduces, base)
    if why is not None:
        raise ValueError(f"{program} of {inputs!r} is not eligible for the GPU: {why}")
    job = splits.file_job(base, PROGRAMS[program][0], "hbmr.models.wordtable:WordTableSplitJob",
                          inputs, output, maps)
    job.set(PROGRAM_KEY, program)
    job.set_num_reduce_tasks(reduces)
    return job


def wordcount_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    return gpu_job("wordcount", inputs, output, reduces, base, maps)


def multifilewc_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    return gpu_job("multifilewc", inputs, output, reduces, base, maps)


def aggregatewordcount_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    return gpu_job("aggregatewordcount", inputs, output, reduces, base, maps)


def aggregatewordhist_job(inputs, output, reduces=1, base=None, maps=None) -> JobConf:
    return gpu_job("aggregatewordhist", inputs, output, reduces, base, maps)
