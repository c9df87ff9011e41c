"""What the split-level jobs over files share: the input files and their
eligibility, a SequenceFile split in device memory, and output parts that
appear in the output directory only when complete."""
from __future__ import annotations

import contextlib
import os

DEFAULT_CLASS = "org.apache.hadoop.io.BytesWritable"


def input_files(inputs):
    """The files of a path or a list of paths: a directory gives its files in
    name order without the hidden ones (``_SUCCESS``, ``.crc``)."""
    paths = [inputs] if isinstance(inputs, str) else list(inputs)
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in sorted(os.listdir(p))
                      if not f.startswith(("_", "."))]
        else:
            files.append(p)
    return files


def file_reason(f, seen=None):
    """None if the record kernels take the SequenceFile ``f`` (a local file,
    uncompressed or RECORD- / BLOCK-compressed with SnappyCodec, byte-string
    keys), else the reason they do not.  ``seen`` (a set) receives the (key
    class, value class) names of a file they take."""
    from ..io import sequencefile as seqf
    from ..ops import recsort, seqz
    if not os.path.isfile(f):
        return f"input {f} is not a local file"
    with seqf.Reader(f) as r:
        if r.compression != seqf.NONE and not seqz.is_snappy_file(r):
            return f"{r.compression}-compressed input {f}"
        if r.key_class_name not in recsort.KEY_CLASSES:
            return (f"key class {r.key_class_name} of {f} (byte-string keys only: "
                    "BytesWritable, Text)")
        if seen is not None:
            seen.add((r.key_class_name, r.value_class_name))
    return None


def first_classes(files):
    """(key class, value class) names of the first file; BytesWritable without one."""
    from ..io import sequencefile as seqf
    if not files:
        return DEFAULT_CLASS, DEFAULT_CLASS
    with seqf.Reader(files[0]) as r:
        return r.key_class_name, r.value_class_name


def is_snappy_compressed(path) -> bool:
    """Whether the SequenceFile ``path`` is RECORD- or BLOCK-compressed with
    SnappyCodec: the compressed files :func:`load_record_split` takes."""
    from ..ops import seqz
    return seqz.file_header(path) is not None


def load_split_flagged(path, start, length, device):
    """(data, index, compressed): :func:`load_record_split`, and whether the
    split was decompressed.  The file's header is looked at once, here."""
    import torch

    from ..ops import recsort, seqz
    header = seqz.file_header(path)
    if header is not None:
        return (*seqz.load_split(path, start, length, device, header=header), True)
    data, index = recsort.index_records(path, start, length)
    data, index = torch.from_numpy(data), torch.from_numpy(index)
    if str(device) != "cpu":
        data, index = data.to(device), index.to(device)
    return data, index, False


def load_record_split(path, start, length, device):
    """(data uint8[bytes], index int64[4, n]) of the records a
    SequenceFileRecordReader over (path, start, length) returns, as tensors on
    ``device``: of an uncompressed file the raw range and index of
    ``recsort.index_records``; of a Snappy RECORD- or BLOCK-compressed file the
    frames of the decompressed records back to back, decoded and assembled on
    the device (``hbmr.ops.seqz.load_split``)."""
    return load_split_flagged(path, start, length, device)[:2]


@contextlib.contextmanager
def part_writer(out, name, key_class=None, value_class=None):
    """Writes ``out/name`` under ``out/_temporary`` and moves it into place on a
    clean exit: a ``sequencefile.Writer`` of the two classes, or without a key
    class a binary file."""
    from ..io import sequencefile as seqf
    tmp = os.path.join(out, "_temporary")
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, name)
    with (open(path, "wb") if key_class is None else
          seqf.Writer(path, key_class, value_class)) as w:
        yield w
    os.replace(path, os.path.join(out, name))


def finish_output(out):
    """Drops ``out/_temporary`` and marks the output directory complete."""
    import shutil
    shutil.rmtree(os.path.join(out, "_temporary"), ignore_errors=True)
    open(os.path.join(out, "_SUCCESS"), "wb").close()
