"""Snappy RECORD- and BLOCK-compressed SequenceFile splits as the
``(data uint8[bytes], index int64[4, n])`` of an uncompressed split
(:func:`hbmr.ops.recsort.index_records`), built in device memory: the host
plans from the headers alone (native/io/seqzindex.cc), the Snappy streams are
decoded by the kernel of :mod:`hbmr.ops.snappydec`, and native/kernels/
seqblock.hip turns what they hold into frames.

``data`` holds the frames of the split's records in record order, back to back
and without sync escapes; a frame is ``>ii(len(k) + len(v), len(k)) + k + v``
of the raw key and the decompressed value.

* :func:`plan` — the byte range to load, the chunk table and, RECORD: the
  whole record index, BLOCK: the block table.  ``IOError`` naming the file (and
  the block) on any framing error.
* :func:`load_split` — on a GPU one H2D copy of the tables and the file range,
  one decode launch over all chunks, the seqblock kernels, one status read; on
  ``cpu`` the twin from ``sequencefile.Reader`` records.
* :func:`decode_lengths`, :func:`build_index`, :func:`assemble` — the kernels
  one at a time over a caller's own buffers.

On a GPU the native library must load (no silent fallback).
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import torch

from . import _lib, recsort, snappydec

RECORD, BLOCK = 1, 2
SNAPPY = "org.apache.hadoop.io.compress.SnappyCodec"
# status bits of a block (seqblock.hip)
MID_VINT, COUNT, RANGE, SUM, KEY_PREFIX = 1, 2, 4, 8, 16
_STATUS = {MID_VINT: "a length column ends inside a vint",
           COUNT: "the length columns do not hold the block's record count",
           RANGE: "a length negative or above 2^31 - 1",
           SUM: "the lengths do not add up to the keys or values column",
           KEY_PREFIX: "a key's length prefix contradicts its length"}


def status_text(code):
    """What the bits of a block's status say."""
    return "; ".join(t for bit, t in _STATUS.items() if code & bit) or f"status {code}"

_ptr = _lib.ptr
_INDEX = None


def _index_fn():
    global _INDEX
    if _INDEX is None:
        L = ctypes.CDLL(recsort._CPU_PATH)
        P, L64 = ctypes.c_void_p, ctypes.c_long
        L.hbmr_seqz_index.argtypes = [ctypes.c_char_p, L64, ctypes.c_char_p, ctypes.c_int,
                                      ctypes.c_int, L64, L64, P, P, L64, P, L64, P, L64]
        L.hbmr_seqz_index.restype = L64
        L.hbmr_seqz_last_error.restype = ctypes.c_char_p
        _INDEX = L
    return _INDEX


def is_snappy_file(reader) -> bool:
    """Whether an open ``sequencefile.Reader`` is over a RECORD- or
    BLOCK-compressed file of SnappyCodec."""
    return reader.decompress and getattr(reader.codec, "JAVA_NAME", None) == SNAPPY


def file_header(path):
    """(mode, prefix, header end, sync) of a Snappy-compressed SequenceFile, None
    for any other SequenceFile: the one look at the file's header a load needs."""
    from ..fs import strip_scheme
    from ..io import sequencefile as seqf
    with seqf.Reader(strip_scheme(str(path))) as r:
        if not is_snappy_file(r):
            return None
        if r.key_class_name not in recsort.KEY_CLASSES:
            raise ValueError(f"{path}: key class {r.key_class_name}")
        prefix = 4 if r.key_class_name == recsort.KEY_CLASSES[0] else 0
        return (BLOCK if r.block_compressed else RECORD), prefix, r.header_end, r.sync


def _header(path, header=None):
    header = header or file_header(path)
    if header is None:
        raise ValueError(f"{path}: not a Snappy-compressed SequenceFile")
    return header


def plan(path, start, length, header=None):
    """The plan of the split ``(path, start, length)``: a dict of ``mode``
    (RECORD / BLOCK), ``prefix`` (4: BytesWritable keys, 0: Text), ``lo`` and
    ``hi`` (the file range to load), ``n`` records, ``chunks`` (int64[4, c], the
    decode kernel's table with sources relative to ``lo``), ``data_bytes`` and
    RECORD: ``recs`` (int64[7, n]: the four index rows, then the key's offset
    in the range, its length and the value's uncompressed length; a value's
    chunks decode to ``foff + 8 + klen``), BLOCK: ``blocks`` (int64[10, b]: the
    record count, the record base, the offset and length of the four columns in
    a columns buffer of ``cols_bytes`` that the chunks decode into).
    ``header``: the file's :func:`file_header`, if the caller has it."""
    from ..fs import strip_scheme
    p = strip_scheme(str(path))
    mode, prefix, header_end, sync = _header(p, header)
    L = _index_fn()
    dims = np.zeros(7, dtype=np.int64)

    def call(chunks, recs, blocks):
        rc = L.hbmr_seqz_index(
            p.encode(), header_end, sync, mode, prefix, start, length, dims.ctypes.data,
            *(w for t in (chunks, recs, blocks)
              for w in ((None, 0) if t is None else (t.ctypes.data, t.shape[1]))))
        if rc != 0:
            raise IOError(L.hbmr_seqz_last_error().decode(errors="replace"))
        return dims.copy()

    first = call(None, None, None)
    n, c, nb = int(first[2]), int(first[3]), int(first[4])
    chunks = np.zeros((4, c), dtype=np.int64)
    recs = np.zeros((7, n), dtype=np.int64) if mode == RECORD else None
    blocks = np.zeros((10, nb), dtype=np.int64) if mode == BLOCK else None
    if not np.array_equal(call(chunks, recs, blocks), first):
        raise IOError(f"{path}: file changed while it was read")
    return {"path": str(path), "file": p, "mode": mode, "prefix": prefix, "lo": int(first[0]),
            "hi": int(first[1]), "n": n, "chunks": chunks, "recs": recs, "blocks": blocks,
            "data_bytes": int(first[5]), "cols_bytes": int(first[6])}


# --------------------------------------------------------------------------- the twin
def _payload(kb, prefix):
    """(offset, length) of the key payload in the serialized key ``kb``."""
    from ..io.vint import decode_vint
    if prefix:
        if len(kb) < 4 or struct.unpack(">i", kb[:4])[0] != len(kb) - 4:
            raise IOError("corrupt BytesWritable key")
        return 4, len(kb) - 4
    try:
        plen, poff = decode_vint(kb, 0)
    except Exception:
        raise IOError("corrupt Text key") from None
    if plen < 0 or poff + plen != len(kb):
        raise IOError("corrupt Text key")
    return poff, plen


def pack_records(recs, prefix):
    """(data, index) host tensors of the (key, value) byte pairs ``recs``."""
    out = bytearray()
    index = np.zeros((4, len(recs)), dtype=np.int64)
    for i, (kb, vb) in enumerate(recs):
        poff, plen = _payload(kb, prefix)
        index[:, i] = (len(out), 8 + len(kb) + len(vb), len(out) + 8 + poff, plen)
        out += struct.pack(">ii", len(kb) + len(vb), len(kb)) + kb + vb
    data = torch.frombuffer(out, dtype=torch.uint8) if out else torch.empty(0, dtype=torch.uint8)
    return data, torch.from_numpy(index)


def load_split_cpu(path, start, length, header=None):
    """The twin: the same (data, index) from ``sequencefile.Reader`` records."""
    from ..mapred.formats import FileSplit, SequenceFileRecordReader
    _, prefix, _, _ = _header(path, header)
    name = str(path)
    rr = SequenceFileRecordReader(None, FileSplit(name, start, length))
    recs = []
    try:
        while True:
            raw = rr.next_raw()
            if raw is None:
                break
            recs.append(raw)
        return pack_records(recs, prefix)
    except IOError as e:
        raise IOError(e if name in str(e) else f"{name}: {e}") from None
    except Exception as e:
        raise IOError(f"{name}: malformed compressed SequenceFile ({e})") from None
    finally:
        rr.close()


# --------------------------------------------------------------------------- kernels
def _check_blocks(blocks, cols_bytes, n):
    """The block table's ranges lie inside the columns buffer and its records
    are consecutive (the kernels trust the table)."""
    if blocks.dtype != torch.int64 or blocks.dim() != 2 or blocks.shape[0] != 10 or \
            blocks.device.type != "cpu":
        raise ValueError("blocks: host int64[10, b] required")
    t = blocks.numpy()
    if t.shape[1] == 0:
        if n:
            raise ValueError("blocks: records without a block")
        return
    base = np.concatenate([[0], np.cumsum(t[0])])
    if t.min() < 0 or t[0].max() >= 1 << 31 or not np.array_equal(t[1], base[:-1]) or \
            base[-1] != n or (t[2::2] + t[3::2]).max() > cols_bytes:
        raise ValueError("blocks: a block lies outside the columns buffer or its record slots")


def decode_lengths(cols, blocks, n, stream=None, _blocks_dev=None, status=None, klen=None,
                   vlen=None):
    """(klen int64[n], vlen int64[n], status int32[b]) on cols' device: the
    vint kernel over the length columns of ``blocks`` (host int64[10, b]) in
    ``cols``.  A block with a nonzero status has unspecified lengths in its own
    slots; no other slot is written (``klen`` / ``vlen``: the caller's own
    int64 buffers of at least n slots).  The table is validated here unless the
    caller hands over its device copy, which says it has done so."""
    nb = int(blocks.shape[1]) if blocks.dim() == 2 else -1
    if cols.dtype != torch.uint8 or cols.dim() != 1 or not cols.is_contiguous() or \
            cols.device.type != "cuda":
        raise ValueError("cols: contiguous uint8[bytes] on a GPU required")
    if _blocks_dev is None:
        _check_blocks(blocks, int(cols.numel()), n)
    with _lib.stream_ctx(stream):
        outs = []
        for t in (klen, vlen):
            if t is None:
                t = torch.empty(n, dtype=torch.int64, device=cols.device)
            elif t.dtype != torch.int64 or t.numel() < n or not t.is_contiguous() or \
                    t.device != cols.device:
                raise ValueError("klen, vlen: contiguous int64[>= n] on cols' device required")
            outs.append(t)
        klen, vlen = outs
        if status is None:
            status = torch.empty(nb, dtype=torch.int32, device=cols.device)
        if nb:
            bdev = _blocks_dev if _blocks_dev is not None else \
                blocks.contiguous().to(cols.device, non_blocking=True)
            rc = _lib.load().hbmr_seqblock_vint(_ptr(cols), _ptr(bdev), nb, _ptr(klen), _ptr(vlen),
                                                _ptr(status), _lib.stream_handle(stream))
            _lib.check(rc, "hbmr_seqblock_vint")
    return klen, vlen, status


def build_index(cols, bdev, klen, vlen, status, prefix, stream=None):
    """(index int64[4, n], ksrc, vsrc, klen, vlen) from the decoded lengths:
    the lengths of a block whose status is nonzero count as 0, frame offsets are
    a global exclusive scan of ``8 + klen + vlen``, key and value sources
    exclusive scans inside each block's columns; the key payload comes from the
    key's first bytes, and a prefix that contradicts ``klen`` sets the block's
    status.  Device work only."""
    n = int(klen.numel())
    nb = int(bdev.shape[1])
    with _lib.stream_ctx(stream):
        rec_block = torch.repeat_interleave(torch.arange(nb, device=cols.device), bdev[0],
                                            output_size=n)
        ok = status[rec_block] == 0
        klen, vlen = torch.where(ok, klen, 0), torch.where(ok, vlen, 0)
        flen = klen + vlen + 8
        foff = torch.cumsum(flen, 0) - flen
        first = bdev[1][rec_block]
        ck, cv = torch.cumsum(klen, 0) - klen, torch.cumsum(vlen, 0) - vlen
        ksrc = (ck - ck[first] + bdev[4][rec_block]).contiguous()
        vsrc = (cv - cv[first] + bdev[8][rec_block]).contiguous()
        index = torch.empty((4, n), dtype=torch.int64, device=cols.device)
        rc = _lib.load().hbmr_seqblock_index(
            _ptr(cols), int(cols.numel()), _ptr(foff), _ptr(klen), _ptr(vlen), _ptr(ksrc),
            _ptr(rec_block), n, prefix, _ptr(index), _ptr(status), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_seqblock_index")
    return index, ksrc, vsrc, klen, vlen


def assemble(out, foff, klen, vlen, keys, ksrc, vals=None, vsrc=None, stream=None):
    """Write into ``out`` (uint8, device) at ``foff[r]`` the frame header of
    record r, its key ``keys[ksrc[r] : + klen[r]]`` and its value
    ``vals[vsrc[r] : + vlen[r]]``; without ``vals`` header and key only (the
    value's place in the frame is left as it is).  A record whose frame or
    sources do not lie inside their buffers is left out; no other byte of
    ``out`` is written."""
    n = int(foff.numel())
    for t in (foff, klen, vlen, ksrc) + (() if vals is None else (vsrc,)):
        if t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() or \
                t.device != out.device:
            raise ValueError("assemble: contiguous int64[n] on out's device required")
    for t in (out, keys) + (() if vals is None else (vals,)):
        if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or \
                t.device != out.device or t.device.type != "cuda":
            raise ValueError("assemble: contiguous uint8[bytes] on one GPU required")
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        if vals is None:
            rc = lib.hbmr_seqblock_heads(_ptr(keys), int(keys.numel()), _ptr(ksrc), _ptr(foff),
                                         _ptr(klen), _ptr(vlen), n, _ptr(out), int(out.numel()),
                                         _lib.stream_handle(stream))
            _lib.check(rc, "hbmr_seqblock_heads")
        else:
            rc = lib.hbmr_seqblock_assemble(_ptr(keys), int(keys.numel()), _ptr(ksrc), _ptr(vals),
                                            int(vals.numel()), _ptr(vsrc), _ptr(foff), _ptr(klen),
                                            _ptr(vlen), n, _ptr(out), int(out.numel()),
                                            _lib.stream_handle(stream))
            _lib.check(rc, "hbmr_seqblock_assemble")
    return out


# --------------------------------------------------------------------------- the loader
def _words(*arrays):
    """The int64 arrays back to back as bytes, and each one's (offset, shape)."""
    parts, where, at = [], [], 0
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.int64)
        where.append((at, a.shape))
        parts.append(a.reshape(-1).view(np.uint8))
        at += a.nbytes
    return parts, where, at


def load_split(path, start, length, device, stream=None, stages=None, header=None):
    """(data, index) of the split on ``device``.  ``IOError`` naming the file on
    bad framing, and on a GPU the first chunk whose stream is malformed or the
    first block whose columns contradict themselves.  ``stages``: a list that
    receives (name, start event, end event) per device stage; ``header``: the
    file's :func:`file_header`, if the caller has it."""
    if str(device) == "cpu":
        return load_split_cpu(path, start, length, header)
    pl = plan(path, start, length, header)
    device = torch.device(device)
    n, c = pl["n"], int(pl["chunks"].shape[1])
    name = pl["path"]
    if n == 0:
        return (torch.empty(0, dtype=torch.uint8, device=device),
                torch.empty((4, 0), dtype=torch.int64, device=device))
    record = pl["mode"] == RECORD
    table = pl["recs"] if record else pl["blocks"]
    nb = 0 if record else int(table.shape[1])
    nbytes = pl["hi"] - pl["lo"]
    # one host buffer, one copy: the tables, then the file range read in place
    parts, where, tbytes = _words(pl["chunks"], table)
    host = torch.empty(tbytes + nbytes, dtype=torch.uint8)
    h = host.numpy()
    at = 0
    for part in parts:
        h[at:at + part.size] = part
        at += part.size
    with open(pl["file"], "rb", buffering=0) as f:
        f.seek(pl["lo"])
        got, view = 0, memoryview(h[tbytes:])
        while got < nbytes:
            k = f.readinto(view[got:])
            if not k:
                raise IOError(f"{name}: short read")
            got += k
    target = pl["data_bytes"] if record else pl["cols_bytes"]
    snappydec._check_table(host[tbytes:], torch.from_numpy(pl["chunks"]), target)
    if record:
        r = pl["recs"]
        if (r[4:].min() < 0 or (r[4] + r[5]).max() > nbytes or
                (r[0] + r[1]).max() > pl["data_bytes"]):
            raise ValueError(f"{name}: a record lies outside the loaded range or the output")
    else:
        _check_blocks(torch.from_numpy(table), pl["cols_bytes"], n)

    def mark(what, fn):
        if stages is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        stages.append((what, a, b))
        return out

    with _lib.stream_ctx(stream):
        dev = host.to(device)
        cdev = dev[where[0][0]:where[1][0]].view(torch.int64)
        tdev = dev[where[1][0]:tbytes].view(torch.int64).view(table.shape)
        src = dev[tbytes:]
        status = torch.zeros(c + nb, dtype=torch.int32, device=device)
        lib = _lib.load()

        def decode(out):
            if c:
                rc = lib.hbmr_snappy_decode(_ptr(src), _ptr(cdev), c, _ptr(out), _ptr(status),
                                            _lib.stream_handle(stream))
                _lib.check(rc, "hbmr_snappy_decode")

        data = torch.empty(pl["data_bytes"], dtype=torch.uint8, device=device)
        if record:
            mark("decode", lambda: decode(data))
            mark("assemble", lambda: assemble(data, tdev[0], tdev[5], tdev[6], src, tdev[4],
                                              stream=stream))
            index = tdev[:4].clone()
        else:
            cols = torch.empty(pl["cols_bytes"], dtype=torch.uint8, device=device)
            mark("decode", lambda: decode(cols))
            bstat = status[c:]
            klen, vlen, _ = mark("vint", lambda: decode_lengths(
                cols, torch.from_numpy(table), n, stream, _blocks_dev=tdev, status=bstat))
            index, ksrc, vsrc, klen, vlen = mark("index", lambda: build_index(
                cols, tdev, klen, vlen, bstat, pl["prefix"], stream))
            mark("assemble", lambda: assemble(data, index[0], klen, vlen, cols, ksrc, cols, vsrc,
                                              stream))
            del cols
        st = status.cpu().numpy()          # the one host read
        del dev, src, cdev, tdev
    bad = np.flatnonzero(st)
    if bad.size:
        i = int(bad[0])
        if i < c:
            raise IOError(f"{name}: malformed snappy stream in chunk {i} of {c} "
                          f"(decoder code {int(st[i])})")
        raise IOError(f"{name}: block {i - c} of {nb}: {status_text(int(st[i]))}")
    return data, index
