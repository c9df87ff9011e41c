"""Snappy-compressed input on the device: the chunk table of a Hadoop-framed
Snappy file (native/io/snappyindex.cc) and the decode kernel over it
(native/kernels/snappydec.hip), with the host decoder
(:func:`hbmr.io.snappy.hadoop_decompress`, native/io/snappy.cc) as the twin.

A ``.snappy`` file is a sequence of blocks, each a run of independent raw
Snappy streams ("chunks") of at most ``buffersize - buffersize/6 - 32`` input
bytes.  :func:`chunk_table` lists them from the headers alone as an
``int64[4, n]`` table — per chunk the offset of the raw stream in the file, its
compressed length, the offset of its output and its uncompressed length —
and the kernel decodes one chunk per wave.

* :func:`decode_file` — the decompressed bytes of a file as a ``uint8`` tensor:
  on a GPU one H2D copy of the table and the file, one launch, one read of the
  status; on ``cpu`` the twin.  Both raise ``IOError`` naming the file.
* :func:`decode_chunks` — the kernel (or, for host tensors, the twin chunk by
  chunk) over a caller's own buffer and table.

On a GPU the native library must load (no silent fallback).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ..io import snappy
from . import _lib

_INDEX = None


def _index_fn():
    global _INDEX
    if _INDEX is None:
        f = ctypes.CDLL(snappy._PATH).hbmr_snappy_index
        f.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                      ctypes.POINTER(ctypes.c_long)]
        f.restype = ctypes.c_long
        _INDEX = f
    return _INDEX


def chunk_table(data, name="<bytes>"):
    """(table int64[4, n], total): the chunks of the framed stream ``data`` and
    the size of its output.  ``IOError`` naming ``name`` on bad framing: a
    truncated header, a chunk length <= 0 or past the end, chunk lengths that do
    not add up to their block's header, a preamble over ``22 n + 64``."""
    data = bytes(data)
    fn = _index_fn()
    total = ctypes.c_long(0)
    n = fn(data, len(data), None, 0, ctypes.byref(total))
    if n < 0:
        raise IOError(f"{name}: truncated or malformed snappy block stream")
    table = np.zeros((4, n), dtype=np.int64)
    if n and fn(data, len(data), table.ctypes.data, n, ctypes.byref(total)) != n:
        raise IOError(f"{name}: truncated or malformed snappy block stream")
    return torch.from_numpy(table), int(total.value)


def _check_table(src, table, out_bytes):
    """The table's ranges lie inside both buffers (the kernel trusts them)."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[0] != 4 or \
            table.device.type != "cpu":
        raise ValueError("table: host int64[4, n] required")
    if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous():
        raise ValueError("src: contiguous uint8[bytes] required")
    t = table.numpy()
    if t.shape[1] and (t.min() < 0 or (t[0] + t[1]).max() > src.numel() or
                       (t[2] + t[3]).max() > out_bytes or t.max() >= 1 << 40):
        raise ValueError("table: a chunk lies outside the source or the output buffer")


def decode_chunks(src, table, out=None, stream=None, _table_dev=None):
    """(out, status): decode the raw Snappy streams ``table`` lists in ``src``
    (uint8) into ``out`` (uint8 on src's device; allocated to fit if None).
    ``status`` is int32[n] on src's device: 0, or a nonzero code for a chunk
    whose stream is malformed — its bytes of ``out`` are then unspecified, and
    no byte outside a chunk's output range is written either way."""
    n = int(table.shape[1]) if table.dim() == 2 else -1
    if out is None:
        need = int((table[2] + table[3]).max()) if n > 0 else 0
        out = torch.empty(max(need, 0), dtype=torch.uint8, device=src.device)
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or \
            out.device != src.device:
        raise ValueError("out: contiguous uint8[bytes] on the source's device required")
    _check_table(src, table, int(out.numel()))
    if src.device.type != "cuda":
        return out, _decode_chunks_host(src, table, out)
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        status = torch.empty(n, dtype=torch.int32, device=src.device)
        if n:
            tdev = _table_dev if _table_dev is not None else \
                table.contiguous().to(src.device, non_blocking=True)
            rc = lib.hbmr_snappy_decode(_lib.ptr(src), _lib.ptr(tdev), n, _lib.ptr(out),
                                        _lib.ptr(status), _lib.stream_handle(stream))
            _lib.check(rc, "hbmr_snappy_decode")
    return out, status


def _decode_chunks_host(src, table, out):
    """The twin: hbmr_snappy_decompress chunk by chunk."""
    L = snappy._lib()
    s, o = src.numpy(), out.numpy()
    status = np.zeros(table.shape[1], dtype=np.int32)
    for i, (a, c, d, u) in enumerate(table.numpy().T.tolist()):
        buf = ctypes.create_string_buffer(max(u, 1))
        raw = s[a:a + c].tobytes()
        if L.hbmr_snappy_uncompressed_length(raw, c) != u or \
                L.hbmr_snappy_decompress(raw, c, buf, u) != u:
            status[i] = 1
        else:
            o[d:d + u] = np.frombuffer(buf, dtype=np.uint8, count=u)
    return torch.from_numpy(status)


def first_bad_chunk(status):
    """(index, code) of the first chunk with a nonzero status, or None: the one
    host read of a decode."""
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    return (int(bad[0]), int(st[bad[0]])) if bad.size else None


def decode_file(path, device, stream=None):
    """uint8 tensor on ``device``: the decompressed bytes of the Hadoop-framed
    Snappy file ``path``.  ``IOError`` naming the file on bad framing or a
    malformed stream (on a GPU: also the first bad chunk)."""
    from ..fs import strip_scheme
    name = str(path)
    with open(strip_scheme(name), "rb") as f:
        data = f.read()
    if str(device) == "cpu":
        try:
            raw = snappy.hadoop_decompress(data)
        except IOError as e:
            raise IOError(f"{name}: {e}") from None
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
            torch.empty(0, dtype=torch.uint8)
    table, total = chunk_table(data, name)
    n = int(table.shape[1])
    device = torch.device(device)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    # one host buffer, one copy: the table, then the file
    host = torch.empty(32 * n + len(data), dtype=torch.uint8)
    h = host.numpy()
    h[:32 * n] = table.numpy().reshape(-1).view(np.uint8)
    h[32 * n:] = np.frombuffer(data, dtype=np.uint8)
    with _lib.stream_ctx(stream):
        dev = host.to(device)
        tdev = dev[:32 * n].view(torch.int64)
        out = torch.empty(total, dtype=torch.uint8, device=device)
        out, status = decode_chunks(dev[32 * n:], table, out, stream, _table_dev=tdev)
        bad = first_bad_chunk(status)
    if bad is not None:
        raise IOError(f"{name}: malformed snappy stream in chunk {bad[0]} of {n} "
                      f"(decoder code {bad[1]})")
    return out
