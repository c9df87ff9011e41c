"""Record sort: variable-length byte-string keys carrying variable-length
values (native/kernels/recsort.hip, native/io/recindex.cc) and its CPU twin —
SURVEY.md K4/K9 in their general form, the map and reduce of GPU Sort
(hbmr/models/sort.py).

A split is ``data`` (uint8[bytes], the raw byte range of a SequenceFile) and
``index`` (int64[4, n]: per record the offset and length of its frame
``[recordLen][keyLen][key][value]`` and of its key payload).  Order is
WritableComparator.compareBytes on the payload within a partition; equal keys
keep their record order.

* :func:`index_records` / :func:`layout` — the host pieces (C++).
* :func:`sort_records` — partition + string sort + frame gather on the device;
  :func:`sort_records_cpu` — the same results from Python's ``sorted``.
* :func:`round_key` — the 64-bit key of one sort round.

On a GPU the native library must load (no silent fallback).
"""
from __future__ import annotations

import bisect
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import sort as _sort

FOFF, FLEN, KOFF, KLEN = range(4)
KEY_CLASSES = ("org.apache.hadoop.io.BytesWritable", "org.apache.hadoop.io.Text")
SYNC_SIZE = 20

_CPU_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib",
                         "libhbmr_cpu.so")
_CPU = None


def _cpu_lib():
    global _CPU
    if _CPU is None:
        if not os.path.exists(_CPU_PATH):
            raise RuntimeError(f"{_CPU_PATH} missing: run native/build.py")
        L = ctypes.CDLL(_CPU_PATH)
        P, L64 = ctypes.c_void_p, ctypes.c_long
        L.hbmr_seq_index_records.argtypes = [ctypes.c_char_p, L64, L64, P, P, L64]
        L.hbmr_seq_index_records.restype = L64
        L.hbmr_seq_index_last_error.restype = ctypes.c_char_p
        L.hbmr_seq_layout.argtypes = [P, L64, L64, L64, P, P, P]
        L.hbmr_seq_layout.restype = L64
        _CPU = L
    return _CPU


# --------------------------------------------------------------------------- host pieces
def index_records(path, start, length):
    """(data uint8[bytes], index int64[4, n]) of the records a
    SequenceFileRecordReader over (path, start, length) returns: the raw byte
    range that holds them (sync escapes included, not indexed) and, relative
    to it, each record's frame and key payload."""
    from ..fs import strip_scheme
    lib = _cpu_lib()
    p = strip_scheme(str(path))
    rng = np.zeros(2, dtype=np.int64)
    n = lib.hbmr_seq_index_records(p.encode(), start, length, rng.ctypes.data, None, 0)
    if n < 0:
        raise IOError(f"indexing {path}: {lib.hbmr_seq_index_last_error().decode(errors='replace')}")
    index = np.empty((4, n), dtype=np.int64)
    if n:
        got = lib.hbmr_seq_index_records(p.encode(), start, length, rng.ctypes.data,
                                         index.ctypes.data, n)
        if got != n:
            raise IOError(f"indexing {path}: file changed while it was read")
    nbytes = int(rng[1] - rng[0])
    data = np.fromfile(p, dtype=np.uint8, count=nbytes, offset=int(rng[0])) if nbytes else \
        np.empty(0, dtype=np.uint8)
    if data.size != nbytes:
        raise IOError(f"indexing {path}: short read")
    return data, index


def layout(frame_lens, pos, last_sync=0):
    """Offsets of frames of ``frame_lens`` bytes in a file body that begins at
    file position ``pos`` of a Writer whose last sync position is
    ``last_sync``: (dst int64[n], gaps int64[g], total).  ``gaps`` are the body
    offsets of the 20-byte sync escapes, where ``Writer.append_raw`` would
    write them for the same records."""
    lens = np.ascontiguousarray(frame_lens, dtype=np.int64)
    n = lens.size
    dst = np.empty(n, dtype=np.int64)
    gaps = np.empty(max(1, n), dtype=np.int64)
    total = np.zeros(1, dtype=np.int64)
    g = _cpu_lib().hbmr_seq_layout(lens.ctypes.data, n, int(pos), int(last_sync), dst.ctypes.data,
                                   gaps.ctypes.data, total.ctypes.data)
    return dst, gaps[:g].copy(), int(total[0])


def write_part(writer, data, index, order=None, stream=None):
    """Append the records ``order`` (int32 record ids; None: all, in index
    order) of (data, index) to ``writer`` (a fresh or open
    ``sequencefile.Writer``) through the layout path: frame lengths → layout →
    one gather into the file body → the sync escapes filled in.  Returns the
    number of records."""
    flen = index[FLEN] if order is None else index[FLEN][order.long()]
    n = int(flen.numel())
    if n == 0:
        return 0
    dst, gaps, total = layout(flen.cpu().numpy(), writer.out.tell(), writer.last_sync_pos)
    dst_t = torch.from_numpy(dst).to(data.device)
    body = gather_frames(data, order, index[FOFF], index[FLEN], dst_t, total, stream)
    writer.append_frames(body.cpu().numpy(), gaps)
    return n


# --------------------------------------------------------------------------- order
def round_key(payload: bytes, d: int) -> int:
    """The 64-bit key of sort round ``d``: (payload[7d : 7d+7] zero-padded,
    big-endian) << 8 | min(len - 7d, 8).  A low byte <= 7: the key ends in this
    round; 8: it continues."""
    left = max(0, len(payload) - 7 * d)
    chunk = payload[7 * d:7 * d + 7]
    return int.from_bytes(chunk + b"\0" * (7 - len(chunk)), "big") << 8 | min(left, 8)


def round_keys(payload: bytes):
    """The round keys of a payload through the round in which it ends."""
    out = []
    d = 0
    while True:
        k = round_key(payload, d)
        out.append(k)
        if k & 0xFF <= 7:
            return out
        d += 1


_POW31 = np.ones(1, dtype=np.int64)


def _pow31(n):
    global _POW31
    if _POW31.size <= n:
        p = np.empty(max(n + 1, 2 * _POW31.size), dtype=np.int64)
        p[0] = 1
        for i in range(1, p.size):
            p[i] = (p[i - 1] * 31) & 0xFFFFFFFF
        _POW31 = p
    return _POW31


def hash_partition_cpu(payload, nparts: int) -> int:
    """(hashBytes(payload) & INT_MAX) % nparts (HashPartitioner over a
    BytesWritable or Text key), by powers of 31 mod 2^32."""
    b = np.frombuffer(bytes(payload), dtype=np.int8).astype(np.int64)
    n = b.size
    p = _pow31(n)
    h = (int(p[n]) + int((b * p[:n][::-1]).sum())) & 0xFFFFFFFF
    return (h & 0x7FFFFFFF) % nparts


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def payloads(data, index):
    raw = _np(data).tobytes()
    idx = _np(index)
    return [raw[o:o + n] for o, n in zip(idx[KOFF].tolist(), idx[KLEN].tolist())]


def frames(data, index):
    raw = _np(data).tobytes()
    idx = _np(index)
    return [raw[o:o + n] for o, n in zip(idx[FOFF].tolist(), idx[FLEN].tolist())]


def partitions_cpu(keys, nparts, split_points=None):
    if split_points is not None:
        pts = list(split_points)
        return [bisect.bisect_right(pts, k) for k in keys]
    if nparts <= 1:
        return [0] * len(keys)
    return [hash_partition_cpu(k, nparts) for k in keys]


def sort_records_cpu(data, index, nparts, split_points=None):
    """The CPU twin of :func:`sort_records` (same results, host tensors)."""
    keys = payloads(data, index)
    parts = partitions_cpu(keys, nparts, split_points)
    order = sorted(range(len(keys)), key=lambda i: (parts[i], keys[i]))
    fr = frames(data, index)
    part_records, part_bytes = [0] * nparts, [0] * nparts
    for i in order:
        part_records[parts[i]] += 1
        part_bytes[parts[i]] += len(fr[i])
    blob = b"".join(fr[i] for i in order)
    return (torch.tensor(order, dtype=torch.int32), part_records, part_bytes,
            torch.frombuffer(bytearray(blob), dtype=torch.uint8) if blob else
            torch.empty(0, dtype=torch.uint8))


# --------------------------------------------------------------------------- device
_ptr = _lib.ptr


def _rows(index):
    if index.dtype != torch.int64 or index.dim() != 2 or index.shape[0] != 4:
        raise ValueError("index int64[4, n] required")
    index = index.contiguous()
    return index[FOFF], index[FLEN], index[KOFF], index[KLEN]


def hash_partition(data, index, nparts, stream=None):
    """int32[n]: HashPartitioner's partition of each record's key payload."""
    foff, flen, koff, klen = _rows(index)
    n = int(koff.numel())
    if data.device.type != "cuda":
        return torch.tensor(partitions_cpu(payloads(data, index), nparts), dtype=torch.int32)
    part = torch.empty(n, dtype=torch.int32, device=data.device)
    rc = _lib.load().hbmr_recsort_hash_partition(_ptr(data), _ptr(koff), _ptr(klen), n, nparts,
                                                 _ptr(part), _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_recsort_hash_partition")
    return part


def round_keys_device(data, index, rec, d, stream=None):
    """int64[m] (uint64 bits): round key ``d`` of the records ``rec`` (int32)."""
    foff, flen, koff, klen = _rows(index)
    m = int(rec.numel())
    keys = torch.empty(m, dtype=torch.int64, device=data.device)
    vals = torch.empty(m, dtype=torch.int32, device=data.device)
    rc = _lib.load().hbmr_recsort_round_keys(_ptr(data), _ptr(koff), _ptr(klen), _ptr(rec), m, d,
                                             _ptr(keys), _ptr(vals), _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_recsort_round_keys")
    return keys


def _split_point_tensors(split_points, device):
    pts = [bytes(p) for p in split_points]
    lens = np.array([len(p) for p in pts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if pts else lens
    blob = np.frombuffer(b"".join(pts) or b"\0", dtype=np.uint8).copy()
    return (torch.from_numpy(blob).to(device), torch.from_numpy(offs).to(device),
            torch.from_numpy(lens).to(device))


def sort_perm(data, index, nparts, split_points=None, stream=None, stats=None, part=None):
    """(perm int32[n], part_records list[nparts]): the record ids ordered by
    (partition, key payload), stable, and the records per partition.
    ``stats`` (a dict) receives ``rounds``.  ``part`` (int32[n], values in
    [0, nparts)): the records' partitions, computed by the caller, in place of
    HashPartitioner's."""
    foff, flen, koff, klen = _rows(index)
    n = int(koff.numel())
    dev = data.device
    if split_points is not None and len(split_points) != nparts - 1:
        raise ValueError(f"{nparts} partitions need {nparts - 1} split points")
    if part is not None:
        if split_points is not None:
            raise ValueError("either split points or precomputed partitions")
        if part.dtype != torch.int32 or part.numel() != n or part.device != dev:
            raise ValueError("part: int32[n] on the data's device required")
        if n and (int(part.min()) < 0 or int(part.max()) >= nparts):
            raise ValueError("part: a partition outside [0, nparts)")
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), [0] * nparts
    if n >= 1 << 31:
        raise ValueError("at most 2^31 - 1 records per sort")
    if dev.type != "cuda":
        if part is not None:
            keys, parts = payloads(data, index), part.tolist()
            order = sorted(range(n), key=lambda i: (parts[i], keys[i]))
            return (torch.tensor(order, dtype=torch.int32),
                    np.bincount(part.numpy(), minlength=nparts).tolist())
        perm, part_records, _, _ = sort_records_cpu(data, index, nparts, split_points)
        return perm, part_records
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        st = _lib.stream_handle(stream)
        nb = data.numel()
        if bool(((koff < 0) | (klen < 0) | (koff + klen > nb) | (foff < 0) | (flen < 0) |
                 (foff + flen > nb)).any()):
            raise ValueError("record index points outside the data")
        counts = None
        if split_points is None and nparts > 1:
            if part is None:
                part = hash_partition(data, index, nparts, stream)
            seg64 = part.to(torch.int64)
            perm = torch.arange(n, dtype=torch.int32, device=dev)
            _sort.radix_sort_pairs(seg64, perm, 0, max(1, (nparts - 1).bit_length()), stream)
            seg = seg64.to(torch.int32)
            counts = torch.bincount(part, minlength=nparts)
        else:
            perm = torch.arange(n, dtype=torch.int32, device=dev)
            seg = torch.zeros(n, dtype=torch.int32, device=dev)
        pos = torch.arange(n, dtype=torch.int32, device=dev)
        cur = [pos, perm.clone(), seg]
        nxt = [torch.empty_like(pos) for _ in range(3)]
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        wsb = int(lib.hbmr_recsort_round_workspace_bytes(n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        seg_bits = max(1, max(n - 1, nparts - 1).bit_length())
        max_rounds = (int(klen.max()) + 1 + 6) // 7
        m, d = n, 0
        while m > 0:
            if d >= max_rounds:
                raise RuntimeError(f"record sort still has {m} active records after {d} rounds")
            rc = lib.hbmr_recsort_round(_ptr(data), _ptr(koff), _ptr(klen), d, m, seg_bits,
                                        _ptr(cur[0]), _ptr(cur[1]), _ptr(cur[2]), _ptr(perm),
                                        _ptr(nxt[0]), _ptr(nxt[1]), _ptr(nxt[2]), _ptr(count),
                                        _ptr(ws), wsb, st)
            _lib.check(rc, "hbmr_recsort_round")
            m = int(count.item())          # the one host read of a round
            cur, nxt = nxt, cur
            d += 1
        if stats is not None:
            stats["rounds"] = d
        if split_points is not None and nparts > 1:
            sp, sp_off, sp_len = _split_point_tensors(split_points, dev)
            cuts = torch.empty(nparts - 1, dtype=torch.int64, device=dev)
            rc = lib.hbmr_recsort_cuts(_ptr(data), _ptr(koff), _ptr(klen), _ptr(perm), n,
                                       _ptr(sp), _ptr(sp_off), _ptr(sp_len), nparts - 1,
                                       _ptr(cuts), st)
            _lib.check(rc, "hbmr_recsort_cuts")
            edges = [0] + cuts.tolist() + [n]
            part_records = [edges[i + 1] - edges[i] for i in range(nparts)]
        elif counts is not None:
            part_records = counts.tolist()
        else:
            part_records = [n] + [0] * (nparts - 1)
    return perm, part_records


def _chunk_table(dst_off, lens, out, skip_empty=False, chunk=None):
    """(base int64[n + 1], entry int32[total], total): the chunk table of a copy
    of n runs of ``lens`` bytes to the offsets ``dst_off`` of ``out``.  A run is
    cut into chunks of ``chunk`` bytes (hbmr_recsort_chunk_bytes() if None)
    counted from the 16-byte boundary below its first byte in memory; ``base`` is
    the exclusive scan of the chunks per run, ``entry`` the run of each chunk.
    ``skip_empty``: an empty run gets no chunk (else one if it starts off a
    boundary)."""
    if chunk is None:
        chunk = int(_lib.load().hbmr_recsort_chunk_bytes())
    n = int(lens.numel())
    nch = (((dst_off + out.data_ptr()) & 15) + lens + (chunk - 1)) // chunk
    if skip_empty:
        nch = torch.where(lens > 0, nch, 0)
    base = torch.zeros(n + 1, dtype=torch.int64, device=out.device)
    torch.cumsum(nch, 0, out=base[1:])
    total = int(base[-1].item())
    entry = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=out.device), nch,
                                    output_size=total)
    return base, entry, total


def gather_frames(data, order, foff, flen, dst_off, out_bytes, stream=None, check=True, out=None):
    """uint8[out_bytes] with frame ``order[i]`` (None: i) of ``data`` copied to
    offset ``dst_off[i]``; bytes no frame covers are left unset (``out``: this
    device buffer of out_bytes, whose other bytes stay as they are).  ``check``
    validates the offsets against both buffers first (one host read)."""
    n = int(dst_off.numel())
    dev = data.device
    sel = None if order is None else order.long()
    lens = flen if sel is None else flen[sel]
    if check and n:
        src_off = foff if sel is None else foff[sel]
        bad = ((src_off < 0) | (lens < 0) | (src_off + lens > data.numel()) | (dst_off < 0) |
               (dst_off + lens > out_bytes)).any()
        if sel is not None:
            bad = bad | (sel < 0).any() | (sel >= foff.numel()).any()
        if bool(bad):
            raise ValueError("gather_frames: a frame lies outside its buffer")
    if dev.type != "cuda":
        out = np.zeros(out_bytes, dtype=np.uint8)
        src = data.numpy()
        src_off = foff if sel is None else foff[sel]
        for s, ln, d in zip(src_off.tolist(), lens.tolist(), dst_off.tolist()):
            out[d:d + ln] = src[s:s + ln]
        return torch.from_numpy(out)
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        if out is None:
            out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or out.numel() != out_bytes or out.device != dev or \
                not out.is_contiguous():
            raise ValueError("gather_frames: out must be contiguous uint8[out_bytes] on the device")
        if n == 0 or out_bytes == 0:
            return out
        base, entry, total = _chunk_table(dst_off, lens, out)
        rc = lib.hbmr_recsort_gather(_ptr(data), _ptr(order), _ptr(foff), _ptr(flen),
                                     _ptr(dst_off.contiguous()), _ptr(base), _ptr(entry), n, total,
                                     _ptr(out), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_recsort_gather")
    return out


def sort_records(data, index, nparts, split_points=None, stream=None, stats=None):
    """Partition, sort and gather the records of (data, index): returns
    ``(perm, part_records, part_bytes, blob)`` — the record ids ordered by
    (partition, key payload) with equal keys in record order, the records and
    frame bytes of each partition, and the frames in that order back to back.
    Partitions: HashPartitioner over the payload, or with ``split_points``
    (nparts - 1 sorted payloads) TotalOrderPartitioner's.  Host tensors take
    :func:`sort_records_cpu`."""
    if data.device.type != "cuda":
        return sort_records_cpu(data, index, nparts, split_points)
    foff, flen, koff, klen = _rows(index)
    perm, part_records = sort_perm(data, index, nparts, split_points, stream, stats)
    n = int(perm.numel())
    with _lib.stream_ctx(stream):
        if n == 0:
            return perm, part_records, [0] * nparts, torch.empty(0, dtype=torch.uint8,
                                                                 device=data.device)
        ends = torch.cumsum(flen[perm.long()], 0)
        edges = np.cumsum(part_records)
        at = ends[torch.from_numpy(np.maximum(edges - 1, 0)).to(ends.device)].tolist()
        part_ends = [a if e > 0 else 0 for a, e in zip(at, edges.tolist())]
        part_bytes = [part_ends[0]] + [part_ends[i] - part_ends[i - 1] for i in range(1, nparts)]
        dst = ends - flen[perm.long()]
        blob = gather_frames(data, perm, foff, flen, dst, part_ends[-1], stream, check=False)
    return perm, part_records, part_bytes, blob
