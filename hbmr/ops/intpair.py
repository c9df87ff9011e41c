"""Int-pair text: SecondarySort's map and reduce on a split's bytes
(native/kernels/intpair.hip) and the CPU twin — the stages of GPU SecondarySort
(hbmr/models/secondarysort.py).

The definition is the classic job's (hbmr/examples/secondarysort.py):

* a line is an entry of ``split(b"\\n")`` (the last may lack its newline); the
  map is ``str(line).split()``, skipped with fewer than two tokens, else
  ``first, second = int(t0), int(t1)``.  The ASCII white space of ``str.split``
  is 9-13, 28-31 and 32.
* the device (and the twin) take tokens of the form ``[+-]?[0-9]+`` with a
  value in int32.  A split is *irregular* if it holds a byte >= 0x80, or a line
  of at least two tokens whose first or second is not of that form (``1_0``,
  ``0x1``, ``+``, ``2147483648``).  :func:`parse_slow`, the classic expression
  over the decoded text, then redoes the whole split; a token ``int()``
  rejects, or a value outside int32, raises as the classic map does.
* the key is the word of ``IntPair.serialize``: ``(first + 2^31) << 32 |
  (second + 2^31)``, held in int64 storage and ordered unsigned.
* the partition is ``abs(first * 127) % R`` (FirstPartitioner on Python ints).
* a part's text: the records in key order, ``<first>\\t<second>\\n`` each, and
  the separator line in front of the first record of every distinct ``first``.

Stages: :func:`line_starts`, :func:`parse_lines`, :func:`compact` (together
:func:`parse`), :func:`partition`, :func:`sort_keys`, :func:`lengths`,
:func:`fill` (together :func:`format_part`).  Host tensors take the twin
(numpy, no Python step per record); on a GPU the native library must load (no
silent fallback).
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib
from .sort import gather_u64, radix_sort_keys, radix_sort_pairs
from .wordtab import offsets

SKIP, RECORD, IRREGULAR = 0, 1, 2
SEPARATOR_LINE = b"-" * 48 + b"\n"          # SEPARATOR of examples/secondarysort.py and '\n'
RECORD_MAX = 24                              # "-2147483648\t-2147483648\n"
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1

_SPACE = np.zeros(256, dtype=bool)
_SPACE[[9, 10, 11, 12, 13, 28, 29, 30, 31, 32]] = True
_BATCH = 1 << 16                             # records the twin's fill works on at a time
_POW10 = 10 ** np.arange(10, dtype=np.int64)

Parsed = collections.namedtuple("Parsed", "keys lines irregular")
Parsed.__doc__ = """``keys`` int64[records] in line order, ``lines`` the split's
line count, ``irregular`` whether the split needs :func:`parse_slow`."""


def _check_bytes(data):
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("data: contiguous uint8[bytes] required")
    if data.numel() >= 1 << 31:
        raise ValueError("a split of at most 2^31 - 1 bytes required")


def _check_keys(keys):
    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError("keys: contiguous int64[n] required")


def pair_key(first, second):
    """The key word of (first, second) as the signed int64 that stores it."""
    u = ((int(first) + (1 << 31)) << 32) | (int(second) + (1 << 31))
    return u - (1 << 64) if u >= 1 << 63 else u


def firsts(keys):
    """int64: ``first`` of each key (tensor or array)."""
    return ((keys >> 32) & 0xFFFFFFFF) - (1 << 31)


def seconds(keys):
    return (keys & 0xFFFFFFFF) - (1 << 31)


def _excl_scan(counts):
    """(int64 exclusive scan, total) of a device tensor of counts."""
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    return (incl - counts).contiguous(), int(incl[-1]) if incl.numel() else 0


# --------------------------------------------------------------------------- lines
def _line_starts_np(b):
    if b.size == 0:
        return np.zeros(0, dtype=np.int32)
    nl = np.flatnonzero(b == 10)
    return np.concatenate([[0], nl[nl + 1 < b.size] + 1]).astype(np.int32)


def line_starts(data, stream=None):
    """(starts int32[lines], non_ascii): the first byte of each line of the
    split and whether a byte >= 0x80 occurs."""
    _check_bytes(data)
    n = int(data.numel())
    if not _lib.is_cuda(data):
        b = data.numpy()
        return torch.from_numpy(_line_starts_np(b)), bool(b.size and b.max() >= 0x80)
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        st = _lib.stream_handle(stream)
        dev = data.device
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=dev), False
        tc = torch.empty(int(lib.hbmr_intpair_tiles(n)), dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.hbmr_intpair_lines_count(_lib.ptr(data), n, _lib.ptr(tc), _lib.ptr(flag),
                                                st), "hbmr_intpair_lines_count")
        incl = torch.cumsum(tc, 0, dtype=torch.int64)
        base = (incl - tc).contiguous()
        # one host read: the newlines, the last byte and the flag
        newlines, last, high = torch.stack([incl[-1], data[n - 1].long(), flag[0].long()]).tolist()
        nlines = newlines + int(last != 10)
        starts = torch.empty(nlines, dtype=torch.int32, device=dev)
        _lib.check(lib.hbmr_intpair_lines_write(_lib.ptr(data), n, _lib.ptr(base), nlines,
                                                _lib.ptr(starts), st), "hbmr_intpair_lines_write")
        return starts, bool(high)


# --------------------------------------------------------------------------- parse
def _parse_lines_np(b, starts):
    """(status uint8[lines], keys int64[lines]) of the twin."""
    L = starts.size
    status = np.zeros(L, dtype=np.uint8)
    keys = np.zeros(L, dtype=np.int64)
    if L == 0:
        return status, keys
    n = b.size
    sp = _SPACE[b]
    tok = ~sp
    prev_sp = np.concatenate([[True], sp[:-1]])
    next_sp = np.concatenate([sp[1:], [True]])
    tstart = np.flatnonzero(tok & prev_sp)
    tend = np.flatnonzero(tok & next_sp) + 1
    line = np.searchsorted(starts, tstart, side="right") - 1
    per_line = np.bincount(line, minlength=L)
    first_tok = np.cumsum(per_line) - per_line
    two = np.flatnonzero(per_line >= 2)
    if two.size == 0:
        return status, keys
    at = np.stack([first_tok[two], first_tok[two] + 1])          # [2, m]: the two tokens
    s, e = tstart[at].astype(np.int64), tend[at].astype(np.int64)
    sign = (b[s] == 43) | (b[s] == 45)
    neg = b[s] == 45
    ds = s + sign
    digit = (b >= 48) & (b <= 57)
    junk = np.concatenate([[0], np.cumsum(~digit)])
    bad = (e == ds) | (junk[e] != junk[ds])
    nonzero = np.append(np.flatnonzero(b != 48), n)
    lead = np.minimum(nonzero[np.searchsorted(nonzero, ds)], e)  # past the leading zeros
    sig = e - lead
    bad |= sig > 10
    val = np.zeros(s.shape, dtype=np.int64)
    for j in range(10):
        take = (j < sig) & ~bad
        pos = np.where(take, e - 1 - j, 0)
        val += np.where(take, b[pos].astype(np.int64) - 48, 0) * _POW10[j]
    val = np.where(neg, -val, val)
    bad |= (val < INT_MIN) | (val > INT_MAX)
    bad_line = bad[0] | bad[1]
    status[two] = np.where(bad_line, IRREGULAR, RECORD)
    word = ((val[0] + (1 << 31)).astype(np.uint64) << np.uint64(32)) | \
        (val[1] + (1 << 31)).astype(np.uint64)
    keys[two] = np.where(bad_line, 0, word.view(np.int64))
    return status, keys


def parse_lines(data, starts, stream=None):
    """(status uint8[lines], keys int64[lines], block_counts): per line SKIP,
    RECORD or IRREGULAR and a record's key (else 0); ``block_counts`` is the
    kernel's count of records per 256 lines (None from the twin)."""
    return _parse_lines(data, starts, stream)[:3]


def _parse_lines(data, starts, stream):
    """:func:`parse_lines` and the kernel's irregular flag (int32[1]; None from the twin)."""
    _check_bytes(data)
    L = int(starts.numel())
    if starts.dtype != torch.int32 or starts.device != data.device or L > data.numel():
        raise ValueError("starts: int32[lines] on the data's device required")
    if not _lib.is_cuda(data):
        status, keys = _parse_lines_np(data.numpy(), starts.numpy())
        return torch.from_numpy(status), torch.from_numpy(keys), None, None
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        dev = data.device
        status = torch.empty(L, dtype=torch.uint8, device=dev)
        keys = torch.empty(L, dtype=torch.int64, device=dev)
        bc = torch.empty(int(lib.hbmr_intpair_blocks(L)), dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if L:
            rc = lib.hbmr_intpair_parse(_lib.ptr(data), int(data.numel()), _lib.ptr(starts), L,
                                        _lib.ptr(status), _lib.ptr(keys), _lib.ptr(bc),
                                        _lib.ptr(flag), _lib.stream_handle(stream))
            _lib.check(rc, "hbmr_intpair_parse")
        return status, keys, bc, flag


def compact(status, keys, block_counts=None, stream=None, scan=None):
    """int64[records]: the keys of the RECORD lines, in line order (``scan``:
    :func:`_excl_scan` of ``block_counts`` where the caller has it)."""
    if not _lib.is_cuda(keys):
        return keys[status == RECORD].contiguous()
    lib = _lib.load()
    L = int(keys.numel())
    with _lib.stream_ctx(stream):
        base, nrec = scan if scan is not None else _excl_scan(block_counts)
        out = torch.empty(nrec, dtype=torch.int64, device=keys.device)
        rc = lib.hbmr_intpair_compact(_lib.ptr(status), _lib.ptr(keys), L, _lib.ptr(base), nrec,
                                      _lib.ptr(out), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_intpair_compact")
        return out


def parse(data, stream=None):
    """:class:`Parsed` of a split: line starts, per-line parse, compaction."""
    starts, non_ascii = line_starts(data, stream)
    status, keys, bc, flag = _parse_lines(data, starts, stream)
    if flag is None:
        irregular = non_ascii or bool((status == IRREGULAR).any())
        return Parsed(compact(status, keys), int(starts.numel()), irregular)
    with _lib.stream_ctx(stream):
        incl = torch.cumsum(bc, 0, dtype=torch.int64)
        nrec, bad = torch.stack([incl[-1], flag[0].long()]).tolist() if bc.numel() else (0, 0)
        out = compact(status, keys, bc, stream, ((incl - bc).contiguous(), nrec))
    return Parsed(out, int(starts.numel()), non_ascii or bool(bad))


def parse_slow(raw: bytes):
    """int64[records]: the classic map over the decoded text of a split, line by
    line.  Raises ValueError where the classic map fails: a token ``int()``
    rejects, or a value an IntWritable cannot hold."""
    lines = raw.split(b"\n")
    if lines and not lines[-1]:
        lines.pop()
    keys = []
    for line in lines:
        if line.endswith(b"\r"):
            line = line[:-1]
        parts = line.decode("utf-8", errors="replace").split()
        if len(parts) >= 2:
            a, b = int(parts[0]), int(parts[1])
            if not (INT_MIN <= a <= INT_MAX and INT_MIN <= b <= INT_MAX):
                raise ValueError(f"{parts[0]} {parts[1]}: outside the range of an IntWritable")
            keys.append(pair_key(a, b))
    return torch.tensor(keys, dtype=torch.int64)


# --------------------------------------------------------------------------- partition, sort
def partition(keys, nparts, stream=None):
    """int64[n]: ``abs(first * 127) % nparts`` of each key."""
    _check_keys(keys)
    nparts = int(nparts)
    if nparts < 1:
        raise ValueError("at least one partition required")
    if not _lib.is_cuda(keys):
        return torch.from_numpy(np.abs(firsts(keys.numpy()) * 127) % nparts)
    with _lib.stream_ctx(stream):
        parts = torch.empty_like(keys)
        rc = _lib.load().hbmr_intpair_partition(_lib.ptr(keys), int(keys.numel()), nparts,
                                                _lib.ptr(parts), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_intpair_partition")
        return parts


def sort_keys(keys, nparts, stream=None):
    """(keys ordered by (partition, unsigned key), records per partition): the
    radix sort of hbmr/ops/sort.py over the 64-bit key, then with more than one
    partition a stable pass over the partition's bits."""
    _check_keys(keys)
    nparts = int(nparts)
    n = int(keys.numel())
    if not _lib.is_cuda(keys):
        k = keys.numpy().view(np.uint64)
        p = partition(keys, nparts).numpy()
        order = np.lexsort((k, p))
        return (torch.from_numpy(k[order].view(np.int64).copy()),
                np.bincount(p, minlength=nparts).tolist())
    with _lib.stream_ctx(stream):
        keys = radix_sort_keys(keys.clone(), 0, 64, stream)
        if nparts == 1 or n == 0:
            return keys, [n] + [0] * (nparts - 1)
        parts = partition(keys, nparts, stream)
        perm = torch.arange(n, dtype=torch.int32, device=keys.device)
        radix_sort_pairs(parts, perm, 0, max(1, (nparts - 1).bit_length()), stream)
        # the partitions are in order now: their counts are the gaps between cuts
        cuts = torch.searchsorted(parts, torch.arange(nparts + 1, device=keys.device))
        return gather_u64(keys, perm, stream), (cuts[1:] - cuts[:-1]).tolist()


# --------------------------------------------------------------------------- format
def _chars_np(v):
    u = np.abs(v)
    d = np.ones(v.shape, dtype=np.int64)
    for p in _POW10[1:]:
        d += u >= p
    return d + (v < 0)


def _heads_np(k):
    hi = k >> 32
    return np.concatenate([[True], hi[1:] != hi[:-1]]) if k.size else np.zeros(0, dtype=bool)


def heads(keys):
    """bool[n]: whether a record of a part (keys sorted) begins a group — its
    ``first`` differs from its predecessor's; record 0 does."""
    _check_keys(keys)
    h = torch.ones(keys.numel(), dtype=torch.bool, device=keys.device)
    if keys.numel() > 1:
        h[1:] = (keys[1:] >> 32) != (keys[:-1] >> 32)
    return h


def lengths(keys, stream=None):
    """int32[n]: the output bytes of each record of a part (keys sorted): its
    line, and in front of a group head the separator line."""
    _check_keys(keys)
    n = int(keys.numel())
    if not _lib.is_cuda(keys):
        k = keys.numpy()
        ln = _chars_np(firsts(k)) + _chars_np(seconds(k)) + 2 + \
            _heads_np(k) * len(SEPARATOR_LINE)
        return torch.from_numpy(ln.astype(np.int32))
    with _lib.stream_ctx(stream):
        lens = torch.empty(n, dtype=torch.int32, device=keys.device)
        rc = _lib.load().hbmr_intpair_lengths(_lib.ptr(keys), n, _lib.ptr(lens),
                                              _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_intpair_lengths")
        return lens


def _digits_np(v):
    """(chars uint8[m, 11], keep bool[m, 11]): sign and the ten digit places."""
    u = np.abs(v)
    nd = _chars_np(v) - (v < 0)
    ch = np.empty((v.size, 11), dtype=np.uint8)
    ch[:, 0] = 45
    ch[:, 1:] = (u[:, None] // _POW10[::-1][None, :]) % 10 + 48
    keep = np.empty((v.size, 11), dtype=bool)
    keep[:, 0] = v < 0
    keep[:, 1:] = np.arange(10)[None, :] >= (10 - nd)[:, None]
    return ch, keep


def _fill_np(k, head_first):
    """The text of the records ``k`` (a slice of a part; ``head_first``: whether
    its first record is a head)."""
    m = k.size
    hd = _heads_np(k)
    hd[0] = head_first
    sep = np.broadcast_to(np.frombuffer(SEPARATOR_LINE, dtype=np.uint8), (m, len(SEPARATOR_LINE)))
    c1, k1 = _digits_np(firsts(k))
    c2, k2 = _digits_np(seconds(k))
    one = np.ones((m, 1), dtype=bool)
    chars = np.concatenate([sep, c1, np.full((m, 1), 9, np.uint8), c2,
                            np.full((m, 1), 10, np.uint8)], axis=1)
    keep = np.concatenate([np.broadcast_to(hd[:, None], sep.shape), k1, one, k2, one], axis=1)
    return chars[keep]


def fill(keys, offs, out, stream=None):
    """Write the text of a part's records (keys sorted) into ``out`` (uint8) at
    ``offs`` (:func:`offsets` of :func:`lengths` of the same keys).  No byte
    outside ``out[offs[0] : offs[n]]`` is written."""
    _check_keys(keys)
    n = int(keys.numel())
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("out: contiguous uint8[bytes] required")
    if offs.dtype != torch.int64 or offs.numel() != n + 1 or offs.device != keys.device or \
            out.device != keys.device:
        raise ValueError("offs: int64[n + 1] on the keys' device required")
    if n == 0:
        return out
    with _lib.stream_ctx(stream, keys):
        if int(offs[0]) != 0 or int(offs[-1]) > out.numel() or \
                bool((offs[1:] - offs[:-1] != lengths(keys, stream)).any()):
            raise ValueError("offs is not the scan of the records' lengths within the buffer")
    return _fill(keys, offs, out, stream)


def _fill(keys, offs, out, stream):
    n = int(keys.numel())
    if n == 0:
        return out
    if not _lib.is_cuda(keys):
        k, o, dst = keys.numpy(), offs.numpy(), out.numpy()
        for a in range(0, n, _BATCH):
            z = min(n, a + _BATCH)
            dst[o[a]:o[z]] = _fill_np(k[a:z], a == 0 or (k[a] >> 32) != (k[a - 1] >> 32))
        return out
    with _lib.stream_ctx(stream):
        rc = _lib.load().hbmr_intpair_fill(_lib.ptr(keys), _lib.ptr(offs), n, _lib.ptr(out),
                                           _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_intpair_fill")
    return out


def format_part(keys, stream=None):
    """(text uint8[bytes], groups): a part's output from its sorted keys."""
    _check_keys(keys)
    with _lib.stream_ctx(stream, keys):
        lens = lengths(keys, stream)
        offs = offsets(lens)
        total, groups = torch.stack([offs[-1], (lens > RECORD_MAX).sum()]).tolist()
        out = torch.empty(total, dtype=torch.uint8, device=keys.device)
    return _fill(keys, offs, out, stream), groups
