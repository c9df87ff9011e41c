"""Word tables on the reduce side (native/kernels/wordtab.hip) and their CPU
twins: what the word-count family's GPU jobs (hbmr/models/wordtable.py) do
after the shuffle.

A word table is what :mod:`hbmr.ops.text` passes around: a uint8 buffer,
``starts`` / ``lens`` int32 per word and ``counts`` int64 per word.

* :func:`partition` — ``(h & INT_MAX) % nparts`` with ``h`` =
  WritableComparator.hashBytes of the word started from ``seed``: seed 1 is
  ``Text(word)``'s partition, ``seed_of(prefix)`` the partition of
  ``Text(prefix + word)`` without building that key.
* :func:`sort_table` — the word ids by (partition, compareBytes), through the
  record sort of :mod:`hbmr.ops.recsort`.
* :func:`line_lengths` / :func:`fill_lines` / :func:`format_part` — a sorted
  run as ``word\\tcount\\n`` lines in one uint8 tensor.
* :func:`sort_counts` / :func:`count_runs` / :func:`histogram_report` — the
  ValueHistogram report of a table's counts.
* :func:`flag_nonclassic` — whether ``str.split`` and ``bytes.split`` can
  disagree on a buffer.

A host tensor takes the numpy / pure-Python twin.  On a GPU the native library
must load (no silent fallback).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import recsort
from . import sort as _sort
from ..io.writable import hash_bytes

INT_MAX = 0x7FFFFFFF


def seed_of(prefix: bytes) -> int:
    """The hash state after ``prefix``: :func:`partition`'s seed for keys that
    are ``prefix + word``.  ``seed_of(b"") == 1``."""
    return hash_bytes(prefix) & 0xFFFFFFFF


def _check_table(buf, starts, lens, counts=None):
    n = starts.numel()
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError("buf: contiguous uint8[bytes] required")
    for name, t in (("starts", starts), ("lens", lens)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or t.device != buf.device or \
                not t.is_contiguous():
            raise ValueError(f"{name}: contiguous int32[n] on the buffer's device required")
    if counts is not None and (counts.dtype != torch.int64 or counts.numel() != n or
                               counts.device != buf.device or not counts.is_contiguous()):
        raise ValueError("counts: contiguous int64[n] on the buffer's device required")
    if n and bool(((starts < 0) | (lens < 0) |
                   (starts.to(torch.int64) + lens > buf.numel())).any()):
        raise ValueError("a word lies outside the buffer")
    return n


def _check_order(order, n, device):
    if order is None:
        return n
    if order.dtype != torch.int32 or order.dim() != 1 or order.device != device or \
            not order.is_contiguous():
        raise ValueError("order: contiguous int32[m] on the table's device required")
    m = order.numel()
    if m and (int(order.min()) < 0 or int(order.max()) >= n):
        raise ValueError("order: a word id outside the table")
    return m


def words_of(buf, starts, lens):
    """The words of a table as bytes objects (host side; tests and twins)."""
    raw = buf.cpu().numpy().tobytes()
    return [raw[s:s + n] for s, n in zip(starts.tolist(), lens.tolist())]


# --------------------------------------------------------------------------- partition
def partition_of(word: bytes, nparts: int, seed: int = 1) -> int:
    h = seed
    for x in word:
        h = (31 * h + (x - 256 if x > 127 else x)) & 0xFFFFFFFF
    return (h & INT_MAX) % nparts


def partition(buf, starts, lens, nparts, seed=1, stream=None):
    """int32[n]: ``(h & INT_MAX) % nparts`` of each word, ``h`` = hashBytes of the
    word's bytes (signed) started from the 32-bit ``seed``."""
    n = _check_table(buf, starts, lens)
    nparts, seed = int(nparts), int(seed) & 0xFFFFFFFF
    if nparts < 1:
        raise ValueError("at least one partition required")
    if not _lib.is_cuda(buf):
        return torch.tensor([partition_of(w, nparts, seed) for w in words_of(buf, starts, lens)],
                            dtype=torch.int32)
    with _lib.stream_ctx(stream, buf):
        parts = torch.empty(n, dtype=torch.int32, device=buf.device)
        rc = _lib.load().hbmr_wordtab_partition(_lib.ptr(buf), _lib.ptr(starts), _lib.ptr(lens), n,
                                                seed, nparts, _lib.ptr(parts),
                                                _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_wordtab_partition")
    return parts


# --------------------------------------------------------------------------- sort
def sort_table(buf, starts, lens, parts, nparts, stream=None):
    """(order int32[n], part_records list[nparts]): the word ids ordered by
    (partition, word bytes as compareBytes orders them) and the words per
    partition.  ``parts``: :func:`partition`'s result."""
    _check_table(buf, starts, lens)
    s64, l64 = starts.to(torch.int64), lens.to(torch.int64)
    index = torch.stack([s64, l64, s64, l64]).contiguous()
    return recsort.sort_perm(buf, index, int(nparts), stream=stream, part=parts)


# --------------------------------------------------------------------------- format
_POW10 = [10 ** k for k in range(1, 19)]


def _chars_np(c):
    """Decimal characters of signed int64 values, the sign included."""
    u = np.abs(c.astype(np.int64)).view(np.uint64)          # |INT64_MIN| as unsigned
    d = np.ones(c.shape, dtype=np.int64)
    for p in _POW10:
        d += u >= np.uint64(p)
    return d + (c < 0)


def line_lengths(lens, counts, order=None, stream=None):
    """int32[m]: the bytes of the line of word ``order[i]`` (None: i): the word,
    a tab, the decimal count, a newline."""
    n = lens.numel()
    if lens.dtype != torch.int32 or counts.dtype != torch.int64 or counts.numel() != n or \
            counts.device != lens.device:
        raise ValueError("lens int32[n] and counts int64[n] on one device required")
    m = _check_order(order, n, lens.device)
    if not _lib.is_cuda(lens):
        sel = slice(None) if order is None else order.numpy().astype(np.int64)
        return torch.from_numpy((lens.numpy()[sel].astype(np.int64) + 2 +
                                 _chars_np(counts.numpy()[sel])).astype(np.int32))
    with _lib.stream_ctx(stream, lens):
        out = torch.empty(m, dtype=torch.int32, device=lens.device)
        rc = _lib.load().hbmr_wordtab_lengths(_lib.ptr(lens.contiguous()),
                                              _lib.ptr(counts.contiguous()), _lib.ptr(order), m,
                                              _lib.ptr(out), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_wordtab_lengths")
    return out


def offsets(lens):
    """int64[n + 1]: the exclusive scan of the line lengths ``lens``, the total
    last (64 bits: a part may exceed 2 GiB)."""
    offs = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
    torch.cumsum(lens, 0, dtype=torch.int64, out=offs[1:])
    return offs


def _fill(buf, starts, lens, counts, order, offs, total, out, stream):
    m = offs.numel() - 1
    if m == 0 or total == 0:
        return out
    if not _lib.is_cuda(buf):
        words = words_of(buf, starts, lens)
        cs = counts.tolist()
        ids = range(m) if order is None else order.tolist()
        text = b"".join(b"%s\t%d\n" % (words[i], cs[i]) for i in ids)
        out.numpy()[:total] = np.frombuffer(text, dtype=np.uint8)
        return out
    with _lib.stream_ctx(stream, buf):
        rc = _lib.load().hbmr_wordtab_fill(_lib.ptr(buf), _lib.ptr(starts), _lib.ptr(lens),
                                           _lib.ptr(counts), _lib.ptr(order), _lib.ptr(offs), m,
                                           total, _lib.ptr(out), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_wordtab_fill")
    return out


def fill_lines(buf, starts, lens, counts, order, offs, out, stream=None):
    """Write the lines of the words ``order`` (None: all, in table order) into
    ``out`` (uint8) at ``offs`` (:func:`offsets` of :func:`line_lengths` of the
    same words).  No byte outside ``out[0 : offs[m]]`` is written."""
    n = _check_table(buf, starts, lens, counts)
    m = _check_order(order, n, buf.device)
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or \
            out.device != buf.device:
        raise ValueError("out: contiguous uint8[bytes] on the table's device required")
    if offs.dtype != torch.int64 or offs.numel() != m + 1 or offs.device != buf.device or \
            not offs.is_contiguous():
        raise ValueError("offs: contiguous int64[m + 1] on the table's device required")
    if m == 0:
        return out
    with _lib.stream_ctx(stream, buf):
        total = int(offs[-1])
        if int(offs[0]) != 0 or total > out.numel() or \
                bool((offs[1:] - offs[:-1] != line_lengths(lens, counts, order, stream)).any()):
            raise ValueError("offs is not the scan of the lines' lengths within the buffer")
    return _fill(buf, starts, lens, counts, order, offs, total, out, stream)


def format_part(buf, starts, lens, counts, order=None, stream=None):
    """uint8[bytes]: the ``word\\tcount\\n`` lines of the words ``order`` (None:
    all, in table order), back to back."""
    n = _check_table(buf, starts, lens, counts)
    _check_order(order, n, buf.device)
    with _lib.stream_ctx(stream, buf):
        offs = offsets(line_lengths(lens, counts, order, stream))
        total = int(offs[-1])
        out = torch.empty(total, dtype=torch.uint8, device=buf.device)
    return _fill(buf, starts, lens, counts, order, offs, total, out, stream)


# --------------------------------------------------------------------------- histogram
def sort_counts(counts, stream=None):
    """The counts of a table (non-negative int64) in ascending order: the radix
    sort of :mod:`hbmr.ops.sort` on a GPU."""
    if counts.dtype != torch.int64 or counts.dim() != 1:
        raise ValueError("counts: int64[n] required")
    if not _lib.is_cuda(counts) or counts.numel() == 0:
        return torch.sort(counts).values
    with _lib.stream_ctx(stream, counts):
        return _sort.radix_sort_keys(counts.clone(), 0, 64, stream)


def count_runs(sorted_counts):
    """(values int64[k], multiplicities int64[k]): the runs of equal counts."""
    if sorted_counts.dtype != torch.int64 or sorted_counts.dim() != 1:
        raise ValueError("sorted_counts: int64[n] required")
    if sorted_counts.numel() == 0:
        z = torch.empty(0, dtype=torch.int64, device=sorted_counts.device)
        return z, z.clone()
    values, mult = torch.unique_consecutive(sorted_counts, return_counts=True)
    return values, mult.to(torch.int64)


def histogram_report(values, multiplicities) -> str:
    """ValueHistogram's report of the counts that the runs (value,
    multiplicity) stand for, in any order: the runs are expanded and sorted on
    the host, and the sums are ValueHistogram's own sequential ones
    (:func:`hbmr.mapred.lib.aggregate.histogram_report`)."""
    from ..mapred.lib.aggregate import histogram_report as report
    v = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values, dtype=np.int64)
    m = np.asarray(multiplicities.cpu() if isinstance(multiplicities, torch.Tensor)
                   else multiplicities, dtype=np.int64)
    if v.shape != m.shape or (m < 0).any():
        raise ValueError("one non-negative multiplicity per value required")
    return report(np.sort(np.repeat(v, m)).tolist())


# --------------------------------------------------------------------------- tokenisers
def flag_nonclassic(buf) -> bool:
    """True if a byte of ``buf`` is >= 0x80 or in 0x1c-0x1f: where
    ``str(text).split()`` (the mappers of multifilewc and the aggregate
    examples) and ``bytes.split()`` (the device tokeniser) can disagree."""
    if buf.numel() == 0:
        return False
    return bool(((buf >= 0x80) | ((buf >= 0x1C) & (buf <= 0x1F))).any())
