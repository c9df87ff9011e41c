"""Record validation: an order-free digest of the records of a split and the
order and partition checks of SortValidator (native/kernels/recvalidate.hip)
with their CPU twins — the map of GPU SortValidator (hbmr/models/sortvalidate.py).

A split is ``data`` and ``index`` as in :mod:`hbmr.ops.recsort`.  A record is its
frame ``[recordLen][keyLen][key][value]``: ``L = index[FLEN]`` bytes at
``index[FOFF]``; two frames are equal exactly when their raw key and raw value
are.

The frame digest.  ``m = ceil(L / 8)``; ``w_j`` is the little-endian uint64 of the
frame bytes ``[8j, 8j + 8)``, bytes past ``L`` counting as zero — the words are
numbered from the frame's first byte, so the digest does not depend on where the
frame lies in the buffer.  With :func:`mix` the splitmix64 finaliser and all
arithmetic mod 2^64::

    s = sum_j mix(w_j + (j + 1) * WORD_MUL)
    h = mix(s ^ (L * LEN_MUL))

The inner sum is commutative (lanes and chunks take the words in any order); the
outer ``mix`` is not linear, so two records cannot trade words unnoticed, which a
plain sum of word hashes would allow.  A split's digest is four integers:
``records = n``, ``bytes = sum(L - 8)`` (the raw key and value bytes),
``hash_sum = sum h`` and ``hash_sq_sum = sum h^2``, both mod 2^64.

* :func:`digest` / :func:`digest_cpu` — the four integers.
* :func:`check_sorted_part` / :func:`check_sorted_part_cpu` — the records whose
  key is below their predecessor's (compareBytes on the payload) and the
  records HashPartitioner puts in another part than the file's.
* :func:`validate_records` — both over one split with one host read of results.

On a GPU the native library must load (no silent fallback).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, recsort

M64 = (1 << 64) - 1
WORD_MUL = 0x9E3779B97F4A7C15
LEN_MUL = 0xD6E8FEB86659FD93
MIX_MUL_1 = 0xBF58476D1CE4E5B9
MIX_MUL_2 = 0x94D049BB133111EB

_BATCH_WORDS = 1 << 22        # words the twin hashes at a time


def mix(x):
    """The splitmix64 finaliser over a uint64 array (numpy wraps mod 2^64)."""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(MIX_MUL_1)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(MIX_MUL_2)
    return x ^ (x >> np.uint64(31))


def _check_index(data, index):
    """The index rows after the checks every path makes before it touches the
    data (one host read on a device index)."""
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("data: contiguous uint8[bytes] required")
    foff, flen, koff, klen = recsort._rows(index)
    if index.device != data.device:
        raise ValueError("data and index on different devices")
    if int(foff.numel()) >= 1 << 31:
        raise ValueError("at most 2^31 - 1 records per split")
    nb = data.numel()
    if bool(((koff < 0) | (klen < 0) | (koff + klen > nb) | (foff < 0) | (flen < 0) |
             (foff + flen > nb)).any()):
        raise ValueError("record index points outside the data")
    return foff, flen, koff, klen


# --------------------------------------------------------------------------- CPU twins
def _frame_hashes(raw, foff, flen):
    """uint64[n]: the digest of each frame; ``raw`` (uint64, little-endian) is
    the data behind at least 8 zero bytes of padding."""
    n = foff.size
    m = (flen + 7) >> 3
    base = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(m, out=base[1:])
    rec = np.repeat(np.arange(n, dtype=np.int64), m)
    j = np.arange(int(base[-1]), dtype=np.int64) - base[rec]
    # word j of a frame from the two aligned words of the buffer it lies in
    at = (foff >> 3)[rec] + j
    low = ((foff & 7) << 3).astype(np.uint64)[rec]
    w = raw[at] >> low
    off = low > 0                                 # (a shift by 64 is not one)
    w[off] |= raw[at[off] + 1] << (np.uint64(64) - low[off])
    some = m > 0                                  # the last word of a frame: bytes past L are zero
    keep = (8 * (8 - (flen[some] - 8 * (m[some] - 1)))).astype(np.uint64)
    w[base[1:][some] - 1] &= np.uint64(M64) >> keep
    t = mix(w + (j + 1).astype(np.uint64) * np.uint64(WORD_MUL))
    run = np.zeros(t.size + 1, dtype=np.uint64)
    np.cumsum(t, out=run[1:])
    s = run[base[1:]] - run[base[:-1]]
    return mix(s ^ (flen.astype(np.uint64) * np.uint64(LEN_MUL)))


def digest_cpu(data, index):
    """(records, bytes, hash_sum, hash_sq_sum) of the split by numpy, no Python
    step per record."""
    foff, flen, _, _ = _check_index(data, index)
    foff, flen = foff.numpy(), flen.numpy()
    n = int(foff.size)
    nb = int(data.numel())
    raw = np.zeros((nb >> 3) + 2, dtype="<u8")
    raw.view(np.uint8)[:nb] = data.numpy()
    words = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((flen + 7) >> 3, out=words[1:])
    hs = hq = 0
    lo = 0
    while lo < n:                                 # batches of about _BATCH_WORDS words
        hi = int(np.searchsorted(words, words[lo] + _BATCH_WORDS, side="right")) - 1
        hi = min(n, max(hi, lo + 1))
        h = _frame_hashes(raw, foff[lo:hi], flen[lo:hi])
        hs += int(h.sum(dtype=np.uint64))
        hq += int((h * h).sum(dtype=np.uint64))
        lo = hi
    return n, int(flen.sum()) - 8 * n, hs & M64, hq & M64


def check_sorted_part_cpu(data, index, nparts, part):
    """The CPU twin of :func:`check_sorted_part` (host tensors)."""
    _check_index(data, index)
    keys = recsort.payloads(data, index)
    unsorted = sum(1 for a, b in zip(keys, keys[1:]) if b < a)
    mis = 0
    if part is not None:
        mis = sum(1 for p in recsort.partitions_cpu(keys, nparts) if p != part)
    return unsorted, mis


# --------------------------------------------------------------------------- device
def validate_records(data, index, order=False, nparts=1, part=None, stream=None, hashes=True):
    """(records, bytes, hash_sum, hash_sq_sum, unsorted, mispartitioned) of the
    split: its digest (``hashes``; else zeros) and, with ``order``, the records
    whose key is below their predecessor's; with ``part`` (an int) the records
    whose HashPartitioner part of ``nparts`` is another.  On the device the
    kernels write into one small buffer that the host reads once.  Host tensors
    take the twins."""
    if data.device.type != "cuda":
        res = digest_cpu(data, index) if hashes else (0, 0, 0, 0)
        return res + (check_sorted_part_cpu(data, index, nparts, part) if order or part is not None
                      else (0, 0))
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        foff, flen, koff, klen = _check_index(data, index)
        n = int(foff.numel())
        st = _lib.stream_handle(stream)
        out = torch.zeros(6, dtype=torch.int64, device=data.device)
        if hashes:
            rc = lib.hbmr_recvalidate_digest(_lib.ptr(data), _lib.ptr(foff), _lib.ptr(flen), n,
                                             _lib.ptr(out), st)
            _lib.check(rc, "hbmr_recvalidate_digest")
        if order:
            rc = lib.hbmr_recvalidate_order(_lib.ptr(data), _lib.ptr(koff), _lib.ptr(klen), n,
                                            _lib.ptr(out[4:]), st)
            _lib.check(rc, "hbmr_recvalidate_order")
        if part is not None and n:
            got = recsort.hash_partition(data, index, max(1, nparts), stream)
            out[5] = (got != int(part)).sum()
        return tuple(v & M64 for v in out.tolist())      # the one host read of results


def digest(data, index, stream=None):
    """(records, bytes, hash_sum, hash_sq_sum) of the split.  Host tensors take
    :func:`digest_cpu`."""
    if data.device.type != "cuda":
        return digest_cpu(data, index)
    return validate_records(data, index, stream=stream)[:4]


def check_sorted_part(data, index, nparts, part, stream=None):
    """(unsorted, mispartitioned): the records whose key payload is below their
    predecessor's (all descents; equal keys are none) and the records whose
    HashPartitioner part of ``nparts`` is not ``part`` (None: not checked, 0).
    Host tensors take :func:`check_sorted_part_cpu`."""
    if data.device.type != "cuda":
        return check_sorted_part_cpu(data, index, nparts, part)
    return validate_records(data, index, True, nparts, part, stream, hashes=False)[4:]
