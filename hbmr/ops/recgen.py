"""Record generator: RandomWriter's and RandomTextWriter's records written
straight into a SequenceFile body (native/kernels/recgen.hip) and the CPU twin
— the map of GPU RandomWriter (hbmr/models/randomwrite.py).

The definition is counter-based, so any byte is computable alone and the bytes
depend only on (seed, map, record, byte offset).  All arithmetic is unsigned
and wraps; ``lo32``/``hi32`` are the halves of a 64-bit word and
``mulhi32(x, r) = (x * r) >> 32``::

    mix64    the splitmix64 finaliser (hbmr.ops.recvalidate.mix)
    S(m)     = mix64(seed + (m + 1) * S_MUL)            m: map (split) index
    R(m,i)   = mix64(S(m) + (i + 1) * R_MUL)            i: record of the map
    B(m,i,t) = mix64(R(m,i) + (t + 1) * B_MUL)          t: 0 key, 1 value
    w32(j)   : x = lo32(B) + j; x ^= x >> 16; x *= W_MUL_1; x ^= hi32(B);
               x ^= x >> 15; x *= W_MUL_2; x ^= x >> 15

``kind`` BYTES (BytesWritable/BytesWritable): ``params = (min_key, max_key,
min_value, max_value)``, both ends inclusive; ``kl = min_key + mulhi32(lo32(R),
max_key - min_key + 1)``, ``vl`` from ``hi32(R)`` the same way; payload bytes
``4j .. 4j+3`` of stream ``t`` are ``w32(j)`` little-endian; the frame is
``[8+kl+vl][4+kl][kl][key][vl][value]``, integers big-endian.

``kind`` TEXT (Text/Text): ``params`` are the word counts' bounds, drawn the
same way; word ``k`` of stream ``t`` is ``vocabulary[mulhi32(w32(k), V)]``; a
payload is its words joined by one space; the frame is
``[recLen][keyLen][vint(kl)][key][vint(vl)][value]``.

A map writes records ``0 .. n-1``, ``n`` the smallest count whose payload
bytes ``sum(kl + vl)`` reach its target (the classic mapper's stop rule).

* :func:`lengths` — payload lengths (and word counts) of a record range.
* :func:`plan` — the records up to the stop rule and their place in a file body:
  lengths in growing batches, then :func:`hbmr.ops.recsort.layout`.
* :func:`fill` — every frame of a plan written into a buffer; :func:`fill_syncs`
  — the sync escapes of the body's holes.
* :func:`generate` / :func:`generate_cpu` — the three together.

Host tensors take the twin (numpy, no Python step per record); on a GPU the
native library must load (no silent fallback).
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib, recsort
from .recvalidate import M64, mix

S_MUL = 0x9E3779B97F4A7C15
R_MUL = 0xD6E8FEB86659FD93
B_MUL = 0x94D049BB133111EB
W_MUL_1 = 0x21F0AAAD
W_MUL_2 = 0x735A2D97

BYTES, TEXT = "bytes", "text"
KL, VL, NK, NV = range(4)              # the rows of :func:`lengths`
MAX_WORDS = 1024                       # what the text kernels hold in LDS
MAX_VOCABULARY_BYTES = 16384

_BATCH_RECORDS = 1 << 13               # records the twin works on at a time
_MAX_BATCH = 1 << 22                   # records of one lengths call in plan()

Plan = collections.namedtuple("Plan", "index gaps total payload first")
Plan.__doc__ = """``index`` int64[4, n] relative to the body (frame offset and
length, key payload offset and length), ``gaps`` the body offsets of the sync
holes, ``total`` the body's bytes, ``payload`` sum(kl + vl), ``first`` the
first record's number within the map."""


# --------------------------------------------------------------------------- definition
def _mix_int(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def split_word(seed, m):
    """S(m) of ``seed`` (any int: taken mod 2^64)."""
    return _mix_int(((seed & M64) + (m + 1) * S_MUL) & M64)


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def _rec_words(S, first, count):
    i = np.arange(first + 1, first + count + 1, dtype=np.uint64)
    return mix(np.full(count, S, dtype=np.uint64) + i * _u64(R_MUL))


def _stream_words(R, t):
    return mix(R + _u64(((t + 1) * B_MUL) & M64))


def _halves(x):
    return (x & _u64(0xFFFFFFFF)).astype(np.uint32), (x >> _u64(32)).astype(np.uint32)


def _w32(a, b, j):
    x = a + j.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(W_MUL_1)
    x = x ^ b
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(W_MUL_2)
    return x ^ (x >> np.uint32(15))


def _mulhi32(x, r):
    return ((x.astype(np.uint64) * _u64(r)) >> _u64(32)).astype(np.int64)


def check_params(kind, params):
    """The four bounds as ints; ValueError for a range that is none or for
    records that can stay empty forever (both maxima 0)."""
    if kind not in (BYTES, TEXT):
        raise ValueError(f"record kind {kind!r}: {BYTES!r} or {TEXT!r}")
    lo_k, hi_k, lo_v, hi_v = (int(p) for p in params)
    what = "length" if kind == BYTES else "word count"
    for lo, hi, side in ((lo_k, hi_k, "key"), (lo_v, hi_v, "value")):
        if not 0 <= lo <= hi < 1 << 31:
            raise ValueError(f"{side} {what} range [{lo}, {hi}] is not one within [0, 2^31)")
    if hi_k == 0 and hi_v == 0:
        raise ValueError(f"key and value {what}s are both 0: no record ever adds a byte")
    return lo_k, hi_k, lo_v, hi_v


class Vocabulary:
    """The words as the ops take them: a byte blob and the word offsets."""

    def __init__(self, words):
        ws = [w.encode() if isinstance(w, str) else bytes(w) for w in words]
        why = vocabulary_reason(ws)
        if why is not None:
            raise ValueError(why)
        self.words = ws
        self.blob = np.frombuffer(b"".join(ws), dtype=np.uint8).copy()
        self.off = np.zeros(len(ws) + 1, dtype=np.int32)
        np.cumsum([len(w) for w in ws], out=self.off[1:])
        self.lens = np.diff(self.off).astype(np.int64)
        self._device = {}

    def on(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.blob).to(device),
                                 torch.from_numpy(self.off).to(device))
        return self._device[key]


def vocabulary_reason(words):
    """None if the text ops take the vocabulary, else why not."""
    ws = [w.encode() if isinstance(w, str) else bytes(w) for w in words]
    if not ws:
        return "empty vocabulary"
    if any(not w for w in ws):
        return "vocabulary with an empty word"
    nbytes = sum(len(w) for w in ws)
    if len(ws) > MAX_WORDS or nbytes > MAX_VOCABULARY_BYTES:
        return (f"vocabulary of {len(ws)} words in {nbytes} bytes (the text kernels hold at "
                f"most {MAX_WORDS} words in {MAX_VOCABULARY_BYTES} bytes)")
    return None


def _vocab(kind, vocabulary):
    if kind != TEXT:
        return None
    if vocabulary is None:
        raise ValueError("text records need a vocabulary")
    return vocabulary if isinstance(vocabulary, Vocabulary) else Vocabulary(vocabulary)


def _vint_size(v):
    """Bytes of Hadoop's VInt of the non-negative int64 array or tensor ``v``."""
    n = v * 0 + 1
    for above in (127, 255, 65535, (1 << 24) - 1):
        n = n + (v > above)
    return n


def frame_lengths(kind, kl, vl):
    """(frame length, offset of the key payload in the frame) of records with
    payloads of ``kl`` and ``vl`` bytes (int64 arrays or tensors)."""
    if kind == BYTES:
        return 16 + kl + vl, kl * 0 + 12
    ks = _vint_size(kl)
    return 8 + ks + kl + _vint_size(vl) + vl, 8 + ks


# --------------------------------------------------------------------------- CPU twin
def _segments(counts):
    """(base int64[n + 1], rec, pos): for n runs of ``counts`` items the
    exclusive scan, and per item its run and its place in the run."""
    base = np.zeros(counts.size + 1, dtype=np.int64)
    np.cumsum(counts, out=base[1:])
    rec = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    return base, rec, np.arange(int(base[-1]), dtype=np.int64) - base[rec]


def _word_ids(B, counts, V):
    """(base, rec, k, id) of the words of streams ``B`` with ``counts`` words."""
    base, rec, k = _segments(counts)
    a, b = _halves(B)
    return base, rec, k, _mulhi32(_w32(a[rec], b[rec], k), V)


def _words_len(B, counts, voc):
    base, rec, k, ids = _word_ids(B, counts, len(voc.words))
    run = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(voc.lens[ids], out=run[1:])
    return run[base[1:]] - run[base[:-1]] + np.maximum(counts - 1, 0)


def _lengths_cpu(kind, S, first, count, params, voc):
    lo_k, hi_k, lo_v, hi_v = params
    out = np.zeros((4, count), dtype=np.int64)
    for a in range(0, count, _BATCH_RECORDS):
        z = min(count, a + _BATCH_RECORDS)
        R = _rec_words(S, first + a, z - a)
        lo, hi = _halves(R)
        nk = lo_k + _mulhi32(lo, hi_k - lo_k + 1)
        nv = lo_v + _mulhi32(hi, hi_v - lo_v + 1)
        if kind == BYTES:
            out[KL, a:z], out[VL, a:z] = nk, nv
        else:
            out[KL, a:z] = _words_len(_stream_words(R, 0), nk, voc)
            out[VL, a:z] = _words_len(_stream_words(R, 1), nv, voc)
            out[NK, a:z], out[NV, a:z] = nk, nv
    return out


def _put_be32(out, pos, v):
    for i in range(4):
        out[pos + i] = (v >> (8 * (3 - i))) & 0xFF


def _put_vint(out, pos, v):
    n = _vint_size(v)
    one = n == 1
    out[pos[one]] = v[one]
    for nb in range(1, 5):
        sel = n == nb + 1
        if sel.any():
            out[pos[sel]] = 0x90 - nb
            for i in range(1, nb + 1):
                out[pos[sel] + i] = (v[sel] >> (8 * (nb - i))) & 0xFF


def _put_stream(out, B, pos, ln):
    """out[pos[r] : + ln[r]] = the first ln[r] bytes of stream B[r]."""
    base, rec, j = _segments((ln + 3) >> 2)
    a, b = _halves(B)
    w = _w32(a[rec], b[rec], j).astype("<u4").view(np.uint8).reshape(-1, 4)
    q = 4 * j[:, None] + np.arange(4, dtype=np.int64)
    keep = q < ln[rec][:, None]
    out[(pos[rec][:, None] + q)[keep]] = w[keep]


def _put_words(out, B, pos, counts, voc):
    """out[pos[r] : ...] = the ``counts[r]`` words of stream B[r] joined by spaces."""
    base, rec, k, ids = _word_ids(B, counts, len(voc.words))
    if ids.size == 0:
        return
    wl = voc.lens[ids]
    item = wl + (k > 0)                                   # the space goes in front
    excl = np.cumsum(item) - item
    at = pos[rec] + excl - excl[base[rec]] + (k > 0)
    out[at[k > 0] - 1] = 0x20
    _, wrec, t = _segments(wl)
    out[at[wrec] + t] = voc.blob[voc.off[ids][wrec].astype(np.int64) + t]


def _unvint(rest):
    return np.where(rest - 1 <= 127, rest - 1,
                    np.where(rest - 2 < 256, rest - 2,
                             np.where(rest - 3 < 65536, rest - 3,
                                      np.where(rest - 4 < 1 << 24, rest - 4, rest - 5))))


def _fill_cpu(kind, S, first, index, out, params, voc):
    foff, flen, koff, klen = (np.ascontiguousarray(r) for r in index)
    n = foff.size
    for a in range(0, n, _BATCH_RECORDS):
        z = min(n, a + _BATCH_RECORDS)
        fo, fl, kl = foff[a:z], flen[a:z], klen[a:z]
        R = _rec_words(S, first + a, z - a)
        if kind == BYTES:
            vl = fl - 16 - kl
            _put_be32(out, fo, 8 + kl + vl)
            _put_be32(out, fo + 4, 4 + kl)
            _put_be32(out, fo + 8, kl)
            _put_be32(out, fo + 12 + kl, vl)
            _put_stream(out, _stream_words(R, 0), fo + 12, kl)
            _put_stream(out, _stream_words(R, 1), fo + 16 + kl, vl)
        else:
            lo_k, hi_k, lo_v, hi_v = params
            lo, hi = _halves(R)
            nk = lo_k + _mulhi32(lo, hi_k - lo_k + 1)
            nv = lo_v + _mulhi32(hi, hi_v - lo_v + 1)
            ks = _vint_size(kl)
            vl = _unvint(fl - 8 - ks - kl)
            vs = _vint_size(vl)
            _put_be32(out, fo, fl - 8)
            _put_be32(out, fo + 4, ks + kl)
            _put_vint(out, fo + 8, kl)
            _put_vint(out, fo + 8 + ks + kl, vl)
            _put_words(out, _stream_words(R, 0), fo + 8 + ks, nk, voc)
            _put_words(out, _stream_words(R, 1), fo + 8 + ks + kl + vs, nv, voc)


# --------------------------------------------------------------------------- ops
def _ranges(params):
    lo_k, hi_k, lo_v, hi_v = params
    return lo_k, hi_k - lo_k + 1, lo_v, hi_v - lo_v + 1


def lengths(kind, seed, m, first, count, params, device="cpu", vocabulary=None, stream=None):
    """int64[4, count] on ``device``: rows KL and VL, the key and value payload
    lengths of records ``first .. first + count - 1`` of map ``m``, and for text
    NK and NV, their word counts (bytes records: 0)."""
    params = check_params(kind, params)
    voc = _vocab(kind, vocabulary)
    count = int(count)
    if first < 0 or count < 0 or count >= 1 << 31:
        raise ValueError("record range outside [0, 2^31)")
    S = split_word(seed, m)
    if not _lib.is_cuda(device):
        return torch.from_numpy(_lengths_cpu(kind, S, int(first), count, params, voc))
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        out = torch.empty((4, count), dtype=torch.int64, device=device)
        woff = voc.on(device)[1] if voc is not None else None
        rc = lib.hbmr_recgen_lengths(S, int(first), count, int(kind == TEXT), *_ranges(params),
                                     _lib.ptr(woff), len(voc.words) if voc else 0,
                                     _lib.ptr(out), _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_recgen_lengths")
    return out


def _mean_payload(kind, params, voc):
    lo_k, hi_k, lo_v, hi_v = params
    per = 1.0 if kind == BYTES else float(voc.lens.mean()) + 1.0
    return max(1.0, (lo_k + hi_k + lo_v + hi_v) / 2.0 * per)


def plan(kind, seed, m, first, target, params, device="cpu", pos=0, last_sync=0,
         vocabulary=None, max_bytes=None, stream=None):
    """The :class:`Plan` of the records ``first, first + 1, ...`` of map ``m``
    through the first at which their payload bytes reach ``target`` — or, with
    ``max_bytes``, through the last with which the body still stays within
    ``max_bytes`` (at least one record) — laid out as a file body that begins
    at file position ``pos`` of a Writer whose last sync lies at ``last_sync``.
    Lengths come in growing batches, the running sums and the cut are taken on
    the device, the layout is :func:`hbmr.ops.recsort.layout`."""
    params = check_params(kind, params)
    voc = _vocab(kind, vocabulary)
    target = int(target)
    parts, done, paid, framed = [], 0, 0, 0
    batch = min(_MAX_BATCH, max(64, int(target / _mean_payload(kind, params, voc) * 1.05) + 16))
    if max_bytes is not None:
        batch = min(batch, max(64, int(max_bytes) // 16))
    with _lib.stream_ctx(stream):
        while target > 0:
            L = lengths(kind, seed, m, first + done, batch, params, device, voc, stream)
            pay = torch.cumsum(L[KL] + L[VL], 0) + paid
            take = int(torch.searchsorted(pay, target))          # the first that reaches it
            stop = take < batch
            take = take + 1 if stop else batch
            if max_bytes is not None:
                # a frame has at most one sync escape in front of it
                size = torch.cumsum(frame_lengths(kind, L[KL], L[VL])[0] + recsort.SYNC_SIZE, 0)
                fit = int(torch.searchsorted(size + framed, int(max_bytes), right=True))
                if fit < take:
                    take, stop = max(fit, 0 if done else 1), True
                framed += int(size[take - 1]) if take else 0
            parts.append(L[:, :take])
            paid = int(pay[take - 1]) if take else paid
            done += take
            if stop:
                break
            batch = min(_MAX_BATCH, 2 * batch)
        L = torch.cat(parts, dim=1) if parts else \
            torch.zeros((4, 0), dtype=torch.int64, device=device)
        flen, kpre = frame_lengths(kind, L[KL], L[VL])
        dst, gaps, total = recsort.layout(flen.cpu().numpy(), pos, last_sync)
        dst = torch.from_numpy(dst).to(L.device)
        index = torch.stack([dst, flen, dst + kpre, L[KL]]).contiguous()
    return Plan(index, gaps, total, paid, int(first))


def _check_fill(kind, index, out):
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("out: contiguous uint8[bytes] required")
    foff, flen, koff, klen = recsort._rows(index)
    if index.device != out.device:
        raise ValueError("index and out on different devices")
    if int(foff.numel()) >= 1 << 31:
        raise ValueError("at most 2^31 - 1 records per fill")
    head = 16 if kind == BYTES else 10
    if bool(((foff < 0) | (klen < 0) | (klen + head > flen) | (foff + flen > out.numel())).any()):
        raise ValueError("record index points outside the buffer")
    return foff, flen, koff, klen


def fill(kind, seed, m, first, index, out, params=None, vocabulary=None, stream=None):
    """Write the frames of records ``first .. first + n - 1`` of map ``m`` into
    ``out`` (uint8) where ``index`` (int64[4, n], relative to ``out``: a
    :class:`Plan`'s) puts them.  Bytes outside the frames — the sync holes —
    stay as they are.  Text records need their ``params`` and ``vocabulary``."""
    voc = _vocab(kind, vocabulary)
    if kind == TEXT:
        params = check_params(kind, params)
    elif kind != BYTES:
        raise ValueError(f"record kind {kind!r}")
    foff, flen, koff, klen = _check_fill(kind, index, out)
    n = int(foff.numel())
    S = split_word(seed, m)
    if n == 0:
        return out
    if out.device.type != "cuda":
        _fill_cpu(kind, S, int(first), index.numpy(), out.numpy(), params, voc)
        return out
    lib = _lib.load()
    with _lib.stream_ctx(stream):
        st = _lib.stream_handle(stream)
        if kind == BYTES:
            base, entry, total = recsort._chunk_table(foff, flen, out,
                                                      chunk=int(lib.hbmr_recgen_chunk_bytes()))
            rc = lib.hbmr_recgen_fill_bytes(S, int(first), _lib.ptr(foff), _lib.ptr(flen),
                                            _lib.ptr(klen), _lib.ptr(base), _lib.ptr(entry), n,
                                            total, _lib.ptr(out), st)
            _lib.check(rc, "hbmr_recgen_fill_bytes")
        else:
            blob, woff = voc.on(out.device)
            rc = lib.hbmr_recgen_fill_text(S, int(first), n, *_ranges(params), _lib.ptr(blob),
                                           _lib.ptr(woff), len(voc.words), int(voc.blob.size),
                                           _lib.ptr(foff), _lib.ptr(flen), _lib.ptr(klen),
                                           _lib.ptr(out), st)
            _lib.check(rc, "hbmr_recgen_fill_text")
    return out


def fill_syncs(out, gaps, escape, stream=None):
    """Write the 20 bytes ``escape`` (the sync escape and a file's marker) at
    each offset of ``gaps`` of ``out``, as ``Writer.append_frames`` does to the
    file copy."""
    escape = bytes(escape)
    if len(escape) != recsort.SYNC_SIZE:
        raise ValueError(f"a sync escape has {recsort.SYNC_SIZE} bytes")
    gaps = np.asarray(gaps, dtype=np.int64)
    if gaps.size == 0:
        return out
    if gaps.min() < 0 or gaps.max() + recsort.SYNC_SIZE > out.numel():
        raise ValueError("a sync hole lies outside the buffer")
    with _lib.stream_ctx(stream, out):
        at = torch.from_numpy(gaps[:, None] + np.arange(recsort.SYNC_SIZE)).reshape(-1)
        esc = torch.frombuffer(bytearray(escape), dtype=torch.uint8).repeat(gaps.size)
        out[at.to(out.device)] = esc.to(out.device)
    return out


def generate(kind, seed, m, first, target, params, device="cpu", pos=0, last_sync=0,
             vocabulary=None, max_bytes=None, escape=None, stream=None):
    """(data uint8[plan.total] on ``device``, plan): :func:`plan`, then
    :func:`fill`, then with ``escape`` :func:`fill_syncs`.  Without ``escape``
    the sync holes hold zeros on the host and are unset on a GPU."""
    voc = _vocab(kind, vocabulary)
    p = plan(kind, seed, m, first, target, params, device, pos, last_sync, voc, max_bytes, stream)
    with _lib.stream_ctx(stream, device):
        data = torch.empty(p.total, dtype=torch.uint8, device=device) if _lib.is_cuda(device) else \
            torch.zeros(p.total, dtype=torch.uint8)
    fill(kind, seed, m, first, p.index, data, params, voc, stream)
    if escape is not None:
        fill_syncs(data, p.gaps, escape, stream)
    return data, p


def generate_cpu(kind, seed, m, bytes_per_map, params, vocabulary=None, pos=0, last_sync=0,
                 escape=None):
    """(data, index) of the whole map ``m`` by the twin: host tensors."""
    data, p = generate(kind, seed, m, 0, bytes_per_map, params, "cpu", pos, last_sync, vocabulary,
                       None, escape)
    return data, p.index
