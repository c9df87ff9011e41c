"""Record join: the map-side join of sorted SequenceFile splits
(native/kernels/recjoin.hip) and its CPU twin — what CompositeRecordReader does
for ``inner|outer|override(tbl(...), tbl(...), ...)``, on splits in the form of
:mod:`hbmr.ops.recsort` (``data`` uint8[bytes], ``index`` int64[4, n]).

Per key, in compareBytes order of the key payload, the tuple joins emit the
cross product of the sources' value lists (the last source varies fastest);
the value of an output record is the serialized TupleWritable: a header that
depends only on the set of sources that have the key (:func:`tuple_headers`,
built from TupleWritable itself) followed by the written values' bytes, copied
from the source frames.  ``override`` emits the frames of the rightmost source
that has the key.

* :func:`join_records_cpu` — the pure-Python twin: the frames, one by one.
* :func:`group_heads`, :func:`rank_heads`, :func:`plan` — the device stages.
* :func:`join_chunks` — the output in tuple ranges of bounded size (a range may
  end inside the cross product of one key); :func:`join_blob` and
  :func:`write_join` lay the chunks out back to back / into a
  ``sequencefile.Writer`` through ``recsort.layout``.

On a GPU the native library must load (no silent fallback).
"""
from __future__ import annotations

import itertools
import struct

import numpy as np
import torch

from . import _lib
from . import recsort
from .recsort import FLEN, FOFF, KLEN, KOFF, _ptr, _rows

OPS = ("inner", "outer", "override")
MAX_SOURCES = 8
MAX_TUPLES = 1 << 62
CHUNK_BYTES_KEY = "hbmr.join.gpu.chunk.bytes"
CHUNK_BYTES_DEFAULT = 1 << 30
# tuples of one launch: indices of a chunk's pieces stay far below 2^31
_MAX_CHUNK_TUPLES = 1 << 26


class UnsortedInput(ValueError):
    """Source ``source``'s record ``record`` has a key below its predecessor's."""

    def __init__(self, source, record):
        super().__init__(f"source {source}: the key of record {record} is below its "
                         "predecessor's (a join needs sorted inputs)")
        self.source, self.record = source, record


def tuple_headers(value_classes):
    """The serialized TupleWritable up to its values for every written mask:
    list of 2^S byte strings (vint slot count, vlong mask, the slots' class
    names — an unwritten slot's as TupleWritable names it)."""
    from ..mapred.join.tuple import TupleWritable
    S = len(value_classes)
    out = []
    for mask in range(1 << S):
        vals = [value_classes[s]() if mask >> s & 1 else None for s in range(S)]
        body = sum(len(v.serialize()) for v in vals if v is not None)
        raw = TupleWritable(vals).serialize()
        out.append(raw[:len(raw) - body])
    return out


def set_two_level(on: bool) -> None:
    """Rank kernel: search the round keys first (default) or full compares over
    all heads — an A/B knob of tools/bench_join.py."""
    _lib.check(_lib.load().hbmr_recjoin_set_two_level(int(bool(on))), "hbmr_recjoin_set_two_level")


def _check_args(sources, op, headers):
    if op not in OPS:
        raise ValueError(f"join op {op!r}: one of {', '.join(OPS)}")
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError(f"1 to {MAX_SOURCES} join sources")
    if op != "override" and (headers is None or len(headers) != 1 << len(sources)):
        raise ValueError("tuple_headers of the sources' value classes required")


# --------------------------------------------------------------------------- CPU twin
def _groups_cpu(s, data, index):
    """[(key payload, first record, count)] of a sorted source."""
    keys = recsort.payloads(data, index)
    out = []
    for i, k in enumerate(keys):
        if i and k == keys[i - 1]:
            out[-1][2] += 1
            continue
        if i and k < keys[i - 1]:
            raise UnsortedInput(s, i)
        out.append([k, i, 1])
    return out


def plan_cpu(sources, op):
    """[(key, [(first, count) | None per source])] in key order — the keys the
    join emits — and their tuple counts."""
    S = len(sources)
    per_key = {}
    for s, (data, index) in enumerate(sources):
        for k, first, cnt in _groups_cpu(s, data, index):
            per_key.setdefault(k, [None] * S)[s] = (first, cnt)
    keys, counts = [], []
    for k in sorted(per_key):
        g = per_key[k]
        if op == "inner" and any(x is None for x in g):
            continue
        if op == "override":
            n = [x for x in g if x is not None][-1][1]
        else:
            n = 1
            for x in g:
                n *= x[1] if x is not None else 1
        if n > MAX_TUPLES:
            raise OverflowError(f"key {k[:32]!r}: {n} tuples (more than 2^62)")
        keys.append((k, g))
        counts.append(n)
    if sum(counts) > MAX_TUPLES:
        raise OverflowError(f"{sum(counts)} tuples (more than 2^62)")
    return keys, counts


def join_records_cpu(sources, op, headers=None):
    """The frames ``[recordLen][keyLen][key][value]`` of the join, in order (a
    generator; the plan is made, and its errors raised, at the first frame)."""
    _check_args(sources, op, headers)
    keys, _ = plan_cpu(sources, op)
    raws = [recsort._np(d).tobytes() for d, _ in sources]
    idx = [recsort._np(i) for _, i in sources]

    def frame(s, r):
        o = int(idx[s][FOFF, r])
        return raws[s][o:o + int(idx[s][FLEN, r])]

    def value(s, r):
        a = int(idx[s][KOFF, r] + idx[s][KLEN, r])
        return raws[s][a:int(idx[s][FOFF, r] + idx[s][FLEN, r])]

    for _, g in keys:
        have = [s for s, x in enumerate(g) if x is not None]
        if op == "override":
            s = have[-1]
            for r in range(g[s][0], g[s][0] + g[s][1]):
                yield frame(s, r)
            continue
        s0, r0 = have[0], g[have[0]][0]
        kser = raws[s0][int(idx[s0][FOFF, r0]) + 8:int(idx[s0][KOFF, r0] + idx[s0][KLEN, r0])]
        head = kser + headers[sum(1 << s for s in have)]
        lists = [range(x[0], x[0] + x[1]) if x is not None else (None,) for x in g]
        for combo in itertools.product(*lists):
            body = head + b"".join(value(s, r) for s, r in enumerate(combo) if r is not None)
            yield struct.pack(">ii", len(body), len(kser)) + body


# --------------------------------------------------------------------------- device stages
def _validate(data, index):
    foff, flen, koff, klen = _rows(index)
    n = int(koff.numel())
    if n >= 1 << 31:
        raise ValueError("at most 2^31 - 1 records per join source")
    nb = data.numel()
    if n and bool(((foff < 0) | (flen < 8) | (foff + flen > nb) | (koff < foff + 8) | (klen < 0) |
                   (koff + klen > foff + flen)).any()):
        raise ValueError("record index points outside the data")
    return foff, flen, koff, klen


def _heads(data, rows, stream):
    """(head int32[n], bad int32[1]) of the heads kernel, no host read."""
    foff, flen, koff, klen = rows
    n = int(koff.numel())
    head = torch.empty(n, dtype=torch.int32, device=data.device)
    bad = torch.empty(1, dtype=torch.int32, device=data.device)
    rc = _lib.load().hbmr_recjoin_heads(_ptr(data), _ptr(koff), _ptr(klen), n, _ptr(head),
                                        _ptr(bad), _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_recjoin_heads")
    return head, bad


def group_heads(data, index, stream=None, check=True):
    """(head int32[n], bad): head[i] = 1 where record i opens a group of equal
    keys; ``bad`` = the first record whose key is below its predecessor's, or
    None for sorted input."""
    rows = _validate(data, index) if check else _rows(index)
    with _lib.stream_ctx(stream):
        head, bad = _heads(data, rows, stream)
        b = int(bad.item())
    return head, (None if b == -1 else b)


def rank_heads(probe, target, stream=None, check=True, thk=None):
    """(lb int32[Gp], eq int32[Gp]) for ``probe`` = (data, index, head records
    int32[Gp]) against ``target`` = (data, index, head records int32[Gt], keys
    strictly ascending): the number of target heads whose key is below the probe
    head's, and whether target head ``lb`` has the same key.  ``thk``: the
    target heads' round keys 0, if the caller has them."""
    pdata, pindex, prec = probe
    tdata, tindex, trec = target
    if check:
        _validate(pdata, pindex)
        _validate(tdata, tindex)
        for rec, index in ((prec, pindex), (trec, tindex)):
            if rec.dtype != torch.int32:
                raise ValueError("head records int32 required")
            if rec.numel() and bool(((rec < 0) | (rec >= index.shape[1])).any()):
                raise ValueError("a head record lies outside its index")
    _, _, pkoff, pklen = _rows(pindex)
    _, _, tkoff, tklen = _rows(tindex)
    gp, gt = int(prec.numel()), int(trec.numel())
    with _lib.stream_ctx(stream):
        lb = torch.zeros(gp, dtype=torch.int32, device=pdata.device)
        eq = torch.zeros(gp, dtype=torch.int32, device=pdata.device)
        if gp == 0 or gt == 0:
            return lb, eq
        if thk is None:
            thk = recsort.round_keys_device(tdata, tindex, trec, 0, stream)
        rc = _lib.load().hbmr_recjoin_rank(_ptr(pdata), _ptr(pkoff), _ptr(pklen), _ptr(prec), gp,
                                           _ptr(tdata), _ptr(tkoff), _ptr(tklen), _ptr(trec),
                                           _ptr(thk), gt, _ptr(lb), _ptr(eq),
                                           _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_recjoin_rank")
    return lb, eq


class Plan:
    """The K keys a join emits, in key order (device tensors): ``base``
    int64[K + 1] the first tuple of each, ``mask`` int32[K] the sources that
    have it, ``first`` / ``cnt`` int32[S, K] its records in each source,
    ``osrc`` / ``orec`` int32[K] the record the key bytes are taken from
    (override: the source that is emitted)."""

    def __init__(self, sources, op, base, mask, first, cnt, osrc, orec, total):
        self.sources, self.op = sources, op
        self.base, self.mask, self.first, self.cnt = base, mask, first, cnt
        self.osrc, self.orec = osrc, orec
        self.total = total
        self.keys = int(mask.numel())


def plan(sources, op, stream=None, stats=None):
    """Stages 1-3 on the device: group heads, cross ranks, and the keys with
    their tuple counts.  Raises :class:`UnsortedInput` and, for more than 2^62
    tuples, OverflowError."""
    S = len(sources)
    dev = sources[0][0].device
    with _lib.stream_ctx(stream):
        rows = [_validate(d, i) for d, i in sources]
        gfirst, gcnt = [], []
        heads = [_heads(data, r, stream) for (data, _), r in zip(sources, rows)]
        for s, bad in enumerate(torch.cat([b for _, b in heads]).tolist()):   # one host read
            if bad != -1:
                raise UnsortedInput(s, bad)
        for head, _ in heads:
            f = torch.nonzero(head).flatten().to(torch.int32)
            n = int(head.numel())
            end = torch.cat([f[1:], torch.tensor([n], dtype=torch.int32, device=dev)]) if n else f
            gfirst.append(f)
            gcnt.append(end - f)
        hk = [recsort.round_keys_device(d, i, f, 0, stream) if f.numel() else None
              for (d, i), f in zip(sources, gfirst)]
        cols = []                        # per source, of its owners: pos, mask, first, cnt, orec
        for s in range(S):
            G = int(gfirst[s].numel())
            pos = torch.arange(G, dtype=torch.int64, device=dev)
            mask = torch.full((G,), 1 << s, dtype=torch.int32, device=dev)
            first = torch.zeros((S, G), dtype=torch.int32, device=dev)
            cnt = torch.zeros((S, G), dtype=torch.int32, device=dev)
            first[s], cnt[s] = gfirst[s], gcnt[s]
            own = torch.ones(G, dtype=torch.bool, device=dev)
            for t in range(S):
                if t == s or G == 0:
                    continue
                lb, eq = rank_heads((sources[s][0], sources[s][1], gfirst[s]),
                                    (sources[t][0], sources[t][1], gfirst[t]), stream, check=False,
                                    thk=hk[t])
                has = eq != 0
                pos += lb + (eq if t < s else 0)
                mask |= eq << t
                if gfirst[t].numel():
                    at = lb.long().clamp(max=int(gfirst[t].numel()) - 1)
                    first[t] = torch.where(has, gfirst[t][at], 0)
                    cnt[t] = torch.where(has, gcnt[t][at], 0)
                # the key's owner: the leftmost source that has it (override: the rightmost)
                if (t > s) if op == "override" else (t < s):
                    own &= ~has
            if op == "inner":
                own &= mask == (1 << S) - 1
            sel = torch.nonzero(own).flatten()
            cols.append((pos[sel], mask[sel], first[:, sel], cnt[:, sel],
                         torch.full((int(sel.numel()),), s, dtype=torch.int32, device=dev),
                         gfirst[s][sel]))
        pos = torch.cat([c[0] for c in cols])
        order = torch.argsort(pos)       # merged positions are distinct
        mask = torch.cat([c[1] for c in cols])[order].contiguous()
        first = torch.cat([c[2] for c in cols], dim=1)[:, order].contiguous()
        cnt = torch.cat([c[3] for c in cols], dim=1)[:, order].contiguous()
        osrc = torch.cat([c[4] for c in cols])[order].contiguous()
        orec = torch.cat([c[5] for c in cols])[order].contiguous()
        K = int(mask.numel())
        if op == "override":
            tuples = cnt.gather(0, osrc.long()[None, :])[0].long() if K else \
                torch.zeros(0, dtype=torch.int64, device=dev)
            approx = tuples.double()
        else:
            c1 = cnt.clamp(min=1)
            tuples = c1.long().prod(dim=0)
            approx = c1.double().prod(dim=0)
        base = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        torch.cumsum(tuples, 0, out=base[1:])
        total = 0
        if K:                            # one host read: the overflow checks and the total
            big, many, last = torch.stack([approx.max(), approx.sum(), base[-1].double()]).tolist()
            if big > MAX_TUPLES or many > MAX_TUPLES:
                raise OverflowError("the join has more than 2^62 tuples")
            total = int(base[-1].item()) if last >= 2.0 ** 52 else int(last)
    if stats is not None:
        stats.update(keys=K, tuples=total, groups=[int(g.numel()) for g in gfirst])
    p = Plan(sources, op, base, mask, first, cnt, osrc, orec, total)
    p.rows = rows
    return p


class _Emitter:
    """Stages 4-5 over a plan: tuple ranges → frame lengths → frames."""

    def __init__(self, p: Plan, headers, stream=None):
        self.p, self.stream = p, stream
        S = self.S = len(p.sources)
        dev = self.dev = p.base.device
        self.override = p.op == "override"
        hdrs = headers if not self.override else [b""] * (1 << S)
        lens = np.array([len(h) for h in hdrs], dtype=np.int32)
        offs = (np.cumsum(lens) - lens).astype(np.int32)
        blob = np.frombuffer(b"".join(hdrs) or b"\0", dtype=np.uint8).copy()
        self.hdr_len = torch.from_numpy(lens).to(dev)
        self.hdr_off = torch.from_numpy(offs).to(dev)
        self.hdr_bytes = torch.from_numpy(blob).to(dev)
        tab = []
        for (data, _), r in zip(p.sources, p.rows):
            tab += [data.data_ptr()] + [x.data_ptr() for x in r]
        self._rows = p.rows                                   # keeps the row tensors alive
        self.tab = torch.tensor(tab, dtype=torch.int64).to(dev)

    def key_bytes(self):
        """(bytes float64[K], bound float64[K]): each key's frame bytes and an
        upper bound of one of its frames — what the chunk cuts are made from."""
        p, S = self.p, self.S
        K = p.keys
        dev = self.dev
        lo = p.first.long()
        hi = lo + p.cnt.long()
        if self.override:
            total = torch.zeros(K, dtype=torch.float64, device=dev)
            bound = torch.zeros(K, dtype=torch.float64, device=dev)
            for s, (foff, flen, koff, klen) in enumerate(p.rows):
                if not flen.numel():
                    continue
                cum = torch.cat([flen.new_zeros(1), torch.cumsum(flen, 0)])
                mine = p.osrc == s
                total += torch.where(mine, (cum[hi[s]] - cum[lo[s]]).double(), 0.0)
                bound += torch.where(mine, float(flen.max()), 0.0)
            return total, bound
        tuples = (p.base[1:] - p.base[:-1]).double()
        fixed = torch.zeros(K, dtype=torch.float64, device=dev)
        for s, (foff, flen, koff, klen) in enumerate(p.rows):
            if foff.numel():
                at = p.orec.long().clamp(max=int(foff.numel()) - 1)
                fixed += torch.where(p.osrc == s, (koff + klen - foff)[at].double(), 0.0)
        fixed += self.hdr_len[p.mask.long()].double()
        total = tuples * fixed
        bound = fixed.clone()
        for s, (foff, flen, koff, klen) in enumerate(p.rows):
            if not foff.numel():
                continue
            vlen = foff + flen - koff - klen
            cum = torch.cat([vlen.new_zeros(1), torch.cumsum(vlen, 0)])
            c = p.cnt[s]
            total += tuples / c.clamp(min=1).double() * (cum[hi[s]] - cum[lo[s]]).double()
            bound += torch.where(c > 0, float(vlen.max()), 0.0)
        return total, bound

    def expand(self, lo, hi):
        """(tkey int32[T], trec int32[S, T], tlen int64[T]) of tuples [lo, hi)."""
        p, S, T = self.p, self.S, hi - lo
        if not 0 <= lo <= hi <= p.total or T > _MAX_CHUNK_TUPLES:
            raise ValueError(f"tuple range [{lo}, {hi}) of {p.total}")
        with _lib.stream_ctx(self.stream):
            tkey = torch.empty(T, dtype=torch.int32, device=self.dev)
            trec = torch.empty((S, T), dtype=torch.int32, device=self.dev)
            tlen = torch.empty(T, dtype=torch.int64, device=self.dev)
            rc = _lib.load().hbmr_recjoin_expand(
                _ptr(self.tab), S, _ptr(p.base), _ptr(p.mask), _ptr(p.first), _ptr(p.cnt),
                _ptr(p.osrc), _ptr(p.orec), p.keys, int(self.override), _ptr(self.hdr_len), lo, T,
                _ptr(tkey), _ptr(trec), _ptr(tlen), _lib.stream_handle(self.stream))
            _lib.check(rc, "hbmr_recjoin_expand")
        return tkey, trec, tlen

    def pieces(self, expanded, dst_off, out):
        """Writes the record and tuple headers of the expanded tuples' frames at
        ``dst_off`` (int64[T], device) into ``out`` and returns the pieces still
        to copy, S + 1 per tuple (the key, then a value per slot): (psrc
        addresses, plen, pdst offsets in ``out``), int64[T * (S + 1)] each."""
        p, S = self.p, self.S
        tkey, trec, tlen = expanded
        T = int(tkey.numel())
        with _lib.stream_ctx(self.stream):
            dst_off = dst_off.contiguous()
            if bool(((dst_off < 0) | (dst_off + tlen > out.numel())).any()):
                raise ValueError("join frames: a frame lies outside the output buffer")
            P = T * (S + 1)
            psrc = torch.empty(P, dtype=torch.int64, device=self.dev)
            plen = torch.empty(P, dtype=torch.int64, device=self.dev)
            pdst = torch.empty(P, dtype=torch.int64, device=self.dev)
            rc = _lib.load().hbmr_recjoin_frames(
                _ptr(self.tab), S, _ptr(p.mask), _ptr(p.osrc), _ptr(p.orec), int(self.override),
                _ptr(self.hdr_len), _ptr(self.hdr_off), _ptr(self.hdr_bytes), T, _ptr(tkey),
                _ptr(trec), _ptr(tlen), _ptr(dst_off), _ptr(out), _ptr(psrc), _ptr(plen),
                _ptr(pdst), _lib.stream_handle(self.stream))
            _lib.check(rc, "hbmr_recjoin_frames")
        return psrc, plen, pdst

    def copy(self, pieces, out):
        """The piece copy into ``out``: chunk table, then one launch."""
        psrc, plen, pdst = pieces
        with _lib.stream_ctx(self.stream):
            cbase, entry, total = recsort._chunk_table(pdst, plen, out, skip_empty=True)
            if total:
                rc = _lib.load().hbmr_recjoin_copy(_ptr(psrc), _ptr(plen), _ptr(pdst), _ptr(cbase),
                                                   _ptr(entry), total, _ptr(out),
                                                   _lib.stream_handle(self.stream))
                _lib.check(rc, "hbmr_recjoin_copy")

    def fill(self, expanded, dst_off, out_bytes, out=None):
        """uint8[out_bytes] with the expanded tuples' frames at ``dst_off``
        (int64[T], device); bytes no frame covers are left unset."""
        with _lib.stream_ctx(self.stream):
            if out is None:
                out = torch.empty(out_bytes, dtype=torch.uint8, device=self.dev)
            if expanded[0].numel():
                self.copy(self.pieces(expanded, dst_off, out), out)
        return out


def _cuts(em: _Emitter, chunk_bytes):
    """Tuple ranges [lo, hi) whose frames take at most about ``chunk_bytes``:
    whole keys while they fit, a key that alone does not fit cut inside."""
    p = em.p
    out = []
    if p.total == 0:
        return out
    with _lib.stream_ctx(em.stream):
        kbytes, bound = em.key_bytes()
        cum = torch.cat([kbytes.new_zeros(1), torch.cumsum(kbytes, 0)])
        budget = float(max(1, chunk_bytes))
        k, lo = 0, 0
        while lo < p.total:
            start, end = p.base[k:k + 2].tolist()
            if lo == start:
                # whole keys k .. k2 - 1 within the budget (and the launch limit)
                k2 = int(torch.searchsorted(cum, cum[k:k + 1] + budget, right=True).item()) - 1
                k2t = int(torch.searchsorted(p.base, p.base[k:k + 1] + _MAX_CHUNK_TUPLES,
                                             right=True).item()) - 1
                k2 = min(k2, k2t, p.keys)
                if k2 > k:
                    hi = int(p.base[k2].item())
                    out.append((lo, hi))
                    lo, k = hi, k2
                    continue
            per = int(min(_MAX_CHUNK_TUPLES, max(1.0, budget // max(1.0, float(bound[k].item())))))
            while lo < end:                  # the key alone exceeds the budget: cut inside
                hi = min(end, lo + per)
                out.append((lo, hi))
                lo = hi
            k += 1
    return out


class Chunk:
    """A tuple range of the join's output: ``flen`` (int64 numpy) its frame
    lengths, ``body(dst, total)`` the frames at offsets ``dst`` (int64 numpy)
    of a uint8 buffer of ``total`` bytes (a host numpy array)."""

    def __init__(self, flen, body):
        self.flen, self.body = flen, body


def _cpu_chunks(sources, op, headers, chunk_bytes):
    frames, size = [], 0
    for fr in join_records_cpu(sources, op, headers):
        if frames and size + len(fr) > chunk_bytes:
            yield _cpu_chunk(frames)
            frames, size = [], 0
        frames.append(fr)
        size += len(fr)
    if frames:
        yield _cpu_chunk(frames)


def _cpu_chunk(frames):
    def body(dst, total):
        out = np.zeros(total, dtype=np.uint8)
        for d, fr in zip(dst.tolist(), frames):
            out[d:d + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        return out
    return Chunk(np.array([len(f) for f in frames], dtype=np.int64), body)


def join_chunks(sources, op, headers=None, chunk_bytes=CHUNK_BYTES_DEFAULT, stream=None,
                stats=None):
    """The join of ``sources`` ([(data, index)], all on one device) as
    :class:`Chunk` s of at most ``chunk_bytes`` of frames each (one frame, if a
    frame alone is larger).  Host tensors take :func:`join_records_cpu`."""
    _check_args(sources, op, headers)
    if sources[0][0].device.type != "cuda":
        yield from _cpu_chunks(sources, op, headers, chunk_bytes)
        return
    p = plan(sources, op, stream, stats)
    em = _Emitter(p, headers, stream)
    for lo, hi in _cuts(em, chunk_bytes):
        ex = em.expand(lo, hi)

        def body(dst, total, ex=ex):
            with _lib.stream_ctx(stream):    # the copies to and from the host too
                dst_t = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to(em.dev)
                return em.fill(ex, dst_t, total).cpu().numpy()
        with _lib.stream_ctx(stream):
            flen = ex[2].cpu().numpy()
        yield Chunk(flen, body)


def join_blob(sources, op, headers=None, chunk_bytes=CHUNK_BYTES_DEFAULT, stream=None, lead=0):
    """(frame lengths int64 numpy, bytes): the join's frames back to back, each
    chunk's behind ``lead`` unset bytes of its buffer (the destination
    misalignment of its first frame)."""
    lens, parts = [], []
    for ch in join_chunks(sources, op, headers, chunk_bytes, stream):
        dst = lead + np.cumsum(ch.flen) - ch.flen
        total = lead + int(ch.flen.sum())
        parts.append(bytes(ch.body(dst, total)[lead:]))
        lens.append(ch.flen)
    return (np.concatenate(lens) if lens else np.empty(0, dtype=np.int64)), b"".join(parts)


def write_join(writer, sources, op, headers=None, chunk_bytes=CHUNK_BYTES_DEFAULT, stream=None):
    """Append the join's records to ``writer`` (a ``sequencefile.Writer``) chunk
    by chunk through the layout path.  Returns the number of records."""
    n = 0
    for ch in join_chunks(sources, op, headers, chunk_bytes, stream):
        dst, gaps, total = recsort.layout(ch.flen, writer.out.tell(), writer.last_sync_pos)
        writer.append_frames(ch.body(dst, total), gaps)
        n += int(ch.flen.size)
    return n
