"""K-Means map/combine/reduce ops on MI355X (entry points in native/kernels/kmeans.hip,
HIP kernels in its sections native/kernels/kmeans/*.h).

Data layout contract (built by :class:`hbmr.gpu.split_cache.SplitCache`):

* points: ``bf16 [n, dp]`` with ``dp`` in {64, 128, 256} (feature dim zero-padded),
* centroids: fp32 master copy ``[k, d]`` plus a bf16 image ``[k_pad, dp]`` and
  ``chalf = -||c||²/2`` (fp32, ``[k_pad]``); padded clusters carry -1e30 so they
  never win the arg-max,
* partial sums: **int64 fixed point** ``[k, dp]`` (``Σ round(x·2^fx_shift)``) and
  int64 counts ``[k]`` — exact and order-independent, so K-Means results are
  bitwise reproducible for any placement of map tasks over CPUs/GPUs and any
  GPU count (integer RCCL all-reduce is exact too).

Host plumbing every arm shares: ``_on`` (stream context), ``scratch_buf``
(buffers grown on demand, also used by hbmr.models.kmeans), ``_check_rows`` /
``_check_stats`` (argument checks) and ``order_after`` (the cross-stream rule
of the reference partitions).  Exact mode's batch is ``_RefineBatch``: the
per-call constants and the ctypes tables over a group's splits, built once.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading

import torch

from . import _lib
from ._lib import ptr
from ..utils.trace import TRACE

SUPPORTED_DP = (64, 128, 256)
FX_SHIFT = 24  # fixed-point fraction bits of the partial sums
# exact mode's Elkan scan: neighbours listed per centroid (past them the scan
# checks every centroid); HBMR_KMEANS_NBR_L overrides
NBR_L = 256


def padded_dim(d: int) -> int:
    for dp in SUPPORTED_DP:
        if d <= dp:
            return dp
    raise ValueError(f"feature dim {d} > {SUPPORTED_DP[-1]} not supported by the MFMA kernel")


def padded_k(k: int) -> int:
    return ((k + 63) // 64) * 64


def _on(stream):
    """``torch.cuda.stream(stream)``; nothing for None (the caller's current stream)."""
    return contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)


def scratch_buf(scratch: dict, key, n: int, dtype, device, floor: int = 0) -> torch.Tensor:
    """``scratch[key]``: a flat buffer of at least ``n`` elements, kept across
    calls and replaced (by one of ``max(n, floor)``) only when it is too small.
    It may be longer than asked for: the kernels take pointers and counts."""
    buf = scratch.get(key)
    if buf is None or buf.numel() < n:
        buf = scratch[key] = torch.empty(max(n, floor), dtype=dtype, device=device)
    return buf


def _top3_scratch(scratch: dict, kind: str, n: int, device):
    """The top-3 assign's (cand [2n], scores [n], margin [2n]) of ``kind``."""
    return (scratch_buf(scratch, (kind, "cand"), 2 * n, torch.int32, device)[:2 * n],
            scratch_buf(scratch, (kind, "scores"), n, torch.float32, device)[:n],
            scratch_buf(scratch, (kind, "margin"), 2 * n, torch.float32, device)[:2 * n])


def _check_rows(xs, dp: int, dtypes=None) -> None:
    """Every x: contiguous ``[n, dp]`` rows, all of one dtype (among ``dtypes``)."""
    dt = xs[0].dtype
    if (dtypes is not None and dt not in dtypes) or \
            any(x.dtype != dt or x.shape[1] != dp or not x.is_contiguous() for x in xs):
        raise ValueError(f"splits must be contiguous [n, {dp}] rows of one type ({dtypes})")


def _check_stats(stats: torch.Tensor) -> None:
    if stats.dtype != torch.int64 or stats.numel() < 3:
        raise ValueError("stats must be int64 [3]")


def new_partials(k: int, dp: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    return (torch.zeros(k, dp, dtype=torch.int64, device=device),
            torch.zeros(k, dtype=torch.int64, device=device))


def partials_to_float(sums: torch.Tensor, counts: torch.Tensor, d: int | None = None,
                      fx_shift: int = FX_SHIFT):
    s = sums.to(torch.float64) / float(1 << fx_shift)
    if d is not None:
        s = s[:, :d]
    return s, counts.to(torch.float64)


def _build_image16(img: "CentroidImage", dtype):
    """(c16, chalf, |c|, max |c|, |c - c~|, max, tiled c16 or None) of ``img``
    on the current stream (hbmr_kmeans_image16, hbmr_kmeans_image16_tiled)."""
    dev = img.cen.device
    c16 = torch.empty(img.k_pad, img.dp, dtype=dtype, device=dev)
    ch = torch.empty(img.k_pad, dtype=torch.float32, device=dev)
    cn = torch.empty(img.k, dtype=torch.float32, device=dev)
    ce = torch.empty(img.k, dtype=torch.float32, device=dev)
    mx = torch.empty(2, dtype=torch.float32, device=dev)
    rc = _lib.load().hbmr_kmeans_image16(
        ptr(img.cen), img.k, img.d, img.dp, img.k_pad, int(dtype == torch.float16), ptr(c16),
        ptr(ch), ptr(cn), ptr(ce), ptr(mx), _lib.stream_handle(None))
    _lib.check(rc, "hbmr_kmeans_image16")
    c16t = None
    if img.dp in (64, 128):
        # the v3 fused assign's tiled copy (hbmr_kmeans_image16_tiled)
        c16t = torch.empty_like(c16)
        rc = _lib.load().hbmr_kmeans_image16_tiled(ptr(c16), img.k_pad, img.dp, ptr(c16t),
                                                   _lib.stream_handle(None))
        _lib.check(rc, "hbmr_kmeans_image16_tiled")
    return c16, ch, cn, mx[0:1], ce, mx[1:2], c16t


def _neighbors_native(img: "CentroidImage", L: int):
    """(indices [k, L], distances [k, L], L, pair distances or None) in one
    kernel (hbmr_kmeans_centroid_nbr): pairwise fp64 distances, bounds rounded
    outward, per-row bitonic sort in LDS — instead of ~40 small torch launches
    whose host time held the interpreter lock at the iteration seam."""
    dev = img.cen.device
    di = torch.empty(img.k, L, dtype=torch.int32, device=dev)
    f = torch.empty(img.k, L, dtype=torch.float32, device=dev)
    pd = torch.empty(img.k, img.k, dtype=torch.float32, device=dev) \
        if img.k <= PAIR_DIST_MAX_K else None
    rc = _lib.load().hbmr_kmeans_centroid_nbr(ptr(img.cen), img.k, img.d, L, ptr(di), ptr(f),
                                              ptr(pd), _lib.stream_handle(None))
    _lib.check(rc, "hbmr_kmeans_centroid_nbr")
    return di, f, L, pd


def _neighbors_torch(img: "CentroidImage", L: int):
    """The same table where the native kernel does not apply: squared
    distances by the Gram form in fp64 (one DGEMM instead of a pairwise
    kernel: ~0.8 ms per image at k = 1024), with the form's rounding error
    bounded explicitly: |D2 - D| <= (d + 4) 2^-53 (|a|^2 + |b|^2) for fp32
    inputs, so the lower bounds (Elkan's scan order and stop rule) and upper
    bounds (the pair rule) stay rigorous."""
    c = img.cen.double()
    n2 = (c * c).sum(1)
    nsum = n2[:, None] + n2[None, :]
    d2 = torch.addmm(nsum, c, c.T, beta=1.0, alpha=-2.0)
    err = nsum * ((img.d + 4) * 2.0 ** -53 * 1.01)
    lo = (d2 - err).clamp_(min=0.0).sqrt_()
    lo.fill_diagonal_(0.0)
    dv, di = lo.sort(dim=1, stable=True)
    dv, di = dv[:, :L].contiguous(), di[:, :L].to(torch.int32).contiguous()
    f = dv.float()
    f = torch.where(f.double() > dv, torch.nextafter(f, torch.full_like(f, -1.0)), f)
    # the full matrix of upper bounds rounded UP (the pair rule of the
    # certification's step 1); k <= PAIR_DIST_MAX_K
    pd = None
    if img.k <= PAIR_DIST_MAX_K:
        hi = (d2 + err).clamp_(min=0.0).sqrt_()
        hi.fill_diagonal_(0.0)
        pd = _f32_up(hi).contiguous()
    return di, f.contiguous(), L, pd


class CentroidImage:
    """Device-resident centroids in the layout the assign kernel consumes."""

    def __init__(self, centroids: torch.Tensor, device, fx_shift: int = FX_SHIFT):
        c = centroids.detach().to(device=device, dtype=torch.float32).contiguous()
        self.k, self.d = c.shape
        self.dp = padded_dim(self.d)
        self.k_pad = padded_k(self.k)
        self.fx_shift = fx_shift
        self.device = c.device
        self.cen = c
        self.cbf = torch.zeros(self.k_pad, self.dp, dtype=torch.bfloat16, device=device)
        self.chalf = torch.empty(self.k_pad, dtype=torch.float32, device=device)
        self.shift2 = torch.zeros(self.k, dtype=torch.float32, device=device)
        self._lock = threading.Lock()
        self.refresh()

    def successor(self, sums, counts) -> "CentroidImage":
        """The next iteration's image, on the current stream: private copies of
        this one's buffers, updated from the reduced ``sums`` / ``counts``
        (``refresh``).  This image stays as it is; the new one has its own
        empty 16-bit image / neighbour caches and nothing else of this one's."""
        img = CentroidImage.__new__(CentroidImage)
        img.k, img.d, img.dp, img.k_pad = self.k, self.d, self.dp, self.k_pad
        img.fx_shift, img.device = self.fx_shift, self.device
        img.cen = self.cen.clone()
        img.cbf = self.cbf.clone()
        img.chalf = self.chalf.clone()
        img.shift2 = torch.zeros_like(self.shift2)
        img._lock = threading.Lock()
        img.refresh(sums, counts)
        return img

    def refresh(self, sums=None, counts=None, stream=None):
        """Reduce-side update: c = sums/counts (clusters with count 0 keep their
        centroid), then rebuild the bf16 image and -||c||²/2."""
        lib = _lib.load()
        rc = lib.hbmr_kmeans_update(ptr(sums), ptr(counts), self.fx_shift, self.k, self.d,
                                    self.dp, self.k_pad, ptr(self.cen), ptr(self.cbf),
                                    ptr(self.chalf), ptr(self.shift2),
                                    _lib.stream_handle(stream))
        _lib.check(rc, "hbmr_kmeans_update")
        self._img16 = {}       # exact mode's 16-bit images and neighbour table: on demand
        self._nbr = {}

    def _once(self, cache: dict, key, build):
        """``cache[key]``, built once per image by ``build()`` on the first
        caller's stream; every caller's current stream waits for that build."""
        with self._lock:
            ent = cache.get(key)
            if ent is None:
                vals = build()
                ev = torch.cuda.Event()
                ev.record()
                ent = cache[key] = (ev, vals)
        torch.cuda.current_stream().wait_event(ent[0])
        return ent[1]

    def set_centroids(self, centroids: torch.Tensor, stream=None):
        self.cen.copy_(centroids.to(self.cen.device, torch.float32))
        self.refresh(stream=stream)

    def image16(self, dtype=torch.float16):
        """Exact mode's 16-bit centroid image for MFMA operands of ``dtype``
        (fp16, the default, or bf16): (c16 [k_pad, dp], chalf [k_pad] =
        -|c~|²/2, |c_j| [k], max |c_j| [1], |c_j - c~_j| [k], max [1]) — norms
        and rounding errors in fp64 rounded up (hbmr_kmeans_image16), built
        once per image on the first caller's stream; other streams wait."""
        return self._once(self._img16, dtype, lambda: _build_image16(self, dtype))[:6]

    def image16_tiled(self, dtype=torch.float16):
        """The tiled copy of ``image16(dtype)[0]`` (32-row tiles, 16-byte pieces
        piece-major) the v3 fused assign stages lane-linearly, or None (dp > 128)."""
        self.image16(dtype)
        return self._img16[dtype][1][6]

    def norms(self, dtype=torch.float16):
        """(|c_j| [k], max_j |c_j| [1], |c_j - c~_j| [k], max_j |c_j - c~_j| [1])
        for the 16-bit image of ``dtype`` (exact mode's certification bound)."""
        _, _, cn, cm, ce, cem = self.image16(dtype)
        return cn, cm, ce, cem

    def neighbors(self, L: int | None = None):
        """Each centroid's L nearest centroids (itself first) and their
        distances, fp64 rounded DOWN to fp32 — exact mode's Elkan scan.  Built
        once per image on the first caller's stream; other streams wait on it."""
        def build():
            n = int(os.environ.get("HBMR_KMEANS_NBR_L", NBR_L)) if L is None else L
            n = max(1, min(n, self.k))
            native = self.cen.is_cuda and self.k <= NBR_NATIVE_MAX_K and self.d <= 256
            return (_neighbors_native if native else _neighbors_torch)(self, n)
        return self._once(self._nbr, "table", build)[:3]

    def pair_dist(self):
        """|c_a - c_b| for every pair, fp64 rounded up to fp32 [k, k] (None past
        PAIR_DIST_MAX_K clusters): the certification's pair rule."""
        self.neighbors()
        return self._nbr["table"][1][3]

    def max_shift(self) -> float:
        return float(self.shift2.max().sqrt().item()) if self.k else 0.0


def assign(points: torch.Tensor, img: CentroidImage, labels: torch.Tensor | None = None,
           scores: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """labels[i] = argmin_j ||x_i - c_j||² (MFMA bf16 GEMM + fused arg-max)."""
    n, dp = points.shape
    if points.dtype != torch.bfloat16 or dp != img.dp or not points.is_contiguous():
        raise ValueError("points must be contiguous bf16 [n, dp] matching the centroid image")
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=points.device)
    lib = _lib.load()
    rc = lib.hbmr_kmeans_assign_bf16(ptr(points), n, dp, ptr(img.cbf), ptr(img.chalf),
                                     img.k_pad, ptr(labels), ptr(scores),
                                     _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_kmeans_assign_bf16")
    return labels


ACCUM_AUTO, ACCUM_LDS, ACCUM_SORTED = 0, 1, 2
_workspaces: dict = {}


def workspace_bytes(n: int, k: int) -> int:
    return int(_lib.load().hbmr_kmeans_accum_workspace_bytes(n, k))


def batch_scratch_sizes(ns: list, k: int) -> tuple[int, int]:
    """(label entries, workspace bytes) a map batch over splits of sizes ``ns`` needs
    (grouped kernels keep every split's labels/permutation side by side)."""
    lib = _lib.load()
    total = int(sum(ns))
    ws = max(int(lib.hbmr_kmeans_batch_workspace_bytes(total, len(ns), k)),
             int(lib.hbmr_kmeans_accum_workspace_bytes(max(ns), k)))
    return total, ws


def accum_workspace(n: int, k: int, device) -> torch.Tensor:
    """Per-(device, stream-free) scratch for the sorted combiner, grown on demand.

    Reused across calls on the same device; callers that run accumulations on
    several streams concurrently must pass their own ``workspace``."""
    key = torch.device(device)
    return scratch_buf(_workspaces, key, workspace_bytes(n, k), torch.uint8, key, floor=1 << 20)


def accumulate(points: torch.Tensor, labels: torch.Tensor, k: int, sums: torch.Tensor,
               counts: torch.Tensor, fx_shift: int = FX_SHIFT, stream=None,
               workspace: torch.Tensor | None = None, mode: int = ACCUM_AUTO) -> None:
    """sums[label] += round(x·2^fx_shift), counts[label] += 1 (int64 fixed point).

    Small k uses LDS-privatised accumulators; large k a counting sort of the
    labels followed by a segmented row sum (no atomics in the hot loop)."""
    n, dp = points.shape
    if sums.shape != (k, dp) or sums.dtype != torch.int64:
        raise ValueError(f"sums must be int64 [{k}, {dp}]")
    if counts.shape != (k,) or counts.dtype != torch.int64:
        raise ValueError(f"counts must be int64 [{k}]")
    if points.dtype not in (torch.bfloat16, torch.float32) or not points.is_contiguous() or \
            dp not in SUPPORTED_DP or labels.numel() < n:
        raise ValueError("points must be contiguous bf16/fp32 [n, dp] with n labels")
    lib = _lib.load()
    if workspace is None and mode != ACCUM_LDS:
        workspace = accum_workspace(n, k, points.device)
    fn, name = ((lib.hbmr_kmeans_accum_f32, "hbmr_kmeans_accum_f32")
                if points.dtype == torch.float32 else
                (lib.hbmr_kmeans_accum_bf16, "hbmr_kmeans_accum_bf16"))
    rc = fn(ptr(points), n, dp, ptr(labels), k, ptr(sums), ptr(counts), fx_shift,
            ptr(workspace), 0 if workspace is None else workspace.numel(), mode,
            _lib.stream_handle(stream))
    _lib.check(rc, name)


# --------------------------------------------------------------------------- exact mode
def _f32_up(v: torch.Tensor) -> torch.Tensor:
    """fp64 → fp32 rounded towards +inf (an upper bound stays an upper bound)."""
    f = v.float()
    return torch.where(f.double() < v, torch.nextafter(f, torch.full_like(f, float("inf"))), f)


class ExactSplit:
    """A split held for exact mode (``hbmr.kmeans.exact``): the 16-bit copy the
    MFMA assign reads (``xb``: fp16 by default — 11 significant bits, so the
    certification flags ~8x fewer points than with bf16's 8 — or bf16), the
    fp32 data (rows padded to dp) the certification re-score and the combiner
    read, and per point |x| (fp32 data), |x~|² (16-bit copy) and the rounding
    error |x - x~| (an upper bound), computed in fp64 once when the split is
    made resident (hbmr_kmeans_exact_prep)."""
    __slots__ = ("xb", "x32", "xnorm", "xbn2", "xerr", "d")

    def __init__(self, x32: torch.Tensor, dp: int, dtype=torch.float16):
        n, d = x32.shape
        self.d = d
        dev = x32.device
        if dp == d:
            self.x32 = x32.contiguous()
        else:
            self.x32 = torch.zeros(n, dp, dtype=torch.float32, device=dev)
            self.x32[:, :d] = x32
        if dev.type == "cuda":
            self.xb = torch.empty(n, dp, dtype=dtype, device=dev)
            self.xnorm = torch.empty(n, dtype=torch.float32, device=dev)
            self.xbn2 = torch.empty(n, dtype=torch.float32, device=dev)
            self.xerr = torch.empty(n, dtype=torch.float32, device=dev)
            rc = _lib.load().hbmr_kmeans_exact_prep(
                ptr(self.x32), n, dp, dp, dp, int(dtype == torch.float16), ptr(self.xb),
                ptr(self.xnorm), ptr(self.xbn2), ptr(self.xerr), _lib.stream_handle(None))
            _lib.check(rc, "hbmr_kmeans_exact_prep")
            return
        x64 = self.x32.double()
        self.xnorm = x64.norm(dim=1).float()
        lim = 65504.0 if dtype == torch.float16 else float("inf")
        xb = self.x32.clamp(-lim, lim).to(dtype)
        xb64 = xb.double()
        self.xbn2 = xb64.pow(2).sum(1).float()
        self.xerr = _f32_up((x64 - xb64).norm(dim=1))
        self.xb = xb.contiguous()

    @property
    def shape(self):
        return self.xb.shape

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.xb, self.x32, self.xnorm,
                                                          self.xbn2, self.xerr))


def assign_top3(points: torch.Tensor, img: CentroidImage, labels, cand, scores, margin,
                stream=None) -> None:
    """bf16 MFMA assign keeping the three best clusters: labels [n] (best),
    cand [2n] (second | third), scores [n] (best score), margin [2n]
    (best - second | best - third)."""
    n, dp = points.shape
    if points.dtype not in (torch.bfloat16, torch.float16) or dp != img.dp or \
            not points.is_contiguous():
        raise ValueError("points must be contiguous bf16/fp16 [n, dp] matching the image")
    for t, dt, m in ((labels, torch.int32, 1), (cand, torch.int32, 2), (scores, torch.float32, 1),
                     (margin, torch.float32, 2)):
        if t.numel() != m * n or t.dtype != dt or not t.is_contiguous():
            raise ValueError("top-3 outputs: labels/scores [n], cand/margin [2n]")
    with _on(stream):
        c16, ch = img.image16(points.dtype)[:2]
    fn = "hbmr_kmeans_assign_top3_f16" if points.dtype == torch.float16 else \
        "hbmr_kmeans_assign_top3_bf16"
    rc = getattr(_lib.load(), fn)(
        ptr(points), n, dp, ptr(c16), ptr(ch), img.k_pad, ptr(labels),
        ptr(cand), ptr(scores), ptr(margin), _lib.stream_handle(stream))
    _lib.check(rc, fn)


REFINE_VERSION = int(os.environ.get("HBMR_REFINE", "3"))
MAX_REFINE_BATCH = 64     # splits per refine v3 batch (the kernels' split table)
# the pair rule of the certification keeps a [k, k] centroid distance matrix
PAIR_DIST_MAX_K = int(os.environ.get("HBMR_PAIR_DIST_MAX_K", "8192"))
# the native neighbour table sorts a row of k keys in LDS (k <= 8192)
NBR_NATIVE_MAX_K = int(os.environ.get("HBMR_NBR_NATIVE_MAX_K", "8192"))
# exact batches: one top-3 launch + one step-1 launch per up to 64 splits
# (HBMR_EXACT_GROUPED=0: a launch of each per split)
GROUPED_EXACT = os.environ.get("HBMR_EXACT_GROUPED", "1") != "0"
# step 1 of the certification inside the grouped top-3 kernel's epilogue
# (HBMR_EXACT_FUSED_Q1=0: the separate step-1 scan over materialised arrays)
FUSED_Q1 = os.environ.get("HBMR_EXACT_FUSED_Q1", "1") != "0"


def _check_refine_dim(img: "CentroidImage") -> None:
    """Refine v3 reads the fp32 centroid rows ([k, d], row stride d) as 16-byte
    vectors (hbmr_kmeans_refine_batch_finish): refused here, before anything is
    launched.  HBMR_REFINE=1 or 2 selects the single-kernel form, which takes
    any d (it falls back to its scalar-load kernel where rows are not whole
    16-byte vectors)."""
    if REFINE_VERSION >= 3 and img.d % 8:
        raise ValueError(f"refine v3 needs d % 8 == 0 (d = {img.d}): HBMR_REFINE=2 takes any d")


class _RefineBatch:
    """Up to 64 splits of one exact call: its per-call constants, the ctypes
    tables over the splits (built once, here) and refine v3 over them —
    ``open`` before the first certification launch, ``q1`` right after each
    split's top-3 assign (its candidate scratch may be reused by the next
    split) or one grouped step 1 by the caller, ``finish`` once (step 2 +
    Elkan scan over the batch's queues)."""

    def __init__(self, splits: list, img: "CentroidImage", stats, scratch, stream,
                 c16=None, ch=None):
        _check_refine_dim(img)
        self.splits, self.img, self.stats, self.stream = splits, img, stats, stream
        self.scratch = {} if scratch is None else scratch
        self.c16, self.ch = c16, ch
        self.dt = splits[0].xb.dtype
        self.dev = splits[0].x32.device
        self.lib = _lib.load()
        self.st = _lib.stream_handle(stream)
        self.B = B = len(splits)
        self.sizes = [sp.shape[0] for sp in splits]
        self.N = sum(self.sizes)
        self.ns = (ctypes.c_long * B)(*self.sizes)
        P = ctypes.c_void_p * B
        self.xb, self.x32, self.xnorm, self.xbn2, self.xerr = (
            P(*[getattr(sp, a).data_ptr() for sp in splits])
            for a in ("xb", "x32", "xnorm", "xbn2", "xerr"))
        self.labels = [None] * B

    def open(self):
        """The queue workspace (kept in ``scratch`` across calls: one stream
        orders the reuse) and the image's norms / neighbour table / pair
        distances, waited for on the batch's stream."""
        need = int(self.lib.hbmr_kmeans_refine_batch_bytes(self.B, self.ns))
        if need < 0:
            raise ValueError("refine batch of 1..64 splits expected")
        self.ws = scratch_buf(self.scratch, "refine_ws", need, torch.uint8, self.dev)
        with _on(self.stream):
            self.norms = self.img.norms(self.dt)
            self.nbr = self.img.neighbors()
            self.pd = self.img.pair_dist()
        return self

    def labels_at(self, labels_ptr: int) -> None:
        """The splits' labels lie back to back from address ``labels_ptr``."""
        for i, n in enumerate(self.sizes):
            self.labels[i] = labels_ptr
            labels_ptr += 4 * n

    def q1(self, i, labels_ptr: int, cand, scores, margin):
        sp, img = self.splits[i], self.img
        cn, cmax, ce, cemax = self.norms
        self.labels[i] = labels_ptr
        rc = self.lib.hbmr_kmeans_refine_batch_q1(
            self.B, self.ns, i, img.d, img.k, img.k_pad, ptr(sp.xnorm),
            ptr(sp.xbn2), ptr(sp.xerr), ptr(cn), ptr(cmax), ptr(ce), ptr(cemax),
            labels_ptr, ptr(cand), ptr(scores), ptr(margin), ptr(self.stats),
            ptr(self.ws), self.ws.numel(), int(i == 0), ptr(self.pd), self.st)
        _lib.check(rc, "hbmr_kmeans_refine_batch_q1")

    def finish(self):
        img = self.img
        _, cmax, _, cemax = self.norms
        ni, nd, L = self.nbr
        ls = (ctypes.c_void_p * self.B)(*self.labels)
        rc = self.lib.hbmr_kmeans_refine_batch_finish(
            self.B, self.ns, self.x32, ls, img.d, self.splits[0].x32.shape[1], ptr(img.cen),
            img.k, img.k_pad, ptr(cmax), ptr(cemax), ptr(ni), ptr(nd), L, ptr(self.stats),
            self.stats.numel(), ptr(self.ws), self.ws.numel(), self.st)
        _lib.check(rc, "hbmr_kmeans_refine_batch_finish")


def _refine_single(lib, sp: ExactSplit, img: CentroidImage, norms, nbr, labels: int, cand: int,
                   scores: int, margin: int, stats: torch.Tensor, st: int) -> None:
    """The single-kernel refine (hbmr_kmeans_refine_f32) of one split;
    ``labels`` .. ``margin`` are device addresses."""
    cn, cmax, ce, cemax = norms
    ni, nd, L = nbr
    rc = lib.hbmr_kmeans_refine_f32(
        ptr(sp.x32), sp.shape[0], img.d, sp.x32.shape[1], ptr(sp.xnorm), ptr(sp.xbn2),
        ptr(sp.xerr), ptr(img.cen), img.k, img.k_pad, ptr(cn), ptr(cmax), ptr(ce), ptr(cemax),
        ptr(ni), ptr(nd), L, labels, cand, scores, margin, ptr(stats), stats.numel(), st)
    _lib.check(rc, "hbmr_kmeans_refine_f32")


def refine_f32(split: ExactSplit, img: CentroidImage, labels, cand, scores, margin,
               stats: torch.Tensor, stream=None, scratch: dict | None = None) -> None:
    """Certify the MFMA labels against the fp32 data; re-score the uncertain
    points in fp64 (refine v3, the queue pipeline; HBMR_REFINE=1 and 2 both mean
    the older single-kernel form, hbmr_kmeans_refine_f32, which picks its
    vector-load or scalar-load kernel by d and alignment).  stats (int64 [3]) +=
    (flagged, relabelled, points
    that needed the neighbour scan); a [5] stats also counts the scan's
    neighbour distances and its full scans."""
    n = split.shape[0]
    _check_stats(stats)
    if labels.numel() != n or cand.numel() != 2 * n or margin.numel() != 2 * n:
        raise ValueError("labels [n], cand/margin [2n] from assign_top3 expected")
    if REFINE_VERSION >= 3:
        rb = _RefineBatch([split], img, stats, scratch, stream).open()
        rb.q1(0, labels.data_ptr(), cand, scores, margin)
        rb.finish()
        return
    with _on(stream):
        norms = img.norms(split.xb.dtype)
        nbr = img.neighbors()
    _refine_single(_lib.load(), split, img, norms, nbr, ptr(labels), ptr(cand), ptr(scores),
                   ptr(margin), stats, _lib.stream_handle(stream))


def assign_exact(split: ExactSplit, img: CentroidImage, stats: torch.Tensor,
                 scratch: dict | None = None, stream=None) -> torch.Tensor:
    """Exact labels of the split's fp32 points: top-3 bf16 assign +
    certification / fp64 re-score.  Returns labels [n] (a scratch view)."""
    _check_refine_dim(img)
    n = split.shape[0]
    dev = split.xb.device
    scratch = {} if scratch is None else scratch
    # one set per split size: the labels are returned, and stay a split's own
    # until the next call over a split of the same size
    bufs = scratch.get(("exact", n))
    if bufs is None:
        bufs = scratch[("exact", n)] = tuple(
            torch.empty(m * n, dtype=t, device=dev)
            for m, t in ((1, torch.int32), (2, torch.int32), (1, torch.float32),
                         (2, torch.float32)))
    lab, cand, sc, mg = bufs
    assign_top3(split.xb, img, lab, cand, sc, mg, stream=stream)
    refine_f32(split, img, lab, cand, sc, mg, stats, stream=stream, scratch=scratch)
    return lab


def bounds_supported(img: CentroidImage) -> bool:
    """Whether ``assign_exact_batch(..., bounds=)`` can run for this image: the
    bounded pass is a form of the grouped, fused v3 assign (dp <= 128), so not
    where the v2 kernel is selected (hbmr_kmeans_set_exact_kernel(2) /
    HBMR_EXACT_V3=v2), which has no bounded form."""
    return REFINE_VERSION >= 3 and img.dp <= 128 and GROUPED_EXACT and FUSED_Q1 and \
        img.cen.is_cuda and _lib.load().hbmr_kmeans_get_exact_kernel() == 3


def assign_exact_batch(splits: list, img: CentroidImage, stats: torch.Tensor, out: torch.Tensor,
                       scratch: dict | None = None, stream=None, bounds: list | None = None,
                       skipped: torch.Tensor | None = None) -> None:
    """Exact labels of a batch of splits, written back to back into ``out``
    (int32 [sum n]): the top-3 assign and the step-1 certification per split
    (the candidate / score / margin scratch shared by every split: one stream
    orders the reuse), then step 2 and the neighbour scan once per up to 64
    splits (refine v3), with the centroid norms / neighbour lists fetched once
    and the labels written in place.

    ``bounds``: one ``Baseline`` per split (its reference partition).  A point
    whose stored ``gap`` — a certified lower bound of (distance to the nearest
    other centroid - distance to its own) against the centroids ``ref`` —
    exceeds what its own and the farthest-moving centroid moved since keeps
    its label without a single distance (hbmr_kmeans_assign_top3_q1_bounded);
    the labels are the same exact arg-min.  Every baseline leaves with ``gap``
    rewritten for the labels in ``out`` and the centroids of ``img``
    (``pending``), and with no ``ref``: the bounds count again once ``g`` has
    advanced to exactly these labels (``delta_combine(..., keep_bounds=True)``),
    and are lost if anything else happens to ``g`` first or this call raises.
    ``skipped`` (int64 [1], device) += the points not assigned."""
    if not splits:
        return
    _check_refine_dim(img)
    if bounds is not None and (len(bounds) != len(splits) or not bounds_supported(img)):
        raise ValueError("bounds: one baseline per split, grouped fused v3 assign (dp <= 128)")
    dev = splits[0].xb.device
    total = sum(sp.shape[0] for sp in splits)
    if out.dtype != torch.int32 or out.numel() < total or not out.is_contiguous():
        raise ValueError("out must be contiguous int32 with room for every split's labels")
    _check_stats(stats)
    dt = splits[0].xb.dtype
    _check_rows([sp.xb for sp in splits], img.dp, (torch.bfloat16, torch.float16))
    if not all(sp.x32.is_contiguous() for sp in splits):
        raise ValueError("exact splits must hold contiguous fp32 rows")
    scratch = {} if scratch is None else scratch
    cand, sc, mg = _top3_scratch(scratch, "exact-batch", max(sp.shape[0] for sp in splits), dev)
    grouped = REFINE_VERSION >= 3 and img.dp <= 128 and GROUPED_EXACT
    with _on(stream):
        c16, ch, *norms = img.image16(dt)
        # the neighbour table is waited for only where the certification
        # needs it (after the first top-3 launch: the reduce builds it on its
        # own stream while that assign runs)
        nbr = (None, None, 0) if grouped else img.neighbors()
        # the centroids the bounds will refer to: a private copy (the image's
        # buffers are refreshed in place), made in-stream, shared by the batch
        newref = None
        if bounds is not None:
            img.cen.record_stream(torch.cuda.current_stream())
            newref = img.cen.clone()
    lib = _lib.load()
    top3 = lib.hbmr_kmeans_assign_top3_f16 if dt == torch.float16 else \
        lib.hbmr_kmeans_assign_top3_bf16
    st = _lib.stream_handle(stream)
    pc, ps, pm = ptr(cand), ptr(sc), ptr(mg)
    base, off = out.data_ptr(), 0
    for g0 in range(0, len(splits), MAX_REFINE_BATCH):
        group = splits[g0:g0 + MAX_REFINE_BATCH]
        rb = _RefineBatch(group, img, stats, scratch, stream, c16, ch) \
            if REFINE_VERSION >= 3 else None
        if grouped:
            _exact_group(rb, base + 4 * off,
                         None if bounds is None else bounds[g0:g0 + MAX_REFINE_BATCH],
                         skipped, newref)
            off += rb.N
            continue
        if rb is not None:
            rb.open()
        for i, sp in enumerate(group):
            n = sp.shape[0]
            pl = base + 4 * off
            rc = top3(ptr(sp.xb), n, img.dp, ptr(c16), ptr(ch), img.k_pad, pl, pc, ps, pm, st)
            _lib.check(rc, "hbmr_kmeans_assign_top3")
            if rb is not None:
                rb.q1(i, pl, cand, sc, mg)
            else:
                _refine_single(lib, sp, img, norms, nbr, pl, pc, ps, pm, stats, st)
            off += n
        if rb is not None:
            rb.finish()


def order_after(bases: list, attrs: tuple, st) -> None:
    """Order a batch on stream ``st`` behind the baselines it reads.  Their
    tensors ``attrs`` may have been written (g, gap) / allocated (S0, N0, ref)
    on another stream — another slot's, or a reduce's: wait for the end of the
    batch that last updated each (``event``, where its ``stream`` is not
    ``st``), and keep the memory from being reused under this stream's pending
    reads — once per event and per allocation: the baselines of a batch share
    a few slabs, and an attribute that is None is skipped."""
    events, blocks = {}, {}
    for b in bases:
        if b.event is not None and b.stream is not None and b.stream != st:
            events[id(b.event)] = b.event
        for a in attrs:
            t = getattr(b, a)
            if t is not None:
                base = t._base if t._base is not None else t
                blocks[id(base)] = base
    for ev in events.values():
        st.wait_event(ev)
    for t in blocks.values():
        t.record_stream(st)


def _bounded_group(rb: _RefineBatch, bases, labels_ptr: int, skipped, newref):
    """The bounded form of the fused grouped assign (shift, sweep, assign over
    the lists): see ``assign_exact_batch``.  ``newref``: the batch's copy of
    ``img.cen``, which the rewritten bounds refer to (``Baseline.pending``)."""
    img, lib = rb.img, rb.lib
    cur = torch.cuda.current_stream() if rb.stream is None else rb.stream
    with torch.cuda.stream(cur):
        for b in bases:
            if b.gap is None:
                # an allocation of its own per split: it is charged to the
                # split's cache entry and has to go when that split is evicted
                b.gap, b.ref = torch.empty(b.g.numel(), dtype=torch.float32, device=rb.dev), None
        for b, n in zip(bases, rb.sizes):
            if b.g.numel() != n or b.gap.numel() != n or \
                    (b.ref is not None and (tuple(b.ref.shape) != tuple(img.cen.shape) or
                                            not b.ref.is_contiguous())):
                raise ValueError("bounds: baseline does not match its split / the centroids")
        order_after(bases, ("g", "gap", "ref"), cur)
        need = int(lib.hbmr_kmeans_bound_workspace_bytes(rb.N, rb.B, img.k))
        bws = scratch_buf(rb.scratch, "bound_ws", need, torch.uint8, rb.dev)
    P = ctypes.c_void_p * rb.B
    cn, cmax, ce, cemax = rb.norms
    # the gaps are rewritten for THIS batch's labels from here on: they bound
    # nothing about ``g`` until it has advanced to those labels
    # (Baseline.labels_advanced), and nothing at all if that never happens
    refs = [b.ref for b in bases]
    for b in bases:
        b.ref = b.pending = None
    rc = lib.hbmr_kmeans_assign_top3_q1_bounded(
        rb.B, rb.xb, rb.ns, img.dp, int(rb.dt == torch.float16), ptr(img.image16_tiled(rb.dt)),
        ptr(rb.ch), img.k_pad, labels_ptr, rb.xnorm, rb.xbn2, rb.xerr, img.d, img.k, ptr(cn),
        ptr(cmax), ptr(ce), ptr(cemax), ptr(rb.ws), rb.ws.numel(), ptr(rb.pd),
        P(*[b.g.data_ptr() for b in bases]), P(*[b.gap.data_ptr() for b in bases]),
        P(*[ptr(r) for r in refs]), ptr(img.cen), ptr(bws), bws.numel(), ptr(skipped), rb.st)
    _lib.check(rc, "hbmr_kmeans_assign_top3_q1_bounded")
    for b in bases:
        b.pending = newref


def _exact_group(rb: _RefineBatch, labels_ptr: int, bases=None, skipped=None, newref=None):
    """Top-3 assign and certification of up to 64 splits with grouped launches;
    labels of the group written back to back at ``labels_ptr``.  Step 1 runs
    in the top-3 kernel's epilogue (bounded: hbmr_kmeans_assign_top3_q1_bounded,
    or hbmr_kmeans_assign_top3_q1_grouped: no candidate / score / margin
    arrays), or as hbmr_kmeans_assign_top3_grouped + hbmr_kmeans_refine_batch_q1g."""
    img, lib, st = rb.img, rb.lib, rb.st
    f16 = int(rb.dt == torch.float16)
    fused = bases is not None or (FUSED_Q1 and img.dp <= 128)
    if not fused:
        # launched before the certification's inputs are waited for (``open``)
        cand, sc, mg = _top3_scratch(rb.scratch, "exact-group", rb.N, rb.dev)
        rc = lib.hbmr_kmeans_assign_top3_grouped(
            rb.B, rb.xb, rb.ns, img.dp, f16, ptr(rb.c16), ptr(rb.ch), img.k_pad, labels_ptr,
            ptr(cand), ptr(sc), ptr(mg), st)
        _lib.check(rc, "hbmr_kmeans_assign_top3_grouped")
    rb.open()
    cn, cmax, ce, cemax = rb.norms
    if fused and TRACE.on:
        TRACE.instant("kmeans.top3_launch", n=rb.B)
    if bases is not None:
        _bounded_group(rb, bases, labels_ptr, skipped, newref)
    elif fused:
        rc = lib.hbmr_kmeans_assign_top3_q1_grouped(
            rb.B, rb.xb, rb.ns, img.dp, f16, ptr(rb.c16), ptr(img.image16_tiled(rb.dt)),
            ptr(rb.ch), img.k_pad, labels_ptr, rb.xnorm, rb.xbn2, rb.xerr, img.d, img.k, ptr(cn),
            ptr(cmax), ptr(ce), ptr(cemax), ptr(rb.ws), rb.ws.numel(), ptr(rb.pd), st)
        _lib.check(rc, "hbmr_kmeans_assign_top3_q1_grouped")
    else:
        rc = lib.hbmr_kmeans_refine_batch_q1g(
            rb.B, rb.ns, img.d, img.k, img.k_pad, rb.xnorm, rb.xbn2, rb.xerr, ptr(cn), ptr(cmax),
            ptr(ce), ptr(cemax), labels_ptr, ptr(cand), ptr(sc), ptr(mg), ptr(rb.ws), rb.ws.numel(),
            ptr(rb.pd), st)
        _lib.check(rc, "hbmr_kmeans_refine_batch_q1g")
    rb.labels_at(labels_ptr)
    rb.finish()


def map_split_exact(split: ExactSplit, img: CentroidImage, sums, counts, scratch: dict,
                    stats: torch.Tensor, stream=None) -> torch.Tensor:
    """One exact-mode GPU map task: top-3 assign, certification + fp64 re-score,
    then the int64 fixed-point combiner over the fp32 rows.  Returns the
    labels (a view of ``scratch``, as ``assign_exact``'s)."""
    lab = assign_exact(split, img, stats, scratch, stream=stream)
    ws = scratch_buf(scratch, "ws", workspace_bytes(split.shape[0], img.k), torch.uint8,
                     split.xb.device, floor=1 << 20)
    accumulate(split.x32, lab, img.k, sums, counts, fx_shift=img.fx_shift, stream=stream,
               workspace=ws)
    return lab


def map_batch_gpu(splits: list, img: CentroidImage, sums: torch.Tensor, counts: torch.Tensor,
                  labels: torch.Tensor, workspace: torch.Tensor, stream=None,
                  zero_outputs: bool = True) -> None:
    """A batch of map tasks in one native call: splits[t] (bf16 [n_t, dp]) →
    sums[t] ([B, k, dp] int64), counts[t] ([B, k] int64)."""
    B = len(splits)
    if B == 0:
        return
    _check_rows(splits, img.dp, (torch.bfloat16,))
    if sums.shape != (B, img.k, img.dp) or counts.shape != (B, img.k):
        raise ValueError("batch output shape mismatch")
    need_lab, need_ws = batch_scratch_sizes([s.shape[0] for s in splits], img.k)
    if labels.numel() < need_lab:
        raise ValueError("labels scratch too small")
    lib = _lib.load()
    if workspace.numel() < need_ws:
        raise ValueError("workspace too small")
    ptrs = (ctypes.c_void_p * B)(*[s.data_ptr() for s in splits])
    ns = (ctypes.c_long * B)(*[s.shape[0] for s in splits])
    rc = lib.hbmr_kmeans_map_batch(B, ptrs, ns, img.dp, ptr(img.cbf), ptr(img.chalf), img.k_pad,
                                   img.k, ptr(labels), ptr(workspace), workspace.numel(),
                                   ptr(sums), ptr(counts), img.fx_shift, int(zero_outputs),
                                   _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_kmeans_map_batch")


# --------------------------------------------------------------------------- delta combiner
class Baseline:
    """Reference partition of one split for the delta combiner: labels ``g``
    (int32 [n]) and its exact partials ``S0`` (int64 [k, dp]), ``N0`` (int64
    [k]).  Invariant: S0[c] = Σ_{g(p)=c} fx(x_p), N0[c] = #{p: g(p)=c} — it
    holds for ANY g, so the map output computed against it is bit-identical to
    the direct combiner's; it only pays off when few points changed label.
    ``event`` marks the end of the batch that last updated it (its stream is
    ``stream``): a batch on another stream waits for it first.

    Exact mode's bounded assign (``assign_exact_batch(..., bounds=)``) adds
    ``gap`` (fp32 [n]): a certified lower bound of min_{j != g(p)} |x_p - c_j|
    - |x_p - c_g(p)| (distances over the fp32 data), 0 where none is known,
    against the centroids ``ref`` (fp32 [k, d], a private copy shared by the
    splits of a batch).  ``ref`` None: ``gap`` (if allocated) holds nothing and
    no point of the split can be skipped.

    The bounds mean something only for the labels they were written for, so
    they follow ``g``: a bounded assign rewrites ``gap`` for ITS labels, clears
    ``ref`` and leaves the centroids in ``pending``; whatever advances ``g``
    calls ``labels_advanced``, which makes ``pending`` the new ``ref`` only if
    ``g`` went to exactly those labels and otherwise drops the bounds."""
    __slots__ = ("g", "S0", "N0", "event", "stream", "data_ptr", "n", "gap", "ref", "pending")

    def __init__(self, g, S0, N0, data_ptr, n):
        self.g, self.S0, self.N0 = g, S0, N0
        self.gap = self.ref = self.pending = None
        self.event = None
        self.stream = None
        self.data_ptr, self.n = data_ptr, n

    def labels_advanced(self, bounded: bool = False) -> None:
        """``g`` now holds other labels.  ``bounded``: the ones the last
        bounded assign over this baseline wrote ``gap`` for."""
        self.ref = self.pending if bounded else None
        self.pending = None


def delta_workspace_bytes(total: int, ntasks: int, k: int) -> int:
    return int(_lib.load().hbmr_kmeans_delta_workspace_bytes(total, ntasks, k))


def _delta_args(xs, bases, stream):
    """The delta kernels' tables over a batch (rows, sizes, g, S0, N0), with
    the batch ordered behind its reference partitions (``order_after``)."""
    B = len(xs)
    order_after(bases, ("g", "S0", "N0"),
                torch.cuda.current_stream() if stream is None else stream)
    P = ctypes.c_void_p * B
    return (P(*[x.data_ptr() for x in xs]), (ctypes.c_long * B)(*[x.shape[0] for x in xs]),
            P(*[b.g.data_ptr() for b in bases]), P(*[b.S0.data_ptr() for b in bases]),
            P(*[b.N0.data_ptr() for b in bases]))


def map_batch_delta(splits: list, img: CentroidImage, sums: torch.Tensor, counts: torch.Tensor,
                    labels: torch.Tensor, workspace: torch.Tensor, bases: list,
                    stream=None) -> None:
    """A batch of map tasks against reference partitions (hbmr_kmeans_map_batch_delta):
    grouped MFMA assign, then the delta combiner.  sums/counts [B, k, dp] /
    [B, k] are overwritten; every ``bases[t]`` advances to this batch's labels."""
    B = len(splits)
    if B == 0:
        return
    if B > 64 or len(bases) != B:
        raise ValueError("at most 64 splits per delta batch, one baseline each")
    _check_rows(splits, img.dp, (torch.bfloat16,))
    for s, b in zip(splits, bases):
        if b.g.numel() != s.shape[0] or tuple(b.S0.shape) != (img.k, img.dp) or \
                b.N0.numel() != img.k:
            raise ValueError("baseline does not match its split")
    if sums.shape != (B, img.k, img.dp) or counts.shape != (B, img.k) or \
            not sums.is_contiguous() or not counts.is_contiguous():
        raise ValueError("batch output shape mismatch")
    total = sum(s.shape[0] for s in splits)
    if labels.numel() < total:
        raise ValueError("labels scratch too small")
    need = delta_workspace_bytes(total, B, img.k)
    if workspace.numel() < need:
        raise ValueError("workspace too small")
    ptrs, ns, gs, s0, n0 = _delta_args(splits, bases, stream)
    for b in bases:
        b.labels_advanced()           # exact mode's bounds, if any, were for other labels
    rc = _lib.load().hbmr_kmeans_map_batch_delta(
        B, ptrs, ns, img.dp, ptr(img.cbf), ptr(img.chalf), img.k_pad, img.k, ptr(labels),
        ptr(workspace), workspace.numel(), ptr(sums), ptr(counts), img.fx_shift, gs, s0, n0,
        _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_kmeans_map_batch_delta")


def delta_combine(xs: list, labels: torch.Tensor, k: int, sums: torch.Tensor,
                  counts: torch.Tensor, workspace: torch.Tensor, bases: list,
                  fx_shift: int = FX_SHIFT, stream=None, keep_bounds: bool = False) -> None:
    """The delta combiner alone over precomputed labels (concatenated in task
    order): rows are bf16 or fp32 (exact mode) ``[n_t, dp]``.  Every
    ``bases[t]`` advances to ``labels``, and loses its per-point bounds unless
    ``keep_bounds``: ``labels`` are then what a bounded ``assign_exact_batch``
    over the same baselines just wrote, and its bounds take effect."""
    B = len(xs)
    if B == 0:
        return
    # g is rewritten below: the bounds fall unless all of it succeeds
    pend = [b.pending for b in bases]
    for b in bases:
        b.labels_advanced()
    dp = xs[0].shape[1]
    _check_rows(xs, dp)
    if any(b.g.numel() != x.shape[0] for x, b in zip(xs, bases)):
        raise ValueError("delta_combine: rows/baselines mismatch")
    if B > 64 or dp not in SUPPORTED_DP or sums.shape != (B, k, dp) or counts.shape != (B, k):
        raise ValueError("delta_combine: shape mismatch")
    total = sum(x.shape[0] for x in xs)
    need = delta_workspace_bytes(total, B, k)
    if workspace.numel() < need or labels.numel() < total:
        raise ValueError("delta_combine: scratch too small")
    ptrs, ns, gs, s0, n0 = _delta_args(xs, bases, stream)
    rc = _lib.load().hbmr_kmeans_delta_combine(
        B, ptrs, ns, dp, int(xs[0].dtype == torch.float32), k, ptr(labels), ptr(workspace),
        workspace.numel(), ptr(sums), ptr(counts), fx_shift, gs, s0, n0,
        _lib.stream_handle(stream))
    _lib.check(rc, "hbmr_kmeans_delta_combine")
    if keep_bounds:
        for b, p in zip(bases, pend):
            b.ref = p


def map_split_gpu(points, img: CentroidImage, sums, counts, labels=None, stream=None):
    """One GPU K-Means map task over an HBM-resident split: assign + combine."""
    labels = assign(points, img, labels=labels, stream=stream)
    accumulate(points, labels, img.k, sums, counts, fx_shift=img.fx_shift, stream=stream)
    return labels


def map_split_cpu(points: torch.Tensor, centroids: torch.Tensor, sums: torch.Tensor,
                  counts: torch.Tensor, nthreads: int = 1, labels: torch.Tensor | None = None,
                  fx_shift: int = FX_SHIFT, exact: bool = False, stats: list | None = None):
    """CPU K-Means map task (native C++, fp32 math, int64 fixed-point partials).

    ``sums`` is int64 ``[k, d]`` (or ``[k, dp]``: only the first d columns are
    touched).  Returns the partial cost Σ min_j ||x - c_j||².  ``exact``: near
    ties (fp32 margin within the fp32 error bound) are re-scored in fp64;
    ``stats[0]`` += re-scored points.
    """
    x = points.detach().to(torch.float32).contiguous()
    c = centroids.detach().to(torch.float32).contiguous()
    n, d = x.shape
    k = c.shape[0]
    if counts.shape != (k,) or counts.dtype != torch.int64 or sums.dtype != torch.int64:
        raise ValueError("sums/counts must be int64")
    target = sums
    if sums.shape != (k, d):
        target = torch.zeros(k, d, dtype=torch.int64)
    cost = ctypes.c_double(0.0)
    lib = _lib.load()
    res = ctypes.c_long(0)
    rc = lib.hbmr_kmeans_map_cpu_f32_ex(ptr(x), n, d, ptr(c), k, ptr(labels), ptr(target),
                                        ptr(counts), ctypes.byref(cost), fx_shift, int(nthreads),
                                        int(exact), ctypes.byref(res))
    _lib.check(rc, "hbmr_kmeans_map_cpu_f32_ex")
    if stats is not None:
        stats[0] += res.value
    if target is not sums:
        sums[:, :d] += target
    return cost.value
