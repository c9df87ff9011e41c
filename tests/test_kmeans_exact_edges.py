"""Exact K-Means at the edges: every implementation of the certified assign
(refine v1 / v2 / v3, the fused v2 and v3 epilogues, the unfused and ungrouped
batch paths, the bounded pass, the CPU slot) against the fp64 arg-min of the
fp32 data, on inputs that break the assumptions the bounds were derived under:
k < 3 (padded top-3 slots), k off the 64 padding, d off the 8-lane slices and
padded inside dp, dp = 256, every point flagged, a large common offset, fp16
subnormals and saturation, exact fp64 ties, empty and one-row splits, and more
than 64 splits in one batch.

Reference: pairwise squared distances from the DIFFERENCES in fp64 (the Gram
form cancels on offset data).  ``want`` is their arg-min (lowest index on
ties).  A point is fp64-inseparable if more than one centroid has
D_j <= D_min (1 + tol), tol = 2 (d + 2) 2^-53: the project's bound for one fp64
sum of d squared differences ((d + 2) 2^-53, see kmeans_centroid_nbr_kernel),
once for the kernel's summation order and once for the reference's.

Conditions on the inputs, asserted from the reference alone before any kernel
runs (``Case.conditions``): blobs / offset / scales / tiny / huge have no
inseparable point; in lattice / dups every tied set has bit-equal distances
(so "lowest index" is well defined); collapse may have inseparable points,
which are checked by distance instead of by index.

Shapes: the eight of ``SHAPES`` plus three of ``EXTRA_SHAPES`` — k = 2 and
k = 3 with d % 8 == 0 (refine v3 refuses d % 8 != 0 with a ValueError, so the
k < 3 shapes of ``SHAPES`` with d = 3 / 100 reach only v1 and the CPU slot) and
one d = 256 shape for the ungrouped dp = 256 batch branch.
"""
import functools

import pytest
import torch

from hbmr.ops import kmeans as km

FAMILIES = ("blobs", "offset", "collapse", "scales", "tiny", "huge", "lattice", "dups")
NO_TIES = ("blobs", "offset", "scales", "tiny", "huge")
EXACT_TIES = ("lattice", "dups")

# (n, d, k): k < 3, k < 8 tracks, k just past a 64 pad, k > NBR_L, d % 8 != 0,
# all three dp, n on both sides of the 256-point workgroup and of the
# 256 * kQ1Per * kQShards shard stride
SHAPES = ((1, 8, 1), (5, 3, 2), (257, 100, 3), (1000, 40, 37), (4099, 128, 96),
          (3000, 200, 70), (2000, 64, 300), (8193, 64, 65))
EXTRA_SHAPES = ((5, 8, 2), (300, 16, 3), (1500, 256, 70))
ALL_SHAPES = SHAPES + EXTRA_SHAPES
# 70 splits of 1-40 rows: two refine groups (MAX_REFINE_BATCH = 64)
SIZES70 = torch.randint(1, 41, (70,), generator=torch.Generator().manual_seed(70)).tolist()
SHAPE70 = (sum(SIZES70), 64, 65)
PLACEMENT_SHAPE = (4099, 128, 96)

BATCH_MODES = {"fused-v3": (3, True, True), "fused-v2": (2, True, True),
               "unfused": (3, True, False), "ungrouped": (3, False, False)}


def _sid(shape):
    return "x".join(str(v) for v in shape)


def _tol(d):
    return 2.0 * (d + 2) * 2.0 ** -53


def _sqdist(x32, c32):
    """|x - c_j|^2 in fp64 from the differences (no Gram form: no cancellation)."""
    return torch.cdist(x32.double(), c32.double(),
                       compute_mode="donot_use_mm_for_euclid_dist") ** 2


class Case:
    """Points, centroids and the fp64 reference of one (family, shape)."""

    def __init__(self, family, shape, x, c):
        self.family, self.shape, self.x, self.c = family, shape, x, c
        self.tol = _tol(shape[1])
        self.D = _sqdist(x, c)
        self.dmin = self.D.min(dim=1).values
        self.want = self.D.argmin(dim=1)
        # argmin's tie rule, spelled out: the lowest index that reaches the minimum
        hit = (self.D == self.dmin[:, None]).double()
        assert torch.equal(hit.argmax(dim=1), self.want)
        self.tied = self.D <= (self.dmin * (1.0 + self.tol))[:, None]
        self.insep = self.tied.sum(1) > 1

    def conditions(self):
        """What the assertions below rely on, from the reference alone."""
        if self.family in NO_TIES:
            assert int(self.insep.sum()) == 0, (self.family, self.shape, int(self.insep.sum()))
        elif self.family in EXACT_TIES:
            same = self.D == self.dmin[:, None]
            assert bool((same | ~self.tied).all()), (self.family, self.shape)
        return self


def _blobs(g, n, d, k):
    """k/2 true centres (10 N(0,1)) with unit noise: near-ties are common."""
    nc = max(1, k // 2)
    centres = 10.0 * torch.randn(nc, d, generator=g)
    which = torch.randint(nc, (n,), generator=g)
    return centres[which] + torch.randn(n, d, generator=g)


def _points(family, shape, seed):
    n, d, k = shape
    g = torch.Generator().manual_seed(seed)
    if family == "lattice":
        x = torch.randint(-3, 4, (n, d), generator=g).float()
    elif family == "collapse":
        # 1024 + delta, |delta| < 0.25: the fp16 (ulp 1 above, 0.5 below) and
        # bf16 (ulp 8 / 4) copies are identically 1024
        x = 1024.0 + 0.49 * (torch.rand(n, d, generator=g) - 0.5)
    else:
        x = _blobs(g, n, d, k)
        if family == "offset":
            x = 1000.0 + 0.01 * x
        elif family == "scales":
            x = x * torch.pow(2.0, torch.randint(-12, 13, (d,), generator=g).float())
        elif family == "tiny":
            x = x * 1e-6
        elif family == "huge":
            x = x * 3000.0
    c = x[torch.randperm(n, generator=g)[:k]].clone()
    if family == "dups":
        if k >= 4:
            c[3] = c[1]
        if k >= 2:
            c[k - 1] = c[0]
        for i, j in enumerate((0, 1 % k, 3 % k, k - 1, 2 % k)):
            if i < n:
                x[n - 1 - i] = c[j]
    return x.contiguous(), c.contiguous(), g


def _seed(family, shape):
    return 1000 * FAMILIES.index(family) + 7 * shape[0] + 3 * shape[1] + shape[2]


@functools.lru_cache(maxsize=None)
def _case(family, shape):
    x, c, _ = _points(family, shape, _seed(family, shape))
    assert c.shape == (shape[2], shape[1]) and x.shape == shape[:2]
    if family == "collapse":
        assert bool(((x - 1024.0).abs() < 0.25).all())
        for dt in (torch.float16, torch.bfloat16):
            assert bool((x.to(dt).float() == 1024.0).all())
    return Case(family, shape, x, c).conditions()


@functools.lru_cache(maxsize=None)
def _moved(family, shape):
    """The case's points against moved centroids (the bounded pass's second
    pass): + 0.02 N(0,1), the lattice by an integer step."""
    cs = _case(family, shape)
    g = torch.Generator().manual_seed(_seed(family, shape) + 1)
    if family == "lattice":
        c2 = cs.c + torch.randint(-1, 2, cs.c.shape, generator=g).float()
    else:
        c2 = cs.c + 0.02 * torch.randn(cs.c.shape, generator=g)
        if family == "collapse":                     # stay inside 1024 +- 0.25
            c2 = c2.clamp(1024.0 - 0.249, 1024.0 + 0.249)
            assert bool((c2.half().float() == 1024.0).all())
    return Case(family, shape, cs.x, c2.contiguous()).conditions()


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    """The cached cases (a few hundred MB of references) go with the module."""
    yield
    for f in (_case, _moved, _gpu):
        f.cache_clear()


def _check_labels(cs, got):
    n, d, k = cs.shape
    got = got.detach().cpu().long()
    assert got.shape == (n,)
    assert bool(((got >= 0) & (got < k)).all()), "labels outside [0, k)"
    dg = cs.D.gather(1, got[:, None])[:, 0]
    far = dg > cs.dmin * (1.0 + cs.tol)
    assert not bool(far.any()), (int(far.sum()), far.nonzero().flatten()[:8].tolist())
    sep = ~cs.insep
    bad = (got != cs.want) & sep
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
    if cs.family != "collapse":
        # no inseparable points (NO_TIES), or exact ties only: the lowest index
        bad = got != cs.want
        assert not bool(bad.any()), (int(bad.sum()), bad.nonzero().flatten()[:8].tolist(),
                                     got[bad][:8].tolist(), cs.want[bad][:8].tolist())


def _check_stats(cs, stats):
    n, _, k = cs.shape
    flagged, relabelled = int(stats[0]), int(stats[1])
    assert 0 <= relabelled <= flagged <= n, (relabelled, flagged, n)
    if cs.family == "collapse" and k >= 2:
        # every score is equal: a margin of 0 exceeds no bound
        assert flagged == n, (flagged, n)
    if k == 1:
        assert flagged == 0
    return flagged, relabelled


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("shape", ALL_SHAPES + (SHAPE70,), ids=_sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_inputs_meet_the_conditions(family, shape):
    cs = _case(family, shape)
    assert cs.D.shape == (shape[0], shape[2]) and bool(torch.isfinite(cs.D).all())
    if family in EXACT_TIES and shape[0] >= 1000:
        assert int(cs.insep.sum()) > 0              # the ties the family is for exist
    if shape[1] <= 128:
        _moved(family, shape)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_cpu_slot_exact_labels_and_partials(family, shape):
    cs = _case(family, shape)
    n, d, k = shape
    lab = torch.full((n + 7,), -1, dtype=torch.int32)
    sums = torch.zeros(k, d, dtype=torch.int64)
    counts = torch.zeros(k, dtype=torch.int64)
    km.map_split_cpu(cs.x, cs.c, sums, counts, nthreads=3, labels=lab, exact=True)
    assert int((lab[n:] != -1).sum()) == 0
    _check_labels(cs, lab[:n])
    got = lab[:n].long()
    assert torch.equal(counts, torch.bincount(got, minlength=k))
    q = torch.round(cs.x.double() * (1 << km.FX_SHIFT)).long()
    assert torch.equal(sums, torch.zeros(k, d, dtype=torch.int64).index_add_(0, got, q))


# ------------------------------------------------------------------------------ GPU
def _dt(name):
    return torch.float16 if name == "f16" else torch.bfloat16


@functools.lru_cache(maxsize=None)
def _gpu(family, shape):
    cs = _case(family, shape)
    return cs.x.cuda(), cs.c.cuda()


def _splits(xg, sizes, d, dt):
    out, o = [], 0
    for n in sizes:
        out.append(km.ExactSplit(xg[o:o + n].contiguous(), km.padded_dim(d), dt))
        o += n
    assert o == xg.shape[0]
    return out


def _edge_sizes(n):
    """[1, 255, 0, 256, 257, rest] (an empty split in the middle), cut to n rows."""
    out, left = [], n
    for s in (1, 255, 0, 256, 257):
        s = min(s, left)
        out.append(s)
        left -= s
    return out + [left]


def _call(fn, *args, **kw):
    """Skip only what the API itself refuses: refine v3 with d % 8 != 0."""
    try:
        return fn(*args, **kw)
    except ValueError as e:
        if "d % 8" not in str(e):
            raise
        pytest.skip(f"rejected by the API with ValueError: {e}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("version", [1, 2, 3])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_assign_exact_per_split(family, shape, version, dtype, monkeypatch):
    """refine v3, and v2 / v1 (the single-kernel forms: v1 wherever d % 8 != 0)."""
    monkeypatch.setattr(km, "REFINE_VERSION", version)
    cs = _case(family, shape)
    n, d, k = shape
    xg, cg = _gpu(family, shape)
    img = km.CentroidImage(cg, "cuda")
    sp = km.ExactSplit(xg, km.padded_dim(d), _dt(dtype))
    first = torch.empty(n, dtype=torch.int32, device="cuda")
    cand = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    sc, mg = torch.empty(n, device="cuda"), torch.empty(2 * n, device="cuda")
    km.assign_top3(sp.xb, img, first, cand, sc, mg)
    assert bool(((first >= 0) & (first < k)).all())
    # the labels land in a guarded buffer: nothing is written past them
    buf = torch.full((n + 7,), -1, dtype=torch.int32, device="cuda")
    scratch = {("exact", n): (buf[:n], torch.empty_like(cand), torch.empty_like(sc),
                              torch.empty_like(mg))}
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    lab = _call(km.assign_exact, sp, img, stats, scratch)
    torch.cuda.synchronize()
    assert lab.data_ptr() == buf.data_ptr() and int((buf[n:] != -1).sum()) == 0
    print(f"{family} {_sid(shape)} v{version} {dtype}: (flagged, relabelled, scanned, "
          f"neighbour distances, full scans) = {stats.tolist()}, "
          f"MFMA arg-max off the truth at {int((first.cpu().long() != cs.want).sum())} points")
    _check_labels(cs, lab)
    _, relabelled = _check_stats(cs, stats)
    assert relabelled == int((first != lab).sum())


def _batch(cs, xg, cg, sizes, dtype, mode):
    """assign_exact_batch over ``sizes`` in ``mode``: (labels [n], stats, the image)."""
    kern, grouped, fused = BATCH_MODES[mode]
    n, d, _ = cs.shape
    img = km.CentroidImage(cg, "cuda")
    sps = _splits(xg, sizes, d, _dt(dtype))
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    out = torch.full((n + 7,), -1, dtype=torch.int32, device="cuda")
    lib = km._lib.load()
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(km, "GROUPED_EXACT", grouped)
        mp.setattr(km, "FUSED_Q1", fused)
        lib.hbmr_kmeans_set_exact_kernel(kern)
        _call(km.assign_exact_batch, sps, img, stats, out, {})
        torch.cuda.synchronize()
    finally:
        lib.hbmr_kmeans_set_exact_kernel(-1)
        mp.undo()
    assert int((out[n:] != -1).sum()) == 0
    return out[:n], stats, img


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mode", list(BATCH_MODES))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_assign_exact_batch(family, shape, mode, dtype):
    """The batch paths (fused v3 / v2 epilogue, unfused, ungrouped; dp = 256 is
    always ungrouped) over splits of 1, 255, 0, 256, 257 rows and the rest."""
    cs = _case(family, shape)
    xg, cg = _gpu(family, shape)
    lab, stats, _ = _batch(cs, xg, cg, _edge_sizes(shape[0]), dtype, mode)
    _check_labels(cs, lab)
    _check_stats(cs, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mode", list(BATCH_MODES))
@pytest.mark.parametrize("family", FAMILIES)
def test_seventy_splits_equal_one_split(family, mode, dtype):
    """70 splits of 1-40 rows: two refine groups, the labels written across the
    seam; they equal the labels of the concatenated rows as one split."""
    cs = _case(family, SHAPE70)
    xg, cg = _gpu(family, SHAPE70)
    assert len(SIZES70) > km.MAX_REFINE_BATCH
    lab, stats, img = _batch(cs, xg, cg, SIZES70, dtype, mode)
    _check_labels(cs, lab)
    _check_stats(cs, stats)
    one = km.ExactSplit(xg, km.padded_dim(SHAPE70[1]), _dt(dtype))
    s1 = torch.zeros(5, dtype=torch.int64, device="cuda")
    want = km.assign_exact(one, img, s1)
    assert torch.equal(lab, want)


def _pass(sps, img, bases, total):
    """One bounded pass (the protocol of test_kmeans_bounds._pass): the
    baselines' labels advance as the delta combiner advances them.  Returns
    (labels, stats, skipped, list length per split)."""
    out = torch.full((total + 7,), -1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = {}
    _call(km.assign_exact_batch, sps, img, stats, out, scratch, bounds=bases, skipped=skipped)
    torch.cuda.synchronize()
    assert int((out[total:] != -1).sum()) == 0
    cnt = scratch["bound_ws"][:4 * len(sps)].view(torch.int32).tolist()
    o = 0
    for b, sp in zip(bases, sps):
        assert b.ref is None and b.pending is not None
        b.g.copy_(out[o:o + sp.shape[0]])
        b.labels_advanced(bounded=True)
        o += sp.shape[0]
    return out[:total], stats, int(skipped[0]), cnt


def _check_gap(cs, lab, gap, flagged):
    """0 <= gap <= (distance to the nearest other centroid) - (distance to the
    label's), fp64; 0 for at least the flagged points."""
    n, _, k = cs.shape
    lab = lab.detach().cpu().long()
    gap = gap.detach().cpu().double()
    assert gap.shape == (n,) and bool((gap >= 0).all()) and bool(torch.isfinite(gap).all())
    assert int((gap == 0).sum()) >= flagged
    if k == 1:
        assert bool((gap == 0).all())               # fewer than two clusters: no bound
        return
    dist = cs.D.sqrt()
    own = dist.gather(1, lab[:, None])[:, 0]
    other = dist.scatter(1, lab[:, None], float("inf")).min(dim=1).values
    over = gap > (other - own).clamp(min=0.0)
    assert not bool(over.any()), (int(over.sum()), over.nonzero().flatten()[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [s for s in ALL_SHAPES if s[1] <= 128], ids=_sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_bounded_passes(family, shape, dtype):
    """A first bounded pass over fresh baselines, then a second after the
    centroids moved (skips by the stored gaps), over the edge split sizes."""
    cs, cs2 = _case(family, shape), _moved(family, shape)
    n, d, k = shape
    xg, cg = _gpu(family, shape)
    img = km.CentroidImage(cg, "cuda")
    assert km.bounds_supported(img)
    sizes = _edge_sizes(n)
    sps = _splits(xg, sizes, d, _dt(dtype))
    bases = [km.Baseline(torch.zeros(m, dtype=torch.int32, device="cuda"), None, None, 0, m)
             for m in sizes]
    lab, stats, skipped, cnt = _pass(sps, img, bases, n)
    assert cnt == sizes and skipped == 0            # no prior gaps: every row listed
    _check_labels(cs, lab)
    flagged, _ = _check_stats(cs, stats)
    gap = torch.cat([b.gap for b in bases])
    _check_gap(cs, lab, gap, flagged)
    if cs.family == "collapse" and k >= 2:
        assert bool((gap == 0).all())
    c2 = cs2.c.cuda()
    lab2, stats2, skipped2, cnt2 = _pass(sps, km.CentroidImage(c2, "cuda"), bases, n)
    print(f"{family} {_sid(shape)} {dtype}: flagged {int(stats[0])} then {int(stats2[0])}, "
          f"skipped {skipped2} of {n}, median gap {gap.median().item():.3g}")
    assert all(0 <= a <= b for a, b in zip(cnt2, sizes))
    assert skipped2 == n - sum(cnt2)
    _check_labels(cs2, lab2)
    flagged2, _ = _check_stats(cs2, stats2)
    assert flagged2 <= sum(cnt2)
    _check_gap(cs2, lab2, torch.cat([b.gap for b in bases]), flagged2)
    assert all(torch.equal(b.ref, c2) for b in bases)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("family", ["offset", "lattice", "dups"])
def test_partials_do_not_depend_on_placement(family, dtype):
    """The GPU map task's fixed-point sums and counts are bit-equal to the CPU
    slot's (same labels, order-independent integer sums)."""
    cs = _case(family, PLACEMENT_SHAPE)
    n, d, k = PLACEMENT_SHAPE
    xg, cg = _gpu(family, PLACEMENT_SHAPE)
    img = km.CentroidImage(cg, "cuda")
    sp = km.ExactSplit(xg, km.padded_dim(d), _dt(dtype))
    sums, counts = km.new_partials(k, img.dp, "cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    km.map_split_exact(sp, img, sums, counts, {}, stats)
    torch.cuda.synchronize()
    csum = torch.zeros(k, d, dtype=torch.int64)
    ccnt = torch.zeros(k, dtype=torch.int64)
    km.map_split_cpu(cs.x, cs.c, csum, ccnt, nthreads=3, exact=True)
    assert torch.equal(counts.cpu(), ccnt)
    assert torch.equal(sums[:, :d].cpu(), csum) and int((sums[:, d:] != 0).sum()) == 0
