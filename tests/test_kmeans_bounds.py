"""Exact K-Means with per-point bounds (hbmr.kmeans.exact.bounds): the
reference partition of a split keeps a certified lower bound ``gap`` of
(distance to the nearest other centroid - distance to the point's own) against
the centroids ``ref``; a point whose bound outlasts the centroids' shift keeps
its label without a distance (hbmr_kmeans_assign_top3_q1_bounded: shift, sweep,
list-driven v3 assign).  Checked against fp64 distances of the fp32 data."""
import functools

import pytest
import torch

from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.jobconf import JobConf
from hbmr.models import kmeans as K

pytestmark = pytest.mark.gpu

SIZES = (1000, 256, 4097)          # one grouped call: < 1, exactly 1 and > 16 workgroups


def _dist(x32, c32):
    """|x - c_j| in fp64 from the differences (no Gram form: no cancellation)."""
    return torch.cdist(x32.double(), c32.double(),
                       compute_mode="donot_use_mm_for_euclid_dist")


def _truth(x32, c32):
    """(fp64 arg-min, second-smallest - smallest distance)."""
    two = _dist(x32, c32).topk(2, dim=1, largest=False, sorted=True)
    return two.indices[:, 0].to(torch.int32), two.values[:, 1] - two.values[:, 0]


def _splits(x, sizes, d):
    from hbmr.ops import kmeans as km
    out, o = [], 0
    for n in sizes:
        out.append(km.ExactSplit(x[o:o + n].contiguous(), km.padded_dim(d)))
        o += n
    return out


def _bases(sizes):
    from hbmr.ops import kmeans as km
    return [km.Baseline(torch.zeros(n, dtype=torch.int32, device="cuda"), None, None, 0, n)
            for n in sizes]


def _pass(sps, c, bases, scratch=None):
    """One bounded pass against centroids ``c``; the baselines' labels advance
    as the delta combiner advances them.  Returns (labels, flagged, skipped,
    list length per split)."""
    from hbmr.ops import kmeans as km
    img = c if isinstance(c, km.CentroidImage) else km.CentroidImage(c, "cuda")
    total = sum(sp.shape[0] for sp in sps)
    out = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = {} if scratch is None else scratch
    km.assign_exact_batch(sps, img, stats, out, scratch, bounds=bases, skipped=skipped)
    # the bounded workspace opens with the splits' list lengths (u32)
    cnt = scratch["bound_ws"][:4 * len(sps)].view(torch.int32).tolist()
    o = 0
    for b, sp in zip(bases, sps):
        # the rewritten bounds wait for the labels: none in force until then
        assert b.ref is None and b.pending is not None
        b.g.copy_(out[o:o + sp.shape[0]])
        b.labels_advanced(bounded=True)
        o += sp.shape[0]
    return out, int(stats[0]), int(skipped[0]), cnt


@functools.lru_cache(maxsize=None)
def _pool(k, d):
    """Points with k/2 true centers (duplicated blobs: near-ties), k centroids
    picked among them, the fp64 truth and a first bounded pass (no prior gaps);
    shared by the tests, never modified."""
    n = sum(SIZES)
    x = K.synthetic_points(3, 0, n, d, k // 2, "cuda")
    g = torch.Generator(device="cuda").manual_seed(k + d)
    c = x[torch.randperm(n, device="cuda", generator=g)[:k]].clone()
    sps = _splits(x, SIZES, d)
    bases = _bases(SIZES)
    lab, flagged, skipped, cnt = _pass(sps, c, bases)
    gap = torch.cat([b.gap for b in bases]).clone()
    return dict(x=x, c=c, lab=lab, flagged=flagged, skipped=skipped, cnt=cnt, gap=gap,
                truth=_truth(x, c))


def _carry(p, rows, c_ref, gap=None):
    """A split of the pool's ``rows`` with the bounds the first pass left."""
    from hbmr.ops import kmeans as km
    d = p["x"].shape[1]
    sp = km.ExactSplit(p["x"][rows].contiguous(), km.padded_dim(d))
    b = km.Baseline(p["lab"][rows].clone(), None, None, 0, rows.numel())
    b.gap = (p["gap"][rows] if gap is None else gap).clone()
    b.ref = c_ref.clone()
    return sp, b


@pytest.mark.parametrize("k,d", [(64, 128), (96, 128), (64, 64), (96, 64)])
def test_fresh_bounds_are_sound(k, d):
    p = _pool(k, d)
    tl, tg = p["truth"]
    assert torch.equal(p["lab"], tl)
    assert p["cnt"] == list(SIZES) and p["skipped"] == 0      # no prior gaps: every row listed
    gap = p["gap"].double()
    assert bool((gap >= 0).all()) and bool((gap <= tg).all())
    # a certified point's bound is positive, a flagged point's is 0
    assert 0 < p["flagged"] < sum(SIZES)
    assert int((gap == 0).sum()) == p["flagged"]
    print(f"k={k} d={d}: flagged {p['flagged']}, median gap / truth "
          f"{(gap / tg.clamp(min=1e-30))[gap > 0].median().item():.3f}")


@pytest.mark.parametrize("k,d", [(64, 128), (96, 128), (64, 64), (96, 64)])
def test_skip_is_exact_and_bounds_decay(k, d):
    p = _pool(k, d)
    n = sum(SIZES)
    sps = _splits(p["x"], SIZES, d)
    bases, o = [], 0
    for sz in SIZES:
        bases.append(_carry(p, torch.arange(o, o + sz, device="cuda"), p["c"])[1])
        o += sz
    g = torch.Generator(device="cuda").manual_seed(1)
    c2 = p["c"] + 0.02 * torch.randn(p["c"].shape, device="cuda", generator=g)
    lab, _, skipped, cnt = _pass(sps, c2, bases)
    tl, tg = _truth(p["x"], c2)
    assert torch.equal(lab, tl)
    assert skipped == n - sum(cnt) and 0 < skipped < n
    gap = torch.cat([b.gap for b in bases]).double()
    assert bool((gap >= 0).all()) and bool((gap <= tg).all())
    assert all(torch.equal(b.ref, c2) for b in bases)
    print(f"k={k} d={d}: skipped {skipped} of {n}")


def test_list_lengths_at_the_workgroup_edges():
    """Empty list, every row listed, lists of exactly 256 and 257 rows (one
    workgroup / one more), and a split without bounds, in one grouped call."""
    from hbmr.ops import kmeans as km
    k, d = 64, 128
    p = _pool(k, d)
    pos = torch.nonzero(p["gap"] > 0).flatten()
    assert pos.numel() >= 2500
    sp0, b0 = _carry(p, pos[:700], p["c"])                     # zero shift: nothing listed

    def forced(rows, m):                                       # m rows lose their bound
        gp = p["gap"][rows].clone()
        gp[torch.randperm(rows.numel(), device="cuda")[:m]] = 0.0
        return _carry(p, rows, p["c"], gp)
    sp1, b1 = forced(pos[700:1300], 256)
    sp2, b2 = forced(pos[1300:2300], 257)
    rows3 = torch.arange(300, device="cuda")
    sp3 = km.ExactSplit(p["x"][rows3].contiguous(), km.padded_dim(d))
    b3 = _bases([300])[0]                                      # gap None
    sps, bases = [sp0, sp1, sp2, sp3], [b0, b1, b2, b3]
    lab, _, skipped, cnt = _pass(sps, p["c"], bases)
    assert cnt == [0, 256, 257, 300]
    assert skipped == 700 + 600 + 1000 + 300 - sum(cnt)
    want = torch.cat([p["truth"][0][r] for r in (pos[:700], pos[700:1300], pos[1300:2300], rows3)])
    assert torch.equal(lab, want)
    assert b3.gap is not None and bool((b3.gap.double() <= p["truth"][1][rows3]).all())
    # a shift larger than every gap: every row is listed
    c_far = p["c"] + (p["gap"].max() + 1.0)
    sp4, b4 = _carry(p, pos[:700], p["c"])
    lab, _, skipped, cnt = _pass([sp4], c_far, [b4])
    assert cnt == [700] and skipped == 0
    assert torch.equal(lab, _truth(p["x"][pos[:700]], c_far)[0])


def test_stale_reference_uses_the_shift_since_ref():
    """Bounds two centroid versions old: the shift is |c - ref|, not the last
    update's (here zero)."""
    k, d = 64, 128
    p = _pool(k, d)
    rows = torch.arange(sum(SIZES), device="cuda")
    sp, b = _carry(p, rows, p["c"])
    g = torch.Generator(device="cuda").manual_seed(2)
    c1 = p["c"] + 0.1 * torch.randn(p["c"].shape, device="cuda", generator=g)
    c2 = c1.clone()                                            # version 2 = version 1: no shift
    lab, _, skipped, cnt = _pass([sp], c2, [b])
    tl, tg = _truth(p["x"], c2)
    assert int((tl != p["lab"]).sum()) > 0                     # labels did change since ref
    assert torch.equal(lab, tl)
    assert 0 < skipped < rows.numel()
    assert bool((b.gap.double() <= tg).all())


def test_job_with_bounds_is_bit_identical():
    n, k, d, sp = 400000, 64, 128, 100000
    inp = f"synthetic:{n}:5"
    got = {}
    for on in (True, False):
        conf = JobConf()
        conf.set_boolean(K.EXACT_KEY, True)
        conf.set_boolean(K.BOUNDS_KEY, on)
        conf.set(K.NCENTERS_KEY, str(k // 2))
        with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
            drv = K.KMeansDriver(cl.submit_job, lambda rj: rj._impl.jip.result[0], conf=conf,
                                 k=k, d=d, inp=inp, split_points=sp)
            for _ in range(6):
                r = drv.step()
            got[on] = (drv.centroids().clone(),
                       r["counters"].get("KMEANS", "EXACT_BOUND_SKIPPED_POINTS"),
                       r["counters"].get("KMEANS", "EXACT_FLAGGED_POINTS"))
    assert torch.equal(got[True][0], got[False][0])
    print("skipped in iteration 6:", got[True][1], "of", n, "flagged", got[True][2])
    assert got[True][1] > 0 and not got[False][1]
    assert got[True][2] > 0 and got[False][2] > 0


def test_bounds_follow_the_labels():
    """The bounds hold for the labels they were written for and no others: a
    combiner pass that advances the baseline to other labels (a job without
    bounds, other centroids) drops them, a bounded pass's own take effect only
    once the combiner has advanced the baseline to ITS labels, and one whose
    labels never arrive leaves none."""
    from hbmr.ops import kmeans as km
    k, d = 64, 128
    p = _pool(k, d)
    n = sum(SIZES)
    sp, b = _carry(p, torch.arange(n, device="cuda"), p["c"])
    dp = sp.x32.shape[1]
    b.S0, b.N0 = km.new_partials(k, dp, "cuda")
    km.accumulate(sp.x32, b.g, k, b.S0, b.N0)
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(km.delta_workspace_bytes(n, 1, k), dtype=torch.uint8, device="cuda")
    scratch = {}
    img = km.CentroidImage(p["c"], "cuda")

    def combine(lab, keep):
        sums = torch.empty(1, k, dp, dtype=torch.int64, device="cuda")
        counts = torch.empty(1, k, dtype=torch.int64, device="cuda")
        km.delta_combine([sp.x32], lab, k, sums, counts, ws, [b], keep_bounds=keep)
        s, c = km.new_partials(k, dp, "cuda")
        km.accumulate(sp.x32, lab, k, s, c)
        assert torch.equal(b.g, lab) and torch.equal(sums[0], s) and torch.equal(counts[0], c)
        b.S0, b.N0 = sums[0], counts[0]

    def bounded():
        out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        skipped.zero_()
        km.assign_exact_batch([sp], img, stats, out, scratch, bounds=[b], skipped=skipped)
        assert b.ref is None and b.pending is not None
        assert torch.equal(out, p["truth"][0])
        return out, int(skipped[0])

    # a job without bounds over other centroids (every centroid renamed)
    c_y = p["c"].roll(1, 0).contiguous()
    lab_y = torch.empty(n, dtype=torch.int32, device="cuda")
    km.assign_exact_batch([sp], km.CentroidImage(c_y, "cuda"), stats, lab_y, scratch)
    assert torch.equal(lab_y, _truth(p["x"], c_y)[0])
    assert int((lab_y != p["lab"]).sum()) == n
    combine(lab_y, keep=False)
    assert b.ref is None and b.pending is None
    # back to the centroids the dropped bounds referred to: zero shift, yet
    # nothing may be skipped
    out, sk = bounded()
    assert sk == 0
    combine(out, keep=True)
    assert torch.equal(b.ref, p["c"]) and b.pending is None
    # now the bounds are in force: zero shift, every certified point skipped
    out, sk = bounded()
    assert sk == int((p["gap"] > 0).sum())
    # ... but this pass's labels never reach the baseline
    combine(lab_y, keep=False)
    assert b.ref is None and b.pending is None
    out, sk = bounded()
    assert sk == 0


def test_jobs_with_and_without_bounds_share_a_split():
    """Every exact job over a resident split shares its reference partition,
    whatever its conf: bounds on (ends at centroids C) -> bounds off with other
    centroids -> bounds on from C again must give what the first run gave."""
    from hbmr.models.kmeans import STORE
    n, k, d, sp = 200000, 64, 128, 100000
    inp = f"synthetic:{n}:6"

    def conf(on):
        c = JobConf()
        c.set_boolean(K.EXACT_KEY, True)
        c.set_boolean(K.BOUNDS_KEY, on)
        c.set(K.NCENTERS_KEY, str(k // 2))
        return c

    def skipped(r):
        return r["counters"].get("KMEANS", "EXACT_BOUND_SKIPPED_POINTS")

    with LocalCluster(conf(True), num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        def driver(on, run_id, start=None):
            drv = K.KMeansDriver(cl.submit_job, lambda rj: rj._impl.jip.result[0], conf=conf(on),
                                 k=k, d=d, inp=inp, split_points=sp, run_id=run_id)
            if start is not None:                  # as KMeansDriver.resume does
                drv.iteration = 1
                STORE.put_host(drv.key(1), start)
            return drv
        x = driver(True, "bounds-x")
        for _ in range(3):
            x.step()
        c3 = x.centroids().clone()
        r = x.step()
        c4 = x.centroids().clone()
        assert skipped(r) > 0                      # the splits carry live bounds against c3
        y = driver(False, "bounds-y", c3.roll(1, 0).contiguous())
        assert not skipped(y.step())
        z = driver(True, "bounds-z", c3.clone())
        r = z.step()
        assert torch.equal(z.centroids(), c4)
        assert not skipped(r)                      # y's labels carried no bounds
        r = z.step()
        assert skipped(r) > 0
