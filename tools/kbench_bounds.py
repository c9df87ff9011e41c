"""The bounded exact assign (hbmr_kmeans_assign_top3_q1_bounded: centroid
shift, bound sweep, list-driven v3 assign) timed alone at chosen skip shares,
beside the unbounded grouped call, on the bench's data: 12.5M points x 128-d,
k=1024, after a few Lloyd iterations.

A skip share s is imposed on the stored bounds before every repetition (outside
the timed region): a random s of each split's rows get a bound no shift can
reach, the others 0, and the reference centroids are the current ones.  "natural"
keeps the bounds a first pass left and moves the centroids by one Lloyd step.

This is a timing tool only.  With an imposed share the stored labels are not
the arg-min of the rows given the unreachable bound, so the labels those runs
leave in ``out`` are meaningless; only the "natural" runs compute real ones.

usage: python tools/kbench_bounds.py [--shares 0,0.5,0.85,0.97,natural] [--points N] [--reps R]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hbmr.models import kmeans as K  # noqa: E402
from hbmr.ops import kmeans as km  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=12_500_000)
    ap.add_argument("--split", type=int, default=781_250)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shares", default="0,0.5,0.85,0.97,natural")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, k, d = a.points, a.k, a.d
    dp = km.padded_dim(d)
    x32 = K.synthetic_points(7, 0, n, d, k, dev)
    img = km.CentroidImage(K.initial_centroids("synthetic:%d:7" % n, k, d), dev)
    splits = [km.ExactSplit(x32[s:s + a.split], dp, torch.float16) for s in range(0, n, a.split)]
    del x32
    ns = [sp.shape[0] for sp in splits]
    bases = [km.Baseline(torch.zeros(m, dtype=torch.int32, device=dev), None, None, 0, m)
             for m in ns]
    out = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = {}

    def lloyd_step(bounds):
        """One exact iteration; the baselines' labels advance as the combiner's do."""
        km.assign_exact_batch(splits, img, stats, out, scratch, bounds=bounds, skipped=skipped)
        sums, cnt = km.new_partials(k, dp, dev)
        o = 0
        for sp, b in zip(splits, bases):
            b.g.copy_(out[o:o + sp.shape[0]])
            b.labels_advanced(bounded=bounds is not None)
            km.accumulate(sp.x32, b.g, k, sums, cnt)
            o += sp.shape[0]
        img.refresh(sums, cnt)

    for _ in range(a.iters):
        lloyd_step(bases)
    torch.cuda.synchronize()

    def timed(fn, prep):
        ts = []
        for _ in range(a.reps + 1):
            prep()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        ts = sorted(ts[1:])
        return round(ts[len(ts) // 2], 3), round(ts[0], 3)

    med, best = timed(lambda: km.assign_exact_batch(splits, img, stats, out, scratch),
                      lambda: None)
    print(json.dumps({"mode": "unbounded", "exact_batch_ms": med, "best_ms": best}), flush=True)

    keep = [(b.gap.clone(), b.ref) for b in bases]
    prev = keep[0][1]
    for share in a.shares.split(","):
        if share == "natural":
            def prep():
                for b, (gp, rf) in zip(bases, keep):
                    b.gap.copy_(gp)
                    b.ref = rf
        else:
            s = float(share)
            masks = [torch.rand(m, device=dev) < s for m in ns]

            def prep():
                cur = img.cen.clone()
                for b, m in zip(bases, masks):
                    b.gap.copy_(m.float() * 3.0e38)
                    b.ref = cur
        skipped.zero_()
        med, best = timed(
            lambda: km.assign_exact_batch(splits, img, stats, out, scratch, bounds=bases,
                                          skipped=skipped), prep)
        cnt = scratch["bound_ws"][:4 * len(splits)].view(torch.int32).sum().item()
        print(json.dumps({"mode": "bounded", "share": share, "exact_batch_ms": med,
                          "best_ms": best, "listed": cnt, "skip_share": round(1 - cnt / n, 4),
                          "max_shift": round((img.cen - prev).norm(dim=1).max().item(), 4)
                          if share == "natural" else 0.0}), flush=True)


if __name__ == "__main__":
    main()
