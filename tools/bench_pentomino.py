"""GPU Pentomino on one MI355X: the exact-cover kernels of
native/kernels/exactcover.hip on 6×10 with the 12 pentominoes and on a board of
the 18 one-sided pentominoes, next to the C++ counter of
native/cpu/exactcover.cc on one core and on 16 threads, measured in the same
run; and ``pentomino -gpu`` end to end against the classic job.

Per board: the expansion depth A/B (whole ``count_gpu`` time for each number of
breadth-first levels), then with the best depth the time per level kernel
group, the count kernel's time and longest single launch, tree nodes
(placements made) per second, and the spread between the first and the last
workgroup of one count launch to finish (device clock, 100 MHz).  The CPU
yardstick counts the same prefixes on the 12-piece board; on the one-sided board
the whole problem is minutes of CPU time, so both sides also count one sample
of the frontier (every ``--sample``-th state two levels below the prefixes)
and the rates over that sample are what is compared.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.examples import dancing  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.ops import exactcover as E  # noqa: E402


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def run_count(tab, prefixes, levels, capacity):
    """One count_gpu with every kernel group timed by a synchronise before the
    next: (seconds, counts, placements, {(kind, level): [seconds, launches, states]},
    longest count launch)."""
    groups, last = {}, [None, 0.0]
    longest = [0.0]

    def close(now):
        if last[0] is not None:
            g = groups.setdefault(last[0][:2], [0.0, 0, 0])
            g[0] += now - last[1]
            g[1] += 1
            g[2] += last[0][2]
            if last[0][0] == "count":
                longest[0] = max(longest[0], now - last[1])

    def on_launch(kind, level, n):
        now = sync_time()
        close(now)
        last[0], last[1] = (kind, level, n), now

    stats = {}
    t0 = sync_time()
    counts = E.count_gpu(tab, prefixes, levels=levels, capacity=capacity, on_launch=on_launch,
                         stats=stats)
    t1 = sync_time()
    close(t1)
    return t1 - t0, counts.cpu(), stats["placements"], groups, longest[0]


def plain_count(tab, prefixes, levels, capacity, reps):
    """Best whole-call time of count_gpu without the per-group synchronises."""
    best = float("inf")
    for _ in range(reps + 1):                  # the first is the warm-up
        t0 = sync_time()
        counts = E.count_gpu(tab, prefixes, levels=levels, capacity=capacity)
        t1 = sync_time()
        best = min(best, t1 - t0)
    return best, counts.cpu()


def frontier(tab, prefixes, levels, capacity):
    """The first chunk of states ``levels`` below the prefixes, on the device."""
    words = torch.from_numpy(E.states(tab, prefixes).view("int64")).cuda()
    for _ in range(levels):
        words = next(iter(E.expand_gpu(tab, words, capacity)))
    return words


def wg_spread(tab, words, nprefixes):
    blocks = E.count_blocks(tab, int(words.shape[0]))
    clock = torch.zeros(2 * blocks, dtype=torch.int64, device="cuda")
    counts = torch.zeros(nprefixes, dtype=torch.int64, device="cuda")
    E.count_states_gpu(tab, words, counts, wg_clock=clock)
    c = clock.cpu().view(blocks, 2)
    start, ends = int(c[:, 0].min()), c[:, 1]
    return {"states": int(words.shape[0]), "workgroups": blocks,
            "first_done_ms": round((int(ends.min()) - start) / 1e5, 3),
            "last_done_ms": round((int(ends.max()) - start) / 1e5, 3),
            "spread_ms": round((int(ends.max()) - int(ends.min())) / 1e5, 3)}


def cpu_rate(tab, words, nprefixes, threads):
    nodes = [0]
    t0 = time.perf_counter()
    counts = E.count_states_cpu(tab, words, nprefixes, threads=threads, nodes=nodes)
    dt = time.perf_counter() - t0
    return dt, nodes[0], counts


def bench_board(p, name, depth_list, capacity, reps, sample):
    tab = E.table(p)
    prefixes = p.split(2)
    out = {"board": name, "pieces": tab.npieces, "rows": tab.nrows, "mask_words": tab.words,
           "prefixes": len(prefixes), "capacity": capacity}
    ab = {}
    ref = None
    for levels in depth_list:
        dt, counts = plain_count(tab, prefixes, levels, capacity, reps)
        ab[str(levels)] = round(dt * 1e3, 2)
        ref = counts if ref is None else ref
        assert torch.equal(counts, ref), f"levels {levels} changes the counts"
    best = int(min(ab, key=ab.get))
    out["depth_ab_ms"] = ab
    out["levels"] = best
    out["solutions"] = int(ref.sum())
    dt, counts, placed, groups, longest = run_count(tab, prefixes, best, capacity)
    assert torch.equal(counts, ref)
    out["placements"] = placed
    out["count_gpu_ms"] = ab[str(best)]
    out["nodes_per_s"] = round(placed / (ab[str(best)] / 1e3))
    out["kernel_groups"] = {f"{k}{lv}": {"ms": round(g[0] * 1e3, 3), "launches": g[1],
                                         "states": g[2]}
                            for (k, lv), g in sorted(groups.items(), key=lambda kv: kv[0][1])}
    count_ms = sum(g[0] for (k, _), g in groups.items() if k == "count") * 1e3
    out["count_kernel_ms"] = round(count_ms, 3)
    out["count_kernel_nodes_per_s"] = round(placed / (count_ms / 1e3)) if count_ms else None
    out["longest_count_launch_ms"] = round(longest * 1e3, 3)
    out["wg_finish"] = wg_spread(tab, frontier(tab, prefixes, best, capacity), len(prefixes))

    # the CPU yardstick
    first = E.states(tab, prefixes)
    if sample <= 1:
        words, what = first, "all prefixes"
    else:
        two = E.expand(tab, E.expand(tab, first))
        words, what = two[::sample], f"every {sample}th state two levels below the prefixes"
    dev = torch.from_numpy(words.view("int64")).cuda()
    gpu_counts = torch.zeros(len(prefixes), dtype=torch.int64, device="cuda")
    scratch = torch.zeros(2, dtype=torch.int64, device="cuda")
    for part in E.expand_gpu(tab, dev, capacity):      # warm
        pass
    t0 = sync_time()
    level = [dev]
    for _ in range(max(0, best - (0 if sample <= 1 else 2))):
        level = [c for w in level for c in E.expand_gpu(tab, w, capacity)]
    for w in level:
        E.count_states_gpu(tab, w, gpu_counts, scratch)
    gpu_dt = sync_time() - t0
    one_dt, nodes, one = cpu_rate(tab, words, len(prefixes), 1)
    many_dt, nodes16, many = cpu_rate(tab, words, len(prefixes), 16)
    assert one.tolist() == many.tolist() == gpu_counts.cpu().tolist() and nodes == nodes16
    out["yardstick"] = {
        "states": what, "placements": nodes, "solutions": int(one.sum()),
        "cpu_1_thread_s": round(one_dt, 3), "cpu_1_thread_nodes_per_s": round(nodes / one_dt),
        "cpu_16_threads_s": round(many_dt, 3),
        "cpu_16_threads_nodes_per_s": round(nodes / many_dt),
        "gpu_s": round(gpu_dt, 4), "gpu_nodes_per_s": round(nodes / gpu_dt),
        "gpu_vs_1_thread": round(one_dt / gpu_dt, 1),
        "gpu_vs_16_threads": round(many_dt / gpu_dt, 1)}
    return out


def end_to_end(width, height, classic_cap):
    """``pentomino -gpu`` (its own LocalCluster over the GPU, as the command
    line makes it) against the classic program in a process of its own, ended
    after ``classic_cap`` seconds."""
    tmp = tempfile.mkdtemp(prefix="bench-pent-")
    try:
        with LocalCluster(JobConf(), num_trackers=1, gpus=[[0]]) as cl:
            dancing.run_pentomino(os.path.join(tmp, "warm"), 20, 3, cluster=cl, gpu=True)
            t0 = time.perf_counter()
            n = dancing.run_pentomino(os.path.join(tmp, "g"), width, height, cluster=cl, gpu=True)
            gpu_s = time.perf_counter() - t0
        gpu_part = open(os.path.join(tmp, "g", "part-00000"), "rb").read()
        out = {"board": f"{height}x{width}", "solutions": n, "gpu_s": round(gpu_s, 3)}
        cmd = [sys.executable, "-m", "hbmr", "examples", "pentomino", os.path.join(tmp, "c"),
               "-width", str(width), "-height", str(height)]
        t0 = time.perf_counter()
        try:
            subprocess.run(cmd, capture_output=True, timeout=classic_cap, check=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            out["classic_s"] = round(time.perf_counter() - t0, 1)
            out["same_output"] = open(os.path.join(tmp, "c", "part-00000"),
                                      "rb").read() == gpu_part
            out["speedup"] = round(out["classic_s"] / gpu_s, 1)
        except subprocess.TimeoutExpired:
            out["classic_s"] = f"over {classic_cap} s"
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--onesided", default="5x18", help="HxW of the one-sided board")
    ap.add_argument("--depths", default="2,4,6,8,9,10")
    ap.add_argument("--capacity", type=int, default=E.DEFAULT_CAPACITY)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--onesided-depths", default="6,7,8,9,10")
    ap.add_argument("--sample", type=int, default=8,
                    help="the one-sided board's CPU yardstick takes every N-th frontier state")
    ap.add_argument("--classic-cap", type=int, default=30)
    ap.add_argument("--skip-onesided", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pentomino needs a GPU"
    depths = [int(x) for x in a.depths.split(",")]
    res = {"benchmark": "GPU Pentomino exact-cover kernels and end-to-end job (1 MI355X)",
           "reps": a.reps, "boards": []}
    res["boards"].append(bench_board(dancing.Pentomino(10, 6), "6x10", depths, a.capacity,
                                     a.reps, 1))
    if not a.skip_onesided:
        h, w = (int(x) for x in a.onesided.split("x"))
        res["boards"].append(bench_board(dancing.OneSidedPentomino(w, h),
                                         f"one-sided {a.onesided}",
                                         [int(x) for x in a.onesided_depths.split(",")],
                                         a.capacity, 0, a.sample))
    if not a.skip_e2e:
        res["end_to_end"] = [end_to_end(15, 4, 120), end_to_end(10, 6, a.classic_cap)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
