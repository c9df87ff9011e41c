"""GPU SecondarySort on one MI355X: the warm stages of hbmr/ops/intpair.py over
"a b\\n" lines held in HBM (``first`` from 10,000 values, ``second`` uniform in
int32) — parse, partition + sort, lengths + fill — next to three yardsticks
measured in the same run over the same bytes: a read-only ``torch.sum`` of the
input viewed as int64 (for the parse), ``zero_()`` of a buffer of the output's
size (for the fill) and ``radix_sort_keys`` alone over the same number of keys
(for the sort); and ``secondarysort -gpu`` end to end, cold and with the splits
resident, against the classic job on 8 CPU slots over the same 8 files.
Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.examples import secondarysort as example  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.ops import intpair  # noqa: E402
from hbmr.ops.sort import radix_sort_keys  # noqa: E402

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def lines(nbytes, seed=1, batch=1 << 20):
    """About ``nbytes`` of "a b\\n" lines as a uint8 array."""
    rng = np.random.default_rng(seed)
    values = rng.integers(INT_MIN, INT_MAX, 10_000, dtype=np.int64, endpoint=True)
    parts, size = [], 0
    while size < nbytes:
        a = values[rng.integers(0, values.size, batch)]
        b = rng.integers(INT_MIN, INT_MAX, batch, dtype=np.int64, endpoint=True)
        c1, k1 = intpair._digits_np(a)
        c2, k2 = intpair._digits_np(b)
        one = np.ones((batch, 1), dtype=bool)
        chars = np.concatenate([c1, np.full((batch, 1), 32, np.uint8), c2,
                                np.full((batch, 1), 10, np.uint8)], axis=1)
        text = chars[np.concatenate([k1, one, k2, one], axis=1)]
        if size + text.size > nbytes:
            text = text[:int(np.flatnonzero(text[:nbytes - size] == 10)[-1]) + 1]
            parts.append(text)
            break
        parts.append(text)
        size += text.size
    return np.concatenate(parts)


def stages(data, nparts, reps):
    nb = int(data.numel())
    parsed = intpair.parse(data)
    assert not parsed.irregular and parsed.keys.numel() == parsed.lines
    keys = parsed.keys
    n = int(keys.numel())
    starts, _ = intpair.line_starts(data)
    status, lkeys, bc = intpair.parse_lines(data, starts)
    t_lines = timed(lambda: intpair.line_starts(data), reps)
    t_parse_k = timed(lambda: intpair.parse_lines(data, starts), reps)
    t_compact = timed(lambda: intpair.compact(status, lkeys, bc), reps)
    t_parse = timed(lambda: intpair.parse(data), reps)
    del status, lkeys, bc, starts
    words = data[:nb - nb % 8].view(torch.int64)
    t_sum = timed(lambda: torch.sum(words), reps)
    t_part = timed(lambda: intpair.partition(keys, nparts), reps)
    t_sort = timed(lambda: intpair.sort_keys(keys, nparts), reps)
    t_radix = timed(lambda: radix_sort_keys(keys.clone()), reps)
    skeys = radix_sort_keys(keys.clone())
    text, groups = intpair.format_part(skeys)
    out_bytes = int(text.numel())
    lens = intpair.lengths(skeys)
    offs = intpair.offsets(lens)
    t_len = timed(lambda: intpair.lengths(skeys), reps)
    t_fill = timed(lambda: intpair._fill(skeys, offs, text, None), reps)
    t_format = timed(lambda: intpair.format_part(skeys), reps)
    t_zero = timed(lambda: text.zero_(), reps)
    ms = lambda s: round(s * 1e3, 3)  # noqa: E731
    gbs = lambda b, s: round(b / s / 1e9, 1)  # noqa: E731
    return {"input_bytes": nb, "lines": parsed.lines, "records": n, "groups": groups,
            "output_bytes": out_bytes, "partitions": nparts,
            "lines_pass_ms": ms(t_lines), "parse_kernel_ms": ms(t_parse_k),
            "compact_ms": ms(t_compact), "parse_ms": ms(t_parse),
            "parse_gb_per_s": gbs(nb, t_parse),
            "torch_sum_int64_ms": ms(t_sum), "torch_sum_gb_per_s": gbs(nb, t_sum),
            "parse_vs_torch_sum": round(t_sum / t_parse, 3),
            "partition_ms": ms(t_part), "partition_sort_ms": ms(t_sort),
            "radix_sort_keys_ms": ms(t_radix),
            "partition_sort_vs_radix_sort_keys": round(t_radix / t_sort, 3),
            "lengths_ms": ms(t_len), "fill_ms": ms(t_fill), "format_ms": ms(t_format),
            "fill_gb_per_s": gbs(out_bytes, t_fill), "zero_ms": ms(t_zero),
            "zero_gb_per_s": gbs(out_bytes, t_zero),
            "fill_vs_zero": round(t_zero / t_fill, 3),
            "format_vs_zero": round(t_zero / t_format, 3)}


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


def end_to_end(text, files, reduces, tmp):
    inp = os.path.join(tmp, "in")
    os.makedirs(inp)
    ends = np.flatnonzero(text == 10) + 1
    cuts = [0] + [int(ends[len(ends) * (i + 1) // files - 1]) for i in range(files)]
    for i in range(files):
        text[cuts[i]:cuts[i + 1]].tofile(os.path.join(inp, f"file{i:02d}.txt"))
    res = {"files": files, "reduces": reduces, "input_bytes": int(cuts[-1]),
           "records": int(ends.size)}
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("cold", "resident"):
            t = time.perf_counter()
            rj = example.run(inp, os.path.join(tmp, f"gpu-{run}"), reduces, cluster=cl,
                             maps=files, gpu=True)
            res[f"gpu_{run}_s"] = round(time.perf_counter() - t, 3)
            assert rj.isSuccessful()
            print(f"# secondarysort -gpu {run}: {res[f'gpu_{run}_s']} s", file=sys.stderr,
                  flush=True)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        rj = example.run(inp, os.path.join(tmp, "classic"), reduces, cluster=cl, maps=files)
        res["classic_8_cpu_slots_s"] = round(time.perf_counter() - t, 3)
        assert rj.isSuccessful()
    print(f"# classic secondarysort: {res['classic_8_cpu_slots_s']} s", file=sys.stderr, flush=True)
    want = _parts(os.path.join(tmp, "classic"))
    res["same_output"] = all(_parts(os.path.join(tmp, f"gpu-{r}")) == want
                             for r in ("cold", "resident"))
    res["output_bytes"] = sum(len(v) for v in want.values())
    res["speedup_cold"] = round(res["classic_8_cpu_slots_s"] / res["gpu_cold_s"], 1)
    res["speedup_resident"] = round(res["classic_8_cpu_slots_s"] / res["gpu_resident_s"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="MiB of lines in HBM")
    ap.add_argument("--e2e-mb", type=int, default=32,
                    help="MiB of lines of the end-to-end jobs, over all files (0: skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", type=int, default=8, help="partitions of partition + sort")
    ap.add_argument("--files", type=int, default=8, help="input files, end to end")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_secondarysort.py measures on a GPU; none is visible")
    res = {"benchmark": "GPU SecondarySort warm stages and end-to-end job (1 MI355X)",
           "reps": a.reps, "mb": a.mb, "e2e_mb": a.e2e_mb}
    text = lines(a.mb << 20)
    print(f"# {text.size} bytes of lines generated", file=sys.stderr, flush=True)
    res["stages"] = stages(torch.from_numpy(text).cuda(), a.parts, a.reps)
    print(f"# {json.dumps(res['stages'])}", file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    if a.e2e_mb:
        tmp = tempfile.mkdtemp(prefix="bench-secondarysort-")
        try:
            res["end_to_end"] = end_to_end(text[:a.e2e_mb << 20] if a.e2e_mb < a.mb else
                                           lines(a.e2e_mb << 20), a.files, a.parts, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
