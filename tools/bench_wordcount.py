"""The GPU word-count family on one MI355X, three figures in one run:

* ``wordtab_fill_kernel`` in output bytes per second next to ``zero_()`` and a
  ``torch`` copy of the same byte count, interleaved in one process, at
  1 M words of 2-9 bytes and at 10,000 words of 4 KiB;
* the device reduce (``sort_table`` + ``format_part`` + the one copy to the
  host) against the host reduce of ``WordCountSplitJob`` (``text.sorted_items``
  + the join) over the same merged table, at 10^4, 10^6 and 10^7 distinct words;
* each program with ``-gpu`` (a fresh cluster, then warm) against its classic
  job on 8 CPU slots over one generated corpus.

Medians of ``--reps`` runs after a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.examples import driver  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.ops import text, wordtab  # noqa: E402

PROGRAMS = ["wordcount", "multifilewc", "aggregatewordcount", "aggregatewordhist"]
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
DEV = "cuda"


def interleaved(fns, reps):
    """Median seconds of each function, run in turn ``reps`` times after one
    warm-up round."""
    times = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t)
    return {k: statistics.median(v) for k, v in times.items()}


def word_table(n, lo, hi, seed=1, distinct=True):
    """A word table of ``n`` words of lo..hi letters on the GPU: (buf, starts,
    lens, counts), the buffer being the words' ``b"word\\n"`` blob.
    ``distinct``: word i ends in the base-26 digits of i (and is at least that
    long)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, n, endpoint=True).astype(np.int64)
    digits = max(1, int(np.ceil(np.log(max(n, 2)) / np.log(26)))) if distinct else 0
    lens = np.maximum(lens, digits)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    raw = LETTERS[rng.integers(0, 26, int(lens.sum() + n))]
    raw[starts + lens] = 10
    ids = np.arange(n)
    for d in range(digits):
        raw[starts + lens - 1 - d] = LETTERS[ids % 26]
        ids //= 26
    counts = rng.integers(1, 100_000, n)
    return (torch.from_numpy(raw).to(DEV), torch.from_numpy(starts.astype(np.int32)).to(DEV),
            torch.from_numpy(lens.astype(np.int32)).to(DEV), torch.from_numpy(counts).to(DEV))


def fill_rates(n, lo, hi, reps):
    buf, starts, lens, counts = word_table(n, lo, hi, distinct=False)
    order = torch.randperm(n, device=DEV).to(torch.int32)
    offs = wordtab.offsets(wordtab.line_lengths(lens, counts, order))
    total = int(offs[-1])
    out = torch.empty(total, dtype=torch.uint8, device=DEV)
    src = torch.empty_like(out)
    t = interleaved({"fill": lambda: wordtab._fill(buf, starts, lens, counts, order, offs, total,
                                                   out, None),
                     "zero": lambda: out.zero_(),
                     "copy": lambda: out.copy_(src)}, reps)
    wordtab._fill(buf, starts, lens, counts, order, offs, total, out, None)
    if n <= 20_000:                                       # what was timed wrote the right bytes
        words, cs = wordtab.words_of(buf, starts, lens), counts.tolist()
        assert out.cpu().numpy().tobytes() == \
            b"".join(b"%s\t%d\n" % (words[i], cs[i]) for i in order.tolist())
    gbs = lambda s: round(total / s / 1e9, 1)  # noqa: E731
    return {"words": n, "word_bytes": [lo, hi], "output_bytes": total,
            "fill_ms": round(t["fill"] * 1e3, 3), "fill_gb_per_s": gbs(t["fill"]),
            "zero_gb_per_s": gbs(t["zero"]), "copy_gb_per_s": gbs(t["copy"]),
            "fill_vs_zero": round(t["zero"] / t["fill"], 3),
            "fill_vs_copy": round(t["copy"] / t["fill"], 3)}


def host_reduce(blob, counts):
    """The reduce tail of WordCountSplitJob: the merged table to the host,
    Python's sorted, the join."""
    items = text.sorted_items(blob, counts)
    return b"".join(w + b"\t" + str(n).encode() + b"\n" for w, n in items)


def device_reduce(buf, starts, lens, counts):
    parts = wordtab.partition(buf, starts, lens, 1)
    order, _ = wordtab.sort_table(buf, starts, lens, parts, 1)
    return wordtab.format_part(buf, starts, lens, counts, order).cpu().numpy().tobytes()


def reduce_compare(n, reps):
    buf, starts, lens, counts = word_table(n, 2, 12, seed=n)
    fns = {"device": lambda: device_reduce(buf, starts, lens, counts),
           "host": lambda: host_reduce(buf, counts)}
    if n <= 10 ** 6:
        same = fns["device"]() == fns["host"]()
        t = interleaved(fns, reps)
    else:
        # the host reduce takes minutes here: one timed run of each, the device
        # reduce after a run of its own (the host one has nothing to warm up)
        reps, t, got = 1, {}, {}
        fns["device"]()
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = fn()
            t[k] = time.perf_counter() - t0
        same = got["device"] == got["host"]
    return {"distinct_words": n, "table_bytes": int(buf.numel()), "reps": reps,
            "device_reduce_ms": round(t["device"] * 1e3, 2),
            "host_reduce_ms": round(t["host"] * 1e3, 2),
            "host_over_device": round(t["host"] / t["device"], 2), "same_output": same}


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


def corpus(tmp, nbytes, files, vocab):
    """``files`` files of lines of 1-12 words drawn by a Zipf law from ``vocab``
    random words."""
    rng = np.random.default_rng(7)
    words = [bytes(LETTERS[rng.integers(0, 26, rng.integers(2, 12))]) + b"%d" % i
             for i in range(vocab)]
    inp = os.path.join(tmp, "in")
    os.makedirs(inp)
    per = nbytes // files
    for f in range(files):
        size, lines = 0, []
        while size < per:
            ids = np.minimum(rng.zipf(1.3, rng.integers(1, 12)) - 1, vocab - 1)
            line = b" ".join(words[i] for i in ids)
            lines.append(line)
            size += len(line) + 1
        with open(os.path.join(inp, f"file{f:02d}.txt"), "wb") as fh:
            fh.write(b"\n".join(lines) + b"\n")
    return inp


def end_to_end(nbytes, files, reduces, tmp):
    inp = corpus(tmp, nbytes, files, 200_000)
    res = {"files": files, "reduces": reduces,
           "input_bytes": sum(os.path.getsize(os.path.join(inp, f)) for f in os.listdir(inp))}

    def args(p, out):
        if p in ("wordcount", "multifilewc"):
            return [inp, out, "-r", str(reduces), "-m", str(files)]
        return [inp, out, str(reduces)]
    gconf = JobConf()
    gconf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    for p in PROGRAMS:
        r = {}
        with LocalCluster(gconf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
            for run in ("fresh", "warm"):
                t = time.perf_counter()
                assert driver.run(p, args(p, os.path.join(tmp, f"{p}-gpu-{run}")) + ["-gpu"],
                                  cluster=cl) == 0
                r[f"gpu_{run}_s"] = round(time.perf_counter() - t, 3)
        with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
            t = time.perf_counter()
            assert driver.run(p, args(p, os.path.join(tmp, f"{p}-classic")), cluster=cl) == 0
            r["classic_8_cpu_slots_s"] = round(time.perf_counter() - t, 3)
        want = _parts(os.path.join(tmp, f"{p}-classic"))
        r["same_output"] = all(_parts(os.path.join(tmp, f"{p}-gpu-{run}")) == want
                               for run in ("fresh", "warm"))
        r["output_bytes"] = sum(len(v) for v in want.values())
        r["speedup_fresh"] = round(r["classic_8_cpu_slots_s"] / r["gpu_fresh_s"], 2)
        r["speedup_warm"] = round(r["classic_8_cpu_slots_s"] / r["gpu_warm_s"], 2)
        print(f"# {p}: {json.dumps(r)}", file=sys.stderr, flush=True)
        res[p] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reduce-sizes", default="10000,1000000,10000000")
    ap.add_argument("--e2e-mb", type=int, default=32,
                    help="MiB of the end-to-end corpus over all files (0: skip)")
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--reduces", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wordcount.py measures on a GPU; none is visible")
    res = {"benchmark": "GPU word-count family: fill kernel, device reduce, end to end "
                        "(1 MI355X)", "reps": a.reps}
    res["fill"] = [fill_rates(1_000_000, 2, 9, a.reps), fill_rates(10_000, 4096, 4096, a.reps)]
    print(f"# {json.dumps(res['fill'])}", file=sys.stderr, flush=True)
    res["reduce"] = []
    for n in (int(x) for x in a.reduce_sizes.split(",") if x):
        res["reduce"].append(reduce_compare(n, a.reps))
        print(f"# {json.dumps(res['reduce'][-1])}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if a.e2e_mb:
        tmp = tempfile.mkdtemp(prefix="bench-wordcount-")
        try:
            res["end_to_end"] = end_to_end(a.e2e_mb << 20, a.files, a.reduces, tmp)
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
