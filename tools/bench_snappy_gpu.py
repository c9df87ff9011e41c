"""Snappy-compressed text input on one MI355X (hbmr/ops/snappydec.py,
native/kernels/snappydec.hip), in one run over the same files:

* the decode kernel over ``--mb`` MiB of decoded text, in output bytes per
  second, for two inputs: Zipf word text (the corpus law of
  tools/bench_wordcount.py) and ``"a b\\n"`` int-pair lines, which consist of short
  elements (about 5 output bytes each against 11);
* the yardsticks: the host decoder (native/io/snappy.cc) on 1 thread and on 16
  threads, one chunk range per thread, and a ``torch`` device copy of the output
  bytes;
* the chunk count and the element count (literals, copies) of each input;
* ``wordcount -gpu`` over ``--files`` ``.snappy`` files, on a fresh cluster and
  again with the decoded splits resident, against the classic job on 8 CPU
  slots over the same files.

An input is one generated unit of 77 full chunks (about 16 MiB) compressed
once and repeated as blocks of the file: chunks are independent, so every
block is the same decode work.  Medians of ``--reps`` runs after a warm-up.
Prints one JSON line."""
import argparse
import concurrent.futures as cf
import ctypes
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

from hbmr.io import snappy  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.models import splits  # noqa: E402
from hbmr.models import wordcount as wc_model  # noqa: E402
from hbmr.ops import snappydec  # noqa: E402

LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
CHUNK_INPUT = snappy.BUFFER_SIZE_DEFAULT - (snappy.BUFFER_SIZE_DEFAULT // 6 + 32)
UNIT = 77 * CHUNK_INPUT
THREADS = 16


def zipf_text(nbytes, vocab=200_000, seed=7):
    rng = np.random.default_rng(seed)
    words = [bytes(LETTERS[rng.integers(0, 26, rng.integers(2, 12))]) + b"%d" % i
             for i in range(vocab)]
    lines, size = [], 0
    while size < nbytes:
        ids = np.minimum(rng.zipf(1.3, rng.integers(1, 12)) - 1, vocab - 1)
        lines.append(b" ".join(words[i] for i in ids))
        size += len(lines[-1]) + 1
    return (b"\n".join(lines) + b"\n")[:nbytes - 1] + b"\n"


def pair_text(nbytes, seed=3):
    """``"a b\\n"`` lines: ``a`` of 100 values, ``b`` of 300 (fully random
    seconds are digit noise that no LZ77 shortens): elements of a few bytes."""
    rng = np.random.default_rng(seed)
    n = nbytes // 4 + 1
    seconds = rng.integers(-10 ** 6, 10 ** 6, 300)
    a, b = rng.integers(-50, 50, n), seconds[rng.integers(0, seconds.size, n)]
    text = "".join(f"{x} {y}\n" for x, y in zip(a.tolist(), b.tolist())).encode()
    return text[:nbytes - 1] + b"\n"


def count_elements(data, table):
    """(literals, copies) of the chunks of ``data``."""
    lits = copies = 0
    for a, c, _, _ in table.t().tolist():
        s = data[a:a + c]
        i = 1
        while s[i - 1] & 0x80:
            i += 1
        while i < c:
            tag = s[i]
            kind = tag & 3
            if kind == 0:
                ln = tag >> 2
                i += 1
                if ln >= 60:
                    nb = ln - 59
                    ln = int.from_bytes(s[i:i + nb], "little")
                    i += nb
                i += ln + 1
                lits += 1
            else:
                i += (2, 3, 5)[kind - 1]
                copies += 1
    return lits, copies


def kernel_ms(fn, reps):
    """Median device time of ``fn`` by events."""
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def host_threads(data, table, total, threads):
    """Seconds of the host decoder over ``threads`` chunk ranges (ctypes calls
    release the GIL)."""
    decompress = ctypes.CDLL(snappy._PATH).hbmr_snappy_decompress    # a handle of its own
    decompress.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long]
    decompress.restype = ctypes.c_long
    out = ctypes.create_string_buffer(total)
    base = ctypes.addressof(out)
    rows = table.t().tolist()
    n = len(rows)
    view = (ctypes.c_char * len(data)).from_buffer_copy(data)
    src = ctypes.addressof(view)

    def work(k):
        for a, c, d, u in rows[k * n // threads:(k + 1) * n // threads]:
            if decompress(src + a, c, base + d, u) != u:
                raise RuntimeError("host decoder failed")
    with cf.ThreadPoolExecutor(threads) as ex:
        t = time.perf_counter()
        list(ex.map(work, range(threads)))
        return time.perf_counter() - t, out.raw


def kernel_and_yardsticks(name, unit, blocks, reps):
    block = snappy.hadoop_compress(unit)
    data = block * blocks
    table, total = snappydec.chunk_table(data)
    assert total == len(unit) * blocks
    ut, _ = snappydec.chunk_table(block)
    lits, copies = count_elements(block, ut)
    res = {"input": name, "decoded_bytes": total, "compressed_bytes": len(data),
           "ratio": round(total / len(data), 2), "chunks": int(table.shape[1]),
           "literals": lits * blocks, "copies": copies * blocks,
           "output_bytes_per_element": round(len(unit) / (lits + copies), 1)}
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    tdev = table.contiguous().cuda()
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(out)

    def launch():
        snappydec.decode_chunks(src, table, out, _table_dev=tdev)
    k = kernel_ms(launch, reps) / 1e3
    bad = snappydec.first_bad_chunk(snappydec.decode_chunks(src, table, out, _table_dev=tdev)[1])
    copy = kernel_ms(lambda: other.copy_(out), reps) / 1e3
    one = min(host_threads(data, table, total, 1)[0] for _ in range(2))
    many, plain = min((host_threads(data, table, total, THREADS) for _ in range(3)),
                      key=lambda r: r[0])
    res["same_output"] = bad is None and plain == unit * blocks and \
        out.cpu().numpy().tobytes() == plain
    gbs = lambda s: round(total / s / 1e9, 2)  # noqa: E731
    res.update({"kernel_ms": round(k * 1e3, 3), "kernel_gb_per_s": gbs(k),
                "host_1_thread_gb_per_s": gbs(one), f"host_{THREADS}_threads_gb_per_s": gbs(many),
                "device_copy_gb_per_s": gbs(copy),
                "kernel_vs_host_1_thread": round(one / k, 1),
                f"kernel_vs_host_{THREADS}_threads": round(many / k, 2),
                "kernel_vs_device_copy": round(copy / k, 4)})
    # a file with few chunks has little parallelism: the first 10 chunks alone
    few = table[:, :10].contiguous()
    fdev = few.cuda()
    fk = kernel_ms(lambda: snappydec.decode_chunks(src, few, out, _table_dev=fdev), reps) / 1e3
    res["ten_chunks"] = {"decoded_bytes": int(few[3].sum()), "kernel_ms": round(fk * 1e3, 3),
                         "kernel_gb_per_s": round(int(few[3].sum()) / fk / 1e9, 2)}
    return res


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


def end_to_end(nbytes, files, tmp):
    inp = os.path.join(tmp, "in")
    os.makedirs(inp)
    per = nbytes // files
    chunks = 0
    for f in range(files):
        data = snappy.hadoop_compress(zipf_text(per, seed=100 + f))
        chunks += int(snappydec.chunk_table(data)[0].shape[1])
        with open(os.path.join(inp, f"part-{f:05d}.snappy"), "wb") as fh:
            fh.write(data)
    res = {"files": files, "decoded_bytes": per * files, "chunks": chunks,
           "compressed_bytes": sum(os.path.getsize(os.path.join(inp, f)) for f in os.listdir(inp))}
    gconf = JobConf()
    gconf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(gconf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("cold", "resident"):
            t = time.perf_counter()
            rj = wc_model.run(inp, os.path.join(tmp, f"gpu-{run}"), 1, cluster=cl, gpu=True)
            res[f"gpu_{run}_s"] = round(time.perf_counter() - t, 3)
            res[f"gpu_{run}_decoded_bytes"] = rj.getCounters().get(
                splits.COMPRESSED_INPUT_GROUP, splits.SNAPPY_DECODED_BYTES)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        wc_model.run(inp, os.path.join(tmp, "classic"), 1, cluster=cl)
        res["classic_8_cpu_slots_s"] = round(time.perf_counter() - t, 3)
    want = _parts(os.path.join(tmp, "classic"))
    res["same_output"] = all(_parts(os.path.join(tmp, f"gpu-{r}")) == want
                             for r in ("cold", "resident"))
    res["speedup_cold"] = round(res["classic_8_cpu_slots_s"] / res["gpu_cold_s"], 2)
    res["speedup_resident"] = round(res["classic_8_cpu_slots_s"] / res["gpu_resident_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mb", type=int, default=256, help="MiB of decoded text per input")
    ap.add_argument("--e2e-mb", type=int, default=16,
                    help="MiB of decoded text of the end-to-end corpus over all files (0: skip)")
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_snappy_gpu.py measures on a GPU; none is visible")
    blocks = max(1, round((a.mb << 20) / UNIT))
    res = {"benchmark": "Snappy decode kernel, host decoder and device copy; wordcount -gpu over "
                        ".snappy files (1 MI355X)", "reps": a.reps, "unit_bytes": UNIT,
           "blocks": blocks, "kernel": []}
    for name, gen in (("zipf-words", zipf_text), ("int-pairs", pair_text)):
        res["kernel"].append(kernel_and_yardsticks(name, gen(UNIT), blocks, a.reps))
        print(f"# {json.dumps(res['kernel'][-1])}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if a.e2e_mb:
        tmp = tempfile.mkdtemp(prefix="bench-snappy-")
        try:
            res["end_to_end"] = end_to_end(a.e2e_mb << 20, a.files, tmp)
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
