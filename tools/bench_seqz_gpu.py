"""Snappy-compressed SequenceFile splits on one MI355X (hbmr/ops/seqz.py,
native/kernels/seqblock.hip), in one run over the same files:

* ``--mb`` MiB of decoded records of two shapes, RandomWriter-like
  (BytesWritable keys of 10-1000 bytes, values to 20 KB: about 100 frames a
  1 MB block) and RandomTextWriter-like (Text keys and values of words: about
  1,500 frames a block), each as a RECORD- and as a BLOCK-compressed file;
* per file the loader's stages by device events (decode, vint, index,
  assemble), the whole load (plan, read, H2D copy and kernels) by the wall
  clock, and the yardsticks: a ``torch`` device copy of the output bytes,
  ``recsort.gather_frames`` over the same frames, and the host path
  (``sequencefile.Reader`` through ``SequenceFileRecordReader``) over the first
  ``--host-mb`` MiB on 1 process and over 16 windows on 16 processes;
* ``sort -gpu`` over the RandomWriter-like records (``--sort-mb`` MiB): cold
  and resident on the compressed files, on the same records uncompressed (after
  a throw-away job over other files that warms the cluster up), and the classic
  job on 8 CPU slots.

A file is one generated unit (``--unit-mb``) written by ``sequencefile.Writer``
and its body repeated: records and blocks are independent, so every repeat is
the same work.  Medians of ``--reps`` runs after a warm-up.  Prints one JSON
line and writes it to ``--out``."""
import argparse
import concurrent.futures as cf
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.io import sequencefile as seqf  # noqa: E402
from hbmr.io.compress import SnappyCodec  # noqa: E402
from hbmr.io.writable import BytesWritable, Text  # noqa: E402

WORDS = [b"w%d" % i + b"abcdefghij"[:i % 9] for i in range(1000)]


def unit_records(shape, nbytes, seed=5):
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < nbytes:
        if shape == "randomwriter":
            k = rng.integers(0, 256, int(rng.integers(10, 1000)), dtype=np.uint8).tobytes()
            v = rng.integers(0, 256, int(rng.integers(0, 20000)), dtype=np.uint8).tobytes()
        else:
            k = b" ".join(WORDS[i] for i in rng.integers(0, 1000, int(rng.integers(5, 10))))
            v = b" ".join(WORDS[i] for i in rng.integers(0, 1000, int(rng.integers(20, 100))))
        out.append((k, v))
        size += 16 + len(k) + len(v)
    return out


def write_repeated(path, recs, kcls, mode, repeats):
    """The records through Writer once; the file is its body ``repeats`` times."""
    kw = {} if mode == "NONE" else dict(compression=mode, codec=SnappyCodec())
    tmp = path + ".unit"
    with seqf.Writer(tmp, kcls, kcls, **kw) as w:
        for k, v in recs:
            w.append(kcls(k), kcls(v))
        sync = w.sync
    with seqf.Reader(tmp) as r:
        head = r.header_end
    raw = open(tmp, "rb").read()
    os.remove(tmp)
    body = raw[head:]
    if not body.startswith(b"\xff\xff\xff\xff" + sync):      # RECORD / NONE: a marker between
        body = b"\xff\xff\xff\xff" + sync + body
    with open(path, "wb") as f:
        f.write(raw[:head])
        for _ in range(repeats):
            f.write(body)
    return path


def _host_window(args):
    from hbmr.mapred.formats import FileSplit, SequenceFileRecordReader
    path, start, length = args
    rr = SequenceFileRecordReader(None, FileSplit(path, start, length))
    n = 0
    for k, v in iter(rr.next_raw, None):
        n += 8 + len(k) + len(v)
    rr.close()
    return n


def host_path(path, nbytes_file, limit):
    """MB/s of decoded bytes of the Python reader on 1 and on 16 processes."""
    span = min(nbytes_file, limit)
    t = time.perf_counter()
    got = _host_window((path, 0, span))
    one = got / (time.perf_counter() - t) / 1e6
    cuts = [span * i // 16 for i in range(17)]
    with cf.ProcessPoolExecutor(16) as ex:
        list(ex.map(_host_window, [(path, 0, 1)] * 16))           # start the workers
        t = time.perf_counter()
        got = sum(ex.map(_host_window, [(path, a, b - a) for a, b in zip(cuts, cuts[1:])]))
        many = got / (time.perf_counter() - t) / 1e6
    return {"host_1_MBps": round(one, 1), "host_16_MBps": round(many, 1)}


def median_events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def load_stages(path, size, reps):
    """Median ms per stage and of the whole load; the last (data, index)."""
    import torch
    from hbmr.ops import seqz
    seqz.load_split(path, 0, size, "cuda")
    per, wall = {}, []
    for _ in range(reps):
        stages = []
        torch.cuda.synchronize()
        t = time.perf_counter()
        data, index = seqz.load_split(path, 0, size, "cuda", stages=stages)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        for name, a, b in stages:
            per.setdefault(name, []).append(a.elapsed_time(b))
    out = {k + "_ms": round(statistics.median(v), 3) for k, v in per.items()}
    out["load_wall_ms"] = round(statistics.median(wall), 2)
    return out, data, index


def bench_file(path, reps):
    import torch
    from hbmr.ops import recsort
    size = os.path.getsize(path)
    res, data, index = load_stages(path, size, reps)
    nbytes = int(data.numel())
    res.update(file_MB=round(size / 1e6, 1), decoded_MB=round(nbytes / 1e6, 1),
               records=int(index.shape[1]))
    res["device_copy_ms"] = round(median_events(lambda: data.clone(), reps), 3)
    foff, flen = index[0].contiguous(), index[1].contiguous()
    res["gather_frames_ms"] = round(median_events(
        lambda: recsort.gather_frames(data, None, foff, flen, foff, nbytes, check=False), reps), 3)
    if "vint_ms" in res:          # RECORD: the assemble stage writes headers and keys only
        res["assemble_GBps"] = round(nbytes / res["assemble_ms"] / 1e6, 1)
    res["gather_GBps"] = round(nbytes / res["gather_frames_ms"] / 1e6, 1)
    del data, index
    torch.cuda.empty_cache()
    return res


def sort_jobs(root, mb, unit_mb):
    from hbmr.examples import sort as sort_example
    from hbmr.mapred import JobConf
    from hbmr.mapred.cluster import LocalCluster
    from hbmr.models import sort as sort_job
    recs = unit_records("randomwriter", unit_mb << 20)
    reps = max(1, mb // unit_mb)
    dirs = {}
    for mode in ("NONE", "RECORD", "BLOCK"):
        d = os.path.join(root, f"sort-{mode}")
        os.makedirs(d)
        for part in range(2):
            write_repeated(os.path.join(d, f"part-{part:05d}"), recs, BytesWritable, mode,
                           max(1, reps // 2))
        dirs[mode] = d
    out = {}
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    warm = os.path.join(root, "sort-warm")
    os.makedirs(warm)
    write_repeated(os.path.join(warm, "part-00000"), recs[:200], BytesWritable, "BLOCK", 1)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        # a throw-away job over other files: library load and first launches are not timed
        rj = cl.submit_job(sort_job.gpu_job(warm, os.path.join(root, "o-warm"), 4, maps=1))
        rj.waitForCompletion(600)
        for mode, d in dirs.items():
            for run in ("cold", "resident"):
                o = os.path.join(root, f"o-{mode}-{run}")
                t = time.perf_counter()
                rj = cl.submit_job(sort_job.gpu_job(d, o, 4, maps=1))
                ok = rj.waitForCompletion(600) and rj.isSuccessful()
                out[f"sort_gpu_{mode}_{run}_s"] = round(time.perf_counter() - t, 2) if ok else None
                shutil.rmtree(o, ignore_errors=True)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        o = os.path.join(root, "o-classic")
        t = time.perf_counter()
        rj = sort_example.run(dirs["RECORD"], o, 4, cluster=cl)
        out["sort_classic_8_cpu_slots_RECORD_s"] = round(time.perf_counter() - t, 2) \
            if rj.isSuccessful() else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--unit-mb", type=int, default=16)
    ap.add_argument("--host-mb", type=int, default=32)
    ap.add_argument("--sort-mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/seqz_1gpu.json")
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix="seqz-bench-")
    res = {"mb": a.mb, "unit_mb": a.unit_mb, "host_mb": a.host_mb, "sort_mb": a.sort_mb,
           "reps": a.reps, "files": {}}
    try:
        files = {}
        for shape, kcls in (("randomwriter", BytesWritable), ("randomtextwriter", Text)):
            recs = unit_records(shape, a.unit_mb << 20)
            for mode in ("RECORD", "BLOCK"):
                name = f"{shape}-{mode}"
                files[name] = write_repeated(os.path.join(root, name + ".seq"), recs, kcls, mode,
                                             max(1, a.mb // a.unit_mb))
        # the host path first: its worker processes start before the GPU is opened
        for name, path in files.items():
            res["files"][name] = host_path(path, os.path.getsize(path), a.host_mb << 20)
        for name, path in files.items():
            res["files"][name].update(bench_file(path, a.reps))
            print(name, json.dumps(res["files"][name]), flush=True)
            os.remove(path)
        if a.sort_mb:
            res["sort"] = sort_jobs(root, a.sort_mb, a.unit_mb)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
