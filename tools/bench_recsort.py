"""GPU Sort on one MI355X: the warm map pipeline of hbmr/ops/recsort.py
(partition → string sort by rounds → variable-length record gather) over
RandomWriter-shaped (keys 10–1000 B, values 0–20000 B) and
RandomTextWriter-shaped records held in HBM, next to two reference points
measured in the same run: the fixed-100-byte record gather of TeraSort
(``hbmr_gather_records``) on the same number of bytes, and the classic ``sort``
job end to end on the same records written as SequenceFiles, against the
split-level job.  Prints one JSON line."""
import argparse
import json
import os
import random
import shutil
import struct
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.examples import sort as sort_example  # noqa: E402
from hbmr.examples.randomwriter import _WORDS  # noqa: E402
from hbmr.io import sequencefile as seqf  # noqa: E402
from hbmr.io.vint import encode_vint  # noqa: E402
from hbmr.io.writable import BytesWritable, Text  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.models import sort as sort_job  # noqa: E402
from hbmr.ops import recsort  # noqa: E402
from hbmr.ops import sort as tsort  # noqa: E402


def _put_be32(buf, offs, vals):
    for j in range(4):
        buf[offs + j] = ((vals >> (24 - 8 * j)) & 0xFF).astype(np.uint8)


def random_writer_records(nbytes, seed=1):
    """Frames [recLen][keyLen][len key][len value] of BytesWritable pairs over
    random bytes: (data uint8, index int64[4, n])."""
    rng = np.random.default_rng(seed)
    n = int(nbytes / (16 + 505 + 10000) * 1.05) + 16
    kl = rng.integers(10, 1001, n)
    vl = rng.integers(0, 20001, n)
    fl = 16 + kl + vl
    n = int(np.searchsorted(np.cumsum(fl), nbytes)) or 1
    kl, vl, fl = kl[:n], vl[:n], fl[:n]
    foff = np.cumsum(fl) - fl
    data = rng.integers(0, 256, int(fl.sum()), dtype=np.uint8)
    _put_be32(data, foff, 8 + kl + vl)
    _put_be32(data, foff + 4, 4 + kl)
    _put_be32(data, foff + 8, kl)
    _put_be32(data, foff + 12 + kl, vl)
    return data, np.stack([foff, fl, foff + 12, kl]).astype(np.int64)


def random_text_records(nbytes, seed=2):
    """RandomTextWriter's records: Text keys of 5–10 and values of 10–100 words."""
    rnd = random.Random(seed)
    words = [w.encode() for w in _WORDS]
    vals = []
    for _ in range(4096):
        v = b" ".join(rnd.choices(words, k=rnd.randint(10, 100)))
        vals.append(encode_vint(len(v)) + v)
    parts, idx, off = [], [[], [], [], []], 0
    while off < nbytes:
        k = b" ".join(rnd.choices(words, k=rnd.randint(5, 10)))
        kb = encode_vint(len(k)) + k
        vb = vals[rnd.randrange(4096)]
        parts.append(struct.pack(">ii", len(kb) + len(vb), len(kb)) + kb + vb)
        ln = 8 + len(kb) + len(vb)
        idx[0].append(off)
        idx[1].append(ln)
        idx[2].append(off + 8 + len(kb) - len(k))
        idx[3].append(len(k))
        off += ln
    data = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return data, np.array(idx, dtype=np.int64)


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


def map_pipeline(data, index, nparts, reps):
    n, nb = index.shape[1], data.numel()
    stats = {}
    perm, _, _, blob = recsort.sort_records(data, index, nparts, stats=stats)
    assert blob.numel() == int(index[1].sum())
    total = timed(lambda: recsort.sort_records(data, index, nparts), reps)
    part = timed(lambda: recsort.hash_partition(data, index, nparts), reps)
    sort = timed(lambda: recsort.sort_perm(data, index, nparts), reps)
    lens = index[1][perm.long()]
    dst = torch.cumsum(lens, 0) - lens
    gath = timed(lambda: recsort.gather_frames(data, perm, index[0], index[1], dst, blob.numel(),
                                               check=False), reps)
    return {"records": n, "bytes": nb, "partitions": nparts, "rounds": stats["rounds"],
            "pipeline_ms": round(total * 1e3, 2), "pipeline_gb_per_s": round(nb / total / 1e9, 2),
            "partition_ms": round(part * 1e3, 3), "rounds_ms": round((sort - part) * 1e3, 2),
            "gather_ms": round(gath * 1e3, 3),
            "gather_gb_per_s_copied": round(blob.numel() / gath / 1e9, 1),
            "gather_gb_per_s_read_plus_written": round(2 * blob.numel() / gath / 1e9, 1)}


def fixed_gather(nbytes, reps):
    """TeraSort's fixed-record gather (100-byte records, random permutation)."""
    n = nbytes // 100
    rec = torch.randint(0, 256, (n, 100), dtype=torch.uint8, device="cuda")
    perm = torch.randperm(n, device="cuda").to(torch.int32)
    s = timed(lambda: tsort.gather_records(rec, perm), reps)
    return {"records": n, "ms": round(s * 1e3, 3), "gb_per_s_copied": round(n * 100 / s / 1e9, 1)}


def write_files(data, index, dirname, cls, files):
    os.makedirs(dirname)
    d, ix = torch.from_numpy(data), torch.from_numpy(index)
    n = index.shape[1]
    for f in range(files):
        order = torch.arange(f * n // files, (f + 1) * n // files, dtype=torch.int32)
        with seqf.Writer(os.path.join(dirname, f"part-{f:05d}"), cls, cls) as w:
            recsort.write_part(w, d, ix, order)


def end_to_end(data, index, cls, reduces, maps, tmp):
    inp = os.path.join(tmp, "in")
    write_files(data, index, inp, cls, maps)
    res = {"input_bytes": sum(os.path.getsize(os.path.join(inp, f)) for f in os.listdir(inp)),
           "records": int(index.shape[1]), "reduces": reduces, "maps": maps}
    print(f"# files written ({res['input_bytes']} bytes)", file=sys.stderr, flush=True)
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("cold", "warm"):
            out = os.path.join(tmp, f"gpu-{run}")
            t = time.perf_counter()
            rj = cl.submit_job(sort_job.gpu_job(inp, out, reduces, maps=maps))
            assert rj.waitForCompletion(900) and rj.isSuccessful(), rj.getFailureInfo()
            res[f"split_job_{run}_s"] = round(time.perf_counter() - t, 3)
            print(f"# split job {run}: {res[f'split_job_{run}_s']} s", file=sys.stderr, flush=True)
    cconf = JobConf()
    cconf.set_num_map_tasks(maps)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        rj = sort_example.run(inp, os.path.join(tmp, "classic"), reduces, conf=cconf, cluster=cl)
        assert rj.isSuccessful()
        res["classic_job_s"] = round(time.perf_counter() - t, 3)
    print(f"# classic job: {res['classic_job_s']} s", file=sys.stderr, flush=True)
    same = True
    for p in range(reduces):
        keys = []
        for d in ("gpu-warm", "classic"):
            with seqf.Reader(os.path.join(tmp, d, f"part-{p:05d}")) as r:
                ks = []
                while True:
                    raw = r.next_raw()
                    if raw is None:
                        break
                    ks.append(raw[0])
                keys.append(ks)
        same = same and keys[0] == keys[1]
    res["same_key_sequence_per_part"] = same
    res["split_job_faster"] = res["split_job_warm_s"] < res["classic_job_s"] and \
        res["split_job_cold_s"] < res["classic_job_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="bytes in HBM per input")
    ap.add_argument("--e2e-mb", type=int, default=None,
                    help="bytes per input of the end-to-end jobs (default: --mb; 0: skip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reduces", type=int, default=4)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    e2e_mb = a.mb if a.e2e_mb is None else a.e2e_mb
    res = {"benchmark": "GPU Sort warm map pipeline and end-to-end job (1 MI355X)",
           "reps": a.reps, "inputs": {}}
    res["fixed_100_byte_gather"] = fixed_gather(a.mb << 20, a.reps)
    for name, gen, cls in (("random_writer", random_writer_records, BytesWritable),
                           ("random_text_writer", random_text_records, Text)):
        data, index = gen(a.mb << 20)
        print(f"# {name}: {index.shape[1]} records generated", file=sys.stderr, flush=True)
        ent = {"map_pipeline": map_pipeline(torch.from_numpy(data).cuda(),
                                            torch.from_numpy(index).cuda(), a.reduces, a.reps)}
        ent["map_pipeline"]["gather_vs_fixed_100_byte"] = round(
            ent["map_pipeline"]["gather_gb_per_s_copied"] /
            res["fixed_100_byte_gather"]["gb_per_s_copied"], 3)
        print(f"# {name}: {json.dumps(ent['map_pipeline'])}", file=sys.stderr, flush=True)
        if e2e_mb:
            if e2e_mb != a.mb:
                data, index = gen(e2e_mb << 20)
            tmp = tempfile.mkdtemp(prefix="bench-recsort-")
            try:
                ent["end_to_end"] = end_to_end(data, index, cls, a.reduces, a.maps, tmp)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        res["inputs"][name] = ent
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
