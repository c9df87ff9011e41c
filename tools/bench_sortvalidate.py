"""GPU SortValidator on one MI355X: the warm passes of hbmr/ops/recvalidate.py
(record digest, order check, partition check) over RandomWriter-shaped and
RandomTextWriter-shaped records held in HBM (tools/bench_recsort.py's two
inputs), next to two passes over the same bytes measured in the same run — a
read-only ``torch.sum`` of the buffer viewed as int64 and the variable-length
record gather of GPU Sort (``recsort.gather_frames``) — and ``sortvalidate -gpu``
end to end, cold and with the splits resident, against the classic job on 8
CPU slots over the same 8-file sort input and output.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_recsort import (random_text_records, random_writer_records, timed,  # noqa: E402
                           write_files)

from hbmr.benchmarks import sortvalidator  # noqa: E402
from hbmr.io.writable import BytesWritable, Text  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.models import sort as sort_job  # noqa: E402
from hbmr.ops import _lib, recsort, recvalidate  # noqa: E402


def passes(data, index, nparts, reps):
    """The warm passes over one split in HBM; rates are over the frame bytes
    (``torch.sum``: over the whole buffer, which holds nothing else here)."""
    n, nb = int(index.shape[1]), int(data.numel())
    frame_bytes = int(index[1].sum())
    want = recvalidate.digest(data, index)
    assert want[:2] == (n, frame_bytes - 8 * n)
    lib = _lib.load()
    out = torch.zeros(4, dtype=torch.int64, device=data.device)
    foff, flen = index[0], index[1]

    def kernel():
        _lib.check(lib.hbmr_recvalidate_digest(data.data_ptr(), foff.data_ptr(), flen.data_ptr(), n,
                                               out.data_ptr(), _lib.stream_handle()), "digest")

    kern = timed(kernel, reps)
    assert tuple(v & recvalidate.M64 for v in out.tolist()) == want
    call = timed(lambda: recvalidate.digest(data, index), reps)
    order = timed(lambda: recvalidate.check_sorted_part(data, index, nparts, None), reps)
    both = timed(lambda: recvalidate.check_sorted_part(data, index, nparts, 0), reps)
    words = data[:nb - nb % 8].view(torch.int64)
    read = timed(lambda: torch.sum(words), reps)
    dst = torch.cumsum(flen, 0) - flen
    gath = timed(lambda: recsort.gather_frames(data, None, foff, flen, dst, frame_bytes,
                                               check=False), reps)
    gbs = lambda s: round(frame_bytes / s / 1e9, 1)  # noqa: E731
    return {"records": n, "bytes": nb, "frame_bytes": frame_bytes,
            "digest_kernel_ms": round(kern * 1e3, 3), "digest_gb_per_s": gbs(kern),
            "digest_call_ms": round(call * 1e3, 3),
            "order_ms": round(order * 1e3, 3),
            "partition_ms": round((both - order) * 1e3, 3),
            "torch_sum_int64_ms": round(read * 1e3, 3),
            "torch_sum_gb_per_s": round(words.numel() * 8 / read / 1e9, 1),
            "gather_frames_ms": round(gath * 1e3, 3), "gather_gb_per_s_copied": gbs(gath),
            "digest_vs_torch_sum": round(read / kern, 3),
            "digest_vs_gather_frames": round(gath / kern, 3)}


def end_to_end(data, index, cls, files, tmp):
    inp, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    write_files(data, index, inp, cls, files)
    res = {"files_per_side": files, "records": int(index.shape[1]),
           "input_bytes": sum(os.path.getsize(os.path.join(inp, f)) for f in os.listdir(inp))}
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        rj = cl.submit_job(sort_job.gpu_job(inp, out, files, maps=files))
        assert rj.waitForCompletion(900) and rj.isSuccessful(), rj.getFailureInfo()
    print(f"# sorted into {files} parts", file=sys.stderr, flush=True)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("cold", "resident"):
            t = time.perf_counter()
            got = sortvalidator.validate(inp, out, cluster=cl, gpu=True)
            res[f"gpu_{run}_s"] = round(time.perf_counter() - t, 3)
            assert got["ok"], got
            print(f"# sortvalidate -gpu {run}: {res[f'gpu_{run}_s']} s", file=sys.stderr,
                  flush=True)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        want = sortvalidator.validate(inp, out, cluster=cl)
        res["classic_8_cpu_slots_s"] = round(time.perf_counter() - t, 3)
    print(f"# classic sortvalidate: {res['classic_8_cpu_slots_s']} s", file=sys.stderr, flush=True)
    res["same_result"] = got == want
    res["speedup_cold"] = round(res["classic_8_cpu_slots_s"] / res["gpu_cold_s"], 1)
    res["speedup_resident"] = round(res["classic_8_cpu_slots_s"] / res["gpu_resident_s"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="bytes in HBM per input")
    ap.add_argument("--e2e-mb", type=int, default=None,
                    help="bytes per input of the end-to-end jobs (default: --mb; 0: skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", type=int, default=4, help="partitions of the partition check")
    ap.add_argument("--files", type=int, default=8, help="files per side, end to end")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    e2e_mb = a.mb if a.e2e_mb is None else a.e2e_mb
    res = {"benchmark": "GPU SortValidator warm passes and end-to-end job (1 MI355X)",
           "reps": a.reps, "mb": a.mb, "e2e_mb": e2e_mb, "inputs": {}}
    for name, gen, cls in (("random_writer", random_writer_records, BytesWritable),
                           ("random_text_writer", random_text_records, Text)):
        data, index = gen(a.mb << 20)
        print(f"# {name}: {index.shape[1]} records generated", file=sys.stderr, flush=True)
        ent = {"passes": passes(torch.from_numpy(data).cuda(), torch.from_numpy(index).cuda(),
                                a.parts, a.reps)}
        print(f"# {name}: {json.dumps(ent['passes'])}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        if e2e_mb:
            if e2e_mb != a.mb:
                data, index = gen(e2e_mb << 20)
            tmp = tempfile.mkdtemp(prefix="bench-sortvalidate-")
            try:
                ent["end_to_end"] = end_to_end(data, index, cls, a.files, tmp)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        res["inputs"][name] = ent
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
