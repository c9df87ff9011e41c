"""GPU RandomWriter on one MI355X: the passes of hbmr/ops/recgen.py (lengths,
plan, fill) for RandomWriter's and RandomTextWriter's records at their default
shapes, next to two passes over the same bytes measured in the same run — a
write-only ``torch.Tensor.zero_()`` of a buffer of the body's size and the
variable-length record gather of GPU Sort (``recsort.gather_frames``) over the
same frames — and end to end ``randomwriter -gpu`` against the classic job on
8 CPU slots for 8 maps, then ``sort -gpu`` over the generated directory on the
same cluster (the parts resident in HBM) against ``sort -gpu`` over the same
files in a fresh cluster.  Prints one JSON line."""
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

from bench_recsort import timed  # noqa: E402

from hbmr.examples import randomwriter  # noqa: E402
from hbmr.examples import sort as sort_example  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.ops import _lib, recgen, recsort  # noqa: E402

GPU_GROUP = "hbmr.GpuCounters"
KINDS = (("random_writer", recgen.BYTES, (10, 1000, 0, 20000), None),
         ("random_text_writer", recgen.TEXT, (5, 10, 10, 100), randomwriter._WORDS))


def passes(kind, params, words, target, reps):
    """The passes of one map of ``target`` payload bytes; rates are over the
    frame bytes (``zero_``: over the whole body, sync holes included)."""
    dev = torch.device("cuda", 0)
    voc = recgen.Vocabulary(words) if words else None
    p = recgen.plan(kind, 0, 0, 0, target, params, dev, vocabulary=voc)
    n, total = int(p.index.shape[1]), p.total
    frame_bytes = int(p.index[1].sum())
    data = torch.zeros(total, dtype=torch.uint8, device=dev)
    recgen.fill(kind, 0, 0, 0, p.index, data, params, voc)
    # the head of the body is the twin's
    want, windex = recgen.generate_cpu(kind, 0, 0, min(target, 4 << 20), params, voc)
    k = int(windex.shape[1]) - 1
    assert torch.equal(p.index[:, :k].cpu(), windex[:, :k])
    head = int(windex[0, k])
    assert torch.equal(data[:head].cpu(), want[:head])
    lens = timed(lambda: recgen.lengths(kind, 0, 0, 0, n, params, dev, voc), reps)
    plan = timed(lambda: recgen.plan(kind, 0, 0, 0, target, params, dev, vocabulary=voc), reps)
    call = timed(lambda: recgen.fill(kind, 0, 0, 0, p.index, data, params, voc), reps)
    lib = _lib.load()
    foff, flen, koff, klen = (r.contiguous() for r in p.index)
    S = recgen.split_word(0, 0)
    if kind == recgen.BYTES:
        base, entry, nch = recsort._chunk_table(foff, flen, data,
                                                chunk=int(lib.hbmr_recgen_chunk_bytes()))

        def kernel():
            _lib.check(lib.hbmr_recgen_fill_bytes(S, 0, foff.data_ptr(), flen.data_ptr(),
                                                  klen.data_ptr(), base.data_ptr(),
                                                  entry.data_ptr(), n, nch, data.data_ptr(),
                                                  _lib.stream_handle()), "fill_bytes")
    else:
        blob, woff = voc.on(dev)

        def kernel():
            _lib.check(lib.hbmr_recgen_fill_text(S, 0, n, *recgen._ranges(params),
                                                 blob.data_ptr(), woff.data_ptr(), len(voc.words),
                                                 int(voc.blob.size), foff.data_ptr(),
                                                 flen.data_ptr(), klen.data_ptr(), data.data_ptr(),
                                                 _lib.stream_handle()), "fill_text")
    kern = timed(kernel, reps)
    other = torch.empty_like(data)
    zero = timed(other.zero_, reps)
    gath = timed(lambda: recsort.gather_frames(data, None, foff, flen, foff, total, check=False,
                                               out=other), reps)
    last = int(foff[-1])
    assert torch.equal(other[last:], data[last:])
    gbs = lambda s: round(frame_bytes / s / 1e9, 1)  # noqa: E731
    return {"records": n, "body_bytes": total, "frame_bytes": frame_bytes,
            "lengths_ms": round(lens * 1e3, 3), "plan_ms": round(plan * 1e3, 3),
            "fill_call_ms": round(call * 1e3, 3), "fill_kernel_ms": round(kern * 1e3, 3),
            "fill_gb_per_s": gbs(kern),
            "zero_ms": round(zero * 1e3, 3), "zero_gb_per_s": round(total / zero / 1e9, 1),
            "gather_frames_ms": round(gath * 1e3, 3), "gather_gb_per_s_copied": gbs(gath),
            "fill_vs_zero": round(zero / kern, 3), "fill_vs_gather_frames": round(gath / kern, 3)}


def end_to_end(text, per_map, maps, tmp):
    gen, out = os.path.join(tmp, "gen"), os.path.join(tmp, "out")
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    conf.set_num_map_tasks(1)                          # the sort takes whole files
    res = {"maps": maps, "bytes_per_map": per_map}

    def sort(cl, where, name):
        t = time.perf_counter()
        rj = sort_example.run(gen, where, maps, conf=conf, cluster=cl, gpu=True)
        res[f"sort_gpu_{name}_s"] = round(time.perf_counter() - t, 3)
        assert rj.isSuccessful()
        cs = rj.getCounters()
        res[f"sort_gpu_{name}_cache_hits"] = cs.get(GPU_GROUP, "GPU_SPLIT_CACHE_HITS")
        res[f"sort_gpu_{name}_cache_misses"] = cs.get(GPU_GROUP, "GPU_SPLIT_CACHE_MISSES")
        print(f"# sort -gpu {name}: {res[f'sort_gpu_{name}_s']} s", file=sys.stderr, flush=True)

    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("first", "warm"):                  # first: code objects load, HBM is claimed
            shutil.rmtree(gen, ignore_errors=True)
            t = time.perf_counter()
            rj = randomwriter.run(gen, maps, per_map, text, 0, conf=conf, cluster=cl, gpu=True)
            res[f"gpu_{run}_s"] = round(time.perf_counter() - t, 3)
            assert rj.isSuccessful()
            print(f"# randomwriter -gpu {run}: {res[f'gpu_{run}_s']} s", file=sys.stderr,
                  flush=True)
        res["output_bytes"] = sum(os.path.getsize(os.path.join(gen, f)) for f in os.listdir(gen))
        sort(cl, out + "-resident", "same_cluster")
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        sort(cl, out + "-fresh", "fresh_cluster")
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        rj = randomwriter.run(os.path.join(tmp, "classic"), maps, per_map, text, cluster=cl)
        res["classic_8_cpu_slots_s"] = round(time.perf_counter() - t, 3)
        assert rj.isSuccessful()
    print(f"# classic: {res['classic_8_cpu_slots_s']} s", file=sys.stderr, flush=True)
    res["speedup_warm"] = round(res["classic_8_cpu_slots_s"] / res["gpu_warm_s"], 1)
    res["sort_resident_vs_fresh"] = round(res["sort_gpu_fresh_cluster_s"] /
                                          res["sort_gpu_same_cluster_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="payload bytes of the kernel passes")
    ap.add_argument("--e2e-mb", type=int, default=256,
                    help="payload bytes of the end-to-end jobs, over all maps (0: skip)")
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randomwriter needs a GPU")
    res = {"benchmark": "GPU RandomWriter passes and end-to-end jobs (1 MI355X)",
           "reps": a.reps, "mb": a.mb, "e2e_mb": a.e2e_mb, "kinds": {}}
    for name, kind, params, words in KINDS:
        ent = {"params": list(params), "passes": passes(kind, params, words, a.mb << 20, a.reps)}
        print(f"# {name}: {json.dumps(ent['passes'])}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        if a.e2e_mb:
            tmp = tempfile.mkdtemp(prefix="bench-randomwriter-")
            try:
                ent["end_to_end"] = end_to_end(kind == recgen.TEXT, (a.e2e_mb << 20) // a.maps,
                                               a.maps, tmp)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        res["kinds"][name] = ent
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
