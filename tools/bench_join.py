"""GPU Join on one MI355X: the warm map pipeline of hbmr/ops/recjoin.py (group
heads → cross ranks → plan → tuple expansion → headers and piece copy) over two
sorted sources in HBM, made from RandomWriter- and RandomTextWriter-shaped
records (tools/bench_recsort.py) by ``sort -gpu``'s own ops with about half of
each source's keys in the other; once with unique keys and once with every
record twice (2 x 2 tuples per shared key).  In the same run: a plain device
copy of the output bytes and ``recsort.gather_frames`` over the output frames
(the floor and the existing gather the emit stage is judged against), the rank
kernel with and without its round-key level, and ``join -gpu`` end to end, cold
and with the splits resident, against the classic job on 8 CPU slots over the
same 8-part inputs.  Prints one JSON line."""
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

from bench_recsort import random_text_records, random_writer_records  # noqa: E402
from hbmr.examples import join as join_example  # noqa: E402
from hbmr.io import sequencefile as seqf  # noqa: E402
from hbmr.io.writable import BytesWritable, Text  # noqa: E402
from hbmr.mapred import JobConf  # noqa: E402
from hbmr.mapred.cluster import LocalCluster  # noqa: E402
from hbmr.models import join as join_job  # noqa: E402
from hbmr.ops import recjoin, recsort  # noqa: E402


def timed(fn, reps):
    """Best of ``reps`` in ms, by device events around warmed launches."""
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def sorted_source(data, index, nparts=1):
    """(blob, index over blob, records per partition): the records ordered by
    (partition, key) with sort -gpu's ops."""
    perm, recs, _, blob = recsort.sort_records(data, index, nparts)
    p = perm.long()
    flen = index[1][p]
    foff = torch.cumsum(flen, 0) - flen
    idx = torch.stack([foff, flen, foff + (index[2] - index[0])[p], index[3][p]]).contiguous()
    return blob, idx, recs


def two_sources(data, index, twice):
    """Records [0, 2n/3) and [n/3, n) of one input: half of each source's keys
    are in the other.  ``twice``: every record two times."""
    n = index.shape[1]
    a, b = index[:, :2 * n // 3], index[:, n // 3:]
    if twice:
        a, b = a.repeat_interleave(2, dim=1), b.repeat_interleave(2, dim=1)
    return a.contiguous(), b.contiguous()


def map_pipeline(sources, vcls, op, reps):
    headers = recjoin.tuple_headers([vcls, vcls])
    nin = sum(int(d.numel()) for d, _ in sources)
    stats = {}
    p = recjoin.plan(sources, op, stats=stats)
    em = recjoin._Emitter(p, headers)
    ex = em.expand(0, p.total)
    dst = torch.cumsum(ex[2], 0) - ex[2]
    nout = int(ex[2].sum())
    out = torch.empty(nout, dtype=torch.uint8, device="cuda")
    heads = [torch.nonzero(recjoin.group_heads(d, i, check=False)[0]).flatten().to(torch.int32)
             for d, i in sources]
    pr = [(sources[s][0], sources[s][1], heads[s]) for s in range(2)]

    def ranks():
        recjoin.rank_heads(pr[0], pr[1], check=False)
        recjoin.rank_heads(pr[1], pr[0], check=False)

    def whole():
        q = recjoin.plan(sources, op)
        e = recjoin._Emitter(q, headers)
        x = e.expand(0, q.total)
        e.fill(x, torch.cumsum(x[2], 0) - x[2], nout, out)

    res = {"op": op, "input_records": [int(i.shape[1]) for _, i in sources], "input_bytes": nin,
           "keys": stats["keys"], "groups": stats["groups"], "tuples": p.total,
           "output_bytes": nout}
    res["heads_ms"] = round(timed(lambda: [recjoin.group_heads(d, i, check=False)
                                           for d, i in sources], reps), 3)
    ab = {True: float("inf"), False: float("inf")}
    for _ in range(2):                                # the two rank variants alternating
        for two_level in (True, False):
            recjoin.set_two_level(two_level)
            ab[two_level] = min(ab[two_level], timed(ranks, reps))
    recjoin.set_two_level(True)
    res["rank_ms"] = round(ab[True], 3)
    res["rank_ms_plain_search"] = round(ab[False], 3)
    res["plan_ms"] = round(timed(lambda: recjoin.plan(sources, op), reps), 3)
    res["expand_ms"] = round(timed(lambda: em.expand(0, p.total), reps), 3)
    pieces = em.pieces(ex, dst, out)
    res["headers_ms"] = round(timed(lambda: em.pieces(ex, dst, out), reps), 3)
    # the copy: one launch over pieces that name their source by address, against
    # recsort's gather called per source for the values and per owner for the keys
    S, T = len(sources), int(ex[0].numel())
    pdst = pieces[2].view(T, S + 1)
    own_src, own_rec = p.osrc[ex[0].long()], p.orec[ex[0].long()]
    # per source: where a record's value and its serialized key lie
    spans = [(koff + klen, foff + flen - koff - klen, foff + 8, koff + klen - foff - 8)
             for foff, flen, koff, klen in p.rows]

    def reused():
        for s, (data, _) in enumerate(sources):
            voff, vlen, kstart, kser = spans[s]
            sel = torch.nonzero(ex[1][s] >= 0).flatten()
            recsort.gather_frames(data, ex[1][s][sel], voff, vlen, pdst[:, 1 + s][sel], nout,
                                  check=False, out=other)
            sel = torch.nonzero(own_src == s).flatten()
            recsort.gather_frames(data, own_rec[sel], kstart, kser, pdst[:, 0][sel], nout,
                                  check=False, out=other)

    em.copy(pieces, out)
    other = out.clone()                               # headers in place; the pieces again
    reused()
    assert torch.equal(other, out)
    ab = {"new": float("inf"), "reused": float("inf")}
    for _ in range(2):                                # alternating
        ab["new"] = min(ab["new"], timed(lambda: em.copy(pieces, out), reps))
        ab["reused"] = min(ab["reused"], timed(reused, reps))
    del other
    res["piece_copy_ms"] = round(ab["new"], 3)
    res["piece_copy_ms_recsort_gather_per_source"] = round(ab["reused"], 3)
    best = {"frames": res["headers_ms"], "copy": ab["new"]}
    total = timed(whole, reps)
    res["pipeline_ms"] = round(total, 3)
    res["pipeline_gb_per_s_in_plus_out"] = round((nin + nout) / total / 1e6, 2)
    emit = best["frames"] + best["copy"]
    res["emit_gb_per_s_written"] = round(nout / emit / 1e6, 1)
    # the floor and the existing gather, over the same output frames
    copy = timed(lambda: out.clone(), reps)
    gath = timed(lambda: recsort.gather_frames(out, None, dst, ex[2], dst, nout, check=False), reps)
    res["device_copy_ms"] = round(copy, 3)
    res["gather_frames_ms"] = round(gath, 3)
    res["emit_vs_device_copy"] = round(copy / emit, 3)
    res["emit_vs_gather_frames"] = round(gath / emit, 3)
    res["pipeline_vs_device_copy"] = round(copy / total, 3)
    res["pipeline_vs_gather_frames"] = round(gath / total, 3)
    return res


def write_parts(dirname, blob, idx, recs, cls):
    os.makedirs(dirname)
    blob, idx = blob.cpu(), idx.cpu()
    r0 = 0
    for p, n in enumerate(recs):
        with seqf.Writer(os.path.join(dirname, f"part-{p:05d}"), cls, cls) as w:
            recsort.write_part(w, blob, idx, torch.arange(r0, r0 + n, dtype=torch.int32))
        r0 += n


def end_to_end(data, index, cls, parts, tmp, op="outer"):
    dirs = []
    for s, ix in enumerate(two_sources(data, index, False)):
        blob, idx, recs = sorted_source(data, ix, parts)
        dirs.append(os.path.join(tmp, f"src{s}"))
        write_parts(dirs[-1], blob, idx, recs, cls)
    res = {"op": op, "parts": parts, "input_bytes": sum(
        os.path.getsize(os.path.join(d, f)) for d in dirs for f in os.listdir(d))}
    print(f"# files written ({res['input_bytes']} bytes)", file=sys.stderr, flush=True)
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for run in ("cold", "warm"):
            t = time.perf_counter()
            rj = cl.submit_job(join_job.gpu_job(dirs, os.path.join(tmp, f"gpu-{run}"), op))
            assert rj.waitForCompletion(900) and rj.isSuccessful(), rj.getFailureInfo()
            res[f"split_job_{run}_s"] = round(time.perf_counter() - t, 3)
            print(f"# split job {run}: {res[f'split_job_{run}_s']} s", file=sys.stderr, flush=True)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=8) as cl:
        t = time.perf_counter()
        rj = join_example.run(dirs, os.path.join(tmp, "classic"), op, cluster=cl, out_key=cls)
        assert rj.isSuccessful()
        res["classic_job_s"] = round(time.perf_counter() - t, 3)
    print(f"# classic job: {res['classic_job_s']} s", file=sys.stderr, flush=True)
    same, n = True, 0
    for p in range(parts):
        got = []
        for d in ("gpu-warm", "classic"):
            recs = []
            with seqf.Reader(os.path.join(tmp, d, f"part-{p:05d}")) as r:
                while True:
                    raw = r.next_raw()
                    if raw is None:
                        break
                    recs.append(raw)
            got.append(recs)
        same = same and got[0] == got[1]
        n += len(got[0])
    res["output_records"] = n
    res["same_records_per_part"] = same
    res["split_job_faster"] = max(res["split_job_cold_s"], res["split_job_warm_s"]) < \
        res["classic_job_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=384, help="bytes of each generated input")
    ap.add_argument("--e2e-mb", type=int, default=96,
                    help="bytes of each input of the end-to-end jobs (0: skip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = {"benchmark": "GPU Join warm map pipeline and end-to-end job (1 MI355X)",
           "reps": a.reps, "inputs": {}}
    for name, gen, cls in (("random_writer", random_writer_records, BytesWritable),
                           ("random_text_writer", random_text_records, Text)):
        ent = {}
        for case, twice, mb in (("unique_keys", False, a.mb), ("every_record_twice", True,
                                                               a.mb // 4)):
            data, index = gen(mb << 20)
            data, index = torch.from_numpy(data).cuda(), torch.from_numpy(index).cuda()
            sources = [sorted_source(data, ix)[:2] for ix in two_sources(data, index, twice)]
            del data, index
            for op in ("inner", "outer"):
                ent[f"{case}_{op}"] = map_pipeline(sources, cls, op, a.reps)
                print(f"# {name} {case} {op}: {json.dumps(ent[f'{case}_{op}'])}", file=sys.stderr,
                      flush=True)
            del sources
            torch.cuda.empty_cache()
        if a.e2e_mb:
            data, index = gen(a.e2e_mb << 20)
            tmp = tempfile.mkdtemp(prefix="bench-join-")
            try:
                ent["end_to_end"] = end_to_end(torch.from_numpy(data).cuda(),
                                               torch.from_numpy(index).cuda(), cls, a.parts, tmp)
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
