"""GPU SortValidator (split-level job, native/kernels/recvalidate.hip): the
record digest's twin against the definition, its sensitivity and invariances,
the order and partition checks against Python ``bytes`` comparison and
HashPartitioner, the job's result against the classic SortValidator's on sound
and tampered sort outputs, and the kernels against the twins."""
import logging
import os
import random
import shutil

import numpy as np
import pytest
import torch
from test_sort_gpu import ADVERSARIAL, _build, _write

from hbmr.benchmarks import sortvalidator
from hbmr.examples import randomwriter
from hbmr.examples import sort as sort_example
from hbmr.io import sequencefile as seqf
from hbmr.io.writable import BytesWritable, IntWritable, Text
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.lib.basic import HashPartitioner
from hbmr.models import sort as sort_job
from hbmr.models import sortvalidate as validate_job
from hbmr.ops import recsort, recvalidate

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------- the definition
def _mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def _frame_hash(fr):
    s = 0
    for j in range((len(fr) + 7) // 8):
        w = int.from_bytes(fr[8 * j:8 * j + 8], "little")
        s = (s + _mix((w + (j + 1) * 0x9E3779B97F4A7C15) & M64)) & M64
    return _mix(s ^ (len(fr) * 0xD6E8FEB86659FD93 & M64))


def _digest_by_definition(data, index):
    hs = [_frame_hash(f) for f in recsort.frames(data, index)]
    return (len(hs), sum(len(f) - 8 for f in recsort.frames(data, index)), sum(hs) & M64,
            sum(h * h for h in hs) & M64)


def _mixed_records(n, seed):
    rnd = random.Random(seed)
    keys = [rnd.randbytes(rnd.choice((0, 1, 7, 8, 9, 30, 200))) for _ in range(n)]
    vals = [rnd.randbytes(rnd.choice((0, 1, 3, 4, 5, 12, 13, 64, 700))) for _ in range(n)]
    if n > 2:
        keys[1], vals[1] = b"", b""
    return keys, vals


# ----------------------------------------------------------------------------- CPU: digest
@pytest.mark.parametrize("kind", ["bytes", "text"])
def test_digest_twin_equals_definition(kind):
    keys, vals = _mixed_records(300, 11)
    data, index = _build(keys, vals, kind)
    want = _digest_by_definition(data, index)
    assert want[0] == 300 and want[1] == int(index[1].sum()) - 8 * 300
    assert {int(x) % 8 for x in index[1]} == set(range(8))       # every tail length
    assert recvalidate.digest_cpu(data, index) == want
    assert recvalidate.digest(data, index) == want                # host tensors: the twin
    for n in (0, 1, 2):
        data, index = _build(keys[:n], vals[:n], kind, junk_every=1)
        assert recvalidate.digest_cpu(data, index) == _digest_by_definition(data, index)
    assert recvalidate.digest_cpu(*_build([], [])) == (0, 0, 0, 0)
    data, index = _build([b""], [b""], kind)                     # empty key and value
    assert recvalidate.digest_cpu(data, index)[:2] == (1, int(index[1][0]) - 8)
    assert recvalidate.digest_cpu(data, index)[2] == _frame_hash(bytes(data.numpy()))


def test_digest_twin_in_batches(monkeypatch):
    keys, vals = _mixed_records(300, 12)
    data, index = _build(keys, vals)
    want = recvalidate.digest_cpu(data, index)
    monkeypatch.setattr(recvalidate, "_BATCH_WORDS", 50)
    assert recvalidate.digest_cpu(data, index) == want == _digest_by_definition(data, index)


def test_digest_rejects_index_outside_data():
    data, index = _build([b"k1", b"k2"], [b"v", b"w"])
    for row, val in ((0, -1), (1, int(data.numel())), (2, int(data.numel())), (3, -2)):
        bad = index.clone()
        bad[row, 1] = val
        with pytest.raises(ValueError, match="record index points outside the data"):
            recvalidate.digest(data, bad)
        with pytest.raises(ValueError, match="record index points outside the data"):
            recvalidate.check_sorted_part(data, bad, 3, 0)


def test_digest_sees_every_bit_of_a_frame():
    data, index = _build([b"key-of-11-b"], [b"value-14-bytes"])
    assert int(index[1][0]) == 41 and data.numel() == 41
    base = recvalidate.digest_cpu(data, index)
    seen = {base[2]}
    for bit in range(328):
        d = data.clone()
        d[bit // 8] ^= 1 << (bit % 8)
        got = recvalidate.digest_cpu(d, index)
        assert got[:2] == base[:2] and got[2] not in seen, bit
        seen.add(got[2])


def test_digest_sees_words_and_values_traded_between_records():
    rnd = random.Random(3)
    keys = [rnd.randbytes(20), rnd.randbytes(20)]
    vals = [rnd.randbytes(28), rnd.randbytes(28)]
    data, index = _build(keys, vals, junk_every=2)
    assert index[1].tolist() == [64, 64]
    base = recvalidate.digest_cpu(data, index)
    a, b = index[0].tolist()
    for j in range(2, 8):                     # words 0 and 1 are equal: lengths and the key's own
        d = data.clone()
        d[a + 8 * j:a + 8 * j + 8] = data[b + 8 * j:b + 8 * j + 8]
        d[b + 8 * j:b + 8 * j + 8] = data[a + 8 * j:a + 8 * j + 8]
        got = recvalidate.digest_cpu(d, index)
        assert got[:2] == base[:2] and got[2] != base[2], j
    swapped = recvalidate.digest_cpu(*_build(keys, vals[::-1], junk_every=2))
    assert swapped[:2] == base[:2] and swapped[2] != base[2]


def test_digest_ignores_record_order_and_junk():
    keys, vals = _mixed_records(200, 4)
    base = recvalidate.digest_cpu(*_build(keys, vals))
    order = list(range(200))
    random.Random(5).shuffle(order)
    for junk_every in (0, 1, 3):
        data, index = _build([keys[i] for i in order], [vals[i] for i in order],
                             junk_every=junk_every)
        assert recvalidate.digest_cpu(data, index) == base
    covered = np.zeros(data.numel(), dtype=bool)
    for o, n in zip(index[0].tolist(), index[1].tolist()):
        covered[o:o + n] = True
    assert (~covered).sum() == 20 * (200 // 3)
    data[torch.from_numpy(~covered)] = 0x5A
    assert recvalidate.digest_cpu(data, index) == base


def test_digest_twin_is_vectorised():
    import time
    n = 100_000
    rng = np.random.default_rng(0)
    flen = rng.integers(16, 400, n)
    foff = np.cumsum(flen) - flen
    data = torch.from_numpy(rng.integers(0, 256, int(flen.sum()), dtype=np.uint8))
    index = torch.from_numpy(np.stack([foff, flen, foff + 8, flen - 8]).astype(np.int64))
    took = float("inf")
    for _ in range(3):                        # the first call also pays for fresh pages
        t = time.perf_counter()
        got = recvalidate.digest_cpu(data, index)
        took = min(took, time.perf_counter() - t)
    assert got[:2] == (n, int(flen.sum()) - 8 * n)
    few = torch.tensor([0, 1, n // 2, n - 1])
    assert recvalidate.digest_cpu(data, index[:, few])[2] == \
        sum(_frame_hash(f) for f in recsort.frames(data, index[:, few])) & M64
    print(f"digest_cpu: {n} records, {int(flen.sum())} bytes in {took:.3f} s")
    assert took < 1.0          # a Python step per record would take longer than that


# ----------------------------------------------------------------------------- CPU: order, part
PAYLOADS = ADVERSARIAL + [b"abcdefgh\0", b"abcdefghi", b"abcdefgh\x80", b"\xff" * 9, b"\0" * 9]


def _adversarial_keys(n, seed):
    rnd = random.Random(seed)
    keys = [rnd.choice(PAYLOADS) for _ in range(n)]
    for i in range(3, n, 5):
        keys[i] = keys[i - 1]                 # equal neighbours
    return keys


@pytest.mark.parametrize("kind", ["bytes", "text"])
def test_check_sorted_part_twin_equals_python(kind):
    assert {len(k) for k in PAYLOADS} >= {0, 7, 8, 9}
    keys = _adversarial_keys(400, 2)
    data, index = _build(keys, [b"v%d" % i for i in range(400)], kind)
    descents = sum(1 for a, b in zip(keys, keys[1:]) if b < a)
    equal = sum(1 for a, b in zip(keys, keys[1:]) if b == a)
    assert descents > 100 and equal >= 79
    wr = BytesWritable if kind == "bytes" else Text
    hp = HashPartitioner()
    for nparts, part in ((3, 0), (3, 2), (7, 4), (1, 0)):
        mis = sum(1 for k in keys if hp.getPartition(wr(k), None, nparts) != part)
        assert recvalidate.check_sorted_part_cpu(data, index, nparts, part) == (descents, mis)
        assert recvalidate.check_sorted_part(data, index, nparts, part) == (descents, mis)
    assert recvalidate.check_sorted_part_cpu(data, index, 3, None) == (descents, 0)
    srt = sorted(keys)
    data, index = _build(srt, [b""] * 400, kind)
    assert recvalidate.check_sorted_part_cpu(data, index, 1, 0) == (0, 0)
    for n in (0, 1):
        few = _build(srt[:n], [b""] * n, kind)
        assert recvalidate.check_sorted_part_cpu(*few, 3, None) == (0, 0)


# ----------------------------------------------------------------------------- the job
def _local():
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    return conf


def _read_raw(path):
    with seqf.Reader(path) as r:
        return r.key_class, r.value_class, list(iter(r.next_raw, None))


def _rewrite(path, kc, vc, recs):
    with seqf.Writer(path, kc, vc) as w:
        for kb, vb in recs:
            w.append_raw(kb, vb)


@pytest.fixture(scope="module")
def sorted_dirs(tmp_path_factory):
    """RandomWriter input, its hash-partitioned and its totally ordered sort."""
    base = tmp_path_factory.mktemp("sv")
    inp = str(base / "in")
    JobClient.runJob(randomwriter.make_job(inp, maps=2, bytes_per_map=200_000), verbose=False)
    JobClient.runJob(sort_example.make_job(inp, str(base / "out"), reduces=3), verbose=False)
    sort_example.run(inp, str(base / "total"), 3, (0.5, 1000, 10), conf=_local())
    return base


@pytest.fixture(scope="module")
def cpu_cluster():
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        yield cl


def _copy(sorted_dirs, tmp_path, out="out"):
    shutil.copytree(sorted_dirs / "in", tmp_path / "in")
    shutil.copytree(sorted_dirs / out, tmp_path / "out")
    return str(tmp_path / "in"), str(tmp_path / "out")


def _both(inp, out, cluster, total_order=False):
    """The split job's result, checked against the classic job's."""
    want = sortvalidator.validate(inp, out, total_order=total_order)
    got = sortvalidator.validate(inp, out, cluster=cluster, total_order=total_order, gpu=True)
    assert got == want and list(got) == list(want)
    return got


def _tamper(out, case):
    p0, p1 = os.path.join(out, "part-00000"), os.path.join(out, "part-00001")
    kc, vc, recs = _read_raw(p1)
    assert len(recs) >= 3 and len({k for k, _ in recs[:3]}) == 3
    if case == "swap":
        recs[0], recs[1] = recs[1], recs[0]
    elif case == "drop":
        del recs[1]
    elif case == "move":
        _, _, other = _read_raw(p0)
        recs = sorted(recs + [other.pop(0)], key=lambda kv: kc.raw_sort_key(kv[0]))
        _rewrite(p0, kc, vc, other)
    elif case == "value-byte":
        i = next(i for i, (_, vb) in enumerate(recs) if len(vb) > 4)
        kb, vb = recs[i]
        recs[i] = (kb, vb[:-1] + bytes([vb[-1] ^ 0x10]))
    elif case == "exchange-parts":
        os.replace(p0, p0 + ".tmp")
        os.replace(p1, p0)
        os.replace(p0 + ".tmp", p1)
        return
    _rewrite(p1, kc, vc, recs)


def _check_case(res, case):
    if case == "sound":
        assert res["ok"] and res["IN_RECORDS"] == res["OUT_RECORDS"] > 10
    elif case == "swap":
        assert not res["ok"] and res["UNSORTED_RECORDS"] == 1 and res["checksum_match"]
        assert res["MISPARTITIONED_RECORDS"] == 0
    elif case == "drop":
        assert not res["ok"] and res["IN_RECORDS"] == res["OUT_RECORDS"] + 1
        assert not res["checksum_match"] and res["UNSORTED_RECORDS"] == 0
    elif case == "move":
        assert not res["ok"] and res["MISPARTITIONED_RECORDS"] == 1 and res["checksum_match"]
        assert res["UNSORTED_RECORDS"] == 0
    elif case == "value-byte":
        assert not res["ok"] and not res["checksum_match"]
        assert res["IN_RECORDS"] == res["OUT_RECORDS"] and res["IN_BYTES"] == res["OUT_BYTES"]
        assert res["UNSORTED_RECORDS"] == res["MISPARTITIONED_RECORDS"] == 0
    elif case == "exchange-parts":
        assert not res["ok"] and res["RANGE_OVERLAPS"] >= 1 and res["checksum_match"]
        assert res["UNSORTED_RECORDS"] == 0 and "MISPARTITIONED_RECORDS" in res


@pytest.mark.parametrize("case", ["sound", "swap", "drop", "move", "value-byte"])
def test_job_on_cpu_slots_equals_classic(sorted_dirs, cpu_cluster, tmp_path, case):
    inp, out = _copy(sorted_dirs, tmp_path)
    if case != "sound":
        _tamper(out, case)
    _check_case(_both(inp, out, cpu_cluster), case)


@pytest.mark.parametrize("case", ["sound", "exchange-parts"])
def test_job_on_cpu_slots_total_order(sorted_dirs, cpu_cluster, tmp_path, case):
    inp, out = _copy(sorted_dirs, tmp_path, "total")
    if case != "sound":
        _tamper(out, case)
    res = _both(inp, out, cpu_cluster, total_order=True)
    assert "RANGE_OVERLAPS" in res
    _check_case(res, case)


def test_job_splits_are_whole_files_under_sort_keys(sorted_dirs):
    inp, out = str(sorted_dirs / "in"), str(sorted_dirs / "out")
    job = validate_job.gpu_job(inp, out)
    sj = validate_job.ValidateSplitJob()
    sj.configure(job)
    assert sj.needs_reduce is False
    splits = sj.get_splits(job, ["t0"])
    files = sorted(os.path.join(d, f) for d in (inp, out) for f in os.listdir(d)
                   if f.startswith("part-"))
    assert sorted(s.params["path"] for s in splits) == files and len(files) == 5
    for s in splits:
        size = os.path.getsize(s.params["path"])
        assert s.key == f"sort:{s.params['path']}:0:{size}"
        assert (s.params["start"], s.params["length"]) == (0, size)
    # GPU Sort's own key for a file it reads as one split
    sort_conf = sort_example.make_job(inp, out + "x")
    sort_conf.set_num_map_tasks(1)
    sort_splits = sort_job.SortSplitJob().get_splits(sort_conf, [])
    assert {s.key for s in sort_splits} == {s.key for s in splits if "/in/" in s.key}
    assert sj.side_of(files[0]) == ("IN", None)
    assert sj.side_of(os.path.join(out, "part-00002")) == ("OUT", 2)
    split = sj.load_split(splits[0], "cpu")
    assert sorted(split) == ["data", "index"]


def test_ineligible_directories_run_the_classic_job(tmp_path, caplog, capsys):
    rnd = random.Random(7)
    recs = [(rnd.randbytes(rnd.randint(0, 40)), rnd.randbytes(rnd.randint(0, 90)))
            for _ in range(40)]
    comp, ints, plain = tmp_path / "comp", tmp_path / "ints", tmp_path / "plain"
    for d in (comp, ints, plain):
        d.mkdir()
    _write(comp / "part-00000", recs, compression="RECORD")
    _write(plain / "part-00000", recs)
    with seqf.Writer(str(ints / "part-00000"), IntWritable, BytesWritable) as w:
        for i, (_, v) in enumerate(recs):
            w.append(IntWritable((i * 37) % 41 - 20), BytesWritable(v))
    local = _local()
    for name, d in (("comp", comp), ("ints", ints), ("plain", plain)):
        sort_example.run(str(d), str(tmp_path / f"{name}-out"), 2, conf=local)
    with pytest.raises(ValueError, match="RECORD-compressed"):
        validate_job.gpu_job(str(comp), str(tmp_path / "comp-out"))
    with pytest.raises(ValueError, match="key class org.apache.hadoop.io.IntWritable"):
        validate_job.gpu_job(str(ints), str(tmp_path / "ints-out"))
    with pytest.raises(ValueError, match="RECORD-compressed"):          # the output side alone
        validate_job.gpu_job(str(plain), str(comp))
    with pytest.raises(ValueError, match="is not a local file"):
        validate_job.gpu_job(str(tmp_path), str(tmp_path / "plain-out"))
    texts = tmp_path / "texts"
    texts.mkdir()
    _write(texts / "part-00000", recs, Text, BytesWritable)
    with pytest.raises(ValueError, match="different key/value classes"):
        validate_job.gpu_job(str(texts), str(tmp_path / "plain-out"))
    assert validate_job.gpu_job(str(plain), str(tmp_path / "plain-out")).get_num_reduce_tasks() == 0
    for name, d in (("comp", comp), ("ints", ints)):
        out = str(tmp_path / f"{name}-out")
        want = sortvalidator.validate(str(d), out, conf=local)
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="hbmr.benchmarks.sortvalidator"):
            got = sortvalidator.validate(str(d), out, conf=local, gpu=True)
        assert "not eligible for the GPU" in caplog.text and "classic sortvalidate" in caplog.text
        assert got == want and got["ok"] and got["IN_RECORDS"] == len(recs)
        args = ["-sortInput", str(d), "-sortOutput", out, "-gpu"]
        assert sortvalidator.main(args) == 0
        kc, vc, raw = _read_raw(os.path.join(out, "part-00001"))
        _rewrite(os.path.join(out, "part-00001"), kc, vc, raw[1:])
        assert sortvalidator.main(args) == 1
        assert "FAILED" in capsys.readouterr().out


# ----------------------------------------------------------------------------- GPU
def _alignment_case():
    """Frames of the lengths at which the digest kernel changes its path (a
    partial last slot, whole slots, whole and partial steps of 256 bytes, many
    steps) at every start misalignment 0-15, junk in between, the last frame
    ending on the buffer's last byte."""
    rnd = random.Random(21)
    lens = list(range(16, 49)) + [255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 20000]
    parts, foff, flen, off = [], [], [], 0
    for mis in range(16):
        for ln in lens:
            pad = (mis - off) % 16 or 16
            parts.append(b"\xff" * pad)
            off += pad
            parts.append(rnd.randbytes(ln))
            foff.append(off)
            flen.append(ln)
            off += ln
    raw = b"".join(parts)
    assert foff[-1] + flen[-1] == len(raw)
    assert {(o % 16, n) for o, n in zip(foff, flen)} == {(m, n) for m in range(16) for n in lens}
    foff, flen = np.array(foff), np.array(flen)
    index = np.stack([foff, flen, foff + 8, flen - 8]).astype(np.int64)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8), torch.from_numpy(index)


@pytest.mark.gpu
def test_gpu_digest_every_alignment_and_length():
    data, index = _alignment_case()
    want = recvalidate.digest_cpu(data, index)
    assert want == _digest_by_definition(data, index)
    pad = torch.zeros(data.numel() + 1, dtype=torch.uint8, device="cuda")
    for shift in (0, 1):                      # the buffer itself aligned and not
        buf = pad[shift:shift + data.numel()]
        buf.copy_(data)
        assert buf.data_ptr() % 16 == shift
        assert recvalidate.digest(buf, index.cuda()) == want
    one = index[:, -1:].contiguous()          # the frame that ends the buffer, alone
    assert recvalidate.digest(data.cuda(), one.cuda()) == recvalidate.digest_cpu(data, one)
    with pytest.raises(ValueError, match="record index points outside the data"):
        bad = index.clone()
        bad[1, -1] += 1
        recvalidate.digest(data.cuda(), bad.cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_gpu_digest_small(n):
    keys, vals = _mixed_records(n, 30 + n)
    for kind in ("bytes", "text"):
        data, index = _build(keys, vals, kind, junk_every=3)
        assert recvalidate.digest(data.cuda(), index.cuda()) == recvalidate.digest_cpu(data, index)


@pytest.mark.gpu
def test_gpu_digest_random_writer_records():
    rnd = random.Random(8)
    n = 5000
    keys = [rnd.randbytes(rnd.randint(10, 1000)) for _ in range(n)]
    vals = [rnd.randbytes(rnd.randint(0, 20000)) for _ in range(n)]
    data, index = _build(keys, vals)
    want = recvalidate.digest_cpu(data, index)
    assert want[0] == n and want[1] == int(index[1].sum()) - 8 * n
    got = recvalidate.digest(data.cuda(), index.cuda())
    assert got == want
    # a permutation of the index rows, on another stream: the same digest
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    st = torch.cuda.Stream()
    assert recvalidate.digest(data.cuda(), index[:, perm].contiguous().cuda(), stream=st) == want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_gpu_check_sorted_part_adversarial(n):
    keys = _adversarial_keys(n, 40 + n)
    for kind in ("bytes", "text"):
        data, index = _build(keys, [b"v"] * n, kind, junk_every=2)
        for nparts, part in ((3, 1), (1, 0), (3, None)):
            want = recvalidate.check_sorted_part_cpu(data, index, nparts, part)
            assert recvalidate.check_sorted_part(data.cuda(), index.cuda(), nparts, part) == want
    if n == 257:
        assert want[0] > 50


@pytest.mark.gpu
def test_gpu_check_sorted_part_planted():
    rnd = random.Random(10)
    nparts, part = 3, 1
    pool = [rnd.randbytes(rnd.randint(1, 60)) for _ in range(16000)]
    pool += [p + b"\0" for p in pool[:200]] + [p[:-1] for p in pool[200:400]]   # prefixes
    parts = recsort.partitions_cpu(pool, nparts)
    mine = sorted(k for k, p in zip(pool, parts) if p == part)[:5000]
    other = [k for k, p in zip(pool, parts) if p != part]
    assert len(mine) == 5000
    for i in range(20):                       # a record of another part, wherever it falls
        mine[100 + 233 * i] = other[i]
    for i in range(20):                       # descents: neighbours exchanged
        j = 50 + 241 * i
        mine[j], mine[j + 1] = mine[j + 1], mine[j]
    data, index = _build(mine, [b"v"] * 5000)
    want = recvalidate.check_sorted_part_cpu(data, index, nparts, part)
    assert want[1] == 20 and 20 <= want[0] <= 40
    d, ix = data.cuda(), index.cuda()
    assert recvalidate.check_sorted_part(d, ix, nparts, part) == want
    assert recvalidate.check_sorted_part(d, ix, nparts, None) == (want[0], 0)
    assert recvalidate.validate_records(d, ix, True, nparts, part) == \
        recvalidate.digest_cpu(data, index) + want


@pytest.mark.gpu
def test_gpu_validate_job_equals_classic(sorted_dirs, tmp_path):
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for case in ("sound", "swap", "value-byte"):
            (tmp_path / case).mkdir()
            inp, out = _copy(sorted_dirs, tmp_path / case)
            if case != "sound":
                _tamper(out, case)
            _check_case(_both(inp, out, cl), case)
        # the files of the last pair are resident: a second job loads none of them
        rj = cl.submit_job(validate_job.gpu_job(inp, out))
        assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
        cs = rj.getCounters()
        assert cs.get(JOB_GROUP, "GPU_MAP_TASKS") == 5
        assert cs.get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_HITS") == 5
        assert cs.get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_MISSES") == 0
        inp, out = _copy(sorted_dirs, tmp_path, "total")
        _tamper(out, "exchange-parts")
        _check_case(_both(inp, out, cl, total_order=True), "exchange-parts")
