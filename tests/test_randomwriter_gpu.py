"""GPU RandomWriter / RandomTextWriter (split-level job, native/kernels/recgen.hip):
the record definition written out again in plain Python, the twin against it,
the stop rule, the written file against ``Writer.append_raw``, the resident
split against the native indexer, the job on CPU slots, and the kernels and the
job on the GPU against the twin."""
import logging
import os
import struct

import numpy as np
import pytest
import torch

from hbmr.benchmarks import sortvalidator
from hbmr.examples import randomwriter
from hbmr.examples import sort as sort_example
from hbmr.gpu.split_cache import SplitCache
from hbmr.io import sequencefile as seqf
from hbmr.io.vint import encode_vint
from hbmr.io.writable import BytesWritable, Text
from hbmr.mapred import JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.task import TaskReporter
from hbmr.models import randomwrite as write_job
from hbmr.models import records
from hbmr.models import sort as sort_job
from hbmr.models import sortvalidate as validate_job
from hbmr.ops import recgen, recsort

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
GPU_GROUP = "hbmr.GpuCounters"
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
WORDS = [w.encode() for w in randomwriter._WORDS]
BYTES_DEFAULT = (10, 1000, 0, 20000)
TEXT_DEFAULT = (5, 10, 10, 100)


# ----------------------------------------------------------------------------- the definition
def _mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def _S(seed, m):
    return _mix((seed + (m + 1) * 0x9E3779B97F4A7C15) & M64)


def _R(seed, m, i):
    return _mix((_S(seed, m) + (i + 1) * 0xD6E8FEB86659FD93) & M64)


def _B(R, t):
    return _mix((R + (t + 1) * 0x94D049BB133111EB) & M64)


def _w32(B, j):
    a, b = B & M32, B >> 32
    x = (a + j) & M32
    x ^= x >> 16
    x = x * 0x21F0AAAD & M32
    x ^= b
    x ^= x >> 15
    x = x * 0x735A2D97 & M32
    return x ^ (x >> 15)


def _mulhi(x, r):
    return (x * r) >> 32


def _record(kind, seed, m, i, params, words=None):
    """(key payload, value payload, raw key, raw value) of record i of map m."""
    lo_k, hi_k, lo_v, hi_v = params
    R = _R(seed, m, i)
    nk = lo_k + _mulhi(R & M32, hi_k - lo_k + 1)
    nv = lo_v + _mulhi(R >> 32, hi_v - lo_v + 1)
    out = []
    for t, n in ((0, nk), (1, nv)):
        B = _B(R, t)
        if kind == "bytes":
            p = b"".join(_w32(B, j).to_bytes(4, "little") for j in range((n + 3) // 4))[:n]
            out.append((p, struct.pack(">i", n) + p))
        else:
            p = b" ".join(words[_mulhi(_w32(B, k), len(words))] for k in range(n))
            out.append((p, encode_vint(len(p)) + p))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _records(kind, seed, m, total, params, words=None):
    """The records of a map by the classic loop's stop rule."""
    recs, left = [], total
    while left > 0:
        r = _record(kind, seed, m, len(recs), params, words)
        recs.append(r)
        left -= len(r[0]) + len(r[1])
    return recs


def _frame(rec):
    return struct.pack(">ii", len(rec[2]) + len(rec[3]), len(rec[2])) + rec[2] + rec[3]


def _check_against_definition(data, index, recs, pos=0):
    fr = [_frame(r) for r in recs]
    assert index.shape == (4, len(recs))
    assert recsort.frames(data, index) == fr
    assert recsort.payloads(data, index) == [r[0] for r in recs]
    dst, gaps, total = recsort.layout(np.array([len(f) for f in fr], dtype=np.int64), pos, 0)
    assert index[recsort.FOFF].tolist() == dst.tolist() and data.numel() == total
    assert index[recsort.FLEN].tolist() == [len(f) for f in fr]
    prefix = [len(r[2]) - len(r[0]) for r in recs]
    assert (index[recsort.KOFF] - index[recsort.FOFF]).tolist() == [8 + p for p in prefix]
    assert index[recsort.KLEN].tolist() == [len(r[0]) for r in recs]
    return gaps


# ----------------------------------------------------------------------------- CPU: the twin
BYTES_CASES = {"default": (BYTES_DEFAULT, 60_000), "min==max": ((7, 7, 33, 33), 3_000),
               "min_key=0": ((0, 5, 0, 9), 700), "max_value=0": ((1, 40, 0, 0), 2_500)}
TEXT_CASES = {"default": (TEXT_DEFAULT, WORDS, 20_000), "min==max": ((3, 3, 4, 4), WORDS, 3_000),
              "min_key=0": ((0, 2, 0, 3), WORDS, 1_500),
              "max_value=0": ((1, 4, 0, 0), WORDS, 1_500),
              "one word": (TEXT_DEFAULT, [b"x"], 5_000)}


@pytest.mark.parametrize("m", [0, 7])
@pytest.mark.parametrize("seed", [0, 1, (1 << 63) + 5])
def test_twin_equals_definition_bytes(seed, m):
    for params, total in BYTES_CASES.values():
        recs = _records("bytes", seed, m, total, params)
        data, index = recgen.generate_cpu("bytes", seed, m, total, params)
        gaps = _check_against_definition(data, index, recs)
        assert (len(gaps) > 0) == (data.numel() > 2100)
        L = recgen.lengths("bytes", seed, m, 0, len(recs), params)
        assert L[recgen.KL].tolist() == [len(r[0]) for r in recs]
        assert L[recgen.VL].tolist() == [len(r[1]) for r in recs]
    assert {len(r[0]) for r in _records("bytes", seed, m, 700, (0, 5, 0, 9))} >= {0, 5}


@pytest.mark.parametrize("m", [0, 7])
@pytest.mark.parametrize("seed", [0, 1, (1 << 63) + 5])
def test_twin_equals_definition_text(seed, m):
    for params, words, total in TEXT_CASES.values():
        recs = _records("text", seed, m, total, params, words)
        data, index = recgen.generate_cpu("text", seed, m, total, params, words)
        _check_against_definition(data, index, recs)
        L = recgen.lengths("text", seed, m, 0, len(recs), params, vocabulary=words)
        assert L[recgen.KL].tolist() == [len(r[0]) for r in recs]
        assert L[recgen.VL].tolist() == [len(r[1]) for r in recs]
        assert all(params[0] <= k <= params[1] for k in L[recgen.NK].tolist())
        assert all(params[2] <= v <= params[3] for v in L[recgen.NV].tolist())


def test_twin_works_in_batches(monkeypatch):
    want_b = recgen.generate_cpu("bytes", 3, 1, 40_000, (10, 100, 0, 300))
    want_t = recgen.generate_cpu("text", 3, 1, 40_000, TEXT_DEFAULT, WORDS)
    monkeypatch.setattr(recgen, "_BATCH_RECORDS", 7)
    for want, got in ((want_b, recgen.generate_cpu("bytes", 3, 1, 40_000, (10, 100, 0, 300))),
                      (want_t, recgen.generate_cpu("text", 3, 1, 40_000, TEXT_DEFAULT, WORDS))):
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


def test_stop_rule():
    for kind, params, words in (("bytes", BYTES_DEFAULT, None), ("text", TEXT_DEFAULT, WORDS)):
        r0 = _record(kind, 0, 0, 0, params, words)
        one = len(r0[0]) + len(r0[1])
        for total, want_n in ((1, 1), (one, 1), (one + 1, 2), (200_000, None)):
            p = recgen.plan(kind, 0, 0, 0, total, params, vocabulary=words)
            n = int(p.index.shape[1])
            pay = [len(r[0]) + len(r[1]) for r in (_record(kind, 0, 0, i, params, words)
                                                  for i in range(n))]
            assert sum(pay) >= total > sum(pay[:-1])
            assert p.payload == sum(pay) and (want_n is None or n == want_n)
        assert recgen.plan(kind, 0, 0, 0, 0, params, vocabulary=words).index.shape == (4, 0)


def test_plan_in_growing_batches_and_record_ranges(monkeypatch):
    """The cut is the same however the lengths arrive, and a plan bounded by
    ``max_bytes`` continues where the one before it ended."""
    whole = recgen.plan("bytes", 5, 2, 0, 300_000, (10, 100, 0, 300))
    monkeypatch.setattr(recgen, "_mean_payload", lambda *a: 1e9)      # batches of 64, 128, ...
    again = recgen.plan("bytes", 5, 2, 0, 300_000, (10, 100, 0, 300))
    assert torch.equal(whole.index, again.index) and whole.payload == again.payload
    first, left, flens, pos = 0, 300_000, [], 0
    while left > 0:
        p = recgen.plan("bytes", 5, 2, first, left, (10, 100, 0, 300), max_bytes=5_000, pos=pos)
        assert 0 < p.total <= 5_000 and p.first == first
        flens += p.index[recsort.FLEN].tolist()
        first += p.index.shape[1]
        left -= p.payload
        pos += p.total
    assert flens == whole.index[recsort.FLEN].tolist()
    huge = recgen.plan("bytes", 5, 2, 0, 10_000, (4000, 4000, 4000, 4000), max_bytes=100)
    assert huge.index.shape[1] == 1                                   # at least one record


def test_parameters_that_never_end_are_refused(tmp_path):
    for kind in ("bytes", "text"):
        with pytest.raises(ValueError, match="no record ever adds a byte"):
            recgen.plan(kind, 0, 0, 0, 100, (0, 0, 0, 0), vocabulary=WORDS)
    with pytest.raises(ValueError, match="range"):
        recgen.lengths("bytes", 0, 0, 0, 4, (5, 4, 0, 9))
    conf = JobConf()
    conf.set_int("test.randomwrite.max_key", 0)
    conf.set_int("test.randomwrite.min_key", 0)
    conf.set_int("test.randomwrite.max_value", 0)
    with pytest.raises(ValueError, match="no record ever adds a byte"):
        write_job.gpu_job(str(tmp_path / "o"), base=conf)
    with pytest.raises(ValueError, match="no record ever adds a byte"):
        randomwriter.run(str(tmp_path / "o"), conf=conf, gpu=True)
    assert not (tmp_path / "o").exists()


def test_determinism_and_separation():
    def gen(seed, m):
        return recgen.generate_cpu("bytes", seed, m, 100_000, BYTES_DEFAULT)

    a, b = gen(0, 0), gen(0, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert recsort.frames(*gen(0, 0))[0] != recsort.frames(*gen(1, 0))[0]
    assert recsort.frames(*gen(0, 0))[0] != recsort.frames(*gen(0, 1))[0]
    data, index = recgen.generate_cpu("bytes", 0, 0, 400_000, (10, 40, 0, 0))
    keys = recsort.payloads(data, index)
    assert len(keys) >= 10_000 and min(len(k) for k in keys) >= 10
    assert len(set(keys[:10_000])) == 10_000
    data, index = recgen.generate_cpu("bytes", 0, 0, 1 << 20, (0, 0, 1000, 20000))
    values = np.concatenate([data.numpy()[o + 16:o + n] for o, n in
                             zip(index[0].tolist(), index[1].tolist())])
    assert values.size >= 1 << 20
    assert np.bincount(values[:1 << 20], minlength=256).min() > 0


@pytest.mark.parametrize("word,count,payload,prefix", [
    (127, 1, 127, 1), (63, 2, 127, 1), (128, 1, 128, 2), (255, 1, 255, 2), (127, 2, 255, 2),
    (256, 1, 256, 3), (1, 50, 99, 1), (2, 43, 128, 2)])
def test_text_lengths_at_the_vint_boundaries(word, count, payload, prefix):
    words = [b"w" * word]
    params = (count, count, count, count)
    recs = _records("text", 0, 0, 3 * 2 * payload, params, words)
    assert len(recs) == 3 and all(len(r[0]) == len(r[1]) == payload for r in recs)
    assert all(len(r[2]) - payload == prefix == len(encode_vint(payload)) for r in recs)
    data, index = recgen.generate_cpu("text", 0, 0, 3 * 2 * payload, params, words)
    _check_against_definition(data, index, recs)
    assert (index[recsort.KOFF] - index[recsort.FOFF]).tolist() == [8 + prefix] * 3
    assert index[recsort.FLEN].tolist() == [8 + 2 * (prefix + payload)] * 3


def test_vocabulary_limits():
    assert recgen.vocabulary_reason(WORDS) is None
    assert recgen.vocabulary_reason([b"ab"] * 1024) is None
    assert recgen.vocabulary_reason([b"a" * 16] * 1024) is None
    assert "1025 words" in recgen.vocabulary_reason([b"ab"] * 1025)
    assert "16385 bytes" in recgen.vocabulary_reason([b"a" * 16384, b"b"])
    assert "empty" in recgen.vocabulary_reason([]) and "empty" in recgen.vocabulary_reason([b""])
    with pytest.raises(ValueError, match="1025 words"):
        recgen.lengths("text", 0, 0, 0, 4, TEXT_DEFAULT, vocabulary=[b"ab"] * 1025)
    with pytest.raises(ValueError, match="need a vocabulary"):
        recgen.lengths("text", 0, 0, 0, 4, TEXT_DEFAULT)


def test_fill_leaves_other_bytes_and_rejects_frames_outside():
    p = recgen.plan("bytes", 0, 0, 0, 9_000, (10, 100, 0, 300), pos=90)
    assert len(p.gaps) >= 2
    out = torch.full((p.total + 7,), 0xA5, dtype=torch.uint8)
    recgen.fill("bytes", 0, 0, 0, p.index, out)
    covered = np.zeros(p.total + 7, dtype=bool)
    for o, n in zip(p.index[0].tolist(), p.index[1].tolist()):
        covered[o:o + n] = True
    assert (out.numpy()[~covered] == 0xA5).all() and (~covered).sum() == 20 * len(p.gaps) + 7
    esc = bytes(range(1, 21))
    recgen.fill_syncs(out, p.gaps, esc)
    assert all(bytes(out[g:g + 20].numpy()) == esc for g in p.gaps.tolist())
    with pytest.raises(ValueError, match="outside the buffer"):
        recgen.fill("bytes", 0, 0, 0, p.index, out[:p.total - 1])
    bad = p.index.clone()
    bad[recsort.KLEN, 0] = bad[recsort.FLEN, 0]
    with pytest.raises(ValueError, match="outside the buffer"):
        recgen.fill("bytes", 0, 0, 0, bad, out)
    with pytest.raises(ValueError, match="outside the buffer"):
        recgen.fill_syncs(out, [out.numel() - 19], esc)


# ----------------------------------------------------------------------------- CPU: a map
class _Ctx:
    """What a map of the split job asks of its task context."""

    def __init__(self, device="cpu", stream=None):
        self.device = device
        self.stream = stream
        self.reporter = TaskReporter()
        self.split_cache = SplitCache()


def _run_map(out, text, seed, m, total, device="cpu", keys=None):
    conf = JobConf()
    for k, v in (keys or {}).items():
        conf.set(k, v)
    job = write_job.gpu_job(str(out), 8, total, text, seed, base=conf)
    sj = write_job.RandomWriteSplitJob()
    sj.configure(job)
    spec = sj.get_splits(job, [])[m]
    assert sj.load_split(spec, device) is spec and sj.cache_inputs is False
    ctx = _Ctx(device)
    res = sj.map_cpu(ctx, spec) if device == "cpu" else sj.map_gpu(ctx, spec)
    return sj, ctx, res


def _read_raw(path):
    with seqf.Reader(path) as r:
        return r.key_class, r.value_class, r.sync, list(iter(r.next_raw, None))


@pytest.mark.parametrize("text", [False, True], ids=["bytes", "text"])
def test_file_equals_writer(tmp_path, text):
    """The part of a map — several chunks, several sync intervals — read back
    record by record and compared byte for byte with what Writer.append_raw
    writes for the definition's records."""
    kind, words = ("text", WORDS) if text else ("bytes", None)
    prefix = "test.randomtextwrite." if text else "test.randomwrite."
    keys = {} if text else {prefix + "max_key": 100, prefix + "max_value": 500}
    keys[write_job.CHUNK_KEY] = 5000
    params = TEXT_DEFAULT if text else (10, 100, 0, 500)
    sj, ctx, res = _run_map(tmp_path / "o", text, 9, 3, 30_000, keys=keys)
    part = str(tmp_path / "o" / "part-00003")
    recs = _records(kind, 9, 3, 30_000, params, words)
    kc, vc, sync, raw = _read_raw(part)
    assert (kc, vc) == ((Text, Text) if text else (BytesWritable, BytesWritable))
    assert raw == [(r[2], r[3]) for r in recs]
    assert res == {"records": len(recs), "bytes": os.path.getsize(part)}
    assert not os.listdir(tmp_path / "o" / "_temporary")
    with seqf.Writer(str(tmp_path / "twin"), kc, vc) as w:
        other = w.sync
        for r in recs:
            w.append_raw(r[2], r[3])
    got = open(part, "rb").read()
    want = open(tmp_path / "twin", "rb").read().replace(other, sync)
    assert got == want and got.count(sync) >= 1 + len(got) // 4000
    cs = ctx.reporter.counters
    group = "RandomTextWriter" if text else "RandomWriter"
    assert cs.get(group, "BYTES_WRITTEN") == sum(len(r[0]) + len(r[1]) for r in recs)
    if not text:
        assert cs.get(group, "RECORDS_WRITTEN") == len(recs)
    assert ctx.split_cache.resident() == []            # several chunks: nothing resident


@pytest.mark.parametrize("text", [False, True], ids=["bytes", "text"])
def test_resident_split_equals_indexer(tmp_path, text):
    sj, ctx, res = _run_map(tmp_path / "o", text, 4, 1, 50_000)
    part = str(tmp_path / "o" / "part-00001")
    size = os.path.getsize(part)
    assert ctx.split_cache.resident() == [[f"sort:{part}:0:{size}", "cpu"]]
    split = ctx.split_cache.get(f"sort:{part}:0:{size}", "cpu")
    data, index = recsort.index_records(part, 0, size)
    assert sorted(split) == ["data", "index"] and index.shape[1] == res["records"] > 3
    assert np.array_equal(split["data"].numpy(), data)
    assert np.array_equal(split["index"].numpy(), index)
    # the key is GPU Sort's and GPU SortValidator's for the file
    conf = sort_example.make_job(str(tmp_path / "o"), str(tmp_path / "sorted"))
    conf.set_num_map_tasks(1)
    assert [s.key for s in sort_job.SortSplitJob().get_splits(conf, [])] == \
        [f"sort:{part}:0:{size}"]
    _, ctx, _ = _run_map(tmp_path / "p", text, 4, 1, 50_000,
                        keys={write_job.RESIDENT_KEY: "false"})
    assert ctx.split_cache.resident() == []


# ----------------------------------------------------------------------------- CPU: the job
@pytest.fixture(scope="module")
def cpu_cluster():
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        yield cl


def _parts(d):
    return sorted(f for f in os.listdir(d) if not f.startswith("."))


@pytest.mark.parametrize("text", [False, True], ids=["bytes", "text"])
def test_job_on_cpu_slots(cpu_cluster, tmp_path, text):
    out = str(tmp_path / "gen")
    main = randomwriter.main_text if text else randomwriter.main
    assert main([out, "-m", "3", "-b", "60000", "-seed", "6", "-gpu"], cluster=cpu_cluster) == 0
    assert _parts(out) == ["_SUCCESS", "part-00000", "part-00001", "part-00002"]
    kind, params, words = ("text", TEXT_DEFAULT, WORDS) if text else ("bytes", BYTES_DEFAULT, None)
    for m in range(3):
        raw = _read_raw(os.path.join(out, f"part-{m:05d}"))[3]
        assert raw == [(r[2], r[3]) for r in _records(kind, 6, m, 60_000, params, words)]
    rj = randomwriter.run(str(tmp_path / "again"), 3, 60_000, text, 6, cluster=cpu_cluster,
                          gpu=True)
    want = [_records(kind, 6, m, 60_000, params, words) for m in range(3)]
    cs = rj.getCounters()
    group = "RandomTextWriter" if text else "RandomWriter"
    assert cs.get(group, "BYTES_WRITTEN") == sum(len(r[0]) + len(r[1]) for rs in want for r in rs)
    if not text:
        assert cs.get(group, "RECORDS_WRITTEN") == sum(len(rs) for rs in want)
    # the classic sort and SortValidator take the output
    rj = sort_example.run(out, str(tmp_path / "sorted"), 2, cluster=cpu_cluster)
    assert rj.isSuccessful()
    res = sortvalidator.validate(out, str(tmp_path / "sorted"), cluster=cpu_cluster)
    assert res["ok"] and res["IN_RECORDS"] == sum(len(rs) for rs in want)


def test_ineligible_jobs_run_the_classic_job(tmp_path, caplog, monkeypatch):
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    local.set_boolean("mapred.output.compress", True)
    with pytest.raises(ValueError, match="compressed output"):
        write_job.gpu_job(str(tmp_path / "x"), base=local)
    with pytest.raises(ValueError, match="not a local one"):
        write_job.gpu_job("hdfs://nn:1/x")
    with caplog.at_level(logging.WARNING, logger="hbmr.examples.randomwriter"):
        assert randomwriter.main([str(tmp_path / "comp"), "-m", "1", "-b", "5000", "-gpu"],
                                 conf=local) == 0
    assert "not eligible for the GPU: compressed output" in caplog.text
    assert "classic randomwriter" in caplog.text
    with seqf.Reader(str(tmp_path / "comp" / "part-00000")) as r:
        assert r.compression != seqf.NONE
    local.set_boolean("mapred.output.compress", False)
    monkeypatch.setattr(randomwriter, "_WORDS", ["ab%d" % i for i in range(1025)])
    with pytest.raises(ValueError, match="1025 words"):
        write_job.gpu_job(str(tmp_path / "x"), text=True)
    assert write_job.gpu_job(str(tmp_path / "x")).get_num_reduce_tasks() == 0    # bytes: no words
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="hbmr.examples.randomwriter"):
        assert randomwriter.main_text([str(tmp_path / "big"), "-m", "1", "-b", "5000", "-gpu"],
                                      conf=local) == 0
    assert "1025 words" in caplog.text and "classic randomtextwriter" in caplog.text
    assert _read_raw(str(tmp_path / "big" / "part-00000"))[3]


def test_without_gpu_the_classic_job_is_unchanged(tmp_path):
    for text, mapper in ((False, randomwriter.RandomMapper), (True, randomwriter.RandomTextMapper)):
        job = randomwriter.make_job(str(tmp_path / "o"), 2, 1000, text)
        assert job.get_mapper_class() is mapper and job.get("hbmr.splitjob.class") is None
    job = write_job.gpu_job(str(tmp_path / "o"), 3, 1000, True, 11)
    assert job.get("hbmr.splitjob.class") == "hbmr.models.randomwrite:RandomWriteSplitJob"
    assert job.get_long(write_job.SEED_KEY, 0) == 11 and job.get_num_map_tasks() == 3


# ----------------------------------------------------------------------------- GPU
def _dev():
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bytes", "text"])
def test_gpu_lengths_equal_twin(kind):
    words = WORDS if kind == "text" else None
    cases = [BYTES_DEFAULT, (7, 7, 33, 33), (10, 10, 0, 1), (4, 5, 8, 9)] if kind == "bytes" else \
        [TEXT_DEFAULT, (3, 3, 4, 4), (5, 5, 0, 1), (4, 5, 8, 9)]
    for params in cases:
        for first in (0, 12345):
            for count in (0, 1, 63, 64, 65, 257, 100_000):
                if count == 100_000 and params is not cases[0]:
                    continue
                want = recgen.lengths(kind, 2, 5, first, count, params, vocabulary=words)
                got = recgen.lengths(kind, 2, 5, first, count, params, _dev(), words)
                assert got.device.type == "cuda" and got.shape == (4, count)
                assert torch.equal(got.cpu(), want), (params, first, count)


def _hand_plan(kind, lens, sync_every=5):
    """Frames of the given payload lengths at every destination misalignment
    0-15, 0xA5 in front and in between (20-byte holes after some frames, short
    pads after the others), the last frame ending on the buffer's last byte."""
    foff, flen, koff, klen, off = [], [], [], [], 0
    i = 0
    for mis in range(16):
        for kl, vl in lens:
            pad = (mis - off) % 16 or 16
            if i % sync_every == 0:
                pad += 32                                 # a sync hole and more
            off += pad
            fl, kpre = recgen.frame_lengths(kind, np.int64(kl), np.int64(vl))
            foff.append(off)
            flen.append(int(fl))
            koff.append(off + int(kpre))
            klen.append(kl)
            off += int(fl)
            i += 1
    return torch.tensor([foff, flen, koff, klen], dtype=torch.int64), off


def _check_fill(kind, seed, m, first, index, total, params=None, words=None):
    want = torch.full((total,), 0xA5, dtype=torch.uint8)
    recgen.fill(kind, seed, m, first, index, want, params, words)
    for shift in (0, 5):                  # the buffer itself at two alignments in memory
        raw = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device=_dev())
        out = raw[shift:shift + total]
        recgen.fill(kind, seed, m, first, index.to(_dev()), out, params, words)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), (kind, shift)
        assert (raw[:shift].cpu() == 0xA5).all() and (raw[shift + total:].cpu() == 0xA5).all()
    return want


@pytest.mark.gpu
def test_gpu_fill_bytes_every_alignment():
    klens = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33]
    vlens = [0, 1, 2, 3, 4, 5, 12, 13, 255, 256, 257, 4095, 4096, 4097, 20000]
    lens = [(klens[i % len(klens)], v) for i, v in enumerate(vlens)] + \
        [(k, vlens[(3 * i) % 9]) for i, k in enumerate(klens)] + [(1000, 0), (0, 0)]
    index, total = _hand_plan("bytes", lens)
    assert {int(o) % 16 for o in index[0]} == set(range(16)) and index.shape[1] == 16 * len(lens)
    want = _check_fill("bytes", 3, 2, 77, index, total)
    # the twin's frames are the definition's, holes and the bytes in front are untouched
    covered = np.zeros(total, dtype=bool)
    for i, (o, n, kl) in enumerate(zip(index[0].tolist(), index[1].tolist(), index[3].tolist())):
        covered[o:o + n] = True
        if i % 37 == 0:
            kp, vp, kb, vb = _record("bytes", 3, 2, 77 + i, (kl, kl, n - 16 - kl, n - 16 - kl))
            assert bytes(want[o:o + n].numpy()) == _frame((kp, vp, kb, vb))
    assert (want.numpy()[~covered] == 0xA5).all() and not covered[:16].any() and covered[-1]


def _fill_small(kind):
    """0-65 records through plan + fill, equal to generate_cpu."""
    params, words = ((1, 40, 0, 70), None) if kind == "bytes" else ((1, 3, 0, 6), WORDS)
    for n in (0, 1, 2, 3, 15, 16, 17, 64, 65):
        L = recgen.lengths(kind, 1, 0, 0, max(n, 1), params, vocabulary=words)
        target = int((L[0] + L[1])[:n].sum()) if n else 0
        want, index = recgen.generate_cpu(kind, 1, 0, target, params, words)
        assert index.shape[1] == n
        got, p = recgen.generate(kind, 1, 0, 0, target, params, _dev(), vocabulary=words,
                                 escape=b"\0" * 20)
        assert torch.equal(p.index.cpu(), index) and torch.equal(got.cpu(), want)


@pytest.mark.gpu
def test_gpu_fill_bytes_small():
    _fill_small("bytes")


@pytest.mark.gpu
def test_gpu_fill_text_small():
    _fill_small("text")


TEXT_GPU_CASES = {
    "one 1-byte word": ([b"x"], [(1, 1, 1, 1), (5, 10, 10, 100), (100, 100, 100, 100)]),
    "standard": (WORDS, [(1, 1, 1, 1), (5, 10, 10, 100), (100, 100, 100, 100), (0, 1, 0, 2)]),
    "1024 words in 16 KiB": ([bytes([65 + i % 26]) * 16 for i in range(1024)],
                             [(1, 1, 1, 1), (5, 10, 10, 100), (100, 100, 100, 100)]),
    "vint 127": ([b"w" * 127], [(1, 1, 1, 1)]), "vint 128": ([b"w" * 128], [(1, 1, 1, 1)]),
    "vint 255": ([b"w" * 127], [(2, 2, 2, 2)]), "vint 256": ([b"w" * 256], [(1, 1, 1, 1)]),
    "vint 65536": ([b"w" * 8000, b"v" * 8191], [(9, 9, 1, 1)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TEXT_GPU_CASES))
def test_gpu_fill_text_every_alignment(case):
    words, all_params = TEXT_GPU_CASES[case]
    for params in all_params:
        per = 3 if params[3] >= 100 else 6
        L = recgen.lengths("text", 8, 1, 40, 16 * per, params, vocabulary=words)
        lens = list(zip(L[0].tolist(), L[1].tolist()))
        off, rows = 0, []                   # `per` records at each misalignment 0-15
        for i, (kl, vl) in enumerate(lens):
            pad = (i // per - off) % 16 or 16
            pad += 32 if i % 5 == 0 else 0
            off += pad
            fl, kpre = recgen.frame_lengths("text", np.int64(kl), np.int64(vl))
            rows.append((off, int(fl), off + int(kpre), kl))
            off += int(fl)
        index = torch.tensor(rows, dtype=torch.int64).t().contiguous()
        assert {int(o) % 16 for o in index[0]} == set(range(16))
        want = _check_fill("text", 8, 1, 40, index, off, params, words)
        covered = np.zeros(off, dtype=bool)
        for o, n in zip(index[0].tolist(), index[1].tolist()):
            covered[o:o + n] = True
        assert (want.numpy()[~covered] == 0xA5).all() and covered[-1]
        o, n = index[0, 7].item(), index[1, 7].item()
        assert bytes(want[o:o + n].numpy()) == _frame(_record("text", 8, 1, 47, params, words))


@pytest.mark.gpu
@pytest.mark.parametrize("text", [False, True], ids=["bytes", "text"])
def test_gpu_generated_split_equals_indexer(tmp_path, text):
    sj, ctx, res = _run_map(tmp_path / "o", text, 4, 1, 300_000, device=_dev())
    part = str(tmp_path / "o" / "part-00001")
    size = os.path.getsize(part)
    assert ctx.split_cache.resident() == [[f"sort:{part}:0:{size}", 0]]
    split = ctx.split_cache.get(f"sort:{part}:0:{size}", 0)
    data, index = records.load_record_split(part, 0, size, _dev())
    assert split["data"].device == data.device and split["index"].device == index.device
    assert torch.equal(split["data"], data) and torch.equal(split["index"], index)
    assert index.shape[1] == res["records"] > 3
    twin = _run_map(tmp_path / "c", text, 4, 1, 300_000)[1].split_cache.get(
        f"sort:{tmp_path / 'c' / 'part-00001'}:0:{size}", "cpu")
    assert torch.equal(twin["index"], index.cpu())
    assert _read_raw(part)[3] == _read_raw(str(tmp_path / "c" / "part-00001"))[3]


@pytest.mark.gpu
@pytest.mark.parametrize("text", [False, True], ids=["bytes", "text"])
def test_gpu_job_equals_cpu_slots(tmp_path, text):
    main = randomwriter.main_text if text else randomwriter.main
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        assert main([str(tmp_path / "cpu"), "-m", "3", "-b", "300000", "-seed", "5", "-gpu"],
                    cluster=cl) == 0
    for resident in (True, False):
        conf = JobConf()
        conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
        conf.set_boolean(write_job.RESIDENT_KEY, resident)
        gen = str(tmp_path / f"gen-{resident}")
        out = str(tmp_path / f"out-{resident}")
        with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
            rj = randomwriter.run(gen, 3, 300_000, text, 5, conf=conf, cluster=cl, gpu=True)
            assert rj.isSuccessful() and rj.getCounters().get(JOB_GROUP, "GPU_MAP_TASKS") == 3
            assert _parts(gen) == ["_SUCCESS", "part-00000", "part-00001", "part-00002"]
            for p in _parts(gen)[1:]:
                assert _read_raw(os.path.join(gen, p))[3] == \
                    _read_raw(str(tmp_path / "cpu" / p))[3]
            hit, miss = ("GPU_SPLIT_CACHE_HITS", "GPU_SPLIT_CACHE_MISSES") if resident else \
                ("GPU_SPLIT_CACHE_MISSES", "GPU_SPLIT_CACHE_HITS")
            sort_conf = JobConf(conf)
            sort_conf.set_num_map_tasks(1)             # whole-file splits
            rj = sort_example.run(gen, out, 2, conf=sort_conf, cluster=cl, gpu=True)
            assert rj.isSuccessful()
            cs = rj.getCounters()
            assert cs.get(GPU_GROUP, hit) == 3 and cs.get(GPU_GROUP, miss) == 0
            rj = cl.submit_job(validate_job.gpu_job(gen, out))
            assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
            cs = rj.getCounters()
            # the three inputs are resident either way by now (the sort loaded them);
            # the two sorted parts are not
            assert cs.get(GPU_GROUP, "GPU_SPLIT_CACHE_HITS") == 3
            assert cs.get(GPU_GROUP, "GPU_SPLIT_CACHE_MISSES") == 2
            res = sortvalidator.validate(gen, out, cluster=cl, gpu=True)
            assert res["ok"] and res["IN_RECORDS"] == res["OUT_RECORDS"] > 30
