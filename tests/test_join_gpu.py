"""GPU Join (map-only split-level job, native/kernels/recjoin.hip): the CPU twin
against the classic CompositeRecordReader job, ``join -gpu`` against the
classic job's parts, eligibility and its fallbacks, unsorted input, chunked
output, and on the GPU every kernel against the twin, bit for bit."""
import bisect
import logging
import os
import random
import struct

import numpy as np
import pytest
import torch

from hbmr.examples import join as join_example
from hbmr.io import sequencefile as seqf
from hbmr.io.writable import BytesWritable, IntWritable, Text
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.formats import TextOutputFormat
from hbmr.mapred.join import TupleWritable
from hbmr.models import join as join_job
from hbmr.ops import recjoin, recsort

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
TASK_GROUP = "org.apache.hadoop.mapred.Task$Counter"
OPS = ("inner", "outer", "override")

ADVERSARIAL = [b"", b"\0", b"\0\0", b"ab", b"ab\0", b"ab\0\0"] + \
    [bytes([97 + (i * 7 + n) % 26 for i in range(n)]) for n in (6, 7, 8, 13, 14, 15, 21)] + \
    [b"abcdef\0", b"abcdefg", b"abcdefg\0", b"abcdefgh", b"abcdefg\0\0\0\0\0\0\0",
     b"abcdefg\0\0\0\0\0\0\0\0", b"\x7f", b"\x80", b"\xff", b"\x7f\x80", b"\x80\x7f", b"\xff\0",
     b"ab\x7f", b"ab\x80", b"ab\xff", b"abcdefg\x80", b"abcdefg\x7f", b"abcdef\xff\xff",
     b"\xff" * 7, b"\xff" * 8, b"\xff" * 14, b"\xff" * 15, b"\0" * 7, b"\0" * 8, b"\0" * 21]


# ----------------------------------------------------------------------------- builders
def _build(records, kcls=BytesWritable, vcls=BytesWritable, pad=None):
    """(data uint8 tensor, index int64[4, n] tensor) of the (key, value) records
    as a SequenceFile holds their frames; ``pad(i)`` junk bytes stand before
    frame i (default: 20, a sync escape's place, before every 7th)."""
    parts, idx, off = [], [[], [], [], []], 0
    for i, (k, v) in enumerate(records):
        junk = pad(i) if pad else (20 if i % 7 == 6 else 0)
        parts.append(b"\xee" * junk)
        off += junk
        kb, vb = kcls(k).serialize(), vcls(v).serialize()
        fr = struct.pack(">ii", len(kb) + len(vb), len(kb)) + kb + vb
        idx[0].append(off)
        idx[1].append(len(fr))
        idx[2].append(off + 8 + len(kb) - len(k))
        idx[3].append(len(k))
        parts.append(fr)
        off += len(fr)
    raw = b"".join(parts)
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
        torch.empty(0, dtype=torch.uint8)
    return data, torch.tensor(idx, dtype=torch.int64).reshape(4, len(records))


def _val(rnd, tag, i, lo=0, hi=40):
    """An ASCII value (valid in Text and BytesWritable) that names its record."""
    tail = bytes(rnd.choice(b"abcdefghij") for _ in range(rnd.randint(lo, hi)))
    return f"{tag}:{i}:".encode() + tail


def _draw(pool, rnd, counts, share=0.7):
    """Per source ``counts[s]`` keys drawn (with repeats) from its own random
    ``share`` of the pool, sorted: partial overlap, duplicates."""
    out = []
    for n in counts:
        mine = rnd.sample(pool, max(1, int(len(pool) * share)))
        out.append(sorted(rnd.choice(mine) for _ in range(n)))
    return out


def _records(keysets, rnd, **kw):
    return [[(k, _val(rnd, s, i, **kw)) for i, k in enumerate(keys)]
            for s, keys in enumerate(keysets)]


def _write(path, records, kcls=BytesWritable, vcls=BytesWritable, **kw):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with seqf.Writer(str(path), kcls, vcls, **kw) as w:
        for k, v in records:
            w.append(kcls(k), vcls(v))
    return str(path)


def _parts(out):
    res = {}
    for fn in sorted(os.listdir(out)):
        if fn.startswith("part-"):
            recs = []
            with seqf.Reader(os.path.join(out, fn)) as r:
                while True:
                    raw = r.next_raw()
                    if raw is None:
                        break
                    recs.append(raw)
            res[fn] = recs
    return res


def _split_frames(frames):
    out = []
    for fr in frames:
        _, kl = struct.unpack(">ii", fr[:8])
        out.append((fr[8:8 + kl], fr[8 + kl:]))
    return out


def _local():
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    return conf


def _pool(rnd, text, n=300):
    if text:
        words = [f"word{i}" for i in range(30)]
        return sorted({" ".join(rnd.choice(words) for _ in range(rnd.randint(1, 12))).encode()
                       for _ in range(n)})
    return sorted({rnd.randbytes(rnd.randint(0, 120)) for _ in range(n)} | {b""})


def _inputs(tmp, text, nsrc, vclasses, nparts=2, seed=11, counts=(200, 150, 100)):
    """``nsrc`` source directories of ``nparts`` sorted part files each."""
    rnd = random.Random(seed + text)
    kcls = Text if text else BytesWritable
    pool = _pool(rnd, text)
    dirs = [str(tmp / f"src{s}") for s in range(nsrc)]
    for p in range(nparts):
        recs = _records(_draw(pool, rnd, counts[:nsrc]), rnd)
        for s in range(nsrc):
            _write(os.path.join(dirs[s], f"part-{p:05d}"), recs[s], kcls, vclasses[s])
    return dirs, kcls


def _file_sources(dirs, part):
    out, vcls = [], []
    for d in dirs:
        f = os.path.join(d, f"part-{part:05d}")
        data, index = recsort.index_records(f, 0, os.path.getsize(f))
        out.append((torch.from_numpy(data), torch.from_numpy(index)))
        with seqf.Reader(f) as r:
            vcls.append(r.value_class)
    return out, vcls


def _masks(records, nsrc):
    """The written masks of serialized TupleWritables (vint count, vlong mask)."""
    assert nsrc < 8
    return {v[1] for _, v in records}


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("op", OPS)
def test_join_records_cpu_equals_classic(tmp_path, op, nsrc, text):
    vclasses = [BytesWritable] * 3 if op == "override" else [BytesWritable, Text, BytesWritable]
    dirs, kcls = _inputs(tmp_path, text, nsrc, vclasses)
    out = str(tmp_path / "classic")
    job = join_example.make_job(dirs, out, op, 0, _local(), out_key=kcls,
                                out_value=BytesWritable if op == "override" else TupleWritable)
    assert JobClient.runJob(job).isSuccessful()
    want = _parts(out)
    assert list(want) == ["part-00000", "part-00001"]
    seen = set()
    for p, name in enumerate(want):
        sources, vcls = _file_sources(dirs, p)
        headers = None if op == "override" else recjoin.tuple_headers(vcls)
        got = _split_frames(recjoin.join_records_cpu(sources, op, headers))
        assert got == want[name], (name, len(got), len(want[name]))
        assert len(got) > 20
        seen |= _masks(got, nsrc)
    if op == "outer" and nsrc == 3:
        assert seen == set(range(1, 8))          # every combination of sources occurs


def _last_job(cl):
    return cl.jt.get_job(list(cl.jt.jobs)[-1])


@pytest.mark.parametrize("trackers", [1, 2])
def test_join_gpu_flag_equals_classic(tmp_path, trackers):
    """``join ... -gpu`` on CPU slots: the split job runs (no silent fallback)
    and its parts hold the classic job's records."""
    for text in (False, True):
        base = tmp_path / f"t{int(text)}"
        dirs, kcls = _inputs(base, text, 3, [BytesWritable] * 3, nparts=3)
        key_opt = ["-outKey", "hbmr.io.writable:" + ("Text" if text else "BytesWritable")]
        with LocalCluster(JobConf(), num_trackers=trackers, cpu_slots=2) as cl:
            for op in OPS:
                val_opt = []
                if op == "override":
                    val_opt = ["-outValue", "hbmr.io.writable:BytesWritable"]
                args = key_opt + val_opt + ["-joinOp", op] + dirs
                assert join_example.main(args + [str(base / f"c-{op}")], cluster=cl) == 0
                assert _last_job(cl).getJobName() == "join"
                assert join_example.main(["-gpu"] + args + [str(base / f"g-{op}")], cluster=cl) == 0
                rj = _last_job(cl)
                want, got = _parts(base / f"c-{op}"), _parts(base / f"g-{op}")
                assert list(want) == ["part-00000", "part-00001", "part-00002"]
                assert got == want
                n = sum(len(v) for v in want.values())
                assert n > 50
                assert rj.getJobName() == join_job.JOB_NAME
                cs = rj.getCounters()
                assert cs.get(TASK_GROUP, "MAP_OUTPUT_RECORDS") == n
                assert cs.get(TASK_GROUP, "MAP_INPUT_RECORDS") == 3 * 450
                assert cs.get(TASK_GROUP, "MAP_INPUT_BYTES") > 0
                assert os.path.exists(base / f"g-{op}" / "_SUCCESS")
                assert not os.path.exists(base / f"g-{op}" / "_temporary")


def _ineligible_cases(tmp):
    """(name, gpu_job arguments, reason pattern, the classic job can run it)"""
    rnd = random.Random(2)
    keys = sorted(rnd.randbytes(rnd.randint(1, 30)) for _ in range(40))
    recs = [(k, b"v%d" % i) for i, k in enumerate(keys)]
    a = [str(tmp / "a0"), str(tmp / "a1")]
    for d in a:
        _write(os.path.join(d, "part-00000"), recs)
    comp = str(tmp / "comp")
    _write(os.path.join(comp, "part-00000"), recs, compression="RECORD")
    txt = str(tmp / "txt")
    _write(os.path.join(txt, "part-00000"), [(k.hex().encode(), v) for k, v in recs], Text,
           BytesWritable)
    tval = str(tmp / "tval")
    _write(os.path.join(tval, "part-00000"), recs, BytesWritable, Text)
    ints = str(tmp / "ints")
    os.makedirs(ints)
    with seqf.Writer(os.path.join(ints, "part-00000"), IntWritable, BytesWritable) as w:
        for i in range(40):
            w.append(IntWritable(i - 20), BytesWritable(b"x"))
    cmp_conf, def_conf, zip_conf = JobConf(), JobConf(), JobConf()
    cmp_conf.set("mapred.join.keycomparator", "x:Y")
    def_conf.set("mapred.join.define.mine", "hbmr.mapred.join.readers:InnerJoinRecordReader")
    zip_conf.set_boolean("mapred.output.compress", True)
    sf = "hbmr.mapred.formats:SequenceFileInputFormat"
    t0, t1 = f'tbl({sf},"{a[0]}")', f'tbl({sf},"{a[1]}")'
    nested = f"inner(inner({t0},{t1}),{t0})"
    other_fmt = f'inner(tbl(hbmr.mapred.formats:KeyValueTextInputFormat,"{a[0]}"),{t1})'
    return [
        ("nested", dict(inputs=a, expr=nested), "nested join expression", False),
        ("format", dict(inputs=a, expr=other_fmt), "custom input format", False),
        ("operator", dict(inputs=a, join_type="mine"), "join operator 'mine'", False),
        ("one", dict(inputs=a[:1]), "1 join sources", False),
        ("nine", dict(inputs=[a[0]] * 9), "9 join sources", False),
        ("comparator", dict(inputs=a, base=cmp_conf), "custom key comparator x:Y", False),
        ("define", dict(inputs=a, base=def_conf), "custom join operator", False),
        ("reduces", dict(inputs=a, reduces=1), "1 reduces", True),
        ("outformat", dict(inputs=a, out_format=TextOutputFormat), "custom output format", True),
        ("zipped", dict(inputs=a, base=zip_conf), "compressed output", True),
        ("remote", dict(inputs=[a[0], "hdfs://nn:1/x"]), "not a local path", False),
        ("compressed", dict(inputs=[a[0], comp]), "RECORD-compressed input", True),
        ("intkeys", dict(inputs=[ints, ints]), "key class org.apache.hadoop.io.IntWritable", True),
        ("keyclasses", dict(inputs=[a[0], txt]), "different key classes", False),
        ("valueclasses", dict(inputs=[a[0], tval], join_type="override"),
         "different value classes", True),
    ]


def test_gpu_job_refuses_ineligible_and_join_falls_back(tmp_path, caplog):
    cases = _ineligible_cases(tmp_path)
    assert join_job.gpu_job(cases[0][1]["inputs"], str(tmp_path / "ok")).get_job_name() == \
        join_job.JOB_NAME
    for name, kw, why, runnable in cases:
        kw = dict(kw)
        inputs = kw.pop("inputs")
        with pytest.raises(ValueError, match=why):
            join_job.gpu_job(inputs, str(tmp_path / f"{name}-x"), **kw)
        if not runnable:
            continue
        base = kw.pop("base", None)
        conf = JobConf(base)
        conf.set("mapred.job.tracker", "local")
        if name == "intkeys":
            kw["out_key"] = IntWritable
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="hbmr.examples.join"):
            rj = join_example.run(inputs, str(tmp_path / f"{name}-g"), conf=conf, gpu=True, **kw)
        assert rj.isSuccessful() and rj.getJobName() == "join", name
        assert any(why in r.getMessage() and "classic join job" in r.getMessage()
                   for r in caplog.records), name
        rj = join_example.run(inputs, str(tmp_path / f"{name}-c"), conf=conf, **kw)
        assert rj.isSuccessful()
        if name not in ("outformat", "zipped"):
            got, want = _parts(tmp_path / f"{name}-g"), _parts(tmp_path / f"{name}-c")
            assert got == want and sum(len(v) for v in want.values()) >= 40, name


def test_unsorted_input_fails_the_job(tmp_path):
    rnd = random.Random(4)
    keys = sorted(rnd.randbytes(rnd.randint(1, 30)) for _ in range(300))
    bad = list(keys)
    bad[120], bad[121] = bad[121], bad[120]          # record 121 is below record 120
    bad[250], bad[251] = bad[251], bad[250]
    assert bad[121] < bad[120]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write(os.path.join(a, "part-00000"), [(k, b"v") for k in keys])
    _write(os.path.join(b, "part-00000"), [(k, b"w") for k in bad])
    sources, _ = _file_sources([a, b], 0)
    with pytest.raises(recjoin.UnsortedInput, match="source 1: the key of record 121 "):
        list(recjoin.join_records_cpu(sources, "override"))
    conf = JobConf()
    conf.set_int("mapred.map.max.attempts", 1)
    with LocalCluster(conf, num_trackers=1, cpu_slots=1) as cl:
        rj = cl.submit_job(join_job.gpu_job([a, b], str(tmp_path / "out"), "outer", base=conf))
        assert rj.waitForCompletion(60)
        assert not rj.isSuccessful()
        info = str(rj.getFailureInfo())
    assert os.path.join(b, "part-00000") in info and "record 121" in info, info
    assert not os.path.exists(tmp_path / "out" / "part-00000")


def _dup_sources(big=(40, 30), kcls=BytesWritable):
    """Two or three sources with one key that has 40 x 30 (x ...) records among
    other keys, some shared."""
    rnd = random.Random(8)
    keys = sorted({rnd.randbytes(rnd.randint(1, 20)) for _ in range(60)})
    hot = keys[31]
    sets = []
    for s, n in enumerate(big):
        mine = [k for i, k in enumerate(keys) if k != hot and (i + s) % 3]
        sets.append(sorted(mine + [hot] * n))
    recs = _records(sets, rnd)
    return [_build(r, kcls, BytesWritable) for r in recs], recs


@pytest.mark.parametrize("op", OPS)
def test_chunk_budget_cuts_inside_a_group(tmp_path, op):
    sources, _ = _dup_sources()
    headers = recjoin.tuple_headers([BytesWritable, BytesWritable])
    frames = list(recjoin.join_records_cpu(sources, op, headers))
    chunks = list(recjoin.join_chunks(sources, op, headers, chunk_bytes=3000))
    if op != "override":
        assert len(frames) > 1200 and len(chunks) > 20      # the 40 x 30 group spans chunks
    assert all(int(c.flen.sum()) <= 3000 for c in chunks)
    assert sum(int(c.flen.size) for c in chunks) == len(frames)
    vcls = BytesWritable if op == "override" else TupleWritable
    for name, budget in (("whole", 1 << 30), ("cut", 3000)):
        with seqf.Writer(str(tmp_path / name), BytesWritable, vcls) as w:
            assert recjoin.write_join(w, sources, op, headers, budget) == len(frames)
    whole, cut = _parts_of(tmp_path / "whole"), _parts_of(tmp_path / "cut")
    assert whole == cut == _split_frames(frames)


def _parts_of(path):
    recs = []
    with seqf.Reader(str(path)) as r:
        while True:
            raw = r.next_raw()
            if raw is None:
                return recs
            recs.append(raw)


def _overflow_sources():
    recs = [(b"k", b"")] * 300                       # 300^8 > 2^62
    return [_build(recs)] * 8


def test_product_overflow_raises():
    sources = _overflow_sources()
    headers = recjoin.tuple_headers([BytesWritable] * 8)
    with pytest.raises(OverflowError, match="2\\^62"):
        next(recjoin.join_records_cpu(sources, "outer", headers))
    assert len(list(recjoin.join_records_cpu(sources, "override"))) == 300


def test_tuple_headers_are_tuplewritables():
    hs = recjoin.tuple_headers([BytesWritable, Text, BytesWritable])
    assert len(hs) == 8
    v = [BytesWritable(b"abc"), None, BytesWritable(b"")]
    assert TupleWritable(v).serialize() == hs[5] + v[0].serialize() + v[2].serialize()
    assert hs[0] == TupleWritable([None] * 3).serialize()
    # an unwritten slot is named Text whatever its source holds, a written one by its class
    assert hs[1].count(b"org.apache.hadoop.io.Text") == 2
    assert hs[7].count(b"org.apache.hadoop.io.Text") == 1


# ----------------------------------------------------------------------------- GPU
def _families():
    rnd = random.Random(23)
    prefix = rnd.randbytes(40)
    base = rnd.randbytes(1000)
    long_pool = [base]
    for p in (15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 998, 999):
        for x in (0, 0x7f, 0x80, 0xff):
            long_pool.append(base[:p] + bytes([x]) + base[p + 1:])
    long_pool += [base[:n] for n in (15, 16, 17, 255, 256, 257, 999)]
    big = (2500, 2200, 2000)
    return {
        # few keys: few draws, or the cross products of the duplicates explode
        "adversarial": (BytesWritable, _draw(ADVERSARIAL, rnd, (150, 120, 100), 0.8)),
        "prefix40": (BytesWritable,
                     _draw([prefix + rnd.randbytes(rnd.randint(0, 20)) for _ in range(3000)], rnd,
                           big)),
        "random": (BytesWritable,
                   _draw([rnd.randbytes(rnd.randint(0, 300)) for _ in range(3000)], rnd, big)),
        "text": (Text, _draw(_pool(rnd, True, 3000), rnd, big)),
        "long1000": (BytesWritable, _draw(sorted(set(long_pool)), rnd, (200, 180, 160), 0.8)),
        "identical": (BytesWritable, [[b"\x81k" * 40] * 40, [b"\x81k" * 40] * 30,
                                      [b"\x81k" * 40] * 2]),
        "disjoint": (BytesWritable, [sorted(b"a" + rnd.randbytes(9) for _ in range(2100)),
                                     sorted(b"b" + rnd.randbytes(9) for _ in range(2300))]),
    }


_FAM = {}
VCLS = [BytesWritable, Text, BytesWritable]


def _family(name):
    """(sources, headers, {op: the twin's frames joined}) built once."""
    if not _FAM:
        rnd = random.Random(29)
        for nm, (kcls, keysets) in _families().items():
            recs = _records(keysets, rnd)
            sources = [_build(r, kcls, VCLS[s]) for s, r in enumerate(recs)]
            _FAM[nm] = {"sources": sources, "cpu": {},
                        "headers": recjoin.tuple_headers(VCLS[:len(sources)])}
    return _FAM[name]


def _twin(fam, op):
    if op not in fam["cpu"]:
        frames = list(recjoin.join_records_cpu(fam["sources"], op, fam["headers"]))
        fam["cpu"][op] = (np.array([len(f) for f in frames], dtype=np.int64), b"".join(frames))
    return fam["cpu"][op]


def _cuda(sources):
    return [(d.cuda(), i.cuda()) for d, i in sources]


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["adversarial", "prefix40", "random", "text", "long1000",
                                  "identical", "disjoint"])
def test_gpu_join_equals_twin(name, op):
    fam = _family(name)
    wlens, wblob = _twin(fam, op)
    if name == "identical" and op != "override":
        assert wlens.size == 40 * 30 * 2
    if name == "disjoint":
        assert wlens.size == (0 if op == "inner" else 4400)   # inner: a part with no records
    # the identical keys again under a budget that cuts inside their one group
    budgets = (1 << 30, 4096) if name in ("identical", "adversarial") else (1 << 30,)
    for budget in budgets:
        lens, blob = recjoin.join_blob(_cuda(fam["sources"]), op, fam["headers"], budget)
        assert np.array_equal(lens, wlens)
        assert blob == wblob


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_gpu_join_small(n, nsrc, op):
    rnd = random.Random(100 + n)
    pool = [rnd.randbytes(rnd.randint(0, 12)) for _ in range(max(2, n))]
    headers = recjoin.tuple_headers(VCLS[:nsrc])
    for empty in (None, 1):                          # all of n records; source 1 empty
        keysets = _draw(pool, rnd, [n] * nsrc, 0.8)
        if empty is not None:
            keysets[empty] = []
        sources = [_build(r, BytesWritable, VCLS[s])
                   for s, r in enumerate(_records(keysets, rnd))]
        frames = list(recjoin.join_records_cpu(sources, op, headers))
        lens, blob = recjoin.join_blob(_cuda(sources), op, headers)
        assert lens.tolist() == [len(f) for f in frames]
        assert blob == b"".join(frames)


def _heads_cpu(keys):
    head = [1 if i == 0 or keys[i - 1] < keys[i] else 0 for i in range(len(keys))]
    bad = [i for i in range(1, len(keys)) if keys[i] < keys[i - 1]]
    return head, (bad[0] if bad else None)


@pytest.mark.gpu
def test_gpu_heads_kernel():
    rnd = random.Random(31)
    base = rnd.randbytes(600)
    keys = []
    for n in range(34):                              # equal keys at every length 0..33
        keys += [base[:n], base[:n]]
    for n in (255, 256, 257, 511, 512, 513, 600):
        keys += [base[:n], base[:n]]
    for p in (0, 1, 15, 16, 17, 31, 32, 33, 254, 255, 256, 257, 598, 599):
        k = bytearray(base)
        k[p] ^= 0x80
        keys += [base, bytes(k), base[:p], base]     # above, below and a prefix at a piece edge
    keys += ADVERSARIAL
    keys = keys * 12                                 # several hundred workgroups of 16 pairs
    rnd.shuffle(keys)
    pads = [rnd.randrange(16) for _ in keys]
    data, index = _build([(k, b"v") for k in keys], pad=lambda i: pads[i])
    koffs = index[2].tolist()
    mis = {(a % 16, b % 16) for a, b in zip(koffs[:-1], koffs[1:])}
    assert {a for a, _ in mis} == set(range(16)) == {b for _, b in mis}
    whead, wbad = _heads_cpu(keys)
    assert wbad is not None and sum(1 for i in range(1, len(keys)) if keys[i] < keys[i - 1]) > 100
    head, bad = recjoin.group_heads(data.cuda(), index.cuda())
    assert head.tolist() == whead
    assert bad == wbad                               # the first of many offending records
    # sorted input: no offender, and the heads are the distinct keys
    skeys = sorted(keys)
    data, index = _build([(k, b"v") for k in skeys], pad=lambda i: pads[i])
    head, bad = recjoin.group_heads(data.cuda(), index.cuda())
    assert bad is None and head.tolist() == _heads_cpu(skeys)[0]
    assert int(head.sum()) == len(set(keys))
    # an index that points outside the data is refused before any launch
    broken = index.clone()
    broken[3, 5] = data.numel()
    with pytest.raises(ValueError, match="outside the data"):
        recjoin.group_heads(data.cuda(), broken.cuda())


@pytest.mark.gpu
def test_gpu_rank_kernel():
    rnd = random.Random(37)
    prefix = rnd.randbytes(40)
    tkeys = sorted(({prefix + rnd.randbytes(rnd.randint(0, 20)) for _ in range(1500)} |
                    {rnd.randbytes(rnd.randint(1, 30)) for _ in range(1500)} |
                    set(ADVERSARIAL)) - {b""})
    absent = [prefix + rnd.randbytes(rnd.randint(0, 20)) for _ in range(700)] + \
        [rnd.randbytes(rnd.randint(1, 30)) for _ in range(300)] + \
        [k + b"\0" for k in tkeys[::9]] + [k[:-1] for k in tkeys[::11]]
    probes = [b"", b"\xff" * 50, tkeys[0], tkeys[-1]] + rnd.sample(tkeys, 1200) + absent
    rnd.shuffle(probes)
    assert b"" in probes and b"" < tkeys[0] and b"\xff" * 50 > tkeys[-1]
    tdata, tindex = _build([(k, b"t") for k in tkeys])
    pdata, pindex = _build([(k, b"p") for k in probes])
    want_lb = [bisect.bisect_left(tkeys, k) for k in probes]
    want_eq = [int(i < len(tkeys) and tkeys[i] == k) for i, k in zip(want_lb, probes)]
    assert 1000 < sum(want_eq) < len(probes) - 500
    trec = torch.arange(len(tkeys), dtype=torch.int32).cuda()
    prec = torch.arange(len(probes), dtype=torch.int32).cuda()
    probe, target = (pdata.cuda(), pindex.cuda(), prec), (tdata.cuda(), tindex.cuda(), trec)
    try:
        for two_level in (True, False):
            recjoin.set_two_level(two_level)
            lb, eq = recjoin.rank_heads(probe, target)
            assert lb.tolist() == want_lb, two_level
            assert eq.tolist() == want_eq, two_level
    finally:
        recjoin.set_two_level(True)
    # a subset of the heads (every third record), and no heads at all
    sub = trec[::3].contiguous()
    lb, eq = recjoin.rank_heads(probe, (target[0], target[1], sub))
    skeys = tkeys[::3]
    assert lb.tolist() == [bisect.bisect_left(skeys, k) for k in probes]
    lb, eq = recjoin.rank_heads(probe, (target[0], target[1], sub[:0]))
    assert not lb.any() and not eq.any()
    with pytest.raises(ValueError, match="outside its index"):
        recjoin.rank_heads(probe, (target[0], target[1], trec + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["outer", "override"])
def test_gpu_output_frames_every_misalignment(op):
    rnd = random.Random(41)
    vlens = [0, 1, 15, 16, 17, 20_000]
    keys = sorted({rnd.randbytes(rnd.randint(0, 40)) for _ in range(36)})
    recs = []
    for s in range(2):
        mine = [k for i, k in enumerate(keys) if (i + s) % 4]
        mine = sorted(mine + mine[::5])              # some keys twice
        recs.append([(k, bytes(rnd.choice(b"xyz") for _ in range(vlens[(i + s) % 6])))
                     for i, k in enumerate(mine)])
    vcls = [Text, BytesWritable]                     # the slots' class names differ
    sources = [_build(r, BytesWritable, vcls[s]) for s, r in enumerate(recs)]
    headers = recjoin.tuple_headers(vcls)
    assert headers[1] != headers[2][:len(headers[1])]
    frames = list(recjoin.join_records_cpu(sources, op, headers))
    assert len(frames) > 40
    dev = _cuda(sources)
    for lead in range(16):
        lens, blob = recjoin.join_blob(dev, op, headers, lead=lead)
        assert lens.tolist() == [len(f) for f in frames], lead
        assert blob == b"".join(frames), lead


@pytest.mark.gpu
def test_gpu_product_overflow_raises():
    sources = _cuda(_overflow_sources())
    with pytest.raises(OverflowError, match="2\\^62"):
        recjoin.plan(sources, "outer")
    assert recjoin.plan(sources, "override").total == 300


@pytest.mark.gpu
def test_gpu_join_job_equals_classic(tmp_path):
    dirs, kcls = _inputs(tmp_path, False, 3, [BytesWritable] * 3, nparts=3, seed=19,
                         counts=(2500, 2200, 2000))
    for op in OPS:
        job = join_example.make_job(dirs, str(tmp_path / f"c-{op}"), op, 0, _local(),
                                    out_value=BytesWritable if op == "override" else TupleWritable)
        assert JobClient.runJob(job).isSuccessful()
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for i, op in enumerate(OPS):
            rj = cl.submit_job(join_job.gpu_job(dirs, str(tmp_path / f"g-{op}"), op))
            assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
            cs = rj.getCounters()
            assert cs.get(JOB_GROUP, "GPU_MAP_TASKS") == 3
            # the splits are the same files for every operator: loaded once
            assert cs.get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_HITS") == (3 if i else 0)
            want, got = _parts(tmp_path / f"c-{op}"), _parts(tmp_path / f"g-{op}")
            assert list(want) == ["part-00000", "part-00001", "part-00002"]
            assert got == want
            assert cs.get(TASK_GROUP, "MAP_OUTPUT_RECORDS") == sum(len(v) for v in want.values())
