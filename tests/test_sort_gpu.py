"""GPU Sort (split-level job, native/kernels/recsort.hip): the round keys against
``bytes`` comparison, the record sort and its partitioners against Python's
``sorted`` / HashPartitioner / TotalOrderPartitioner, the native indexer
against the SequenceFile record reader, the layout path against
``sequencefile.Writer``, and the job's parts against the classic sort's."""
import collections
import os
import random
import struct

import numpy as np
import pytest
import torch

from hbmr.examples import randomwriter
from hbmr.examples import sort as sort_example
from hbmr.io import sequencefile as seqf
from hbmr.io.writable import BytesWritable, IntWritable, Text, hash_bytes
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.formats import FileSplit, SequenceFileRecordReader
from hbmr.mapred.lib.basic import HashPartitioner, TotalOrderPartitioner
from hbmr.models import sort as sort_job
from hbmr.ops import recsort

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
TASK_GROUP = "org.apache.hadoop.mapred.Task$Counter"

ADVERSARIAL = [b"", b"\0", b"\0\0", b"ab", b"ab\0", b"ab\0\0"] + \
    [bytes([97 + (i * 7 + n) % 26 for i in range(n)]) for n in (6, 7, 8, 13, 14, 15, 21)] + \
    [b"abcdef\0", b"abcdefg", b"abcdefg\0", b"abcdefgh", b"abcdefg\0\0\0\0\0\0\0",
     b"abcdefg\0\0\0\0\0\0\0\0", b"\x7f", b"\x80", b"\xff", b"\x7f\x80", b"\x80\x7f", b"\xff\0",
     b"ab\x7f", b"ab\x80", b"ab\xff", b"abcdefg\x80", b"abcdefg\x7f", b"abcdef\xff\xff",
     b"\xff" * 7, b"\xff" * 8, b"\xff" * 14, b"\xff" * 15, b"\0" * 7, b"\0" * 8, b"\0" * 21]


# ----------------------------------------------------------------------------- builders
def _build(keys, values, kind="bytes", junk_every=7):
    """(data uint8 tensor, index int64[4, n] tensor) of frames as a SequenceFile
    holds them, with 20 junk bytes (a sync escape's place) now and then."""
    wr = BytesWritable if kind == "bytes" else Text
    parts, idx, off = [], [[], [], [], []], 0
    for i, (k, v) in enumerate(zip(keys, values)):
        if junk_every and i % junk_every == junk_every - 1:
            parts.append(b"\xff" * 20)
            off += 20
        kb, vb = wr(k).serialize(), BytesWritable(v).serialize()
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
    return data, torch.tensor(idx, dtype=torch.int64).reshape(4, len(keys))


def _values(n, rnd, lo=0, hi=60):
    return [struct.pack(">i", i) + rnd.randbytes(rnd.randint(lo, hi)) for i in range(n)]


def _key_sets():
    rnd = random.Random(17)
    n = 5000
    vocab = [f"w{i}".encode() * (1 + i % 3) for i in range(40)]
    pool = [rnd.randbytes(rnd.randint(10, 1000)) for _ in range(50)]
    prefix = rnd.randbytes(40)
    return {
        "random": ("bytes", [rnd.randbytes(rnd.randint(10, 1000)) for _ in range(n)]),
        "adversarial": ("bytes", [rnd.choice(ADVERSARIAL) for _ in range(n)]),
        "identical": ("bytes", [b"\x81k" * 500] * n),
        "prefix40": ("bytes", [prefix + rnd.randbytes(rnd.randint(0, 20)) for _ in range(n)]),
        "vocab": ("text", [b" ".join(rnd.choice(vocab) for _ in range(rnd.randint(1, 3)))
                           for _ in range(n)]),
        "duplicates": ("bytes", [rnd.choice(pool) for _ in range(n)]),
    }


_SETS = {}


def _set(name):
    """(kind, keys, data, index, {nparts/split points → CPU result}) built once."""
    if not _SETS:
        rnd = random.Random(5)
        for nm, (kind, keys) in _key_sets().items():
            data, index = _build(keys, _values(len(keys), rnd), kind)
            _SETS[nm] = {"kind": kind, "keys": keys, "data": data, "index": index, "cpu": {}}
    return _SETS[name]


def _split_points(keys, nparts):
    s = sorted(keys)
    return [s[len(s) * i // nparts] for i in range(1, nparts)]     # each equals a key


def _cpu(name, nparts, total_order):
    s = _set(name)
    key = (nparts, total_order)
    if key not in s["cpu"]:
        pts = _split_points(s["keys"], nparts) if total_order else None
        s["cpu"][key] = (pts, recsort.sort_records_cpu(s["data"], s["index"], nparts, pts))
    return s["cpu"][key]


def _write(path, records, kcls=BytesWritable, vcls=BytesWritable, **kw):
    with seqf.Writer(str(path), kcls, vcls, **kw) as w:
        for k, v in records:
            w.append(kcls(k), vcls(v))
    return str(path)


def _records(seed=3, n=300, text=False):
    rnd = random.Random(seed)
    if text:
        words = [f"word{i}" for i in range(30)]
        keys = [" ".join(rnd.choice(words) for _ in range(rnd.randint(1, 40))).encode()
                for _ in range(n)]
    else:
        keys = [rnd.randbytes(rnd.randint(0, 300)) for _ in range(n)]
    keys[5] = keys[n - 9] = keys[17]                   # duplicates
    return [(k, rnd.randbytes(rnd.randint(0, 400))) for k in keys]


# ----------------------------------------------------------------------------- CPU
def test_round_keys_order_like_bytes():
    keys = sorted(set(ADVERSARIAL))
    assert {len(k) for k in keys} >= {0, 1, 2, 6, 7, 8, 13, 14, 15, 21}
    seqs = [recsort.round_keys(k) for k in keys]
    assert all(a < b for a, b in zip(seqs, seqs[1:]))      # strictly: equal sequences = equal keys
    rnd = random.Random(1)
    more = [bytes(rnd.choice(b"\0\x01ab\x7f\x80\xff") for _ in range(rnd.randint(0, 23)))
            for _ in range(3000)]
    assert sorted(more, key=recsort.round_keys) == sorted(more)
    assert recsort.round_key(b"ab", 0) == int.from_bytes(b"ab\0\0\0\0\0", "big") << 8 | 2
    assert recsort.round_key(b"abcdefgh", 0) & 0xFF == 8 and recsort.round_key(b"abcdefgh", 1) == \
        int.from_bytes(b"h\0\0\0\0\0\0", "big") << 8 | 1
    assert len(recsort.round_keys(b"x" * 1000)) == (1000 + 1 + 6) // 7


@pytest.mark.parametrize("text", [False, True])
def test_sort_records_cpu_equals_sorted(tmp_path, text):
    cls = Text if text else BytesWritable
    recs = _records(text=text)
    path = _write(tmp_path / "in.seq", recs, cls)
    data, index = recsort.index_records(path, 0, os.path.getsize(path))
    assert index.shape == (4, len(recs))
    assert recsort.payloads(data, index) == [k for k, _ in recs]
    raw = [(cls(k).serialize(), BytesWritable(v).serialize()) for k, v in recs]
    fr = [struct.pack(">ii", len(k) + len(v), len(k)) + k + v for k, v in raw]
    hp = HashPartitioner()
    for nparts in (1, 3, 7):
        parts = [hp.getPartition(cls(k), None, nparts) for k, _ in recs]
        want = sorted(range(len(recs)), key=lambda i: (parts[i], cls.raw_sort_key(raw[i][0])))
        perm, prec, pbytes, blob = recsort.sort_records_cpu(torch.from_numpy(data),
                                                           torch.from_numpy(index), nparts)
        assert perm.tolist() == want
        assert prec == [parts.count(p) for p in range(nparts)]
        assert pbytes == [sum(len(fr[i]) for i in want if parts[i] == p) for p in range(nparts)]
        assert bytes(blob.numpy()) == b"".join(fr[i] for i in want)


def test_hash_partitions_equal_hash_partitioner():
    rnd = random.Random(2)
    keys = [rnd.randbytes(n) for n in (0, 1, 31, 32, 33, 1000) for _ in range(4)] + \
        [b"\x80" * 33, b"\xff" * 1000]
    for nparts in (3, 7, 1000003):
        assert [recsort.hash_partition_cpu(k, nparts) for k in keys] == \
            [(hash_bytes(k) & 0x7FFFFFFF) % nparts for k in keys]
    assert recsort.partitions_cpu([b"a\xff"], 5) == \
        [HashPartitioner().getPartition(Text(b"a\xff"), None, 5)]


def test_total_order_partitions_equal_partitioner():
    keys = [b"", b"a", b"ab", b"ab\0", b"b", b"b", b"c", b"\xff"]
    pts = [b"ab", b"b", b"b\0"]
    job = JobConf()
    job.set_map_output_key_class(BytesWritable)
    TotalOrderPartitioner.set_split_points(job, [BytesWritable(p) for p in pts], "inproc:t")
    top = TotalOrderPartitioner()
    top.configure(job)
    want = [top.getPartition(BytesWritable(k), None, 4) for k in keys]
    assert want == [0, 0, 1, 1, 2, 2, 3, 3]               # a key equal to a point: upper part
    assert recsort.partitions_cpu(keys, 4, pts) == want
    rnd = random.Random(4)
    order = list(range(len(keys)))
    rnd.shuffle(order)
    data, index = _build([keys[i] for i in order], [b"v%d" % i for i in order])
    perm, prec, _, _ = recsort.sort_records_cpu(data, index, 4, pts)
    assert [keys[order[i]] for i in perm.tolist()] == sorted(keys)
    assert prec == [2, 2, 2, 2]


def _reader_records(path, start, length):
    rr = SequenceFileRecordReader(JobConf(), FileSplit(path, start, length))
    out = []
    while True:
        raw = rr.next_raw()
        if raw is None:
            break
        out.append(raw)
    rr.close()
    return out


def test_indexer_equals_record_reader(tmp_path):
    recs = _records(seed=8, n=200)
    path = _write(tmp_path / "a.seq", recs)
    size = os.path.getsize(path)
    raw = open(path, "rb").read()
    with seqf.Reader(path) as r:
        sync, header = r.sync, r.header_end
    syncs = [i for i in range(len(raw)) if raw[i:i + 20] == b"\xff\xff\xff\xff" + sync]
    assert len(syncs) > 5
    # a range that starts inside a record, one without a sync, one past the last sync, all
    gap = next(b - a for a, b in zip(syncs, syncs[1:]) if b - a > 400)
    nosync = next(a for a, b in zip(syncs, syncs[1:]) if b - a == gap) + 30
    ranges = [(0, size), (header + 13, 5000), (nosync, 100), (syncs[2] + 1, syncs[5] - syncs[2]),
              (syncs[-1] + 1, size), (0, header), (size // 2, size), (syncs[3], 1), (size, 10)]
    total = 0
    for start, length in ranges:
        want = _reader_records(path, start, length)
        data, index = recsort.index_records(path, start, length)
        got = list(zip(recsort.payloads(data, index), recsort.frames(data, index)))
        assert len(got) == len(want), (start, length)
        for (payload, frame), (kb, vb) in zip(got, want):
            assert payload == kb[4:]
            assert frame == struct.pack(">ii", len(kb) + len(vb), len(kb)) + kb + vb
        total += len(want)
    assert _reader_records(path, nosync, 100) == [] and total > len(recs)
    # splits cover every record exactly once
    cut = [0, size // 3, size // 2, size]
    n = sum(recsort.index_records(path, a, b - a)[1].shape[1] for a, b in zip(cut, cut[1:]))
    assert n == len(recs)
    # Text keys with 1- and 2-byte vint prefixes; an empty file
    tpath = _write(tmp_path / "t.seq", _records(seed=9, n=60, text=True), Text)
    data, index = recsort.index_records(tpath, 0, os.path.getsize(tpath))
    want = _reader_records(tpath, 0, os.path.getsize(tpath))
    assert recsort.payloads(data, index) == [Text.raw_sort_key(k) for k, _ in want]
    assert max(index[3]) > 127 and min(index[3]) < 128
    empty = _write(tmp_path / "e.seq", [])
    data, index = recsort.index_records(empty, 0, os.path.getsize(empty))
    assert data.size == 0 and index.shape == (4, 0)
    with pytest.raises(IOError, match="compressed"):
        recsort.index_records(_write(tmp_path / "c.seq", recs[:5], compression="RECORD"), 0, 100)


def test_part_written_through_layout_equals_writer(tmp_path):
    recs = _records(seed=12, n=250) + [(b"k", b"")] * 3
    src = _write(tmp_path / "src.seq", recs)
    data, index = recsort.index_records(src, 0, os.path.getsize(src))
    data, index = torch.from_numpy(data), torch.from_numpy(index)
    order = torch.tensor(sorted(range(len(recs)), key=lambda i: recs[i][0]), dtype=torch.int32)
    got_path = str(tmp_path / "got.seq")
    with seqf.Writer(got_path, BytesWritable, BytesWritable) as w:
        assert recsort.write_part(w, data, index, order) == len(recs)
        got_sync = w.sync
    want_path = str(tmp_path / "want.seq")
    with seqf.Writer(want_path, BytesWritable, BytesWritable) as w:
        for i in order.tolist():
            w.append(BytesWritable(recs[i][0]), BytesWritable(recs[i][1]))
        want_sync = w.sync
    got, want = open(got_path, "rb").read(), open(want_path, "rb").read()
    assert want.count(want_sync) > 10
    # the same bytes, sync escapes at the same offsets, up to the files' own markers
    assert got == want.replace(want_sync, got_sync)
    with seqf.Reader(got_path) as r:
        back = [(k.get(), v.get()) for k, v in r]
    assert back == [recs[i] for i in order.tolist()]
    # appended behind records written the ordinary way
    with seqf.Writer(got_path, BytesWritable, BytesWritable) as w:
        for k, v in recs[:40]:
            w.append(BytesWritable(k), BytesWritable(v))
        recsort.write_part(w, data, index, order)
    with seqf.Reader(got_path) as r:
        assert [(k.get(), v.get()) for k, v in r] == recs[:40] + [recs[i] for i in order.tolist()]


def _random_input(tmp_path, text, maps=3, per_map=60_000):
    """RandomWriter / RandomTextWriter files plus a file of duplicated keys."""
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    conf.set_int("test.randomwrite.max_value", 3000)
    inp = str(tmp_path / "in")
    rj = JobClient.runJob(randomwriter.make_job(inp, maps, per_map, text, conf))
    assert rj.isSuccessful()
    cls = Text if text else BytesWritable
    keys = []
    for f in sorted(os.listdir(inp)):
        if f.startswith("part-"):
            with seqf.Reader(os.path.join(inp, f)) as r:
                keys += [k.bytes for k, _ in r]
    assert len(keys) > 50
    rnd = random.Random(6)
    dup = [(keys[i], rnd.randbytes(rnd.randint(0, 50))) for i in range(0, len(keys), 4)] * 2
    dup += [(keys[0], b"")] * 2
    rnd.shuffle(dup)
    _write(os.path.join(inp, "part-dup"), dup, cls, cls)
    return inp


def _parts(out):
    res = {}
    for fn in sorted(os.listdir(out)):
        if fn.startswith("part-"):
            with seqf.Reader(os.path.join(out, fn)) as r:
                recs = []
                while True:
                    raw = r.next_raw()
                    if raw is None:
                        break
                    recs.append(raw)
            res[fn] = recs
    return res


def _assert_same_parts(got_dir, want_dir):
    """Per part the same key sequence; per run of equal keys the same multiset
    of values (Hadoop does not fix their order across maps)."""
    got, want = _parts(got_dir), _parts(want_dir)
    assert list(got) == list(want) and sum(len(v) for v in want.values()) > 50
    for name in want:
        assert [k for k, _ in got[name]] == [k for k, _ in want[name]], name
        gv, wv = collections.defaultdict(list), collections.defaultdict(list)
        for k, v in got[name]:
            gv[k].append(v)
        for k, v in want[name]:
            wv[k].append(v)
        assert {k: sorted(v) for k, v in gv.items()} == {k: sorted(v) for k, v in wv.items()}
    assert os.path.exists(os.path.join(got_dir, "_SUCCESS"))
    assert not os.path.exists(os.path.join(got_dir, "_temporary"))
    return want


@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("trackers", [1, 2])
def test_sort_gpu_flag_equals_classic(tmp_path, trackers, text):
    inp = _random_input(tmp_path, text)
    to = (0.5, 1000, 10)
    with LocalCluster(JobConf(), num_trackers=trackers, cpu_slots=2) as cl:
        sort_example.run(inp, str(tmp_path / "c-hash"), 3, cluster=cl)
        sort_example.run(inp, str(tmp_path / "c-total"), 3, to, cluster=cl)
        job = sort_job.gpu_job(inp, str(tmp_path / "g-hash"), 3, maps=4)
        rj = cl.submit_job(job)
        assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
        cs = rj.getCounters()
        rj = sort_example.run(inp, str(tmp_path / "g-total"), 3, to, cluster=cl, gpu=True)
        assert rj.isSuccessful()
    want = _assert_same_parts(tmp_path / "g-hash", tmp_path / "c-hash")
    n = sum(len(v) for v in want.values())
    assert list(want) == ["part-00000", "part-00001", "part-00002"]
    assert cs.get(TASK_GROUP, "MAP_INPUT_RECORDS") == n
    assert cs.get(TASK_GROUP, "REDUCE_OUTPUT_RECORDS") == n
    assert cs.get(TASK_GROUP, "MAP_INPUT_BYTES") > 0
    want = _assert_same_parts(tmp_path / "g-total", tmp_path / "c-total")
    # totally ordered: every key of a part is below every key of the next
    cls = Text if text else BytesWritable
    seq = [cls.raw_sort_key(k) for name in want for k, _ in want[name]]
    assert seq == sorted(seq) and all(want.values())


def test_gpu_job_refuses_ineligible_inputs(tmp_path):
    recs = _records(n=40)
    comp = tmp_path / "comp"
    comp.mkdir()
    _write(comp / "part-00000", recs, compression="RECORD")
    ints = tmp_path / "ints"
    ints.mkdir()
    with seqf.Writer(str(ints / "part-00000"), IntWritable, BytesWritable) as w:
        for i, (_, v) in enumerate(recs):
            w.append(IntWritable((i * 37) % 41 - 20), BytesWritable(v))
    with pytest.raises(ValueError, match="RECORD-compressed"):
        sort_job.gpu_job(str(comp), str(tmp_path / "o1"))
    with pytest.raises(ValueError, match="key class org.apache.hadoop.io.IntWritable"):
        sort_job.gpu_job(str(ints), str(tmp_path / "o2"))
    plain = tmp_path / "plain"
    plain.mkdir()
    _write(plain / "part-00000", recs)
    with pytest.raises(ValueError, match="custom input format"):
        sort_job.gpu_job(str(plain), str(tmp_path / "o3"), in_format=randomwriter.RandomInputFormat)
    base = JobConf()
    base.set("mapred.output.key.comparator.class", "x:Y")
    with pytest.raises(ValueError, match="comparator"):
        sort_job.gpu_job(str(plain), str(tmp_path / "o4"), base=base)
    assert sort_job.gpu_job(str(plain), str(tmp_path / "o5"), 2).get_num_reduce_tasks() == 2
    # `sort -gpu` on such inputs is the classic job
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    for name, d in (("comp", comp), ("ints", ints)):
        sort_example.run(str(d), str(tmp_path / f"{name}-c"), 2, conf=local)
        sort_example.run(str(d), str(tmp_path / f"{name}-g"), 2, conf=local, gpu=True)
        got, want = _parts(tmp_path / f"{name}-g"), _parts(tmp_path / f"{name}-c")
        assert got == want and sum(len(v) for v in want.values()) == len(recs)


# ----------------------------------------------------------------------------- GPU
def _check_gpu_sort(data, index, nparts, pts, want, stats=None):
    perm, prec, pbytes, blob = recsort.sort_records(data.cuda(), index.cuda(), nparts, pts,
                                                    stats=stats)
    wperm, wrec, wbytes, wblob = want
    assert prec == wrec and pbytes == wbytes
    assert torch.equal(perm.cpu(), wperm)
    assert torch.equal(blob.cpu(), wblob)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "adversarial", "identical", "prefix40", "vocab",
                                  "duplicates"])
def test_gpu_sort_records_equals_cpu(name):
    s = _set(name)
    for nparts, total_order in ((1, False), (3, False), (4, True)):
        pts, want = _cpu(name, nparts, total_order)
        stats = {}
        _check_gpu_sort(s["data"], s["index"], nparts, pts, want, stats)
        if name == "identical":
            assert stats["rounds"] == (1000 + 1 + 6) // 7       # every round is active
        if name == "prefix40":
            assert stats["rounds"] >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_gpu_sort_records_small(n):
    for name in ("random", "adversarial", "duplicates"):
        s = _set(name)
        rnd = random.Random(n)
        data, index = _build(s["keys"][:n], _values(n, rnd), s["kind"], junk_every=3)
        for nparts, pts in ((1, None), (3, None), (3, _split_points(s["keys"][:n], 3) if n else
                                       [b"a", b"b"])):
            want = recsort.sort_records_cpu(data, index, nparts, pts)
            _check_gpu_sort(data, index, nparts, pts, want)


@pytest.mark.gpu
def test_gpu_round_keys_and_hash_partition():
    rnd = random.Random(3)
    keys = ADVERSARIAL + [rnd.randbytes(n) for n in (0, 1, 31, 32, 33, 1000) for _ in range(5)] + \
        [bytes(rnd.randint(0x80, 0xFF) for _ in range(n)) for n in (1, 31, 32, 33, 1000)]
    data, index = _build(keys, [b"v"] * len(keys), junk_every=2)
    data, index = data.cuda(), index.cuda()
    for nparts in (3, 7, 1000003):
        got = recsort.hash_partition(data, index, nparts).tolist()
        assert got == [(hash_bytes(k) & 0x7FFFFFFF) % nparts for k in keys]
    rec = torch.arange(len(keys), dtype=torch.int32, device="cuda")
    for d in (0, 1, 2, 142, 143):
        got = recsort.round_keys_device(data, index, rec, d).cpu().numpy().view(np.uint64)
        assert got.tolist() == [recsort.round_key(k, d) for k in keys]


def _gather_case():
    """Frames of every length residue mod 16 at every source and destination
    alignment mod 16, zero-length ones, and one of 70,000 bytes."""
    rnd = random.Random(9)
    lens = [r + 16 * ((sa + da) % 4) for sa in range(16) for da in range(16) for r in range(16)]
    align = [(sa, da) for sa in range(16) for da in range(16) for _ in range(16)]
    lens.insert(1000, 70_000)
    align.insert(1000, (5, 11))
    lens += [0, 0, 1029, 1024, 1040]
    align += [(3, 3), (0, 9), (15, 1), (0, 0), (1, 0)]
    foff, dst, so, do = [], [None] * len(lens), 0, 0
    for ln, (sa, _) in zip(lens, align):
        so += (sa - so) % 16
        foff.append(so)
        so += ln
    order = list(range(len(lens)))
    rnd.shuffle(order)
    for i in order:                       # the destination holds the frames in shuffled order
        do += (align[i][1] - do) % 16
        dst[i] = do
        do += lens[i]
    src = np.frombuffer(rnd.randbytes(so), dtype=np.uint8)
    return src, np.array(foff), np.array(lens), np.array(order), np.array([dst[i] for i in order]), do


@pytest.mark.gpu
def test_gpu_gather_frames_every_alignment():
    src, foff, lens, order, dst, total = _gather_case()
    assert {(int(f) % 16, int(d) % 16, int(n) % 16)
            for f, d, n in zip(foff[order], dst, lens[order])} >= \
        {(a, b, c) for a in range(16) for b in range(16) for c in range(16)}
    want = np.zeros(total, dtype=np.uint8)
    mask = np.zeros(total, dtype=bool)
    for i, d in zip(order.tolist(), dst.tolist()):
        want[d:d + lens[i]] = src[foff[i]:foff[i] + lens[i]]
        mask[d:d + lens[i]] = True
    args = [torch.from_numpy(a.astype(np.int64)).cuda() for a in (foff, lens, dst)]
    pad = torch.zeros(src.size + 1, dtype=torch.uint8, device="cuda")
    for shift in (0, 1):                  # the source buffer itself aligned and not
        buf = pad[shift:shift + src.size]
        buf.copy_(torch.from_numpy(src.copy()))
        assert buf.data_ptr() % 16 == shift
        got = recsort.gather_frames(buf, torch.from_numpy(order.astype(np.int32)).cuda(), args[0],
                                    args[1], args[2], total).cpu().numpy()
        assert np.array_equal(got[mask], want[mask])
    # without a permutation, back to back (the layout of a map output)
    dense = np.cumsum(lens) - lens
    got = recsort.gather_frames(pad[:src.size].copy_(torch.from_numpy(src.copy())), None, args[0],
                                args[1], torch.from_numpy(dense).cuda(), int(lens.sum()))
    assert bytes(got.cpu().numpy()) == b"".join(bytes(src[f:f + n]) for f, n in zip(foff, lens))
    with pytest.raises(ValueError, match="outside"):
        recsort.gather_frames(pad[:src.size], None, args[0], args[1], args[2], total - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("text", [False, True])
def test_gpu_sort_job_equals_classic(tmp_path, text):
    inp = _random_input(tmp_path, text, maps=3, per_map=150_000)
    to = (0.5, 1000, 10)
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    sort_example.run(inp, str(tmp_path / "c-hash"), 3, conf=local)
    classic = sort_example.make_job(inp, str(tmp_path / "c-total"), 3, to, local)
    assert JobClient.runJob(classic).isSuccessful()
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        for out, pfile in (("g-hash", None),
                           ("g-total", classic.get("total.order.partitioner.path"))):
            job = sort_job.gpu_job(inp, str(tmp_path / out), 3, pfile, maps=6)
            rj = cl.submit_job(job)
            assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
            assert rj.getCounters().get(JOB_GROUP, "GPU_MAP_TASKS") >= 6
    _assert_same_parts(tmp_path / "g-hash", tmp_path / "c-hash")
    _assert_same_parts(tmp_path / "g-total", tmp_path / "c-total")
