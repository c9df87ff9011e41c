"""Snappy RECORD- and BLOCK-compressed SequenceFile splits for the record
kernels (hbmr/ops/seqz.py, native/io/seqzindex.cc): the host plan against the
Python reader, the CPU twin, eligibility, the three jobs on CPU slots against
the classic jobs, malformed files, and the plan stand-alone under sanitizers.
The device side is tests/test_seqz_gpu.py."""
from __future__ import annotations

import collections
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

from hbmr.benchmarks import sortvalidator
from hbmr.examples import join as join_example
from hbmr.examples import sort as sort_example
from hbmr.io import sequencefile as seqf
from hbmr.io.compress import SnappyCodec
from hbmr.io.vint import decode_vint
from hbmr.io.writable import BytesWritable, Text
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.formats import FileSplit, SequenceFileRecordReader
from hbmr.mapred.join import TupleWritable
from hbmr.models import join as join_job
from hbmr.models import records
from hbmr.models import sort as sort_job
from hbmr.models import sortvalidate as validate_job
from hbmr.ops import recsort, seqz, snappydec

MODES = ("RECORD", "BLOCK")
KEY_CLASSES = (BytesWritable, Text)
COUNTS = (0, 1, 2, 65, 300)


def make_records(n, seed=5, text=False, max_value=2500):
    """(key payload, value payload) pairs: empty keys, empty values, values of
    several Snappy chunks at buffer size 1024, compressible and not."""
    rnd = random.Random(seed * 1000 + n)
    out = []
    for i in range(n):
        kl = (0, 1, 3, 10, 40, 130)[rnd.randrange(6)] if i % 5 else 0
        if text:
            k = bytes(rnd.randrange(97, 123) for _ in range(kl))
        else:
            k = rnd.randbytes(kl)
        vl = 0 if i % 7 == 3 else rnd.choice((1, 20, 200, 900, max_value))
        v = rnd.randbytes(vl) if i % 2 else bytes(rnd.randrange(97, 100) for _ in range(vl))
        out.append((k, v))
    return out


def write_file(path, recs, kcls=BytesWritable, mode="BLOCK", block_size=300, vcls=BytesWritable,
               codec=None, raw_empty=False):
    """``raw_empty``: an empty value is written as zero raw bytes (no
    BytesWritable length), the zero-length value of the loader's contract."""
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    kw = {}
    if mode != "NONE":
        kw = dict(compression=mode, codec=codec or SnappyCodec(buffer_size=1024),
                  block_size=block_size)
    with seqf.Writer(str(path), kcls, vcls, **kw) as w:
        for k, v in recs:
            if raw_empty and not v:
                w.append_raw(kcls(k).serialize(), b"")
            else:
                w.append(kcls(k), vcls(v))
    return str(path)


def reader_records(path, start, length):
    rr = SequenceFileRecordReader(None, FileSplit(path, start, length))
    out = list(iter(rr.next_raw, None))
    rr.close()
    return out


def pack(recs):
    return b"".join(struct.pack(">ii", len(k) + len(v), len(k)) + k + v for k, v in recs)


def _vints(col, n):
    out, at = [], 0
    for _ in range(n):
        v, at = decode_vint(col, at)
        out.append(v)
    assert at == len(col)
    return out


def execute_plan(pl):
    """The records and the index of a plan, carried out on the host: the chunks
    through the decoder's twin, the columns through Python."""
    raw = np.fromfile(pl["file"], dtype=np.uint8, count=pl["hi"] - pl["lo"], offset=pl["lo"])
    src = torch.from_numpy(raw)
    chunks = torch.from_numpy(pl["chunks"])
    if pl["mode"] == seqz.RECORD:
        data = torch.zeros(pl["data_bytes"], dtype=torch.uint8)
        _, status = snappydec.decode_chunks(src, chunks, data)
        assert not status.any()
        data, rows = data.numpy(), pl["recs"]
        recs = []
        for foff, flen, _, _, ksrc, klen, vlen in rows.T.tolist():
            assert flen == 8 + klen + vlen
            recs.append((raw[ksrc:ksrc + klen].tobytes(),
                         data[foff + 8 + klen:foff + flen].tobytes()))
        return recs, rows[:4]
    cols = torch.zeros(pl["cols_bytes"], dtype=torch.uint8)
    _, status = snappydec.decode_chunks(src, chunks, cols)
    assert not status.any()
    cols = cols.numpy().tobytes()
    recs = []
    for n, base, o0, l0, o1, l1, o2, l2, o3, l3 in pl["blocks"].T.tolist():
        assert base == len(recs)
        klens, vlens = _vints(cols[o0:o0 + l0], n), _vints(cols[o2:o2 + l2], n)
        assert sum(klens) == l1 and sum(vlens) == l3
        for kl, vl in zip(klens, vlens):
            recs.append((cols[o1:o1 + kl], cols[o3:o3 + vl]))
            o1, o3 = o1 + kl, o3 + vl
    return recs, None


def sync_positions(path):
    with seqf.Reader(path) as r:
        sync, at = r.sync, r.header_end
    body = open(path, "rb").read()
    out = []
    while True:
        at = body.find(b"\xff\xff\xff\xff" + sync, at)
        if at < 0:
            return out
        out.append(at)
        at += 20


def windows(path):
    """Cuts of the file: its start, a sync escape, inside a block or record
    behind another, the middle, one byte before the end, the end."""
    size = os.path.getsize(path)
    syncs = sync_positions(path)
    cuts = {0, size // 2, max(0, size - 1), size}
    if syncs:
        cuts |= {syncs[len(syncs) // 3], min(size, syncs[len(syncs) // 2] + 27),
                 min(size, syncs[-1] + 3)}
    cuts = sorted(cuts)
    return list(zip(cuts, cuts[1:]))


# ----------------------------------------------------------------------------- plan
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kcls", KEY_CLASSES)
@pytest.mark.parametrize("mode", MODES)
def test_plan_equals_record_reader(tmp_path, mode, kcls, n):
    recs = make_records(n, text=kcls is Text)
    path = write_file(tmp_path / "f.seq", recs, kcls, mode, raw_empty=True)
    size = os.path.getsize(path)
    want = reader_records(path, 0, size)
    assert len(want) == n and (n < 65 or any(v == b"" for _, v in want))
    pl = seqz.plan(path, 0, size)
    got, index = execute_plan(pl)
    assert got == want and pl["n"] == n and pl["data_bytes"] == len(pack(want))
    if index is not None:
        data, twin_index = seqz.pack_records(want, pl["prefix"])
        assert np.array_equal(index, twin_index.numpy())
    if n >= 65:
        if mode == "BLOCK":
            assert pl["blocks"].shape[1] > 5
        assert pl["chunks"].shape[1] > n // 2       # multi-chunk values or columns
    seen = []
    for a, b in windows(path):
        pl = seqz.plan(path, a, b - a)
        got, _ = execute_plan(pl)
        assert got == reader_records(path, a, b - a), (a, b)
        seen += got
    assert seen == want


def test_windows_cut_inside_a_block_and_on_a_sync(tmp_path):
    path = write_file(tmp_path / "f.seq", make_records(300), BytesWritable, "BLOCK")
    syncs = sync_positions(path)
    cuts = [a for a, _ in windows(path)]
    assert any(c in syncs for c in cuts) and any(c - 27 in syncs for c in cuts)
    # a block belongs to the window its sync escape starts in
    on = syncs[len(syncs) // 3]
    assert seqz.plan(path, on, 1)["n"] > 0 and seqz.plan(path, on + 1, 1)["n"] == 0


# ----------------------------------------------------------------------------- twin
@pytest.mark.parametrize("kcls", KEY_CLASSES)
@pytest.mark.parametrize("mode", MODES)
def test_twin_equals_frames_packed_by_hand(tmp_path, mode, kcls):
    recs = make_records(65, text=kcls is Text)
    path = write_file(tmp_path / "f.seq", recs, kcls, mode, raw_empty=True)
    with seqf.Reader(path) as r:
        raw = list(iter(r.next_raw, None))
    assert len(raw) == len(recs) and [v[4:] for _, v in raw] == [v for _, v in recs]
    assert any(v == b"" for _, v in raw)
    data, index = seqz.load_split(path, 0, os.path.getsize(path), "cpu")
    assert data.numpy().tobytes() == pack(raw)
    assert recsort.frames(data, index) == [pack([r]) for r in raw]
    assert recsort.payloads(data, index) == [k for k, _ in recs]
    a, b = windows(path)[1]
    data, index = records.load_record_split(path, a, b - a, "cpu")
    assert data.numpy().tobytes() == pack(reader_records(path, a, b - a))


# ----------------------------------------------------------------------------- eligibility
def test_snappy_files_are_eligible_default_codec_files_are_not(tmp_path):
    recs = make_records(20)
    for mode in MODES:
        snap = write_file(tmp_path / f"{mode}.snappy.seq", recs, BytesWritable, mode)
        seen = set()
        assert records.file_reason(snap, seen) is None
        assert seen == {(BytesWritable.java_name(), BytesWritable.java_name())}
        assert records.is_snappy_compressed(snap)
        zl = write_file(tmp_path / f"{mode}.zlib.seq", recs, BytesWritable, mode, codec="default")
        assert records.file_reason(zl) == f"{mode}-compressed input {zl}"
        assert not records.is_snappy_compressed(zl)
        with pytest.raises(IOError):
            recsort.index_records(snap, 0, os.path.getsize(snap))
    plain = write_file(tmp_path / "plain.seq", recs, BytesWritable, "NONE")
    assert records.file_reason(plain) is None and not records.is_snappy_compressed(plain)
    base = JobConf()
    base.set_boolean("mapred.output.compress", True)
    assert sort_job.why_ineligible(str(tmp_path / "RECORD.snappy.seq"), base) == "compressed output"


# ----------------------------------------------------------------------------- jobs
JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
TASK_GROUP = "org.apache.hadoop.mapred.Task$Counter"
SNAPPY_GROUP, DECODED = "hbmr.CompressedInputCounters", "SNAPPY_DECODED_BYTES"


def local_conf():
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    return conf


def last_job(cl):
    return cl.jt.get_job(list(cl.jt.jobs)[-1])


def parts(out):
    res = {}
    for fn in sorted(os.listdir(out)):
        if fn.startswith("part-"):
            with seqf.Reader(os.path.join(out, fn)) as r:
                res[fn] = list(iter(r.next_raw, None))
    return res


def assert_same_sort(got_dir, want_dir):
    """Per part the same key sequence; per run of equal keys the same multiset
    of values (Hadoop does not fix their order across maps)."""
    got, want = parts(got_dir), parts(want_dir)
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
    return want


def sort_input(root, text=False, n=400):
    """A RECORD- and a BLOCK-compressed Snappy file (and keys in both)."""
    kcls = Text if text else BytesWritable
    recs = make_records(n, seed=9, text=text, max_value=1500)
    inp = root / "in"
    write_file(inp / "part-00000", recs[:n // 2] + recs[:20], kcls, "RECORD")
    write_file(inp / "part-00001", recs[n // 2:] + recs[:20], kcls, "BLOCK", block_size=4000)
    return str(inp)


def join_inputs(root, nparts=2):
    """Two sorted sources: one RECORD-, one BLOCK-compressed."""
    rnd = random.Random(4)
    pool = sorted({rnd.randbytes(rnd.randint(0, 60)) for _ in range(200)} | {b""})
    dirs = [str(root / "src0"), str(root / "src1")]
    for p in range(nparts):
        for s, mode in enumerate(MODES):
            keys = sorted(rnd.choices(pool, k=120))
            recs = [(k, rnd.randbytes(rnd.choice((0, 5, 60, 1200)))) for k in keys]
            write_file(os.path.join(dirs[s], f"part-{p:05d}"), recs, BytesWritable, mode,
                       block_size=3000)
    return dirs


def compress_dir(d, mode):
    """Rewrite the parts of a directory as Snappy-compressed files."""
    for fn in sorted(os.listdir(d)):
        if fn.startswith("part-"):
            path = os.path.join(d, fn)
            with seqf.Reader(path) as r:
                kc, vc, raw = r.key_class, r.value_class, list(iter(r.next_raw, None))
            with seqf.Writer(path, kc, vc, compression=mode, codec=SnappyCodec(buffer_size=1024),
                             block_size=3000) as w:
                for kb, vb in raw:
                    w.append_raw(kb, vb)


def run_sort_jobs(cl, tmp, inp):
    """`sort -gpu`, hash and -totalOrder, over ``inp`` on ``cl``; returns the
    RunningJobs (their outputs are g-hash and g-total)."""
    to = (0.5, 1000, 10)
    rjs = []
    for out, kw in (("g-hash", {}), ("g-total", {"total_order": to})):
        rj = sort_example.run(inp, str(tmp / out), 3, kw.get("total_order"), cluster=cl, gpu=True)
        assert rj.isSuccessful() and rj.getJobName() == "sorter-gpu"
        rjs.append(rj)
    return rjs


def classic_sorts(tmp, inp):
    to = (0.5, 1000, 10)
    sort_example.run(inp, str(tmp / "c-hash"), 3, conf=local_conf())
    sort_example.run(inp, str(tmp / "c-total"), 3, to, conf=local_conf())


@pytest.mark.parametrize("text", [False, True])
def test_sort_on_cpu_slots_equals_classic(tmp_path, text):
    inp = sort_input(tmp_path, text)
    classic_sorts(tmp_path, inp)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        rjs = run_sort_jobs(cl, tmp_path, inp)
    want = assert_same_sort(tmp_path / "g-hash", tmp_path / "c-hash")
    n = sum(len(v) for v in want.values())
    cs = rjs[0].getCounters()
    assert cs.get(TASK_GROUP, "MAP_INPUT_RECORDS") == n == 440
    nbytes = sum(8 + len(k) + len(v) for v in want.values() for k, v in v)
    assert cs.get(TASK_GROUP, "MAP_INPUT_BYTES") == nbytes
    assert cs.get(SNAPPY_GROUP, DECODED) == nbytes
    assert_same_sort(tmp_path / "g-total", tmp_path / "c-total")


def test_join_on_cpu_slots_equals_classic(tmp_path):
    dirs = join_inputs(tmp_path)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        for op in ("inner", "outer"):
            job = join_example.make_job(dirs, str(tmp_path / f"c-{op}"), op, 0, local_conf(),
                                        out_value=TupleWritable)
            assert JobClient.runJob(job).isSuccessful()
            rj = cl.submit_job(join_job.gpu_job(dirs, str(tmp_path / f"g-{op}"), op))
            assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
            assert rj.getJobName() == join_job.JOB_NAME
            want, got = parts(tmp_path / f"c-{op}"), parts(tmp_path / f"g-{op}")
            assert list(want) == ["part-00000", "part-00001"] and got == want
            assert sum(len(v) for v in want.values()) > 50


@pytest.mark.parametrize("total_order", [False, True])
def test_sortvalidate_on_cpu_slots_equals_classic(tmp_path, total_order):
    inp = sort_input(tmp_path)
    out = str(tmp_path / "out")
    sort_example.run(inp, out, 3, (0.5, 1000, 10) if total_order else None, conf=local_conf())
    compress_dir(out, "BLOCK" if total_order else "RECORD")
    want = sortvalidator.validate(inp, out, total_order=total_order)
    assert want["ok"] and want["IN_RECORDS"] == 440
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        got = sortvalidator.validate(inp, out, cluster=cl, total_order=total_order, gpu=True)
        assert last_job(cl).getJobName() == validate_job.JOB_NAME
    assert got == want and list(got) == list(want)


# ----------------------------------------------------------------------------- malformed
def _block_layout(path):
    """Of the first block: the position of its sync escape, of its record count
    and per column (position of the length vint, position of the stream,
    compressed length)."""
    with seqf.Reader(path) as r:
        at = r.header_end
    body = open(path, "rb").read()
    nat = at + 20
    _, p = decode_vint(body, nat)
    cols = []
    for _ in range(4):
        clen, q = decode_vint(body, p)
        cols.append((p, q, clen))
        p = q + clen
    return at, nat, cols, body


def malformed_files(root):
    """{case: path}: one file per framing error of the plan."""
    recs = make_records(40, seed=2, max_value=300)
    good = write_file(root / "good-block.seq", recs, BytesWritable, "BLOCK", block_size=1 << 20)
    at, nat, cols, body = _block_layout(good)
    assert cols[3][1] + cols[3][2] == len(body)           # one block

    def put(name, data):
        p = root / f"{name}.seq"
        p.write_bytes(bytes(data))
        return str(p)

    out = {}
    b = bytearray(body)
    b[at + 7] ^= 0x55
    out["wrong-sync"] = put("wrong-sync", b)
    b = bytearray(body)
    b[at:at + 4] = struct.pack(">i", 5)
    out["missing-sync"] = put("missing-sync", b)
    out["truncated-block"] = put("truncated-block", body[:cols[0][0]])
    out["column-past-end"] = put("column-past-end", body[:cols[3][1] + cols[3][2] // 2])
    b = bytearray(body)
    orig = struct.unpack(">i", body[cols[1][1]:cols[1][1] + 4])[0]
    assert orig > 1
    b[cols[1][1]:cols[1][1] + 4] = struct.pack(">i", orig - 1)
    out["chunks-do-not-add-up"] = put("chunks-do-not-add-up", b)
    out["vint-off-file"] = put("vint-off-file", body[:nat])
    b = bytearray(body)
    assert b[nat] == 40
    b[nat] = 127                                           # more records than length vints
    out["count-above-columns"] = put("count-above-columns", b)
    # RECORD: a sync escape inside the file, and a value whose chunks overshoot
    rec = write_file(root / "good-record.seq", make_records(65, seed=2), BytesWritable, "RECORD")
    body = open(rec, "rb").read()
    syncs = sync_positions(rec)
    assert syncs
    b = bytearray(body)
    b[syncs[0] + 9] ^= 0x55
    out["record-wrong-sync"] = put("record-wrong-sync", b)
    pl = seqz.plan(rec, 0, len(body))
    r = int(np.flatnonzero(pl["recs"][6] > 1)[0])
    vpos = pl["lo"] + int(pl["recs"][4][r] + pl["recs"][5][r])
    b = bytearray(body)
    b[vpos:vpos + 4] = struct.pack(">i", struct.unpack(">i", body[vpos:vpos + 4])[0] - 1)
    out["record-chunks-do-not-add-up"] = put("record-chunks-do-not-add-up", b)
    out["record-truncated"] = put("record-truncated", body[:len(body) - 3])
    return good, rec, out


MALFORMED = {"wrong-sync": "sync check failure", "missing-sync": "expected sync before block",
             "truncated-block": "truncated block",
             "column-past-end": "compressed length past the end",
             "chunks-do-not-add-up": "do not add up", "vint-off-file": "vint runs off the file",
             "count-above-columns": "record count above what its length columns hold",
             "record-wrong-sync": "sync check failure",
             "record-chunks-do-not-add-up": "do not add up", "record-truncated": "corrupt record"}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_file_raises_ioerror_naming_the_file(tmp_path, case):
    _, _, bad = malformed_files(tmp_path)
    path = bad[case]
    with pytest.raises(IOError, match=re.escape(path) + ".*" + MALFORMED[case]) as e:
        seqz.plan(path, 0, os.path.getsize(path))
    assert ("block 0" in str(e.value)) == (not case.startswith("record-"))


# ----------------------------------------------------------------------------- sanitizers
def _selftest_args(path):
    with seqf.Reader(path) as r:
        mode = seqz.BLOCK if r.block_compressed else seqz.RECORD
        prefix = 4 if r.key_class_name == recsort.KEY_CLASSES[0] else 0
        return [path, str(r.header_end), str(mode), str(prefix)]


def test_plan_stand_alone_under_asan_ubsan(tmp_path):
    """native/tests/seqzindex_selftest.cc, a program of its own with the plan
    compiled in under -fsanitize=address,undefined, over good files (whole and
    in windows) and the malformed ones."""
    import importlib.util
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hbmr_native_build",
                                                  os.path.join(root, "native", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_sanitized("asan")["seqzindex_selftest"]
    good_block, good_record, bad = malformed_files(tmp_path)
    text = write_file(tmp_path / "text.seq", make_records(65, text=True), Text, "BLOCK")
    empty = write_file(tmp_path / "empty.seq", [], Text, "RECORD")
    args, want = [], []
    for path in (good_block, good_record, text, empty):
        size = os.path.getsize(path)
        for a, b in [(0, size)] + windows(path):
            pl = seqz.plan(path, a, b - a)
            table = pl["recs"] if pl["mode"] == seqz.RECORD else pl["blocks"]
            nb = 0 if pl["mode"] == seqz.RECORD else table.shape[1]
            words = [pl["lo"], pl["hi"], pl["n"], pl["chunks"].shape[1], nb, pl["data_bytes"],
                     pl["cols_bytes"]] + pl["chunks"].reshape(-1).tolist() + \
                table.reshape(-1).tolist()
            want.append(" ".join(str(w) for w in words))
            args += _selftest_args(path) + [str(a), str(b - a)]
    for case in sorted(bad):
        size = os.path.getsize(bad[case])
        src = good_record if case.startswith("record") else good_block
        args += [bad[case]] + _selftest_args(src)[1:] + ["0", str(size)]
        want.append("bad")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want
