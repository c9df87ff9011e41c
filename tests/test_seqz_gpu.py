"""The device side of Snappy-compressed SequenceFile splits (hbmr/ops/seqz.py,
native/kernels/seqblock.hip): the vint kernel and the assemble kernel alone,
``load_split`` against the twin, corrupted chunks, and the three jobs on a GPU
cluster against the classic jobs."""
from __future__ import annotations

import os
import random
import re
import struct

import numpy as np
import pytest
import torch

from hbmr.benchmarks import sortvalidator
from hbmr.examples import join as join_example
from hbmr.io.vint import encode_vint
from hbmr.io.writable import BytesWritable, Text
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.join import TupleWritable
from hbmr.models import join as join_job
from hbmr.models import sort as sort_job
from hbmr.models import sortvalidate as validate_job
from hbmr.ops import seqz
from test_seqz import (DECODED, JOB_GROUP, KEY_CLASSES, MODES, SNAPPY_GROUP, assert_same_sort,
                       compress_dir, join_inputs, last_job, local_conf,
                       make_records, parts, sort_input, windows, write_file)

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -7


# ----------------------------------------------------------------------------- vint kernel
def _vint_layout(blocks, mis=0, spoil=None):
    """(cols bytes, table int64[10, b], n): the length columns of ``blocks``
    ([(klens, vlens)]) laid out from offset ``mis`` on, one block after another
    with an odd gap; the keys and values columns are the (unread) range [0,
    sum).  ``spoil``: {block: fn(kcol, vcol, n) -> (kcol, vcol, n)}."""
    table = np.zeros((10, len(blocks)), dtype=np.int64)
    buf = bytearray(mis)
    base = 0
    for b, (klens, vlens) in enumerate(blocks):
        kcol = b"".join(encode_vint(x) for x in klens)
        vcol = b"".join(encode_vint(x) for x in vlens)
        n = len(klens)
        if spoil and b in spoil:
            kcol, vcol, n = spoil[b](kcol, vcol, n)
        table[0, b], table[1, b] = n, base
        table[2, b], table[3, b] = len(buf), len(kcol)
        buf += kcol + b"\x7f" * (b % 3)
        table[6, b], table[7, b] = len(buf), len(vcol)
        buf += vcol + b"\x7f" * ((b + 1) % 3)
        table[5, b], table[9, b] = sum(klens), sum(vlens)
        base += n
    return bytes(buf), table, base


def _run_vint(blocks, mis=0, spoil=None, cols_bytes=None):
    raw, table, n = _vint_layout(blocks, mis, spoil)
    need = max(len(raw), int(table[5].max(initial=0)), int(table[9].max(initial=0)))
    cols = torch.empty(cols_bytes or need, dtype=torch.uint8, device="cuda")
    cols[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if raw else \
        cols[:0]
    klen = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    vlen = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    k, v, status = seqz.decode_lengths(cols, torch.from_numpy(table), n, klen=klen, vlen=vlen)
    torch.cuda.synchronize()
    assert k.data_ptr() == klen.data_ptr()
    return klen.cpu().tolist(), vlen.cpu().tolist(), status.cpu().tolist(), table


def _mixed_lengths(rnd, n):
    """Lengths of every vint size that keep a column sum small."""
    out = []
    for _ in range(n):
        kind = rnd.randrange(8)
        out.append((0, 1, 127, 128, 255, 256, rnd.randrange(128), rnd.randrange(70000))[kind])
    return out


def test_vint_every_size():
    lens = [0, 127, 128, 255, 256, 65535, 65536, 1 << 24, (1 << 31) - 1]
    small = [3, 0, 1, 200, 0, 70000, 5, 127, 128]
    for blocks in ([(lens, small)], [(small, lens[:8] + [0]), (lens[:8] + [1], small)]):
        k, v, status, _ = _run_vint(blocks)
        assert status == [0] * len(blocks)
        want_k = sum((b[0] for b in blocks), [])
        want_v = sum((b[1] for b in blocks), [])
        assert k == want_k + [SENTINEL] * GUARD and v == want_v + [SENTINEL] * GUARD


@pytest.mark.parametrize("mis", range(16))
def test_vint_counts_blocks_and_misalignment(mis):
    rnd = random.Random(mis)
    counts = [0, 1, 2, 63, 64, 65, 257]
    nblocks = (1, 2, 65)[mis % 3]
    blocks = []
    for b in range(nblocks):
        n = counts[(b + mis) % len(counts)]
        blocks.append((_mixed_lengths(rnd, n), _mixed_lengths(rnd, n)))
    k, v, status, _ = _run_vint(blocks, mis)
    assert status == [0] * nblocks
    assert k == sum((b[0] for b in blocks), []) + [SENTINEL] * GUARD
    assert v == sum((b[1] for b in blocks), []) + [SENTINEL] * GUARD


SPOILS = {
    "mid-vint": lambda k, v, n: (k[:-1], v, n),                 # the last vint has 3 bytes
    "one-too-few": lambda k, v, n: (k, v, n + 1),
    "one-too-many": lambda k, v, n: (k, v + b"\x05", n),
    "negative": lambda k, v, n: (b"\x80" + k[1:], v, n),
    "left-over-after-n": lambda k, v, n: (k + b"\x00\x00", v, n),
}


@pytest.mark.parametrize("where", [1, 2])
@pytest.mark.parametrize("case", sorted(SPOILS))
def test_vint_bad_block_between_good_ones(case, where):
    """The bad block (in the middle, then last before the guard slots) gets a
    nonzero status, the good ones their lengths, the guard slots nothing."""
    rnd = random.Random(3)
    blocks = []
    for n in (65, 70, 64):
        kl = _mixed_lengths(rnd, n - 1) + [40000]
        blocks.append((kl[:1] + [0] * 8 + kl[9:] if case == "negative" else kl,
                       _mixed_lengths(rnd, n)))
    k, v, status, table = _run_vint(blocks, 5, {where: SPOILS[case]})
    assert [s != 0 for s in status] == [b == where for b in range(3)], status
    at = 0
    for b, (kl, vl) in enumerate(blocks):
        n = int(table[0, b])
        if b != where:
            assert k[at:at + n] == kl and v[at:at + n] == vl
        at += n
    assert k[at:] == [SENTINEL] * GUARD and v[at:] == [SENTINEL] * GUARD


def test_vint_sums_must_match_the_columns():
    blocks = [([1, 2, 3], [4, 5, 6]), ([7, 8], [9, 10]), ([1], [1])]
    raw, table, n = _vint_layout(blocks)
    table[9, 1] += 1
    cols = torch.zeros(64, dtype=torch.uint8, device="cuda")
    cols[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    k, v, status = seqz.decode_lengths(cols, torch.from_numpy(table), n)
    assert status.cpu().tolist() == [0, seqz.SUM, 0]
    assert k.cpu().tolist() == [1, 2, 3, 7, 8, 1]


# ----------------------------------------------------------------------------- index kernel
def _text_key(n, fill=b"t"):
    return encode_vint(n) + fill * n


INDEX_CASES = {
    # prefix: (good keys, {bad kind: key bytes})
    4: ([struct.pack(">i", n) + b"b" * n for n in (0, 1, 5, 300)],
        {"klen-3": b"\0\0\0", "klen-0": b"", "wrong-length": struct.pack(">i", 5) + b"abc",
         "negative-length": struct.pack(">i", -1) + b"abc"}),
    0: ([_text_key(n) for n in (0, 1, 127, 128, 255, 256, 70000)],       # 1-, 2- and 3-byte vints
        {"vint-longer-than-key": b"\x8e\x01", "negative-vint": b"\x80" + b"\0" * 8 + b"xy",
         "klen-0": b"", "length-short": encode_vint(4) + b"abc",
         "length-long": encode_vint(300) + b"a" * 301}),
}


def _index_layout(blocks, mis):
    """(cols bytes, table): the keys columns of ``blocks`` ([[key bytes]]) one
    after another from offset ``mis`` on with odd gaps; the other columns are
    not read by the index build."""
    table = np.zeros((10, len(blocks)), dtype=np.int64)
    buf, base = bytearray(b"\xee" * mis), 0
    for b, keys in enumerate(blocks):
        table[0, b], table[1, b] = len(keys), base
        table[4, b], table[5, b] = len(buf), sum(len(k) for k in keys)
        table[8, b] = 1000 * b
        buf += b"".join(keys) + b"\xee" * (b % 3)
        base += len(keys)
    return bytes(buf), table


def _run_index(prefix, blocks, vlens, mis=3, status=None, stretch_last=0):
    raw, table = _index_layout(blocks, mis)
    keys = [k for blk in blocks for k in blk]
    klen = [len(k) for k in keys]
    klen[-1] += stretch_last
    status = torch.zeros(len(blocks), dtype=torch.int32, device="cuda") if status is None else \
        status
    index, ksrc, vsrc, kl, vl = seqz.build_index(
        _dev(raw), torch.from_numpy(table).cuda(), _i64(klen), _i64(vlens), status, prefix)
    torch.cuda.synchronize()
    return index.cpu().tolist(), ksrc.cpu().tolist(), vsrc.cpu().tolist(), status.cpu().tolist(), \
        table, keys


def _want_index(prefix, keys, klen, vlens):
    rows, at, bad = [], 0, []
    for k, kl, vl in zip(keys, klen, vlens):
        try:
            assert kl == len(k)
            poff, plen = seqz._payload(k, prefix)
        except (IOError, AssertionError):
            poff, plen = 0, 0
            bad.append(len(rows))
        rows.append((at, 8 + kl + vl, at + 8 + poff, plen))
        at += 8 + kl + vl
    return [list(r) for r in zip(*rows)], bad


@pytest.mark.parametrize("prefix", [4, 0])
def test_index_kernel_alone_good_and_bad_keys(prefix):
    """`build_index` over hand-built columns: the index rows of every record,
    and KEY_PREFIX for exactly the blocks that hold a key whose prefix
    contradicts its length, each between good blocks."""
    good, bads = INDEX_CASES[prefix]
    rnd = random.Random(prefix)
    blocks, bad_blocks = [], []
    for kind in [None] + sorted(bads):
        if kind is not None:                        # the bad key between good keys of its block
            bad_blocks.append(len(blocks))
            blocks.append([good[1], bads[kind], good[2]])
        blocks.append([rnd.choice(good) for _ in range((1, 3, 65)[len(blocks) % 3])])
        blocks.append([])                           # and a block without records
    vlens = [rnd.choice((0, 1, 17, 5000)) for blk in blocks for _ in blk]
    index, ksrc, vsrc, status, table, keys = _run_index(prefix, blocks, vlens)
    assert status == [seqz.KEY_PREFIX if b in bad_blocks else 0 for b in range(len(blocks))]
    want, bad = _want_index(prefix, keys, [len(k) for k in keys], vlens)
    assert len(bad) == len(bads) and index == want
    at = 0
    for b, blk in enumerate(blocks):                # sources: scans inside each block's columns
        ko, vo = int(table[4, b]), int(table[8, b])
        for k in blk:
            assert (ksrc[at], vsrc[at]) == (ko, vo)
            ko, vo, at = ko + len(k), vo + vlens[at], at + 1


@pytest.mark.parametrize("prefix", [4, 0])
def test_index_kernel_key_outside_columns_and_block_already_bad(prefix):
    good, _ = INDEX_CASES[prefix]
    blocks = [good[:3], good[1:4], good[:2]]
    vlens = [3] * 8
    # the last key reaches past the end of the columns buffer: its block alone
    index, _, _, status, _, keys = _run_index(prefix, blocks, vlens, stretch_last=1 << 20)
    assert status == [0, 0, seqz.KEY_PREFIX]
    klen = [len(k) for k in keys]
    klen[-1] += 1 << 20
    want, bad = _want_index(prefix, keys, klen, vlens)
    assert bad == [7] and index == want
    # a block the vint kernel gave a status: its lengths count as 0, the others' rows hold
    pre = torch.tensor([0, seqz.COUNT, 0], dtype=torch.int32, device="cuda")
    index, _, _, status, _, _ = _run_index(prefix, blocks, vlens, status=pre)
    assert status[0] == 0 and status[2] == 0 and status[1] & seqz.COUNT
    assert index[1] == [8 + len(k) + 3 for k in blocks[0]] + [8] * 3 + \
        [8 + len(k) + 3 for k in blocks[2]]
    assert index[0] == [sum(index[1][:i]) for i in range(8)]


# ----------------------------------------------------------------------------- assemble kernel
VALUE_LENGTHS = list(range(49)) + [255, 256, 257, 4095, 4096, 4097, 20000]


def _assemble_case(seed=1):
    rnd = random.Random(seed)
    recs = []
    for i in range(34 * 5):
        recs.append((rnd.randbytes(i % 34), rnd.randbytes(VALUE_LENGTHS[i % len(VALUE_LENGTHS)])))
    keys, vals, ksrc, vsrc = bytearray(), bytearray(), [], []
    for i, (k, v) in enumerate(recs):
        keys += rnd.randbytes((i * 7 + 3) % 16 + (16 - len(keys) % 16) % 16)   # misalignment i*7+3
        ksrc.append(len(keys))
        keys += k
        vals += rnd.randbytes((i * 5 + 1) % 16 + (16 - len(vals) % 16) % 16)
        vsrc.append(len(vals))
        vals += v
    assert {s % 16 for s in ksrc} == set(range(16)) == {s % 16 for s in vsrc}
    return recs, bytes(keys), bytes(vals), ksrc, vsrc


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _i64(xs):
    return torch.tensor(xs, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("with_values", [True, False])
def test_assemble_every_alignment_leaves_guards(with_values, shift):
    recs, keys, vals, ksrc, vsrc = _assemble_case()
    frames = [struct.pack(">ii", len(k) + len(v), len(k)) + k + v for k, v in recs]
    foff, at = [], 0
    for i, fr in enumerate(frames):                     # frame i at misalignment 11 i + shift
        at += (i * 11 - at) % 16
        foff.append(at)
        at += len(fr)
    foff, total = np.array(foff + [at]), at
    assert {int(o + shift) % 16 for o in foff[:-1]} == set(range(16))
    fill = bytes((i * 31 + 7) % 251 for i in range(64 + shift + total + 64))
    buf = _dev(fill)
    assert buf.data_ptr() % 16 == 0
    out = buf[64 + shift:64 + shift + total]            # the last frame ends on out's last byte
    klen, vlen = _i64([len(k) for k, _ in recs]), _i64([len(v) for _, v in recs])
    if with_values:
        seqz.assemble(out, _i64(foff[:-1].tolist()), klen, vlen, _dev(keys), _i64(ksrc),
                      _dev(vals), _i64(vsrc))
    else:
        seqz.assemble(out, _i64(foff[:-1].tolist()), klen, vlen, _dev(keys), _i64(ksrc))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    want = bytearray(fill)
    for o, fr, (k, v) in zip(foff[:-1].tolist(), frames, recs):
        a = 64 + shift + o
        n = len(fr) if with_values else 8 + len(k)
        want[a:a + n] = fr[:n]
    assert got[:64 + shift] == fill[:64 + shift] and got[-64:] == fill[-64:]
    assert got == bytes(want)


def test_assemble_leaves_out_records_outside_their_buffers():
    keys, vals = _dev(b"k" * 40), _dev(b"v" * 40)
    fill = torch.full((200,), 9, dtype=torch.uint8, device="cuda")
    out = fill[50:150]
    # frame past out, key past keys, value past vals, negative length, then a good one
    foff = _i64([90, 0, 0, 0, 40])
    klen = _i64([4, 30, 4, -1, 4])
    vlen = _i64([4, 4, 30, 4, 6])
    ksrc = _i64([0, 20, 0, 0, 1])
    vsrc = _i64([0, 0, 20, 0, 2])
    seqz.assemble(out, foff, klen, vlen, keys, ksrc, vals, vsrc)
    want = bytearray(b"\x09" * 200)
    want[90:108] = struct.pack(">ii", 10, 4) + b"kkkk" + b"vvvvvv"
    assert fill.cpu().numpy().tobytes() == bytes(want)


# ----------------------------------------------------------------------------- load_split
def _assert_equals_twin(path, start, length):
    want_data, want_index = seqz.load_split(path, start, length, "cpu")
    data, index = seqz.load_split(path, start, length, "cuda")
    assert data.device.type == "cuda" and index.device.type == "cuda"
    assert torch.equal(index.cpu(), want_index)
    assert torch.equal(data.cpu(), want_data)
    return int(index.shape[1])


@pytest.mark.parametrize("kcls", KEY_CLASSES)
@pytest.mark.parametrize("mode", MODES)
def test_load_split_equals_twin(tmp_path, mode, kcls):
    for n in (0, 1, 2, 63, 64, 65, 257):
        for block_size in ((1, 3000) if mode == "BLOCK" else (300,)):
            recs = make_records(n, seed=n, text=kcls is Text)
            path = write_file(tmp_path / f"{n}-{block_size}.seq", recs, kcls, mode, block_size,
                              raw_empty=True)
            size = os.path.getsize(path)
            assert _assert_equals_twin(path, 0, size) == n
            if n == 257:
                pl = seqz.plan(path, 0, size)
                if mode == "BLOCK":
                    assert pl["blocks"].shape[1] == (257 if block_size == 1 else
                                                     pytest.approx(60, abs=40))
                else:
                    assert (pl["recs"][6] == 0).any() and pl["chunks"].shape[1] > 257
                # windows that start in mid-file
                seen = 0
                for a, b in windows(path):
                    seen += _assert_equals_twin(path, a, b - a)
                assert seen == n


def _corrupt_chunk(path, pl, c):
    """Overwrite the body of chunk c with a copy element of offset 0."""
    at = pl["lo"] + int(pl["chunks"][0, c])
    u = int(pl["chunks"][3, c])
    pre = 1 if u < 128 else 2 if u < (1 << 14) else 3
    assert int(pl["chunks"][1, c]) >= pre + 2
    body = bytearray(open(path, "rb").read())
    body[at + pre:at + pre + 2] = b"\x01\x00"
    open(path, "wb").write(bytes(body))


@pytest.mark.parametrize("mode", MODES)
def test_corrupted_chunk_raises_ioerror(tmp_path, mode):
    path = write_file(tmp_path / "f.seq", make_records(65), BytesWritable, mode, 3000)
    size = os.path.getsize(path)
    pl = seqz.plan(path, 0, size)
    if mode == "RECORD":
        c = int(np.flatnonzero(pl["chunks"][3] > 100)[3])          # inside a value
    else:
        b = pl["blocks"].shape[1] // 2                               # a key-length column
        c = int(np.flatnonzero(pl["chunks"][2] == pl["blocks"][2, b])[0])
    _corrupt_chunk(path, pl, c)
    with pytest.raises(IOError, match=re.escape(path) + f".*chunk {c} of"):
        seqz.load_split(path, 0, size, "cuda")
    with pytest.raises(IOError, match=re.escape(path)):
        seqz.load_split(path, 0, size, "cpu")


def test_block_whose_lengths_contradict_its_columns_raises(tmp_path):
    """A length column that decodes, but to other lengths: the block's status."""
    from hbmr.io import sequencefile as seqf
    from hbmr.io.compress import SnappyCodec
    path = str(tmp_path / "f.seq")
    codec = SnappyCodec(buffer_size=1024)
    with seqf.Writer(path, BytesWritable, BytesWritable, compression="BLOCK", codec=codec,
                     block_size=1 << 20) as w:
        for k, v in make_records(30, max_value=200):
            w.append(BytesWritable(k), BytesWritable(v))
        w.sync_now()
        # a second block by hand: three records, value lengths that add up to one byte more
        w.out.write(struct.pack(">i", -1) + w.sync)
        w.out.write(encode_vint(3))
        ks = [BytesWritable(b"a").serialize(), BytesWritable(b"bc").serialize(),
              BytesWritable(b"").serialize()]
        for col in (b"".join(encode_vint(len(k)) for k in ks), b"".join(ks),
                    encode_vint(4) + encode_vint(5) + encode_vint(4), b"\0\0\0\0" * 3):
            c = codec.compress(col)
            w.out.write(encode_vint(len(c)) + c)
    size = os.path.getsize(path)
    assert seqz.plan(path, 0, size)["blocks"].shape[1] == 2
    with pytest.raises(IOError, match=re.escape(path) + ".*block 1 of 2"):
        seqz.load_split(path, 0, size, "cuda")


# ----------------------------------------------------------------------------- jobs
def _gpu_cluster():
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    return LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0)


def _cache(rj):
    cs = rj.getCounters()
    return (cs.get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_HITS"),
            cs.get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_MISSES"), cs.get(SNAPPY_GROUP, DECODED))


def test_gpu_sort_and_validate_jobs_equal_classic(tmp_path):
    from hbmr.examples import sort as sort_example
    inp = sort_input(tmp_path, n=600)
    nbytes = sum(8 + len(k) + len(v) for recs in parts(inp).values() for k, v in recs)
    sort_example.run(inp, str(tmp_path / "c-hash"), 3, conf=local_conf())
    classic = sort_example.make_job(inp, str(tmp_path / "c-total"), 3, (0.5, 1000, 10),
                                    local_conf())
    assert JobClient.runJob(classic).isSuccessful()
    want = sortvalidator.validate(inp, str(tmp_path / "c-hash"))
    assert want["ok"] and want["IN_RECORDS"] == 640
    with _gpu_cluster() as cl:
        # one split per file: the validator's splits
        first = cl.submit_job(sort_job.gpu_job(inp, str(tmp_path / "g-hash"), 3, maps=1))
        assert first.waitForCompletion(120) and first.isSuccessful(), first.getFailureInfo()
        assert first.getJobName() == "sorter-gpu"
        assert first.getCounters().get(JOB_GROUP, "GPU_MAP_TASKS") == 2
        assert _cache(first) == (0, 2, nbytes)
        second = cl.submit_job(sort_job.gpu_job(inp, str(tmp_path / "g-total"), 3,
                                                classic.get("total.order.partitioner.path"),
                                                maps=1))
        assert second.waitForCompletion(120) and second.isSuccessful(), second.getFailureInfo()
        assert _cache(second) == (2, 0, 0)
        # the validator finds the two input splits resident, and takes compressed parts
        compress_dir(str(tmp_path / "c-hash"), "BLOCK")
        got = sortvalidator.validate(inp, str(tmp_path / "c-hash"), cluster=cl, gpu=True)
        rj = last_job(cl)
        assert rj.getJobName() == validate_job.JOB_NAME
        assert _cache(rj) == (2, 3, nbytes)
    assert got == want
    assert_same_sort(tmp_path / "g-hash", tmp_path / "c-hash")
    assert_same_sort(tmp_path / "g-total", tmp_path / "c-total")


def test_gpu_join_job_equals_classic(tmp_path):
    dirs = join_inputs(tmp_path)
    with _gpu_cluster() as cl:
        for i, op in enumerate(("inner", "outer")):
            job = join_example.make_job(dirs, str(tmp_path / f"c-{op}"), op, 0, local_conf(),
                                        out_value=TupleWritable)
            assert JobClient.runJob(job).isSuccessful()
            rj = cl.submit_job(join_job.gpu_job(dirs, str(tmp_path / f"g-{op}"), op))
            assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
            assert rj.getJobName() == join_job.JOB_NAME
            assert rj.getCounters().get(JOB_GROUP, "GPU_MAP_TASKS") == 2
            hits, misses, decoded = _cache(rj)
            assert (hits, misses) == ((2, 0) if i else (0, 2))
            assert (decoded == 0) == bool(i)
            want, got = parts(tmp_path / f"c-{op}"), parts(tmp_path / f"g-{op}")
            assert list(want) == ["part-00000", "part-00001"] and got == want
