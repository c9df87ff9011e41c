"""GPU SecondarySort (split-level job, native/kernels/intpair.hip): the twin's
stages against the definition in plain Python (``str.split``, ``int``,
``abs(a * 127) % R``, ``str(a) + "\\t" + str(b) + "\\n"``), each kernel against
the twin, and the job's parts against the classic job's, byte for byte."""
import logging
import os
import random
import re

import numpy as np
import pytest
import torch

from hbmr.examples import secondarysort as example
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.models import secondarysort as ss_job
from hbmr.ops import intpair

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
TASK_GROUP = "org.apache.hadoop.mapred.Task$Counter"
COUNTERS = ["MAP_INPUT_RECORDS", "MAP_OUTPUT_RECORDS", "REDUCE_INPUT_GROUPS",
            "REDUCE_INPUT_RECORDS", "REDUCE_OUTPUT_RECORDS"]
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
SPACES = [9, 11, 12, 13, 28, 29, 30, 31, 32]          # str.split's ASCII set without '\n'
SEP = example.SEPARATOR.bytes + b"\n"


# ----------------------------------------------------------------------------- definition
def _nasty_pool():
    pool = []
    for w in SPACES:
        w = bytes([w])
        pool += [b"1" + w + b"2", w + b"3 4", b"5 6" + w, w + w + b"-7" + w + w + b"8" + w + w]
    pool += [b"9 10\r", b"\r", b"", b"   ", b"\t", b"42", b" 42 ", b"junk", b"1_0", b"\x00",
             b"1 2 3", b"4 5 x y", b"6 7 0x1 1_0", b"+5 -0", b"-0 +0", b"007 -007",
             b"0" * 37 + b"123 -" + b"0" * 39 + b"9", b"-2147483648 2147483647",
             b"2147483647 -2147483648", b"+2147483647 -1", b"12 12", b"12 12", b"-12 11"]
    return pool


def _nasty(nlines, newline_last=True, seed=0):
    pool = _nasty_pool()
    rnd = random.Random(seed)
    lines = [pool[i % len(pool)] for i in range(nlines)]
    rnd.shuffle(lines)
    raw = b"\n".join(lines) + (b"\n" if nlines and newline_last else b"")
    if nlines and not newline_last and not lines[-1]:
        raw += b"8 8"                                  # a last line without its newline
    return raw


def _lines(raw):
    lines = raw.split(b"\n")
    if lines and not lines[-1]:
        lines.pop()
    return lines


def _starts(raw):
    out, pos = [], 0
    for ln in _lines(raw):
        out.append(pos)
        pos += len(ln) + 1
    return out


_DEVICE_FORM = re.compile(r"[+-]?[0-9]+")


def _ref_parse(raw):
    """(status, key) per line by the definition."""
    out = []
    for ln in _lines(raw):
        toks = ln.decode("ascii").split()
        if len(toks) < 2:
            out.append((intpair.SKIP, 0))
            continue
        ok = all(_DEVICE_FORM.fullmatch(t) and INT_MIN <= int(t) <= INT_MAX for t in toks[:2])
        out.append((intpair.RECORD, intpair.pair_key(int(toks[0]), int(toks[1]))) if ok
                   else (intpair.IRREGULAR, 0))
    return out


def _ref_text(pairs):
    """A part's text from its (first, second) pairs in key order."""
    out, prev = [], None
    for a, b in pairs:
        if a != prev:
            out.append(SEP)
            prev = a
        out.append((str(a) + "\t" + str(b) + "\n").encode())
    return b"".join(out)


def _tensor(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
        torch.empty(0, dtype=torch.uint8)


def _keys(pairs):
    return torch.tensor([intpair.pair_key(a, b) for a, b in pairs], dtype=torch.int64)


def _pairs(keys):
    return list(zip(intpair.firsts(keys).tolist(), intpair.seconds(keys).tolist()))


NASTY_SIZES = [(0, True), (1, True), (1, False), (2, True), (63, True), (64, True), (65, True),
               (65, False), (64, False), (257, True), (600, False)]


def _digit_pairs():
    """Every digit count 1-10 of both signs for first and for second, sorted,
    with groups of one record and one group of 1,000."""
    vals = [0]
    for d in range(1, 11):
        lo, hi = 10 ** (d - 1), min(10 ** d - 1, INT_MAX)
        vals += [lo, hi, -lo, -hi]
    vals += [INT_MIN, INT_MAX]
    pairs = [(a, b) for a in vals for b in (0, a, -5, 77)] + [(3, b) for b in vals] + \
        [(250, b * 3 - 1500) for b in range(1000)]
    return sorted(set(pairs)) + [(INT_MAX, INT_MAX)] * 3          # duplicates stay records


# ----------------------------------------------------------------------------- CPU: the twin
@pytest.mark.parametrize("nlines,newline_last", NASTY_SIZES)
def test_twin_parse_equals_definition(nlines, newline_last):
    raw = _nasty(nlines, newline_last, seed=nlines)
    assert len(_lines(raw)) == nlines
    data = _tensor(raw)
    starts, non_ascii = intpair.line_starts(data)
    assert starts.tolist() == _starts(raw) and not non_ascii
    status, keys, _ = intpair.parse_lines(data, starts)
    want = _ref_parse(raw)
    assert list(zip(status.tolist(), keys.tolist())) == want
    parsed = intpair.parse(data)
    assert parsed.lines == nlines
    assert parsed.keys.tolist() == [k for s, k in want if s == intpair.RECORD]
    assert parsed.irregular == any(s == intpair.IRREGULAR for s, _ in want)
    if not parsed.irregular:
        assert intpair.parse_slow(raw).tolist() == parsed.keys.tolist()


def test_nasty_set_holds_what_it_should():
    raw = _nasty(600, False, seed=600)
    st = [s for s, _ in _ref_parse(raw)]
    assert st.count(intpair.RECORD) > 300 and st.count(intpair.SKIP) > 60
    assert not raw.endswith(b"\n") and b"\r\n" in raw
    pairs = set(_pairs(intpair.parse(_tensor(raw)).keys))
    assert {(INT_MIN, INT_MAX), (INT_MAX, INT_MIN), (5, 0), (0, 0), (7, -7), (123, -9),
            (-7, 8), (6, 7), (1, 2)} <= pairs


@pytest.mark.parametrize("line,flag", [
    (b"1_0 2", True), (b"2 1_0", True), (b"0x1 2", True), (b"+ 2", True), (b"2 -", True),
    (b"2147483648 1", True), (b"1 -2147483649", True), (b"1 2\xc3\xa9", True),
    (b"3 4 \x80", True), (b"\xff", True), (b"1 2\x003", True), (b"1 +-2", True),
    (b"1 2 x", False), (b"1 2 1_0 0x1", False), (b"junk", False), (b"1_0", False),
    (b"0x1 ", False), (b"2147483647 -2147483648", False), (b"99999999999", False)])
def test_irregular_flag(line, flag):
    for raw in (line, line + b"\n", b"1 2\n" * 300 + line + b"\n" + b"3 4\n" * 300):
        assert intpair.parse(_tensor(raw)).irregular is flag


def test_slow_path_is_the_classic_map():
    assert _pairs(intpair.parse_slow(b"1_0 2\n 3\x1f4 5\n6\n\n+7 -0_0\r\n")) == \
        [(10, 2), (3, 4), (7, 0)]
    for raw in (b"x y\n", b"1 2147483648\n", b"-2147483649 1\n", b"0x1 2\n"):
        with pytest.raises(ValueError):
            intpair.parse_slow(raw)


def _partition_firsts():
    return [INT_MIN, INT_MIN + 1, -16_909_321, -16_909_320, -1, 0, 1, 2, 126, 127, 16_909_320,
            16_909_321, 1 << 30, INT_MAX - 1, INT_MAX] + \
        random.Random(4).sample(range(INT_MIN, INT_MAX), 300)


@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 128])
def test_twin_partition_and_sort_equal_definition(nparts):
    rnd = random.Random(nparts)
    pairs = [(a, rnd.choice([INT_MIN, -1, 0, 5, INT_MAX])) for a in _partition_firsts()] * 2
    rnd.shuffle(pairs)
    keys = _keys(pairs)
    want = [abs(a * 127) % nparts for a, _ in pairs]
    assert any(abs(a * 127) >= 1 << 32 for a, _ in pairs)
    assert intpair.partition(keys, nparts).tolist() == want
    got, counts = intpair.sort_keys(keys, nparts)
    order = sorted(range(len(pairs)), key=lambda i: (want[i], pairs[i]))
    assert _pairs(got) == [pairs[i] for i in order]
    assert counts == [want.count(p) for p in range(nparts)]


def test_twin_heads_lengths_fill_equal_definition():
    pairs = _digit_pairs()
    keys = _keys(pairs)
    assert keys.numpy().view(np.uint64).tolist() == sorted(keys.numpy().view(np.uint64).tolist())
    want_heads = [i == 0 or pairs[i][0] != pairs[i - 1][0] for i in range(len(pairs))]
    assert intpair.heads(keys).tolist() == want_heads
    want_len = [len(f"{a}\t{b}\n") + (len(SEP) if h else 0) for (a, b), h in zip(pairs, want_heads)]
    lens = intpair.lengths(keys)
    assert lens.tolist() == want_len
    offs = intpair.offsets(lens)
    assert offs.tolist() == [sum(want_len[:i]) for i in range(len(pairs) + 1)]
    text, groups = intpair.format_part(keys)
    assert bytes(text.numpy()) == _ref_text(pairs)
    assert groups == sum(want_heads)
    for n in (0, 1, 2, 63, 64, 65):
        text, groups = intpair.format_part(keys[:n].contiguous())
        assert bytes(text.numpy()) == _ref_text(pairs[:n])
    with pytest.raises(ValueError, match="scan"):
        intpair.fill(keys, offs + 1, torch.zeros(int(offs[-1]) + 1, dtype=torch.uint8))


# ----------------------------------------------------------------------------- CPU: the job
def _job_lines(seed, n):
    rnd = random.Random(seed)
    firsts = [INT_MIN, INT_MAX, 0, -1, 1] + [rnd.randint(-10 ** e, 10 ** e) for e in range(1, 10)
                                             for _ in range(5)]
    assert len(firsts) == 50
    seconds = [INT_MIN, INT_MAX, 0] + [rnd.randint(INT_MIN, INT_MAX) for _ in range(400)]
    lines = []
    for i in range(n):
        a, b = rnd.choice(firsts), rnd.choice(seconds)
        if i % 97 == 0:
            lines.append(b"")                                       # skipped lines
        elif i % 89 == 0:
            lines.append(b"%d" % a)
        elif i % 83 == 0:
            lines.append(b" %s%d\t%011d more tokens " % (b"+" if a >= 0 else b"", a, b))
        else:
            lines.append(b"%d %d" % (a, b))
    return lines


@pytest.fixture(scope="module")
def job_input(tmp_path_factory):
    """Three files of about 7,000 lines and the classic job's output for R = 1, 3."""
    root = tmp_path_factory.mktemp("secondarysort")
    inp = root / "in"
    inp.mkdir()
    for f in range(3):
        lines = _job_lines(f, 7000 + 13 * f)
        (inp / f"file{f}.txt").write_bytes(b"\n".join(lines) + (b"\n" if f != 1 else b""))
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    classic = {}
    for R in (1, 3):
        out = str(root / f"classic-{R}")
        rj = JobClient.runJob(example.make_job(str(inp), out, R, local), verbose=False)
        classic[R] = (out, {c: rj.getCounters().get(TASK_GROUP, c) for c in COUNTERS})
    return str(inp), classic


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


def _assert_same_output(got_dir, want_dir):
    got, want = _parts(got_dir), _parts(want_dir)
    assert list(got) == list(want) and want
    for name in want:
        assert got[name] == want[name], name
    assert os.path.exists(os.path.join(got_dir, "_SUCCESS"))
    assert not os.path.exists(os.path.join(got_dir, "_temporary"))
    return want


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("trackers", [1, 2])
def test_secondarysort_gpu_flag_equals_classic(tmp_path, job_input, trackers, R):
    inp, classic = job_input
    out = str(tmp_path / "out")
    with LocalCluster(JobConf(), num_trackers=trackers, cpu_slots=2) as cl:
        rj = example.run(inp, out, R, cluster=cl, maps=5, gpu=True)
        assert rj.isSuccessful()
        cs = rj.getCounters()
    want = _assert_same_output(out, classic[R][0])
    assert list(want) == [f"part-{p:05d}" for p in range(R)]
    assert sum(len(v) for v in want.values()) > 100_000
    assert {c: cs.get(TASK_GROUP, c) for c in COUNTERS} == classic[R][1]
    assert cs.get(ss_job.SECONDARYSORT_GROUP, ss_job.SECONDARYSORT_CPU_FALLBACK_SPLITS) == 0
    assert cs.get(JOB_GROUP, "CPU_MAP_TASKS") >= 3


def test_empty_partition_gives_an_empty_part(tmp_path):
    inp = tmp_path / "in.txt"
    inp.write_bytes(b"3 1\n3 0\n6 5\n")                 # 3 * 127 and 6 * 127 are 0 mod 3
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    JobClient.runJob(example.make_job(str(inp), str(tmp_path / "c"), 3, local), verbose=False)
    with LocalCluster(JobConf(), num_trackers=2, cpu_slots=1) as cl:
        assert example.run(str(inp), str(tmp_path / "g"), 3, cluster=cl, gpu=True).isSuccessful()
    want = _assert_same_output(str(tmp_path / "g"), str(tmp_path / "c"))
    assert [len(v) for v in want.values()] == [len(SEP) * 2 + 12, 0, 0]


def test_irregular_split_takes_the_slow_path(tmp_path):
    inp = tmp_path / "in.txt"
    inp.write_bytes(b"5 6\n1_0 2\n5 -1\n10 1\n\n7\n")
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    JobClient.runJob(example.make_job(str(inp), str(tmp_path / "c"), 2, local), verbose=False)
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=1) as cl:
        rj = example.run(str(inp), str(tmp_path / "g"), 2, cluster=cl, gpu=True)
        assert rj.isSuccessful()
        cs = rj.getCounters()
        want = _assert_same_output(str(tmp_path / "g"), str(tmp_path / "c"))
        assert b"10\t1\n10\t2\n" in b"".join(want.values())
        assert cs.get(ss_job.SECONDARYSORT_GROUP, ss_job.SECONDARYSORT_CPU_FALLBACK_SPLITS) == 1
        assert cs.get(TASK_GROUP, "MAP_INPUT_RECORDS") == 6
        # a line the classic map fails on fails the job, as it fails the classic one
        bad = tmp_path / "bad.txt"
        bad.write_bytes(b"5 6\nx y\n")
        with pytest.raises(Exception):
            JobClient.runJob(example.make_job(str(bad), str(tmp_path / "cb"), 1, local),
                             verbose=False)
        with pytest.raises(RuntimeError, match="Job failed"):
            example.run(str(bad), str(tmp_path / "gb"), 1, cluster=cl, gpu=True)


def test_gpu_job_refuses_ineligible_jobs(tmp_path, caplog):
    plain = tmp_path / "plain.txt"
    plain.write_bytes(b"2 1\n1 2\n1 1\n")
    import gzip
    gz = tmp_path / "in.txt.gz"
    gz.write_bytes(gzip.compress(plain.read_bytes()))
    with pytest.raises(ValueError, match="compressed input"):
        ss_job.gpu_job(str(gz), str(tmp_path / "o1"))
    with pytest.raises(ValueError, match="not a local file"):
        ss_job.gpu_job("hdfs://namenode:8020/in.txt", str(tmp_path / "o2"))
    base = JobConf()
    base.set_boolean("mapred.output.compress", True)
    with pytest.raises(ValueError, match="compressed output"):
        ss_job.gpu_job(str(plain), str(tmp_path / "o3"), base=base)
    base = JobConf()
    base.set("mapred.textoutputformat.separator", ",")
    with pytest.raises(ValueError, match="separator"):
        ss_job.gpu_job(str(plain), str(tmp_path / "o4"), base=base)
    assert ss_job.gpu_job(str(plain), str(tmp_path / "o5"), 2).get_num_reduce_tasks() == 2
    # `secondarysort -gpu` on such a job is the classic job, and says why
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    local.set("mapred.textoutputformat.separator", ",")
    with caplog.at_level(logging.WARNING, logger="hbmr.examples.secondarysort"):
        assert example.run(str(plain), str(tmp_path / "g"), 1, conf=local, gpu=True).isSuccessful()
    assert "separator" in caplog.text and "classic secondarysort job" in caplog.text
    text = (tmp_path / "g" / "part-00000").read_bytes()
    assert text == SEP + b"1,1\n1,2\n" + SEP + b"2,1\n"
    local.set("mapred.textoutputformat.separator", "\t")
    assert example.run(str(gz), str(tmp_path / "z"), 1, conf=local, gpu=True).isSuccessful()
    assert (tmp_path / "z" / "part-00000").read_bytes() == text.replace(b",", b"\t")


def test_cli_takes_r_m_and_gpu(tmp_path):
    inp = tmp_path / "in.txt"
    inp.write_bytes(b"2 1\n1 2\n1 1\n-4 4\n")
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=1) as cl:
        assert example.main([str(inp), str(tmp_path / "c"), "-r", "2"], cluster=cl) == 0
        assert example.main([str(inp), str(tmp_path / "g"), "-r", "2", "-m", "2", "-gpu"],
                            cluster=cl) == 0
    _assert_same_output(str(tmp_path / "g"), str(tmp_path / "c"))


# ----------------------------------------------------------------------------- GPU
def _check_gpu_parse(raw, mis=0):
    """The parse kernels on ``raw`` held at misalignment ``mis`` against the twin."""
    data = _tensor(raw)
    pad = torch.full((len(raw) + 16,), 0x39, dtype=torch.uint8, device="cuda")   # '9' around it
    buf = pad[mis:mis + len(raw)]
    buf.copy_(data)
    assert len(raw) == 0 or buf.data_ptr() % 16 == mis
    starts, non_ascii = intpair.line_starts(buf)
    wstarts, wnon = intpair.line_starts(data)
    assert torch.equal(starts.cpu(), wstarts) and non_ascii == wnon
    status, keys, bc = intpair.parse_lines(buf, starts)
    wstatus, wkeys, _ = intpair.parse_lines(data, wstarts)
    assert torch.equal(status.cpu(), wstatus) and torch.equal(keys.cpu(), wkeys)
    got, want = intpair.parse(buf), intpair.parse(data)
    assert torch.equal(got.keys.cpu(), want.keys)
    assert (got.lines, got.irregular) == (want.lines, want.irregular)
    assert torch.equal(intpair.compact(status, keys, bc).cpu(), want.keys)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("nlines,newline_last", NASTY_SIZES)
def test_gpu_parse_equals_twin(nlines, newline_last):
    _check_gpu_parse(_nasty(nlines, newline_last, seed=nlines))


@pytest.mark.gpu
def test_gpu_parse_every_misalignment_and_tile_edges():
    raw = _nasty(600, False, seed=600)
    assert len(raw) > 4096                       # more than one newline tile
    for mis in range(16):
        _check_gpu_parse(raw[mis:], mis)
    # a newline on either side of a tile edge, and a line that ends on the buffer's last byte
    for n in (4095, 4096, 4097):
        body = b"1 2\n" * ((n - 1) // 4)
        raw = body + b"7" * (n - 1 - len(body)) + b"\n" + b"3 4"
        assert raw[n - 1:n] == b"\n"
        _check_gpu_parse(raw, 3)
    want = _check_gpu_parse(b"5 6\n7 8", 5)
    assert _pairs(want.keys) == [(5, 6), (7, 8)]
    for line, flag in ((b"1_0 2", True), (b"1 2 x", False), (b"junk", False), (b"1 2\xff", True),
                       (b"2147483648 1", True), (b"1 -2147483649", True)):
        assert _check_gpu_parse(b"1 2\n" * 300 + line + b"\n").irregular is flag


@pytest.mark.gpu
def test_gpu_parse_long_digit_lines_are_bounded():
    digits = b"1234567890" * 10_000
    # one token: skipped whatever it holds; as a second token: irregular, never a wrapped value
    one = _check_gpu_parse(digits, 1)
    assert (one.lines, one.irregular, one.keys.numel()) == (1, False, 0)
    two = _check_gpu_parse(b"1 " + digits, 7)
    assert (two.lines, two.irregular, two.keys.numel()) == (1, True, 0)
    three = _check_gpu_parse(b"3 4\n-" + b"0" * 100_000 + b"12 " + b"0" * 99_999 + b"7\n5 6", 2)
    assert _pairs(three.keys) == [(3, 4), (-12, 7), (5, 6)] and not three.irregular


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 128])
def test_gpu_partition_and_sort_equal_twin(nparts):
    rnd = random.Random(nparts)
    pairs = [(a, rnd.randint(INT_MIN, INT_MAX)) for a in _partition_firsts()] * 3
    rnd.shuffle(pairs)
    for n in (len(pairs), 0, 1, 2, 257):
        keys = _keys(pairs[:n])
        assert torch.equal(intpair.partition(keys.cuda(), nparts).cpu(),
                           intpair.partition(keys, nparts))
        got, counts = intpair.sort_keys(keys.cuda(), nparts)
        want, wcounts = intpair.sort_keys(keys, nparts)
        assert torch.equal(got.cpu(), want) and counts == wcounts


@pytest.mark.gpu
def test_gpu_format_equals_twin():
    pairs = _digit_pairs()
    keys = _keys(pairs)
    # heads on either side of a workgroup boundary: records 255, 256 and 257
    for cut in (254, 255, 256):
        shifted = [(-9, 0)] * cut + [(a, b) for a, b in pairs if a > -9]
        k = _keys(shifted)
        assert intpair.heads(k)[cut] and not intpair.heads(k)[cut - 1]
        text, groups = intpair.format_part(k.cuda())
        wtext, wgroups = intpair.format_part(k)
        assert torch.equal(text.cpu(), wtext) and groups == wgroups
    want, wgroups = intpair.format_part(keys)
    assert torch.equal(intpair.lengths(keys.cuda()).cpu(), intpair.lengths(keys))
    text, groups = intpair.format_part(keys.cuda())
    assert torch.equal(text.cpu(), want) and groups == wgroups
    for n in (0, 1, 2, 63, 64, 65):
        text, _ = intpair.format_part(keys[:n].contiguous().cuda())
        assert torch.equal(text.cpu(), intpair.format_part(keys[:n].contiguous())[0])


@pytest.mark.gpu
def test_gpu_fill_every_destination_misalignment_leaves_guards():
    keys = _keys(_digit_pairs())
    want, _ = intpair.format_part(keys)
    dkeys = keys.cuda()
    offs = intpair.offsets(intpair.lengths(dkeys))
    total = int(offs[-1])
    assert total == want.numel()
    for mis in range(16):
        pad = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = pad[16 + mis:16 + mis + total]
        assert out.data_ptr() % 16 == mis
        intpair.fill(dkeys, offs, out)
        got = pad.cpu()
        assert torch.equal(got[16 + mis:16 + mis + total], want)
        assert bool((got[:16 + mis] == 0xA5).all()) and bool((got[16 + mis + total:] == 0xA5).all())


@pytest.mark.gpu
def test_gpu_secondarysort_job_equals_classic(tmp_path, job_input):
    inp, classic = job_input
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    out = str(tmp_path / "out")
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        job = ss_job.gpu_job(inp, out, 3, maps=6)
        rj = cl.submit_job(job)
        assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
        cs = rj.getCounters()
        nsplits = len(ss_job.SecondarySortSplitJob().get_splits(job, []))
    _assert_same_output(out, classic[3][0])
    assert nsplits >= 3 and cs.get(JOB_GROUP, "GPU_MAP_TASKS") == nsplits
    assert cs.get(ss_job.SECONDARYSORT_GROUP, ss_job.SECONDARYSORT_CPU_FALLBACK_SPLITS) == 0
    assert {c: cs.get(TASK_GROUP, c) for c in COUNTERS} == classic[3][1]
