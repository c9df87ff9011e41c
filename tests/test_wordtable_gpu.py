"""The GPU word-count family (hbmr/models/wordtable.py, hbmr/ops/wordtab.py,
native/kernels/wordtab.hip): the twins against plain Python (``sorted``,
``b"%s\\t%d\\n"``, ``hash_bytes(prefix + word)``, ``ValueHistogram``), the four
``-gpu`` programs against their classic jobs byte for byte, and each kernel
against its twin."""
import gzip
import os
import random

import pytest
import torch

from hbmr.examples import aggregatewordcount as agg_example
from hbmr.examples import driver
from hbmr.examples import multifilewc as mf_example
from hbmr.io.writable import hash_bytes
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.mapred.lib.aggregate import ValueAggregatorJob, ValueHistogram
from hbmr.models import wordcount as wc_model
from hbmr.models import wordtable
from hbmr.ops import wordtab

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
TASK_GROUP = "org.apache.hadoop.mapred.Task$Counter"
PROGRAMS = ["wordcount", "multifilewc", "aggregatewordcount", "aggregatewordhist"]
SEEDS = [b"", b"LongValueSum:"]
NPARTS = [1, 2, 3, 7, 128]
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


# ----------------------------------------------------------------------------- tables
def _table(words, counts=None, src_mis=None, device="cpu"):
    """A word table of ``words``: back to back with one filler byte between
    them, or (``src_mis``) every word starting at that offset past a multiple of
    16 in a buffer whose first byte is 16-byte aligned."""
    raw, starts = bytearray(), []
    for w in words:
        if src_mis is not None:
            raw += b"#" * ((src_mis - len(raw)) % 16)
        starts.append(len(raw))
        raw += w + b"#"
    buf = torch.frombuffer(raw, dtype=torch.uint8) if raw else torch.empty(0, dtype=torch.uint8)
    t = (buf, torch.tensor(starts, dtype=torch.int32),
         torch.tensor([len(w) for w in words], dtype=torch.int32),
         torch.tensor(list(counts) if counts is not None else [1] * len(words), dtype=torch.int64))
    if device != "cpu":
        t = tuple(x.to(device) for x in t)
        assert src_mis is None or not words or t[0].data_ptr() % 16 == 0
    return t


def _lines(words, counts, order=None):
    ids = range(len(words)) if order is None else order
    return b"".join(b"%s\t%d\n" % (words[i], counts[i]) for i in ids)


def _hash_words(n, seed, lengths=range(1, 41)):
    """n distinct words over every byte but the white space of bytes.split(),
    with 0x80 and 0xff planted, their lengths cycling through ``lengths``."""
    rnd = random.Random(seed)
    alphabet = [b for b in range(256) if b not in (9, 10, 11, 12, 13, 32)]
    lengths = list(lengths)
    words, tries = set(), 0
    while len(words) < n:
        ln = lengths[tries % len(lengths)]               # (the short words run out: move on)
        tries += 1
        w = bytearray(rnd.choice(alphabet) for _ in range(ln))
        w[rnd.randrange(ln)] = rnd.choice([0x80, 0xFF, 0x7F, w[0]])
        words.add(bytes(w))
    return sorted(words, key=lambda w: rnd.random())


def _sort_words():
    """Prefixes of one another, words equal through bytes 7 and 14 (the sort's
    round boundaries), 0x7f / 0x80 / 0xff first bytes."""
    words = {b"a" * k for k in range(1, 24)}
    words |= {b"abcdefg" + t for t in (b"", b"\x00", b"h", b"\x80", b"\xff", b"hh", b"h\x00")}
    words |= {b"abcdefghijklmn" + t for t in (b"", b"\x00", b"o", b"\x7f", b"\x80", b"\xff", b"oo")}
    words |= {f + b"tail" for f in (b"\x7f", b"\x80", b"\xff", b"\x00", b"\x01")}
    words |= {b"\x7f", b"\x80", b"\xff", b"\xff\xff", b"\x80\x00"}
    return sorted(words, key=lambda w: hash_bytes(w))


def _seeded_parts(words, nparts, prefix):
    return [(hash_bytes(prefix + w) & 0x7FFFFFFF) % nparts for w in words]


# ----------------------------------------------------------------------------- CPU: the twins
def test_hash_seed_identity():
    assert hash_bytes(b"") == 1 and wordtab.seed_of(b"") == 1
    for p in (b"LongValueSum:", b"\xff\x80x"):
        for w in (b"", b"a", b"Stra\xc3\x9fe", b"\x80" * 40):
            want = ((hash_bytes(p) - 1) * 31 ** len(w) + hash_bytes(w)) & 0xFFFFFFFF
            assert hash_bytes(p + w) & 0xFFFFFFFF == want


@pytest.mark.parametrize("prefix", SEEDS)
@pytest.mark.parametrize("nparts", NPARTS)
def test_twin_partition_equals_definition(nparts, prefix):
    words = _hash_words(400, nparts)
    assert {len(w) for w in words} == set(range(1, 41))
    assert any(0x80 in w for w in words) and any(0xFF in w for w in words)
    buf, starts, lens, _ = _table(words)
    got = wordtab.partition(buf, starts, lens, nparts, wordtab.seed_of(prefix))
    assert got.dtype == torch.int32 and got.tolist() == _seeded_parts(words, nparts, prefix)


@pytest.mark.parametrize("nparts", [1, 3])
def test_twin_sort_table_equals_sorted(nparts):
    words = _sort_words() + _hash_words(300, 5)
    buf, starts, lens, _ = _table(words)
    parts = wordtab.partition(buf, starts, lens, nparts)
    order, nrec = wordtab.sort_table(buf, starts, lens, parts, nparts)
    want = sorted(range(len(words)), key=lambda i: (parts[i].item(), words[i]))
    assert order.dtype == torch.int32 and order.tolist() == want
    assert nrec == [parts.tolist().count(p) for p in range(nparts)]


def _digit_counts():
    cs = [0, -1, INT64_MIN, INT64_MAX]
    for d in range(1, 20):
        lo, hi = 10 ** (d - 1), min(10 ** d - 1, INT64_MAX)
        cs += [lo, hi, -lo, -hi]
    return cs


def test_twin_lengths_and_format_equal_definition():
    counts = _digit_counts()
    words = _hash_words(len(counts), 9)
    buf, starts, lens, cnt = _table(words, counts)
    order = list(range(len(words)))
    random.Random(3).shuffle(order)
    ot = torch.tensor(order, dtype=torch.int32)
    assert wordtab.line_lengths(lens, cnt, ot).tolist() == \
        [len(b"%s\t%d\n" % (words[i], counts[i])) for i in order]
    assert bytes(wordtab.format_part(buf, starts, lens, cnt, ot).numpy()) == \
        _lines(words, counts, order)
    assert bytes(wordtab.format_part(buf, starts, lens, cnt).numpy()) == _lines(words, counts)
    ll = wordtab.line_lengths(lens, cnt)
    with pytest.raises(ValueError, match="scan"):
        wordtab.fill_lines(buf, starts, lens, cnt, None, wordtab.offsets(ll) + 1,
                           torch.zeros(int(ll.sum()) + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="outside the buffer"):
        wordtab.format_part(buf, starts + 10 ** 6, lens, cnt)
    with pytest.raises(ValueError, match="outside the table"):
        wordtab.format_part(buf, starts, lens, cnt, torch.tensor([len(words)], dtype=torch.int32))


def _five_decades(n):
    rnd = random.Random(50)
    return [int(10 ** (5 * rnd.random())) for _ in range(n)]


HISTOGRAM_CASES = {"one": [7], "even": [3, 1, 4, 1, 5, 9], "odd": [2, 7, 1, 8, 2, 8, 1],
                   "equal": [12] * 9, "decades": _five_decades(50_000)}


@pytest.fixture(scope="module")
def histogram_reports():
    """ValueHistogram's own report of each case, computed once."""
    out = {}
    for name, cs in HISTOGRAM_CASES.items():
        h = ValueHistogram()
        for i, c in enumerate(cs):
            h.addNextValue(f"w{i}\t{c}")
        out[name] = h.getReport()
    return out


@pytest.mark.parametrize("case", list(HISTOGRAM_CASES))
def test_histogram_report_equals_value_histogram(case, histogram_reports):
    cs = HISTOGRAM_CASES[case]
    values, mult = wordtab.count_runs(wordtab.sort_counts(torch.tensor(cs, dtype=torch.int64)))
    assert values.tolist() == sorted(set(cs)) and mult.tolist() == [cs.count(v) for v in
                                                                     values.tolist()]
    assert wordtab.histogram_report(values, mult) == histogram_reports[case]
    # runs merged from several ranks come unsorted and with repeated values
    half = len(cs) // 2
    runs = [wordtab.count_runs(wordtab.sort_counts(torch.tensor(part, dtype=torch.int64)))
            for part in (cs[half:], cs[:half])]
    assert wordtab.histogram_report(torch.cat([r[0] for r in runs]),
                                    torch.cat([r[1] for r in runs])) == histogram_reports[case]
    if case == "decades":
        assert len(cs) >= 50_000 and max(cs) >= 10_000 * max(1, min(cs))
    assert wordtab.histogram_report(torch.empty(0, dtype=torch.int64),
                                    torch.empty(0, dtype=torch.int64)) == "0"


def test_flag_nonclassic():
    for raw, flag in ((b"", False), (b"plain ascii\t\x0b\x0c\r\n\x00\x1b\x20\x7f", False),
                      (b"a\x1cb", True), (b"a\x1fb", True), (b"a\x80", True), (b"\xff", True),
                      (b"Stra\xc3\x9fe", True)):
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
            torch.empty(0, dtype=torch.uint8)
        assert wordtab.flag_nonclassic(t) is flag
    assert "a\x1cb".split() == ["a", "b"] and b"a\x1cb".split() == [b"a\x1cb"]


# ----------------------------------------------------------------------------- CPU: the jobs
def _local():
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    return conf


def _classic(program, inp, out, reduces):
    """The classic job of ``program`` on the LocalJobRunner."""
    if program == "wordcount":
        job = wc_model.make_job(inp, out, reduces, _local())
    elif program == "multifilewc":
        job = mf_example.make_job(inp, out, 2, _local(), reduces)
    else:
        plug = agg_example.WordHistogramPlugIn if program == "aggregatewordhist" else \
            agg_example.WordCountPlugIn
        job = ValueAggregatorJob.createValueAggregatorJob(inp, out, [plug], reduces, _local())
    assert JobClient.runJob(job, verbose=False).isSuccessful()
    return out


def _args(program, inp, out, reduces, maps=None):
    if program in ("wordcount", "multifilewc"):
        return [inp, out, "-r", str(reduces)] + (["-m", str(maps)] if maps else [])
    return [inp, out, str(reduces)]


def _run_gpu(cl, program, inp, out, reduces, maps=None):
    """``driver.run(program, [..., "-gpu"])`` on ``cl``; returns the counters of
    the job it submitted, which must be the split-level job."""
    seen = []
    submit = cl.submit_job

    def spy(job):
        rj = submit(job)
        seen.append((job, rj))
        return rj
    cl.submit_job = spy
    try:
        assert driver.run(program, _args(program, inp, out, reduces, maps) + ["-gpu"],
                          cluster=cl) == 0
    finally:
        cl.submit_job = submit
    assert len(seen) == 1
    job, rj = seen[0]
    assert job.get("hbmr.splitjob.class") == "hbmr.models.wordtable:WordTableSplitJob"
    assert job.get(wordtable.PROGRAM_KEY) == program
    return job, rj.getCounters()


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


def _assert_same_output(got_dir, want_dir, reduces):
    got, want = _parts(got_dir), _parts(want_dir)
    assert list(want) == [f"part-{p:05d}" for p in range(reduces)]
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert os.path.exists(os.path.join(got_dir, "_SUCCESS"))
    assert not os.path.exists(os.path.join(got_dir, "_temporary"))
    return want


def _ascii_lines(seed, n):
    rnd = random.Random(seed)
    vocab = [b"w%d" % i for i in range(150)] + [b"The", b"the", b"a:b", b"x" * 70, b"0", b"-1",
                                                b"LongValueSum:", b"\x00nul", b"~\x7f"]
    seps = [b" ", b"  ", b"\t", b"\x0b", b"\x0c", b" \t "]
    lines = []
    for i in range(n):
        toks = [rnd.choice(vocab) for _ in range(rnd.randrange(0, 9))]
        line = b"".join(t + rnd.choice(seps) for t in toks)
        lines.append(line + (b"\r" if i % 7 == 0 else b""))
    return lines


def _write_ascii(root, nlines):
    inp = root / "in"
    inp.mkdir()
    for f in range(3):
        lines = _ascii_lines(f, nlines + 13 * f)
        # the second file ends without a newline
        (inp / f"file{f}.txt").write_bytes(b"\n".join(lines) + (b"\n" if f != 1 else b" end"))
    raw = b"".join(p.read_bytes() for p in inp.iterdir())
    assert max(raw) < 0x80 and not any(0x1C <= b <= 0x1F for b in raw)
    assert b"x" * 70 in raw and b"\x0b" in raw and b"\r\n" in raw and b"\t" in raw
    return str(inp)


@pytest.fixture(scope="module")
def ascii_corpus(tmp_path_factory):
    """Three pure-ASCII files and each program's classic output for R = 1, 3."""
    root = tmp_path_factory.mktemp("wordtable")
    inp = _write_ascii(root, 120)
    return inp, {(p, R): _classic(p, inp, str(root / f"classic-{p}-{R}"), R)
                 for p in PROGRAMS for R in (1, 3)}


def test_driver_starts_wordcount(tmp_path, ascii_corpus):
    inp, classic = ascii_corpus
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        assert driver.run("wordcount", [inp, str(tmp_path / "out")], cluster=cl) == 0
    _assert_same_output(str(tmp_path / "out"), classic["wordcount", 1], 1)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("trackers", [1, 2])
@pytest.mark.parametrize("program", PROGRAMS)
def test_gpu_flag_equals_classic(tmp_path, ascii_corpus, program, trackers, R):
    inp, classic = ascii_corpus
    out = str(tmp_path / "out")
    with LocalCluster(JobConf(), num_trackers=trackers, cpu_slots=2) as cl:
        _, cs = _run_gpu(cl, program, inp, out, R)
    want = _assert_same_output(out, classic[program, R], R)
    assert sum(len(v) for v in want.values()) > (1000 if "hist" not in program else 20)
    if program == "aggregatewordhist":
        assert [bool(v) for v in want.values()].count(True) == 1
    # a condition, not a report: the test must not pass by falling back
    assert cs.get(wordtable.WORDTABLE_GROUP, wordtable.WORDTABLE_CPU_FALLBACK_SPLITS) == 0
    assert cs.get(JOB_GROUP, "CPU_MAP_TASKS") >= 2
    assert cs.get(TASK_GROUP, "REDUCE_INPUT_GROUPS") > 150
    assert cs.get(TASK_GROUP, "MAP_INPUT_BYTES") >= sum(
        os.path.getsize(os.path.join(inp, f)) for f in os.listdir(inp))


def _write_planted(root):
    """Four files of one size; file2 holds ``Straße``, file3 a lone 0xa0, a
    no-break space and 0x1c; file0 and file1 are ASCII."""
    inp = root / "planted"
    inp.mkdir()
    bodies = [b"\n".join(_ascii_lines(10 + f, 40)) for f in range(4)]
    bodies[2] += b"\nStra\xc3\x9fe und Stra\xc3\x9fe the"
    bodies[3] += b"\na\xa0b x\xc2\xa0y p\x1cq p q the"
    size = max(len(b) for b in bodies) + 1
    for f, b in enumerate(bodies):
        (inp / f"file{f}.txt").write_bytes(b + b" " * (size - 1 - len(b)) + b"\n")
    return str(inp)


@pytest.fixture(scope="module")
def planted_corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("wordtable-planted")
    inp = _write_planted(root)
    return inp, {p: _classic(p, inp, str(root / f"classic-{p}"), 2) for p in PROGRAMS}


def _check_planted(cl, tmp_path, planted_corpus, program):
    inp, classic = planted_corpus
    out = str(tmp_path / f"out-{program}")
    job, cs = _run_gpu(cl, program, inp, out, 2, maps=2 if program == "multifilewc" else None)
    want = _assert_same_output(out, classic[program], 2)
    text = b"".join(want.values())
    nsplits = len(wordtable.WordTableSplitJob().get_splits(job, []))
    # text splits: one per file, two of them planted; multifilewc: two files per
    # map, the planted files in the second
    flagged = {"wordcount": 0, "multifilewc": 1}.get(program, 2)
    assert nsplits == (2 if program == "multifilewc" else 4)
    assert cs.get(wordtable.WORDTABLE_GROUP, wordtable.WORDTABLE_CPU_FALLBACK_SPLITS) == flagged
    return text


@pytest.mark.parametrize("program", PROGRAMS)
def test_planted_bytes_take_the_classic_tokeniser(tmp_path, planted_corpus, program):
    with LocalCluster(JobConf(), num_trackers=2, cpu_slots=1) as cl:
        text = _check_planted(cl, tmp_path, planted_corpus, program)
    kv = dict(line.rsplit(b"\t", 1) for line in text.split(b"\n") if line)
    if program == "wordcount":
        assert kv[b"a\xa0b"] == kv[b"x\xc2\xa0y"] == kv[b"p\x1cq"] == b"1" and kv[b"p"] == b"1"
    elif program != "aggregatewordhist":
        assert kv[b"Stra\xc3\x9fe"] == b"2" and kv[b"a\xef\xbf\xbdb"] == b"1"
        assert kv[b"x"] == kv[b"y"] == b"1" and kv[b"p"] == kv[b"q"] == b"2"


def test_multifilewc_edge_cases(tmp_path):
    inp = tmp_path / "in"
    inp.mkdir()
    (inp / "a.txt").write_bytes(b"one two\nthree foo")          # no final newline
    (inp / "b.txt").write_bytes(b"bar one\n")                   # "foo" + "bar" must not join
    (inp / "c.txt").write_bytes(b"")
    (inp / "d.txt").write_bytes(b"\n\n  \n")
    (inp / "e.txt").write_bytes(b"two")
    want_dir = _classic("multifilewc", str(inp), str(tmp_path / "classic"), 2)
    with LocalCluster(JobConf(), num_trackers=2, cpu_slots=1) as cl:
        for maps in (1, 2, 9):                                  # 9: more maps than files
            out = str(tmp_path / f"out-{maps}")
            job, cs = _run_gpu(cl, "multifilewc", str(inp), out, 2, maps=maps)
            want = _assert_same_output(out, want_dir, 2)
            assert cs.get(wordtable.WORDTABLE_GROUP, wordtable.WORDTABLE_CPU_FALLBACK_SPLITS) == 0
            assert len(wordtable.WordTableSplitJob().get_splits(job, [])) <= 5
    text = b"".join(want.values())
    assert b"foo\t1\n" in text and b"bar\t1\n" in text and b"foobar" not in text
    assert b"one\t2\n" in text and b"two\t2\n" in text
    assert wordtable.read_files([str(inp / f) for f in ("a.txt", "c.txt", "b.txt", "e.txt")]) == \
        b"one two\nthree foo\nbar one\ntwo\n"


def test_gpu_job_refuses_ineligible_jobs(tmp_path, caplog):
    import logging
    plain = tmp_path / "plain.txt"
    plain.write_bytes(b"b a\na c\n")
    gz = tmp_path / "in.txt.gz"
    gz.write_bytes(gzip.compress(plain.read_bytes()))
    for program in PROGRAMS:
        with pytest.raises(ValueError, match="compressed input"):
            wordtable.gpu_job(program, str(gz), str(tmp_path / "o1"))
        with pytest.raises(ValueError, match="0 reduces"):
            wordtable.gpu_job(program, str(plain), str(tmp_path / "o2"), 0)
    base = JobConf()
    base.set_boolean("mapred.output.compress", True)
    with pytest.raises(ValueError, match="compressed output"):
        wordtable.wordcount_job(str(plain), str(tmp_path / "o3"), base=base)
    assert wordtable.aggregatewordhist_job(str(plain), str(tmp_path / "o4"),
                                           3).get_num_reduce_tasks() == 3
    # `wordcount -gpu` on such an input is the classic job, and says why
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=1) as cl:
        with caplog.at_level(logging.WARNING, logger="hbmr.models.wordcount"):
            assert driver.run("wordcount", [str(gz), str(tmp_path / "g"), "-gpu"], cluster=cl) == 0
    assert "compressed input" in caplog.text and "classic wordcount job" in caplog.text
    assert (tmp_path / "g" / "part-00000").read_bytes() == b"a\t2\nb\t1\nc\t1\n"


# ----------------------------------------------------------------------------- GPU: the kernels
def _misaligned(t, mis, fill=0x23):
    """``t`` on the GPU at ``mis`` bytes past a multiple of 16."""
    pad = torch.full((t.numel() + 32,), fill, dtype=torch.uint8, device="cuda")
    view = pad[mis:mis + t.numel()]
    view.copy_(t)
    assert t.numel() == 0 or view.data_ptr() % 16 == mis
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", SEEDS)
def test_gpu_partition_equals_twin(prefix):
    seed = wordtab.seed_of(prefix)
    words = _hash_words(257, 7, list(range(1, 34)) + [300])
    assert any(len(w) == 300 for w in words) and any(w[0] >= 0x80 for w in words)
    for n in (0, 1, 2, 63, 64, 65, 257):
        buf, starts, lens, _ = _table(words[:n])
        for nparts in NPARTS:
            want = wordtab.partition(buf, starts, lens, nparts, seed)
            got = wordtab.partition(buf.cuda(), starts.cuda(), lens.cuda(), nparts, seed)
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    # word starts at every misalignment: the same table in a shifted buffer
    buf, starts, lens, _ = _table(words[:65])
    want = wordtab.partition(buf, starts, lens, 7, seed)
    assert want.tolist() == _seeded_parts(words[:65], 7, prefix)
    for mis in range(16):
        got = wordtab.partition(_misaligned(buf, mis), starts.cuda(), lens.cuda(), 7, seed)
        assert torch.equal(got.cpu(), want)


@pytest.mark.gpu
def test_gpu_line_lengths_equal_twin():
    counts = _digit_counts()
    assert {len(str(abs(c))) for c in counts} == set(range(1, 20))
    words = _hash_words(len(counts), 9)
    _, _, lens, cnt = _table(words, counts)
    order = list(range(len(words)))
    random.Random(3).shuffle(order)
    ot = torch.tensor(order[:-5], dtype=torch.int32)             # not the identity, not all
    for o in (None, ot):
        want = wordtab.line_lengths(lens, cnt, o)
        got = wordtab.line_lengths(lens.cuda(), cnt.cuda(), None if o is None else o.cuda())
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert wordtab.line_lengths(lens, cnt, ot).tolist() == \
        [len(words[i]) + 2 + len(str(counts[i])) for i in order[:-5]]


def _check_gpu_fill(table, words, counts, order=None, dst_mis=0):
    """The fill kernel into a destination at ``dst_mis`` with 64 guard bytes on
    either side, against the lines in plain Python."""
    buf, starts, lens, cnt = table
    want = _lines(words, counts, order)
    ot = None if order is None else torch.tensor(order, dtype=torch.int32, device="cuda")
    offs = wordtab.offsets(wordtab.line_lengths(lens, cnt, ot))
    total = int(offs[-1]) if offs.numel() else 0
    assert total == len(want)
    pad = torch.full((64 + 16 + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    a = 64 + dst_mis
    out = pad[a:a + total]                       # the last line ends on the buffer's last byte
    assert total == 0 or out.data_ptr() % 16 == dst_mis
    wordtab.fill_lines(buf, starts, lens, cnt, ot, offs, out)
    got = pad.cpu()
    assert bytes(got[a:a + total].numpy()) == want
    assert bool((got[:a] == 0xA5).all()) and bool((got[a + total:] == 0xA5).all())


@pytest.mark.gpu
def test_gpu_fill_every_misalignment_leaves_guards():
    lengths = list(range(1, 34)) + [255, 256, 257, 4095, 4096, 4097, 20_000]
    rnd = random.Random(11)
    words = [bytes(rnd.randrange(33, 256) for _ in range(n)) for n in lengths]
    counts = [rnd.choice([0, 7, -3, 10 ** rnd.randrange(19), INT64_MIN]) for _ in words]
    order = list(range(len(words)))
    rnd.shuffle(order)
    for src_mis in range(16):
        table = _table(words, counts, src_mis=src_mis, device="cuda")
        assert all(s % 16 == src_mis for s in table[1].tolist())
        for dst_mis in range(16):
            _check_gpu_fill(table, words, counts, order, dst_mis)


@pytest.mark.gpu
def test_gpu_fill_small_and_many():
    rnd = random.Random(12)
    words = _hash_words(257, 13, range(1, 12))
    counts = [rnd.randrange(1, 10 ** rnd.randrange(1, 8)) for _ in words]
    for n in list(range(66)) + [257]:
        _check_gpu_fill(_table(words[:n], counts[:n], device="cuda"), words[:n], counts[:n],
                        dst_mis=n % 16)
    # many workgroups: 100,000 words of two to nine bytes
    many = [b"%x" % (i * 2654435761 % (1 << 4 * rnd.randrange(2, 10))) for i in range(100_000)]
    many = [w.rjust(2, b"g") for w in many]
    assert {len(w) for w in many} == set(range(2, 10))
    mcounts = [rnd.randrange(1, 5000) for _ in many]
    _check_gpu_fill(_table(many, mcounts, device="cuda"), many, mcounts, dst_mis=5)
    assert len(_lines(many, mcounts)) > 100 * wordtab._lib.load().hbmr_wordtab_tile_bytes()
    # a '\n', a '\t' and a digit on either side of a tile edge (destination aligned:
    # the edge is byte 4096 of the text); line 1 is "bbbb\t123\n" behind a long word
    tile = wordtab._lib.load().hbmr_wordtab_tile_bytes()
    for edge in (tile - 1, tile):
        for back in (7, 9, 11):                  # line 1's tab, its digit '2', its newline
            ws = [b"L" * (edge - back), b"bbbb", b"tail"]
            cs = [7, 123, 45]
            text = _lines(ws, cs)
            assert text[edge:edge + 1] == {7: b"\t", 9: b"2", 11: b"\n"}[back]
            _check_gpu_fill(_table(ws, cs, device="cuda"), ws, cs, dst_mis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("nparts,prefix", [(1, b""), (3, b""), (3, b"LongValueSum:")])
def test_gpu_sort_table_equals_sorted(nparts, prefix):
    seed = wordtab.seed_of(prefix)
    special = _sort_words()
    assert len(special) > 40
    big = special + [w for w in _hash_words(50_000, 21, range(1, 30)) if w not in set(special)]
    assert len(big) >= 50_000 and len(set(big)) == len(big)
    for words in [special[:n] for n in range(66)] + [big]:
        buf, starts, lens, _ = _table(words, device="cuda")
        parts = wordtab.partition(buf, starts, lens, nparts, seed)
        assert parts.tolist() == _seeded_parts(words, nparts, prefix)
        order, nrec = wordtab.sort_table(buf, starts, lens, parts, nparts)
        hb, hs, hl, _ = _table(words)
        worder, wnrec = wordtab.sort_table(hb, hs, hl, parts.cpu(), nparts)
        assert torch.equal(order.cpu(), worder) and nrec == wnrec
        if len(words) <= 65:
            p = parts.tolist()
            assert order.tolist() == sorted(range(len(words)), key=lambda i: (p[i], words[i]))


@pytest.mark.gpu
def test_gpu_count_runs_equals_twin():
    rnd = random.Random(14)
    cases = [[], [5], [9] * 257, list(range(1, 258)), [rnd.choice([1, 1, 2, 3, 10 ** 12])
                                                       for _ in range(257)]]
    for cs in cases:
        rnd.shuffle(cs)
        host = torch.tensor(cs, dtype=torch.int64)
        want = wordtab.count_runs(wordtab.sort_counts(host))
        got = wordtab.count_runs(wordtab.sort_counts(host.cuda()))
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
        assert got[0].dtype == got[1].dtype == torch.int64
        assert want[0].tolist() == sorted(set(cs)) and int(want[1].sum()) == len(cs)


# ----------------------------------------------------------------------------- GPU: the jobs
@pytest.fixture(scope="module")
def gpu_corpus(tmp_path_factory):
    """Three pure-ASCII files of about 1,500 lines and each program's classic
    output for R = 3."""
    root = tmp_path_factory.mktemp("wordtable-gpu")
    inp = _write_ascii(root, 1500)
    return inp, {p: _classic(p, inp, str(root / f"classic-{p}"), 3) for p in PROGRAMS}


def _gpu_cluster():
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    return LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0)


@pytest.mark.gpu
@pytest.mark.parametrize("program", PROGRAMS)
def test_gpu_jobs_equal_classic(tmp_path, gpu_corpus, program):
    inp, classic = gpu_corpus
    out = str(tmp_path / "out")
    with _gpu_cluster() as cl:
        job, cs = _run_gpu(cl, program, inp, out, 3, maps=4 if program == "multifilewc" else None)
        nsplits = len(wordtable.WordTableSplitJob().get_splits(job, []))
    _assert_same_output(out, classic[program], 3)
    # (MultiFileInputFormat closes a map once it holds a third of the bytes: two maps here)
    assert nsplits >= (2 if program == "multifilewc" else 3)
    assert cs.get(JOB_GROUP, "GPU_MAP_TASKS") >= nsplits
    assert cs.get(wordtable.WORDTABLE_GROUP, wordtable.WORDTABLE_CPU_FALLBACK_SPLITS) == 0


@pytest.mark.gpu
def test_gpu_flagged_split_falls_back(tmp_path, planted_corpus):
    with _gpu_cluster() as cl:
        text = _check_planted(cl, tmp_path, planted_corpus, "aggregatewordcount")
    kv = dict(line.rsplit(b"\t", 1) for line in text.split(b"\n") if line)
    assert kv[b"Stra\xc3\x9fe"] == b"2" and kv[b"p"] == b"2" and kv[b"a\xef\xbf\xbdb"] == b"1"
