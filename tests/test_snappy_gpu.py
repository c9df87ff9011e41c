"""Snappy-compressed text input of the split-level text jobs: the chunk table
(native/io/snappyindex.cc), the decode kernel (native/kernels/snappydec.hip)
through hbmr/ops/snappydec.py, and the jobs over ``.snappy`` files.

Streams are built by the element-list encoder below, so every element form is
reached whatever the project's compressor emits.  Expected bytes come from the
host decoder (hbmr.io.snappy) or from the known plain text, never from the code
under test."""
import gzip
import os
import random

import numpy as np
import pytest
import torch

from hbmr.examples import driver
from hbmr.examples import grep as grep_example
from hbmr.examples import secondarysort as ss_example
from hbmr.io import snappy
from hbmr.io.compress import SnappyCodec
from hbmr.mapred import JobClient, JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.models import grep as grep_job
from hbmr.models import secondarysort as ss_job
from hbmr.models import wordcount as wc_model
from hbmr.models import wordtable
from hbmr.ops import snappydec

JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
GROUP, DECODED = "hbmr.CompressedInputCounters", "SNAPPY_DECODED_BYTES"
GUARD = 64


# ----------------------------------------------------------------------------- the encoder
def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _encode(elements, ulen=None):
    """A raw Snappy stream of ``("lit", bytes[, length field bytes])``,
    ``("copy", offset, length, offset bytes)`` and ``("raw", bytes)`` (written
    as they are) elements.  The preamble is ``ulen``, by default what the
    elements produce.  Nothing is checked: a malformed stream is built the
    same way."""
    body, produced = bytearray(), 0
    for e in elements:
        if e[0] == "lit":
            data = e[1]
            n = len(data) - 1
            nb = e[2] if len(e) > 2 else (0 if n < 60 else 1 if n < 1 << 8 else
                                          2 if n < 1 << 16 else 3 if n < 1 << 24 else 4)
            if nb == 0:
                assert n < 60
                body.append(n << 2)
            else:
                assert n < 1 << (8 * nb)
                body.append((59 + nb) << 2)
                body += n.to_bytes(nb, "little")
            body += data
            produced += len(data)
        elif e[0] == "copy":
            _, off, ln, ob = e
            if ob == 1:
                assert 4 <= ln <= 11 and off < 2048
                body.append(1 | ((ln - 4) << 2) | ((off >> 8) << 5))
                body.append(off & 0xFF)
            else:
                assert 1 <= ln <= 64 and ob in (2, 4) and off < 1 << (8 * ob)
                body.append((2 if ob == 2 else 3) | ((ln - 1) << 2))
                body += off.to_bytes(ob, "little")
            produced += ln
        else:
            body += e[1]
    return _varint(produced if ulen is None else ulen) + bytes(body)


def _frame(streams, plain_len):
    """One Hadoop block holding ``streams`` as its chunks."""
    return plain_len.to_bytes(4, "big") + b"".join(len(s).to_bytes(4, "big") + s for s in streams)


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


def _zipf_text(nbytes, seed=7, vocab=5000):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    words = [bytes(letters[rng.integers(0, 26, rng.integers(2, 12))]) + b"%d" % i
             for i in range(vocab)]
    lines, size = [], 0
    while size < nbytes:
        ids = np.minimum(rng.zipf(1.3, rng.integers(1, 12)) - 1, vocab - 1)
        lines.append(b" ".join(words[i] for i in ids))
        size += len(lines[-1]) + 1
    return (b"\n".join(lines) + b"\n")[:nbytes]


def _pair_text(nbytes, seed=3):
    rnd = random.Random(seed)
    out, size = [], 0
    while size < nbytes:
        out.append(b"%d %d\n" % (rnd.randrange(-50, 50), rnd.randrange(-10 ** 6, 10 ** 6)))
        size += len(out[-1])
    return b"".join(out)[:nbytes]


# ----------------------------------------------------------------------------- CPU: the table
def _framed_cases():
    one = snappy.hadoop_compress(b"hello hello hello hello\n")
    cases = {"empty": (b"", b""), "lone-header": (snappy.hadoop_compress(b""), b""),
             "one-chunk": (one, b"hello hello hello hello\n")}
    max_in = 1024 - (1024 // 6 + 32)
    text = _zipf_text(5 * max_in)
    for chunks in (1, 2, 5):
        plain = text[:chunks * max_in - 7]
        cases[f"{chunks}-chunks"] = (snappy.hadoop_compress(plain, 1024), plain)
    plains = [text[:300], b"", text[300:3000], b"x"]
    cases["blocks"] = (b"".join(snappy.hadoop_compress(p, 1024) for p in plains), b"".join(plains))
    return cases


@pytest.mark.parametrize("case", ["empty", "lone-header", "one-chunk", "1-chunks", "2-chunks",
                                  "5-chunks", "blocks"])
def test_chunk_table_matches_framing(case):
    data, plain = _framed_cases()[case]
    assert snappy.hadoop_decompress(data) == plain
    table, total = snappydec.chunk_table(data)
    assert table.dtype == torch.int64 and table.shape[0] == 4 and total == len(plain)
    src, clen, dst, ulen = table.tolist()
    n = len(src)
    if case in ("empty", "lone-header"):
        assert n == 0
    if case.endswith("-chunks"):
        assert n == int(case[0])
    if case == "blocks":
        assert n == 1 + 4 + 1                    # 300 bytes, 2,700 bytes of 822 a chunk, "x"
    # the lengths add up to the file: every byte is a chunk's or a 4-byte header's
    blocks = 0 if case == "empty" else 4 if case == "blocks" else 1
    assert sum(clen) + 4 * n + 4 * blocks == len(data)
    run = 0
    for i in range(n):
        assert dst[i] == run                     # a running sum
        run += ulen[i]
        assert int.from_bytes(data[src[i] - 4:src[i]], "big") == clen[i]
        piece = data[src[i]:src[i] + clen[i]]
        assert snappy.hadoop_decompress(_frame([piece], ulen[i])) == plain[dst[i]:dst[i] + ulen[i]]
    assert run == total


def _bad_framing():
    good = snappy.hadoop_compress(_zipf_text(3000), 1024)
    stream = snappy.compress(b"abcdabcdabcd")
    return {
        "truncated block header": good + b"\x00\x00",
        "truncated chunk header": good[:4] + good[4:6],
        "chunk length 0": (12).to_bytes(4, "big") + (0).to_bytes(4, "big") + stream,
        "chunk length negative": (12).to_bytes(4, "big") + b"\xff\xff\xff\xfe" + stream,
        "chunk past the end": good[:-1],
        "chunks do not add up": (11).to_bytes(4, "big") + len(stream).to_bytes(4, "big") + stream,
        # a stream of n = 4 bytes may claim 22 n + 64 = 152 bytes, not 153
        "preamble too large": _frame([_varint(153) + b"\x00a"], 153),
    }


def test_chunk_table_rejects_bad_framing(tmp_path):
    for name, data in _bad_framing().items():
        with pytest.raises(IOError):
            snappy.hadoop_decompress(data)       # the host decoder rejects it too
        with pytest.raises(IOError, match="some-name"):
            snappydec.chunk_table(data, "some-name")
        p = tmp_path / "bad.snappy"
        p.write_bytes(data)
        with pytest.raises(IOError, match="bad.snappy"):
            snappydec.decode_file(str(p), "cpu")
    # the largest preamble the bound lets through is a question for the decoder
    table, total = snappydec.chunk_table(_frame([_varint(152) + b"\x00a"], 152))
    assert table.tolist() == [[8], [4], [0], [152]] and total == 152


def test_chunk_table_stand_alone_under_asan_ubsan(tmp_path):
    """native/tests/snappyindex_selftest.cc, a program of its own with the walk
    compiled in under -fsanitize=address,undefined, over the good files and the
    bad-framing cases."""
    import importlib.util
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hbmr_native_build",
                                                  os.path.join(root, "native", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_sanitized("asan")["snappyindex_selftest"]
    files, want = [], []
    for i, (data, _) in enumerate(_framed_cases().values()):
        table, total = snappydec.chunk_table(data)
        cols = "".join(" %d:%d:%d:%d" % tuple(c) for c in table.t().tolist())
        want.append(f"{table.shape[1]} {total}{cols}")
        files.append(tmp_path / f"good{i}")
        files[-1].write_bytes(data)
    for i, data in enumerate(_bad_framing().values()):
        want.append("bad")
        files.append(tmp_path / f"bad{i}")
        files[-1].write_bytes(data)
    r = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want


def test_decode_file_cpu_equals_codec(tmp_path):
    for name, (data, plain) in _framed_cases().items():
        p = tmp_path / f"{name}.snappy"
        p.write_bytes(data)
        got = snappydec.decode_file(str(p), "cpu")
        assert got.dtype == torch.uint8 and got.device.type == "cpu"
        assert bytes(got.numpy()) == SnappyCodec().decompress(data) == plain


def test_decode_chunks_twin_and_table_checks():
    plain = _zipf_text(4000)
    data = snappy.hadoop_compress(plain, 1024)
    table, total = snappydec.chunk_table(data)
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    out, status = snappydec.decode_chunks(src, table)
    assert bytes(out.numpy()) == plain and not status.any() and total == len(plain)
    for row, value in ((0, len(data)), (1, len(data)), (2, total), (3, total), (0, -1)):
        t = table.clone()
        t[row, -1] = value
        with pytest.raises(ValueError, match="outside"):
            snappydec.decode_chunks(src, t, torch.empty(total, dtype=torch.uint8))


# ----------------------------------------------------------------------------- CPU: the jobs
def _local():
    conf = JobConf()
    conf.set("mapred.job.tracker", "local")
    return conf


def test_snappy_input_is_eligible_other_codecs_are_not(tmp_path):
    plain = b"2 1\n1 2\nfoo bar foo\n"
    sn = tmp_path / "in.snappy"
    sn.write_bytes(snappy.hadoop_compress(plain))
    gz = tmp_path / "in.txt.gz"
    gz.write_bytes(gzip.compress(plain))
    assert wordtable.why_ineligible(str(sn), 1) is None
    assert ss_job.why_ineligible(str(sn)) is None
    assert wordtable.why_ineligible(str(gz), 1) == f"compressed input {gz}"
    assert ss_job.why_ineligible(str(gz)) == f"compressed input {gz}"
    for ext in (".bz2", ".deflate"):
        other = tmp_path / f"in{ext}"
        other.write_bytes(b"x")
        assert wordtable.why_ineligible(str(other), 1) == f"compressed input {other}"
    with pytest.raises(ValueError, match="compressed input"):
        grep_job.gpu_job(str(gz), str(tmp_path / "o1"), "foo")
    with pytest.raises(ValueError, match="not a local file"):
        grep_job.gpu_job("hdfs://namenode:8020/in.txt", str(tmp_path / "o2"), "foo")
    assert grep_job.gpu_job(str(sn), str(tmp_path / "o3"), "foo").get(
        "hbmr.splitjob.class") == "hbmr.models.grep:GrepSplitJob"
    assert wordtable.wordcount_job(str(sn), str(tmp_path / "o4")) is not None
    assert ss_job.gpu_job(str(sn), str(tmp_path / "o5")) is not None


def _grep_falls_back_on_gz(tmp_path, caplog):
    import logging
    gz = tmp_path / "in.txt.gz"
    gz.write_bytes(gzip.compress(b"foo bar foo\nbar\n"))
    with caplog.at_level(logging.WARNING, logger="hbmr.examples.grep"):
        rj = grep_example.run(str(gz), str(tmp_path / "g"), "foo|bar", conf=_local(), gpu=True)
    assert rj.isSuccessful()
    assert "compressed input" in caplog.text and "classic search job" in caplog.text


def test_grep_gpu_flag_over_gz_runs_the_classic_search(tmp_path, caplog):
    _grep_falls_back_on_gz(tmp_path, caplog)
    part = [f for f in os.listdir(tmp_path / "g") if f.startswith("part-")]
    text = b"".join((tmp_path / "g" / f).read_bytes() for f in part)
    assert text == b"2\tbar\n2\tfoo\n" or text == b"2\tfoo\n2\tbar\n"


PROGRAMS = ["wordcount", "multifilewc", "aggregatewordcount", "grep", "secondarysort"]
PATTERN = r"w[1-4]\d?|1\d+"


def _job_text(seed, nbytes):
    """Lines that every program has work in: words, and int pairs."""
    rnd = random.Random(seed)
    lines, size = [], 0
    while size < nbytes:
        if rnd.random() < 0.5:
            lines.append(b"%d %d" % (rnd.randrange(-40, 40), rnd.randrange(-10 ** 5, 10 ** 5)))
        else:
            lines.append(b"%d %d " % (rnd.randrange(9), rnd.randrange(99)) +
                         b" ".join(b"w%d" % rnd.randrange(60) for _ in range(rnd.randrange(8))))
        size += len(lines[-1]) + 1
    return b"\n".join(lines) + b"\n"


def _write_snappy_input(root, big=0):
    """3 ``.snappy`` files of a few KiB (buffer size 1024: several chunks each):
    one has no final newline, one is empty; ``big``: one more file of that many
    bytes at the default buffer size.  Returns (dir, {file: plain})."""
    inp = root / "in"
    inp.mkdir()
    plains = {"a.snappy": _job_text(1, 5000), "b.snappy": _job_text(2, 3000)[:-1] + b" 7",
              "c.snappy": b""}
    assert not plains["b.snappy"].endswith(b"\n")
    for name, plain in plains.items():
        (inp / name).write_bytes(snappy.hadoop_compress(plain, 1024))
    if big:
        plains["d.snappy"] = _job_text(4, big)
        (inp / "d.snappy").write_bytes(snappy.hadoop_compress(plains["d.snappy"]))
    return str(inp), plains


def _run_classic(program, inp, out):
    """The classic job of ``program`` over ``inp`` on the LocalJobRunner."""
    from hbmr.examples import aggregatewordcount as agg_example
    from hbmr.examples import multifilewc as mf_example
    from hbmr.mapred.lib.aggregate import ValueAggregatorJob
    if program == "grep":
        assert grep_example.run(inp, out, PATTERN, conf=_local()).isSuccessful()
        return out
    if program == "wordcount":
        job = wc_model.make_job(inp, out, 2, _local())
    elif program == "multifilewc":
        job = mf_example.make_job(inp, out, 2, _local(), 2)
    elif program == "secondarysort":
        job = ss_example.make_job(inp, out, 2, _local())
    else:
        job = ValueAggregatorJob.createValueAggregatorJob(inp, out, [agg_example.WordCountPlugIn],
                                                          2, _local())
    assert JobClient.runJob(job, verbose=False).isSuccessful()
    return out


def _run_gpu_flag(cl, program, inp, out):
    """``program`` through its ``-gpu`` entry point on ``cl``; returns the
    counters of the split-level job it submitted (there must be exactly one).
    grep's second job, the classic grep-sort, goes through the local runner
    behind the ``-gpu`` search, as it does for the classic output it is
    compared with: it needs a CPU slot, which a GPU-only cluster lacks, and on
    a cluster with several slots the reduce merges its maps' segments in the
    order they complete, so rows of equal count come out in an order no run
    fixes (:func:`_check_grep_entry_point` runs the whole entry point)."""
    seen = []
    submit = cl.submit_job

    def spy(job):
        rj = submit(job)
        seen.append((job, rj))
        return rj
    cl.submit_job = spy
    try:
        if program == "grep":
            assert grep_example._search_gpu(inp, out + "-search", PATTERN, 0, None, cl) is not None
            assert grep_example._sort(out + "-search", out, _local(), None, False).isSuccessful()
        elif program == "secondarysort":
            assert ss_example.run(inp, out, 2, cluster=cl, gpu=True).isSuccessful()
        elif program in ("wordcount", "multifilewc"):
            assert driver.run(program, [inp, out, "-r", "2", "-m", "2", "-gpu"], cluster=cl) == 0
        else:
            assert driver.run(program, [inp, out, "2", "-gpu"], cluster=cl) == 0
    finally:
        cl.submit_job = submit
    split = [rj for job, rj in seen if job.get("hbmr.splitjob.class")]
    assert len(split) == 1, [job.get_job_name() for job, _ in seen]
    return split[0].getCounters()


def _parts(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))
            if f.startswith("part-")}


@pytest.fixture(scope="module")
def snappy_corpus(tmp_path_factory):
    """The small files and each program's classic output over them, once."""
    root = tmp_path_factory.mktemp("snappy-jobs")
    inp, plains = _write_snappy_input(root)
    return inp, plains, {p: _run_classic(p, inp, str(root / f"classic-{p}")) for p in PROGRAMS}


def _check_grep_entry_point(cl, tmp_path, inp, classic):
    """``grep -gpu`` as a whole on a cluster with CPU slots (both jobs on it):
    the classic job's rows, by count descending; rows of equal count in any
    order (see :func:`_run_gpu_flag`)."""
    out = str(tmp_path / "out-grep-whole")
    assert grep_example.run(inp, out, PATTERN, cluster=cl, gpu=True).isSuccessful()
    got, want = _parts(out), _parts(classic)
    assert list(got) == list(want) == ["part-00000"]
    rows = got["part-00000"].splitlines()
    assert sorted(rows) == sorted(want["part-00000"].splitlines())
    counts = [int(r.split(b"\t")[0]) for r in rows]
    assert counts == sorted(counts, reverse=True)


def _check_job(cl, tmp_path, program, inp, plains, classic):
    out = str(tmp_path / f"out-{program}")
    cs = _run_gpu_flag(cl, program, inp, out)
    got, want = _parts(out), _parts(classic)
    assert want and list(got) == list(want)
    for name in want:
        assert got[name] == want[name], (program, name)
    assert sum(len(v) for v in want.values()) > 100
    assert cs.get(GROUP, DECODED) == sum(len(v) for v in plains.values())
    return cs


@pytest.mark.parametrize("program", PROGRAMS)
def test_jobs_on_cpu_slots_equal_classic_over_snappy_input(tmp_path, snappy_corpus, program):
    inp, plains, classic = snappy_corpus
    with LocalCluster(JobConf(), num_trackers=1, cpu_slots=2) as cl:
        cs = _check_job(cl, tmp_path, program, inp, plains, classic[program])
        if program == "grep":
            _check_grep_entry_point(cl, tmp_path, inp, classic[program])
    assert cs.get(JOB_GROUP, "CPU_MAP_TASKS") >= 1


def test_corrupt_file_fails_the_map_not_the_process(tmp_path):
    inp = tmp_path / "bad.snappy"
    good = snappy.hadoop_compress(b"one two\n" * 50)
    inp.write_bytes(good[:-3] + b"\xff\xff\xff")           # framing intact, stream malformed
    with pytest.raises(IOError):
        snappy.hadoop_decompress(inp.read_bytes())
    conf = JobConf()
    conf.set_int("mapred.map.max.attempts", 1)
    with LocalCluster(conf, num_trackers=1, cpu_slots=1) as cl:
        with pytest.raises(RuntimeError, match="Job failed"):
            wc_model.run(str(inp), str(tmp_path / "o"), 1, conf=conf, cluster=cl, gpu=True)
        # the cluster goes on
        ok = tmp_path / "ok.snappy"
        ok.write_bytes(good)
        assert wc_model.run(str(ok), str(tmp_path / "o2"), 1, cluster=cl, gpu=True).isSuccessful()
    assert (tmp_path / "o2" / "part-00000").read_bytes() == b"one\t50\ntwo\t50\n"


# ----------------------------------------------------------------------------- GPU: the kernel
def _layout(streams, src_mis=0, dst_mis=None, guard=GUARD):
    """A source buffer and a table for ``streams``: every stream begins at
    ``src_mis`` past a multiple of 16, destination i at ``dst_mis[i]`` (default:
    i) past one with ``guard`` bytes in front; after the last destination comes
    nothing, as after the last stream.  Returns (src bytes, table, out size,
    expected [(dst offset, plain)])."""
    src, rows, want = bytearray(), [], []
    dpos = 0
    for i, s in enumerate(streams):
        src += b"\xEE" * ((src_mis - len(src)) % 16)
        plain = snappy.decompress(s) if isinstance(s, bytes) else s[1]
        raw = s if isinstance(s, bytes) else s[0]
        dpos += guard
        dm = i % 16 if dst_mis is None else dst_mis[i]
        dpos += (dm - dpos) % 16
        rows.append((len(src), len(raw), dpos, len(plain)))
        want.append((dpos, plain))
        src += raw
        dpos += len(plain)
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).t().contiguous()
    return bytes(src), table, dpos, want


def _decode_on_gpu(streams, src_mis=0, dst_mis=None):
    """Decode ``streams`` in one launch into a guarded buffer; returns (status
    list, [(got, want)] per chunk, whether every guard byte is untouched)."""
    src, table, size, want = _layout(streams, src_mis, dst_mis)
    pad = torch.full((16 + len(src),), 0xEE, dtype=torch.uint8)
    pad[16:] = torch.frombuffer(bytearray(src), dtype=torch.uint8) if src else pad[16:]
    dsrc = pad.cuda()[16:]
    assert dsrc.data_ptr() % 16 == 0 and dsrc.numel() == len(src)
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    _, status = snappydec.decode_chunks(dsrc, table, out)
    got = out.cpu().numpy()
    mask = np.ones(size, dtype=bool)
    pairs = []
    for off, plain in want:
        mask[off:off + len(plain)] = False
        pairs.append((got[off:off + len(plain)].tobytes(), plain))
    return status.tolist(), pairs, bool((got[mask] == 0xA5).all())


def _assert_all_decoded(streams, **kw):
    status, pairs, guards = _decode_on_gpu(streams, **kw)
    assert status == [0] * len(streams)
    for i, (got, want) in enumerate(pairs):
        assert got == want, f"chunk {i} of {len(pairs)}"
    assert guards


@pytest.mark.gpu
def test_gpu_decode_every_element_form():
    streams = []
    for n in (1, 59, 60, 61, 255, 256, 257, 65_536, 65_537):
        streams.append(_encode([("lit", _rand(n, n))]))
    streams.append(_encode([("lit", _rand(100, 5), 4), ("lit", b"tail")]))
    streams.append(_encode([("lit", _rand(61, 6), 2), ("lit", _rand(300, 7), 3)]))
    for ln in (4, 11):
        for off in (1, 255, 256, 2_047):
            streams.append(_encode([("lit", _rand(2_047, off)), ("copy", off, ln, 1),
                                    ("lit", b"after")]))
    for ln in (1, 64):
        for off in (1, 2_048, 65_535):
            streams.append(_encode([("lit", _rand(65_535, off)), ("copy", off, ln, 2),
                                    ("lit", b"after")]))
    for ln in (1, 33, 64):
        for off in (1, 65_536, 70_000):
            streams.append(_encode([("lit", _rand(70_001, off)), ("copy", off, ln, 4),
                                    ("copy", 70_001, 64, 4), ("lit", b"after")]))
    assert streams[-1][:3] == _varint(70_001 + 64 + 64 + 5)
    _assert_all_decoded(streams)


def _random_stream(seed, elements, max_lit=100):
    """Any valid stream: literals of 1..max_lit bytes, copies of every form at
    any offset into what was produced, overlapping or not."""
    rnd = random.Random(seed)
    els, produced = [("lit", rnd.randbytes(rnd.randrange(1, 9)))], 8
    produced = len(els[0][1])
    for _ in range(elements):
        if rnd.random() < 0.3:
            data = rnd.randbytes(rnd.choice([1, 2, 5, 17, 60, 61, rnd.randrange(1, max_lit + 1)]))
            els.append(("lit", data))
            produced += len(data)
            continue
        off = rnd.choice([1, 2, 3, rnd.randrange(1, 70), rnd.randrange(1, produced + 1),
                          produced])
        off = min(off, produced)
        ln = rnd.choice([1, 4, 11, 63, 64, rnd.randrange(1, 65)])
        ob = rnd.choice([2, 4]) if off < 1 << 16 else 4
        if 4 <= ln <= 11 and off < 2048 and rnd.random() < 0.5:
            ob = 1
        els.append(("copy", off, ln, ob))
        produced += ln
    return _encode(els)


@pytest.mark.gpu
def test_gpu_overlapping_copies():
    streams = []
    for off in (1, 2, 3, 7, 63, 64, 65):
        for ln in (1, 4, 63, 64):
            # directly after a literal of exactly `off` bytes, and again after that copy
            streams.append(_encode([("lit", _rand(off, off)), ("copy", off, ln, 2),
                                    ("copy", off, ln, 4), ("copy", min(off, ln), ln, 2),
                                    ("lit", b"!")]))
            if ln == 4:
                streams.append(_encode([("lit", _rand(off, off)), ("copy", off, ln, 1),
                                        ("copy", off, ln, 1)]))
    # chains of 1,000 copies, each reading the previous element's output
    for seed in range(4):
        rnd = random.Random(seed)
        els, prev = [("lit", rnd.randbytes(8))], 8
        for _ in range(1000):
            off = prev if seed == 0 else rnd.randrange(1, prev + 1)
            ln = prev if seed == 0 else rnd.randrange(1, 65)
            els.append(("copy", off, ln, rnd.choice([2, 4])))
            prev = ln
        streams.append(_encode(els))
    streams += [_random_stream(100 + s, 1500) for s in range(8)]
    assert all(len(snappy.decompress(s)) > 0 for s in streams[-12:])
    _assert_all_decoded(streams)


@pytest.mark.gpu
def test_gpu_decode_every_misalignment_leaves_guards():
    rnd = random.Random(9)
    streams = []
    for i in range(16):
        streams.append(_encode([("lit", rnd.randbytes(300 + 17 * i)), ("copy", 5, 64, 2),
                                ("lit", rnd.randbytes(1 + i)), ("copy", 290, 33, 2),
                                ("lit", rnd.randbytes(64 + i)), ("copy", 1, 7, 1)]))
    for src_mis in range(16):
        # destination i of this launch at (i + src_mis) mod 16: over the 16 launches every
        # chunk meets every pair, and each of the 16 misalignments ends a buffer once
        _assert_all_decoded(streams, src_mis=src_mis,
                            dst_mis=[(i + src_mis) % 16 for i in range(16)])


@pytest.mark.gpu
def test_gpu_decode_chunk_counts():
    text = _zipf_text(1 << 20)
    rnd = random.Random(21)
    pool = []
    for i in range(257):
        n = 0 if i % 9 == 0 else rnd.choice([1, 3_000, rnd.randrange(0, 3_001)])
        a = rnd.randrange(0, len(text) - 3_000)
        pool.append(snappy.compress(text[a:a + n]))
    assert pool[0] == b"\x00" and any(len(snappy.decompress(s)) == 3_000 for s in pool)
    for n in (0, 1, 2, 63, 64, 65, 257):
        _assert_all_decoded(pool[:n])
    big = snappy.compress(text)
    assert big[:3] == _varint(1 << 20)
    _assert_all_decoded([pool[1], (big, text), pool[2]])


@pytest.mark.gpu
@pytest.mark.parametrize("buffer_size", [snappy.BUFFER_SIZE_DEFAULT, 1024])
def test_gpu_decode_equals_codec_on_real_data(tmp_path, buffer_size):
    n = 1 << 20
    plains = {"zipf": _zipf_text(n), "pairs": _pair_text(n), "random": _rand(n, 1),
              "one-byte": b"z" * n}
    for name, plain in plains.items():
        data = snappy.hadoop_compress(plain, buffer_size)
        p = tmp_path / f"{name}.snappy"
        p.write_bytes(data)
        got = snappydec.decode_file(str(p), "cuda")
        assert got.device.type == "cuda" and got.dtype == torch.uint8
        assert got.cpu().numpy().tobytes() == plain, name
    assert len(snappy.hadoop_compress(plains["random"], buffer_size)) > n       # all literals
    assert len(snappy.hadoop_compress(plains["one-byte"], buffer_size)) < n // 10


def _malformed():
    """One stream for each of the host decoder's rejections, with a preamble
    the chunk table's bound lets through."""
    return {
        "truncated literal": _encode([("raw", bytes([9 << 2]) + b"12345")], ulen=10),
        "truncated literal length": _encode([("lit", b"abcd"), ("raw", bytes([61 << 2, 1]))],
                                            ulen=100),
        "truncated copy operand": _encode([("lit", b"abcd"), ("raw", bytes([2 | (3 << 2), 4]))],
                                          ulen=8),
        "offset 0": _encode([("lit", b"abcd"), ("copy", 0, 4, 2)]),
        "offset past the bytes produced": _encode([("lit", b"abcd"), ("copy", 5, 4, 2)]),
        "4-byte offset past the bytes produced": _encode([("lit", b"abcd"),
                                                          ("copy", 0xFFFFFFFF, 4, 4)]),
        "output overrun by a copy": _encode([("lit", b"abcd"), ("copy", 4, 4, 2)], ulen=6),
        "output overrun by a literal": _encode([("lit", b"abcd"), ("lit", b"efgh" * 40)], ulen=100),
        "output short of the preamble": _encode([("lit", b"abcd")], ulen=20),
        "preamble runs on": b"\x80\x80\x80",
    }


def test_host_decoder_rejects_the_malformed_streams():
    for name, s in _malformed().items():
        with pytest.raises(IOError):
            snappy.decompress(s)
        if name != "preamble runs on":
            assert snappy._lib().hbmr_snappy_uncompressed_length(s, len(s)) >= 0, name


@pytest.mark.gpu
def test_gpu_malformed_streams_set_status(tmp_path):
    test_host_decoder_rejects_the_malformed_streams()            # first, on the CPU
    good = [snappy.compress(_zipf_text(700, seed=s)) for s in (1, 2)]
    bad = {k: v for k, v in _malformed().items() if k != "preamble runs on"}
    streams, where = [good[0]], {}
    for name, s in bad.items():
        where[len(streams)] = name
        want = snappy._lib().hbmr_snappy_uncompressed_length(s, len(s))
        streams += [(s, b"\x00" * want), good[len(streams) % 2]]
    status, pairs, guards = _decode_on_gpu(streams)
    for i, (got, want) in enumerate(pairs):
        if i in where:
            assert status[i] != 0, where[i]
        else:
            assert status[i] == 0 and got == want, i
    assert guards
    # a file holding such a chunk between good ones: IOError naming the file
    for name, s in bad.items():
        want = snappy._lib().hbmr_snappy_uncompressed_length(s, len(s))
        p = tmp_path / "bad.snappy"
        p.write_bytes(_frame([good[0], s, good[1]], 700 + want + 700))
        with pytest.raises(IOError, match="bad.snappy"):
            snappydec.decode_file(str(p), "cpu")
        with pytest.raises(IOError, match=r"bad\.snappy.* chunk 1 "):
            snappydec.decode_file(str(p), "cuda")


# ----------------------------------------------------------------------------- GPU: the jobs
def _gpu_cluster():
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    return LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0)


@pytest.fixture(scope="module")
def snappy_corpus_big(tmp_path_factory):
    """The small files plus one of about 1 MiB (several chunks of the default
    size), and each program's classic output."""
    root = tmp_path_factory.mktemp("snappy-jobs-gpu")
    inp, plains = _write_snappy_input(root, big=1 << 20)
    assert snappydec.chunk_table(open(os.path.join(inp, "d.snappy"), "rb").read())[0].shape[1] >= 4
    return inp, plains, {p: _run_classic(p, inp, str(root / f"classic-{p}")) for p in PROGRAMS}


@pytest.mark.gpu
@pytest.mark.parametrize("program", PROGRAMS)
def test_gpu_jobs_equal_classic_over_snappy_input(tmp_path, snappy_corpus_big, program):
    inp, plains, classic = snappy_corpus_big
    with _gpu_cluster() as cl:
        cs = _check_job(cl, tmp_path, program, inp, plains, classic[program])
    assert cs.get(JOB_GROUP, "GPU_MAP_TASKS") >= 1 and cs.get(JOB_GROUP, "CPU_MAP_TASKS") == 0


@pytest.mark.gpu
def test_gpu_second_job_finds_decoded_split_resident(tmp_path):
    plain = _job_text(8, 300_000)
    inp = tmp_path / "in.snappy"
    inp.write_bytes(snappy.hadoop_compress(plain))
    counters = []
    with _gpu_cluster() as cl:
        for run in range(2):
            rj = wc_model.run(str(inp), str(tmp_path / f"o{run}"), 1, cluster=cl, gpu=True)
            assert rj.isSuccessful()
            counters.append(rj.getCounters())
    assert counters[0].get(GROUP, DECODED) == len(plain)
    assert counters[0].get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_MISSES") == 1
    assert counters[1].get(GROUP, DECODED) == 0
    assert counters[1].get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_HITS") == 1
    assert counters[1].get("hbmr.GpuCounters", "GPU_SPLIT_CACHE_MISSES") == 0
    assert _parts(str(tmp_path / "o0")) == _parts(str(tmp_path / "o1"))
