"""GPU Grep (split-level job, native/kernels/grep.hip): the pattern compiler's
DFA against Python ``re`` (RegexMapper's matcher: leftmost-first, finditer),
the match-table primitives against collections.Counter, and the job's output
equal to the classic grep's."""
import collections
import os
import random
import re

import pytest
import torch

from hbmr.examples import grep as grep_example
from hbmr.mapred import JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.models import grep as grep_job
from hbmr.ops import grep, text

PATTERNS = [r"w[1-4]", r"a|ab", r"(a|ab)(c|bcd)?", r"[a-z]+", r"foo|foobar", r"ab*c?", r"^w\d+",
            r"\d+$", r"a.c", r"(ab)+", r"x*xy?", r"[^ ]+ [^ ]+", r"a{2,3}", r"(a|b)*abb", r"a+?b",
            r"(a|ab)(b|bc)", r"\w+@\w+", r"(?:fo|foo)(?:o|ob)ar?", r"(a*)*b"]
INELIGIBLE = [r"a*", r"^$", r"\bfoo", r"(a)\1", r".*foo", "é"]
ALPHABET = "abcxyfo w12 d@"
COUNTER_GROUP = "hbmr.GrepCounters"
JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"


def _lines_of(data):
    """(offset, line) pairs under LineRecordReader's rule."""
    off = 0
    raws = data.split(b"\n")
    if raws and not raws[-1]:
        raws.pop()
    for raw in raws:
        yield off, raw[:-1] if raw.endswith(b"\r") else raw
        off += len(raw) + 1


def _re_spans(pat, data):
    rx = re.compile(pat)
    return [(off + m.start(), m.end() - m.start()) for off, ln in _lines_of(data)
            for m in rx.finditer(ln.decode())]


def _re_counts(pat, data):
    rx = re.compile(pat)
    return dict(collections.Counter(m.group().encode() for _, ln in _lines_of(data)
                                    for m in rx.finditer(ln.decode())))


def _table(blob, counts):
    return dict(text.parse_table(bytes(blob.cpu().numpy()), counts.cpu()))


def _small_buffer(seed=3, n=400):
    rnd = random.Random(seed)
    lines = []
    for i in range(n):
        ln = "".join(rnd.choice(ALPHABET) for _ in range(rnd.randint(0, 40)))
        if i % 11 == 0:
            ln = ln[:5] + "\r" + ln[5:]          # a lone \r inside a line
        lines.append(ln + ("\r" if i % 5 == 0 else ""))
    return "\n".join(lines).encode()             # no final newline


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("pat", PATTERNS)
def test_simulate_equals_re_finditer(pat):
    prog = grep.compile_pattern(pat)
    assert prog is not None, grep.why_ineligible(pat)
    assert prog.nstates * prog.nclasses * 2 <= 32 << 10 and prog.accept[0] == 0
    for seed in (3, 4):
        data = _small_buffer(seed)
        assert b"\r\n" in data and not data.endswith(b"\n")
        assert grep.simulate(prog, data) == _re_spans(pat, data)
        assert grep.simulate(prog, data + b"\n") == _re_spans(pat, data + b"\n")


def test_leftmost_first_not_leftmost_longest():
    assert grep.simulate(grep.compile_pattern(r"a|ab"), b"ab") == [(0, 1)]
    assert grep.simulate(grep.compile_pattern(r"\d+$"), b"12 34\r\n56\r") == [(3, 2), (7, 2)]
    assert grep.simulate(grep.compile_pattern(r"^w\d+"), b"w1 w2\nxw3\nw45") == [(0, 2), (10, 3)]


def test_eligibility():
    for pat in PATTERNS:
        assert grep.compile_pattern(pat) is not None and grep.why_ineligible(pat) is None
    for pat in INELIGIBLE:
        assert grep.compile_pattern(pat) is None, pat
        assert grep.why_ineligible(pat)
    assert grep.compile_pattern(r"w[1-4]", 1) is None
    assert grep.compile_pattern(r"(w)[1-4]", 1) is None
    assert "squared" in grep.why_ineligible(r".*foo")
    assert "empty" in grep.why_ineligible(r"a*")
    assert grep.compile_pattern(r"a{2,17}") is None and grep.compile_pattern(r"a{2,16}") is not None
    assert grep.compile_pattern(r"(?i)abc") is None
    assert grep.compile_pattern(r"(a|b|c|x|y){16}(a|b){16}(x|y){16}w", max_states=8) is None
    with pytest.raises(ValueError, match="empty"):
        grep_job.gpu_job("in", "out", r"a*")


def test_cpu_match_tables():
    data = b"foo bar  foo bar\r\nx foo bar\nfoo  bar\n\nfoo bar"
    pat = r"[^ ]+ [^ ]+"
    blob, counts = grep.count_matches_cpu(data, pat)
    want = _re_counts(pat, data)
    assert want == {b"foo bar": 3, b"x foo": 1} and _table(blob, counts) == want
    assert _table(*grep.count_matches_cpu(data, r"(f)(o+)", 2)) == {b"oo": 5}
    mb, mc, pb, pw = grep.merge_tables_cpu(bytes(blob.numpy()) * 2, torch.cat([counts, counts]), 3)
    items = text.parse_table(bytes(mb.numpy()), mc)
    assert dict(items) == {w: 2 * n for w, n in want.items()}
    assert sum(pw) == len(want) and sum(pb) == mb.numel()
    i = 0
    for p, nw in enumerate(pw):
        assert all(text.partition_of(w, 3) == p for w, _ in items[i:i + nw])
        assert pb[p] == sum(len(w) + 1 for w, _ in items[i:i + nw])
        i += nw
    # the device-side entry point takes host tensors to the CPU twin
    gb, gc, non_ascii = grep.count_matches(torch.frombuffer(bytearray(data), dtype=torch.uint8),
                                           grep.compile_pattern(pat))
    assert _table(gb, gc) == want and not non_ascii


def _corpus(tmp_path, files=3, lines=300, seed=5, unicode_words=True):
    rnd = random.Random(seed)
    vocab = [f"w{i}" for i in range(40)] + ["foo", "foobar", "ab", "abb", "x@y", "a@b.c", "12"]
    if unicode_words:
        vocab += ["Straße", "naïve"]
    d = tmp_path / "in"
    d.mkdir()
    for f in range(files):
        out = []
        for j in range(lines):
            words = [rnd.choice(vocab) for _ in range(rnd.randint(0, 12))]
            out.append(" ".join(words) + ("\r" if j % 7 == 0 else ""))
        (d / f"part-{f}").write_text("\n".join(out) + ("\n" if f != 1 else ""), encoding="utf-8")
    return d


def _outputs(out):
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))
            if fn.startswith("part-")}


@pytest.mark.parametrize("trackers", [1, 2])
def test_grep_gpu_flag_equals_classic(tmp_path, trackers):
    inp = _corpus(tmp_path)
    pat = r"w[1-4]\d?|\w+@\w+|Stra\w+"
    with LocalCluster(JobConf(), num_trackers=trackers, cpu_slots=2) as cl:
        grep_example.run(str(inp), str(tmp_path / "classic"), pat, cluster=cl)
        grep_example.run(str(inp), str(tmp_path / "gpu"), pat, cluster=cl, gpu=True)
        job = grep_job.gpu_job(str(inp), str(tmp_path / "search"), pat, maps=4)
        rj = cl.submit_job(job)
        assert rj.waitForCompletion(60) and rj.isSuccessful(), rj.getFailureInfo()
        assert rj.getCounters().get(COUNTER_GROUP, "GREP_CPU_FALLBACK_SPLITS") > 0
        if trackers == 1:
            # an ineligible pattern takes the classic search job
            grep_example.run(str(inp), str(tmp_path / "c2"), r"\bfoo\w*", cluster=cl)
            grep_example.run(str(inp), str(tmp_path / "g2"), r"\bfoo\w*", cluster=cl, gpu=True)
            assert _outputs(tmp_path / "g2") == _outputs(tmp_path / "c2")
    assert sorted(os.listdir(tmp_path / "search")) == \
        ["_SUCCESS"] + [f"part-{r:05d}" for r in range(trackers)]
    got, want = _outputs(tmp_path / "gpu"), _outputs(tmp_path / "classic")
    assert list(got) == ["part-00000"] and want["part-00000"]
    if trackers == 1:
        assert got == want
    else:
        rows = got["part-00000"].splitlines()
        assert sorted(rows) == sorted(want["part-00000"].splitlines())
        counts = [int(r.split(b"\t")[0]) for r in rows]
        assert counts == sorted(counts, reverse=True)


# ----------------------------------------------------------------------------- GPU
_SNIPPET = "w12 abcabb foobar a@b xxy aab w3 abbc aac 12"


def _big_buffer():
    """~256 KiB of random ASCII lines: \\r\\n endings, one line of > 8 KiB that
    spans tiles (tile and lane boundaries fall inside matches), a match at the
    last byte with no final newline."""
    rnd = random.Random(11)
    parts, size = [], 0
    while size < 6000:
        ln = "".join(rnd.choice(ALPHABET) for _ in range(rnd.randint(0, 80)))
        ln += "\r\n" if rnd.random() < 0.3 else "\n"
        parts.append(ln)
        size += len(ln)
    long_line = "".join(_SNIPPET[rnd.randint(0, 5):] + " " for _ in range(220)) + "\n"
    assert len(long_line) > 8192
    parts.append(long_line)
    size += len(long_line)
    while size < 256 << 10:
        ln = "".join(rnd.choice(ALPHABET) for _ in range(rnd.randint(0, 80)))
        ln += "\r\n" if rnd.random() < 0.3 else "\n"
        parts.append(ln)
        size += len(ln)
    parts.append("ab abb foobar xy a@b w12")
    return "".join(parts).encode()


_BIG = {}


def _big():
    if not _BIG:
        data = _big_buffer()
        _BIG["data"] = data
        _BIG["dev"] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return _BIG["data"], _BIG["dev"]


def test_big_buffer_shape():
    data = _big_buffer()
    assert max(len(ln) for _, ln in _lines_of(data)) > 4096 and b"\r\n" in data
    assert not data.endswith(b"\n") and max(data) < 0x80
    for pat in (r"[a-z]+", r"[^ ]+ [^ ]+", r"\w+@\w+"):
        spans = _re_spans(pat, data)
        # a match across a 4096-byte tile boundary (also a 16-byte lane boundary)
        assert any(s // 4096 != (s + ln - 1) // 4096 for s, ln in spans), pat
        assert any(s // 16 != (s + ln - 1) // 16 and s // 4096 == (s + ln - 1) // 4096
                   for s, ln in spans), pat
    for pat in (r"\d+$", r"[^ ]+ [^ ]+"):
        s, ln = _re_spans(pat, data)[-1]
        assert s + ln == len(data), pat


@pytest.mark.gpu
@pytest.mark.parametrize("pat", PATTERNS)
def test_gpu_count_matches_equals_re(pat):
    data, buf = _big()
    prog = grep.compile_pattern(pat)
    assert prog is not None, grep.why_ineligible(pat)
    blob, counts, non_ascii = grep.count_matches(buf, prog)
    assert not non_ascii
    assert _table(blob, counts) == _re_counts(pat, data)


@pytest.mark.gpu
def test_gpu_candidates_and_selection_equal_simulate():
    """The kernels' intermediate results: every start offset's match and the
    finditer selection, position by position."""
    data, buf = _big()
    data, buf = data[:40000], buf[:40000].clone()
    for pat in (r"(a|ab)(c|bcd)?", r"[^ ]+ [^ ]+", r"\d+$", r"^w\d+"):
        prog = grep.compile_pattern(pat)
        pos, ln, end, _ = grep.candidates(buf, prog)
        assert list(zip(pos.tolist(), ln.tolist())) == grep._candidates(prog, data), pat
        assert end.tolist() == [p + n for p, n in zip(pos.tolist(), ln.tolist())]
        spos, slen = grep.select(pos, ln, end)
        assert list(zip(spos.tolist(), slen.tolist())) == _re_spans(pat, data), pat


@pytest.mark.gpu
def test_gpu_count_matches_empty_tiny_and_unaligned():
    prog = grep.compile_pattern(r"x+y?")
    blob, counts, non_ascii = grep.count_matches(torch.empty(0, dtype=torch.uint8, device="cuda"),
                                                 prog)
    assert blob.numel() == 0 and counts.numel() == 0 and not non_ascii
    one = torch.frombuffer(bytearray(b"x"), dtype=torch.uint8).cuda()
    assert _table(*grep.count_matches(one, prog)[:2]) == {b"x": 1}
    assert _table(*grep.count_matches(one, grep.compile_pattern(r"y"))[:2]) == {}
    buf = torch.frombuffer(bytearray(b"yxx xy\nxxy x"), dtype=torch.uint8).cuda()
    assert buf[1:].data_ptr() % 16 != 0
    assert _table(*grep.count_matches(buf[1:], prog)[:2]) == {b"xx": 1, b"xy": 1, b"xxy": 1,
                                                               b"x": 1}


@pytest.mark.gpu
def test_gpu_count_matches_table_growth(monkeypatch):
    """More distinct matches than the first table holds: overflow → retry larger."""
    monkeypatch.setattr(grep, "INITIAL_TABLE", 1024)
    data = b" ".join([b"u%d" % i for i in range(50_000)] * 2)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    blob, counts, _ = grep.count_matches(buf, grep.compile_pattern(r"u\d+"))
    got = _table(blob, counts)
    assert len(got) == 50_000 and set(got.values()) == {2}
    assert got.keys() == {b"u%d" % i for i in range(50_000)}


@pytest.mark.gpu
def test_gpu_count_matches_hot_key():
    """One match string is most of the matches (LDS pre-aggregation path)."""
    rnd = random.Random(2)
    words = [rnd.choice([b"the"] * 92 + [b"of"] * 5 + [b"w%d" % rnd.randint(0, 5000)] * 3)
             for _ in range(300_000)]
    data = b" ".join(words) + b"\n"
    pat = r"[a-z]+\d*"
    want = _re_counts(pat, data)
    assert sum(want.values()) == 300_000 and want[b"the"] >= 270_000
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    blob, counts, _ = grep.count_matches(buf, grep.compile_pattern(pat))
    assert _table(blob, counts) == want


@pytest.mark.gpu
def test_gpu_matches_with_spaces_merge_into_partitions():
    data, buf = _big()
    pat = r"[^ ]+ [^ ]+"
    blob, counts, _ = grep.count_matches(buf, grep.compile_pattern(pat))
    got = _table(blob, counts)
    assert got == _re_counts(pat, data) and all(b" " in w for w in got)
    mb, mc, pb, pw = grep.merge_tables(torch.cat([blob, blob]), torch.cat([counts, counts]), 4)
    items = text.parse_table(bytes(mb.cpu().numpy()), mc.cpu())
    assert dict(items) == {w: 2 * n for w, n in got.items()} and len(items) == len(got)
    i = 0
    for p, nw in enumerate(pw):
        assert all(text.partition_of(w, 4) == p for w, _ in items[i:i + nw])
        assert pb[p] == sum(len(w) + 1 for w, _ in items[i:i + nw])
        i += nw
    assert sum(pb) == mb.numel() and sum(pw) == len(items)


@pytest.mark.gpu
def test_gpu_non_ascii_flag():
    prog = grep.compile_pattern(r"[a-z]+")
    data = b"abc def\n" * 1000 + b"caf\xc3\xa9 x\n" + b"abc def\n" * 1000
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert grep.count_matches(buf, prog)[2] is True
    clean = torch.frombuffer(bytearray(data.replace(b"\xc3\xa9", b"e")), dtype=torch.uint8).cuda()
    assert grep.count_matches(clean, prog)[2] is False


@pytest.mark.gpu
def test_gpu_grep_job_equals_classic(tmp_path):
    inp = _corpus(tmp_path, files=4, lines=2000, unicode_words=False)
    pat = r"w[1-4]\d?|\w+@\w+"
    conf = JobConf()
    conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=0) as cl:
        job = grep_job.gpu_job(str(inp), str(tmp_path / "search"), pat, maps=6)
        rj = cl.submit_job(job)
        assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
        cs = rj.getCounters()
        assert cs.get(JOB_GROUP, "GPU_MAP_TASKS") >= 6
        assert cs.get(COUNTER_GROUP, "GREP_CPU_FALLBACK_SPLITS") == 0
    # the grep-sort job is a classic job: it needs CPU slots, which this cluster
    # does not have, so it and the classic run go through the local runner
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    grep_example._sort(str(tmp_path / "search"), str(tmp_path / "gpu"), local, None, False)
    grep_example.run(str(inp), str(tmp_path / "classic"), pat, conf=local)
    got, want = _outputs(tmp_path / "gpu"), _outputs(tmp_path / "classic")
    assert want["part-00000"] and got == want
