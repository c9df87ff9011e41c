"""What the byte-string jobs share: the hash aggregate past its LDS table
(native/kernels/bytes/span_table.h under text.hip and grep.hip), the per-file
eligibility reasons of hbmr/models/records.py and the examples' ``-gpu``
fallback (hbmr/examples/_gpu.py)."""
import collections
import logging
import random

import pytest
import torch

from hbmr.io import sequencefile as seqf
from hbmr.io.writable import BytesWritable, IntWritable, Text
from hbmr.ops import grep, text

GROUP = 4096          # items of one workgroup of the insert kernels; its LDS table has 2048 slots


def _got(data, us, ul, uc):
    return {data[s:s + n]: c for s, n, c in zip(us.tolist(), ul.tolist(), uc.tolist())}


@pytest.mark.gpu
def test_gpu_word_aggregate_past_lds_table():
    """One workgroup, twice as many distinct words as LDS slots: the LDS probes
    run out and those words go straight into the global table."""
    rnd = random.Random(11)
    words = set()
    while len(words) < GROUP:
        words.add(bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz")
                        for _ in range(rnd.randint(3, 9))))
    words = sorted(words)
    rnd.shuffle(words)
    data = b" ".join(words) + b"\n"
    weights = [rnd.randint(1, 1000) for _ in words]
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    starts, lens = text.tokenize(buf)
    assert starts.numel() == GROUP
    us, ul, uc, up = text.aggregate(buf, starts, lens, torch.tensor(weights).cuda(), 3)
    want = collections.Counter()
    for w, n in zip(words, weights):
        want[w] += n
    got = _got(data, us, ul, uc)
    assert len(got) == us.numel() == GROUP and got == dict(want)
    assert up.tolist() == [text.partition_of(data[s:s + n], 3)
                           for s, n in zip(us.tolist(), ul.tolist())]


@pytest.mark.gpu
def test_gpu_span_aggregate_past_lds_table():
    """The same over spans that hold spaces, some of them repeated at other offsets."""
    rnd = random.Random(12)
    distinct = set()
    while len(distinct) < GROUP - 96:
        distinct.add(b" ".join(bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz")
                                     for _ in range(rnd.randint(1, 4)))
                               for _ in range(rnd.randint(2, 3))))
    distinct = sorted(distinct)
    spans = distinct + distinct[:96]            # 96 spans occur twice
    rnd.shuffle(spans)
    data, starts, lens = b"", [], []
    for s in spans:
        data += b"x" * rnd.randint(0, 3)        # spans lie back to back or apart, at any alignment
        starts.append(len(data))
        lens.append(len(s))
        data += s
    weights = [rnd.randint(1, 1000) for _ in spans]
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    dev = buf.device
    us, ul, uc, up = grep.aggregate(buf, torch.tensor(starts, dtype=torch.int32, device=dev),
                                    torch.tensor(lens, dtype=torch.int32, device=dev),
                                    torch.tensor(weights, device=dev), 3)
    want = collections.Counter()
    for s, n in zip(spans, weights):
        want[s] += n
    got = _got(data, us, ul, uc)
    assert len(got) == us.numel() == GROUP - 96 and got == dict(want)
    assert up.tolist() == [text.partition_of(data[s:s + n], 3)
                           for s, n in zip(us.tolist(), ul.tolist())]


def _seq(path, key_class, compression="NONE"):
    with seqf.Writer(str(path), key_class, BytesWritable, compression=compression) as w:
        w.append(key_class(1) if key_class is IntWritable else key_class(b"k"), BytesWritable(b"v"))
    return str(path)


def test_file_reasons_and_gpu_fallback_warning(tmp_path, caplog):
    from hbmr.examples._gpu import run_gpu_job
    from hbmr.models import records
    ok = _seq(tmp_path / "ok.seq", Text)
    seen = set()
    assert records.file_reason(ok, seen) is None
    assert seen == {("org.apache.hadoop.io.Text", "org.apache.hadoop.io.BytesWritable")}
    comp = _seq(tmp_path / "comp.seq", Text, "RECORD")
    assert records.file_reason(comp, seen) == f"RECORD-compressed input {comp}"
    ints = _seq(tmp_path / "int.seq", IntWritable)
    assert records.file_reason(ints, seen) == (
        f"key class org.apache.hadoop.io.IntWritable of {ints} (byte-string keys only: "
        "BytesWritable, Text)")
    sub = tmp_path / "dir"
    sub.mkdir()
    assert records.file_reason(str(sub), seen) == f"input {sub} is not a local file"
    assert len(seen) == 1

    def build():
        raise ValueError("sort of 'in' is not eligible for the GPU: compressed output")
    log = logging.getLogger("hbmr.examples.sort")
    with caplog.at_level(logging.WARNING, logger=log.name):
        assert run_gpu_job(build, "sort", None, None, log) is None
    assert [(r.name, r.levelname, r.getMessage()) for r in caplog.records] == [
        ("hbmr.examples.sort", "WARNING", "sort of 'in' is not eligible for the GPU: "
         "compressed output; running the classic sort job")]
