"""hbmr/models/splits.py: what the split-level jobs share above the kernels.

The job tests compare each job's parts, counters and refusals with the classic
job; these check the shared functions on their own, against their definitions.
"""
import itertools
import os

import pytest
import torch

from hbmr.io import sequencefile as seqf
from hbmr.io.writable import BytesWritable
from hbmr.mapred import FileInputFormat, JobConf
from hbmr.models import grep, secondarysort, sort, sortvalidate, splits, wordcount, wordtable


# ----------------------------------------------------------------------------- ownership
@pytest.mark.parametrize("world", range(1, 10))
def test_owned_ranges_tile_the_partitions_by_the_rule(world):
    for nparts in range(1, 21):
        ranges = [splits.owned(r, world, nparts) for r in range(world)]
        taken = [rg for rg in ranges if rg != (0, 0)]
        # contiguous, disjoint, covering [0, R): each begins where the last ended
        assert taken[0][0] == 0 and taken[-1][1] == nparts
        assert all(a[1] == b[0] for a, b in zip(taken, taken[1:]))
        assert all(lo < hi for lo, hi in taken)
        for r, (lo, hi) in enumerate(ranges):
            for p in range(nparts):
                assert (lo <= p < hi) == (p * world // nparts == r)
                assert splits.owner_of(p, world, nparts) == p * world // nparts
        assert (len(taken) < world) == (world > nparts)


# ----------------------------------------------------------------------------- regrouping
NPARTS = 5
FIELDS = [splits.Field("a", "na", torch.uint8), splits.Field("b", "nb", torch.int64, (3,))]


def _outputs():
    """Three map outputs: ``a`` uint8[sum na], ``b`` int64[sum nb, 3], every
    element distinct, the two count lists different (zeros among them)."""
    counts = [([2, 0, 3, 1, 4], [1, 2, 0, 0, 3]), ([0, 0, 5, 0, 1], [4, 1, 1, 2, 0]),
              ([1, 1, 1, 1, 1], [0, 0, 0, 6, 0])]
    outs, a0, b0 = [], 0, 0
    for na, nb in counts:
        a = torch.arange(a0, a0 + sum(na), dtype=torch.uint8)
        b = torch.arange(b0, b0 + 3 * sum(nb), dtype=torch.int64).reshape(-1, 3)
        outs.append({"a": a, "na": na, "b": b, "nb": nb})
        a0, b0 = a0 + sum(na), b0 + 3 * sum(nb)
    return outs


@pytest.mark.parametrize("world", [1, 2, 3, 7])
def test_by_destination_equals_its_definition(world):
    outs = _outputs()
    got = splits.by_destination(outs, world, NPARTS, FIELDS, torch.device("cpu"))
    assert len(got) == len(FIELDS)
    for f, (t, send) in zip(FIELDS, got):
        pieces, want_send = [], []
        for j in range(world):
            owned = [p for p in range(NPARTS) if p * world // NPARTS == j]
            n = 0
            for o in outs:
                prefix = [0] + list(itertools.accumulate(o[f.counts]))
                lo, hi = (prefix[owned[0]], prefix[owned[-1] + 1]) if owned else (0, 0)
                pieces.append(o[f.tensor][lo:hi])
                n += hi - lo
            want_send.append(n)
        assert send == want_send
        assert sum(send) == sum(sum(o[f.counts]) for o in outs) == t.shape[0]
        assert t.dtype == f.dtype and torch.equal(t, torch.cat(pieces))
    if world == 7:
        assert got[0][1].count(0) >= 2       # ranks that own nothing get nothing


def test_by_destination_without_outputs_gives_typed_empties():
    (a, na), (b, nb) = splits.by_destination([], 3, NPARTS, FIELDS, torch.device("cpu"))
    assert a.dtype == torch.uint8 and tuple(a.shape) == (0,)
    assert b.dtype == torch.int64 and tuple(b.shape) == (0, 3)
    assert na == nb == [0, 0, 0]


# ----------------------------------------------------------------------------- keys
def _conf(*paths):
    conf = JobConf()
    FileInputFormat.setInputPaths(conf, *paths)
    conf.set_num_map_tasks(1)
    return conf


def test_whole_file_key_is_sorts_and_the_validators(tmp_path):
    path = str(tmp_path / "part-00000")
    with seqf.Writer(path, BytesWritable, BytesWritable) as w:
        for i in range(20):
            w.append(BytesWritable(b"k%02d" % i), BytesWritable(b"v" * i))
    key = splits.whole_file_key(path, os.path.getsize(path))
    assert [s.key for s in sort.SortSplitJob().get_splits(_conf(path), [])] == [key]
    assert [s.key for s in sortvalidate.ValidateSplitJob().get_splits(_conf(path), [])] == [key]


def test_text_jobs_give_a_file_one_key(tmp_path):
    path = str(tmp_path / "in.txt")
    with open(path, "wb") as f:
        f.write(b"1 2\n3 4\n" * 50)
    conf = _conf(path)
    conf.set(wordtable.PROGRAM_KEY, "wordcount")
    keys = [[s.key for s in cls().get_splits(conf, ["t0", "t1"])]
            for cls in (grep.GrepSplitJob, secondarysort.SecondarySortSplitJob,
                        wordcount.WordCountSplitJob, wordtable.WordTableSplitJob)]
    assert keys[0] == [splits.text_key(path, 0, os.path.getsize(path))]
    assert all(k == keys[0] for k in keys)


# ----------------------------------------------------------------------------- decoded bytes
class _Reporter:
    def __init__(self):
        self.counts = {}

    def incrCounter(self, group, name, n):
        self.counts[group, name] = self.counts.get((group, name), 0) + n


class _Ctx:
    def __init__(self, key, reporter):
        self.spec = type("Spec", (), {"split": {"key": key}})()
        self.reporter = reporter


def test_decoded_note_is_counted_once_by_its_own_map():
    job, rep = wordcount.WordCountSplitJob(), _Reporter()
    counter = (splits.COMPRESSED_INPUT_GROUP, splits.SNAPPY_DECODED_BYTES)
    splits.note_decoded(job, "k1", 700)
    splits.note_decoded(job, "k2", 11)
    splits.count_snappy_decoded(job, _Ctx("k1", rep))
    assert rep.counts == {counter: 700}
    splits.count_snappy_decoded(job, _Ctx("k1", rep))      # the split found resident
    assert rep.counts == {counter: 700}
    splits.count_snappy_decoded(job, _Ctx("k2", rep))      # the other key's note was left alone
    assert rep.counts == {counter: 711}


# ----------------------------------------------------------------------------- eligibility
def test_reason_strings(tmp_path):
    for name in ("a.txt", "b.gz", "c.snappy"):
        (tmp_path / name).write_bytes(b"x\n")
    (tmp_path / "d").mkdir()
    (tmp_path / "d" / "sub").mkdir()
    txt, gz, snappy, sub = (str(tmp_path / n) for n in ("a.txt", "b.gz", "c.snappy", "d/sub"))
    assert splits.text_input_reason([txt, snappy]) is None          # .snappy is taken
    assert splits.text_input_reason(str(tmp_path / "d")) == f"input {sub} is not a local file"
    (tmp_path / "e").mkdir()
    (tmp_path / "e" / "part.txt").write_bytes(b"x\n")
    assert splits.text_input_reason(str(tmp_path / "e")) is None    # a directory: its files
    assert splits.text_input_reason([txt, gz]) == f"compressed input {gz}"
    assert splits.compressed_input_reason(snappy) is None and splits.is_snappy(snappy)

    plain, packed, comma = JobConf(), JobConf(), JobConf()
    packed.set_boolean("mapred.output.compress", True)
    comma.set("mapred.textoutputformat.separator", ",")
    assert splits.text_output_reason(None) is None and splits.text_output_reason(plain) is None
    assert splits.text_output_reason(packed) == "compressed output"
    assert splits.text_output_reason(comma) == "mapred.textoutputformat.separator is not a tab"

    assert splits.local_output_reason(str(tmp_path), plain) is None
    assert splits.local_output_reason("file://" + str(tmp_path), None) is None
    assert splits.local_output_reason(str(tmp_path), packed) == "compressed output"
    assert splits.local_output_reason("hdfs://nn/out", plain) == \
        "output directory hdfs://nn/out is not a local one"
    # the jobs hand the same strings on
    assert secondarysort.why_ineligible([txt, gz], comma) == \
        "mapred.textoutputformat.separator is not a tab"
    assert wordtable.why_ineligible([txt, gz], 1, plain) == f"compressed input {gz}"
