"""GPU Pentomino: the exact-cover twin against the classic solver, the C++
counter and the HIP kernels against the twin, and the split job against the
classic job's output."""
import importlib.util
import logging
import os
import subprocess

import numpy as np
import pytest
import torch

from hbmr.examples import dancing
from hbmr.examples.dancing import OneSidedPentomino, Pentomino
from hbmr.mapred import JobConf
from hbmr.mapred.cluster import LocalCluster
from hbmr.models import pentomino as pent_job
from hbmr.ops import exactcover as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_GROUP = "org.apache.hadoop.mapred.JobInProgress$Counter"
SIZES = [0, 1, 2, 63, 64, 65, 257]


class Board:
    """One board's table, its ``split(2)`` prefixes and the twin's count for
    each: made once, read by every test that needs them."""

    def __init__(self, width, height):
        self.p = Pentomino(width, height)
        self.tab = E.table(self.p)
        self.prefixes = self.p.split(2)
        self.nodes = [0]
        self.counts = E.count(self.tab, self.prefixes, self.nodes)
        self.counts.setflags(write=False)
        # the twin's levels below the prefixes, down to one of 257 states or more
        self.levels = [E.states(self.tab, self.prefixes)]
        while len(self.levels[-1]) < 257:
            self.levels.append(E.expand(self.tab, self.levels[-1]))


@pytest.fixture(scope="module")
def b3x20():
    return Board(20, 3)


@pytest.fixture(scope="module")
def b4x15():
    return Board(15, 4)


@pytest.fixture(scope="module")
def boards(b3x20, b4x15):
    return {"3x20": b3x20, "4x15": b4x15}


@pytest.fixture(scope="module")
def onesided():
    """One-sided 3×30 with the first 64 prefixes of ``split(4)`` and the C++
    counter's count for each."""
    p = OneSidedPentomino(30, 3)
    tab = E.table(p)
    prefixes = p.split(4)[:64]
    return p, tab, prefixes, E.count_cpu(tab, prefixes)


# ----------------------------------------------------------------------------- CPU
def test_twin_totals(b3x20, b4x15):
    assert len(b3x20.prefixes) == 85 and int(b3x20.counts.sum()) == 4
    assert len(b4x15.prefixes) == 65 and int(b4x15.counts.sum()) == 402
    assert E.count(b3x20.tab, [[]]).tolist() == [4]


def test_twin_per_prefix_equals_classic_solver(b3x20):
    want = [b3x20.p.solve(prefix=pre) for pre in b3x20.prefixes]
    assert b3x20.counts.tolist() == want and sum(want) == 4


def test_cells_are_numbered_along_the_shorter_side(b3x20):
    """The whole 3×20 search makes 68 thousand placements with cells numbered
    along the short side (numbered along the long side it does not finish in
    minutes); the bound is that figure rounded up to the next hundred thousand."""
    tab = b3x20.tab
    assert (tab.bit(1, 0), tab.bit(0, 1)) == (1, 3)
    tall = E.table(Pentomino(3, 20))
    assert (tall.bit(0, 1), tall.bit(1, 0)) == (1, 3)
    nodes = [0]
    assert E.count(tab, [[]], nodes).tolist() == [4]
    print("placements, 3x20 from the empty board:", nodes[0])
    assert 0 < nodes[0] <= 100_000
    nodes = [0]
    assert E.count_cpu(tall, [[]], nodes=nodes).tolist() == [4] and nodes[0] <= 100_000


def test_prefix_edge_cases(b3x20):
    tab = b3x20.tab
    covers = b3x20.p.split(12)                 # a 12-row prefix is a whole tiling
    assert len(covers) == 4
    dead = b3x20.prefixes[int(np.flatnonzero(b3x20.counts == 0)[0])]
    for fn in (E.count, E.count_cpu):
        assert fn(tab, [covers[0]]).tolist() == [1]
        assert fn(tab, [dead]).tolist() == [0]
        assert fn(tab, [covers[1], dead, covers[2]]).tolist() == [1, 0, 1]
        assert fn(tab, []).tolist() == []
    with pytest.raises(ValueError, match="meets an earlier row"):
        E.states(tab, [[covers[0][0], covers[0][0]]])


def test_cpp_counter_equals_twin(b3x20, b4x15):
    for b in (b3x20, b4x15):
        for threads in (1, 4):
            nodes = [0]
            got = E.count_cpu(b.tab, b.prefixes, threads=threads, nodes=nodes)
            assert got.tolist() == b.counts.tolist()
            assert nodes[0] == b.nodes[0]
        # the same counts from the states one and two levels further down
        for level in b.levels[1:3]:
            assert E.count_states_cpu(b.tab, level, len(b.prefixes)).tolist() == b.counts.tolist()
    few = b4x15.levels[1][:40]
    assert (E.count_states_cpu(b4x15.tab, few, 65).tolist() ==
            E.count_states(b4x15.tab, few, 65).tolist())


def test_boards_with_the_wrong_cell_count_give_zero():
    for p in (Pentomino(10, 5), Pentomino(7, 9), OneSidedPentomino(10, 6)):
        tab = E.table(p)
        assert not tab.solvable
        pre = p.split(1)[:3]
        assert len(pre) == 3
        assert E.count(tab, pre).tolist() == [0, 0, 0]
        assert E.count_cpu(tab, pre).tolist() == [0, 0, 0]


ONESIDED_SUBSET = [i for i in range(32) if i not in (11, 17)] + [222, 282]


def test_onesided_twin_equals_classic_solver():
    """32 prefixes of ``split(4)`` on 3×30, fixed: the first 32, with the two
    the classic solver is slowest on (11 and 17, over 5 s each here, of 24 s
    for the 32) swapped for 222 and 282, which have completions and take about
    a second each.  Six of the 32 have completions (3, 7, 13, 14, 222, 282);
    the classic solver takes about 14 s over them here."""
    p = OneSidedPentomino(30, 3)
    tab = E.table(p)
    assert len(p.names) == 18 and tab.words == 2 and tab.ncells == 90
    prefixes = p.split(4)
    sub = [prefixes[i] for i in ONESIDED_SUBSET]
    assert len(sub) == 32
    got = E.count(tab, sub)
    assert got.tolist() == [p.solve(prefix=pre) for pre in sub]
    assert int((got > 0).sum()) == 6
    assert E.count_cpu(tab, sub).tolist() == got.tolist()


def test_onesided_pieces():
    names = sorted(OneSidedPentomino.pieces)
    assert len(names) == 18 and [n for n in names if n.endswith("'")] == [
        "F'", "L'", "N'", "P'", "Y'", "Z'"]
    for n in "FLNPYZ":
        a = dancing._orientations(OneSidedPentomino.pieces[n], fixed=True)
        b = dancing._orientations(OneSidedPentomino.pieces[n + "'"], fixed=True)
        assert len(a) == len(b) and not set(a) & set(b)
        assert sorted(a + b) == dancing._orientations(dancing._PIECES[n])
    for n in "ITUVWX":                         # their mirror image is a rotation
        assert (dancing._orientations(dancing._PIECES[n], fixed=True) ==
                dancing._orientations(dancing._PIECES[n]))


def _native_build():
    spec = importlib.util.spec_from_file_location("hbmr_native_build",
                                                  os.path.join(ROOT, "native", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cpp_counter_stand_alone_under_asan_ubsan(tmp_path, b3x20):
    """native/tests/exactcover_selftest.cc, a program of its own with the
    counter compiled in under -fsanitize=address,undefined, on the 3×20 table."""
    exe = _native_build().build_sanitized("asan")["exactcover_selftest"]
    path = str(tmp_path / "3x20.table")
    E.dump(b3x20.tab, b3x20.levels[1], len(b3x20.prefixes), path)
    for threads in ("1", "3"):
        r = subprocess.run([exe, path, threads], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        lines = r.stdout.split("\n")
        assert [int(x) for x in lines[:85]] == b3x20.counts.tolist()
        assert lines[85].startswith("nodes ")


def _part(out):
    assert os.path.exists(os.path.join(out, "_SUCCESS"))
    assert not os.path.exists(os.path.join(out, "_temporary"))
    names = sorted(f for f in os.listdir(out) if f.startswith("part-"))
    assert names == ["part-00000"]
    return open(os.path.join(out, names[0]), "rb").read()


def test_gpu_flag_on_cpu_slots_writes_the_classic_part(tmp_path, capsys):
    classic, gpu = str(tmp_path / "c"), str(tmp_path / "g")
    with LocalCluster(JobConf(), num_trackers=2, cpu_slots=2) as cl:
        assert dancing.distributed_pentomino(classic, 20, 3, 2, cluster=cl) == 4
        assert dancing.main_pentomino([gpu, "-width", "20", "-height", "3", "-gpu"],
                                      cluster=cl) == 0
        assert "4 solutions" in capsys.readouterr().out
        assert dancing.run_pentomino(str(tmp_path / "m"), 20, 3, maps=7, cluster=cl,
                                     gpu=True) == 4
        assert dancing.run_pentomino(str(tmp_path / "o"), 30, 3, onesided=True, maps=3,
                                     cluster=cl, gpu=True) == 92
    want = open(os.path.join(classic, "part-00000"), "rb").read()
    assert want == b"solutions\t4\n"
    assert _part(gpu) == want and _part(str(tmp_path / "m")) == want
    assert _part(str(tmp_path / "o")) == b"solutions\t92\n"


def test_job_shape_and_ineligible_output(tmp_path, caplog):
    job = pent_job.gpu_job(str(tmp_path / "a"), 20, 3)
    assert job.get_num_map_tasks() == pent_job.classic_maps(85) == 17
    splits = pent_job.PentominoSplitJob()
    splits.configure(job)
    ranges = [(s.params["lo"], s.params["hi"]) for s in splits.get_splits(job, [])]
    assert len(ranges) == 17 and ranges[0][0] == 0 and ranges[-1][1] == 85
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert pent_job.gpu_job(str(tmp_path / "b"), 20, 3, maps=500).get_num_map_tasks() == 500
    job = pent_job.gpu_job(str(tmp_path / "b"), 20, 3, maps=500)
    splits.configure(job)
    assert len(splits.get_splits(job, [])) == 85            # never an empty map
    with pytest.raises(ValueError, match="not a local one"):
        pent_job.gpu_job("hdfs://namenode:8020/out", 20, 3)
    base = JobConf()
    base.set_boolean("mapred.output.compress", True)
    with pytest.raises(ValueError, match="compressed output"):
        pent_job.gpu_job(str(tmp_path / "c"), 20, 3, base=base)
    with pytest.raises(ValueError, match="128-bit"):
        pent_job.gpu_job(str(tmp_path / "d"), 13, 10)
    # `pentomino -gpu` on such a job is the classic job, and says why
    local = JobConf()
    local.set("mapred.job.tracker", "local")
    local.set_boolean("mapred.output.compress", True)
    seen = {}

    def classic(out, *a, **kw):
        seen["out"] = out
        return 4
    real = dancing.distributed_pentomino
    dancing.distributed_pentomino = classic
    try:
        with caplog.at_level(logging.WARNING, logger="hbmr.examples.pentomino"):
            assert dancing.run_pentomino(str(tmp_path / "e"), 20, 3, conf=local, gpu=True) == 4
    finally:
        dancing.distributed_pentomino = real
    assert seen["out"] == str(tmp_path / "e")
    assert "compressed output" in caplog.text and "classic pentomino job" in caplog.text


# ----------------------------------------------------------------------------- GPU
def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _rows(words, tab):
    """The states as a sorted list of tuples (a multiset)."""
    w = np.asarray(words.cpu().numpy() if hasattr(words, "cpu") else words)
    return sorted(map(tuple, w.view(np.uint64).reshape(-1, tab.words + 1).tolist()))


def _full_state(tab, src):
    return E._pack(tab, [(tab.full, (1 << tab.npieces) - 1, src)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3x20", "4x15"])
def test_gpu_expand_equals_twin_level_by_level(boards, name):
    b = boards[name]
    tab = b.tab
    longest = int(np.diff(tab.off).max())
    level = b.levels[-1]                       # 257 states or more
    assert len(level) >= 257
    for n in SIZES:
        words = level[:n]
        if n >= 2:                             # a whole tiling among them, not last
            words = np.concatenate([words[:1], _full_state(tab, 5), words[1:n - 1]])
        # two levels in a row: the device's children feed the next level
        for _ in range(2):
            want = E.expand(tab, words)
            parts = list(E.expand_gpu(tab, _dev(words)))
            got = torch.cat(parts) if parts else torch.empty((0, tab.words + 1),
                                                             dtype=torch.int64)
            assert _rows(got, tab) == _rows(want, tab), (name, n)
            # in the twin's order too, not only as a set
            assert np.array_equal(got.cpu().numpy().view(np.uint64).reshape(want.shape), want)
            words = want
        if n >= 2:
            assert tuple(_full_state(tab, 5)[0].tolist()) in _rows(want, tab)
    # states without children, and every state childless
    nchild = [len(E.expand(tab, level[i:i + 1])) for i in range(257)]
    assert 0 in nchild and max(nchild) > 0
    barren = level[:257][np.array(nchild) == 0]
    assert list(E.expand_gpu(tab, _dev(barren))) == []
    # a capacity that cuts the level: parts no longer than it, nothing lost
    words = level[:257]
    want = E.expand(tab, words)
    assert len(want) > 2 * longest
    parts = list(E.expand_gpu(tab, _dev(words), capacity=longest))
    assert len(parts) > 2 and max(int(p.shape[0]) for p in parts) <= longest
    assert np.array_equal(torch.cat(parts).cpu().numpy().view(np.uint64), want)
    with pytest.raises(ValueError, match="longest bucket"):
        list(E.expand_gpu(tab, _dev(words), capacity=longest - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3x20", "4x15"])
def test_gpu_count_equals_twin(boards, name):
    b = boards[name]
    tab, want = b.tab, b.counts.tolist()
    for levels in (0, 1, E.DEFAULT_LEVELS):
        assert E.count_gpu(tab, b.prefixes, levels=levels).cpu().tolist() == want, levels
    # a capacity that cuts the levels into chunks: the second level has over 6,000 states
    launches = []
    got = E.count_gpu(tab, b.prefixes, levels=2, capacity=1024,
                      on_launch=lambda *a: launches.append(a))
    assert got.cpu().tolist() == want
    assert sum(k == "count" for k, _, _ in launches) > 4
    assert max(n for _, _, n in launches) <= 1024
    assert E.count_gpu(tab, []).shape == (0,)
    one = int(np.flatnonzero(b.counts)[0])
    assert E.count_gpu(tab, [b.prefixes[one]]).cpu().tolist() == [want[one]]
    assert E.count_gpu(tab, [[]]).cpu().tolist() == [sum(want)]          # the whole board
    assert E.count_gpu(tab, [[]], levels=0).cpu().tolist() == [sum(want)]
    # the count kernel alone on states that are whole tilings or dead
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    words = np.concatenate([_full_state(tab, 2), b.levels[0][:1] | np.uint64(0),
                            _full_state(tab, 0), _full_state(tab, 2)])
    words[1, tab.words] = (words[1, tab.words] & np.uint64(0xFFFFFFFF)) | np.uint64(1 << 32)
    E.count_states_gpu(tab, _dev(words), counts)
    assert counts.cpu().tolist() == [1, want[0], 2]


@pytest.mark.gpu
def test_gpu_count_more_states_than_resident_lanes():
    """Over 600,000 states for the 262,144 lanes (256 CUs × 1024; 16,384
    groups of 16 lanes, a state each) that hold the table at once, so every
    group comes back to the work counter many times.
    No level of 3×20 or 4×15 is that wide (4×15 peaks at 59,873 states below
    its ``split(2)`` prefixes), so the board is 6×10; there the twin would take
    most of a minute, and the reference is the C++ counter, which the CPU tests
    hold equal to the twin."""
    p = Pentomino(10, 6)
    tab, prefixes = E.table(p), p.split(2)
    want = E.count_cpu(tab, prefixes, threads=4)
    assert int(want.sum()) == 2339
    words = _dev(E.states(tab, prefixes))
    while words.shape[0] < 600_000:
        words = torch.cat(list(E.expand_gpu(tab, words, capacity=1 << 22)))
    assert words.shape[0] > 2 * 262_144
    counts = torch.zeros(len(prefixes), dtype=torch.int64, device="cuda")
    scratch = torch.zeros(2, dtype=torch.int64, device="cuda")
    E.count_states_gpu(tab, words, counts, scratch)
    assert counts.cpu().tolist() == want.tolist()
    fetched, placed = scratch.cpu().tolist()
    assert fetched >= words.shape[0] and placed > 0
    assert E.count_gpu(tab, prefixes).cpu().tolist() == want.tolist()


@pytest.mark.gpu
def test_gpu_128_bit_masks(onesided, boards):
    p, tab, prefixes, cpp = onesided
    want = E.count(tab, prefixes).tolist()
    assert want == cpp.tolist() and sum(want) > 0
    for levels in (0, 2):
        assert E.count_gpu(tab, prefixes, levels=levels).cpu().tolist() == want
    level = E.expand(tab, E.states(tab, prefixes))
    got = torch.cat(list(E.expand_gpu(tab, _dev(level), capacity=64)))
    assert np.array_equal(got.cpu().numpy().view(np.uint64), E.expand(tab, level))
    # a 60-cell table through the two-word kernels counts what the one-word ones count
    for b in boards.values():
        wide = b.tab.widened()
        assert wide.words == 2 and b.tab.words == 1
        assert E.count_gpu(wide, b.prefixes).cpu().tolist() == b.counts.tolist()
        assert E.count_cpu(wide, b.prefixes).tolist() == b.counts.tolist()


@pytest.mark.gpu
def test_gpu_wrong_cell_count_launches_nothing():
    p = Pentomino(10, 5)
    launches = []
    got = E.count_gpu(E.table(p), p.split(1)[:3], on_launch=lambda *a: launches.append(a))
    assert got.cpu().tolist() == [0, 0, 0] and launches == []


@pytest.mark.gpu
@pytest.mark.parametrize("cpu_slots", [0, 2])
def test_gpu_pentomino_job_writes_the_classic_part(tmp_path, cpu_slots):
    conf = JobConf()
    if not cpu_slots:
        conf.set_int("mapred.tasktracker.map.cpu.tasks.maximum", 0)
    with LocalCluster(conf, num_trackers=1, gpus=[[0]], cpu_slots=cpu_slots) as cl:
        for (w, h), total in (((20, 3), 4), ((15, 4), 402)):
            for maps in (None, 1, 7):
                out = str(tmp_path / f"{w}x{h}-{maps}")
                rj = cl.submit_job(pent_job.gpu_job(out, w, h, maps=maps))
                assert rj.waitForCompletion(120) and rj.isSuccessful(), rj.getFailureInfo()
                assert rj._impl.jip.result[0]["solutions"] == total
                assert _part(out) == b"solutions\t%d\n" % total
                cs = rj.getCounters()
                gpu_maps = cs.get(JOB_GROUP, "GPU_MAP_TASKS")
                assert gpu_maps + cs.get(JOB_GROUP, "CPU_MAP_TASKS") == (maps or 17)
                if not cpu_slots:              # mixed: the scheduler places each map
                    assert gpu_maps == (maps or 17)
        out = str(tmp_path / "cli")
        assert dancing.main_pentomino([out, "-width", "15", "-height", "4", "-m", "3", "-gpu"],
                                      cluster=cl) == 0
        assert _part(out) == b"solutions\t402\n"
