"""The host-side seams of the K-Means ops that nothing else exercises on their
own: the grow-on-demand scratch (``scratch_buf``), the cross-stream ordering
rule of the reference partitions (``order_after``) and the next iteration's
centroid image (``CentroidImage.successor``)."""
import pytest
import torch

from hbmr.ops import kmeans as km


# --------------------------------------------------------------------------- scratch_buf
def test_scratch_buf_keeps_grows_and_honours_the_floor():
    s, floor = {}, 8
    sizes = {}
    for n in (0, 1, floor, floor + 1):
        s.clear()
        sizes[n] = km.scratch_buf(s, "a", n, torch.uint8, "cpu", floor=floor).numel()
    assert sizes == {0: floor, 1: floor, floor: floor, floor + 1: floor + 1}
    assert km.scratch_buf({}, "a", 0, torch.uint8, "cpu").numel() == 0     # no floor

    s = {}
    a = km.scratch_buf(s, "a", floor + 1, torch.int32, "cpu", floor=floor)
    assert a.dtype == torch.int32 and a.numel() == floor + 1 and s["a"] is a
    for n in (0, 1, floor, floor + 1):                  # smaller or equal: the same storage
        assert km.scratch_buf(s, "a", n, torch.int32, "cpu", floor=floor) is a
    b = km.scratch_buf(s, "a", floor + 2, torch.int32, "cpu", floor=floor)
    assert b is not a and b.numel() == floor + 2 and s["a"] is b
    assert b.data_ptr() != a.data_ptr()                 # ``a`` is still alive here


def test_scratch_buf_keys_do_not_alias():
    s = {}
    a = km.scratch_buf(s, "a", 4, torch.float32, "cpu")
    b = km.scratch_buf(s, ("a", 1), 4, torch.float32, "cpu")
    assert a.data_ptr() != b.data_ptr() and set(s) == {"a", ("a", 1)}
    a.fill_(1.0)
    b.fill_(2.0)
    assert a.sum() == 4 and km.scratch_buf(s, "a", 2, torch.float32, "cpu") is a


# --------------------------------------------------------------------------- order_after
class _Rec:
    """A stream, an event or a tensor that only records what is done with it."""

    def __init__(self, name, log, base=None):
        self.name, self.log, self._base = name, log, base

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev.name))

    def record_stream(self, st):
        self.log.append(("record_stream", self.name, st.name))

    def __repr__(self):
        return self.name


@pytest.mark.parametrize("attrs", [("g", "S0", "N0"), ("g", "gap", "ref")])
def test_order_after_waits_and_records_once(attrs):
    log = []
    cur, other, third = (_Rec(n, log) for n in ("cur", "other", "third"))
    ev_other, ev_third, ev_cur = (_Rec(n, log) for n in ("ev_other", "ev_third", "ev_cur"))
    slab_a, slab_b = _Rec("slab_a", log), _Rec("slab_b", log)
    own = _Rec("own", log)                       # an allocation of its own (no base)

    def base(first, second, third_t, event, stream):
        b = km.Baseline(None, None, None, 0, 0)
        for a, t in zip(attrs, (first, second, third_t)):
            setattr(b, a, t)
        b.event, b.stream = event, stream
        return b

    def view(of):
        return _Rec("view", log, base=of)

    bases = [base(view(slab_a), view(slab_b), view(slab_b), ev_other, other),
             base(view(slab_a), view(slab_b), None, ev_other, other),     # same event, a None
             base(view(slab_a), own, view(slab_b), ev_third, third),
             base(view(slab_a), view(slab_b), view(slab_b), ev_cur, cur),    # this stream's
             base(view(slab_a), view(slab_b), view(slab_b), None, None)]     # never installed
    km.order_after(bases, attrs, cur)
    waits = [e for e in log if e[0] == "wait_event"]
    recs = [e for e in log if e[0] == "record_stream"]
    assert waits == [("wait_event", "cur", "ev_other"), ("wait_event", "cur", "ev_third")]
    assert recs == [("record_stream", "slab_a", "cur"), ("record_stream", "slab_b", "cur"),
                    ("record_stream", "own", "cur")]
    assert log == waits + recs                   # every wait before the first record


# --------------------------------------------------------------------------- successor
@pytest.mark.gpu
def test_successor_image_is_a_private_update():
    k, d, fx = 3, 8, km.FX_SHIFT
    g = torch.Generator().manual_seed(5)
    cen = torch.randn(k, d, generator=g)
    old = km.CentroidImage(cen, "cuda")
    assert (old.k_pad, old.dp) == (64, 64)
    old.ready = torch.cuda.Event()
    old.ready.record()
    old16 = old.image16()
    old.neighbors()
    before = [t.clone() for t in (old.cen, old.cbf, old.chalf)]

    # cluster 1 is empty; the others get means exactly representable in fp32
    mean = torch.tensor([[0.5] * d, [0.0] * d, [-1.25] * d], dtype=torch.float64)
    counts = torch.tensor([4, 0, 7], dtype=torch.int64)
    sums = torch.zeros(k, old.dp, dtype=torch.int64)
    sums[:, :d] = (mean * counts[:, None].double() * float(1 << fx)).to(torch.int64)
    new = old.successor(sums.cuda(), counts.cuda())
    torch.cuda.synchronize()

    want = mean.float()
    want[1] = cen[1]
    assert torch.equal(new.cen.cpu(), want)
    for t, b in zip((old.cen, old.cbf, old.chalf), before):
        assert torch.equal(t, b)
    for a, b in ((new.cen, old.cen), (new.cbf, old.cbf), (new.chalf, old.chalf),
                 (new.shift2, old.shift2)):
        assert a.data_ptr() != b.data_ptr()
    assert not hasattr(new, "ready")
    assert new._img16 == {} and new._nbr == {} and new._lock is not old._lock
    new16 = new.image16()
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(new16, old16))
    assert old.image16()[0].data_ptr() == old16[0].data_ptr()     # the old cache stays
