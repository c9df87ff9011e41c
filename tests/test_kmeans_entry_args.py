"""Argument checks of the K-Means C entry points that pick a kernel by ``dp``
(the padded row width: 64, 128 or 256): a width with no kernel is refused with
the entry's documented error code before anything is launched or written.

Every ``hbmr_kmeans_*`` entry that dispatches on ``dp`` is called with
``dp = 96``, and those that serve only ``dp <= 128`` also with ``dp = 256``;
all other arguments are valid and tiny (n = 33, k = 3, d = 8, k_pad = 64, one
split).  The entries that take ``dp`` only as a row stride
(hbmr_kmeans_exact_prep, hbmr_kmeans_image16, hbmr_kmeans_update) accept any
multiple of 8 and are not part of this.  The combiners are called in their
automatic mode, where k = 3 takes the LDS path whose first act is the width
dispatch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID = 1           # hipErrorInvalidValue
NOT_SUPPORTED = 801   # hipErrorNotSupported

N, K, D, K_PAD = 33, 3, 8, 64
MAX_DP = 256
SENTINEL = 0xA5


class _Pool:
    """Device buffers carved from one sentinel-filled allocation, so one
    comparison shows that a call wrote to none of them."""

    def __init__(self, nbytes=1 << 20):
        self.mem = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.mem.data_ptr() % 256 == 0
        self.used = 0

    def buf(self, nbytes):
        p = self.mem.data_ptr() + self.used
        self.used += (nbytes + 255) & ~255
        assert self.used <= self.mem.numel()
        return p

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.mem == SENTINEL).all())


def _one(ptr):
    return (ctypes.c_void_p * 1)(ptr)


@pytest.fixture(scope="module")
def env():
    from hbmr.ops import _lib
    lib = _lib.load()
    p = _Pool()
    ns = (ctypes.c_long * 1)(N)
    a = dict(
        lib=lib, pool=p, ns=ns,
        X=p.buf(N * MAX_DP * 4), C=p.buf(K_PAD * MAX_DP * 2), Ct=p.buf(K_PAD * MAX_DP * 2),
        chalf=p.buf(K_PAD * 4), labels=p.buf(N * 4), cand=p.buf(2 * N * 4),
        scores=p.buf(N * 4), margin=p.buf(2 * N * 4),
        sums=p.buf(K * MAX_DP * 8), counts=p.buf(K * 8),
        xnorm=p.buf(N * 4), xbn2=p.buf(N * 4), xerr=p.buf(N * 4),
        cnorm=p.buf(K * 4), cerr=p.buf(K * 4), maxima=p.buf(8), dcc=p.buf(K * 4),
        g=p.buf(N * 4), gap=p.buf(N * 4), cen=p.buf(K * D * 4), skipped=p.buf(8),
        S0=p.buf(K * MAX_DP * 8), N0=p.buf(K * 8),
    )
    a["ws_bytes"] = max(lib.hbmr_kmeans_refine_batch_bytes(1, ns),
                        lib.hbmr_kmeans_batch_workspace_bytes(N, 1, K),
                        lib.hbmr_kmeans_delta_workspace_bytes(N, 1, K))
    a["bws_bytes"] = lib.hbmr_kmeans_bound_workspace_bytes(N, 1, K)
    assert a["ws_bytes"] > 0 and a["bws_bytes"] > 0
    a["ws"] = p.buf(a["ws_bytes"])
    a["bws"] = p.buf(a["bws_bytes"])
    return a


def _assign(a, dp):
    return a["lib"].hbmr_kmeans_assign_bf16(a["X"], N, dp, a["C"], a["chalf"], K_PAD,
                                            a["labels"], a["scores"], None)


def _accum(name):
    def call(a, dp):
        return getattr(a["lib"], name)(a["X"], N, dp, a["labels"], K, a["sums"], a["counts"], 20,
                                       None, 0, 0, None)
    return call


def _top3(name):
    def call(a, dp):
        return getattr(a["lib"], name)(a["X"], N, dp, a["C"], a["chalf"], K_PAD, a["labels"],
                                       a["cand"], a["scores"], a["margin"], None)
    return call


def _image16_tiled(a, dp):
    return a["lib"].hbmr_kmeans_image16_tiled(a["C"], K_PAD, dp, a["Ct"], None)


def _top3_grouped(f16):
    def call(a, dp):
        return a["lib"].hbmr_kmeans_assign_top3_grouped(
            1, _one(a["X"]), a["ns"], dp, f16, a["C"], a["chalf"], K_PAD, a["labels"],
            a["cand"], a["scores"], a["margin"], None)
    return call


def _q1_grouped(a, dp):
    return a["lib"].hbmr_kmeans_assign_top3_q1_grouped(
        1, _one(a["X"]), a["ns"], dp, 1, a["C"], a["Ct"], a["chalf"], K_PAD, a["labels"],
        _one(a["xnorm"]), _one(a["xbn2"]), _one(a["xerr"]), D, K, a["cnorm"], a["maxima"],
        a["cerr"], a["maxima"] + 4, a["ws"], a["ws_bytes"], a["dcc"], None)


def _q1_bounded(a, dp):
    return a["lib"].hbmr_kmeans_assign_top3_q1_bounded(
        1, _one(a["X"]), a["ns"], dp, 1, a["Ct"], a["chalf"], K_PAD, a["labels"],
        _one(a["xnorm"]), _one(a["xbn2"]), _one(a["xerr"]), D, K, a["cnorm"], a["maxima"],
        a["cerr"], a["maxima"] + 4, a["ws"], a["ws_bytes"], a["dcc"], _one(a["g"]),
        _one(a["gap"]), _one(None), a["cen"], a["bws"], a["bws_bytes"], a["skipped"], None)


def _map_batch(a, dp):
    return a["lib"].hbmr_kmeans_map_batch(
        1, _one(a["X"]), a["ns"], dp, a["C"], a["chalf"], K_PAD, K, a["labels"], a["ws"],
        a["ws_bytes"], a["sums"], a["counts"], 20, 0, None)


def _delta_combine(x_f32):
    def call(a, dp):
        return a["lib"].hbmr_kmeans_delta_combine(
            1, _one(a["X"]), a["ns"], dp, x_f32, K, a["labels"], a["ws"], a["ws_bytes"],
            a["sums"], a["counts"], 20, _one(a["g"]), _one(a["S0"]), _one(a["N0"]), None)
    return call


def _map_batch_delta(a, dp):
    return a["lib"].hbmr_kmeans_map_batch_delta(
        1, _one(a["X"]), a["ns"], dp, a["C"], a["chalf"], K_PAD, K, a["labels"], a["ws"],
        a["ws_bytes"], a["sums"], a["counts"], 20, _one(a["g"]), _one(a["S0"]), _one(a["N0"]),
        None)


CASES = [
    ("assign_bf16", _assign, 96, INVALID),
    ("accum_bf16", _accum("hbmr_kmeans_accum_bf16"), 96, INVALID),
    ("accum_f32", _accum("hbmr_kmeans_accum_f32"), 96, INVALID),
    ("assign_top3_bf16", _top3("hbmr_kmeans_assign_top3_bf16"), 96, INVALID),
    ("assign_top3_f16", _top3("hbmr_kmeans_assign_top3_f16"), 96, INVALID),
    ("image16_tiled", _image16_tiled, 96, INVALID),
    ("image16_tiled", _image16_tiled, 256, INVALID),
    ("assign_top3_grouped_bf16", _top3_grouped(0), 96, INVALID),
    ("assign_top3_grouped_f16", _top3_grouped(1), 96, INVALID),
    ("assign_top3_grouped_bf16", _top3_grouped(0), 256, NOT_SUPPORTED),
    ("assign_top3_grouped_f16", _top3_grouped(1), 256, NOT_SUPPORTED),
    ("assign_top3_q1_grouped", _q1_grouped, 96, INVALID),
    ("assign_top3_q1_grouped", _q1_grouped, 256, INVALID),
    ("assign_top3_q1_bounded", _q1_bounded, 96, INVALID),
    ("assign_top3_q1_bounded", _q1_bounded, 256, INVALID),
    ("map_batch", _map_batch, 96, INVALID),
    ("delta_combine_bf16", _delta_combine(0), 96, INVALID),
    ("delta_combine_f32", _delta_combine(1), 96, INVALID),
    ("map_batch_delta", _map_batch_delta, 96, INVALID),
]


@pytest.mark.parametrize("name,call,dp,code", CASES,
                         ids=[f"{c[0]}-dp{c[2]}" for c in CASES])
def test_bad_dp_is_refused_before_any_write(env, name, call, dp, code):
    assert call(env, dp) == code
    assert env["pool"].untouched()
