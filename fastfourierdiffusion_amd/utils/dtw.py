"""Dynamic time warping between sets of series on the device (libffd, csrc/ffd_dtw.hip): DTW of paired rows, the k nearest
references of every query under banded DTW, and the six numbers ``sampling.metrics.DTWMetrics`` reports.

A series is (L, C); for a Sakoe-Chiba half-width w the local cost is c(i, j) = sum_ch (a[i,ch] - b[j,ch])^2 and
D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)) over |i - j| <= w, all in fp32; ``dtw2`` = D(L-1, L-1) is a
SQUARED cost (w = 0: the squared Euclidean distance; w >= L - 1: unconstrained DTW).  A copied row reads exactly 0.0 and
``dtw2(a, b) == dtw2(b, a)`` to the bit.  ``window`` is an int, the half-width in samples, or a float in (0, 1], a share
of the length: ceil(window L).  It is clipped to L - 1; a clipped window above ``MAX_WINDOW`` is refused.
Inputs may be (n, L, C) numpy arrays, host tensors or device tensors (host data is uploaded, float64 is rounded to
fp32).  torch holds memory only.  Without libffd.so or a gfx950 device every call raises ``FFDError``: there is no numpy
fallback.  Every pair of a search is computed: no lower-bound pruning, no early abandoning.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from .. import _native as N
from .wasserstein import _work

MAX_WINDOW, MAX_LEN, MAX_CHANNELS, MAX_K = 64, 4096, 64, 32  # include/ffd.h FFD_DTW_MAX_*
# most device scratch the distance block of one search asks for; a smaller block means more launches, never other results
WORK_BUDGET_BYTES = 1 << 30
SCORE_KEYS = ("dtw_nn_distance_mean", "dtw_coverage_distance_mean", "dtw_warp_gain", "dtw_1nn_accuracy_samples",
              "dtw_1nn_accuracy_originals", "dtw_1nn_accuracy")


def resolve_window(window, length: int) -> int:
    """The half-width in samples of ``window`` for series of ``length``, clipped to length - 1."""
    assert not isinstance(window, (bool, np.bool_)), f"window must be an int or a float in (0, 1], got {window!r}"
    if isinstance(window, numbers.Integral):
        assert window >= 0, f"a window in samples must be >= 0, got {window}"
        w = int(window)
    else:
        assert isinstance(window, numbers.Real), f"window must be an int or a float in (0, 1], got {window!r}"
        assert 0.0 < float(window) <= 1.0, f"a window given as a share of the length must lie in (0, 1], got {window}"
        w = math.ceil(round(float(window) * length, 9))  # 0.1 * 190 is 19, not the 20 of 19.000000000000004
    w = min(w, length - 1)
    if w > MAX_WINDOW:
        raise NotImplementedError(f"a window of {w} samples: the library's bands end at {MAX_WINDOW}")
    return w


def _shape3(x, name: str):
    shape = tuple(x.shape)
    assert len(shape) == 3 and min(shape) >= 1, f"{name} must be (n, L, C) with every extent >= 1, got {shape}"
    return shape


def _series(x) -> torch.Tensor:
    """(n, L, C) fp32 contiguous device tensor of a numpy array / host tensor / device tensor."""
    if isinstance(x, torch.Tensor) and x.device.type == "cuda":
        t = x.detach()
    else:
        if not torch.cuda.is_available():
            raise N.FFDError("the DTW metrics need an MI355X (gfx950) device; there is no CPU fallback")
        if isinstance(x, torch.Tensor):
            t = x.detach().to(torch.float32).to("cuda")
        else:
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda")
    return t.to(torch.float32).contiguous()


def _check_limits(L: int, C: int, what: str) -> None:
    if L > MAX_LEN or C > MAX_CHANNELS or L * C > 65536:
        raise NotImplementedError(f"{what}: series of ({L}, {C}) are outside the library's limits "
                                  f"(L <= {MAX_LEN}, C <= {MAX_CHANNELS}, L C <= 65536)")


def dtw_pairs(a, b, window) -> torch.Tensor:
    """``dtw2(a[i], b[i]; window)`` for the paired rows of ``a`` and ``b`` (n, L, C): an (n,) fp32 device tensor."""
    sa, sb = _shape3(a, "a"), _shape3(b, "b")
    assert sa == sb, f"the two sets are {sa} and {sb}"
    n, L, C = sa
    w = resolve_window(window, L)
    _check_limits(L, C, "dtw_pairs")
    ta = _series(a)
    tb = ta if b is a else _series(b)
    out = torch.empty(n, device=ta.device, dtype=torch.float32)
    N.check(N.lib().ffd_dtw_pairs(ta.data_ptr(), tb.data_ptr(), n, L, C, w, out.data_ptr(), N.current_stream_ptr(ta.device)),
            None, "ffd_dtw_pairs")
    return out


def dtw_neighbours(query, reference, window, k: int = 1, exclude_self: bool = False,
                   budget_bytes: int = WORK_BUDGET_BYTES):
    """The ``k`` nearest rows of ``reference`` (nr, L, C) under ``dtw2`` for every row of ``query`` (nq, L, C):
    ``(dist2, index)``, fp32 (nq, k) ascending and int32 (nq, k) device tensors, ties by the lower index.
    ``exclude_self`` skips the pair i == i and needs ``query is reference`` (or the same device buffer)."""
    sq, sr = _shape3(query, "query"), _shape3(reference, "reference")
    assert sq[1:] == sr[1:], f"the two sets hold series of {sq[1:]} and {sr[1:]}"
    (nq, L, C), nr = sq, sr[0]
    w = resolve_window(window, L)
    k = int(k)
    assert 1 <= k <= MAX_K, f"k must lie in [1, {MAX_K}], got {k}"
    assert k <= nr - int(bool(exclude_self)), f"k = {k} neighbours asked of {nr - int(bool(exclude_self))} rows"
    _check_limits(L, C, "dtw_neighbours")
    r = _series(reference)
    q = r if query is reference else _series(query)
    if exclude_self:
        assert q.data_ptr() == r.data_ptr() and q.shape == r.shape, \
            "exclude_self needs the query set to be the reference set itself"
    lib, dev = N.lib(), r.device
    dist2 = torch.empty((nq, k), device=dev, dtype=torch.float32)
    index = torch.empty((nq, k), device=dev, dtype=torch.int32)
    nbytes = lib.ffd_dtw_work_bytes(nq, nr, L, C, w, k, int(budget_bytes))
    if nbytes == 0:
        raise NotImplementedError(f"dtw_neighbours: a shape outside the library's limits ({nq}, {nr}, {L}, {C})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_dtw_search(q.data_ptr(), nq, r.data_ptr(), nr, L, C, w, k, int(bool(exclude_self)), dist2.data_ptr(),
                               index.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None, "ffd_dtw_search")
    return dist2, index


def self_search(y, window) -> torch.Tensor:
    """What ``dtw_scores`` needs of a set alone: each row's squared DTW distance to its nearest other row, (n,) fp32."""
    return dtw_neighbours(y, y, window, 1, exclude_self=True)[0].reshape(-1)


def dtw_scores(original, samples, window, original_self=None) -> dict:
    """The six numbers of ``SCORE_KEYS`` for the originals Y (n, L, C) and the samples X (m, L, C), as Python floats: the
    searches XX and YY (self excluded; ``original_self``: Y's, from ``self_search``, when the caller keeps it), XY and YX
    at ``window``, XY at window 0, all at k = 1, then one scoring kernel.  The sets are used as given: every pair of
    every search is computed and nothing is subsampled, so the cost is (n + m)^2 L (2 w + 1) cells."""
    sy, sx = _shape3(original, "original"), _shape3(samples, "samples")
    assert sy[1:] == sx[1:], f"the originals hold series of {sy[1:]}, the samples of {sx[1:]}"
    n, m = sy[0], sx[0]
    assert n >= 2 and m >= 2, f"both sets need at least 2 rows, got {n} originals and {m} samples"
    w = resolve_window(window, sy[1])
    _check_limits(sy[1], sy[2], "dtw_scores")
    y, x = _series(original), _series(samples)
    yy = original_self if original_self is not None else self_search(y, w)
    xx = self_search(x, w)
    xy = dtw_neighbours(x, y, w)[0].reshape(-1)
    yx = dtw_neighbours(y, x, w)[0].reshape(-1)
    e2 = xy if w == 0 else dtw_neighbours(x, y, 0)[0].reshape(-1)
    out = torch.empty(6, device=y.device, dtype=torch.float64)
    N.check(N.lib().ffd_dtw_scores(xx.data_ptr(), xy.data_ptr(), yx.data_ptr(), yy.data_ptr(), e2.data_ptr(), n, m,
                                   out.data_ptr(), N.current_stream_ptr(y.device)), None, "ffd_dtw_scores")
    return dict(zip(SCORE_KEYS, out.tolist()))
