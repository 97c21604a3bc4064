"""Nearest-neighbour statistics between two row sets on the device (libffd, csrc/ffd_neighbours.hip): k-nearest-neighbour
search, ball counts, and the eight sample-quality numbers ``sampling.metrics.ManifoldMetrics`` reports.

Rows are flat fp32 vectors (n, D) and distances are squared Euclidean.  The pair distances come from the exact-fp32
matrix cores on rows centred on the reference set's mean; the k kept neighbours of a row are recomputed in fp64 in
difference form, so ``dist2`` is the float64 distance of the returned index and a copied row comes out at exactly 0.0.
Inputs may be numpy arrays, host tensors or device tensors (host data is uploaded, float64 is rounded to fp32).  torch
holds memory only.  Without libffd.so or a gfx950 device every call raises ``FFDError``: there is no numpy fallback.
"""
from __future__ import annotations

import torch

from .. import _native as N
from .wasserstein import _work

MAX_K = 32  # include/ffd.h FFD_NN_MAX_K
# most device scratch the distance block of one search asks for; a smaller block means more launches, never other results
WORK_BUDGET_BYTES = 1 << 30
SCORE_KEYS = ("precision", "recall", "density", "coverage", "authenticity", "nn_distance_mean", "nn_distance_min",
              "copy_share")


def _to_device(x) -> torch.Tensor:
    """(n, D) fp32 contiguous device tensor, as ``utils.wasserstein._to_device`` with this module's message."""
    if not (isinstance(x, torch.Tensor) and x.device.type == "cuda") and not torch.cuda.is_available():
        raise N.FFDError("the nearest-neighbour metrics need an MI355X (gfx950) device; there is no CPU fallback")
    from .wasserstein import _to_device as to_device

    return to_device(x)


def _pair(query, reference, exclude_self: bool):
    r = _to_device(reference)
    q = r if query is reference else _to_device(query)
    assert q.shape[1] == r.shape[1], f"the two sets have {q.shape[1]} and {r.shape[1]} features"
    if exclude_self:
        assert q.data_ptr() == r.data_ptr() and q.shape == r.shape, \
            "exclude_self needs the query set to be the reference set itself"
    return q, r


def nearest_neighbours(query, reference, k: int, exclude_self: bool = False, budget_bytes: int = WORK_BUDGET_BYTES):
    """The ``k`` nearest rows of ``reference`` (nr, D) for every row of ``query`` (nq, D): ``(dist2, index)``, float64
    (nq, k) ascending and int32 (nq, k) device tensors, ties by the lower index.  ``exclude_self`` skips the pair i == i
    and needs ``query is reference`` (or the same device buffer)."""
    q, r = _pair(query, reference, exclude_self)
    (nq, D), nr = q.shape, r.shape[0]
    k = int(k)
    assert 1 <= k <= MAX_K, f"k must lie in [1, {MAX_K}], got {k}"
    assert k <= nr - int(bool(exclude_self)), f"k = {k} neighbours asked of {nr - int(bool(exclude_self))} rows"
    lib, dev = N.lib(), r.device
    dist2 = torch.empty((nq, k), device=dev, dtype=torch.float64)
    index = torch.empty((nq, k), device=dev, dtype=torch.int32)
    nbytes = lib.ffd_nn_work_bytes(nq, nr, D, k, int(budget_bytes))
    if nbytes == 0:
        raise NotImplementedError(f"nearest_neighbours: a shape outside the library's limits ({nq}, {nr}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_nn_search(q.data_ptr(), nq, r.data_ptr(), nr, D, k, int(bool(exclude_self)), dist2.data_ptr(),
                              index.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None, "ffd_nn_search")
    return dist2, index


def ball_counts(query, reference, radius2, exclude_self: bool = False) -> torch.Tensor:
    """count[i] = #{ j : |query_i - reference_j|^2 <= radius2[j] }: int32 (nq,) device tensor.  ``radius2``: (nr,),
    taken as fp32."""
    q, r = _pair(query, reference, exclude_self)
    (nq, D), nr = q.shape, r.shape[0]
    rad = radius2 if isinstance(radius2, torch.Tensor) and radius2.device.type == "cuda" and \
        radius2.dtype == torch.float32 else _to_device(torch.as_tensor(radius2).reshape(-1, 1))
    rad = rad.reshape(-1).contiguous()
    assert rad.numel() == nr, f"{rad.numel()} radii for {nr} reference rows"
    lib, dev = N.lib(), r.device
    count = torch.empty(nq, device=dev, dtype=torch.int32)
    nbytes = lib.ffd_nn_work_bytes(nq, nr, D, 1, 0)
    if nbytes == 0:
        raise NotImplementedError(f"ball_counts: a shape outside the library's limits ({nq}, {nr}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_nn_ball_count(q.data_ptr(), nq, r.data_ptr(), nr, D, rad.data_ptr(), int(bool(exclude_self)),
                                  count.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None,
            "ffd_nn_ball_count")
    return count


def kth_radius2(dist2: torch.Tensor, col: int) -> torch.Tensor:
    """Column ``col`` of a (n, k) search result as the fp32 radii of a ball count (``ffd_nn_radius``)."""
    n, k = dist2.shape
    out = torch.empty(n, device=dist2.device, dtype=torch.float32)
    N.check(N.lib().ffd_nn_radius(dist2.data_ptr(), n, k, int(col), out.data_ptr(), N.current_stream_ptr(dist2.device)),
            None, "ffd_nn_radius")
    return out


def self_search(y: torch.Tensor, k: int):
    """What ``manifold_scores`` needs of a set alone: its self-search at ``k`` and the fp32 k-th radii."""
    dist2, _ = nearest_neighbours(y, y, k, exclude_self=True)
    return dist2, kth_radius2(dist2, k - 1)


def manifold_scores(original, samples, k: int, original_self=None) -> dict:
    """The eight numbers of ``SCORE_KEYS`` for the originals Y (n, D) and the samples X (m, D), as Python floats:
    two self-searches at ``k`` (``original_self``: Y's, from ``self_search``, when the caller keeps it), the two cross
    searches at k = 1, two ball counts, one scoring kernel."""
    y, x = _to_device(original), _to_device(samples)
    n, m = y.shape[0], x.shape[0]
    assert n >= k + 1 and m >= k + 1, f"k = {k} needs at least {k + 1} rows in both sets, got {n} and {m}"
    self_y, rad_y = original_self if original_self is not None else self_search(y, k)
    _, rad_x = self_search(x, k)
    xy_d2, xy_idx = nearest_neighbours(x, y, 1)
    yx_d2, _ = nearest_neighbours(y, x, 1)
    count_x = ball_counts(x, y, rad_y)
    count_y = ball_counts(y, x, rad_x)
    out = torch.empty(8, device=y.device, dtype=torch.float64)
    N.check(N.lib().ffd_nn_scores(self_y.data_ptr(), xy_d2.data_ptr(), xy_idx.data_ptr(), yx_d2.data_ptr(),
                                  count_x.data_ptr(), count_y.data_ptr(), n, m, int(k), out.data_ptr(),
                                  N.current_stream_ptr(y.device)), None, "ffd_nn_scores")
    return dict(zip(SCORE_KEYS, out.tolist()))
