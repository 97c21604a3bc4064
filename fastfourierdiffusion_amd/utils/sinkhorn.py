"""Entropic optimal transport between two row sets on the device (libffd, csrc/ffd_sinkhorn.hip): the softmin of the
squared-distance cost against a potential, an epsilon schedule, the symmetric Sinkhorn loop and the debiased Sinkhorn
divergence (Cuturi 2013; Genevay, Peyre, Cuturi 2018; Feydy et al. 2019); what ``sampling.metrics.SinkhornDivergence``
reports.

softmin_eps(x | y, h)_i = -eps log((1 / nr) sum_j exp((h_j - |x_i - y_j|^2) / eps)) on flat fp32 rows (n, D) with uniform
weights.  The pair distances come from the exact-fp32 matrix cores on rows centred on one vector (``centre``: the
originals' column mean, ``utils.kernel_mmd.column_mean``); the exponentials are fp32 and a row's running (max, sum) keeps
its sum in fp64 in a fixed order, so a row's value has the same bits however the query set is cut.  Potentials are float64
device tensors.  These functions take and return device tensors: a host tensor, another dtype or shape, or an epsilon that
is not positive and finite is refused before any native call.  torch holds memory only.  Without libffd.so or a gfx950
device every call raises ``FFDError``: there is no numpy fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native as N
from .kernel_mmd import _centre, _f64, _rows
from .wasserstein import _work


def _eps(eps) -> float:
    eps = float(eps)
    assert np.isfinite(eps) and eps > 0.0, f"epsilon must be positive and finite, got {eps}"
    return eps


def _schedule(eps_schedule) -> np.ndarray:
    e = np.ascontiguousarray(np.asarray(eps_schedule, np.float64).reshape(-1))
    assert e.size >= 1, "an epsilon schedule needs at least one entry"
    assert np.isfinite(e).all() and (e > 0).all(), f"epsilons must be positive and finite, got {e.tolist()}"
    return e


def softmin(query, ref, centre, h, eps, old=None) -> torch.Tensor:
    """out_i = -eps log((1 / nr) sum_j exp((h_j - |query_i - ref_j|^2) / eps)): a float64 (nq,) device tensor.  ``h``
    float64 (nr,); with ``old`` float64 (nq,) the damped update (old + out) / 2 (``ffd_sinkhorn_softmin``)."""
    same = query is ref
    ref = _rows(ref, "ref")
    query = ref if same else _rows(query, "query")  # one conversion for one set: a non-contiguous tensor is copied once
    (nq, D), nr = query.shape, ref.shape[0]
    assert ref.shape[1] == D, f"the two sets have {D} and {ref.shape[1]} features"
    c, eps = _centre(centre, D), _eps(eps)
    h = _f64(h, "h", (nr,))
    if old is not None:
        old = _f64(old, "old", (nq,))
    lib, dev = N.lib(), query.device
    out = torch.empty(nq, device=dev, dtype=torch.float64)
    nbytes = lib.ffd_sinkhorn_softmin_work_bytes(nq, nr, D)
    if nbytes == 0:
        raise NotImplementedError(f"softmin: a shape outside the library's limits ({nq}, {nr}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_sinkhorn_softmin(query.data_ptr(), nq, ref.data_ptr(), nr, D, c.data_ptr(), h.data_ptr(), eps,
                                     None if old is None else old.data_ptr(), out.data_ptr(), work.data_ptr(), nbytes,
                                     N.current_stream_ptr(dev)), None, "ffd_sinkhorn_softmin")
    return out


def diameter2(y, centre) -> torch.Tensor:
    """4 max_j |y_j - centre|^2, an upper bound of every squared distance inside the set: a float64 device tensor of one
    element (``ffd_sinkhorn_diameter2``).  Where a schedule starts."""
    y = _rows(y, "y")
    n, D = y.shape
    c = _centre(centre, D)
    lib = N.lib()
    out = torch.empty(1, device=y.device, dtype=torch.float64)
    nbytes = lib.ffd_sinkhorn_diameter2_work_bytes(n, D)
    if nbytes == 0:
        raise NotImplementedError(f"diameter2: a shape outside the library's limits ({n}, {D})")
    work = _work(nbytes, y.device)
    N.check(lib.ffd_sinkhorn_diameter2(y.data_ptr(), n, D, c.data_ptr(), out.data_ptr(), work.data_ptr(), nbytes,
                                       N.current_stream_ptr(y.device)), None, "ffd_sinkhorn_diameter2")
    return out


def schedule(diameter2: float, eps: float, scaling: float = 0.5, n_final: int = 3) -> list:
    """diameter2, diameter2 scaling^2, diameter2 scaling^4, ... while above ``eps``, then ``n_final`` entries of ``eps``
    (``ffd_host_sinkhorn_schedule``: host only)."""
    diameter2, eps, scaling, n_final = float(diameter2), _eps(eps), float(scaling), int(n_final)
    assert np.isfinite(diameter2) and diameter2 > 0.0, f"diameter^2 must be positive and finite, got {diameter2}"
    assert 0.0 < scaling < 1.0, f"scaling must lie in (0, 1), got {scaling}"
    assert n_final >= 1, f"n_final must be at least 1, got {n_final}"
    lib = N.lib()
    count = lib.ffd_host_sinkhorn_schedule(diameter2, eps, scaling, n_final, None, 0)
    N.check(min(count, 0), None, "ffd_host_sinkhorn_schedule")
    out = (C.c_double * count)()
    N.check(min(lib.ffd_host_sinkhorn_schedule(diameter2, eps, scaling, n_final, C.addressof(out), count), 0), None,
            "ffd_host_sinkhorn_schedule")
    return list(out)


@dataclass
class SinkhornResult:
    """``divergence`` S = mean (f - p) + mean (g - q); ``ot_xy`` = mean f + mean g, the entropic cost OT_eps(x, y);
    ``change`` the largest |change| of f and g in the last damped pass (large: the schedule did not converge); the four
    potentials as float64 device tensors, f and p over x's rows, g and q over y's."""
    divergence: float
    ot_xy: float
    change: float
    f: torch.Tensor
    g: torch.Tensor
    p: torch.Tensor
    q: torch.Tensor


def sinkhorn_divergence(x, y, centre, eps_schedule, q=None) -> SinkhornResult:
    """The symmetric Sinkhorn loop of x (n, D) against y (m, D) over ``eps_schedule`` and the extrapolation pass at its
    last entry (``ffd_sinkhorn``).  ``q`` float64 (m,): an already converged self potential of y (the ``q`` of an earlier
    result on the same y, centre and schedule); the y|y passes are then skipped."""
    x, y = _rows(x, "x"), _rows(y, "y")
    (n, D), m = x.shape, y.shape[0]
    assert y.shape[1] == D, f"the two sets have {D} and {y.shape[1]} features"
    c, sched = _centre(centre, D), _schedule(eps_schedule)
    if q is not None:
        q = _f64(q, "q", (m,))
    lib, dev = N.lib(), x.device
    f, p = torch.empty(n, device=dev, dtype=torch.float64), torch.empty(n, device=dev, dtype=torch.float64)
    g, q_out = torch.empty(m, device=dev, dtype=torch.float64), torch.empty(m, device=dev, dtype=torch.float64)
    out3 = torch.empty(3, device=dev, dtype=torch.float64)
    nbytes = lib.ffd_sinkhorn_work_bytes(n, m, D)
    if nbytes == 0:
        raise NotImplementedError(f"sinkhorn_divergence: a shape outside the library's limits ({n}, {m}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_sinkhorn(x.data_ptr(), n, y.data_ptr(), m, D, c.data_ptr(), sched.ctypes.data, int(sched.size),
                             None if q is None else q.data_ptr(), f.data_ptr(), g.data_ptr(), p.data_ptr(), q_out.data_ptr(),
                             out3.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None, "ffd_sinkhorn")
    s, ot, change = out3.tolist()
    return SinkhornResult(divergence=s, ot_xy=ot, change=change, f=f, g=g, p=p, q=q_out)


def self_potential(y, centre, eps_schedule) -> torch.Tensor:
    """The converged self potential q of y over ``eps_schedule``, float64 (m,): q <- (q + softmin(y | y, q)) / 2 from 0
    (the first pass undamped), then the undamped pass at the last epsilon -- pass for pass what ``sinkhorn_divergence``
    does for its ``q``, with the same kernels: the same bits."""
    y = _rows(y, "y")
    sched = _schedule(eps_schedule)
    q = torch.zeros(y.shape[0], device=y.device, dtype=torch.float64)
    for k, eps in enumerate(sched):
        q = softmin(y, y, centre, q, eps, old=q if k > 0 else None)
    return softmin(y, y, centre, q, sched[-1])
