"""Scores of a forecast / imputation ensemble against the truth (an extension beyond the reference): the continuous
ranked probability score per point, the energy score per series, quantile bands and the rank of the truth in the
ensemble, computed on the device by libffd (csrc/ffd_ensemble.hip; include/ffd.h ``ffd_ens_pointwise``,
``ffd_ens_energy``).

``DiffusionSampler.impute`` and ``sample_conditional`` draw many completions of one observed series; their output goes
in as it is.  Inputs may be numpy arrays, host tensors or device tensors; float64 input is rounded to fp32 at upload, as
in the Wasserstein metrics.  Without libffd.so or a gfx950 device the call raises ``FFDError``: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from .. import _native as N

# most device scratch one call asks for; larger problems are processed in blocks (no result depends on it)
WORK_BUDGET_BYTES = 1 << 30


def _as_tensor(x) -> torch.Tensor:
    return x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def _shapes(ensemble, truth, mask):
    """-> ensemble (S, m, L, C), truth (S, L, C), weight None or (1 | S, L, C) fp32 with 1 = scored, 0 = observed."""
    ens, y = _as_tensor(ensemble), _as_tensor(truth)
    if ens.dim() == 3:
        ens = ens.unsqueeze(0)
    if ens.dim() != 4:
        raise ValueError(f"ensemble must be (m, L, C) or (S, m, L, C), got {tuple(ens.shape)}")
    S, m, L, Cn = ens.shape
    if y.dim() == 2:
        y = y.unsqueeze(0)
    if tuple(y.shape) != (S, L, Cn):
        raise ValueError(f"truth must be (L, C) or (S, L, C) = {(S, L, Cn)}, got {tuple(y.shape)}")
    w = None
    if mask is not None:
        mk = _as_tensor(mask).to(torch.float32)
        if mk.dim() == 1:
            mk = mk.unsqueeze(-1)
        if mk.dim() == 2:
            mk = mk.unsqueeze(0)
        if mk.dim() != 3 or mk.shape[1] != L or mk.shape[2] not in (1, Cn) or mk.shape[0] not in (1, S):
            raise ValueError(f"mask must be (L,), (L, 1), (L, C) or (S, L, C) matching the ensemble {tuple(ens.shape)}, "
                             f"got {tuple(mk.shape)}")
        if not bool(((mk == 0) | (mk == 1)).all()):
            raise ValueError("mask entries must be 0 or 1")
        w = (1.0 - mk).expand(mk.shape[0], L, Cn)  # the mask marks the observed points; the weight the scored ones
    return ens, y, w


def _device_of(t: torch.Tensor) -> torch.device:
    """The device the scores run on: the ensemble's own if it lives on one, else the current one."""
    if t.device.type == "cuda":
        return t.device
    if not torch.cuda.is_available():
        raise N.FFDError("sampling needs an MI355X (gfx950) device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def ensemble_scores(ensemble, truth, mask=None, quantiles: Sequence[float] = (0.05, 0.5, 0.95), fair: bool = False,
                    energy: bool = True) -> dict:
    """Score an ensemble against the truth.

    ``ensemble``: (m, L, C) -- m completions of one series, the output of ``impute`` / ``sample_conditional`` with a
    shared observation -- or (S, m, L, C); ``truth``: (L, C) or (S, L, C); ``mask``: the OBSERVED mask in the shapes
    ``sample_conditional`` takes (1 = observed): observed points are excluded from every score and their per-point
    outputs are 0.  ``fair``: Ferro's unbiased CRPS / energy estimator (pair sums over m (m - 1) instead of m^2; m >= 2).

    Returns CPU tensors: ``crps`` (S, L, C) and ``crps_mean`` (S,) (the mean over the scored points), ``quantiles``
    (n_q, S, L, C) (numpy's default linear quantile at the given levels), ``below`` / ``equal`` (S, L, C) int32 (members
    < and == the truth: rank, PIT and coverage follow from them), and with ``energy`` the ``energy_score`` (S,).
    float64 except the counts."""
    ens, y, w = _shapes(ensemble, truth, mask)
    S, m, L, Cn = ens.shape
    D = L * Cn
    levels = [float(p) for p in quantiles]
    if any(not 0.0 <= p <= 1.0 for p in levels):
        raise ValueError(f"quantile levels must lie in [0, 1], got {levels}")
    if len(levels) > 64:
        raise ValueError("at most 64 quantile levels")
    if fair and m < 2:
        raise ValueError("fair=True needs at least two members")
    device = _device_of(ens)
    lib, stream = N.lib(), N.current_stream_ptr(device)
    ens_d, y_d = _upload(ens, device), _upload(y, device)
    w_d = _upload(w, device) if w is not None else None
    n_q = len(levels)
    f64 = dict(device=device, dtype=torch.float64)
    crps = torch.empty((S, L, Cn), **f64)
    crps_mean = torch.empty(S, **f64)
    quant = torch.empty((n_q, S, L, Cn), **f64)
    below = torch.empty((S, L, Cn), device=device, dtype=torch.int32)
    equal = torch.empty_like(below)
    nbytes = lib.ffd_ens_work_bytes(S, m, D, n_q, WORK_BUDGET_BYTES)
    if nbytes == 0:
        raise NotImplementedError(f"ensemble of shape {tuple(ens.shape)}: S, m and L * C go up to 2^20")
    work = torch.empty((nbytes + 15) // 16 * 2, **f64)
    w_ptr, w_batch = (w_d.data_ptr(), w_d.shape[0]) if w_d is not None else (None, 1)
    lv = (C.c_double * max(n_q, 1))(*levels)
    N.check(lib.ffd_ens_pointwise(ens_d.data_ptr(), y_d.data_ptr(), w_ptr, w_batch, S, m, D, lv, n_q, int(bool(fair)),
                                  crps.data_ptr(), crps_mean.data_ptr(), quant.data_ptr() if n_q else None,
                                  below.data_ptr(), equal.data_ptr(), work.data_ptr(), nbytes, stream), None,
            "ffd_ens_pointwise")
    out = {"crps": crps.cpu(), "crps_mean": crps_mean.cpu(), "quantiles": quant.cpu(), "below": below.cpu(),
           "equal": equal.cpu()}
    if energy:
        es = torch.empty(S, **f64)
        N.check(lib.ffd_ens_energy(ens_d.data_ptr(), y_d.data_ptr(), w_ptr, w_batch, S, m, D, int(bool(fair)),
                                   es.data_ptr(), work.data_ptr(), nbytes, stream), None, "ffd_ens_energy")
        out["energy_score"] = es.cpu()
    return out
