"""The first two moments of a row set in float64 on the device (libffd, csrc/ffd_pca.hip): mean and covariance, a symmetric
eigensolver, the symmetric square root, the Frechet distance between two fitted Gaussians (Dowson & Landau 1982; the
quantity behind FID, Heusel et al. 2017) and principal-component variances and scores; what
``sampling.metrics.FrechetDistance`` reports.

FD = |mu_x - mu_y|^2 + tr S_x + tr S_y - 2 tr (S_y^1/2 S_x S_y^1/2)^1/2 on flat fp32 rows (n, D), D <= ``MAX_D``.  Means,
covariances, eigenvalues and vectors are float64 device tensors; matrix products run on the fp64 matrix cores and every sum
has one fixed order, so a result keeps its bits from run to run.  The eigensolver is cyclic Jacobi with relative thresholds
only; it reads 8 bytes back per sweep, so ``eigh`` and ``frechet_distance`` synchronise the current stream.  These
functions take and return device tensors: a host tensor, another dtype or shape is refused before any native call.  torch
holds memory only.  Without libffd.so or a gfx950 device every call raises ``FFDError``: there is no numpy fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from .. import _native as N
from .kernel_mmd import _f64, _rows
from .wasserstein import _work

MAX_D = 1024        # include/ffd.h FFD_PCA_MAX_D
MAX_SWEEPS = 30     # the default cap of the Jacobi sweeps


def _dim(D: int) -> int:
    assert 1 <= D <= MAX_D, f"between 1 and {MAX_D} features, got {D}"
    return D


def _sweeps(max_sweeps) -> int:
    max_sweeps = int(max_sweeps)
    assert max_sweeps >= 1, f"max_sweeps must be at least 1, got {max_sweeps}"
    return max_sweeps


def _square(a, name: str) -> torch.Tensor:
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    assert a.dim() == 2 and a.shape[0] == a.shape[1], f"{name}: expected a square float64 matrix, got {tuple(a.shape)}"
    _dim(a.shape[0])
    return _f64(a, name, a.shape)


def _converged(info, what: str, max_sweeps: int) -> None:
    if info[2] != 1.0:
        raise N.FFDError(f"{what}: the Jacobi sweeps did not converge in {max_sweeps} sweeps "
                         f"(off(A) / |A|_F = {info[1]:.3e} after {int(info[0])}; the bar is 2^-53)")


def covariance(x):
    """(mean (D,), unbiased covariance (D, D)) of the rows of x, float64 device tensors (``ffd_cov``).  The covariance is
    bitwise symmetric."""
    x = _rows(x, "x", 2)
    n, D = x.shape
    _dim(D)
    lib, dev = N.lib(), x.device
    mean = torch.empty(D, device=dev, dtype=torch.float64)
    cov = torch.empty((D, D), device=dev, dtype=torch.float64)
    nbytes = lib.ffd_cov_work_bytes(n, D)
    if nbytes == 0:
        raise NotImplementedError(f"covariance: a shape outside the library's limits ({n}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_cov(x.data_ptr(), n, D, mean.data_ptr(), cov.data_ptr(), work.data_ptr(), nbytes,
                        N.current_stream_ptr(dev)), None, "ffd_cov")
    return mean, cov


@dataclass
class EighInfo:
    """``sweeps`` the Jacobi sweeps done, ``off`` the final off(A) / |A|_F."""
    sweeps: int
    off: float


def eigh(a, vectors: bool = True, max_sweeps: int = MAX_SWEEPS, info: bool = False):
    """The eigenvalues of the symmetric matrix ``a`` (its upper triangle is read), ascending, float64 (D,); with ``vectors``
    also the eigenvectors as the columns of a (D, D) tensor (``ffd_sym_eig``).  Raises ``FFDError`` when ``max_sweeps``
    sweeps did not bring off(A) to 2^-53 |A|_F.  ``info``: an ``EighInfo`` is returned as the last element."""
    a = _square(a, "a")
    D, max_sweeps = a.shape[0], _sweeps(max_sweeps)
    lib, dev = N.lib(), a.device
    w = torch.empty(D, device=dev, dtype=torch.float64)
    v = torch.empty((D, D), device=dev, dtype=torch.float64) if vectors else None
    info3 = (C.c_double * 3)()
    nbytes = lib.ffd_sym_eig_work_bytes(D)
    work = _work(nbytes, dev)
    N.check(lib.ffd_sym_eig(a.data_ptr(), D, max_sweeps, w.data_ptr(), None if v is None else v.data_ptr(),
                            C.addressof(info3), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None, "ffd_sym_eig")
    _converged(info3, "eigh", max_sweeps)
    found = (w, v) if vectors else (w,)
    if info:
        found = found + (EighInfo(int(info3[0]), float(info3[1])),)
    return found if len(found) > 1 else found[0]


def sym_root(w, v) -> torch.Tensor:
    """V diag(sqrt(max(w, 0))) V^T, the symmetric square root of the positive part, bitwise symmetric (``ffd_sym_root``)."""
    v = _square(v, "v")
    D = v.shape[0]
    w = _f64(w, "w", (D,))
    lib, dev = N.lib(), v.device
    root = torch.empty((D, D), device=dev, dtype=torch.float64)
    nbytes = lib.ffd_sym_root_work_bytes(D)
    work = _work(nbytes, dev)
    N.check(lib.ffd_sym_root(w.data_ptr(), v.data_ptr(), D, root.data_ptr(), work.data_ptr(), nbytes,
                             N.current_stream_ptr(dev)), None, "ffd_sym_root")
    return root


@dataclass
class FrechetResult:
    """``distance`` = ``mean_term`` + ``cov_term``; ``mean_term`` |mu_x - mu_y|^2; ``cov_term`` tr S_x + tr S_y - 2 tr
    (S_y^1/2 S_x S_y^1/2)^1/2; the two traces."""
    distance: float
    mean_term: float
    cov_term: float
    trace_x: float
    trace_y: float


def frechet_distance(mean_x, cov_x, mean_y, cov_y, root_y=None, max_sweeps: int = MAX_SWEEPS) -> FrechetResult:
    """The Frechet distance between N(mean_x, cov_x) and N(mean_y, cov_y) (``ffd_frechet``).  ``root_y``: the ``sym_root``
    of cov_y's eigenpairs, when it is at hand (the same bits with and without it)."""
    cov_x, cov_y = _square(cov_x, "cov_x"), _square(cov_y, "cov_y")
    D, max_sweeps = cov_x.shape[0], _sweeps(max_sweeps)
    assert cov_y.shape[0] == D, f"the two covariances have {D} and {cov_y.shape[0]} features"
    mean_x, mean_y = _f64(mean_x, "mean_x", (D,)), _f64(mean_y, "mean_y", (D,))
    if root_y is not None:
        root_y = _f64(root_y, "root_y", (D, D))
    lib, dev = N.lib(), cov_x.device
    out5 = torch.empty(5, device=dev, dtype=torch.float64)
    info3 = (C.c_double * 3)()
    nbytes = lib.ffd_frechet_work_bytes(D)
    work = _work(nbytes, dev)
    N.check(lib.ffd_frechet(mean_x.data_ptr(), cov_x.data_ptr(), mean_y.data_ptr(), cov_y.data_ptr(),
                            None if root_y is None else root_y.data_ptr(), D, max_sweeps, out5.data_ptr(),
                            C.addressof(info3), work.data_ptr(), nbytes, N.current_stream_ptr(dev)), None, "ffd_frechet")
    _converged(info3, "frechet_distance", max_sweeps)
    return FrechetResult(*out5.tolist())


def pc_variances(cov, v, k: int) -> torch.Tensor:
    """v_i^T cov v_i for the k eigenvectors of largest eigenvalue (the last k columns of ``v``, as ``eigh`` orders them),
    the largest first: float64 (k,) (``ffd_pca_variances``)."""
    cov, v = _square(cov, "cov"), _square(v, "v")
    D, k = cov.shape[0], int(k)
    assert v.shape[0] == D, f"cov and v have {D} and {v.shape[0]} features"
    assert 1 <= k <= D, f"k must lie in [1, {D}], got {k}"
    lib, dev = N.lib(), cov.device
    out = torch.empty(k, device=dev, dtype=torch.float64)
    nbytes = lib.ffd_pca_variances_work_bytes(D, k)
    work = _work(nbytes, dev)
    N.check(lib.ffd_pca_variances(cov.data_ptr(), v.data_ptr(), D, k, out.data_ptr(), work.data_ptr(), nbytes,
                                  N.current_stream_ptr(dev)), None, "ffd_pca_variances")
    return out


def transform(x, mean, v, k: int) -> torch.Tensor:
    """The scores (x - mean) V[:, top k] of the rows of x on the k axes of largest eigenvalue, the largest first: float64
    (n, k) (``ffd_pca_transform``)."""
    x = _rows(x, "x")
    n, D = x.shape
    _dim(D)
    k = int(k)
    mean, v = _f64(mean, "mean", (D,)), _f64(v, "v", (D, D))
    assert 1 <= k <= D, f"k must lie in [1, {D}], got {k}"
    lib, dev = N.lib(), x.device
    scores = torch.empty((n, k), device=dev, dtype=torch.float64)
    N.check(lib.ffd_pca_transform(x.data_ptr(), n, D, mean.data_ptr(), v.data_ptr(), k, scores.data_ptr(),
                                  N.current_stream_ptr(dev)), None, "ffd_pca_transform")
    return scores
