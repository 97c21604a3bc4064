"""Kernel two-sample statistics between two row sets on the device (libffd, csrc/ffd_mmd.hip): Gaussian-kernel row sums,
the unbiased and biased maximum mean discrepancy, per-sample witness values, a closed-form bandwidth and a permutation
test; what ``sampling.metrics.KernelMMD`` reports.

k_gamma(a, b) = exp(-gamma |a - b|^2) on flat fp32 rows (n, D).  The pair distances come from the exact-fp32 matrix cores
on rows centred on one vector (``centre``: the originals' column mean); kernel values are fp32 and are summed in fp64 in
a fixed order, so a row's sum has the same bits however the query set is cut.  These functions take and return device
tensors: a host tensor, another dtype or shape, or a set of fewer than 2 rows where 2 are needed is refused before any
native call.  torch holds memory only.  Without libffd.so or a gfx950 device every call raises ``FFDError``: there is no
numpy fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from .wasserstein import _work

MAX_GAMMAS = 8             # include/ffd.h FFD_MMD_MAX_GAMMAS
MAX_POOLED = 16384         # include/ffd.h FFD_MMD_MAX_POOLED: rows of both sets together in a permutation test
MAX_PERMUTATIONS = 4096    # include/ffd.h FFD_MMD_MAX_PERMUTATIONS: assignments of one call, the observed one included
DEFAULT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def _rows(x, name: str, min_rows: int = 1) -> torch.Tensor:
    """A (n, D) fp32 contiguous device tensor, or the refusal."""
    t = N.require_gpu_tensor(x, name)
    assert t.dim() == 2, f"{name}: expected a 2d array, got {t.dim()}d"
    assert t.shape[0] >= min_rows and t.shape[1] >= 1, f"{name}: needs at least {min_rows} rows, got {tuple(t.shape)}"
    return t


def _f64(x, name: str, shape) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if x.device.type != "cuda":
        raise N.FFDError(f"{name} lives on {x.device}: the kernel statistics compute on the device only")
    assert x.dtype == torch.float64 and tuple(x.shape) == tuple(shape), \
        f"{name}: expected float64 {tuple(shape)}, got {x.dtype} {tuple(x.shape)}"
    return x.contiguous()


def _gammas(gammas):
    g = np.ascontiguousarray(np.asarray(gammas, np.float64).reshape(-1))
    assert 1 <= g.size <= MAX_GAMMAS, f"between 1 and {MAX_GAMMAS} bandwidths, got {g.size}"
    assert np.isfinite(g).all() and (g >= 0).all(), f"bandwidths must be finite and >= 0, got {g.tolist()}"
    return g


def _centre(centre, D: int) -> torch.Tensor:
    c = N.require_gpu_tensor(centre, "centre").reshape(-1)
    assert c.numel() == D, f"centre has {c.numel()} entries for {D} features"
    return c


def ladder_gammas(sigma2: float, scales=DEFAULT_SCALES) -> list:
    """gamma_s = 1 / (2 sigma^2 s) for every scale s."""
    sigma2 = float(sigma2)
    assert sigma2 > 0 and np.isfinite(sigma2), f"sigma^2 must be positive and finite, got {sigma2}"
    return [1.0 / (2.0 * sigma2 * float(s)) for s in scales]


def column_mean(y) -> torch.Tensor:
    """(D,) fp32 column mean of a set, the vector both sets of a call are centred on (``ffd_mmd_centre``)."""
    y = _rows(y, "y")
    n, D = y.shape
    lib = N.lib()
    out = torch.empty(D, device=y.device, dtype=torch.float32)
    nbytes = lib.ffd_mmd_centre_work_bytes(n, D)
    if nbytes == 0:
        raise NotImplementedError(f"column_mean: a shape outside the library's limits ({n}, {D})")
    work = _work(nbytes, y.device)
    N.check(lib.ffd_mmd_centre(y.data_ptr(), n, D, out.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(y.device)),
            None, "ffd_mmd_centre")
    return out


def bandwidth(y) -> torch.Tensor:
    """sigma^2 = 2 n / (n - 1) mean_j |y_j - ybar|^2, the mean squared distance between two distinct rows: a float64
    device tensor of one element (``ffd_mmd_bandwidth``; all fp64, no pair is formed)."""
    y = _rows(y, "y", 2)
    n, D = y.shape
    lib = N.lib()
    out = torch.empty(1, device=y.device, dtype=torch.float64)
    nbytes = lib.ffd_mmd_bandwidth_work_bytes(n, D)
    if nbytes == 0:
        raise NotImplementedError(f"bandwidth: a shape outside the library's limits ({n}, {D})")
    work = _work(nbytes, y.device)
    N.check(lib.ffd_mmd_bandwidth(y.data_ptr(), n, D, out.data_ptr(), work.data_ptr(), nbytes,
                                  N.current_stream_ptr(y.device)), None, "ffd_mmd_bandwidth")
    return out


def row_sums(a, b, centre, gammas, exclude_self: bool = False) -> torch.Tensor:
    """rowsum[g][i] = sum_j exp(-gammas[g] |a_i - b_j|^2): float64 (n_gamma, na) device tensor.  ``exclude_self`` skips
    the pair i == j and needs ``a`` and ``b`` to be the same device buffer."""
    same = a is b
    b = _rows(b, "b")
    a = b if same else _rows(a, "a")  # one conversion for one set: a non-contiguous tensor is copied once
    (na, D), nb = a.shape, b.shape[0]
    assert b.shape[1] == D, f"the two sets have {D} and {b.shape[1]} features"
    if exclude_self:
        assert a.data_ptr() == b.data_ptr() and a.shape == b.shape, "exclude_self needs a to be b itself"
    c, g = _centre(centre, D), _gammas(gammas)
    lib, dev = N.lib(), a.device
    out = torch.empty((g.size, na), device=dev, dtype=torch.float64)
    nbytes = lib.ffd_mmd_rowsums_work_bytes(na, nb, D, int(g.size))
    if nbytes == 0:
        raise NotImplementedError(f"row_sums: a shape outside the library's limits ({na}, {nb}, {D})")
    work = _work(nbytes, dev)
    N.check(lib.ffd_mmd_rowsums(a.data_ptr(), na, b.data_ptr(), nb, D, c.data_ptr(), g.ctypes.data, int(g.size),
                                int(bool(exclude_self)), out.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(dev)),
            None, "ffd_mmd_rowsums")
    return out


def mmd_scores(rowsum_xx, rowsum_xy, rowsum_yy):
    """``(mmd2, witness)`` from the row sums XX (n_gamma, n; self excluded), XY (n_gamma, n) and YY (n_gamma, m; self
    excluded): ``mmd2`` float64 (2, n_gamma + 1), row 0 unbiased and row 1 biased, the last column the mean kernel's;
    ``witness`` float64 (n,), w_i = xx_i / (n - 1) - xy_i / m for the mean kernel."""
    assert isinstance(rowsum_xx, torch.Tensor) and rowsum_xx.dim() == 2, "rowsum_xx: expected a (n_gamma, n) tensor"
    assert isinstance(rowsum_yy, torch.Tensor) and rowsum_yy.dim() == 2, "rowsum_yy: expected a (n_gamma, m) tensor"
    (ng, n), m = rowsum_xx.shape, rowsum_yy.shape[1]
    assert 1 <= ng <= MAX_GAMMAS, f"between 1 and {MAX_GAMMAS} bandwidths, got {ng}"
    assert n >= 2 and m >= 2, f"both sets need at least 2 rows, got {n} and {m}"
    xx, xy, yy = _f64(rowsum_xx, "rowsum_xx", (ng, n)), _f64(rowsum_xy, "rowsum_xy", (ng, n)), \
        _f64(rowsum_yy, "rowsum_yy", (ng, m))
    dev = xx.device
    mmd2 = torch.empty((2, ng + 1), device=dev, dtype=torch.float64)
    witness = torch.empty(n, device=dev, dtype=torch.float64)
    N.check(N.lib().ffd_mmd_scores(xx.data_ptr(), xy.data_ptr(), yy.data_ptr(), n, m, ng, mmd2.data_ptr(), witness.data_ptr(),
                                   N.current_stream_ptr(dev)), None, "ffd_mmd_scores")
    return mmd2, witness


def permutation_assignments(n: int, m: int, permutations: int, seed: int) -> np.ndarray:
    """(permutations + 1, n + m) uint8 host matrix with n ones per row: row 0 is the observed assignment (the first n
    pooled rows), row p >= 1 the first n entries of the p-th permutation of ``numpy.random.Generator(PCG64([seed, n, m]))``
    -- drawn on the host, as ``Trainer.epoch_order`` draws its orders, so that any restatement judges the same ones."""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(n), int(m)]))
    A = np.zeros((int(permutations) + 1, n + m), np.uint8)
    A[0, :n] = 1
    for p in range(1, int(permutations) + 1):
        A[p, rng.permutation(n + m)[:n]] = 1
    return A


def permutation_test(x, y, centre, gammas, assignments) -> torch.Tensor:
    """T_p of the mean kernel over ``gammas`` for every row of ``assignments`` ((P, n + m) uint8, n ones per row, a host
    array or a device tensor; x's rows come first in the pooled order): float64 (P,) device tensor.  At most
    ``MAX_POOLED`` pooled rows and ``MAX_PERMUTATIONS`` assignments."""
    x, y = _rows(x, "x", 2), _rows(y, "y", 2)
    (n, D), m = x.shape, y.shape[0]
    assert y.shape[1] == D, f"the two sets have {D} and {y.shape[1]} features"
    if n + m > MAX_POOLED:
        raise ValueError(f"a permutation test takes at most {MAX_POOLED} rows of both sets together, got {n} + {m}")
    c, g = _centre(centre, D), _gammas(gammas)
    if isinstance(assignments, torch.Tensor):
        assert assignments.dtype == torch.uint8 and assignments.dim() == 2, "assignments: expected a 2d uint8 tensor"
        A = assignments.to(x.device).contiguous()
    else:
        host = np.ascontiguousarray(assignments)
        assert host.dtype == np.uint8 and host.ndim == 2, "assignments: expected a 2d uint8 array"
        assert ((host != 0).sum(axis=1) == n).all(), f"every assignment needs exactly {n} ones"
        A = torch.from_numpy(host).to(x.device)
    P = A.shape[0]
    assert A.shape[1] == n + m, f"assignments have {A.shape[1]} columns for {n} + {m} rows"
    if P > MAX_PERMUTATIONS:
        raise ValueError(f"at most {MAX_PERMUTATIONS} assignments per call, got {P}")
    lib, dev = N.lib(), x.device
    gbytes, pbytes = lib.ffd_mmd_gram_work_bytes(n, m, D), lib.ffd_mmd_permute_work_bytes(n, m, P)
    if gbytes == 0 or pbytes == 0:
        raise NotImplementedError(f"permutation_test: a shape outside the library's limits ({n}, {m}, {D}, {P})")
    gwork, pwork = _work(gbytes, dev), _work(pbytes, dev)
    out = torch.empty(P, device=dev, dtype=torch.float64)
    stream = N.current_stream_ptr(dev)
    N.check(lib.ffd_mmd_gram(x.data_ptr(), n, y.data_ptr(), m, D, c.data_ptr(), g.ctypes.data, int(g.size), gwork.data_ptr(),
                             gbytes, stream), None, "ffd_mmd_gram")
    N.check(lib.ffd_mmd_permute(gwork.data_ptr(), n, m, A.data_ptr(), P, out.data_ptr(), pwork.data_ptr(), pbytes, stream),
            None, "ffd_mmd_permute")
    return out


def p_value(statistics) -> float:
    """(1 + #{p >= 1 : T_p >= T_0}) / (P + 1) for P permuted assignments behind the observed one."""
    T = statistics.detach().cpu().numpy() if isinstance(statistics, torch.Tensor) else np.asarray(statistics, np.float64)
    return (1.0 + float((T[1:] >= T[0]).sum())) / float(len(T))
