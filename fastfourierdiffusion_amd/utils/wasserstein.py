"""``fdiff.utils.wasserstein`` mirror (reference src/fdiff/utils/wasserstein.py:12-199): sliced and marginal
Wasserstein-2 distances between two sample sets, computed on the device by libffd (csrc/ffd_metrics.hip).

The reference projects with numpy and hands each pair of projections to POT's ``ot.emd2_1d``; with uniform weights
that transport cost has a closed form (the integral of the squared difference of the two quantile functions), which
is what ``ffd_w2_*`` evaluate: projection on the exact-fp32 matrix cores, a segmented sort, an fp64 quantile integral.
numpy only draws the directions (``np.random.default_rng(seed).normal``, one draw per direction, normalised in fp64:
the reference's generator sequence, wasserstein.py:56-59) -- never a distance.

Inputs may be numpy arrays, host tensors or device tensors; host data is uploaded once per object, device tensors are
used in place.  Data and directions are fp32 on the device: float64 input is rounded to fp32 at upload (the reference
computes in fp64 from whatever dtype it is given).  NaN input gives unspecified results (as it does in the reference).
Without libffd.so or a gfx950 device every distance raises ``FFDError``: there is no numpy fallback.
"""
from __future__ import annotations

import hashlib
from typing import Optional

import numpy as np
import torch

from .. import _native as N

# most device scratch one call asks for; more directions than fit are processed in blocks (no result depends on it)
WORK_BUDGET_BYTES = 1 << 30


def _to_device(x) -> torch.Tensor:
    """(n, D) fp32 contiguous device tensor of a numpy array / host tensor / device tensor."""
    if isinstance(x, torch.Tensor) and x.device.type == "cuda":
        t = x.detach()
    else:
        if not torch.cuda.is_available():
            raise N.FFDError("the Wasserstein metrics need an MI355X (gfx950) device; there is no CPU fallback")
        if isinstance(x, torch.Tensor):
            t = x.detach().to(torch.float32).to("cuda")
        else:
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda")
    assert t.dim() == 2, f"expected a 2d array, got {t.dim()}d"
    return t.to(torch.float32).contiguous()


def _work(nbytes: int, device) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 8) + 7) // 8, device=device, dtype=torch.float64)


def _column_mean(x: torch.Tensor) -> torch.Tensor:
    """(1, D) mean sample of a device set (``ffd_col_mean``: fp64 sums in a fixed order)."""
    n, D = x.shape
    lib = N.lib()
    out = torch.empty((1, D), device=x.device, dtype=torch.float32)
    nbytes = lib.ffd_col_mean_work_bytes(n, D)
    work = _work(nbytes, x.device)
    N.check(lib.ffd_col_mean(x.data_ptr(), n, D, out.data_ptr(), work.data_ptr(), nbytes,
                             N.current_stream_ptr(x.device)), None, "ffd_col_mean")
    return out


def _summary(dist: torch.Tensor) -> tuple:
    """(mean, max) of a device vector of distances (``ffd_w2_summary``)."""
    out = torch.empty(2, device=dist.device, dtype=torch.float64)
    N.check(N.lib().ffd_w2_summary(dist.data_ptr(), dist.numel(), out.data_ptr(), N.current_stream_ptr(dist.device)),
            None, "ffd_w2_summary")
    mean, mx = out.tolist()
    return mean, mx


class WassersteinDistances:
    """wasserstein.py:12-40.  ``original_data`` / ``other_data``: (n, d) and (m, d)."""

    def __init__(self, original_data, other_data, normalisation: Optional[str] = "none",
                 seed: Optional[int] = None) -> None:
        self.original_data = original_data
        self.other_data = other_data
        self.normalisation = normalisation
        self.rng = np.random.default_rng(seed)
        self._dev: dict = {}
        self._prepared: Optional[dict] = None  # a Metric's cache of its projected + sorted original set
        self.last_distances: Optional[torch.Tensor] = None  # device copy of the last result

    # -- directions (host, the reference's generator sequence) --
    def random_direction(self, dim: int) -> np.ndarray:
        """wasserstein.py:42-59."""
        vector = self.rng.normal(size=dim)
        return vector / np.linalg.norm(vector)

    def get_random_directions(self, n_directions: int) -> list:
        """wasserstein.py:61-78: ``n_directions`` unit vectors of the data's dimension, in drawing order."""
        out: list = []
        while len(out) < n_directions:
            out.append(self.random_direction(self._dim()))
        return out

    def get_marginal_directions(self) -> list:
        """wasserstein.py:80-93: the standard basis."""
        return list(np.eye(self._dim()))

    def _dim(self) -> int:
        return int(self.original_data.shape[1])

    # -- device plumbing --
    def _standardise(self) -> int:
        if self.normalisation == "none":
            return 0
        if self.normalisation == "standardise":
            return 1
        raise ValueError(f"Unrecognised normalisation type: {self.normalisation}")  # wasserstein.py:160

    def _set(self, which: str) -> torch.Tensor:
        if which not in self._dev:
            self._dev[which] = _to_device(self.original_data if which == "orig" else self.other_data)
        return self._dev[which]

    def _distances(self, dirs: Optional[np.ndarray]) -> np.ndarray:
        """dirs (K, D) fp64 host, or None for the marginal case.  With ``_prepared`` set (a Metric's cache) the
        original set is projected and sorted once per distinct set of directions -- the cache is keyed by the fp32
        directions themselves -- and kept as a (K, n) fp32 device buffer, which the workspace budget does not bound
        (n = 10^6, K = 1000: 4 GB); without it both sets go through the budgeted one-shot entry points."""
        std = self._standardise()
        a, b = self._set("orig"), self._set("other")
        n, D = a.shape
        m = b.shape[0]
        assert b.shape[1] == D, f"the two sets have {D} and {b.shape[1]} features"
        lib, dev = N.lib(), a.device
        stream = N.current_stream_ptr(dev)
        if dirs is None:
            K, U, uptr = D, None, None
        else:
            U = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)).to(dev)
            K, uptr = U.shape[0], U.data_ptr()
        dist = torch.empty(K, device=dev, dtype=torch.float64)
        if self._prepared is not None:
            key = ("marginal", n, D) if U is None else \
                ("sliced", n, hashlib.sha1(U.cpu().numpy().tobytes()).hexdigest())
            if key not in self._prepared:
                prep = torch.empty((K, n), device=dev, dtype=torch.float32)
                nbytes = lib.ffd_w2_work_bytes(n, 0, D, K, WORK_BUDGET_BYTES)
                work = _work(nbytes, dev)
                N.check(lib.ffd_w2_prepare(a.data_ptr(), n, D, uptr, K, prep.data_ptr(), work.data_ptr(), nbytes, stream),
                        None, "ffd_w2_prepare")
                self._prepared[key] = prep
            prep = self._prepared[key]
            nbytes = lib.ffd_w2_work_bytes(0, m, D, K, WORK_BUDGET_BYTES)
            work = _work(nbytes, dev)
            N.check(lib.ffd_w2_against_prepared(prep.data_ptr(), n, b.data_ptr(), m, D, uptr, K, std, dist.data_ptr(),
                                                work.data_ptr(), nbytes, stream), None, "ffd_w2_against_prepared")
        else:
            nbytes = lib.ffd_w2_work_bytes(n, m, D, K, WORK_BUDGET_BYTES)
            work = _work(nbytes, dev)
            if dirs is None:
                rc = lib.ffd_w2_marginal(a.data_ptr(), n, b.data_ptr(), m, D, std, dist.data_ptr(), work.data_ptr(),
                                         nbytes, stream)
            else:
                rc = lib.ffd_w2_sliced(a.data_ptr(), n, b.data_ptr(), m, D, uptr, K, std, dist.data_ptr(),
                                       work.data_ptr(), nbytes, stream)
            N.check(rc, None, "ffd_w2_marginal" if dirs is None else "ffd_w2_sliced")
        self.last_distances = dist
        return dist.cpu().numpy()

    # -- the reference's methods --
    def feature_distance(self, feature: int) -> float:
        """wasserstein.py:95-118: the marginal path on that one column (no product, so an inf elsewhere in a row
        does not reach it)."""
        cols = [self._set(w)[:, feature:feature + 1] for w in ("orig", "other")]
        return float(WassersteinDistances(cols[0], cols[1], self.normalisation).marginal_distances()[0])

    def directional_distance(self, direction: np.ndarray) -> float:
        """wasserstein.py:120-144."""
        return float(self._distances(np.asarray(direction, dtype=np.float64)[None, :])[0])

    def sliced_distances(self, num_directions: int) -> np.ndarray:
        """wasserstein.py:162-181."""
        directions = self.get_random_directions(num_directions)
        return self._distances(np.stack(directions))

    def marginal_distances(self) -> np.ndarray:
        """wasserstein.py:183-199."""
        return self._distances(None)
