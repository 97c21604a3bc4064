"""``fdiff.sampling.metrics`` mirror (reference src/fdiff/sampling/metrics.py:13-217): ``Metric``,
``MetricCollection``, ``SlicedWasserstein``, ``MarginalWasserstein`` with the reference's constructor arguments,
result keys and key order.  Every number comes from libffd (``utils.wasserstein``): distances, their mean / max, the
mean sample of the "dummy" baseline, ``dft`` and ``spectral_density``.  A metric object uploads its original set once
and keeps it projected and sorted between calls (the reference re-creates the same directions from its seed at every
call, metrics.py:113-119).  Each metric object holds its own upload (n x D fp32) and its own prepared buffer
(directions x n fp32, not bounded by the workspace budget): a ``MetricCollection`` built from the reference's config
holds five of each (sliced and marginal in time and frequency, marginal on the spectral density)."""
from __future__ import annotations

from abc import ABC, abstractmethod
from functools import partial

from ..utils import dtw, kernel_mmd, neighbours, pca, sinkhorn
from ..utils.fourier import dft, spectral_density
from ..utils.tensors import check_flat_array
from ..utils.wasserstein import WassersteinDistances, _column_mean, _summary, _to_device


class Metric(ABC):
    # the views of the samples a ``MetricCollection`` builds and calls this metric on
    views = ("time", "freq")

    def __init__(self, original_samples) -> None:
        self.original_samples = check_flat_array(original_samples)
        self._device_set = None
        self._prepared: dict = {}

    @abstractmethod
    def __call__(self, other_samples) -> dict: ...

    @property
    @abstractmethod
    def name(self) -> str: ...

    @property
    def baseline_metrics(self) -> dict:
        return {}

    def _original(self):
        if self._device_set is None:
            self._device_set = _to_device(self.original_samples)
        return self._device_set

    def _wd(self, original, other, cached: bool) -> WassersteinDistances:
        wd = WassersteinDistances(original_data=original, other_data=other, seed=self.random_seed)
        if cached and self.random_seed is not None:
            wd._prepared = self._prepared
        return wd

    def _baseline_sets(self):
        x = self._original()
        n = x.shape[0]
        return x[: n // 2], x[n // 2:], _column_mean(x)  # metrics.py:131-140


def _stats(wd: WassersteinDistances, distances, prefix: str, suffix: str = "", save_all: bool = False) -> dict:
    mean, mx = _summary(wd.last_distances)
    out = {f"{prefix}_mean{suffix}": float(mean), f"{prefix}_max{suffix}": float(mx)}
    if save_all:
        out[f"{prefix}_all"] = distances.tolist()
    return out


class MetricCollection:
    """metrics.py:28-97: every metric once on the time series and once on their ``dft``, optionally the marginal
    metric on the spectral densities; results under ``time_`` / ``freq_`` / ``spectral_`` prefixes, sorted by key.
    A metric class that names fewer ``views`` (``DTWMetrics``: time only) is built and called on those alone."""

    def __init__(self, metrics: list, original_samples=None, include_baselines: bool = True,
                 include_spectral_density: bool = False) -> None:
        # only partially applied metrics are built (metrics.py:43-50); anything else in the list is skipped
        todo = [m for m in metrics if isinstance(m, partial)]
        assert not todo or original_samples is not None, \
            f"Original samples must be provided for metric {todo[0] if todo else None} to be instantiated."
        in_freq = None if original_samples is None else dft(original_samples)
        takes = [getattr(build.func, "views", Metric.views) for build in todo]
        self.metrics_time = [build(original_samples=original_samples) if "time" in views else None
                             for build, views in zip(todo, takes)]
        self.metrics_freq = [build(original_samples=in_freq) if "freq" in views else None
                             for build, views in zip(todo, takes)]
        self.include_baselines = include_baselines
        self.metric_spectral = None
        if include_spectral_density:
            self.metric_spectral = MarginalWasserstein(original_samples=spectral_density(original_samples),
                                                       random_seed=42, save_all_distances=True)

    def _pairs(self):
        """(prefix, metric) in the reference's update order: time then freq, metric by metric; a metric is absent
        (None) from a view it does not take (``Metric.views``)."""
        for in_time, in_freq in zip(self.metrics_time, self.metrics_freq):
            if in_time is not None:
                yield "time", in_time
            if in_freq is not None:
                yield "freq", in_freq

    def __call__(self, other_samples) -> dict:
        views = {"time": other_samples, "freq": dft(other_samples)}
        found: dict = {}
        for prefix, metric in self._pairs():
            _merge(found, prefix, metric(views[prefix]))
        if self.include_baselines:
            found.update(self.baseline_metrics)
        if self.metric_spectral is not None:
            _merge(found, "spectral", self.metric_spectral(spectral_density(other_samples)))
        return {key: found[key] for key in sorted(found)}

    @property
    def baseline_metrics(self) -> dict:
        found: dict = {}
        for prefix, metric in self._pairs():
            _merge(found, prefix, metric.baseline_metrics)
        return found


def _merge(into: dict, prefix: str, values: dict) -> None:
    for key, value in values.items():
        into[f"{prefix}_{key}"] = value


class SlicedWasserstein(Metric):
    """metrics.py:100-158."""

    def __init__(self, original_samples, random_seed: int, num_directions: int,
                 save_all_distances: bool = False) -> None:
        super().__init__(original_samples=original_samples)
        self.random_seed = random_seed
        self.num_directions = num_directions
        self.save_all_distances = save_all_distances

    def __call__(self, other_samples) -> dict:
        wd = self._wd(self._original(), check_flat_array(other_samples), cached=True)
        distances = wd.sliced_distances(self.num_directions)
        return _stats(wd, distances, "sliced_wasserstein", save_all=self.save_all_distances)

    @property
    def baseline_metrics(self) -> dict:
        fold_a, fold_b, avg_sample = self._baseline_sets()
        wd_self = self._wd(fold_a, fold_b, cached=False)
        d_self = wd_self.sliced_distances(self.num_directions)
        wd_dummy = self._wd(self._original(), avg_sample, cached=True)
        d_dummy = wd_dummy.sliced_distances(self.num_directions)
        return {**_stats(wd_self, d_self, "sliced_wasserstein", "_self"),
                **_stats(wd_dummy, d_dummy, "sliced_wasserstein", "_dummy")}

    @property
    def name(self) -> str:
        return "sliced_wasserstein"


class MarginalWasserstein(Metric):
    """metrics.py:161-217."""

    def __init__(self, original_samples, random_seed: int, save_all_distances: bool = False) -> None:
        super().__init__(original_samples=original_samples)
        self.random_seed = random_seed
        self.save_all_distances = save_all_distances

    def __call__(self, other_samples) -> dict:
        wd = self._wd(self._original(), check_flat_array(other_samples), cached=True)
        distances = wd.marginal_distances()
        return _stats(wd, distances, "marginal_wasserstein", save_all=self.save_all_distances)

    @property
    def baseline_metrics(self) -> dict:
        fold_a, fold_b, avg_sample = self._baseline_sets()
        wd_self = self._wd(fold_a, fold_b, cached=False)
        d_self = wd_self.marginal_distances()
        wd_dummy = self._wd(self._original(), avg_sample, cached=True)
        d_dummy = wd_dummy.marginal_distances()
        return {**_stats(wd_self, d_self, "marginal_wasserstein", "_self"),
                **_stats(wd_dummy, d_dummy, "marginal_wasserstein", "_dummy")}

    @property
    def name(self) -> str:
        return "marginal_wasserstein"


class ManifoldMetrics(Metric):
    """Nearest-neighbour statistics of a sample set X against the originals Y (``utils.neighbours``; not in the
    reference, whose metrics are Wasserstein distances only): improved precision / recall (Kynkaanniemi et al. 2019),
    density / coverage (Naeem et al. 2020), authenticity (Alaa et al. 2022), the distance to the nearest original and
    the share of exact copies.  With r_k(y) the distance from y to its k-th neighbour inside Y (itself excluded) and
    rho_k(x) likewise inside X:

    ``precision`` share of x inside some ball (y, r_k(y)); ``recall`` share of y inside some ball (x, rho_k(x));
    ``density`` the balls (y, r_k(y)) holding x, summed over x, over k m; ``coverage`` share of y whose nearest x lies
    within r_k(y); ``authenticity`` share of x further from their nearest original y* than r_1(y*);
    ``nn_distance_mean`` / ``nn_distance_min`` over x of the distance to Y; ``copy_share`` share of x at distance 0.

    The originals' self-search is done once and kept, as ``SlicedWasserstein`` keeps its prepared set.  There is no
    ``_dummy`` baseline: a single mean sample has no rho_k."""

    def __init__(self, original_samples, k: int = 5) -> None:
        super().__init__(original_samples=original_samples)
        assert 1 <= int(k) <= neighbours.MAX_K, f"k must lie in [1, {neighbours.MAX_K}], got {k}"
        self.k = int(k)
        assert self.original_samples.shape[0] >= self.k + 1, \
            f"k = {self.k} needs at least {self.k + 1} original samples, got {self.original_samples.shape[0]}"
        self._original_self = None

    def __call__(self, other_samples) -> dict:
        other = check_flat_array(other_samples)
        assert other.shape[0] >= self.k + 1, f"k = {self.k} needs at least {self.k + 1} samples, got {other.shape[0]}"
        if self._original_self is None:
            self._original_self = neighbours.self_search(self._original(), self.k)
        return neighbours.manifold_scores(self._original(), other, self.k, original_self=self._original_self)

    @property
    def baseline_metrics(self) -> dict:
        x = self._original()
        fold_a, fold_b = x[: x.shape[0] // 2], x[x.shape[0] // 2:]  # the cut of _baseline_sets, without its mean sample
        for fold in (fold_a, fold_b):
            assert fold.shape[0] >= self.k + 1, f"k = {self.k} needs at least {self.k + 1} rows in each half, got {fold.shape[0]}"
        found = neighbours.manifold_scores(fold_a, fold_b, self.k)
        return {f"{key}_self": value for key, value in found.items()}

    @property
    def name(self) -> str:
        return "manifold"


class KernelMMD(Metric):
    """Kernel two-sample statistics of a sample set X against the originals Y (``utils.kernel_mmd``; not in the reference):
    the maximum mean discrepancy with Gaussian kernels exp(-gamma |a - b|^2) (Gretton et al. 2012), per-sample witness
    values and, on request, a permutation test.  The bandwidths are the ladder gamma_s = 1 / (2 sigma^2 s) over ``scales``
    around sigma^2, the originals' mean squared distance between two distinct rows; the headline numbers use the mean
    kernel over the ladder.

    ``mmd2`` the unbiased estimate (expectation 0 when X and Y share a distribution, so it may be negative);
    ``mmd2_biased`` the biased one (>= 0); ``mmd2_s{scale}`` the unbiased estimate at one bandwidth; ``witness_max`` and
    ``witness_share_positive`` over the per-sample values w_i = mean_x' k(x_i, x') - mean_y k(x_i, y), large where the
    samples lie and the originals do not; with ``permutations`` > 0, ``p_value`` = (1 + #{p : T_p >= T_0}) / (P + 1) over
    P relabelings of the pooled rows drawn on the host from ``random_seed``.

    The originals' centre, sigma^2 and self row sums are computed once and kept, as ``ManifoldMetrics`` keeps its
    self-search.  There is no ``_dummy`` baseline.  A permutation test takes at most ``kernel_mmd.MAX_POOLED`` rows of both
    sets together; larger sets are refused, never subsampled silently."""

    def __init__(self, original_samples, scales=kernel_mmd.DEFAULT_SCALES, permutations: int = 0,
                 random_seed: int = 0) -> None:
        super().__init__(original_samples=original_samples)
        self.scales = tuple(float(s) for s in scales)
        assert 1 <= len(self.scales) <= kernel_mmd.MAX_GAMMAS, \
            f"between 1 and {kernel_mmd.MAX_GAMMAS} scales, got {len(self.scales)}"
        assert all(s > 0 for s in self.scales), f"scales must be positive, got {self.scales}"
        self.permutations = int(permutations)
        assert 0 <= self.permutations < kernel_mmd.MAX_PERMUTATIONS, \
            f"permutations must lie in [0, {kernel_mmd.MAX_PERMUTATIONS - 1}], got {permutations}"
        self.random_seed = int(random_seed)
        assert self.original_samples.shape[0] >= 2, "KernelMMD needs at least 2 original samples"
        self._cache = None
        self._baseline = None

    def _prepared_originals(self):
        """(centre, gammas, YY row sums) of the originals, computed once."""
        if self._cache is None:
            y = self._original()
            centre = kernel_mmd.column_mean(y)
            gammas = kernel_mmd.ladder_gammas(float(kernel_mmd.bandwidth(y).item()), self.scales)
            self._cache = (centre, gammas, kernel_mmd.row_sums(y, y, centre, gammas, exclude_self=True))
        return self._cache

    def _check_pooled(self, n: int, m: int) -> None:
        if self.permutations > 0 and n + m > kernel_mmd.MAX_POOLED:
            raise ValueError(f"a permutation test takes at most {kernel_mmd.MAX_POOLED} rows of both sets together, got "
                             f"{n} samples + {m} originals; pass subsamples or permutations=0")

    def _evaluate(self, x, y, centre, gammas, rowsum_yy, with_test: bool = True):
        n, m = x.shape[0], y.shape[0]
        assert n >= 2 and m >= 2, f"both sets need at least 2 rows, got {n} and {m}"
        self._check_pooled(n, m)
        rowsum_xx = kernel_mmd.row_sums(x, x, centre, gammas, exclude_self=True)
        rowsum_xy = kernel_mmd.row_sums(x, y, centre, gammas)
        mmd2, witness = kernel_mmd.mmd_scores(rowsum_xx, rowsum_xy, rowsum_yy)
        unbiased, biased = mmd2.tolist()
        found = {"mmd2": unbiased[-1], "mmd2_biased": biased[-1]}
        for scale, value in zip(self.scales, unbiased):
            found[f"mmd2_s{scale:g}"] = value
        found["witness_max"] = float(witness.max())  # two reductions where the values live: n doubles stay there
        found["witness_share_positive"] = float((witness > 0).sum()) / n
        if with_test and self.permutations > 0:
            assign = kernel_mmd.permutation_assignments(n, m, self.permutations, self.random_seed)
            found["p_value"] = kernel_mmd.p_value(kernel_mmd.permutation_test(x, y, centre, gammas, assign))
        return found, witness

    def __call__(self, other_samples) -> dict:
        centre, gammas, rowsum_yy = self._prepared_originals()
        return self._evaluate(_to_device(check_flat_array(other_samples)), self._original(), centre, gammas, rowsum_yy)[0]

    def witness(self, other_samples):
        """The per-sample witness values of the mean kernel, a float64 (n,) device tensor."""
        centre, gammas, rowsum_yy = self._prepared_originals()
        return self._evaluate(_to_device(check_flat_array(other_samples)), self._original(), centre, gammas, rowsum_yy,
                              with_test=False)[1]

    @property
    def baseline_metrics(self) -> dict:
        if self._baseline is None:  # a function of the originals alone: computed once, as their row sums are
            y = self._original()
            fold_a, fold_b = y[: y.shape[0] // 2], y[y.shape[0] // 2:]  # the cut of ManifoldMetrics.baseline_metrics
            centre, gammas, _ = self._prepared_originals()  # the whole set's centre and bandwidths: comparable with __call__
            fold_a = fold_a.contiguous()
            found, _ = self._evaluate(fold_b.contiguous(), fold_a, centre, gammas,
                                      kernel_mmd.row_sums(fold_a, fold_a, centre, gammas, exclude_self=True))
            self._baseline = {f"{key}_self": value for key, value in found.items()}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "kernel_mmd"


class SinkhornDivergence(Metric):
    """The debiased entropic optimal-transport cost of a sample set X against the originals Y (``utils.sinkhorn``; not in
    the reference, which slices because the full transport problem is out of reach on a host): the Sinkhorn divergence
    S_eps(X, Y) = OT_eps(X, Y) - OT_eps(X, X) / 2 - OT_eps(Y, Y) / 2 of the squared Euclidean cost with uniform weights
    (Genevay, Peyre, Cuturi 2018; Feydy et al. 2019).  It is 0 for equal sets, tends to W_2^2 as eps -> 0 and to an MMD
    as eps -> infinity.  eps = ``blur``^2 sigma^2 with sigma^2 the originals' mean squared distance between two distinct
    rows (``kernel_mmd.bandwidth``): ``blur`` is the resolution as a share of the data's own scale.

    ``sinkhorn_divergence`` S; ``sinkhorn_distance`` sqrt(max(S, 0)); ``sinkhorn_ot`` the undebiased OT_eps(X, Y);
    ``sinkhorn_change`` the largest change of a cross potential in the last damped pass, on the cost's scale: the
    schedule's own statement of convergence; ``sinkhorn_eps`` the final eps.

    The schedule -- eps from the originals' diameter^2 = 4 max_j |y_j - centre|^2 down by ``scaling``^2 per pass to the
    final eps, then ``n_final`` passes there -- depends on the originals alone, so their self potential is computed once
    and kept, as ``ManifoldMetrics`` keeps its self-search.  Samples that spread wider than the data start above the
    schedule's first eps: that shows as a large ``sinkhorn_change``, never as a silent error.  A call runs the x|y, y|x
    and x|x softmins per schedule entry, 2 n m + n^2 pairs each time; the originals' m^2 once.  There is no ``_dummy``
    baseline."""

    def __init__(self, original_samples, blur: float = 0.05, scaling: float = 0.5, n_final: int = 3) -> None:
        super().__init__(original_samples=original_samples)
        self.blur, self.scaling, self.n_final = float(blur), float(scaling), int(n_final)
        assert self.blur > 0.0 and self.blur < float("inf"), f"blur must be positive and finite, got {blur}"
        assert 0.0 < self.scaling < 1.0, f"scaling must lie in (0, 1), got {scaling}"
        assert self.n_final >= 1, f"n_final must be at least 1, got {n_final}"
        assert self.original_samples.shape[0] >= 2, "SinkhornDivergence needs at least 2 original samples"
        self._cache = None
        self._baseline = None

    def _prepared_originals(self):
        """(centre, schedule, self potential) of the originals, computed once."""
        if self._cache is None:
            y = self._original()
            centre = kernel_mmd.column_mean(y)
            eps = self.blur * self.blur * float(kernel_mmd.bandwidth(y).item())
            schedule = sinkhorn.schedule(float(sinkhorn.diameter2(y, centre).item()), eps, self.scaling, self.n_final)
            self._cache = (centre, schedule, sinkhorn.self_potential(y, centre, schedule))
        return self._cache

    def _evaluate(self, x, y, centre, schedule, q):
        found = sinkhorn.sinkhorn_divergence(x, y, centre, schedule, q=q)
        return {"sinkhorn_divergence": found.divergence, "sinkhorn_distance": max(found.divergence, 0.0) ** 0.5,
                "sinkhorn_ot": found.ot_xy, "sinkhorn_change": found.change, "sinkhorn_eps": float(schedule[-1])}, found

    def __call__(self, other_samples) -> dict:
        centre, schedule, q = self._prepared_originals()
        return self._evaluate(_to_device(check_flat_array(other_samples)), self._original(), centre, schedule, q)[0]

    def transport_price(self, other_samples):
        """f - p per sample, a float64 (n,) device tensor: what moving sample i to the originals costs beyond what moving
        it inside its own set costs; large where the samples lie and the originals do not."""
        centre, schedule, q = self._prepared_originals()
        found = self._evaluate(_to_device(check_flat_array(other_samples)), self._original(), centre, schedule, q)[1]
        return found.f - found.p

    @property
    def baseline_metrics(self) -> dict:
        if self._baseline is None:  # a function of the originals alone: computed once
            y = self._original()
            fold_a, fold_b = y[: y.shape[0] // 2], y[y.shape[0] // 2:]  # the cut of ManifoldMetrics.baseline_metrics
            centre, schedule, _ = self._prepared_originals()  # the whole set's centre and schedule: comparable with __call__
            found, _ = self._evaluate(fold_b.contiguous(), fold_a.contiguous(), centre, schedule, None)
            self._baseline = {f"{key}_self": value for key, value in found.items()}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "sinkhorn"


class FrechetDistance(Metric):
    """The Frechet distance of a sample set X against the originals Y (``utils.pca``; not in the reference): the exact
    W_2^2 between the Gaussians fitted to the two sets, the quantity behind FID (Dowson & Landau 1982; Heusel et al. 2017),
    FD = |mu_x - mu_y|^2 + tr S_x + tr S_y - 2 tr (S_y^1/2 S_x S_y^1/2)^1/2, and the samples' variance along the data's
    principal axes.  All of it is float64 on the device.

    ``frechet_distance`` FD; ``frechet_w2`` sqrt(max(FD, 0)); ``frechet_mean_term`` and ``frechet_cov_term`` its two
    parts: whether an error sits in the first or the second moment; ``variance_ratio`` tr S_x / tr S_y;
    ``pc_variance_ratio_min`` / ``pc_variance_ratio_max`` over the data's top ``components`` axes v_i of
    v_i^T S_x v_i / lambda_i: under- or over-dispersion per mode (1 for samples that spread as the data does).

    The originals' mean, covariance, eigenpairs and root are computed once and kept, as ``KernelMMD`` keeps its row sums.
    FD of finite samples is biased upward: ``baseline_metrics`` (the ``_self`` keys, one half of the originals against the
    other) is its zero point.  There is no ``_dummy`` baseline: a single mean sample has no covariance."""

    def __init__(self, original_samples, components: int = 10) -> None:
        super().__init__(original_samples=original_samples)
        self.components = int(components)
        assert self.components >= 1, f"components must be at least 1, got {components}"
        n, D = self.original_samples.shape
        assert n >= 2, "FrechetDistance needs at least 2 original samples"
        assert D <= pca.MAX_D, f"FrechetDistance takes at most {pca.MAX_D} features, got {D}"
        self._cache = None
        self._baseline = None

    @staticmethod
    def _moments(y):
        """(mean, covariance, eigenvalues, eigenvectors, root) of a device set."""
        mean, cov = pca.covariance(y)
        w, v = pca.eigh(cov)
        return mean, cov, w, v, pca.sym_root(w, v)

    def _prepared_originals(self):
        if self._cache is None:
            self._cache = self._moments(self._original())
        return self._cache

    def _evaluate(self, x, prepared) -> dict:
        assert x.shape[0] >= 2, f"FrechetDistance needs at least 2 samples, got {x.shape[0]}"
        mean_y, cov_y, w, v, root = prepared
        mean_x, cov_x = pca.covariance(x)
        found = pca.frechet_distance(mean_x, cov_x, mean_y, cov_y, root_y=root)
        k = min(self.components, w.shape[0])
        ratios = pca.pc_variances(cov_x, v, k) / w.flip(0)[:k]
        return {"frechet_distance": found.distance, "frechet_w2": max(found.distance, 0.0) ** 0.5,
                "frechet_mean_term": found.mean_term, "frechet_cov_term": found.cov_term,
                "variance_ratio": found.trace_x / found.trace_y if found.trace_y != 0.0 else float("nan"),
                "pc_variance_ratio_min": float(ratios.min()), "pc_variance_ratio_max": float(ratios.max())}

    def __call__(self, other_samples) -> dict:
        return self._evaluate(_to_device(check_flat_array(other_samples)), self._prepared_originals())

    def transform(self, samples, k: int = 2):
        """The scores of ``samples`` on the data's ``k`` main axes (centred on the data's mean), float64 (n, k) on the
        device: what the PCA scatter plot shows."""
        mean_y, _, _, v, _ = self._prepared_originals()
        return pca.transform(_to_device(check_flat_array(samples)), mean_y, v, k)

    def explained_variance(self):
        """The data's variance spectrum, the largest first: float64 (D,) on the device."""
        return self._prepared_originals()[2].flip(0)

    @property
    def baseline_metrics(self) -> dict:
        if self._baseline is None:  # a function of the originals alone: computed once
            y = self._original()
            fold_a, fold_b = y[: y.shape[0] // 2], y[y.shape[0] // 2:]  # the cut of ManifoldMetrics.baseline_metrics
            assert fold_a.shape[0] >= 2, f"the baseline needs at least 2 rows in each half, got {fold_a.shape[0]}"
            found = self._evaluate(fold_b.contiguous(), self._moments(fold_a.contiguous()))
            self._baseline = {f"{key}_self": value for key, value in found.items()}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "frechet"


class DTWMetrics(Metric):
    """Dynamic-time-warping statistics of a sample set X against the originals Y (``utils.dtw``; not in the reference): what
    the flat-vector metrics cannot tell apart, a sample of the wrong shape from one that is only mis-timed.  ``dtw2`` is
    the squared banded DTW cost at the Sakoe-Chiba half-width ``window`` (an int in samples, or a float share of the
    length); d(a, S) below is the square root of the smallest ``dtw2`` from a to a row of S (a itself excluded inside its
    own set).

    ``dtw_nn_distance_mean`` mean over x of d(x, Y); ``dtw_coverage_distance_mean`` mean over y of d(y, X);
    ``dtw_warp_gain`` 1 - mean over the x with Euclidean nearest-original distance > 0 of d(x, Y) over that Euclidean
    distance: the share of the nearest-original distance that re-timing removes, in [0, 1], 0 at window 0 and 0.0 when no
    x qualifies; ``dtw_1nn_accuracy_samples`` share of x with d(x, X) < d(x, Y) and ``dtw_1nn_accuracy_originals`` share
    of y with d(y, Y) < d(y, X) (strict: a tie counts as the other class); ``dtw_1nn_accuracy`` their mean, the
    leave-one-out 1-NN two-sample accuracy (Lopez-Paz & Oquab 2017) balanced over the classes: 0.5 means "cannot be told
    apart".

    The originals must be (n, L, C); samples may be (m, L, C) or (m, L C).  The originals' self-search is done once and
    kept, as ``ManifoldMetrics`` keeps its own.  The originals are used as given and never subsampled silently: a call
    computes every pair of five searches, (n + m)^2 L (2 w + 1) cells, and the kept self-search n^2 of them.  Over the
    packed spectrum DTW means nothing, so a ``MetricCollection`` builds this metric on the time view only.  There is no
    ``_dummy`` baseline."""

    views = ("time",)

    def __init__(self, original_samples, window=0.1) -> None:
        shape = tuple(original_samples.shape)
        assert len(shape) == 3, f"DTWMetrics needs the originals as (n, L, C), got {shape}"
        super().__init__(original_samples=original_samples)
        self.length, self.channels = shape[1], shape[2]
        assert shape[0] >= 2, f"DTWMetrics needs at least 2 original samples, got {shape[0]}"
        self.window = dtw.resolve_window(window, self.length)
        self._original_self = None

    def _as_series(self, flat):
        assert flat.shape[1] == self.length * self.channels, \
            f"samples of {flat.shape[1]} values against originals of ({self.length}, {self.channels})"
        return flat.reshape(flat.shape[0], self.length, self.channels)

    def __call__(self, other_samples) -> dict:
        other = check_flat_array(other_samples)
        assert other.shape[0] >= 2, f"DTWMetrics needs at least 2 samples, got {other.shape[0]}"
        y = self._as_series(self._original())
        if self._original_self is None:
            self._original_self = dtw.self_search(y, self.window)
        return dtw.dtw_scores(y, self._as_series(_to_device(other)), self.window, original_self=self._original_self)

    @property
    def baseline_metrics(self) -> dict:
        y = self._as_series(self._original())
        fold_a, fold_b = y[: y.shape[0] // 2], y[y.shape[0] // 2:]  # the cut of ManifoldMetrics.baseline_metrics
        for fold in (fold_a, fold_b):
            assert fold.shape[0] >= 2, f"DTWMetrics needs at least 2 rows in each half, got {fold.shape[0]}"
        found = dtw.dtw_scores(fold_a, fold_b, self.window)
        return {f"{key}_self": value for key, value in found.items()}

    @property
    def name(self) -> str:
        return "dtw"
