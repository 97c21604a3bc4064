"""Host side of the sample metrics (no GPU): the mirror's import paths and signatures, the direction generator, the
metrics config, the refusal of host data without a device -- and the closed form the GPU tests compare against,
checked once against a restatement of POT's greedy 1-D transport."""
import functools
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def w2sq_sorted(a, b):
    """W2^2 of two sorted float64 samples with uniform weights: the integral of the squared quantile difference over
    the intervals between the breakpoints {i/n} U {j/m}, on the integer grid n*m (what ot.emd2_1d returns)."""
    n, m = len(a), len(b)
    bp = np.unique(np.concatenate([np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n]))
    lo, hi = bp[:-1], bp[1:]
    return float(np.sum((hi - lo) * (a[lo // m] - b[lo // n]) ** 2) / (n * m))


def greedy_emd2(a, b):
    """POT's sorted 1-D transport loop restated (weights 1/n and 1/m, squared-distance cost)."""
    n, m = len(a), len(b)
    i = j = 0
    wi, wj, cost = 1.0 / n, 1.0 / m, 0.0
    while True:
        if wi <= wj or j == m - 1:
            cost += wi * (a[i] - b[j]) ** 2
            wj -= wi
            i += 1
            if i == n:
                return cost
            wi = 1.0 / n
        else:
            cost += wj * (a[i] - b[j]) ** 2
            wi -= wj
            j += 1
            if j == m:
                return cost
            wj = 1.0 / m


def test_closed_form_equals_greedy_transport():
    rs = np.random.RandomState(0)
    for n, m in ((37, 101), (101, 37), (64, 64), (50, 1), (7, 1000)):
        a, b = np.sort(rs.randn(n)), np.sort(rs.randn(m) + 0.3)
        assert abs(w2sq_sorted(a, b) - greedy_emd2(a, b)) <= 1e-14 * max(1.0, greedy_emd2(a, b)), (n, m)
    a = np.sort(rs.randn(40))
    assert abs(w2sq_sorted(a, np.array([0.2])) - np.mean((a - 0.2) ** 2)) <= 1e-15  # m = 1
    assert abs(w2sq_sorted(a, a[::-1][::-1]) - 0.0) == 0.0


def test_mirror_modules_and_signatures():
    import fastfourierdiffusion_amd as pkg

    pkg.install_as_fdiff(force=True)
    from fdiff.sampling.metrics import MarginalWasserstein, Metric, MetricCollection, SlicedWasserstein
    from fdiff.utils.tensors import check_flat_array
    from fdiff.utils.wasserstein import WassersteinDistances

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]

    E = inspect.Parameter.empty
    # wasserstein.py:30-36, metrics.py:29-35, 101-107, 162-167
    assert sig(WassersteinDistances.__init__) == [("original_data", E), ("other_data", E), ("normalisation", "none"),
                                                  ("seed", None)]
    assert sig(MetricCollection.__init__) == [("metrics", E), ("original_samples", None), ("include_baselines", True),
                                              ("include_spectral_density", False)]
    assert sig(SlicedWasserstein.__init__) == [("original_samples", E), ("random_seed", E), ("num_directions", E),
                                               ("save_all_distances", False)]
    assert sig(MarginalWasserstein.__init__) == [("original_samples", E), ("random_seed", E),
                                                 ("save_all_distances", False)]
    assert sig(Metric.__init__) == [("original_samples", E)]
    for meth in ("random_direction", "get_random_directions", "get_marginal_directions", "feature_distance",
                 "directional_distance", "sliced_distances", "marginal_distances"):
        assert callable(getattr(WassersteinDistances, meth))
    assert SlicedWasserstein(np.zeros((4, 2, 1)), 1, 3).name == "sliced_wasserstein"
    assert MarginalWasserstein(np.zeros((4, 2, 1)), 1).name == "marginal_wasserstein"
    # tensors.py:5-22
    assert check_flat_array(np.zeros((5, 3, 2))).shape == (5, 6)
    flat = check_flat_array(torch.zeros(5, 3, 2))
    assert isinstance(flat, np.ndarray) and flat.shape == (5, 6)
    with pytest.raises(AssertionError):
        check_flat_array(np.zeros(5))


def test_directions_follow_the_reference_generator():
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    x = np.zeros((3, 11), dtype=np.float32)
    got = WassersteinDistances(x, x, seed=42).get_random_directions(5)
    rng = np.random.default_rng(42)
    for g in got:
        v = rng.normal(size=11)
        assert g.dtype == np.float64 and np.array_equal(g, v / np.linalg.norm(v))
    marg = WassersteinDistances(x, x, seed=42).get_marginal_directions()
    assert np.array_equal(np.stack(marg), np.identity(11))


def test_metrics_config_instantiates():
    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd.sampling import metrics as M
    from fastfourierdiffusion_amd.utils.extraction import instantiate

    pkg.install_as_fdiff(force=True)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "metrics_conf.json")))
    for m in cfg["metrics"]:
        assert m["random_seed"] == "${random_seed}"
        m["random_seed"] = 42  # cmd/conf/sample.yaml
    coll = instantiate(cfg)
    assert isinstance(coll, functools.partial) and coll.func is M.MetricCollection
    assert coll.keywords["include_baselines"] is True and coll.keywords["include_spectral_density"] is True
    sw, mw = coll.keywords["metrics"]
    assert isinstance(sw, functools.partial) and sw.func is M.SlicedWasserstein
    assert sw.keywords == {"random_seed": 42, "num_directions": 1000, "save_all_distances": True}
    assert isinstance(mw, functools.partial) and mw.func is M.MarginalWasserstein
    assert mw.keywords == {"random_seed": 42, "save_all_distances": True}


def test_unknown_normalisation_raises_value_error():
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    x = np.zeros((3, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="Unrecognised normalisation type"):
        WassersteinDistances(x, x, normalisation="minmax", seed=0).sliced_distances(2)


def test_host_arrays_without_a_device_are_refused():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fastfourierdiffusion_amd._native import FFDError
    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    x = np.random.RandomState(0).rand(16, 3, 1).astype(np.float32)
    with pytest.raises(FFDError):
        WassersteinDistances(x.reshape(16, 3), x.reshape(16, 3), seed=0).sliced_distances(4)
    with pytest.raises(FFDError):
        WassersteinDistances(x.reshape(16, 3), x.reshape(16, 3), seed=0).marginal_distances()
    with pytest.raises(FFDError):
        SlicedWasserstein(x, 0, 4)(torch.from_numpy(x))
    with pytest.raises(FFDError):
        MarginalWasserstein(x, 0).baseline_metrics
    with pytest.raises(FFDError):
        MetricCollection([], original_samples=torch.from_numpy(x))


def test_context_free_entry_points_validate_arguments():
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    assert lib.ffd_w2_work_bytes(100, 40, 8, 10, 1 << 30) == 10 * 4 * (100 + 40 + 100)
    assert lib.ffd_w2_work_bytes(100, 40, 8, 10, 7 * 4 * 240) == 7 * 4 * 240  # blocks of 7 directions
    assert lib.ffd_w2_work_bytes(100, 40, 8, 10, 0) == 4 * 240                 # at least one direction
    assert lib.ffd_w2_work_bytes(100, 0, 8, 10, 1 << 30) == 10 * 4 * 100       # prepare
    assert lib.ffd_w2_work_bytes(0, 40, 8, 10, 1 << 30) == 10 * 4 * 80         # against prepared
    assert lib.ffd_col_mean_work_bytes(2049, 5) == 3 * 5 * 8
    p = 4096  # never dereferenced: the calls below fail validation first
    assert lib.ffd_w2_sliced(p, 0, p, 4, 2, p, 3, 0, p, p, 1 << 20, None) == -1
    assert lib.ffd_w2_sliced(p, 4, p, 4, 2, p, 0, 0, p, p, 1 << 20, None) == -1
    assert lib.ffd_w2_sliced(p, 4, p, 4, 2, p, 3, 0, p, p, 8, None) == -1          # work buffer too small
    assert lib.ffd_w2_sliced(p, 4, p, 4, 2, p, (1 << 20) + 1, 0, p, p, 1 << 20, None) == -2
    assert lib.ffd_w2_marginal(p, 4, p, 4, 0, 0, p, p, 1 << 20, None) == -1
    assert lib.ffd_w2_prepare(p, 4, 3, None, 2, p, p, 1 << 20, None) == -1          # marginal needs K == D
    assert lib.ffd_w2_summary(p, 0, p, None) == -1
    assert lib.ffd_col_mean(p, 4, 2, p, p, 0, None) == -1
