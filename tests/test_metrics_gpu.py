"""GPU tests of the sample metrics: every value goes through the Python mirror, so through the C ABI
(ffd_w2_sliced / _marginal / _prepare / _against_prepared / _summary, ffd_col_mean).

Comparator: the reference's arithmetic in float64 numpy with POT's 1-D transport replaced by its closed form
(test_metrics_host.py checks that form against a restatement of POT's greedy loop).  It never calls the code under
test.  Bound: |d_gpu - d_ref| <= TOL_OP * scale per direction and for _mean / _max, TOL_OP = 2e-6 as for every single
operator of this project, scale = max |projection| over both sets (W2 moves by at most the RMS perturbation of the
points; fp32 projection alone costs 1e-8 .. 1e-7 of the scale at these shapes).

Not run: the reference's comparison with ot.sliced.sliced_wasserstein_distance (tests/test_metrics.py:52) -- POT is
not available; its other assertions are test_reference_invariants."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


# ---- comparator (float64 numpy) ----
def w2sq_sorted(a, b):
    n, m = len(a), len(b)
    if n == m:
        return float(np.mean((a - b) ** 2))
    bp = np.unique(np.concatenate([np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n]))
    lo, hi = bp[:-1], bp[1:]
    return float(np.sum((hi - lo) * (a[lo // m] - b[lo // n]) ** 2) / (n * m))


def directions(seed, K, D):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        v = rng.normal(size=D)
        out.append(v / np.linalg.norm(v))
    return np.array(out)


def ref_distances(X, Y, U, normalisation="none"):
    """X (n, D), Y (m, D) as given (fp32 data widened), U (K, D) float64 -> (distances, scale)."""
    PX = X.astype(np.float64) @ U.T
    PY = Y.astype(np.float64) @ U.T
    scale = max(np.abs(PX).max(), np.abs(PY).max())
    sd = np.std(PX, axis=0) if normalisation == "standardise" else np.ones(U.shape[0])
    PX.sort(axis=0)
    PY.sort(axis=0)
    d = np.sqrt(np.array([w2sq_sorted(PX[:, k], PY[:, k]) for k in range(U.shape[0])])) / sd
    return d, scale / sd.min()


def make_sets(n, m, L, C, shift):
    np.random.seed(42)
    X = np.random.rand(n, L * C).astype(np.float32)
    Y = (np.random.rand(m, L * C) + shift).astype(np.float32)
    return X, Y


SHAPES = [(1000, 1000, 2, 1, 1000), (3000, 700, 187, 1, 200), (2000, 512, 512, 8, 64), (1500, 333, 365, 13, 64),
          (1200, 1, 24, 40, 64)]


def check(got, ref, scale, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max() / scale
    print(f"{what}: max error / scale = {err:.3e}")
    assert err <= TOL_OP, (what, err)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n{}m{}L{}C{}K{}".format(*s))
@pytest.mark.parametrize("shift", [0.0, 0.05, 1.0])
@pytest.mark.parametrize("normalisation", ["none", "standardise"])
def test_closed_form(shape, shift, normalisation):
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    n, m, L, Cn, K = shape
    X, Y = make_sets(n, m, L, Cn, shift)
    wd = WassersteinDistances(X, Y, normalisation=normalisation, seed=42)
    got = wd.sliced_distances(K)
    assert got.dtype == np.float64 and got.shape == (K,)
    ref, scale = ref_distances(X, Y, directions(42, K, L * Cn), normalisation)
    check(got, ref, scale, "sliced")
    got_m = wd.marginal_distances()
    assert got_m.shape == (L * Cn,)
    ref_m, scale_m = ref_distances(X, Y, np.identity(L * Cn), normalisation)
    check(got_m, ref_m, scale_m, "marginal")
    f = (L * Cn) // 2
    assert wd.feature_distance(f) == got_m[f]
    assert wd.directional_distance(directions(42, 1, L * Cn)[0]) == got[0]


@pytest.mark.parametrize("shift", [0.0, 0.1, 1.0])
def test_reference_invariants(shift):
    """tests/test_metrics.py:18-82 of the reference without its POT comparison."""
    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, SlicedWasserstein

    np.random.seed(42)
    d1 = np.random.rand(1000, 2, 1)
    d2 = np.random.rand(1000, 2, 1) + shift
    sw = SlicedWasserstein(original_samples=d1, random_seed=42, num_directions=1000, save_all_distances=True)(d2)
    assert list(sw) == ["sliced_wasserstein_mean", "sliced_wasserstein_max", "sliced_wasserstein_all"]
    assert abs(sw["sliced_wasserstein_mean"] - np.mean(sw["sliced_wasserstein_all"])) <= 1e-5
    assert sw["sliced_wasserstein_mean"] <= sw["sliced_wasserstein_max"]
    mw = MarginalWasserstein(original_samples=d1, random_seed=42, save_all_distances=True)(d2)
    assert abs(mw["marginal_wasserstein_mean"] - np.mean(mw["marginal_wasserstein_all"])) <= 1e-5
    assert mw["marginal_wasserstein_mean"] <= mw["marginal_wasserstein_max"]
    assert abs(mw["marginal_wasserstein_mean"] - shift) <= 0.1
    assert abs(mw["marginal_wasserstein_max"] - shift) <= 0.1


def prepare_sorted(lib, rows, budget=1 << 30):
    """Sort the rows of a (K, N) array through ffd_w2_prepare's marginal form: x = rows^T, D = K."""
    from fastfourierdiffusion_amd import _native as N

    K, n = rows.shape
    x = torch.from_numpy(np.ascontiguousarray(rows.T)).cuda()
    out = torch.empty((K, n), device="cuda", dtype=torch.float32)
    nbytes = lib.ffd_w2_work_bytes(n, 0, K, K, budget)
    work = torch.empty(nbytes // 4, device="cuda", dtype=torch.float32)
    rc = lib.ffd_w2_prepare(x.data_ptr(), n, K, None, K, out.data_ptr(), work.data_ptr(), nbytes,
                            N.current_stream_ptr(x.device))
    assert rc == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 32768, 32769, 100003, 2 ** 20 + 1])
@pytest.mark.parametrize("K", [1, 1000])
def test_sort_contract(lib, n, K):
    """Ascending and a permutation of the input: bit for bit np.sort (inputs hold no -0.0 and no NaN)."""
    if K == 1000 and n > 100003:
        K = 40  # 1000 rows of 2^20 keys are 4 GB a buffer; the block logic is the same
    rs = np.random.RandomState(n % 1000 + K)
    rows = rs.randn(K, n).astype(np.float32)
    if K > 4:
        rows[0] = 1.5                                      # all equal
        rows[1] = np.sort(rows[1])                         # already sorted
        rows[2] = np.sort(rows[2])[::-1]                   # reversed
        rows[3, :: max(1, n // 7)] = np.inf                # +-inf and ties
        rows[3, 1:: max(1, n // 5)] = -np.inf
        rows[4] = np.round(rows[4])                        # many ties
    else:
        rows[0, :: max(1, n // 3)] = -np.inf
        rows[0, 1:: max(1, n // 3)] = np.inf
    rows += 0.0  # -0.0 -> +0.0
    got = prepare_sorted(lib, rows)
    want = np.sort(rows, axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if K > 1:  # a scratch buffer for 7 rows: the row blocks of ffd_w2_prepare land where one block puts them
        blocked = prepare_sorted(lib, rows, budget=7 * 4 * n)
        assert np.array_equal(blocked.view(np.uint32), want.view(np.uint32))


def test_exact_cases():
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    X, Y = make_sets(3000, 700, 187, 1, 0.05)
    same = WassersteinDistances(X, X, seed=7)
    assert np.all(same.sliced_distances(64) == 0.0) and np.all(same.marginal_distances() == 0.0)
    # a shift c along direction u moves every projection on u by c |u|^2 = c
    u = directions(3, 1, 187)[0]
    c = np.float32(0.375)
    Xs = (X.astype(np.float64) + float(c) * u).astype(np.float32)
    d = WassersteinDistances(X, Xs, seed=7).directional_distance(u)
    scale = np.abs(X.astype(np.float64) @ u).max() + float(c)
    print(f"shift: got {d!r} want {float(c)!r} error / scale {abs(d - float(c)) / scale:.3e}")
    assert abs(d - float(c)) <= TOL_OP * scale
    # swapping the sets: the integral walks the longer set either way -> the same terms in the same order
    ab = WassersteinDistances(X, Y, seed=7).sliced_distances(64)
    ba = WassersteinDistances(Y, X, seed=7).sliced_distances(64)
    print("swap: max |ab - ba| =", np.abs(ab - ba).max())
    assert np.array_equal(ab, ba)


def test_feature_distance_is_the_column_path():
    """A feature's distance never multiplies by the other columns: an inf elsewhere in a row does not reach it."""
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    X, Y = make_sets(500, 120, 6, 1, 0.1)
    X[3, 1] = np.inf
    Y[5, 4] = -np.inf
    wd = WassersteinDistances(X, Y, seed=1)
    marg = wd.marginal_distances()
    for f in (0, 2, 3, 5):
        assert np.isfinite(marg[f]) and wd.feature_distance(f) == marg[f]
    ref, scale = ref_distances(X[:, [0, 2, 3, 5]], Y[:, [0, 2, 3, 5]], np.identity(4))
    check(marg[[0, 2, 3, 5]], ref, scale, "finite columns beside inf columns")


def test_repeated_calls_on_one_object_with_a_cache():
    """The generator advances between calls (as in the reference), so the second call has new directions: the
    prepared rows of the first must not be paired with them."""
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    X, Y = make_sets(900, 200, 33, 1, 0.05)
    wd = WassersteinDistances(X, Y, seed=9)
    wd._prepared = {}
    first, second = wd.sliced_distances(16), wd.sliced_distances(16)
    U = directions(9, 32, 33)
    ref, scale = ref_distances(X, Y, U)
    check(first, ref[:16], scale, "first call")
    check(second, ref[16:], scale, "second call")
    assert len(wd._prepared) == 2


def test_device_tensors_are_used_in_place():
    """MetricCollection fed device tensors: no host copy of the samples is made (check_flat_array keeps them on the
    device), and the numbers equal those from the same data as host tensors bit for bit."""
    from functools import partial

    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.utils.tensors import check_flat_array

    rs = np.random.RandomState(3)
    X = torch.from_numpy(rs.randn(200, 24, 5).astype(np.float32))
    Y = torch.from_numpy(rs.randn(90, 24, 5).astype(np.float32) + 0.2)
    metrics = [partial(SlicedWasserstein, random_seed=1, num_directions=32, save_all_distances=True),
               partial(MarginalWasserstein, random_seed=1, save_all_distances=True)]
    host = MetricCollection(metrics, original_samples=X, include_spectral_density=True)(Y)
    Xd, Yd = X.cuda(), Y.cuda()
    flat = check_flat_array(Xd)
    assert isinstance(flat, torch.Tensor) and flat.is_cuda and flat.shape == (200, 120)
    assert flat.data_ptr() == Xd.data_ptr()
    coll = MetricCollection(metrics, original_samples=Xd, include_spectral_density=True)
    sw = coll.metrics_time[0]
    assert sw.original_samples.data_ptr() == Xd.data_ptr() and sw._original().data_ptr() == Xd.data_ptr()
    assert coll(Yd) == host


def test_determinism_and_direction_blocks(monkeypatch):
    from fastfourierdiffusion_amd.utils import wasserstein as W

    X, Y = make_sets(1500, 333, 365, 13, 0.05)
    runs = [W.WassersteinDistances(X, Y, normalisation="standardise", seed=42).sliced_distances(64) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    marg = W.WassersteinDistances(X, Y, seed=42).marginal_distances()
    monkeypatch.setattr(W, "WORK_BUDGET_BYTES", 7 * 4 * (1500 + 333 + 1500))  # 7 directions per block
    blocked = W.WassersteinDistances(X, Y, normalisation="standardise", seed=42).sliced_distances(64)
    assert np.array_equal(blocked, runs[0])
    assert np.array_equal(W.WassersteinDistances(X, Y, seed=42).marginal_distances(), marg)
    # the prepared form (a Metric's path) gives the same bits as the one-shot form, blocked or not
    wd = W.WassersteinDistances(X, Y, normalisation="standardise", seed=42)
    wd._prepared = {}
    monkeypatch.setattr(W, "WORK_BUDGET_BYTES", 7 * 4 * 1500)
    assert np.array_equal(wd.sliced_distances(64), runs[0])


# metrics.py: SlicedWasserstein.__call__ gives sliced_wasserstein_{mean,max,all}, MarginalWasserstein.__call__
# marginal_wasserstein_{mean,max,all} (save_all_distances on); MetricCollection.__call__ prefixes them time_ / freq_,
# adds both metrics' baselines {mean,max}_{self,dummy} under the same prefixes, then the spectral_ block of
# MarginalWasserstein(save_all_distances=True), and sorts by key (metrics.py:64-85).
EXPECTED_KEYS = sorted(
    [f"{dom}_{met}_wasserstein_{stat}" for dom in ("time", "freq") for met in ("sliced", "marginal")
     for stat in ("mean", "max", "all", "mean_self", "max_self", "mean_dummy", "max_dummy")]
    + [f"spectral_marginal_wasserstein_{stat}" for stat in ("mean", "max", "all")])


@pytest.mark.parametrize("shape", [(600, 256, 187, 1), (300, 128, 24, 40)], ids=["ecg", "L24C40"])
def test_metric_collection_end_to_end(shape):
    from functools import partial

    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.utils.fourier import dft, spectral_density

    n, m, L, Cn = shape
    K, seed = 64, 42
    rs = np.random.RandomState(5)
    X = torch.from_numpy(rs.randn(n, L, Cn).astype(np.float32))
    Y = torch.from_numpy((0.9 * rs.randn(m, L, Cn) + 0.1).astype(np.float32))
    coll = MetricCollection(
        metrics=[partial(SlicedWasserstein, random_seed=seed, num_directions=K, save_all_distances=True),
                 partial(MarginalWasserstein, random_seed=seed, save_all_distances=True),
                 "not a partial: ignored like in the reference"],
        original_samples=X, include_baselines=True, include_spectral_density=True)
    res = coll(Y)
    assert list(res) == EXPECTED_KEYS
    res2 = coll(Y)  # second call: the prepared original set is reused
    assert res2 == res

    def flat(t):
        return t.reshape(t.shape[0], -1).numpy()

    domains = {"time": (flat(X), flat(Y)), "freq": (flat(dft(X)), flat(dft(Y))),
               "spectral": (flat(spectral_density(X)), flat(spectral_density(Y)))}
    worst = 0.0
    for dom, (A, B) in domains.items():
        D = A.shape[1]
        metrics = {"marginal": np.identity(D)} if dom == "spectral" else \
            {"sliced": directions(seed, K, D), "marginal": np.identity(D)}
        for met, U in metrics.items():
            cases = {"": (A, B)}
            if dom != "spectral":
                cases["_self"] = (A[: n // 2], A[n // 2:])
                cases["_dummy"] = (A, A.astype(np.float64).mean(axis=0, keepdims=True))
            for suffix, (P, Q) in cases.items():
                ref, scale = ref_distances(P, Q, U)
                key = f"{dom}_{met}_wasserstein"
                for stat, val in (("mean", ref.mean()), ("max", ref.max())):
                    err = abs(res[f"{key}_{stat}{suffix}"] - val) / scale
                    worst = max(worst, err)
                    assert err <= TOL_OP, (key, stat, suffix, err)
                if suffix == "":
                    err = np.abs(np.array(res[f"{key}_all"]) - ref).max() / scale
                    worst = max(worst, err)
                    assert err <= TOL_OP, (key, "all", err)
    print(f"metric collection {shape}: worst error / scale = {worst:.3e}")
    # the baselines are the metric itself on the two folds / on the mean sample (m = 1)
    sw = coll.metrics_time[0]
    Xf = flat(X)
    folds = SlicedWasserstein(Xf[: n // 2], seed, K)(Xf[n // 2:])
    assert folds["sliced_wasserstein_mean"] == res["time_sliced_wasserstein_mean_self"]
    assert folds["sliced_wasserstein_max"] == res["time_sliced_wasserstein_max_self"]
    dummy = sw(Xf.astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32))
    assert abs(dummy["sliced_wasserstein_mean"] - res["time_sliced_wasserstein_mean_dummy"]) <= TOL_OP * np.abs(Xf).max()


def test_evaluation_size():
    """n = 87 554, m = 10 000, D = 187, K = 1000 (the ECG evaluation): the kernels compute all 1000 distances, the
    float64 comparator 16 of them (0, 999 and 14 spread between)."""
    from fastfourierdiffusion_amd.utils.wasserstein import WassersteinDistances

    n, m, D, K = 87554, 10000, 187, 1000
    rs = np.random.RandomState(11)
    X = rs.randn(n, D).astype(np.float32)
    Y = (1.1 * rs.randn(m, D) + 0.05).astype(np.float32)
    got = WassersteinDistances(X, Y, seed=42).sliced_distances(K)
    # |x . u| <= |x|: no two projections are further apart than the two largest norms together
    bound = np.linalg.norm(X.astype(np.float64), axis=1).max() + np.linalg.norm(Y.astype(np.float64), axis=1).max()
    assert got.shape == (K,) and np.all(np.isfinite(got)) and np.all(got >= 0) and np.all(got <= bound)
    idx = np.unique(np.concatenate([[0, K - 1], np.linspace(1, K - 2, 14).astype(int)]))
    assert len(idx) == 16
    ref, scale = ref_distances(X, Y, directions(42, K, D)[idx])
    check(got[idx], ref, scale, "evaluation size (16 directions)")
