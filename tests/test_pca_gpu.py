"""GPU tests of the float64 moment statistics (ffd_pca.hip, ``utils.pca``, ``FrechetDistance``) against the numpy restatement
and the LAPACK judge of tests/pca_restatement.py.  Every test prints its measured figures before it asserts.

Bars.  Covariance: the a-priori summation bounds, mean within n 2^-53 mean|x_j|, entries within 2 n 2^-53 sqrt(S_ii S_jj);
exact cases with ==.  Eigensolver: eigenvalues against LAPACK within max(3 x the restatement's own error on that matrix,
D 2^-52 |A|_F); residual |A V - V L| and |V^T V - I| within 3 x the restatement's, with floors D 2^-52 |A|_F and 3 D 2^-52
(3: the project's margin for a device run of a restated algorithm; FMA contraction and another sqrt move individual
roundings, not their count).  FD: within max(3 |restatement - judge|, 10 x the judge's spread between its two argument
orders); the rank-deficient pair within 2 sum_i min(sqrt e, e / sqrt l_i), e the eigenvalue bar of M: the square root of an
eigenvalue near zero turns an error e into sqrt e.

Measured on an MI355X (largest share of the bar over all cases of the test):
  covariance entries                  0.26 (n = 3; 0.05 at n = 63 ... 65, 0.005 at n = 1025); the mean prints as 0.000
  eigenvalues / residual / |V^T V - I| 0.33 / 0.26 / 0.41; sweeps equal the restatement's or one fewer, at most 18
  D = 1024                            6 sweeps in 0.114 s, residual 0.005, |V^T V - I| 0.57 of their floors
  FD against the judge                0.13 ... 0.59 (D = 16 series: 3.2e-14 of the traces against 5.4e-14)
  the rank-deficient pair             4.3e-8 against a bar of 2.9e-6
  pc_variances / transform            0.20 / 0.17
"""
import ctypes as C
import time
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import pca_restatement as PR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
COV_ROWS = (2, 3, 63, 64, 65, 1025, PR.SLAB + 1)
COV_DIMS = (1, 15, 16, 17, 187, 257)


@pytest.fixture(scope="module")
def P():
    from fastfourierdiffusion_amd.utils import pca

    return pca


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ covariance ----
@pytest.mark.parametrize("D", COV_DIMS)
@pytest.mark.parametrize("n", COV_ROWS)
def test_covariance_within_the_summation_bound(P, n, D):
    worst_mean = worst_cov = 0.0
    for family in PR.FAMILIES:
        x = PR.make_rows(n, D, family, 100 + n + D)
        mean, cov = (_host(t) for t in P.covariance(_dev(x)))
        again = [_host(t) for t in P.covariance(_dev(x))]
        jm, jc = PR.judge_cov(x)
        assert mean.shape == (D,) and cov.shape == (D, D) and np.array_equal(cov, cov.T)  # bitwise symmetric
        assert np.array_equal(mean, again[0]) and np.array_equal(cov, again[1])  # bit-identical from run to run
        mean_bar = n * U * np.abs(x.astype(np.float64)).mean(axis=0)
        cov_bar = 2 * n * U * np.sqrt(np.outer(np.diag(jc), np.diag(jc)))
        e_mean, e_cov = np.abs(mean - jm), np.abs(cov - jc)
        worst_mean = max(worst_mean, float((e_mean / mean_bar).max()))
        worst_cov = max(worst_cov, float((e_cov / np.maximum(cov_bar, 1e-300)).max()))
        assert (e_mean <= mean_bar).all(), (family, float((e_mean / mean_bar).max()))
        assert (e_cov <= cov_bar).all(), (family, float((e_cov / np.maximum(cov_bar, 1e-300)).max()))
    print(f"n = {n}, D = {D}: mean at {worst_mean:.3f} of its bound, covariance at {worst_cov:.3f} of its bound")


def _cov_raw(x, fill):
    """ffd_cov into outputs pre-filled with ``fill``."""
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    n, D = x.shape
    mean = torch.full((D,), fill, device="cuda", dtype=torch.float64)
    cov = torch.full((D, D), fill, device="cuda", dtype=torch.float64)
    nbytes = lib.ffd_cov_work_bytes(n, D)
    work = torch.full(((nbytes + 7) // 8,), fill, device="cuda", dtype=torch.float64)
    rc = lib.ffd_cov(x.data_ptr(), n, D, mean.data_ptr(), cov.data_ptr(), work.data_ptr(), nbytes,
                     N.current_stream_ptr(x.device))
    assert rc == 0
    return _host(mean), _host(cov)


def test_covariance_exact_cases_and_prefilled_outputs(P):
    rng = np.random.default_rng(7)
    # constant rows: the mean is the row and every deviation is 0.0
    for n, D in ((2, 1), (65, 17), (PR.SLAB + 1, 187)):
        row = rng.standard_normal(D).astype(np.float32)
        mean, cov = (_host(t) for t in P.covariance(_dev(np.tile(row, (n, 1)))))
        assert np.array_equal(mean, row.astype(np.float64)) and not cov.any()
    # n = 2: deviations +- (x0 - x1) / 2, exact, and the two equal products of an entry add to twice one of them
    for D in (1, 16, 187):
        x = rng.standard_normal((2, D)).astype(np.float32)
        mean, cov = (_host(t) for t in P.covariance(_dev(x)))
        x64 = x.astype(np.float64)
        half = (x64[0] - x64[1]) / 2.0
        assert np.array_equal(mean, (x64[0] + x64[1]) / 2.0)
        assert np.array_equal(cov, 2.0 * np.outer(half, half))
    # integer rows, n - 1 a power of two, column sums divisible by n: every step is exact
    for n, D in ((5, 3), (17, 16), (257, 187), (1025, 65)):
        x = rng.integers(-50, 51, (n, D))
        x[-1] -= x.sum(axis=0) % n
        assert not (x.sum(axis=0) % n).any()
        mean, cov = (_host(t) for t in P.covariance(_dev(x.astype(np.float32))))
        dev_rows = x - x.sum(axis=0) // n
        assert np.array_equal(mean, (x.sum(axis=0) // n).astype(np.float64))
        assert np.array_equal(cov, (dev_rows.T @ dev_rows).astype(np.float64) / (n - 1))
    # every output element is written, whatever the buffers held
    x = _dev(PR.make_rows(PR.SLAB + 1, 187, "offset", 8))
    a, b = _cov_raw(x, float("nan")), _cov_raw(x, 7.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.isfinite(a[1]).all()
    # the deviation form: a mean of 100 under a unit spread costs nothing (the raw-moment form would lose 4 digits)
    mean, cov = a
    jm, jc = PR.judge_cov(_host(x))
    assert np.abs(cov - jc).max() <= 2 * 257 * U * np.diag(jc).max() and abs(mean.mean() - 100.0) < 0.1


# ------------------------------------------------------------------ the eigensolver ----
def _eig_case(P, D, kind):
    case = PR.restated_case(D, kind)
    a = case["a"]
    t = time.time()
    w, v, info = P.eigh(_dev(a), info=True)
    torch.cuda.synchronize()
    t = time.time() - t
    return case, a, _host(w), _host(v), info, t


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("D", PR.EIG_DIMS)
def test_eigensolver_against_lapack_and_the_restatement(P, D, kind):
    case, a, w, v, info, t = _eig_case(P, D, kind)
    fro = case["fro"]
    e_val, res, orth = PR.eig_errors(a, w, v)
    val_bar = max(3 * case["e_val"], D * PR.EPS * fro)
    res_bar = max(3 * case["res"], D * PR.EPS * fro)
    orth_bar = max(3 * case["orth"], 3 * D * PR.EPS)
    print(f"D = {D} {kind}: {info.sweeps} sweeps (restated {case['sweeps']}) in {1e3 * t:.1f} ms; eigenvalues at "
          f"{e_val / val_bar:.3f}, residual at {res / res_bar:.3f}, |V^T V - I| at {orth / orth_bar:.3f} of their bars")
    assert info.sweeps <= 20 and info.off <= PR.STOP
    assert e_val <= val_bar and res <= res_bar and orth <= orth_bar
    assert (np.diff(w) >= 0).all()  # ascending
    if kind == "indefinite" and D > 1:
        assert w[0] < 0 < w[-1]  # negative eigenvalues come out negative
    if kind in ("identity", "diagonal"):
        assert info.sweeps == 0 and np.array_equal(w, np.sort(np.diag(a)))  # exactly, without a rotation
        assert np.array_equal(np.abs(v).sum(axis=0), np.ones(D)) and np.array_equal(a @ v, v * w[None, :])
    # the values do not depend on whether vectors are kept; the run is bit-identical; all thresholds are relative
    da = _dev(a)
    assert np.array_equal(_host(P.eigh(da, vectors=False)), w)
    w2, v2 = P.eigh(da)
    assert np.array_equal(_host(w2), w) and np.array_equal(_host(v2), v)
    w4, v4 = P.eigh(_dev(4.0 * a))
    assert np.array_equal(_host(w4), 4.0 * w) and np.array_equal(_host(v4), v)


def test_eigensolver_reports_a_cap_that_was_hit(P):
    from fastfourierdiffusion_amd import _native as N

    a = _dev(PR.restated_case(64, "indefinite")["a"])
    with pytest.raises(N.FFDError, match="did not converge in 1 sweeps"):
        P.eigh(a, max_sweeps=1)
    lib = N.lib()
    w = torch.empty(64, device="cuda", dtype=torch.float64)
    info = (C.c_double * 3)(-1.0, -1.0, -1.0)
    nbytes = lib.ffd_sym_eig_work_bytes(64)
    work = torch.empty(nbytes // 8, device="cuda", dtype=torch.float64)
    rc = lib.ffd_sym_eig(a.data_ptr(), 64, 1, w.data_ptr(), None, C.addressof(info), work.data_ptr(), nbytes,
                         N.current_stream_ptr(a.device))
    assert rc == 0 and info[0] == 1.0 and info[1] > PR.STOP and info[2] == 0.0
    assert (np.diff(_host(w)) >= 0).all()  # what there is, still in order


def test_eigensolver_at_the_limit(P):
    """D = FFD_PCA_MAX_D, the covariance of 2048 anisotropic rows, judged by its residual alone."""
    D = 1024
    x = _dev(PR.make_rows(2048, D, "anisotropic", 9))
    _, cov = P.covariance(x)
    torch.cuda.synchronize()
    t = time.time()
    w, v, info = P.eigh(cov, info=True)
    torch.cuda.synchronize()
    t = time.time() - t
    a, w, v = _host(cov), _host(w), _host(v)
    fro = float(np.sqrt((a * a).sum()))
    res = float(np.abs(a @ v - v * w[None, :]).max())
    orth = float(np.abs(v.T @ v - np.eye(D)).max())
    print(f"D = 1024: {info.sweeps} sweeps in {t:.3f} s; residual {res / (D * PR.EPS * fro):.3f} of D 2^-52 |A|_F, "
          f"|V^T V - I| {orth / (3 * D * PR.EPS):.3f} of 3 D 2^-52")
    assert info.sweeps <= 20 and res <= D * PR.EPS * fro and orth <= 3 * D * PR.EPS and (np.diff(w) >= 0).all()


# ------------------------------------------------------------------ the Frechet distance ----
@lru_cache(maxsize=None)
def _moment_pair(D, family, n_x, n_y):
    X, Y = PR.make_rows(n_x, D, family, 40 + D), PR.make_rows(n_y, D, family, 41 + D)
    return PR.covariance(X) + PR.covariance(Y)


def _device_fd(P, mx, cx, my, cy, root=None):
    return P.frechet_distance(_dev(mx), _dev(cx), _dev(my), _dev(cy), root_y=root)


@pytest.mark.parametrize("family", PR.FAMILIES)
@pytest.mark.parametrize("D", [16, 187])
def test_frechet_distance_against_the_judge(P, D, family):
    mx, cx, my, cy = _moment_pair(D, family, 2 * D + 7, 3 * D)
    judge, spread = PR.judge_fd(mx, cx, my, cy), PR.judge_spread(mx, cx, my, cy)
    restated = PR.frechet(mx, cx, my, cy)
    bar = max(3 * abs(restated["fd"] - judge), 10 * spread)
    got = _device_fd(P, mx, cx, my, cy)
    scale = restated["trace_x"] + restated["trace_y"]
    print(f"D = {D} {family}: FD {got.distance:.12g}, judge {judge:.12g}; off by {abs(got.distance - judge) / scale:.2e} of the "
          f"traces, bar {bar / scale:.2e} (restatement {abs(restated['fd'] - judge) / scale:.2e}, judge's spread "
          f"{spread / scale:.2e})")
    assert abs(got.distance - judge) <= bar
    assert got.distance == got.mean_term + got.cov_term
    assert abs(got.mean_term - restated["mean_term"]) <= D * PR.EPS * restated["mean_term"]
    assert abs(got.trace_x - restated["trace_x"]) <= D * PR.EPS * scale and abs(got.trace_y - restated["trace_y"]) <= D * PR.EPS * scale
    # a supplied root against a computed one: the same bits
    w, v = P.eigh(_dev(cy))
    root = P.sym_root(w, v)
    assert np.array_equal(_host(root), _host(root).T)  # bitwise symmetric
    assert _device_fd(P, mx, cx, my, cy, root=root) == got


def test_frechet_distance_of_a_rank_deficient_pair(P):
    D = 16
    mx, cx, my, cy = _moment_pair(D, "series", D // 2, D // 2)
    judge, restated = PR.judge_fd(mx, cx, my, cy), PR.frechet(mx, cx, my, cy)
    lam_y, vec_y = np.linalg.eigh(cy)
    half = (vec_y * np.sqrt(np.clip(lam_y, 0.0, None))) @ vec_y.T
    m = half @ cx @ half
    m = (m + m.T) / 2.0
    lam = np.clip(np.linalg.eigvalsh(m), 0.0, None)
    e_restated = float(np.abs(PR.jacobi_eigh(m, vectors=False)[0] - np.linalg.eigvalsh(m)).max())
    e = max(3 * e_restated, D * PR.EPS * float(np.sqrt((m * m).sum())))
    with np.errstate(divide="ignore"):
        bar = 2.0 * float(np.minimum(np.sqrt(e), e / np.sqrt(lam)).sum())
    got = _device_fd(P, mx, cx, my, cy)
    print(f"rank-deficient D = {D}: FD {got.distance:.12g}, judge {judge:.12g}, restated {restated['fd']:.12g}; off by "
          f"{abs(got.distance - judge):.2e}, bar {bar:.2e}")
    assert abs(got.distance - judge) <= bar


@pytest.mark.parametrize("D", [16, 187])
def test_frechet_distance_of_equal_and_of_shifted_sets(P, D):
    """FD(Y, Y) = 0 and FD(Y, Y + v) = |v|^2.  Floor: D 2^-52 (tr S_x + tr S_y), the rounding of the D square roots and the
    sums the value is made of; beside it 3 x the restatement's and 10 x the judge's own distance from 0."""
    _, _, my, cy = _moment_pair(D, "offset", 2 * D + 7, 3 * D)
    scale = 2.0 * float(np.trace(cy))
    floor = D * PR.EPS * scale
    bar = max(3 * abs(PR.frechet(my, cy, my, cy)["fd"]), 10 * abs(PR.judge_fd(my, cy, my, cy)), floor)
    same = _device_fd(P, my, cy, my, cy)
    v = np.random.default_rng(D).integers(-4, 5, D) / 4.0
    v2 = float(v @ v)
    moved = _device_fd(P, my + v, cy, my, cy)
    print(f"D = {D}: FD(Y, Y) = {same.distance:.3e} (bar {bar:.3e}); FD(Y, Y + v) - |v|^2 = {moved.distance - v2:.3e}")
    assert same.mean_term == 0.0 and abs(same.distance) <= bar
    assert abs(moved.mean_term - v2) <= D * PR.EPS * (v2 + np.abs(my).max() ** 2) and abs(moved.distance - v2) <= bar + D * PR.EPS * v2
    assert moved.cov_term == same.cov_term


# ------------------------------------------------------------------ principal components ----
@pytest.mark.parametrize("n,D,k", [(3, 1, 1), (65, 17, 17), (1025, 187, 10), (200, 257, 3)])
def test_pc_variances_and_transform(P, n, D, k):
    x = PR.make_rows(n, D, "series", 60 + D)
    mean, cov = PR.covariance(x)
    w, v = np.linalg.eigh(cov)
    top = v[:, ::-1][:, :k]
    got = _host(P.pc_variances(_dev(cov), _dev(v), k))
    want = PR.pc_variances(cov, v, k)
    bar = 2 * D * U * np.einsum("di,de,ei->i", np.abs(top), np.abs(cov), np.abs(top))  # two chained sums of D terms
    print(f"n = {n}, D = {D}, k = {k}: variances at {float((np.abs(got - want) / bar).max()):.3f} of their bound")
    assert got.shape == (k,) and (np.abs(got - want) <= bar).all()
    scores = _host(P.transform(_dev(x), _dev(mean), _dev(v), k))
    dev_rows = x.astype(np.float64) - mean
    bar = D * U * (np.abs(dev_rows) @ np.abs(top))
    err = np.abs(scores - dev_rows @ top)
    print(f"   scores at {float((err / np.maximum(bar, 1e-300)).max()):.3f} of their bound")
    assert scores.shape == (n, k) and (err <= bar).all()
    assert np.array_equal(scores, _host(P.transform(_dev(x), _dev(mean), _dev(v), k)))


# ------------------------------------------------------------------ the metric, end to end ----
def _close(got, want, rel, traces):
    """FD and its terms within rel x the traces, its root through d sqrt(FD) = d FD / (2 sqrt(FD)), the ratios within rel x
    their size."""
    assert tuple(got) == tuple(want)
    for key, value in want.items():
        stem = key[: -len("_self")] if key.endswith("_self") else key
        if stem == "frechet_w2":
            bar = rel * traces / (2.0 * value)
        elif stem.startswith("frechet_"):
            bar = rel * traces
        else:
            bar = rel * max(abs(value), 1.0)
        assert abs(got[key] - value) <= bar, (key, got[key], value, bar)


def test_frechet_metric_and_collection_end_to_end(P):
    """Against the float64 pipeline.  Every covariance entry is within 2 n 2^-53 of its scale and D of them meet in each of
    D square roots: 4 n D 2^-53 of the quantity's size (the traces for FD and its terms, 1 for the ratios) bounds what the
    two sides can differ by on well-conditioned data."""
    from fastfourierdiffusion_amd.sampling import FrechetDistance, KernelMMD
    from fastfourierdiffusion_amd.sampling import metrics as M

    n, m, D = 300, 420, 24
    X, Y = PR.make_rows(n, D, "offset", 70) - np.float32(99.0), PR.make_rows(m, D, "offset", 71) - np.float32(99.0)
    metric = FrechetDistance(Y, components=5)
    got, want = metric(X), PR.pipeline(X, Y, components=5)
    rel = 4 * m * D * U
    print({key: (got[key], want[key]) for key in want})
    trace = lambda rows: float(np.trace(PR.covariance(rows)[1]))  # noqa: E731
    _close(got, want, rel, trace(X) + trace(Y))
    assert got["frechet_w2"] == max(got["frechet_distance"], 0.0) ** 0.5
    assert metric(X) == got  # the kept originals give the same bits
    base = metric.baseline_metrics
    print(base)
    _close(base, PR.baseline(Y, components=5), rel, trace(Y[: m // 2]) + trace(Y[m // 2:]))
    assert base["frechet_distance_self"] > 0  # the upward bias of finite samples: the zero point of the metric
    spectrum = _host(metric.explained_variance())
    assert spectrum.shape == (D,) and (np.diff(spectrum) <= 0).all()
    assert abs(spectrum.sum() - trace(Y)) <= rel * trace(Y)
    # the scores' sample variance along an axis over the data's is that axis' ratio
    scores = _host(metric.transform(X, 5))
    ratios = scores.var(axis=0, ddof=1) / spectrum[:5]
    assert scores.shape == (n, 5)
    assert abs(ratios.min() - got["pc_variance_ratio_min"]) <= rel and abs(ratios.max() - got["pc_variance_ratio_max"]) <= rel
    # composed: the other metric's keys and values stay as they were
    X3, Y3 = torch.from_numpy(X.reshape(n, 12, 2)), torch.from_numpy(Y.reshape(m, 12, 2))  # series of 12 steps, 2 channels
    alone = M.MetricCollection([partial(KernelMMD, scales=(1.0,))], original_samples=Y3)(X3)
    found = M.MetricCollection([partial(KernelMMD, scales=(1.0,)), partial(FrechetDistance, components=5)],
                               original_samples=Y3)(X3)
    ours = {f"{p}_{key}{suffix}" for p in ("time", "freq") for key in PR.KEYS for suffix in ("", "_self")}
    assert ours <= set(found) and {k: v for k, v in found.items() if k not in ours} == alone
    assert {key: found[f"time_{key}"] for key in PR.KEYS} == got
    assert list(found) == sorted(found)
    Xq, Yq = (M.dft(t).reshape(t.shape[0], -1).cpu().numpy() for t in (X3, Y3))
    _close({key: found[f"freq_{key}"] for key in PR.KEYS}, PR.pipeline(Xq, Yq, components=5), rel, trace(Xq) + trace(Yq))


def test_planted_shrinkage_along_the_first_axis(P):
    """Samples equal to the data but for half the spread along its first principal axis: that axis reads 0.25, no other
    axis moves, and the mean term stays 0.  fp32 rounding of the planted rows moves a deviation by at most 2^-24 max|x|."""
    from fastfourierdiffusion_amd.sampling import FrechetDistance

    Y = PR.make_rows(600, 32, "series", 80)
    mean, cov = PR.covariance(Y)
    w, v = np.linalg.eigh(cov)
    v1 = v[:, -1]
    dev_rows = Y.astype(np.float64) - mean
    X = (mean + dev_rows - 0.5 * np.outer(dev_rows @ v1, v1)).astype(np.float32)
    got = FrechetDistance(Y, components=4)(X)
    rounding = 2.0 ** -24 * float(np.abs(Y).max())
    # a deviation moved by `rounding` moves an axis' variance l by 2 sqrt(l) rounding: relative 2 rounding / sqrt(l), the
    # smallest l of the four axes watched and of the halved one; twice that as the bar
    ratio_bar = 4.0 * rounding / np.sqrt(min(w[-4], w[-1] / 4.0))
    trace_bar = 4.0 * rounding * np.sqrt(32 / w.sum())  # the same over all D columns, Cauchy-Schwarz
    print(got, "ratio bar", ratio_bar, "trace bar", trace_bar)
    assert abs(got["pc_variance_ratio_min"] - 0.25) <= ratio_bar and abs(got["pc_variance_ratio_max"] - 1.0) <= ratio_bar
    assert 0.0 <= got["frechet_mean_term"] <= 32 * rounding ** 2
    # the first axis alone changed: (sqrt l_1 - sqrt(l_1 / 4))^2 = l_1 / 4; the term's derivative in S_x has norm <= 3
    # there and 0 on the axes that kept their variance, and S_x moved by 2 sqrt(l_1 / 4) rounding on that axis
    assert abs(got["frechet_cov_term"] - w[-1] / 4.0) <= 8.0 * rounding * np.sqrt(w[-1])
    assert abs(got["variance_ratio"] - (w.sum() - 0.75 * w[-1]) / w.sum()) <= trace_bar


# ------------------------------------------------------------------ refusals ----
def test_refusals_on_the_device(P):
    from fastfourierdiffusion_amd import _native as N

    x = _dev(PR.make_rows(20, 4, "offset", 1))
    mean, cov = P.covariance(x)
    w, v = P.eigh(cov)
    for call in (lambda: P.covariance(x[:1]), lambda: P.covariance(x.double()), lambda: P.covariance(x[0]),
                 lambda: P.covariance(torch.zeros((3, P.MAX_D + 1), device="cuda")), lambda: P.eigh(cov[:3]),
                 lambda: P.eigh(cov.float()), lambda: P.eigh(cov, max_sweeps=0), lambda: P.sym_root(w[:3], v),
                 lambda: P.frechet_distance(mean, cov, mean[:3], cov), lambda: P.frechet_distance(mean, cov, mean, cov[:3, :3]),
                 lambda: P.pc_variances(cov, v, 0), lambda: P.pc_variances(cov, v, 5), lambda: P.transform(x, mean, v, 5),
                 lambda: P.transform(x, mean.float(), v, 2)):
        with pytest.raises(AssertionError):
            call()
    for call in (lambda: P.covariance(x.cpu()), lambda: P.eigh(cov.cpu()), lambda: P.transform(x, mean.cpu(), v, 2)):
        with pytest.raises(N.FFDError):
            call()
    # the library's own refusals leave device outputs untouched
    lib = N.lib()
    out = torch.full((4, 4), 7.5, device="cuda", dtype=torch.float64)
    mean_out = torch.full((4,), 7.5, device="cuda", dtype=torch.float64)
    nbytes = lib.ffd_cov_work_bytes(20, 4)
    work = torch.empty(nbytes // 8, device="cuda", dtype=torch.float64)
    stream = N.current_stream_ptr(x.device)
    assert lib.ffd_cov(x.data_ptr(), 20, 4, mean_out.data_ptr(), out.data_ptr(), work.data_ptr(), nbytes - 1, stream) == -1
    assert lib.ffd_cov(x.data_ptr(), 20, 4, mean_out.data_ptr(), mean_out.data_ptr(), work.data_ptr(), nbytes, stream) == -1
    assert lib.ffd_cov(x.data_ptr(), 1, 4, mean_out.data_ptr(), out.data_ptr(), work.data_ptr(), nbytes, stream) == -1
    assert lib.ffd_cov(x.data_ptr(), 20, 1025, mean_out.data_ptr(), out.data_ptr(), work.data_ptr(), nbytes, stream) == -2
    info = (C.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.ffd_sym_eig(cov.data_ptr(), 4, -1, mean_out.data_ptr(), out.data_ptr(), C.addressof(info), work.data_ptr(),
                           lib.ffd_sym_eig_work_bytes(4), stream) == -1
    torch.cuda.synchronize()
    assert (out == 7.5).all() and (mean_out == 7.5).all() and list(info) == [-1.0, -1.0, -1.0]
