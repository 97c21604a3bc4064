"""GPU tests of the nearest-neighbour statistics (ffd_nn_search, ffd_nn_ball_count, ffd_nn_scores, ``utils.neighbours``,
``ManifoldMetrics``) against the float64 numpy restatement (tests/neighbours_restatement.py, which never calls the code
under test).

Bars.  ``scale`` is the largest squared norm of a row of either set about the reference mean, ``bar`` = max(2e-6, 3 e_ref)
with e_ref the error of an fp32 centred Gram restatement on the same input (the project's standing form; 2e-6 is the w2
projection's).  A returned distance is the float64 difference-form distance of the returned index within 1e-12 relative,
and lies within [-1e-12, bar] scale of float64's sorted distance: the selection is made on the fp32 Gram form, so a
neighbour within the bar of the k-th may stand in for it and no index-set equality is asked.  A ball count lies between
float64's counts at radius^2 -+ bar scale; tests/test_neighbours_host.py asserts that the two coincide on every Gaussian
case (so equality is what is tested there) and differ for at most 2 % of the rows of a clustered one."""
import functools
from functools import partial

import numpy as np
import pytest
import torch

import neighbours_restatement as NR

pytestmark = pytest.mark.gpu

ALL_CASES = [(c, f) for f in NR.FAMILIES for c in range(len(NR.CASES))]
DEFAULT_BUDGET = 1 << 30
UNIT = 64 * 256 * 4


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


@functools.lru_cache(maxsize=None)
def reference(case, family, self_search=False):
    """Everything float64 says about a case, computed once: the inputs stay unchanged (arrays are read-only)."""
    Q, R, k = NR.make_case(case, family)
    if self_search:
        Q, k = R, min(k, R.shape[0] - 1)
    out = dict(Q=Q, R=R, k=k, scale=NR.scale(Q, R), bar=NR.bar(Q, R), knn=NR.knn(Q, R, k, exclude_self=self_search),
               rad=NR.self_radius2(R, k))
    for a in (Q, R, out["rad"], *out["knn"]):
        a.setflags(write=False)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def run_search(lib, Q, R, k, exclude_self=False, budget=DEFAULT_BUDGET, same=False):
    """ffd_nn_search on outputs pre-filled with NaN / -1; ``same``: the query set is the reference buffer itself."""
    from fastfourierdiffusion_amd import _native as N

    Rd = _dev(R)
    Qd = Rd if same else _dev(Q)
    (nq, D), nr = Qd.shape, Rd.shape[0]
    dist2 = torch.full((nq, k), float("nan"), device="cuda", dtype=torch.float64)
    index = torch.full((nq, k), -1, device="cuda", dtype=torch.int32)
    nbytes = lib.ffd_nn_work_bytes(nq, nr, D, k, budget)
    assert nbytes > 0
    work = torch.empty((nbytes + 15) // 16 * 2, device="cuda", dtype=torch.float64)
    rc = lib.ffd_nn_search(Qd.data_ptr(), nq, Rd.data_ptr(), nr, D, k, int(exclude_self), dist2.data_ptr(), index.data_ptr(),
                           work.data_ptr(), nbytes, N.current_stream_ptr(Rd.device))
    assert rc == 0, rc
    return dist2.cpu().numpy(), index.cpu().numpy()


def run_ball(lib, Q, R, rad, exclude_self=False, same=False):
    from fastfourierdiffusion_amd import _native as N

    Rd, radd = _dev(R), _dev(rad)
    Qd = Rd if same else _dev(Q)
    (nq, D), nr = Qd.shape, Rd.shape[0]
    count = torch.full((nq,), -1, device="cuda", dtype=torch.int32)
    nbytes = lib.ffd_nn_work_bytes(nq, nr, D, 1, 0)
    work = torch.empty((nbytes + 15) // 16 * 2, device="cuda", dtype=torch.float64)
    rc = lib.ffd_nn_ball_count(Qd.data_ptr(), nq, Rd.data_ptr(), nr, D, radd.data_ptr(), int(exclude_self), count.data_ptr(),
                               work.data_ptr(), nbytes, N.current_stream_ptr(Rd.device))
    assert rc == 0, rc
    return count.cpu().numpy()


def check_search_structure(got_d, got_i, nq, nr, k, exclude_self=False):
    """What needs no reference, over all rows: shape, fully overwritten, in range, distinct, ascending, never i."""
    assert got_d.shape == (nq, k) and got_i.shape == (nq, k)
    assert not np.isnan(got_d).any() and (got_i >= 0).all() and (got_i < nr).all()  # fully overwritten, in range
    srt = np.sort(got_i, axis=1)
    assert (np.diff(srt, axis=1) > 0).all() if k > 1 else True  # distinct
    if exclude_self:
        assert (got_i != np.arange(nq)[:, None]).all()
    assert (np.diff(got_d, axis=1) >= 0).all()


def check_search_values(got_d, got_i, Q, R, k, want, scale, bar, rows=None):
    """The value checks on the listed query rows (all for None); ``want``: float64's (dist2, index) of those rows."""
    if rows is not None:
        got_d, got_i, Q = got_d[rows], got_i[rows], Q[rows]
    own = ((Q.astype(np.float64)[:, None, :] - R.astype(np.float64)[got_i]) ** 2).sum(axis=2)
    assert (np.abs(got_d - own) <= 1e-12 * own).all(), np.abs(got_d - own).max()
    assert (got_d[own == 0.0] == 0.0).all()
    diff = (got_d - want[0]) / scale
    same = int((np.sort(got_i, axis=1) == np.sort(want[1], axis=1)).all(axis=1).sum())
    print(f"dist2 - float64 sorted: [{diff.min():.3e}, {diff.max():.3e}] of the scale {scale:.4e}; bar {bar:.3e}; "
          f"index sets equal in {same} of {len(got_d)} rows")
    assert diff.min() >= -1e-12 and diff.max() <= bar, (diff.min(), diff.max(), bar)


def check_search(got_d, got_i, Q, R, k, want_d, scale, bar, exclude_self=False):
    check_search_structure(got_d, got_i, Q.shape[0], R.shape[0], k, exclude_self)
    check_search_values(got_d, got_i, Q, R, k, (want_d, NR.knn(Q, R, k, exclude_self)[1]), scale, bar)


def check_ball(got, Q, R, rad, scale, bar, exclude_self=False, rows=None):
    """``rows``: judge only the listed query rows of the device's counts."""
    lo = NR.ball_counts(Q, R, rad, exclude_self, shift=-bar * scale, rows=rows)
    hi = NR.ball_counts(Q, R, rad, exclude_self, shift=bar * scale, rows=rows)
    assert got.dtype == np.int32 and got.shape == (Q.shape[0],)
    got = got if rows is None else got[rows]
    print(f"counts: {int((got != lo).sum())} rows above float64's lower count, {int((got != hi).sum())} below its upper, "
          f"band open for {int((lo != hi).sum())} of {len(got)} rows, mean count {got.mean():.1f}")
    assert (lo <= got).all() and (got <= hi).all()
    return lo, hi


# ------------------------------------------------------------------ the contracts ----
@pytest.mark.parametrize("case,family", ALL_CASES)
def test_search_contract(lib, case, family):
    ref = reference(case, family)
    got_d, got_i = run_search(lib, ref["Q"], ref["R"], ref["k"])
    check_search(got_d, got_i, ref["Q"], ref["R"], ref["k"], ref["knn"][0], ref["scale"], ref["bar"])


@pytest.mark.parametrize("case,family", ALL_CASES)
def test_ball_count_contract(lib, case, family):
    ref = reference(case, family)
    check_ball(run_ball(lib, ref["Q"], ref["R"], ref["rad"]), ref["Q"], ref["R"], ref["rad"], ref["scale"], ref["bar"])


@pytest.mark.parametrize("case,family", ALL_CASES)
def test_exclude_self(lib, case, family):
    """Q = R, the same buffer: the search and the ball count without the pair i == i."""
    ref = reference(case, family, self_search=True)
    R, k = ref["R"], ref["k"]
    got_d, got_i = run_search(lib, R, R, k, exclude_self=True, same=True)
    check_search(got_d, got_i, R, R, k, ref["knn"][0], ref["scale"], ref["bar"], exclude_self=True)
    # at its own radius every row's k-th neighbour sits on the ball's edge (the band is open there); at 1.5 x it does not
    for rad in (ref["rad"], np.float32(1.5) * ref["rad"]):
        check_ball(run_ball(lib, R, R, rad, exclude_self=True, same=True), R, R, rad, ref["scale"], ref["bar"], exclude_self=True)


def test_k32_of_33_rows(lib):
    """The largest k: every other row of the set, in order."""
    R = np.random.default_rng(4100 + 8).standard_normal((33, 20)).astype(np.float32)
    got_d, got_i = run_search(lib, R, R, 32, exclude_self=True, same=True)
    want_d, _ = NR.knn(R, R, 32, exclude_self=True)
    check_search(got_d, got_i, R, R, 32, want_d, NR.scale(R, R), NR.bar(R, R), exclude_self=True)
    assert (np.sort(got_i, axis=1) == np.array([[j for j in range(33) if j != i] for i in range(33)])).all()


def test_one_row_and_one_column(lib):
    """nq = 1 and D = 1 beyond case 0: a reference set longer than a tile, ties among integers."""
    R = np.arange(300, dtype=np.float32)[:, None] % 7
    Q = np.array([[3.0]], np.float32)
    got_d, got_i = run_search(lib, Q, R, 4)
    assert got_d.tolist() == [[0.0] * 4] and got_i.tolist() == [[3, 10, 17, 24]]
    count = run_ball(lib, Q, R, np.full(300, 1.5, np.float32))  # d^2 is 0, 1, 4, ...: no distance near the radius
    assert count.tolist() == [int(((R[:, 0] - 3.0) ** 2 <= 1.5).sum())]


# ------------------------------------------------------------------ copies and ties ----
def test_planted_copies(lib):
    """Rows of Q overwritten with rows of R come out at exactly 0.0 at that index; two identical rows inside R find each
    other at 0.0 under exclude_self."""
    from fastfourierdiffusion_amd.utils import neighbours

    for family in NR.FAMILIES:
        Q, R, k = (a.copy() if isinstance(a, np.ndarray) else a for a in NR.make_case(4, family))
        planted = {0: 7, 63: 299, 64: 0, 129: 256}
        for qi, ri in planted.items():
            Q[qi] = R[ri]
        got_d, got_i = run_search(lib, Q, R, k)
        for qi, ri in planted.items():
            assert got_d[qi, 0] == 0.0 and got_i[qi, 0] == ri, (family, qi, got_d[qi], got_i[qi])
        assert ((got_d[:, 0] == 0.0).sum()) == len(planted)
        check_search(got_d, got_i, Q, R, k, NR.knn(Q, R, k)[0], NR.scale(Q, R), NR.bar(Q, R))
        got = neighbours.manifold_scores(R, Q, k)
        want = NR.scores(R, Q, k)
        assert got["copy_share"] == want["copy_share"] == len(planted) / Q.shape[0]
        assert got["authenticity"] == want["authenticity"], (family, got, want)
        assert got["nn_distance_min"] == 0.0
        R2 = R.copy()
        R2[200] = R2[3]
        got_d, got_i = run_search(lib, R2, R2, k, exclude_self=True, same=True)
        assert got_d[3, 0] == 0.0 and got_i[3, 0] == 200 and got_d[200, 0] == 0.0 and got_i[200, 0] == 3
        assert (got_d[:, 0] == 0.0).sum() == 2


def test_ties_go_to_the_lower_index(lib):
    """A reference set with a row repeated at indices on both sides of a tile and chunk edge: equal distances, listed by
    index -- at every workspace budget."""
    Q, R, _ = (a.copy() if isinstance(a, np.ndarray) else a for a in NR.make_case(3, "gaussian"))
    twins = [5, 63, 64, 255, 256]
    for j in twins:
        R[j] = R[twins[0]]
    Q[10] = R[twins[0]] + np.float32(0.25)
    Q[64] = R[twins[0]]
    for budget in (0, DEFAULT_BUDGET):
        got_d, got_i = run_search(lib, Q, R, 6, budget=budget)
        for qi in (10, 64):
            assert got_i[qi, :5].tolist() == twins and len(set(got_d[qi, :5].tolist())) == 1, (budget, got_i[qi], got_d[qi])
        assert got_d[64, 0] == 0.0 and got_d[10, 0] > 0.0


# ------------------------------------------------------------------ bit-identity ----
@pytest.mark.parametrize("case,family", [(3, "clustered"), (4, "gaussian"), (6, "clustered"), (7, "gaussian")])
def test_bits_do_not_depend_on_run_budget_or_query_cut(lib, case, family):
    ref = reference(case, family)
    Q, R, k = ref["Q"], ref["R"], ref["k"]
    nq, nr, D = Q.shape[0], R.shape[0], Q.shape[1]
    base = run_search(lib, Q, R, k)
    smallest = lib.ffd_nn_work_bytes(nq, nr, D, k, 0)
    assert smallest < lib.ffd_nn_work_bytes(nq, nr, D, k, 2 * UNIT) <= lib.ffd_nn_work_bytes(nq, nr, D, k, DEFAULT_BUDGET)
    for budget in (DEFAULT_BUDGET, 0, 2 * UNIT, 5 * UNIT):
        again = run_search(lib, Q, R, k, budget=budget)
        assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1]), budget
    if nq > 1:
        h = nq // 2 + 1
        parts = [run_search(lib, Q[:h], R, k, budget=0), run_search(lib, Q[h:], R, k)]
        assert np.array_equal(base[0], np.concatenate([p[0] for p in parts]))
        assert np.array_equal(base[1], np.concatenate([p[1] for p in parts]))
    counts = run_ball(lib, Q, R, ref["rad"])
    assert np.array_equal(counts, run_ball(lib, Q, R, ref["rad"]))
    if nq > 1:
        assert np.array_equal(counts, np.concatenate([run_ball(lib, Q[:h], R, ref["rad"]), run_ball(lib, Q[h:], R, ref["rad"])]))
    self_a = run_search(lib, R, R, min(k, nr - 1), exclude_self=True, same=True, budget=0)
    self_b = run_search(lib, R, R, min(k, nr - 1), exclude_self=True, same=True)
    assert np.array_equal(self_a[0], self_b[0]) and np.array_equal(self_a[1], self_b[1])


# ------------------------------------------------------------------ scores and the metric ----
def _device_arrays(Y, X, k):
    """The six arrays ffd_nn_scores reads, from the library's own primitives, as host arrays."""
    from fastfourierdiffusion_amd.utils import neighbours

    y, x = _dev(Y), _dev(X)
    self_y, rad_y = neighbours.self_search(y, k)
    _, rad_x = neighbours.self_search(x, k)
    xy_d2, xy_idx = neighbours.nearest_neighbours(x, y, 1)
    yx_d2, _ = neighbours.nearest_neighbours(y, x, 1)
    count_x, count_y = neighbours.ball_counts(x, y, rad_y), neighbours.ball_counts(y, x, rad_x)
    assert rad_y.dtype == torch.float32 and np.array_equal(rad_y.cpu().numpy(), self_y[:, k - 1].cpu().numpy().astype(np.float32))
    return [t.cpu().numpy() for t in (self_y, xy_d2, xy_idx, yx_d2, count_x, count_y)]


@pytest.mark.parametrize("case", [4, 6])
@pytest.mark.parametrize("family", NR.FAMILIES)
def test_manifold_metrics_against_the_float64_pipeline(lib, case, family):
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics

    ref = reference(case, family)
    X, Y, k = ref["Q"].copy(), ref["R"].copy(), ref["k"]
    metric = ManifoldMetrics(Y, k=k)
    got = metric(X)
    assert tuple(got) == NR.KEYS
    # the eight numbers are the float64 evaluation of the device's own arrays
    own = NR.scores_from_arrays(*_device_arrays(Y, X, k), k)
    for key in NR.KEYS:
        assert abs(got[key] - own[key]) <= 1e-12 * max(1.0, abs(own[key])), (key, got[key], own[key])
    want = NR.scores(Y, X, k)
    # A radius is itself a search result, up to one bar above float64's, and the count (or the coverage comparison) on
    # it has a bar of its own: two bars, each the widest of the four primitives' own (bar, scale).
    s = max(ref["scale"], NR.scale(Y, X), NR.scale(X, X), NR.scale(Y, Y))
    bar = max(ref["bar"], NR.bar(Y, X), NR.bar(X, X), NR.bar(Y, Y))
    lo, hi = NR.scores(Y, X, k, shift=-2.0 * bar * s), NR.scores(Y, X, k, shift=2.0 * bar * s)
    print({key: (got[key], want[key]) for key in NR.KEYS})
    for key in ("precision", "recall", "density", "coverage"):
        assert lo[key] <= got[key] <= hi[key], (key, lo[key], got[key], hi[key])
    if family == "gaussian":  # the band is closed: the share-valued keys are float64's own
        for key in ("precision", "recall", "coverage", "authenticity", "density", "copy_share"):
            assert lo[key] == hi[key] == want[key]
            assert got[key] == want[key], (key, got[key], want[key])
    # d(x, Y): the squared distances lie within [-1e-12, bar] scale of float64's, so the distances within that over 2 d
    d_min = want["nn_distance_min"]
    for key in ("nn_distance_mean", "nn_distance_min"):
        assert -1e-12 * ref["scale"] <= (got[key] - want[key]) * 2.0 * d_min <= ref["bar"] * ref["scale"], \
            (key, got[key], want[key])
    # the cached original set gives the bits of a fresh object
    assert metric._original_self is not None
    assert metric(X) == got and ManifoldMetrics(Y, k=k)(X) == got
    base = metric.baseline_metrics
    n = Y.shape[0]
    own = NR.scores_from_arrays(*_device_arrays(Y[: n // 2], Y[n // 2:], k), k)
    assert tuple(base) == tuple(f"{key}_self" for key in NR.KEYS)
    for key in NR.KEYS:
        assert abs(base[f"{key}_self"] - own[key]) <= 1e-12 * max(1.0, abs(own[key])), key


def test_metric_collection_in_time_and_frequency(lib):
    from fastfourierdiffusion_amd.sampling import metrics as M
    from fastfourierdiffusion_amd.utils.fourier import dft

    ref = reference(5, "gaussian")
    Y, X, k = ref["Q"][:, :, None].copy(), ref["R"][:, :, None].copy(), 4  # (257, 60, 1) originals, (129, 60, 1) samples
    coll = M.MetricCollection([partial(M.ManifoldMetrics, k=k),
                               partial(M.SlicedWasserstein, random_seed=3, num_directions=8)],
                              original_samples=torch.from_numpy(Y))
    found = coll(torch.from_numpy(X))
    for prefix, view in (("time", lambda a: a), ("freq", lambda a: dft(torch.from_numpy(a)).cpu().numpy())):
        y, x = view(Y).reshape(Y.shape[0], -1), view(X).reshape(X.shape[0], -1)
        alone = M.ManifoldMetrics(y, k=k)  # the collection adds nothing to the metric's own numbers
        for key, value in {**alone(x), **alone.baseline_metrics}.items():
            assert found[f"{prefix}_{key}"] == value, (prefix, key)
        s = max(NR.scale(x, y), NR.scale(y, x), NR.scale(x, x), NR.scale(y, y))
        bar = max(NR.bar(x, y), NR.bar(y, x), NR.bar(x, x), NR.bar(y, y))
        lo, hi = NR.scores(y, x, k, shift=-2.0 * bar * s), NR.scores(y, x, k, shift=2.0 * bar * s)  # two bars: see above
        for key in ("precision", "recall", "density", "coverage"):
            assert lo[key] <= found[f"{prefix}_{key}"] <= hi[key], (prefix, key, lo[key], found[f"{prefix}_{key}"], hi[key])
        assert f"{prefix}_sliced_wasserstein_mean" in found and f"{prefix}_nn_distance_min_self" in found
    assert list(found) == sorted(found) and not any("manifold" in key or key.endswith("nn_distance_dummy") for key in found)
