"""CPU-side tests of the nearest-neighbour statistics (no GPU): the C surface and its argument checks, the Python surface
(``utils.neighbours``, ``ManifoldMetrics``: refusals, keys, composition on a fake native layer) and the numpy
restatement (tests/neighbours_restatement.py) against formulations it shares no code with, the reason the Gram form is
centred, and the facts about the ball-count band that keep the GPU tests from hiding a failure -- for the size cases of
tests/test_neighbours_sizes_gpu.py too: the gapped radii close the band on every row, the row-subset restatement is the
whole one on its rows, and the integer rows of the limit tests are exact in the fp32 Gram form."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import neighbours_restatement as NR
from host_entry_checks import HostBuffers, checks_work, refuses_every_alias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_nn_work_bytes", "ffd_nn_search", "ffd_nn_ball_count", "ffd_nn_radius", "ffd_nn_scores")
ALL_CASES = [(c, f) for f in NR.FAMILIES for c in range(len(NR.CASES))]
SIZE_CASES = [(i, f) for f in NR.FAMILIES for i in range(len(NR.SIZE_CASES))]


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


# ------------------------------------------------------------------ the C surface ----
def _header_args(header, name):
    decl = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert decl, name
    params = [" ".join(p.split()) for p in decl.group(2).split(",")]
    return decl.group(1), [p.rsplit(" ", 1)[0].replace(" *", "*") for p in params]


def test_symbols_header_and_argtypes(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    assert re.search(r"enum\s*\{\s*FFD_NN_MAX_K\s*=\s*32\s*\}", header)
    ctype = {"int": C.c_int, "size_t": C.c_size_t}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype.get(a, C.c_void_p) for a in args] == list(want_args), (name, args)
        assert all(a in ctype or a.endswith("*") for a in args), (name, args)
    assert len(_header_args(header, "ffd_nn_search")[1]) == 12
    assert len(_header_args(header, "ffd_nn_ball_count")[1]) == 11
    assert len(_header_args(header, "ffd_nn_scores")[1]) == 11


def test_work_bytes_monotone_and_nonzero(lib):
    """At budget 0 (one 64 x 256 tile), a middle budget and one no shape here exhausts."""
    values = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 1025, 8193, 60000)
    for budget in (0, 1 << 20, 3 << 20, 1 << 24, 1 << 32):
        base = [65, 257, 17, 5]
        assert lib.ffd_nn_work_bytes(*base, budget) > 0
        for axis in range(4):
            prev = 0
            for v in values:
                if axis == 3 and v > 32:
                    break
                shape = list(base)
                shape[axis] = v
                b = lib.ffd_nn_work_bytes(*shape, budget)
                assert b > 0 and b >= prev, (budget, axis, v, b, prev)
                prev = b
    prev = 0
    for budget in (0, 1, 65535, 65536, 65537, 1 << 17, 1 << 20, 1 << 24, 1 << 30):
        b = lib.ffd_nn_work_bytes(1000, 5000, 187, 5, budget)
        assert b >= prev > -1
        prev = b
    assert lib.ffd_nn_work_bytes(1, 1, 1, 1, 0) >= 64 * 256 * 4
    assert lib.ffd_nn_work_bytes(1 << 24, 1 << 24, 1 << 16, 32, 0) > 0
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0), (4, 4, 4, 33), (-1, 4, 4, 1),
                ((1 << 24) + 1, 4, 4, 1), (4, (1 << 24) + 1, 4, 1), (4, 4, (1 << 16) + 1, 1)):
        assert lib.ffd_nn_work_bytes(*bad, 0) == 0, bad


def test_argument_errors_before_device_work(lib):
    nq, nr, D, k = 6, 9, 5, 3
    need = lib.ffd_nn_work_bytes(nq, nr, D, k, 0)
    b = HostBuffers(q=nq * D * 4, r=nr * D * 4, rad=nr * 4, dist2=nq * k * 8, index=nq * k * 4, count=nq * 4, work=need,
                    out8=64, f64=max(nq, nr) * k * 8, i32=max(nq, nr) * 4)

    def search(query=b.q, nq=nq, ref=b.r, nr=nr, D=D, k=k, excl=0, dist2=b.dist2, index=b.index, work=b.work, nbytes=need):
        return lib.ffd_nn_search(query, nq, ref, nr, D, k, excl, dist2, index, work, nbytes, None)

    def ball(query=b.q, nq=nq, ref=b.r, nr=nr, D=D, rad=b.rad, excl=0, count=b.count, work=b.work, nbytes=need):
        return lib.ffd_nn_ball_count(query, nq, ref, nr, D, rad, excl, count, work, nbytes, None)

    common = (dict(query=None), dict(ref=None), dict(work=None), dict(nq=0), dict(nr=0), dict(D=0), dict(nq=-1), dict(D=-3),
              dict(excl=1), dict(query=b.r, excl=1), dict(nbytes=0), dict(nbytes=need - 64 * 256 * 4), dict(work=b.work + 4),
              dict(work=b.q), dict(work=b.r))
    for kw in common:
        assert search(**kw) == INVALID, kw
        assert ball(**kw) == INVALID, kw
    for kw in (dict(dist2=None), dict(index=None), dict(k=0), dict(k=-1), dict(k=33), dict(k=nr + 1), dict(nr=2, k=3),
               dict(query=b.r, nq=nr, excl=1, k=nr), dict(dist2=b.q), dict(dist2=b.r), dict(index=b.q), dict(index=b.r),
               dict(index=b.dist2), dict(dist2=b.work), dict(index=b.work + 64), dict(nbytes=need - 1)):
        assert search(**kw) == INVALID, kw
    for kw in (dict(rad=None), dict(count=None), dict(count=b.q), dict(count=b.r), dict(count=b.rad), dict(count=b.work),
               dict(rad=b.work)):
        assert ball(**kw) == INVALID, kw
    assert ball(nbytes=lib.ffd_nn_work_bytes(nq, nr, D, 1, 0) - 1) == INVALID
    # every written region on every other region; the workspace misaligned, a byte short, and exactly the need
    assert refuses_every_alias(search, dict(dist2=b.dist2, index=b.index, work=b.work), dict(query=b.q, ref=b.r)) == 12
    assert refuses_every_alias(partial(search, query=b.r, nq=nr), dict(dist2=b.dist2, index=b.index, work=b.work),
                               dict(ref=b.r)) == 9  # the same-set form
    assert refuses_every_alias(ball, dict(count=b.count, work=b.work), dict(query=b.q, ref=b.r, rad=b.rad)) == 8
    checks_work(search, b.work, need)
    checks_work(ball, b.work, lib.ffd_nn_work_bytes(nq, nr, D, 1, 0))
    big = (1 << 24) + 1
    assert search(nr=big) == UNSUPPORTED and search(nq=big) == UNSUPPORTED and search(D=(1 << 16) + 1) == UNSUPPORTED
    assert ball(nr=big) == UNSUPPORTED and ball(D=(1 << 16) + 1) == UNSUPPORTED

    def radius(d=b.f64, n=nq, k=k, col=k - 1, out=b.rad):
        return lib.ffd_nn_radius(d, n, k, col, out, None)

    for kw in (dict(d=None), dict(out=None), dict(n=0), dict(k=0), dict(k=33), dict(col=-1), dict(col=k), dict(out=b.f64)):
        assert radius(**kw) == INVALID, kw
    assert refuses_every_alias(radius, dict(out=b.rad), dict(d=b.f64)) == 1

    def scores(s=b.f64, xd=b.dist2, xi=b.index, yd=b.work, cx=b.count, cy=b.i32, n=nr, m=nq, k=k, out=b.out8):
        return lib.ffd_nn_scores(s, xd, xi, yd, cx, cy, n, m, k, out, None)

    for kw in (dict(s=None), dict(xd=None), dict(xi=None), dict(yd=None), dict(cx=None), dict(cy=None), dict(out=None),
               dict(n=0), dict(m=0), dict(k=0), dict(k=33), dict(out=b.f64), dict(out=b.count)):
        assert scores(**kw) == INVALID, kw
    assert refuses_every_alias(scores, dict(out=b.out8), dict(s=b.f64, xd=b.dist2, xi=b.index, yd=b.work, cx=b.count,
                                                              cy=b.i32)) == 6
    assert b.untouched()


# ------------------------------------------------------------------ the Python surface ----
class _FakeLib:
    """Stands in for libffd: reads the arrays the binding passes (host memory here) and answers with the restatement."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).reshape(shape)

    def ffd_nn_work_bytes(self, nq, nr, D, k, budget):
        return 64

    def ffd_nn_search(self, q, nq, r, nr, D, k, excl, dist2, index, work, nbytes, stream):
        Q, R = self._arr(q, (nq, D), np.float32), self._arr(r, (nr, D), np.float32)
        self.calls.append(("search", nq, nr, k, excl, q == r))
        d, i = NR.knn(Q, R, k, bool(excl))
        self._arr(dist2, (nq, k), np.float64)[:] = d
        self._arr(index, (nq, k), np.int32)[:] = i
        return 0

    def ffd_nn_ball_count(self, q, nq, r, nr, D, rad, excl, count, work, nbytes, stream):
        Q, R = self._arr(q, (nq, D), np.float32), self._arr(r, (nr, D), np.float32)
        self.calls.append(("ball", nq, nr, excl))
        self._arr(count, (nq,), np.int32)[:] = NR.ball_counts(Q, R, self._arr(rad, (nr,), np.float32), bool(excl))
        return 0

    def ffd_nn_radius(self, dist2, n, k, col, out, stream):
        self.calls.append(("radius", n, k, col))
        self._arr(out, (n,), np.float32)[:] = self._arr(dist2, (n, k), np.float64)[:, col].astype(np.float32)
        return 0

    def ffd_nn_scores(self, s, xd, xi, yd, cx, cy, n, m, k, out, stream):
        self.calls.append(("scores", n, m, k))
        got = NR.scores_from_arrays(self._arr(s, (n, k), np.float64), self._arr(xd, (m,), np.float64),
                                    self._arr(xi, (m,), np.int32), self._arr(yd, (n,), np.float64),
                                    self._arr(cx, (m,), np.int32), self._arr(cy, (n,), np.int32), k)
        self._arr(out, (8,), np.float64)[:] = [got[key] for key in NR.KEYS]
        return 0


def _host_rows(x):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    assert t.dim() == 2
    return t.to(torch.float32).contiguous()


@pytest.fixture
def fake(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import metrics
    from fastfourierdiffusion_amd.utils import neighbours

    f = _FakeLib()
    monkeypatch.setattr(metrics, "_to_device", _host_rows)
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    monkeypatch.setattr(neighbours, "_to_device", _host_rows)
    return f


def test_python_refusals(monkeypatch, fake):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics
    from fastfourierdiffusion_amd.utils import neighbours

    Q, R, _ = NR.make_case(1, "gaussian")
    for k in (0, 33, R.shape[0] + 1):
        with pytest.raises(AssertionError):
            neighbours.nearest_neighbours(Q, R, k)
    with pytest.raises(AssertionError):
        neighbours.nearest_neighbours(R, R, R.shape[0], exclude_self=True)
    with pytest.raises(AssertionError):
        neighbours.nearest_neighbours(Q, R, 2, exclude_self=True)  # not the same set
    with pytest.raises(AssertionError):
        neighbours.nearest_neighbours(Q[:, :3], R, 2)
    with pytest.raises(AssertionError):
        neighbours.ball_counts(Q, R, np.ones(R.shape[0] - 1, np.float32))
    for k in (0, 33):
        with pytest.raises(AssertionError):
            ManifoldMetrics(R, k=k)
    with pytest.raises(AssertionError):
        ManifoldMetrics(R[:5], k=5)
    metric = ManifoldMetrics(R, k=5)
    with pytest.raises(AssertionError):
        metric(Q[:5])  # fewer than k + 1 samples
    metric(Q[:6])
    with pytest.raises(AssertionError):
        ManifoldMetrics(R[:11], k=5).baseline_metrics  # a half of 5 rows
    # without a device: a clear error, no fallback
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        neighbours.nearest_neighbours(Q, R, 2)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        neighbours.ball_counts(Q, R, np.ones(R.shape[0], np.float32))
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        ManifoldMetrics(R, k=3)(Q)


def test_manifold_metrics_keys_cache_and_collection(fake):
    from fastfourierdiffusion_amd.sampling import metrics as M

    Q, R, k = NR.make_case(1, "clustered")
    metric = M.ManifoldMetrics(R, k=k)
    assert metric.name == "manifold" and isinstance(metric, M.Metric)
    got = metric(Q)
    assert tuple(got) == NR.KEYS and all(isinstance(v, float) for v in got.values())
    want = NR.scores(R, Q, k)
    assert got == want
    kinds = [c[0] for c in fake.calls]
    assert kinds.count("search") == 4 and kinds.count("ball") == 2 and kinds.count("scores") == 1
    assert ("search", R.shape[0], R.shape[0], k, 1, True) in fake.calls
    assert ("search", Q.shape[0], R.shape[0], 1, 0, False) in fake.calls
    fake.calls.clear()
    assert metric(Q) == got
    assert [c[0] for c in fake.calls].count("search") == 3  # the originals' self-search is kept
    base = metric.baseline_metrics
    assert tuple(base) == tuple(f"{key}_self" for key in NR.KEYS)
    n = R.shape[0]
    assert base == {f"{key}_self": v for key, v in NR.scores(R[: n // 2], R[n // 2:], k).items()}
    assert not any(key.endswith("_dummy") for key in base)


def test_metric_collection_composes_the_metric(fake, monkeypatch):
    from fastfourierdiffusion_amd.sampling import metrics as M

    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x)[:, ::-1].copy())  # any other view of the rows
    Q, R, k = NR.make_case(1, "gaussian")
    coll = M.MetricCollection([partial(M.ManifoldMetrics, k=k)], original_samples=R)
    found = coll(Q)
    want = sorted([f"{p}_{key}" for p in ("time", "freq") for key in NR.KEYS] +
                  [f"{p}_{key}_self" for p in ("time", "freq") for key in NR.KEYS])
    assert list(found) == want
    assert found["time_precision"] == NR.scores(R, Q, k)["precision"]


def test_identical_and_far_sets(fake):
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics

    for case in (1, 4):
        _, R, k = NR.make_case(case, "clustered")
        same = ManifoldMetrics(R, k=k)(R.copy())
        assert same["precision"] == 1.0 and same["recall"] == 1.0 and same["coverage"] == 1.0
        assert same["authenticity"] == 0.0 and same["copy_share"] == 1.0 and same["nn_distance_min"] == 0.0
        # the ball of y holds y itself and its nearest neighbours short of the k-th (its fp32 radius may round below it)
        assert same["density"] >= 1.0
        far = ManifoldMetrics(R, k=k)(R + np.float32(1000.0))
        assert far["precision"] == 0.0 and far["recall"] == 0.0 and far["density"] == 0.0 and far["coverage"] == 0.0
        assert far["authenticity"] == 1.0 and far["copy_share"] == 0.0 and far["nn_distance_min"] > 100.0


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("case,family", ALL_CASES)
def test_restatement_against_a_sort_of_the_expanded_form(case, family):
    """A second formulation: float64 distances from one subtraction array and np.sum, a lexsort over (value, index) per
    row; the distances agree to summation order and the index sets agree wherever the k-th gap exceeds that."""
    Q, R, k = NR.make_case(case, family)
    d = ((Q.astype(np.float64)[:, None, :] - R.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    want_d, want_i = NR.knn(Q, R, k)
    s = NR.scale(Q, R)
    for i in range(Q.shape[0]):
        order = np.lexsort((np.arange(R.shape[0]), d[i]))[:k]
        assert np.abs(d[i][order] - want_d[i]).max() <= 1e-12 * s
        assert np.abs(NR.dist2(Q[i:i + 1], R[want_i[i]])[0] - want_d[i]).max() == 0.0
        assert len(set(want_i[i].tolist())) == k and want_i[i].min() >= 0 and want_i[i].max() < R.shape[0]
        assert (np.diff(want_d[i]) >= 0).all()
    rad = NR.self_radius2(R, k)
    assert rad.dtype == np.float32 and rad.shape == (R.shape[0],)
    counts = NR.ball_counts(Q, R, rad)
    assert np.array_equal(counts, (d <= rad.astype(np.float64)[None, :]).sum(axis=1))


@pytest.mark.parametrize("case", [0, 1])
def test_restatement_against_a_python_loop(case):
    for family in NR.FAMILIES:
        Q, R, k = NR.make_case(case, family)
        got_d, got_i = NR.knn(R, R, min(k, R.shape[0] - 1), exclude_self=True)
        for i in range(R.shape[0]):
            pairs = []
            for j in range(R.shape[0]):
                if j != i:
                    acc = 0.0
                    for d in range(R.shape[1]):
                        t = float(R[i, d]) - float(R[j, d])
                        acc += t * t
                    pairs.append((acc, j))
            pairs.sort()
            kk = got_d.shape[1]
            assert [j for _, j in pairs[:kk]] == got_i[i].tolist()
            assert [v for v, _ in pairs[:kk]] == got_d[i].tolist()
        # ties: a repeated row is found at 0.0, the lower index first
        R2 = np.concatenate([R, R[:2]])
        d, idx = NR.knn(R2, R2, 1, exclude_self=True)
        n = R.shape[0]
        assert d[0, 0] == 0.0 and idx[0, 0] == n and idx[n, 0] == 0
        d, idx = NR.knn(R[:1], R2, 2)
        assert d[0].tolist() == [0.0, 0.0] and idx[0].tolist() == [0, n]


@pytest.mark.parametrize("case,family", ALL_CASES)
def test_row_subsets_of_the_restatement(case, family):
    """``knn_rows`` and ``ball_counts(rows=...)`` are ``knn`` and ``ball_counts`` on their rows, with and without the pair
    i == i; ``size_radius2`` is ``self_radius2`` up to 8193 rows."""
    Q, R, k = NR.make_case(case, family)
    rng = np.random.default_rng(case)
    for A, kk, excl in ((Q, k, False), (R, min(k, R.shape[0] - 1), True)):
        rows = np.sort(rng.choice(A.shape[0], size=min(A.shape[0], 7), replace=False))
        rows[-1] = A.shape[0] - 1
        want_d, want_i = NR.knn(A, R, kk, exclude_self=excl)
        got_d, got_i = NR.knn_rows(A, R, kk, rows, exclude_self=excl)
        assert np.array_equal(got_d, want_d[rows]) and np.array_equal(got_i, want_i[rows]) and got_i.dtype == np.int32
        rad = NR.self_radius2(R, k)
        assert np.array_equal(NR.ball_counts(A, R, rad, excl, shift=1e-3, rows=rows), NR.ball_counts(A, R, rad, excl, shift=1e-3)[rows])
    got = NR.size_radius2(R, k)
    assert got.dtype == np.float32 and np.array_equal(got, NR.self_radius2(R, k))


def test_size_cases_follow_the_recipes_of_make_case():
    """Generator seed 5200 + i, the draws in the order of ``make_case``; the radii of a set longer than 8193 rows come
    from a 512-row subsample and still give balls holding a few rows."""
    assert len(NR.SIZE_CASES) == 8 and NR.SIZE_CASES[2] == (65, 16385, 8, 5)
    for i in (0, 4):
        nq, nr, D, k = NR.SIZE_CASES[i]
        rng = np.random.default_rng(5200 + i)
        R, Q = rng.standard_normal((nr, D)), rng.standard_normal((nq, D))
        got = NR.make_size_case(i, "gaussian")
        assert np.array_equal(got[0], Q.astype(np.float32)) and np.array_equal(got[1], R.astype(np.float32)) and got[2] == k
        rng = np.random.default_rng(5200 + i)
        c = 3 * rng.standard_normal((4, D)) + 10
        R = c[rng.integers(0, 4, nr)] + 0.5 * rng.standard_normal((nr, D))
        Q = c[rng.integers(0, 4, nq)] + 0.5 * rng.standard_normal((nq, D))
        got = NR.make_size_case(i, "clustered")
        assert np.array_equal(got[0], Q.astype(np.float32)) and np.array_equal(got[1], R.astype(np.float32))


@pytest.mark.parametrize("i,family", SIZE_CASES)
def test_gapped_radii_close_every_band(i, family):
    """At ``gapped_radii`` float64's counts at radius^2 -+ bar scale coincide for EVERY row of every size case, so the GPU
    test's second ball count is an equality test; at the radii as they are the band is open for the printed rows."""
    Q, R, k = NR.make_size_case(i, family)
    assert (*Q.shape, R.shape[0], k) == (NR.SIZE_CASES[i][0], NR.SIZE_CASES[i][2], NR.SIZE_CASES[i][1], NR.SIZE_CASES[i][3])
    bar, s = NR.bar(Q, R), NR.scale(Q, R)
    assert 2e-6 <= bar <= 1e-5, bar
    rad = NR.size_radius2(R, k)
    n_open = int((NR.ball_counts(Q, R, rad, shift=-bar * s) != NR.ball_counts(Q, R, rad, shift=bar * s)).sum())
    gapped, moved = NR.gapped_radii(Q, R, rad, bar, s)
    assert gapped.dtype == np.float32 and (gapped >= rad).all() and int((gapped != rad).sum()) == moved
    lo, hi = NR.ball_counts(Q, R, gapped, shift=-bar * s), NR.ball_counts(Q, R, gapped, shift=bar * s)
    mid = NR.ball_counts(Q, R, gapped)
    print(f"size case {i} {family}: bar {bar:.3e}, scale {s:.4e}, band open for {n_open} of {Q.shape[0]} rows as they are; "
          f"{moved} of {len(rad)} radii moved, by at most {float((gapped - rad).max() / (4 * bar * s)):.2f} steps; mean count "
          f"{NR.ball_counts(Q, R, rad).mean():.1f} -> {mid.mean():.1f}")
    assert np.array_equal(lo, hi) and np.array_equal(lo, mid)
    d = NR.dist2(Q, R)
    assert (np.abs(d - gapped.astype(np.float64)[None, :]) > 2.0 * bar * s).all()
    assert 0 < mid.mean() < R.shape[0]  # neither no ball nor every ball


def test_integer_rows_are_exact_in_the_fp32_gram_form():
    """The inputs of the two limit tests: integers below 1021, D = 1.  The fp32 centred Gram form misses the integer squared
    distances by less than 0.5 in both directions while distinct ones differ by at least 1, no query of the long query
    set is equidistant from two reference rows, and every value of the long reference set occurs more than twice."""
    long_rows = NR.hashed_rows(NR.LIMIT_ROWS)
    assert long_rows.shape == (NR.LIMIT_ROWS, 1) and long_rows.dtype == np.float32
    assert long_rows.min() == 0.0 and long_rows.max() == 1020.0 and (long_rows == np.round(long_rows)).all()
    assert long_rows[:3, 0].tolist() == [0.0, 2654435761 % 1021, (2 * 2654435761 % (1 << 32)) % 1021]
    few = np.array(NR.LIMIT_REFERENCE, np.float32)[:, None]
    assert all((a + b) % 2 == 1 and a < b for a, b in zip(NR.LIMIT_REFERENCE, NR.LIMIT_REFERENCE[1:]))
    worst = 0.0
    for a in range(0, NR.LIMIT_ROWS, 1 << 21):  # the mean is the 5 rows': a block of queries at a time changes nothing
        block = long_rows[a:a + (1 << 21)]
        worst = max(worst, float(np.abs(NR.gram32(block, few).astype(np.float64) - NR.dist2(block, few)).max()))
    queries = np.array(NR.LIMIT_QUERIES, np.float32)[:, None]
    worst_r = float(np.abs(NR.gram32(queries, long_rows).astype(np.float64) - NR.dist2(queries, long_rows)).max())
    s = NR.scale(queries, long_rows)
    print(f"integer rows: scale {s:.3e}, Gram error {worst:.4f} (long query set), {worst_r:.4f} (long reference set)")
    assert worst < 0.5 and worst_r < 0.5 and 2.5e5 < s < 2.7e5
    assert np.bincount(long_rows[:, 0].astype(np.int64), minlength=1021).min() > 2
    # offset by 2^23 the rows are still integers in fp32; centred on their mean the Gram form is exact, uncentred it is not
    far = long_rows[:1025] + np.float32(NR.LIMIT_OFFSET)
    assert np.array_equal(far.astype(np.float64), long_rows[:1025].astype(np.float64) + NR.LIMIT_OFFSET)
    assert np.abs(NR.gram32(far[:70], far).astype(np.float64) - NR.dist2(far[:70], far)).max() == 0.0
    assert np.abs(NR.gram32(far[:70], far, centred=False).astype(np.float64) - NR.dist2(far[:70], far)).max() > 0.5


@pytest.mark.parametrize("case", [4, 6])
def test_centring_holds_the_bar_and_the_uncentred_gram_does_not(case):
    """Clustered rows 10 sqrt(D) from the origin, clusters 0.5 sqrt(D) wide: the fp32 Gram form of the rows as they are
    misses float64 by more than the bar; centred on the reference mean it holds it."""
    Q, R, _ = NR.make_case(case, "clustered")
    bar = NR.bar(Q, R)
    cen, unc = NR.e_ref(Q, R, centred=True), NR.e_ref(Q, R, centred=False)
    print(f"case {case}: bar {bar:.3e}, centred {cen:.3e}, uncentred {unc:.3e} of the scale {NR.scale(Q, R):.4e}")
    assert cen <= bar < unc
    assert unc > 3.0 * cen


@pytest.mark.parametrize("case,family", ALL_CASES)
def test_the_ball_count_band(case, family):
    """The GPU test accepts a count between float64's at radius^2 -+ bar scale.  On the Gaussian cases the two coincide for
    every row, so equality is what it tests; on a clustered case they may differ for at most 2 % of the rows."""
    Q, R, k = NR.make_case(case, family)
    rad = NR.self_radius2(R, k)
    bar, s = NR.bar(Q, R), NR.scale(Q, R)
    assert 2e-6 <= bar <= 1e-5, bar
    lo, hi = NR.ball_counts(Q, R, rad, shift=-bar * s), NR.ball_counts(Q, R, rad, shift=bar * s)
    mid = NR.ball_counts(Q, R, rad)
    assert (lo <= mid).all() and (mid <= hi).all()
    n_open = int((lo != hi).sum())
    print(f"case {case} {family}: bar {bar:.3e}, band open for {n_open} of {Q.shape[0]} rows")
    if family == "gaussian":
        assert n_open == 0
    else:
        assert n_open <= 0.02 * Q.shape[0]
