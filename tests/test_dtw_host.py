"""CPU-side tests of the dynamic-time-warping metrics (no GPU): the C surface and its argument checks, the Python surface
(``utils.dtw``, ``DTWMetrics``: refusals, keys, the kept self-search, views and composition on a fake native layer), the
numpy restatement (tests/dtw_restatement.py) against formulations it shares no code with, and the condition on the score
cases that lets the GPU test ask for float64's 1-NN counts exactly."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import dtw_restatement as DR
from host_entry_checks import HostBuffers, checks_work, one_host_prologue, refuses_every_alias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_dtw_work_bytes", "ffd_dtw_search", "ffd_dtw_pairs", "ffd_dtw_scores")


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
    from fastfourierdiffusion_amd.utils import dtw

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    limits = re.search(r"enum\s*\{\s*FFD_DTW_MAX_WINDOW\s*=\s*(\d+),\s*FFD_DTW_MAX_LEN\s*=\s*(\d+),\s*"
                       r"FFD_DTW_MAX_CHANNELS\s*=\s*(\d+),\s*FFD_DTW_MAX_K\s*=\s*(\d+)\s*\}", header)
    assert limits and tuple(int(v) for v in limits.groups()) == \
        (dtw.MAX_WINDOW, dtw.MAX_LEN, dtw.MAX_CHANNELS, dtw.MAX_K) == (64, 4096, 64, 32)
    ctype = {"int": C.c_int, "size_t": C.c_size_t}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype.get(a, C.c_void_p) for a in args] == list(want_args), (name, args)
        assert all(a in ctype or a.endswith("*") for a in args), (name, args)
    assert [len(_header_args(header, name)[1]) for name in NAMES] == [7, 14, 8, 9]
    csrc = os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "ffd_dtw.hip" in re.search(r"^SRCS := (.*)$", make, re.M).group(1)
    # one statement of the merge: the shared header has it, no source repeats it, the DTW source launches it
    shared = open(os.path.join(csrc, "ffd_pairtile.h")).read()
    for piece in ("void k_nn_merge(", "bool nn_before("):
        assert piece in shared, piece
        for source in ("ffd_neighbours.hip", "ffd_mmd.hip", "ffd_dtw.hip"):
            text = open(os.path.join(csrc, source)).read()
            assert piece not in text and '#include "ffd_pairtile.h"' in text, (piece, source)
    one_host_prologue(csrc)  # ... and one statement of the host prologue
    assert "hipLaunchKernelGGL(k_nn_merge" in open(os.path.join(csrc, "ffd_dtw.hip")).read()


def test_work_bytes_monotone_multiple_of_16_and_zero_for_refused(lib):
    base = dict(nq=65, nr=257, L=17, C=2, window=3, k=5, budget=1 << 20)
    order = tuple(base)
    sweeps = dict(nq=(1, 3, 63, 64, 65, 257, 4097, 60000, 1 << 24), nr=(5, 63, 64, 65, 256, 257, 8192, 8193, 1 << 24),
                  L=(1, 2, 17, 187, 512, 4096), C=(1, 2, 3, 64), window=(0, 1, 4, 5, 64, 5000), k=(1, 2, 5, 32),
                  budget=(0, 1, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 26, 1 << 30, 1 << 34))
    for axis, values in sweeps.items():
        prev = 0
        for v in values:
            shape = dict(base)
            shape[axis] = v
            if axis == "C":
                shape["L"] = 8
            b = lib.ffd_dtw_work_bytes(*(shape[key] for key in order))
            assert b >= 65536 and b >= prev and b % 16 == 0, (axis, v, b, prev)
            prev = b
    assert lib.ffd_dtw_work_bytes(1 << 24, 1 << 24, 4096, 16, 64, 32, 1 << 40) == (1 << 15) * 65536
    assert lib.ffd_dtw_work_bytes(2, 3, 4096, 1, 64, 1, 0) == 65536 == lib.ffd_dtw_work_bytes(2, 3, 50, 1, 5000, 1, 0)
    big = (1 << 24) + 1
    for bad in (dict(nq=0), dict(nr=0), dict(L=0), dict(C=0), dict(window=-1), dict(k=0), dict(k=33), dict(nq=-1),
                dict(k=6, nr=5), dict(nq=big), dict(nr=big), dict(L=4097, C=1), dict(C=65, L=8), dict(L=2048, C=33),
                dict(L=200, window=65), dict(L=4096, C=1, window=4095)):
        shape = dict(base)
        shape.update(bad)
        assert lib.ffd_dtw_work_bytes(*(shape[key] for key in order)) == 0, bad


def test_argument_errors_before_device_work(lib):
    nq, nr, L, Cn, w, k = 6, 9, 7, 2, 2, 3
    need = lib.ffd_dtw_work_bytes(nq, nr, L, Cn, w, k, 0)
    b = HostBuffers(q=nq * L * Cn * 4, r=nr * L * Cn * 4, d=nr * k * 4, i=nr * k * 4, work=need, pd=nr * 4, xx=nq * 4, xy=nq * 4,
                     e2=nq * 4, yx=nr * 4, yy=nr * 4, out6=48)

    def search(q=b.q, nq=nq, r=b.r, nr=nr, L=L, Cn=Cn, w=w, k=k, excl=0, d=b.d, i=b.i, work=b.work, nbytes=need):
        return lib.ffd_dtw_search(q, nq, r, nr, L, Cn, w, k, excl, d, i, work, nbytes, None)

    for kw in (dict(q=None), dict(r=None), dict(d=None), dict(i=None), dict(work=None), dict(nq=0), dict(nr=0), dict(L=0),
               dict(Cn=0), dict(nq=-1), dict(L=-3), dict(w=-1), dict(k=0), dict(k=33), dict(k=10), dict(k=-1), dict(excl=1),
               dict(q=b.r, excl=1), dict(q=b.r, nq=nr, excl=1, k=9), dict(nbytes=0), dict(nbytes=need - 1),
               dict(work=b.work + 4), dict(work=b.q), dict(work=b.r), dict(d=b.q), dict(d=b.r), dict(i=b.q), dict(i=b.r),
               dict(i=b.d), dict(d=b.work), dict(i=b.work)):
        assert search(**kw) == INVALID, kw
    # every written region on every other region, two sets and one; the workspace misaligned, a byte short, exactly the need
    assert refuses_every_alias(search, dict(d=b.d, i=b.i, work=b.work), dict(q=b.q, r=b.r)) == 12
    assert refuses_every_alias(partial(search, q=b.r, nq=nr), dict(d=b.d, i=b.i, work=b.work), dict(r=b.r)) == 9
    checks_work(search, b.work, need)
    big = (1 << 24) + 1
    for kw in (dict(nq=big), dict(nr=big), dict(L=4097, Cn=1), dict(Cn=65), dict(L=2048, Cn=33), dict(L=200, w=65),
               dict(L=4096, Cn=1, w=100)):
        assert search(**kw) == UNSUPPORTED, kw

    def pairs(a=b.q, bb=b.r, n=nq, L=L, Cn=Cn, w=w, d=b.pd):
        return lib.ffd_dtw_pairs(a, bb, n, L, Cn, w, d, None)

    for kw in (dict(a=None), dict(bb=None), dict(d=None), dict(n=0), dict(n=-2), dict(L=0), dict(Cn=0), dict(w=-1), dict(d=b.q),
               dict(d=b.r)):
        assert pairs(**kw) == INVALID, kw
    assert refuses_every_alias(pairs, dict(d=b.pd), dict(a=b.q, bb=b.r)) == 2
    for kw in (dict(n=big), dict(L=4097, Cn=1), dict(Cn=65), dict(L=2048, Cn=33), dict(L=200, w=65)):
        assert pairs(**kw) == UNSUPPORTED, kw

    def scores(xx=b.xx, xy=b.xy, yx=b.yx, yy=b.yy, e2=b.e2, n=nr, m=nq, out=b.out6):
        return lib.ffd_dtw_scores(xx, xy, yx, yy, e2, n, m, out, None)

    for kw in (dict(xx=None), dict(xy=None), dict(yx=None), dict(yy=None), dict(e2=None), dict(out=None), dict(n=1), dict(m=1),
               dict(n=0), dict(m=-1), dict(out=b.xx), dict(out=b.xy), dict(out=b.yx), dict(out=b.yy), dict(out=b.e2)):
        assert scores(**kw) == INVALID, kw
    assert refuses_every_alias(scores, dict(out=b.out6), dict(xx=b.xx, xy=b.xy, yx=b.yx, yy=b.yy, e2=b.e2)) == 5
    assert scores(n=big) == UNSUPPORTED and scores(m=big) == UNSUPPORTED
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

    def ffd_dtw_work_bytes(self, nq, nr, L, Cn, w, k, budget):
        return 64

    def ffd_dtw_search(self, q, nq, r, nr, L, Cn, w, k, excl, d, i, work, nbytes, stream):
        self.calls.append(("search", nq, nr, w, k, excl, q == r))
        D = DR.all_pairs(self._arr(q, (nq, L, Cn), np.float32), self._arr(r, (nr, L, Cn), np.float32), w)
        if excl:
            D[np.arange(nq), np.arange(nq)] = np.inf
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        self._arr(d, (nq, k), np.float32)[:] = np.take_along_axis(D, order, axis=1)
        self._arr(i, (nq, k), np.int32)[:] = order
        return 0

    def ffd_dtw_pairs(self, a, b, n, L, Cn, w, d, stream):
        self.calls.append(("pairs", n, w))
        self._arr(d, (n,), np.float32)[:] = DR.dtw2(self._arr(a, (n, L, Cn), np.float32), self._arr(b, (n, L, Cn), np.float32), w)
        return 0

    def ffd_dtw_scores(self, xx, xy, yx, yy, e2, n, m, out, stream):
        self.calls.append(("scores", n, m))
        s = {"xx": self._arr(xx, (m,), np.float32), "xy": self._arr(xy, (m,), np.float32), "yx": self._arr(yx, (n,), np.float32),
             "yy": self._arr(yy, (n,), np.float32), "e2": self._arr(e2, (m,), np.float32)}
        self._arr(out, (6,), np.float64)[:] = list(DR.scores_from_searches(s)[0].values())
        return 0


def _host(x):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.float32).contiguous()


@pytest.fixture
def fake(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import metrics
    from fastfourierdiffusion_amd.utils import dtw

    f = _FakeLib()
    monkeypatch.setattr(metrics, "_to_device", _host)
    monkeypatch.setattr(dtw, "_series", _host)
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    return f


def test_python_refusals_before_any_native_call(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import DTWMetrics
    from fastfourierdiffusion_amd.utils import dtw

    def no_native():
        raise AssertionError("a native call was reached")

    monkeypatch.setattr(N, "lib", no_native)
    monkeypatch.setattr(dtw, "_series", lambda x: no_native())
    A, B = DR.gaussian(6, 20, 2, 1), DR.gaussian(9, 20, 2, 2)
    # window forms
    assert dtw.resolve_window(0, 20) == 0 and dtw.resolve_window(5, 20) == 5 and dtw.resolve_window(np.int64(7), 20) == 7
    assert dtw.resolve_window(100, 20) == 19 and dtw.resolve_window(1.0, 20) == 19 and dtw.resolve_window(0.1, 187) == 19
    assert dtw.resolve_window(0.1, 190) == 19 and dtw.resolve_window(0.25, 20) == 5 and dtw.resolve_window(0.26, 20) == 6
    assert dtw.resolve_window(np.float32(0.5), 20) == 10 and dtw.resolve_window(64, 4096) == 64
    for bad in (-1, 0.0, 1.5, -0.2, "3", None, True, 2.0, [3], float("nan")):
        with pytest.raises(AssertionError):
            dtw.resolve_window(bad, 20)
        with pytest.raises(AssertionError):
            dtw.dtw_pairs(A, A, bad)
        with pytest.raises(AssertionError):
            dtw.dtw_neighbours(A, B, bad)
        with pytest.raises(AssertionError):
            DTWMetrics(B, window=bad)
    # a clipped window above 64
    long_a = np.zeros((3, 200, 1), np.float32)
    for window in (65, 0.5, 1.0, 199, 10 ** 6):
        with pytest.raises(NotImplementedError, match="64"):
            dtw.dtw_pairs(long_a, long_a, window)
        with pytest.raises(NotImplementedError, match="64"):
            dtw.dtw_neighbours(long_a, long_a, window)
        with pytest.raises(NotImplementedError, match="64"):
            DTWMetrics(long_a, window=window)
    assert dtw.resolve_window(10 ** 6, 65) == 64
    # shapes
    with pytest.raises(AssertionError):
        dtw.dtw_pairs(A, B, 2)  # paired rows: the same count
    with pytest.raises(AssertionError):
        dtw.dtw_pairs(A, A[:, :, :1], 2)
    with pytest.raises(AssertionError):
        dtw.dtw_pairs(A.reshape(6, 40), A.reshape(6, 40), 2)
    with pytest.raises(AssertionError):
        dtw.dtw_neighbours(A, B[:, :19], 2)
    with pytest.raises(AssertionError):
        dtw.dtw_neighbours(A, B[:, :, :1], 2)
    with pytest.raises(AssertionError):
        dtw.dtw_neighbours(A[0], B, 2)
    for k in (0, 33, 10):
        with pytest.raises(AssertionError):
            dtw.dtw_neighbours(A, B, 2, k=k)
    with pytest.raises(AssertionError):
        dtw.dtw_neighbours(B, B, 2, k=9, exclude_self=True)
    for shape in ((2, 4097, 1), (2, 8, 65), (2, 2048, 33)):
        with pytest.raises(NotImplementedError):
            dtw.dtw_pairs(np.zeros(shape, np.float32), np.zeros(shape, np.float32), 1)
    # rows
    with pytest.raises(AssertionError):
        dtw.dtw_scores(B, A[:1], 2)
    with pytest.raises(AssertionError):
        dtw.dtw_scores(B[:1], A, 2)
    with pytest.raises(AssertionError):
        DTWMetrics(B[:1])
    with pytest.raises(AssertionError):
        DTWMetrics(B.reshape(9, 40))  # (L, C) must come from the originals
    metric = DTWMetrics(B, window=2)
    assert (metric.length, metric.channels, metric.window) == (20, 2, 2) and DTWMetrics(B).window == 2
    monkeypatch.setattr("fastfourierdiffusion_amd.sampling.metrics._to_device", _host)
    with pytest.raises(AssertionError):
        metric(A[:1])
    with pytest.raises(AssertionError):
        metric(A[:, :19])
    with pytest.raises(AssertionError):
        DTWMetrics(B[:3]).baseline_metrics  # a half of 1 row
    # without a device: a clear error, no fallback
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        dtw.dtw_pairs(A, A, 2)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        dtw.dtw_neighbours(A, B, 2)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        DTWMetrics(B, window=2)(A)


def test_dtw_metrics_keys_kept_self_search_and_baseline(fake):
    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y, w = DR.score_case(0)
    metric = M.DTWMetrics(Y, window=w)
    assert metric.name == "dtw" and isinstance(metric, M.Metric) and metric.views == ("time",)
    assert M.Metric.views == ("time", "freq") == M.SlicedWasserstein.views == M.ManifoldMetrics.views == M.KernelMMD.views
    got = metric(X)
    assert tuple(got) == DR.SCORE_KEYS and all(isinstance(v, float) for v in got.values())
    want, _, _ = DR.pipeline(X, Y, w)
    for key, value in want.items():
        assert got[key] == pytest.approx(value, rel=1e-6, abs=1e-7), key  # (the fake layer hands fp32 arrays over)
    n, m = Y.shape[0], X.shape[0]
    assert fake.calls == [("search", n, n, w, 1, 1, True), ("search", m, m, w, 1, 1, True), ("search", m, n, w, 1, 0, False),
                          ("search", n, m, w, 1, 0, False), ("search", m, n, 0, 1, 0, False), ("scores", n, m)]
    fake.calls.clear()
    assert metric(X.reshape(m, -1)) == got  # (m, L C) samples
    assert [c[:3] for c in fake.calls] == [("search", m, m), ("search", m, n), ("search", n, m), ("search", m, n),
                                           ("scores", n, m)]  # the originals' self-search is kept
    base = metric.baseline_metrics
    assert tuple(base) == tuple(f"{key}_self" for key in DR.SCORE_KEYS)
    half = n // 2
    want_self, _, _ = DR.pipeline(Y[half:], Y[:half], w)
    for key, value in want_self.items():
        assert base[f"{key}_self"] == pytest.approx(value, rel=1e-6, abs=1e-7), key
    fake.calls.clear()
    zero = M.DTWMetrics(Y, window=0)(X)
    assert zero["dtw_warp_gain"] == 0.0 and len(fake.calls) == 5  # XY at window 0 is the search itself
    assert 0.0 <= got["dtw_warp_gain"] <= 1.0


def test_metric_collection_builds_the_metric_on_the_time_view_only(fake, monkeypatch):
    from fastfourierdiffusion_amd.sampling import DTWMetrics
    from fastfourierdiffusion_amd.sampling import metrics as M

    class Flat(M.Metric):  # a two-view metric standing where SlicedWasserstein would
        built = []

        def __init__(self, original_samples, tag):
            super().__init__(original_samples=original_samples)
            Flat.built.append(tag)

        def __call__(self, other):
            return {"flat": float(np.asarray(M.check_flat_array(other)).sum())}

        name = "flat"

    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x)[:, ::-1].copy())  # any other view of the rows
    X, Y, w = DR.score_case(1)
    alone = M.MetricCollection([partial(Flat, tag="a")], original_samples=Y)(X)
    coll = M.MetricCollection([partial(DTWMetrics, window=w), partial(Flat, tag="b")], original_samples=Y)
    assert Flat.built == ["a", "a", "b", "b"]
    assert [type(metric).__name__ for metric in coll.metrics_time] == ["DTWMetrics", "Flat"]
    assert coll.metrics_freq[0] is None and isinstance(coll.metrics_freq[1], Flat)
    found = coll(X)
    want = sorted([f"time_{key}" for key in DR.SCORE_KEYS] + [f"time_{key}_self" for key in DR.SCORE_KEYS] +
                  ["time_flat", "freq_flat"])
    assert list(found) == want and not any(key.startswith("freq_dtw") for key in found)
    assert {key: found[key] for key in alone} == alone  # the other metric's keys and values as without DTW
    assert found["time_dtw_1nn_accuracy"] == DR.pipeline(X, Y, w)[0]["dtw_1nn_accuracy"]


def test_metric_collection_with_sliced_wasserstein_keys(monkeypatch):
    """``DTWMetrics`` beside ``SlicedWasserstein``: the Wasserstein keys of both views as before, DTW keys under
    ``time_`` only (the metrics themselves are replaced by their key sets: no native layer here)."""
    from fastfourierdiffusion_amd.sampling import metrics as M

    def keys_only(cls, keys):
        monkeypatch.setattr(cls, "__call__", lambda self, other: {key: 0.0 for key in keys})
        monkeypatch.setattr(cls, "baseline_metrics", property(lambda self: {f"{key}_self": 0.0 for key in keys}))

    sw_keys = ("sliced_wasserstein_mean", "sliced_wasserstein_max")
    keys_only(M.SlicedWasserstein, sw_keys)
    keys_only(M.DTWMetrics, DR.SCORE_KEYS)
    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x))
    Y = DR.gaussian(8, 12, 2, 5)
    sliced = partial(M.SlicedWasserstein, random_seed=1, num_directions=4)
    before = M.MetricCollection([sliced], original_samples=Y)(Y)
    after = M.MetricCollection([sliced, partial(M.DTWMetrics, window=2)], original_samples=Y)(Y)
    assert [key for key in after if "dtw" not in key] == list(before)
    dtw_keys = [key for key in after if "dtw" in key]
    assert len(dtw_keys) == 12 and all(key.startswith("time_dtw_") for key in dtw_keys)


# ------------------------------------------------------------------ the restatement ----
def _loop_dtw2(a, b, w):
    """The definition as a plain Python triple loop over (i, j, ch), float64."""
    L, Cn = a.shape
    w = min(w, L - 1)
    D = [[float("inf")] * L for _ in range(L)]
    for i in range(L):
        for j in range(L):
            if abs(i - j) > w:
                continue
            c = 0.0
            for ch in range(Cn):
                c += (float(a[i, ch]) - float(b[j, ch])) ** 2
            if i == 0 and j == 0:
                D[i][j] = c
                continue
            best = float("inf")
            if i > 0:
                best = min(best, D[i - 1][j])
            if j > 0:
                best = min(best, D[i][j - 1])
            if i > 0 and j > 0:
                best = min(best, D[i - 1][j - 1])
            D[i][j] = c + best
    return D[L - 1][L - 1]


@pytest.mark.parametrize("family", sorted(DR.FAMILIES))
def test_restatement_is_the_triple_loop(family):
    worst = 0.0
    for L, Cn, seed in ((1, 1, 0), (2, 3, 1), (3, 1, 2), (9, 2, 3), (17, 1, 4), (24, 3, 5)):
        A, B = DR.FAMILIES[family](4, L, Cn, 100 + seed), DR.FAMILIES[family](4, L, Cn, 200 + seed)
        for w in (0, 1, 2, 3, 5, L - 1, L + 7):
            got = DR.dtw2(A, B, w)
            want = np.array([_loop_dtw2(A[p], B[p], w) for p in range(4)])
            worst = max(worst, float(np.abs(got - want).max() / max(want.max(), 1e-300)))
    print(f"{family}: restatement against the triple loop, largest relative difference {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("family", sorted(DR.FAMILIES))
def test_restatement_properties(family):
    A, B = DR.FAMILIES[family](7, 31, 2, 300), DR.FAMILIES[family](7, 31, 2, 301)
    euclid = ((A.astype(np.float64) - B.astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert np.abs(DR.dtw2(A, B, 0) - euclid).max() <= 1e-13 * euclid.max()
    for dtype in (np.float64, np.float32):
        prev = DR.dtw2(A, B, 0, dtype)
        assert prev.dtype == dtype
        for w in (1, 2, 3, 4, 8, 16, 30, 31, 500):
            cur = DR.dtw2(A, B, w, dtype)
            assert (cur <= prev).all() and (cur <= DR.dtw2(A, B, 0, dtype)).all(), (dtype, w)  # non-increasing in w
            assert np.array_equal(cur, DR.dtw2(B, A, w, dtype)), (dtype, w)  # symmetric to the bit
            assert (DR.dtw2(A, A.copy(), w, dtype) == 0.0).all()  # a copy reads exactly 0.0
            prev = cur
        assert np.array_equal(DR.dtw2(A, B, 30, dtype), DR.dtw2(A, B, 500, dtype))  # clipped to L - 1
    P = DR.all_pairs(A[:3], B, 3)
    assert P.shape == (3, 7) and np.array_equal(P[1], DR.dtw2(np.repeat(A[1:2], 7, axis=0), B, 3))


def test_shifted_pulse_costs_nothing_inside_the_band():
    for Cn in (1, 2):
        for w in (0, 1, 3, 4, 8):
            for dtype in (np.float64, np.float32):
                for s in range(w + 1):
                    a, b = DR.shifted_pulse(40, Cn, s)
                    assert DR.dtw2(a, b, w, dtype)[0] == 0.0, (Cn, w, s, dtype)
                a, b = DR.shifted_pulse(40, Cn, w + 1)
                assert DR.dtw2(a, b, w, dtype)[0] > 0.0, (Cn, w, dtype)


def test_integer_rows_are_exact_in_fp32():
    A, B = DR.integer_rows(9, 33, 2, 7), DR.integer_rows(9, 33, 2, 8)
    for w in (0, 2, 5, 32):
        assert np.array_equal(DR.dtw2(A, B, w, np.float32).astype(np.float64), DR.dtw2(A, B, w))


def test_fp32_restatement_share_of_the_scale():
    """The fp32 restatement's distance from float64 as a share of the case's largest value: what the bar's second term
    multiplies by three (printed per length; the GPU tests print the device's share of the bar)."""
    for L, w in ((24, 3), (48, 5), (187, 19), (512, 64)):
        A, B = DR.gaussian(16, L, 1, 400 + L), DR.gaussian(16, L, 1, 401 + L)
        f64, f32 = DR.dtw2(A, B, w), DR.dtw2(A, B, w, np.float32)
        share = float(np.abs(f32 - f64).max() / f64.max())
        print(f"L {L} w {w}: fp32 restatement off float64 by {share:.2e} of the scale, bar {DR.bar(f64, f32) / f64.max():.2e}")
        assert share <= 1e-5 and DR.bar(f64, f32) >= DR.REL * f64.max()


@pytest.mark.parametrize("case", range(len(DR.SCORE_CASES)))
def test_no_row_of_a_score_case_is_within_reach_of_the_bar(case):
    """The GPU test asks for float64's 1-NN counts exactly.  That is fair only if no row's two nearest distances, to its
    own class and to the other, lie within 2 bars of each other in float64: a condition on the inputs, asserted here."""
    X, Y, w = DR.score_case(case)
    n, m, L, Cn, _ = DR.SCORE_CASES[case]
    assert X.shape == (m, L, Cn) and Y.shape == (n, L, Cn) and X.dtype == Y.dtype == np.float32
    s64, s32 = DR.searches(X, Y, w), DR.searches(X, Y, w, np.float32)
    keys = ("xx", "xy", "yx", "yy")
    bar = DR.bar(np.concatenate([s64[key] for key in keys]), np.concatenate([s32[key] for key in keys]))
    gap = min(float(np.abs(s64["xx"] - s64["xy"]).min()), float(np.abs(s64["yy"] - s64["yx"]).min()))
    print(f"case {case}: bar {bar:.3e}, smallest |d_same - d_other| {gap:.3e} = {gap / bar:.0f} bars")
    assert gap > 2.0 * bar
    assert DR.scores_from_searches(s32)[1] == DR.scores_from_searches(s64)[1]
