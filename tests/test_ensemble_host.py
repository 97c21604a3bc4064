"""CPU-side tests of the ensemble scores (no GPU): the C surface and its argument checks, the Python surface
(``ensemble_scores``: shapes, mask inversion, refusal without a device) and the numpy restatement
(tests/ens_restatement.py) against facts it does not share code with -- the pairwise form of the CRPS, np.quantile, the
closed-form CRPS of a Gaussian, and the reason the pair term of the energy score is centred."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import ens_restatement as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_ens_work_bytes", "ffd_ens_pointwise", "ffd_ens_energy")


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


# ------------------------------------------------------------------ the C surface ----
def _header_args(header, name):
    """The parameter list of ``name`` in the header, one C type per parameter."""
    decl = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert decl, name
    params = [" ".join(p.split()) for p in decl.group(2).split(",")]
    return decl.group(1), [p.rsplit(" ", 1)[0].replace(" *", "*") for p in params]


def test_symbols_header_and_argtypes(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "const float*": C.c_void_p, "void*": C.c_void_p,
             "double*": C.c_void_p, "int*": C.c_void_p, "const double*": C.POINTER(C.c_double)}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype[a] for a in args] == list(want_args), (name, args)
    assert len(_header_args(header, "ffd_ens_pointwise")[1]) == 18
    assert len(_header_args(header, "ffd_ens_energy")[1]) == 12


def test_work_bytes_monotone_and_nonzero(lib):
    """At budget 0 (the least a call takes) and at a budget no shape here exhausts (every row and series in one block)."""
    for budget in (0, 1 << 32):
        base = (3, 65, 17)
        b0 = lib.ffd_ens_work_bytes(*base, 3, budget)
        assert b0 > 0
        for axis in range(3):
            prev = 0
            for v in (1, 2, 3, 15, 16, 17, 64, 65, 257, 1024, 1025, 8193):
                shape = list(base)
                shape[axis] = v
                b = lib.ffd_ens_work_bytes(*shape, 3, budget)
                assert b > 0 and b >= prev, (budget, axis, v, b, prev)
                prev = b
    assert lib.ffd_ens_work_bytes(1, 1, 1, 0, 0) > 0
    assert lib.ffd_ens_work_bytes(1 << 20, 1 << 20, 1 << 20, 64, 0) > 0
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 65), (4, 4, 4, -1), ((1 << 20) + 1, 4, 4, 1),
                (4, (1 << 20) + 1, 4, 1), (4, 4, (1 << 20) + 1, 1)):
        assert lib.ffd_ens_work_bytes(*bad, 0) == 0, bad


def test_argument_errors_before_device_work(lib):
    """Every refusal comes before any device work: none of these pointers is a device pointer."""
    buf = np.zeros(1 << 16, np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    S, m, D, nq = 3, 5, 4, 2
    levels = (C.c_double * 64)(*([0.25, 0.75] + [0.5] * 62))
    need = lib.ffd_ens_work_bytes(S, m, D, nq, 0)

    def point(ens=p, truth=p, weight=p, wb=S, S=S, m=m, D=D, lv=levels, nq=nq, fair=0, work=p, nbytes=need):
        return lib.ffd_ens_pointwise(ens, truth, weight, wb, S, m, D, lv, nq, fair, p, p, p, p, p, work, nbytes, None)

    def energy(ens=p, truth=p, weight=p, wb=S, S=S, m=m, D=D, fair=0, out=p, work=p, nbytes=need):
        return lib.ffd_ens_energy(ens, truth, weight, wb, S, m, D, fair, out, work, nbytes, None)

    common = (dict(ens=None), dict(truth=None), dict(work=None), dict(S=0), dict(m=0), dict(D=0), dict(S=-1, wb=-1),
              dict(m=1, fair=1), dict(wb=2), dict(wb=0), dict(nbytes=0), dict(nbytes=8))
    for kw in common:
        assert point(**kw) == INVALID, kw
        assert energy(**kw) == INVALID, kw
    assert energy(out=None) == INVALID
    assert point(nq=65) == INVALID and point(nq=-1) == INVALID and point(lv=None) == INVALID
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        lv = (C.c_double * 2)(0.5, bad)
        assert point(lv=lv) == INVALID, bad
    assert point(S=1, wb=1, nbytes=8 * D + 8 * m - 1) == INVALID  # one byte short of one row's need
    assert energy(S=1, wb=1, nbytes=4 * m * 16) == INVALID         # the centred rows alone: short of one series' need
    big = (1 << 20) + 1
    for kw in (dict(S=big, wb=big), dict(m=big), dict(D=big)):
        assert point(nbytes=1 << 62, **kw) == UNSUPPORTED, kw
        assert energy(nbytes=1 << 62, **kw) == UNSUPPORTED, kw


# ------------------------------------------------------------------ the Python surface ----
class _FakeLib:
    """Stands in for libffd: reads the arrays the binding passes (host memory here) and answers with the restatement."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).reshape(shape)

    def ffd_ens_work_bytes(self, S, m, D, nq, budget):
        return 64

    def _inputs(self, ens, truth, weight, wb, S, m, D):
        X = self._arr(ens, (S, m, D), np.float32)
        y = self._arr(truth, (S, D), np.float32)
        w = self._arr(weight, (wb, D), np.float32) if weight else None
        return X, y, w

    def ffd_ens_pointwise(self, ens, truth, weight, wb, S, m, D, lv, nq, fair, crps, mean, quant, below, equal, work,
                          nbytes, stream):
        X, y, w = self._inputs(ens, truth, weight, wb, S, m, D)
        levels = [lv[i] for i in range(nq)]
        self.calls.append(dict(name="pointwise", X=X.copy(), y=y.copy(), w=None if w is None else w.copy(), wb=wb,
                               levels=levels, fair=fair, nbytes=nbytes))
        self._arr(crps, (S, D), np.float64)[:] = E.crps(X, y, w, fair)
        self._arr(mean, (S,), np.float64)[:] = E.crps_mean(X, y, w, fair)
        if nq:
            self._arr(quant, (nq, S, D), np.float64)[:] = E.quantiles(X, levels, w)
        b, e = E.ranks(X, y, w)
        self._arr(below, (S, D), np.int32)[:] = b
        self._arr(equal, (S, D), np.int32)[:] = e
        return 0

    def ffd_ens_energy(self, ens, truth, weight, wb, S, m, D, fair, out, work, nbytes, stream):
        X, y, w = self._inputs(ens, truth, weight, wb, S, m, D)
        self.calls.append(dict(name="energy", w=None if w is None else w.copy(), wb=wb, fair=fair))
        self._arr(out, (S,), np.float64)[:] = E.energy(X, y, w, fair)
        return 0


@pytest.fixture
def fake(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import forecast

    f = _FakeLib()
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    monkeypatch.setattr(forecast, "_device_of", lambda t: torch.device("cpu"))
    return f


def test_ensemble_scores_shapes_and_mask_inversion(fake):
    from fastfourierdiffusion_amd.sampling import ensemble_scores, forecast

    assert forecast.ensemble_scores is ensemble_scores
    m, L, Cn = 7, 6, 2
    X, y = E.make_case(1, m, L * Cn, seed=3)
    mask = np.zeros(L, np.float32)
    mask[:2] = 1  # a forecast: the first two time points are observed
    out = ensemble_scores(torch.from_numpy(X[0].reshape(m, L, Cn)), y[0].reshape(L, Cn), mask=mask)
    assert list(out) == ["crps", "crps_mean", "quantiles", "below", "equal", "energy_score"]
    assert out["crps"].shape == (1, L, Cn) and out["crps_mean"].shape == (1,) and out["energy_score"].shape == (1,)
    assert out["quantiles"].shape == (3, 1, L, Cn) and out["below"].shape == (1, L, Cn)
    assert out["crps"].dtype == torch.float64 and out["below"].dtype == torch.int32 and out["equal"].dtype == torch.int32
    call = fake.calls[0]
    assert call["levels"] == [0.05, 0.5, 0.95] and call["fair"] == 0 and call["wb"] == 1
    want_w = np.repeat(1.0 - mask, Cn)[None, :]  # the observed mask inverted, broadcast over the channels
    assert np.array_equal(call["w"], want_w) and np.array_equal(fake.calls[1]["w"], want_w)
    assert np.array_equal(call["X"], X) and np.array_equal(call["y"], y)
    assert (out["crps"][0, :2] == 0).all() and (out["crps"][0, 2:] > 0).all()
    assert out["crps_mean"][0] == pytest.approx(float(out["crps"][0, 2:].mean()), rel=1e-14)

    # a batch of series, a per-series (S, L, C) mask, float64 input rounded to fp32, fair, no energy, own levels
    S = 3
    Xb, yb = E.make_case(S, m, L * Cn, seed=4)
    mk = (np.random.default_rng(0).uniform(size=(S, L, Cn)) < 0.5).astype(np.float64)
    fake.calls.clear()
    out = ensemble_scores(Xb.reshape(S, m, L, Cn).astype(np.float64) * (1 + 1e-12), yb.reshape(S, L, Cn), mask=mk,
                          quantiles=(0.0, 1.0), fair=True, energy=False)
    assert "energy_score" not in out and len(fake.calls) == 1
    call = fake.calls[0]
    assert call["wb"] == S and call["fair"] == 1 and call["levels"] == [0.0, 1.0]
    assert np.array_equal(call["w"], 1.0 - mk.reshape(S, L * Cn)) and np.array_equal(call["X"], Xb)
    assert out["quantiles"].shape == (2, S, L, Cn) and out["crps"].shape == (S, L, Cn)
    # no mask: a null weight; (L, 1) and (1, L, C) masks are taken as sample_conditional takes them
    fake.calls.clear()
    ensemble_scores(Xb.reshape(S, m, L, Cn), yb.reshape(S, L, Cn), energy=False)
    assert fake.calls[0]["w"] is None
    ensemble_scores(Xb.reshape(S, m, L, Cn), yb.reshape(S, L, Cn), mask=mask[:, None], energy=False)
    ensemble_scores(Xb.reshape(S, m, L, Cn), yb.reshape(S, L, Cn), mask=np.repeat(mask[None, :, None], Cn, 2), energy=False)
    assert np.array_equal(fake.calls[1]["w"], want_w) and np.array_equal(fake.calls[2]["w"], want_w)

    for bad in (dict(ensemble=Xb[0, 0]), dict(truth=yb.reshape(S, L, Cn)[:2]), dict(mask=np.zeros(L + 1)),
                dict(mask=np.zeros((2, L, Cn))), dict(mask=np.full(L, 0.5)), dict(quantiles=(1.5,)),
                dict(quantiles=tuple([0.5] * 65))):
        kw = dict(ensemble=Xb.reshape(S, m, L, Cn), truth=yb.reshape(S, L, Cn))
        kw.update(bad)
        with pytest.raises(ValueError):
            ensemble_scores(**kw)
    with pytest.raises(ValueError):
        ensemble_scores(Xb.reshape(S, m, L, Cn)[:, :1], yb.reshape(S, L, Cn), fair=True)


def test_ensemble_scores_needs_a_device(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import ensemble_scores

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(N.FFDError, match="no CPU fallback"):
        ensemble_scores(np.zeros((4, 8, 1), np.float32), np.zeros((8, 1), np.float32))


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("m,fair", [(m, f) for m in (1, 2, 7, 64) for f in (False, True) if not (f and m < 2)])
def test_sorted_crps_is_the_pairwise_form(m, fair):
    X, y = E.make_case(2, m, 5, seed=m)
    X[:, : m // 2, 1] = X[:, :1, 1]  # ties between members
    y[:, 2] = X[:, 0, 2]             # and between a member and the truth
    w = np.array([[1, 1, 1, 0, 1]], np.float32)
    a, b = E.crps(X, y, w, fair), E.crps_pairwise(X, y, w, fair)
    scale = np.abs(b).max()
    assert np.abs(a - b).max() <= 1e-12 * scale, (np.abs(a - b).max(), scale)
    assert (a[:, 3] == 0).all()


@pytest.mark.parametrize("fair", [False, True])
def test_energy_is_crps_for_one_coordinate(fair):
    for m in (2, 7, 64):
        X, y = E.make_case(3, m, 1, seed=10 + m)
        a, b = E.energy(X, y, None, fair), E.crps(X, y, None, fair)[:, 0]
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def test_quantiles_are_numpy_quantiles():
    levels = [0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.95, 0.999, 1.0]
    for m in (1, 2, 3, 64, 65, 257):
        X, _ = E.make_case(2, m, 9, seed=m, offset=1.0)
        got = E.quantiles(X, levels)
        want = np.quantile(X.astype(np.float64), levels, axis=1)
        assert np.array_equal(got, want), m


def test_fair_crps_is_unbiased():
    """N(0, 1) ensembles of m = 64 at 4096 independent points, y = 0.3: the mean fair CRPS within 4 standard errors (from
    the 4096 values themselves) of sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)]."""
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((1, 64, 4096))
    y = np.full((1, 4096), 0.3)
    v = E.crps(X, y, None, fair=True)[0]
    z = 0.3
    Phi = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    exact = z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / math.sqrt(math.pi)
    se = v.std(ddof=1) / math.sqrt(v.size)
    print(f"fair CRPS mean {v.mean():.6f}, closed form {exact:.6f}, standard error {se:.2e}")
    assert abs(v.mean() - exact) <= 4.0 * se
    biased = E.crps(X, y, None, fair=False)[0]
    assert biased.mean() - exact > 4.0 * se  # m^2 in place of m (m - 1): too large by E|x - x'| / (2 m)


def test_centring_holds_the_bar_and_the_uncentred_gram_does_not():
    """The reason for the form: a tight ensemble far from the origin (offset 100, spread 1e-2, m = 64, D = 187).  The fp32
    Gram of the rows as they are misses the float64 pair term by far more than the energy bar (n_i is 1.9e6 and fp32
    resolves it to 0.1, d^2 is 0.04); centred on the ensemble mean it holds it."""
    X, y = E.make_case(**E.TIGHT)
    bar, ref, e32 = E.energy_bar(X, y)
    m = X.shape[1]
    exact_pair = E.pair_term(X) / (2.0 * m * m)
    cen = np.abs(E.pair_term(X, None, np.float32, "centred").astype(np.float64) / (2.0 * m * m) - exact_pair)
    unc = np.abs(E.pair_term(X, None, np.float32, "uncentred").astype(np.float64) / (2.0 * m * m) - exact_pair)
    print(f"tight ensemble: bar {bar[0]:.3e}, pair-term error centred {cen[0]:.3e}, uncentred {unc[0]:.3e}, "
          f"energy {ref[0]:.6f}, e32 {e32[0]:.3e}")
    assert unc[0] > bar[0] and unc[0] > 100.0 * bar[0]
    assert cen[0] <= bar[0]
    # in float64 the two forms agree with the definition
    for form in ("centred", "uncentred"):
        assert abs(E.energy(X, y, None, False, np.float64, form)[0] - ref[0]) <= 1e-9
