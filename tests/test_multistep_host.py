"""CPU-side tests of the linear multistep ODE solvers ``ode_ab2`` / ``dpmpp_2m`` (no GPU): the new C-ABI symbols are
exported and bound consistently with include/ffd.h, argument errors come back before any device work, the host
coefficients agree with the float64 restatement, the Python surface (``SDE.ode_multistep_step``,
``DiffusionSampler(solver=...)``) is in place, and the numpy restatement the GPU tests judge the kernels by converges on
the analytic Gaussian case at the recorded float64 rates and is exact on the delta-data case."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import multistep_restatement as M
from fastfourierdiffusion_amd.sampling.sampler import MULTISTEP_SOLVERS
from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_host_multistep_coef", "ffd_ode_multistep_step")
SDES = {"vp": cases.VP, "ve": cases.VE}


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _header_params(name):
    """The parameter declarations of ``name`` in include/ffd.h."""
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared in include/ffd.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return "pointer"
    return {"double": C.c_double, "float": C.c_float, "int": C.c_int}[param.split()[-2]]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_like_the_header(lib, name):
    from fastfourierdiffusion_amd import _native

    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, re.M), f"{name} is not exported"
    res, args = _native.SIGNATURES[name]
    params = _header_params(name)
    assert res is C.c_int and len(args) == len(params), (name, len(args), params)
    for a, p in zip(args, params):
        want = _ctype_of(p)
        if want == "pointer":
            assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_solver_constants_match_the_header():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for key in ("FFD_SOLVER_ODE_AB2", "FFD_SOLVER_DPMPP_2M"):
        m = re.search(key + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == getattr(N, key), key
    assert (N.FFD_SOLVER_ODE_AB2, N.FFD_SOLVER_DPMPP_2M) == (4, 5)


def _desc(sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    return (N.SdeDesc(N.FFD_SDE_VP, 0, kw["beta_min"], kw["beta_max"]) if sde == "vp"
            else N.SdeDesc(N.FFD_SDE_VE, 0, kw["sigma_min"], kw["sigma_max"]))


def test_host_coef_refuses_bad_arguments(lib):
    from fastfourierdiffusion_amd import _native as N

    desc = _desc("vp")
    out = (C.c_double * 5)(*([7.0] * 5))

    def coef(sde=C.byref(desc), solver=N.FFD_SOLVER_DPMPP_2M, tp=0.75, t=0.5, tn=0.25, h=0.25, have=1, o=out):
        return lib.ffd_host_multistep_coef(sde, solver, tp, t, tn, h, have, o)

    assert coef() == 0 and coef(solver=N.FFD_SOLVER_ODE_AB2) == 0
    assert coef(tp=0.1, have=0) == 0  # t_prev is ignored without history
    out[:] = [7.0] * 5
    nan = float("nan")
    for bad in (dict(sde=None), dict(o=None), dict(solver=0), dict(solver=1), dict(solver=2), dict(solver=3), dict(solver=7),
                dict(tn=0.5), dict(tn=0.6), dict(tp=0.5), dict(tp=0.4), dict(t=nan), dict(tn=nan), dict(tp=nan),
                dict(tn=0.0),                                                         # VP: sigma(0) = 0
                dict(solver=N.FFD_SOLVER_ODE_AB2, h=0.0), dict(solver=N.FFD_SOLVER_ODE_AB2, h=-0.25),
                dict(solver=N.FFD_SOLVER_ODE_AB2, h=nan), dict(solver=N.FFD_SOLVER_ODE_AB2, h=float("inf"))):
        assert coef(**bad) == -1, bad
    assert list(out) == [7.0] * 5  # a refused call writes nothing
    assert coef(h=0.0) == 0  # DPM++ reads the grid, not step_size
    bad_sde = N.SdeDesc(5, 0, 0.1, 20.0)
    assert coef(sde=C.byref(bad_sde)) == -1


def test_step_refuses_bad_arguments_without_a_device(lib):
    """Every argument error is FFD_ERR_INVALID (-1), returned before any device work: the pointers below are dummies."""
    P = 0x1000  # never dereferenced
    X, S, G, H = P, 2 * P, 3 * P, 4 * P
    good = (C.c_double * 5)(1.0, 0.5, -0.1, 0.2, 0.0)

    def step(x=X, s=S, g=G, hist=H, coef=good, have=0, B=2, L=5, Cn=3):
        return lib.ffd_ode_multistep_step(x, s, g, hist, coef, have, B, L, Cn, None)

    for bad in (dict(x=None), dict(s=None), dict(g=None), dict(hist=None), dict(coef=None), dict(B=0), dict(L=0), dict(Cn=0),
                dict(B=-3), dict(hist=X), dict(hist=S), dict(hist=X, have=1), dict(hist=S, have=1)):
        assert step(**bad) == -1, bad
    for i in range(5):
        for v in (float("nan"), float("inf"), -float("inf"), 1e300):  # 1e300 is not finite in fp32
            c = (C.c_double * 5)(1.0, 0.5, -0.1, 0.2, 0.3)
            c[i] = v
            assert step(coef=c, have=1) == -1, (i, v)
    assert step(coef=(C.c_double * 5)(1.0, 0.5, -0.1, 0.2, 0.3), have=0) == -1  # no history: coef[4] must be 0


def test_sample_batch_ode_without_a_context(lib):
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    for solver in (N.FFD_SOLVER_ODE_AB2, N.FFD_SOLVER_DPMPP_2M):
        assert lib.ffd_sample_batch_ode(None, 0x1000, 1, ts, 3, 0.5, 0, 2, solver, 0, 0, None) == -1


def interval_cases(N=12):
    """(t_prev, t, t_next) at t = 1 (t_prev: the point a uniform grid would have before it), t = 0.5 and the second-to-last
    point of the N-point grid, and the grid's step size."""
    ts, h = M.grid(N)
    ts = [float(t) for t in ts]
    return [(1.0 + h, 1.0, ts[1]), (0.5 + h, 0.5, 0.5 - h), (ts[-3], ts[-2], ts[-1])], h


@pytest.mark.parametrize("have_prev", [0, 1])
@pytest.mark.parametrize("method", M.METHODS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_host_coef_vs_restatement(lib, sde, method, have_prev):
    from fastfourierdiffusion_amd.schedulers.sde import MULTISTEP_METHODS

    points, h = interval_cases()
    desc = _desc(sde)
    out = (C.c_double * 5)()
    for i, (tp, t, tn) in enumerate(points):
        assert lib.ffd_host_multistep_coef(C.byref(desc), MULTISTEP_METHODS[method], tp, t, tn, h, have_prev, out) == 0
        want = M.coefficients(method, sde, SDES[sde], t, tn, h, tp if have_prev else None)
        for got, w in zip(out, want):
            assert abs(got - w) <= 1e-13 * abs(w), (i, list(out), want)
        if not have_prev:
            assert out[4] == 0.0
        if method == "ode_ab2":  # exactly (a, -cs^2 / 2, 0, -1.5 h, 0.5 h)
            a, cs = M.O.coefficients(sde, SDES[sde], t)
            assert tuple(out) == (a, -0.5 * cs * cs, 0.0, -1.5 * h if have_prev else -h, 0.5 * h if have_prev else 0.0)


def test_dpmpp_coefficients_are_the_exponential_integrator():
    """On a constant data prediction x0 the two-step form reduces to x <- (sigma_n / sigma) x + alpha_n (1 - e^-h) x0:
    cn + cp = c, and cxm1 + qa (cn + cp) = alpha_n / alpha - 1 maps the mean part exactly."""
    points, h = interval_cases()
    for sde, kw in SDES.items():
        for tp, t, tn in points:
            qa, qb, cxm1, cn, cp = M.coefficients("dpmpp_2m", sde, kw, t, tn, h, tp)
            c = M.coefficients("dpmpp_2m", sde, kw, t, tn, h)[3]
            la, ls = M.log_alpha_sigma(sde, kw, t)
            lan, lsn = M.log_alpha_sigma(sde, kw, tn)
            assert abs(cn + cp - c) <= 1e-14 * abs(c) and cp < 0 < cn
            assert abs(qb - math.exp(2 * ls) * qa) <= 1e-14 * qb
            # x = alpha x0 (no noise): the new x is alpha_n x0
            assert abs((1 + cxm1) * math.exp(la) + c - math.exp(lan)) <= 1e-13


class _Model:
    n_channels, max_len = 1, 8
    cache = None

    def __init__(self, sch):
        self.noise_scheduler = sch


def test_python_surface_and_errors():
    from fastfourierdiffusion_amd.sampling import sampler as S
    from fastfourierdiffusion_amd.schedulers.sde import MULTISTEP_METHODS, SDE, VEScheduler, VPScheduler

    for cls in (SDE, VPScheduler, VEScheduler):
        sig = inspect.signature(cls.ode_multistep_step)
        assert list(sig.parameters)[1:] == ["model_output", "timestep", "timestep_next", "sample", "method", "history",
                                            "timestep_prev"]
        assert sig.parameters["history"].default is None and sig.parameters["timestep_prev"].default is None
    assert sorted(S.MULTISTEP_SOLVERS) == sorted(MULTISTEP_METHODS) == ["dpmpp_2m", "ode_ab2"]
    assert sorted(S.SOLVERS) == ["euler_maruyama", "ode_euler", "ode_heun"]  # the recorded Euler / Heun set stays
    assert S.MULTISTEP_SOLVERS == {"ode_ab2": 4, "dpmpp_2m": 5}

    m = _Model(VPScheduler())
    for name in S.MULTISTEP_SOLVERS:
        s = S.DiffusionSampler(m, 4, solver=name)
        assert s.solver == name and s._solver_code() == S.MULTISTEP_SOLVERS[name]
        with pytest.raises(ValueError):
            S.DiffusionSampler(m, 4, solver=name, corrector_steps=1)
        z = torch.zeros(8, 1)
        with pytest.raises(ValueError):
            s.sample_conditional(z, torch.ones(8), 4, 5)
        with pytest.raises(ValueError):
            s.impute(z, torch.ones(8), 4, 5)
        m.num_training_steps = 1
        m.eval = lambda: None
        with pytest.raises(ValueError):
            s.sample(4, 1)  # a one-point grid has no interval
    for bad in ("heun", "ODE_HEUN", "", None, 1, "ab2", "dpmpp", "DPMPP_2M", 4):
        with pytest.raises(ValueError):
            S.DiffusionSampler(m, 4, solver=bad)
    assert S.DiffusionSampler(m, 4).solver == "euler_maruyama"

    sch = VPScheduler()
    sch.set_noise_scaling(8)
    sch.set_timesteps(5)
    x = torch.zeros(2, 8, 1)
    with pytest.raises(ValueError):
        sch.ode_multistep_step(x, 0.5, 0.25, x, "ode_heun")
    with pytest.raises(ValueError):
        sch.ode_multistep_step(x, 0.5, 0.25, x, "ode_ab2", history=x)  # history without its time
    with pytest.raises(ValueError):
        sch.ode_multistep_step(x, 0.5, 0.25, x, "ode_ab2", timestep_prev=0.75)


def test_scheduler_coefficients_need_no_device(lib):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler

    sch = VEScheduler(**cases.VE)
    sch.set_timesteps(12)
    (_, (tp, t, tn), _), h = interval_cases()
    got = sch.multistep_coefficients("dpmpp_2m", t, tn, tp)
    want = M.coefficients("dpmpp_2m", "ve", cases.VE, t, tn, h, tp)
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        sch.multistep_coefficients("dpmpp_2m", 0.25, 0.5)
    with pytest.raises(ValueError):
        sch.multistep_coefficients("heun", 0.5, 0.25)


class _Lib:
    """Stands in for libffd under DiffusionSampler.sample: records the loop calls."""

    def __init__(self):
        self.calls = []

    def ffd_sample_batch_ode(self, hdl, x, B, ts, n_steps, h, first, n_run, solver, cache, g0, stream):
        self.calls.append(("ode", B, n_steps, first, n_run, solver, cache, g0))
        return 0

    def ffd_sample_batch(self, *a):
        self.calls.append(("em",))
        return 0

    def __getattr__(self, name):
        return lambda *a: 0


@pytest.mark.parametrize("name,code", [("ode_ab2", 4), ("dpmpp_2m", 5)])
def test_sample_call_sequence(monkeypatch, name, code):
    """sample() walks the N - 1 intervals of every batch in one ffd_sample_batch_ode call, as the Euler / Heun solvers
    do, draws no step noise and allocates none."""
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    B, L, Cn, n_steps = 2, 8, 1, 7
    m = _Model(VPScheduler())
    m.device = torch.device("cpu")
    m.num_training_steps = n_steps
    m.eval = lambda: None
    lib = _Lib()
    m._ctx = lambda: type("Ctx", (), {"lib": lib, "handle": None})()
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)

    def run(solver):
        lib.calls.clear()
        s = DiffusionSampler(m, B, solver=solver, z_chunk_steps=3)
        monkeypatch.setattr(s, "sample_prior", lambda batch_size, _sample_offset=0: torch.zeros(batch_size, L, Cn))
        s.inject_noise(iter(()))  # any step draw would raise StopIteration
        out = s.sample(2 * B, n_steps)
        assert tuple(out.shape) == (2 * B, L, Cn)
        return list(lib.calls)

    calls = run(name)
    assert calls == [("ode", B, n_steps, 0, n_steps - 1, code, 0, 0)] * 2
    euler = run("ode_euler")
    assert [c[:5] + c[6:] for c in euler] == [c[:5] + c[6:] for c in calls]  # the same chunking as the Euler solver


# float64 relative max errors of the restatement on the analytic Gaussian case (data N(0, 1.5^2), L = 20, Fourier G) at
# N = 17 / 33 / 65 grid points, to three digits
RECORDED = {
    ("vp", "ode_ab2"): (8.92e-3, 2.40e-3, 6.18e-4),
    ("vp", "dpmpp_2m"): (8.82e-2, 2.14e-2, 5.41e-3),
    ("ve", "ode_ab2"): (1.61e-3, 5.08e-4, 1.40e-4),
    ("ve", "dpmpp_2m"): (2.60e-3, 5.53e-4, 1.28e-4),
}
GAUSS_N = (17, 33, 65)


def gaussian_errors(sde, method, dtype=np.float64):
    kw = SDES[sde]
    G = M.fourier_G(20)
    x0 = M.gaussian_start()
    errs = []
    for N in GAUSS_N:
        ts, h = M.grid(N)
        x = M.integrate(method, sde, kw, x0, M.gaussian_score(sde, kw, G), ts, h, G, dtype)
        errs.append(M.rel_max_err(x, M.gaussian_exact(sde, kw, x0, 1.0, float(ts[-1]), G)))
    return errs


def test_recorded_cases_cover_the_public_multistep_solvers():
    assert {s for _, s in RECORDED} == set(MULTISTEP_SOLVERS) == set(M.METHODS)


@pytest.mark.parametrize("sde,method", sorted(RECORDED))
def test_restatement_converges_at_the_recorded_rates(sde, method):
    """Halving ratios of the float64 curve: AB2 VP 3.72 / 3.88, VE 3.18 / 3.63; DPM++ VP 4.12 / 3.96, VE 4.71 / 4.33 (a
    first-order method gives 2).  At 32 evaluations Heun (N = 17) has 3.93e-3 (VP) / 4.78e-3 (VE): AB2 (N = 33) beats it
    on both, DPM++ on VE by a factor of nine, and on VP with this uniform-t grid DPM++ loses to it (2.14e-2)."""
    errs = gaussian_errors(sde, method)
    print(f"gaussian {sde} {method}: float64 {errs}")
    for e, rec in zip(errs, RECORDED[(sde, method)]):
        assert abs(e - rec) <= 5e-3 * rec, (errs, RECORDED[(sde, method)])  # three recorded digits: half a unit of the last
    for a, b in zip(errs, errs[1:]):
        assert 3.0 <= a / b <= 5.5, errs
    # the fp32 emulation (libffd's operation order) sits on the same curve
    for e32, e64 in zip(gaussian_errors(sde, method, np.float32), errs):
        assert abs(e32 - e64) <= 0.02 * e64, (e32, e64)


def test_first_interval_is_the_euler_interval():
    """Without history AB2 is ode_euler's interval (in float64, up to the increment's association)."""
    rng = np.random.default_rng(2)
    G = M.fourier_G(21)
    ts, h = M.grid(12)
    x, s = rng.standard_normal((2, 3, 21, 3))
    for sde, kw in SDES.items():
        got, q = M.step(M.coefficients("ode_ab2", sde, kw, ts[4], ts[5], h), x, s, G)
        assert M.rel_max_err(got, M.O.euler_step(sde, kw, ts[4], x, s, G, h)) < 1e-14
        assert M.rel_max_err(q, M.O.drift(sde, kw, ts[4], x, s, G)) < 1e-14


@pytest.mark.parametrize("N", [2, 3, 7, 17])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_dpmpp_is_exact_on_delta_data(sde, N):
    """Every sample is x0: the score is -(x - alpha x0) / (sigma^2 G^2), the data prediction is x0 at every point of
    every trajectory, and the exponential form lands on alpha(eps) x0 + the scaled noise whatever the grid."""
    kw = SDES[sde]
    G = M.fourier_G(20)
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal((2, 20, 1))
    la, ls = M.log_alpha_sigma(sde, kw, 1.0)
    xs = math.exp(la) * x0 + math.exp(ls) * G[None, :, None].astype(np.float64) * rng.standard_normal((2, 20, 1))
    ts, h = M.grid(N)
    x = M.integrate("dpmpp_2m", sde, kw, xs, M.delta_score(sde, kw, G, x0), ts, h, G)
    assert M.rel_max_err(x, M.delta_exact(sde, kw, xs, 1.0, float(ts[-1]), x0)) < 1e-12
    if N >= 7:  # AB2 has a truncation error here: the property is the exponential form's
        y = M.integrate("ode_ab2", sde, kw, xs, M.delta_score(sde, kw, G, x0), ts, h, G)
        assert M.rel_max_err(y, M.delta_exact(sde, kw, xs, 1.0, float(ts[-1]), x0)) > 1e-6


def test_integrate_splits_with_its_history():
    kw, G = cases.VE, M.fourier_G(20)
    ts, h = M.grid(8)
    x0 = M.gaussian_start()
    fn = M.gaussian_score("ve", kw, G)
    for method in M.METHODS:
        for dtype in (np.float64, np.float32):
            one = M.integrate(method, "ve", kw, x0, fn, ts, h, G, dtype)
            xa, ha = M.integrate_with_history(method, "ve", kw, x0, fn, ts, h, G, dtype, first=0, n_run=3)
            two = M.integrate(method, "ve", kw, xa, fn, ts, h, G, dtype, first=3, hist=ha)
            assert one.dtype == dtype and np.array_equal(one, two)
