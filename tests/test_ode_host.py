"""CPU-side tests of the probability-flow ODE solvers (no GPU): the new C-ABI symbols are exported and bound
consistently with include/ffd.h, argument errors come back before any device work, the Python surface (scheduler
``ode_step``, ``DiffusionSampler(solver=...)``) is in place, and the numpy restatement the GPU tests judge the kernels by
converges on the analytic Gaussian case at the recorded float64 rates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ode_restatement as R
from fastfourierdiffusion_amd.sampling.sampler import SOLVERS
from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_ode_step", "ffd_ode_heun_predict", "ffd_ode_heun_correct", "ffd_sample_batch_ode")


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
        if want == "pointer":  # void* / float* / struct pointers: any ctypes pointer type
            assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_solver_constants_match_the_header():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for key in ("FFD_SOLVER_EULER_MARUYAMA", "FFD_SOLVER_ODE_EULER", "FFD_SOLVER_ODE_HEUN"):
        m = re.search(key + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == getattr(N, key), key


def test_context_free_operators_refuse_bad_arguments_without_a_device(lib):
    """Every argument error is FFD_ERR_INVALID (-1), returned before any device work: the pointers below are dummies."""
    from fastfourierdiffusion_amd import _native as N

    desc = N.SdeDesc(N.FFD_SDE_VP, 0, 0.1, 20.0)
    d = C.byref(desc)
    P = 0x1000  # never dereferenced
    X, S, G, XP, D1 = P, 2 * P, 3 * P, 4 * P, 5 * P

    def euler(sde=d, x=X, s=S, g=G, h=0.1, B=2, L=5, Cn=3):
        return lib.ffd_ode_step(sde, x, s, g, 0.5, h, B, L, Cn, None)

    def predict(sde=d, x=X, s=S, g=G, h=0.1, xp=XP, d1=D1, B=2, L=5, Cn=3):
        return lib.ffd_ode_heun_predict(sde, x, s, g, 0.5, h, xp, d1, B, L, Cn, None)

    def correct(sde=d, x=X, xp=XP, s=S, d1=D1, g=G, h=0.1, B=2, L=5, Cn=3):
        return lib.ffd_ode_heun_correct(sde, x, xp, s, d1, g, 0.5, h, B, L, Cn, None)

    for fn in (euler, predict, correct):
        for bad in (dict(sde=None), dict(x=None), dict(s=None), dict(g=None), dict(B=0), dict(L=0), dict(Cn=0), dict(B=-3),
                    dict(h=0.0), dict(h=-0.1), dict(h=float("nan"))):
            assert fn(**bad) == -1, (fn.__name__, bad)
    for bad in (dict(xp=None), dict(d1=None), dict(xp=X), dict(d1=X), dict(xp=XP, d1=XP)):
        assert predict(**bad) == -1, bad
    for bad in (dict(xp=None), dict(d1=None), dict(xp=X), dict(d1=X)):
        assert correct(**bad) == -1, bad
    # the loop entry without a context
    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    assert lib.ffd_sample_batch_ode(None, X, 1, ts, 3, 0.5, 0, 2, N.FFD_SOLVER_ODE_HEUN, 0, 0, None) == -1


def test_python_surface():
    import inspect

    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import SDE, VEScheduler, VPScheduler

    for cls in (VPScheduler, VEScheduler):
        fn = getattr(cls, "ode_step")
        assert list(inspect.signature(fn).parameters)[1:] == ["model_output", "timestep", "sample"]
        assert inspect.signature(fn).return_annotation == SDE.step.__annotations__["return"]  # SamplingOutput
    sig = inspect.signature(DiffusionSampler.__init__)
    assert sig.parameters["solver"].default == "euler_maruyama"

    class _Model:  # the attributes the constructor reads
        noise_scheduler = VPScheduler()
        n_channels, max_len = 1, 8

    assert DiffusionSampler(_Model(), 4).solver == "euler_maruyama"
    for name in ("ode_euler", "ode_heun"):
        assert DiffusionSampler(_Model(), 4, solver=name).solver == name
    for bad in ("heun", "ODE_HEUN", "", None, 1):
        with pytest.raises(ValueError):
            DiffusionSampler(_Model(), 4, solver=bad)


# float64 relative max errors of the restatement on the analytic Gaussian case at N = 17 / 33 / 65 grid points, as
# recorded to three digits when the solvers were specified
RECORDED = {
    ("vp", "ode_heun"): (3.93e-3, 9.31e-4, 2.27e-4),
    ("vp", "ode_euler"): (3.24e-2, 1.61e-2, 8.05e-3),
    ("ve", "ode_heun"): (4.78e-3, 1.10e-3, 2.63e-4),
    ("ve", "ode_euler"): (9.96e-2, 4.77e-2, 2.34e-2),
}
GAUSS_N = (17, 33, 65)


def gaussian_errors(sde, solver, dtype=np.float64):
    kw = cases.VP if sde == "vp" else cases.VE
    G = R.fourier_G(20)
    x0 = R.gaussian_start()
    errs = []
    for N in GAUSS_N:
        ts, h = R.grid(N)
        x = R.integrate(solver, sde, kw, x0, R.gaussian_score(sde, kw, G), ts, h, G, dtype)
        errs.append(R.rel_max_err(x, R.gaussian_exact(sde, kw, x0, 1.0, float(ts[-1]), G)))
    return errs


def test_recorded_cases_cover_the_public_ode_solvers():
    assert {s for _, s in RECORDED} == set(SOLVERS) - {"euler_maruyama"}


@pytest.mark.parametrize("sde,solver", sorted(RECORDED))
def test_restatement_converges_at_the_recorded_rates(sde, solver):
    errs = gaussian_errors(sde, solver)
    for e, rec in zip(errs, RECORDED[(sde, solver)]):
        assert abs(e - rec) <= 5e-3 * rec, (errs, RECORDED[(sde, solver)])  # three recorded digits: half a unit of the last
    lo, hi = (3.5, 5.0) if solver == "ode_heun" else (1.8, 2.2)  # second / first order under step halving
    for a, b in zip(errs, errs[1:]):
        assert lo <= a / b <= hi, errs
    # the fp32 emulation (libffd's operation order) sits on the same curve
    for e32, e64 in zip(gaussian_errors(sde, solver, np.float32), errs):
        assert abs(e32 - e64) <= 0.02 * e64, (e32, e64)
