"""CPU-side tests of predictor-corrector sampling (no GPU): the new C-ABI symbols are exported and bound consistently with
include/ffd.h, argument errors come back before any device work, the Python surface (``SDE.step_correct``,
``DiffusionSampler(corrector_steps=..., snr=..., corrector_norm=...)``) is in place with its draw order, and the numpy
restatement the GPU tests judge the kernels by is stationary on the analytic Gaussian case where it should be."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pc_restatement as P
from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_langevin_step", "ffd_langevin_work_bytes", "ffd_sample_batch_pc")
SDES = {"vp": cases.VP, "ve": cases.VE}


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _header_decl(name):
    """(return type, parameter declarations) of ``name`` in include/ffd.h."""
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"^(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared in include/ffd.h"
    params = [" ".join(re.sub(r"/\*.*?\*/", "", p).split()) for p in m.group(2).split(",")]
    return m.group(1), params


def _ctype_of(param):
    if "*" in param:
        return "pointer"
    return {"double": C.c_double, "float": C.c_float, "int": C.c_int, "uint64_t": C.c_uint64,
            "uint32_t": C.c_uint32}[param.split()[-2]]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_like_the_header(lib, name):
    from fastfourierdiffusion_amd import _native

    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, re.M), f"{name} is not exported"
    res, args = _native.SIGNATURES[name]
    ret, params = _header_decl(name)
    assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret] and len(args) == len(params), (name, len(args), params)
    for a, p in zip(args, params):
        want = _ctype_of(p)
        if want == "pointer":
            assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_constants_match_the_header():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for key in ("FFD_LANGEVIN_NORM_BATCH", "FFD_LANGEVIN_NORM_SAMPLE", "FFD_SOLVER_PC"):
        m = re.search(key + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == getattr(N, key), key
    assert (N.FFD_LANGEVIN_NORM_BATCH, N.FFD_LANGEVIN_NORM_SAMPLE, N.FFD_SOLVER_PC) == (0, 1, 3)


def test_work_bytes(lib):
    """Row squares (two doubles per row), norms (two doubles per sample), eps and sqrt(2 eps) (two floats per sample)."""
    assert lib.ffd_langevin_work_bytes(3, 21) == 16 * 3 * 21 + 16 * 3 + 8 * 3
    assert lib.ffd_langevin_work_bytes(512, 187) == 16 * 512 * 187 + 24 * 512
    assert lib.ffd_langevin_work_bytes(0, 5) == 0 and lib.ffd_langevin_work_bytes(5, 0) == 0


def test_langevin_step_refuses_bad_arguments_without_a_device(lib):
    """Every argument error is FFD_ERR_INVALID (-1), returned before any device work: the pointers below are dummies."""
    from fastfourierdiffusion_amd import _native as N

    desc = N.SdeDesc(N.FFD_SDE_VP, 0, 0.1, 20.0)
    d = C.byref(desc)
    P_ = 0x1000  # never dereferenced
    X, S, G, W, Z, E = P_, 2 * P_, 3 * P_, 4 * P_, 5 * P_, 6 * P_

    def step(sde=d, x=X, s=S, g=G, h=0.1, snr=0.16, norm=0, z=Z, B=2, L=5, Cn=3, eps=E, work=W):
        return lib.ffd_langevin_step(sde, x, s, g, 0.5, h, snr, norm, z, 1, 0, 0x80000000, B, L, Cn, eps, work, None)

    for bad in (dict(sde=None), dict(x=None), dict(s=None), dict(g=None), dict(work=None), dict(B=0), dict(L=0), dict(Cn=0),
                dict(B=-3), dict(h=0.0), dict(h=-0.1), dict(h=float("nan")), dict(snr=0.0), dict(snr=-0.16),
                dict(snr=float("nan")), dict(norm=2), dict(norm=-1), dict(s=X), dict(work=W + 8)):
        assert step(**bad) == -1, bad
    for bad in (dict(z=None, x=None), dict(eps=None, s=None)):  # z and eps_out may be null: the OTHER argument is refused
        assert step(**bad) == -1, bad


def test_sample_batch_pc_refuses_bad_arguments_without_a_context(lib):
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    assert lib.ffd_sample_batch_pc(None, 0x1000, 1, ts, 3, 0.5, 0, 2, 1, 0.16, N.FFD_LANGEVIN_NORM_BATCH, 0, 0, None, 0, 0,
                                   None) == -1


class _Scheduler:
    """Records what the single-step path asks of the scheduler."""

    def __init__(self):
        self.calls = []
        self.step_size = torch.tensor(0.1)

    def step_correct(self, model_output, sample, snr, timestep, noise=None, norm="batch"):
        from fastfourierdiffusion_amd.schedulers.sde import SamplingOutput

        self.calls.append(("correct", float(model_output[0, 0, 0]), float(noise[0, 0, 0]), snr, timestep, norm))
        return SamplingOutput(prev_sample=sample + 1)

    def step(self, model_output, timestep, sample, noise=None):
        from fastfourierdiffusion_amd.schedulers.sde import SamplingOutput

        self.calls.append(("predict", float(model_output[0, 0, 0]), float(noise[0, 0, 0]), timestep))
        return SamplingOutput(prev_sample=sample + 10)


class _Model:
    """The attributes DiffusionSampler reads; the 'score' is the state it was evaluated at."""
    n_channels, max_len = 1, 8
    cache = None

    def __init__(self, sch):
        self.noise_scheduler = sch
        self.seen = []

    def __call__(self, batch, **kw):
        self.seen.append((float(batch.X[0, 0, 0]), kw))
        return batch.X.clone()


def test_python_surface_defaults_and_errors():
    from fastfourierdiffusion_amd.sampling.sampler import CORRECTOR_NORMS, DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import SDE, VEScheduler, VPScheduler

    for cls in (SDE, VPScheduler, VEScheduler):
        sig = inspect.signature(cls.step_correct)
        assert list(sig.parameters)[1:7] == ["model_output", "sample", "snr", "timestep", "noise", "norm"]  # diffusers' order
        assert sig.parameters["noise"].default is None and sig.parameters["norm"].default == "batch"
    assert "step_correct" not in VPScheduler.__dict__ and "step_correct" not in VEScheduler.__dict__  # the base class's
    sig = inspect.signature(DiffusionSampler.__init__)
    assert sig.parameters["corrector_steps"].default == 0 and sig.parameters["snr"].default == 0.16
    assert sig.parameters["corrector_norm"].default == "batch" and sig.parameters["solver"].default == "euler_maruyama"
    assert sorted(CORRECTOR_NORMS) == ["batch", "sample"]

    m = _Model(VPScheduler())
    s = DiffusionSampler(m, 4)
    assert (s.solver, s.corrector_steps, s.snr, s.corrector_norm) == ("euler_maruyama", 0, 0.16, "batch")
    s = DiffusionSampler(m, 4, corrector_steps=2, snr=0.1, corrector_norm="sample")
    assert (s.corrector_steps, s.snr, s.corrector_norm) == (2, 0.1, "sample")
    for bad in (dict(corrector_steps=-1), dict(snr=0.0), dict(snr=-0.16), dict(snr=float("nan")), dict(corrector_norm="mean"),
                dict(corrector_norm=None), dict(corrector_steps=1, solver="ode_euler"),
                dict(corrector_steps=2, solver="ode_heun")):
        with pytest.raises(ValueError):
            DiffusionSampler(m, 4, **bad)
    DiffusionSampler(m, 4, corrector_steps=0, solver="ode_heun")  # no corrector: the ODE solvers stay available
    sch = VPScheduler()
    sch.set_noise_scaling(8)
    sch.set_timesteps(4)
    x = torch.zeros(2, 8, 1)
    for bad in (dict(norm="mean"), dict(snr=0.0), dict(snr=-1.0)):
        with pytest.raises(ValueError):
            sch.step_correct(x, x, **{"snr": 0.16, "timestep": 0.5, **bad})


def test_single_step_draw_count_and_order():
    """reverse_diffusion_step with n correctors: n + 1 evaluations, each at the state the previous update left, the
    injected draws consumed in order (the correctors', then the predictor's)."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    sch = _Scheduler()
    m = _Model(sch)
    s = DiffusionSampler(m, 2, corrector_steps=2, snr=0.2, corrector_norm="sample")
    s.inject_noise([np.full((2, 8, 1), v, np.float32) for v in (100.0, 200.0, 300.0, 400.0)])
    batch = DiffusableBatch(X=torch.zeros(2, 8, 1), y=None, timesteps=torch.full((2,), 0.5))
    out = s.reverse_diffusion_step(batch)
    assert sch.calls == [("correct", 0.0, 100.0, 0.2, 0.5, "sample"), ("correct", 1.0, 200.0, 0.2, 0.5, "sample"),
                         ("predict", 2.0, 300.0, 0.5)]
    assert [v for v, _ in m.seen] == [0.0, 1.0, 2.0] and float(out[0, 0, 0]) == 12.0
    assert float(next(s._injected)[0, 0, 0]) == 400.0  # exactly three draws were taken


class _Lib:
    """Stands in for libffd under DiffusionSampler.sample: records the loop calls and the z they were handed."""

    def __init__(self, slab):
        self.slab, self.calls = slab, []

    def ffd_sample_batch_pc(self, hdl, x, B, ts, n_steps, h, first, n_run, n_corr, snr, norm, seed, off, z, cache, g0, stream):
        zs = np.frombuffer(C.string_at(z, 4 * self.slab * n_run * (n_corr + 1)), np.float32).reshape(n_run, n_corr + 1, -1)
        self.calls.append(("pc", first, n_run, n_corr, round(snr, 6), norm, zs[:, :, 0].copy()))
        return 0

    def ffd_sample_batch(self, hdl, x, B, ts, n_steps, h, first, n_run, seed, off, z, cache, g0, stream):
        zs = np.frombuffer(C.string_at(z, 4 * self.slab * n_run), np.float32).reshape(n_run, -1)
        self.calls.append(("em", first, n_run, zs[:, 0].copy()))
        return 0

    def __getattr__(self, name):
        return lambda *a: 0


def _stub_sample(monkeypatch, n_steps, **kw):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    B, L, Cn = 2, 8, 1
    m = _Model(VPScheduler())
    m.device = torch.device("cpu")
    m.num_training_steps = n_steps
    m.eval = lambda: None
    lib = _Lib(B * L * Cn)
    m._ctx = lambda: type("Ctx", (), {"lib": lib, "handle": None})()
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    s = DiffusionSampler(m, B, **kw)
    monkeypatch.setattr(s, "sample_prior", lambda batch_size, _sample_offset=0: torch.zeros(batch_size, L, Cn))
    s.inject_noise(np.full((B, L, Cn), float(v), np.float32) for v in range(1000))
    s.sample(B, n_steps)
    return lib.calls


def test_fused_loop_draw_count_order_and_chunking(monkeypatch):
    """sample() hands ffd_sample_batch_pc (n_run, n_corrector + 1, B, L, C) draws in consumption order and cuts the steps
    into chunks of z_chunk_steps // (n_corrector + 1), so that the z buffer keeps its size."""
    calls = _stub_sample(monkeypatch, 7, corrector_steps=2, snr=0.2, corrector_norm="sample", z_chunk_steps=10)
    assert [(c[0], c[1], c[2], c[3], c[4], c[5]) for c in calls] == [("pc", 0, 3, 2, 0.2, 1), ("pc", 3, 3, 2, 0.2, 1),
                                                                    ("pc", 6, 1, 2, 0.2, 1)]
    drawn = np.concatenate([c[6].reshape(-1) for c in calls])
    assert np.array_equal(drawn, np.arange(21, dtype=np.float32))  # 7 steps x 3 draws, in order
    assert np.array_equal(calls[1][6], np.arange(9, 18, dtype=np.float32).reshape(3, 3))
    calls = _stub_sample(monkeypatch, 3, corrector_steps=4, z_chunk_steps=2)  # fewer than one step's draws: one step
    assert [(c[1], c[2]) for c in calls] == [(0, 1), (1, 1), (2, 1)] and calls[0][5] == 0


def test_defaults_leave_the_loop_as_it_was(monkeypatch):
    calls = _stub_sample(monkeypatch, 7, z_chunk_steps=3)
    assert [(c[0], c[1], c[2]) for c in calls] == [("em", 0, 3), ("em", 3, 3), ("em", 6, 1)]
    assert np.array_equal(np.concatenate([c[3] for c in calls]), np.arange(7, dtype=np.float32))


# ---- the restatement on the analytic Gaussian case ----
# mean over positions of (sample variance / exact variance) after 150 corrector steps, "batch" norm, numpy seeds 0..7,
# as recorded when the corrector was specified (min, max), rounded outwards to four digits
RECORDED_BAND = {"ve": (1.0182, 1.0311), "vp": (0.9942, 1.0108)}


@pytest.fixture(scope="module")
def gaussian_runs():
    return {sde: [P.gaussian_stationary_ratio(sde, kw, seed) for seed in range(8)] for sde, kw in SDES.items()}


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_restatement_is_stationary_on_the_gaussian_case(gaussian_runs, sde):
    """Data N(0, 1.5^2), Fourier G, L = 20, C = 1, 4096 samples, 150 steps at t = 0.5 on the 12-point grid, snr 0.16.
    8-seed min / max of the variance ratio: VE 1.0182 .. 1.0311 around 1 / (1 - eps G^2 / 2v) = 1.0239 (eps 0.192);
    VP (alpha 0.086, eps 0.0055) 0.9943 .. 1.0107 around 1.0022.  Wrong variants, 3 seeds: noise sqrt(eps) 0.52 (VE) /
    0.58 (VP); u = G s 0.75 / 0.82; u = s 0.56 / 0.73; noise sqrt(4 eps) 2.02 / 1.62."""
    ratios = [r for r, _ in gaussian_runs[sde]]
    eps = float(np.mean([e for _, e in gaussian_runs[sde]]))
    lo, hi = RECORDED_BAND[sde]
    print(f"gaussian {sde}: ratio {min(ratios):.4f} .. {max(ratios):.4f}, eps {eps:.4g}")
    assert lo <= min(ratios) and max(ratios) <= hi, ratios
    want = P.gaussian_expected_ratio(sde, SDES[sde], eps)
    assert lo <= want <= hi and abs(np.mean(ratios) - want) < 0.5 * (hi - lo), (want, ratios)
    # a wrong noise factor or a missing power of G leaves the band, widened on each side by its own width
    wide = (lo - (hi - lo), hi + (hi - lo))
    for wrong in (dict(_noise_factor=1.0), dict(_noise_factor=4.0), dict(_g_power=1), dict(_g_power=0)):
        r, _ = P.gaussian_stationary_ratio(sde, SDES[sde], 0, **wrong)
        assert not wide[0] <= r <= wide[1], (wrong, r)


def test_sample_norm_inflates_the_variance():
    """The per-sample step size is large exactly for the samples near the mode: at L C = 20 the stationary variance is
    ~1.25 of the exact one (VE), against ~1.02 with the batch mean."""
    r, _ = P.gaussian_stationary_ratio("ve", cases.VE, 0, norm="sample")
    assert 1.20 < r < 1.30, r


def test_restatement_fp32_follows_float64_and_handles_zero_scores():
    rng = np.random.default_rng(5)
    G = P.fourier_G(21)
    _, h = P.grid(12)
    x, s, z = (rng.standard_normal((3, 21, 3)) for _ in range(3))
    s[1] = 0.0
    for sde, kw in SDES.items():
        for norm in P.NORMS:
            a, ea = P.langevin_step(sde, kw, 0.5, x, s, z, G, h, 0.16, norm)
            b, eb = P.langevin_step(sde, kw, 0.5, x, s, z, G, h, 0.16, norm, dtype=np.float32)
            assert b.dtype == np.float32 and P.rel_max_err(b, a) < 1e-6 and np.allclose(ea, eb, rtol=1e-6)
            if norm == "sample":
                assert ea[1] == 0 and np.array_equal(a[1], x[1]) and ea[0] > 0 and ea[2] > 0
            else:
                assert ea[0] == ea[1] == ea[2] > 0
        a, ea = P.langevin_step(sde, kw, 0.5, x, np.zeros_like(s), z, G, h, 0.16, "batch")
        assert np.array_equal(a, x) and not ea.any()
    a, ea = P.langevin_step("vp", cases.VP, 1.0, x, s, z, G, h, 0.16)  # alpha clamps to 0 at t = 1 on this grid
    assert np.array_equal(a, x) and not ea.any() and P.alpha("vp", cases.VP, 1.0, h) == 0.0
    assert abs(P.alpha("vp", cases.VP, 0.5, h) - 0.086) < 1e-3 and P.alpha("ve", cases.VE, 0.5, h) == 1.0
