"""CPU-side tests of conditional sampling by replacement (no GPU): the new C-ABI symbols are exported and bound
consistently with include/ffd.h, every argument error comes back before any device work, the Python surface
(``SDE.cond_project``, ``DiffusionSampler.sample_conditional`` / ``impute``) checks its arguments and hands the loop its
draws in order, and the numpy restatement the GPU tests judge the kernels by has the properties replacement needs.

The loop's own rejections -- the tag range n_steps (n_corrector + 1) > 0x3FFFFFF0, a bad ``ffd_cond_cfg``, a model length
outside the frequency-domain set -- need a context, and a context needs a device: they are returned before any launch all
the same, and tests/test_cond_gpu.py holds them (test_loop_repeats_splits_..., test_loop_refuses_a_length_...).  Without a
context only the NULL-context rejection can be exercised here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cond_restatement as R
from oracle import cases
from test_pc_host import _Model, _ctype_of, _header_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_cond_project", "ffd_sample_batch_cond")
SDES = {"vp": cases.VP, "ve": cases.VE}


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_like_the_header(lib, name):
    from fastfourierdiffusion_amd import _native

    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, re.M), f"{name} is not exported"
    res, args = _native.SIGNATURES[name]
    ret, params = _header_decl(name)
    assert res is C.c_int and ret == "int" and len(args) == len(params), (name, len(args), params)
    for a, p in zip(args, params):
        want = _ctype_of(p)
        if want == "pointer":
            assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_constants_and_struct_match_the_header():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for key in ("FFD_COND_FREQUENCY", "FFD_COND_TIME"):
        m = re.search(key + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == getattr(N, key), key
    m = re.search(r"typedef struct \{([^}]*)\} ffd_cond_cfg;", header)
    assert m
    fields = [re.sub(r"/\*.*?\*/", "", f).split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == [f[0] for f in N.CondCfg._fields_]
    assert C.sizeof(N.CondCfg) == 3 * 8 + 4 * 4
    assert "ffd_cond_project" in header.split("---- Supported transform lengths ----")[1].split("*/")[0]  # the block is extended


# ---------------------------------------------------------------- argument errors: no device work ----
X_, O_, M_, S_, G_, Z_ = (0x1000 * k for k in range(1, 7))  # dummies, never dereferenced


def _project(lib, sde="default", x=X_, obs=O_, mask=M_, std=None, g=G_, z=Z_, obs_batch=2, domain=0, B=2, L=5, Cn=3,
             noiseless=0, kind=0):
    from fastfourierdiffusion_amd import _native as N

    desc = N.SdeDesc(kind, 0, 0.1, 20.0)
    return lib.ffd_cond_project(C.byref(desc) if sde == "default" else sde, x, obs, mask, std, g, 0.5, noiseless, z, 1, 0,
                                R.TAG0, obs_batch, domain, B, L, Cn, None)


def test_cond_project_refuses_bad_arguments_without_a_device(lib):
    for bad in (dict(sde=None), dict(x=None), dict(obs=None), dict(mask=None), dict(g=None), dict(B=0), dict(L=0), dict(Cn=0),
                dict(B=-1), dict(obs_batch=0), dict(obs_batch=3), dict(obs_batch=1, B=0), dict(domain=2), dict(domain=-1),
                dict(domain=1, std=S_), dict(obs=X_), dict(mask=X_), dict(z=X_),
                dict(z=None, x=None), dict(std=None, obs=None)):  # z and std may be null: the OTHER argument is refused
        assert _project(lib, **bad) == -1, bad
    # FFD_ERR_UNSUPPORTED after the argument checks: a frequency-domain length outside its set, an unknown SDE
    for L in (1, 4097, 5000, 8192):
        assert _project(lib, L=L) == -2, L
        assert _project(lib, L=L, obs=None) == -1, L  # INVALID wins
    assert _project(lib, kind=7) == -2 and _project(lib, kind=7, domain=1) == -2
    assert _project(lib, kind=7, x=None) == -1


def test_sample_batch_cond_refuses_bad_arguments_without_a_context(lib):
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    cfg = N.CondCfg(O_, M_, None, 1, N.FFD_COND_FREQUENCY, 1, 0)
    for cond in (None, C.byref(cfg)):
        assert lib.ffd_sample_batch_cond(None, X_, 1, ts, 3, 0.5, 0, 2, 1, 0.16, N.FFD_LANGEVIN_NORM_BATCH, 0, 0, None, 0, 0,
                                         cond, None) == -1


# ---------------------------------------------------------------- Python surface ----
def test_python_surface_and_argument_checks():
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import SDE, VEScheduler, VPScheduler

    sig = inspect.signature(SDE.cond_project)
    assert list(sig.parameters)[1:5] == ["sample", "observed", "mask", "timestep"]
    kw = {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert kw == dict(std=None, domain="frequency", noise=None, seed=None, sample_offset=0, tag=0xC0000000, noiseless=False)
    assert "cond_project" not in VPScheduler.__dict__ and "cond_project" not in VEScheduler.__dict__
    sig = inspect.signature(DiffusionSampler.sample_conditional)
    assert list(sig.parameters)[1:5] == ["observed", "mask", "num_samples", "num_diffusion_steps"]
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        domain=None, feature_std=None, final_replace=True)
    sig = inspect.signature(DiffusionSampler.impute)
    assert list(sig.parameters)[1:4] == ["series_time", "mask", "num_samples"]
    assert sig.parameters["feature_mean"].default is None and sig.parameters["feature_std"].default is None

    sch = VPScheduler()
    sch.set_noise_scaling(8)
    x = torch.zeros(2, 8, 1)
    with pytest.raises(ValueError):
        sch.cond_project(x, x, x, 0.5, domain="wavelet")
    with pytest.raises(ValueError):
        sch.cond_project(x, x, x, 0.5, domain="time", std=torch.ones(8, 1))

    m = _Model(VPScheduler())  # L = 8, C = 1
    m.device = torch.device("cpu")
    obs, mask = torch.zeros(8, 1), torch.ones(8)
    for solver in ("ode_euler", "ode_heun"):
        with pytest.raises(ValueError):
            DiffusionSampler(m, 4, solver=solver).sample_conditional(obs, mask, 4, 3)
    s = DiffusionSampler(m, 4)
    for bad in (dict(observed=torch.zeros(7, 1)), dict(observed=torch.zeros(8, 2)), dict(observed=torch.zeros(3, 8, 1)),
                dict(mask=torch.ones(7)), dict(mask=torch.ones(8, 2)), dict(mask=torch.ones(4, 8, 1)),
                dict(mask=torch.ones(2, 2, 8, 1)), dict(domain="wavelet"), dict(feature_std=torch.ones(8, 2)),
                dict(domain="time", feature_std=torch.ones(8, 1))):
        args = dict(observed=obs, mask=mask, num_samples=4, num_diffusion_steps=3)
        args.update(bad)
        with pytest.raises(ValueError):
            s.sample_conditional(**args)
    for bad in (dict(series_time=torch.zeros(7, 1)), dict(mask=torch.ones(7)), dict(feature_mean=torch.zeros(8, 1))):
        args = dict(series_time=obs, mask=mask, num_samples=4, num_diffusion_steps=3)
        args.update(bad)
        with pytest.raises(ValueError):
            s.impute(**args)


class _Lib:
    """Stands in for libffd under DiffusionSampler._sample: records the conditional loop calls and what they were handed."""

    def __init__(self, slab):
        self.slab, self.calls = slab, []

    def ffd_sample_batch_cond(self, hdl, x, B, ts, n_steps, h, first, n_run, n_corr, snr, norm, seed, off, z, cache, g0, cond,
                              stream):
        cfg = cond._obj
        zs = None
        if z:
            zs = np.frombuffer(C.string_at(z, 4 * self.slab * n_run * (n_corr + 1) * 2), np.float32)
            zs = zs.reshape(n_run, n_corr + 1, 2, -1)[..., 0].copy()
        mask = np.frombuffer(C.string_at(cfg.mask, 4 * cfg.obs_batch * self.slab // B), np.float32).copy()
        self.calls.append(dict(first=first, n_run=n_run, n_corr=n_corr, B=B, off=off, z=zs, obs_batch=cfg.obs_batch,
                               domain=cfg.domain, final=cfg.final_replace, std=cfg.std, mask=mask))
        return 0

    def __getattr__(self, name):
        return lambda *a: 0


def _stub(monkeypatch, n_steps, num_samples, batch, observed, mask, scale_noise=True, inject=True, call=None, **kw):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    L, Cn = 8, 1
    m = _Model(VPScheduler())
    m.device = torch.device("cpu")
    m.num_training_steps = n_steps
    m.scale_noise = scale_noise
    m.eval = lambda: None
    lib = _Lib(batch * L * Cn)
    m._ctx = lambda: type("Ctx", (), {"lib": lib, "handle": None})()
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    s = DiffusionSampler(m, batch, **kw)
    monkeypatch.setattr(s, "sample_prior", lambda batch_size, _sample_offset=0: torch.zeros(batch_size, L, Cn))
    if inject:
        s.inject_noise(np.full((batch, L, Cn), float(v), np.float32) for v in range(1000))
    s.sample_conditional(observed, mask, num_samples, n_steps, **(call or {}))
    return lib.calls


def test_draw_count_order_and_chunking(monkeypatch):
    """(n_run, n_corrector + 1, 2, B, L, C) draws in consumption order -- per update its own, then its projection's --
    and the steps cut so that the z buffer keeps its size."""
    obs, mask = torch.zeros(8, 1), torch.ones(8)
    calls = _stub(monkeypatch, 5, 2, 2, obs, mask, corrector_steps=1, z_chunk_steps=8)
    assert [(c["first"], c["n_run"], c["n_corr"]) for c in calls] == [(0, 2, 1), (2, 2, 1), (4, 1, 1)]
    drawn = np.concatenate([c["z"].reshape(-1) for c in calls])
    assert np.array_equal(drawn, np.arange(20, dtype=np.float32))  # 5 steps x 2 updates x 2 draws, in order
    assert np.array_equal(calls[1]["z"], np.arange(8, 16, dtype=np.float32).reshape(2, 2, 2))
    calls = _stub(monkeypatch, 3, 2, 2, obs, mask, z_chunk_steps=1)  # no corrector: predictor + projection, one step a call
    assert [(c["first"], c["n_run"], c["n_corr"]) for c in calls] == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    assert np.array_equal(np.concatenate([c["z"].reshape(-1) for c in calls]), np.arange(6, dtype=np.float32))
    calls = _stub(monkeypatch, 3, 2, 2, obs, mask, inject=False, rng="philox", seed=3, sample_offset=7)
    assert len(calls) == 1 and calls[0]["z"] is None and calls[0]["off"] == 7  # device draws: no z buffer, one call


def test_observation_batching_domain_and_mask_broadcast(monkeypatch):
    from fastfourierdiffusion_amd import _native as N

    obs1, mask1 = torch.zeros(8, 1), torch.tensor([1., 1, 1, 0, 0, 0, 0, 0])
    calls = _stub(monkeypatch, 2, 4, 2, obs1, mask1)  # shared: obs_batch 1 in both batches
    assert [(c["B"], c["obs_batch"], c["domain"], c["final"], c["std"]) for c in calls] == [(2, 1, N.FFD_COND_FREQUENCY, 1,
                                                                                            None)] * 2
    assert np.array_equal(calls[0]["mask"], mask1.numpy())
    obs4 = torch.zeros(4, 8, 1)
    mask4 = torch.stack([torch.full((8, 1), float(b)) for b in range(4)])
    calls = _stub(monkeypatch, 2, 4, 2, obs4, mask4, scale_noise=False, call=dict(final_replace=False))
    assert [(c["obs_batch"], c["domain"], c["final"]) for c in calls] == [(2, N.FFD_COND_TIME, 0)] * 2  # per batch slices
    assert [sorted(set(c["mask"].tolist())) for c in calls] == [[0.0, 1.0], [2.0, 3.0]]
    calls = _stub(monkeypatch, 2, 4, 2, obs4, mask1, call=dict(domain="time"))  # (L,) mask broadcast over samples
    assert calls[1]["domain"] == N.FFD_COND_TIME and np.array_equal(calls[1]["mask"], np.tile(mask1.numpy(), 2))
    calls = _stub(monkeypatch, 2, 2, 2, obs1, mask1, call=dict(feature_std=torch.ones(8, 1)))
    assert calls[0]["std"] is not None


# ---------------------------------------------------------------- the restatement ----
def _inputs(shape, seed=0, frac=False):
    rng = np.random.default_rng(seed)
    B, L, Cn = shape
    x, z = rng.standard_normal(shape), rng.standard_normal(shape)
    series = rng.standard_normal(shape)
    mask = (rng.random(shape) < 0.5).astype(np.float64)
    if frac:
        mask = rng.random(shape)
    std = rng.uniform(0.5, 2.0, (L, Cn))
    return x, z, series, mask, std


@pytest.mark.parametrize("shape", [(2, 21, 3), (2, 20, 2), (1, 2, 1), (1, 5, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_restatement_properties(sde, shape):
    kw = SDES[sde]
    B, L, Cn = shape
    G = R.fourier_G(L)
    x, z, series, mask, std = _inputs(shape)
    assert np.allclose(R.idft(R.dft(series)), series, atol=1e-12) and np.allclose(R.dft(R.idft(x)), x, atol=1e-12)
    obs = R.dft(series * mask)
    for sd in (None, std):
        for t in (1.0, 0.5, 1e-5):
            y = R.noised_observation(sde, kw, t, obs, z, G)
            one = R.project(sde, kw, t, x, obs, np.ones(shape), z, G, sd)
            assert np.allclose(one, y, atol=1e-12)  # mask = 1 returns y_t
            assert np.array_equal(R.project(sde, kw, t, x, obs, np.zeros(shape), z, G, sd), x)  # mask = 0 returns x
            # independence of the fill at unobserved points
            a = R.project(sde, kw, t, x, obs, mask, z, G, sd, noiseless=True)
            fill = R.dft(series * mask + 3.0 * (1 - mask) * np.random.default_rng(1).standard_normal(shape))
            if sd is None:
                b = R.project(sde, kw, t, x, fill, mask, z, G, sd, noiseless=True)
                assert np.allclose(a, b, atol=1e-12)
                xt = R.idft(a)
                assert np.allclose(xt[mask == 1], series[mask == 1], atol=1e-12)  # observed points exact
                assert np.allclose(xt[mask == 0], R.idft(x)[mask == 0], atol=1e-12)  # the others untouched
    # time domain
    tm = R.project(sde, kw, 0.5, x, series, mask, z, G, domain="time")
    yt = R.noised_observation(sde, kw, 0.5, series, z, G)
    assert np.allclose(tm, np.where(mask == 1, yt, x), atol=1e-12)
    # fp32 in libffd's order follows float64
    xf, zf, of, mf, sf = (np.float32(a) for a in (x, z, obs, _inputs(shape, frac=True)[3], std))
    a = R.project(sde, kw, 0.5, xf, of, mf, zf, G, sf)
    b = R.project(sde, kw, 0.5, xf, of, mf, zf, G, sf, dtype=np.float32)
    assert b.dtype == np.float32 and R.rel_max_err(b, a) < 1e-6


def test_coefficients_are_the_marginal_of_the_scheduler():
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    for sde, cls in (("vp", VPScheduler), ("ve", VEScheduler)):
        sch = cls(**SDES[sde])
        for t in (1.0, 0.5, 1e-5):
            mc, sg = sch.marginal_coeffs(torch.tensor([t], dtype=torch.float64))
            want = R.coefficients(sde, SDES[sde], t)
            # (the scheduler holds sigma_min / sigma_max as fp32 tensors: up to 2^-24 each, relative)
            assert abs(float(mc) - want[0]) < 1e-12 and abs(float(sg) - want[1]) < 2e-7 * want[1]
        assert R.coefficients(sde, SDES[sde], 0.3, noiseless=True) == (1.0, 0.0)


# mean over the unobserved positions of (sample variance / DATA_STD^2) of the float64 restatement on the analytic case
# (white data, prefix mask, 150 steps, one corrector, snr 0.16, 4096 samples), numpy seeds 0..7, as recorded when the
# operator was specified (min, max), rounded outwards to four digits
RECORDED_BAND = {"ve": (1.0148, 1.0372), "vp": (1.0177, 1.0394)}


@pytest.fixture(scope="module")
def analytic_runs():
    return {sde: [R.gaussian_conditional(sde, kw, seed) for seed in range(8)] for sde, kw in SDES.items()}


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_restatement_analytic_case(analytic_runs, sde):
    """White data: observed and unobserved time points are independent, replacement is exact.  The observed points come
    back exactly (final_replace), the unobserved ones have mean 0 and variance DATA_STD^2 x (1 + the corrector's
    discretisation bias, ~1.025).  All eight recorded seeds are rerun: their min / max IS the recorded band (to its
    outward rounding), which the GPU test widens by its own width."""
    lo, hi = RECORDED_BAND[sde]
    ratios = []
    for seed, (xt, series, mask) in enumerate(analytic_runs[sde]):
        ratio, worst = R.unobserved_stats(xt, mask)
        ratios.append(ratio)
        assert worst < 5.0, (seed, worst)
        assert np.abs(xt[:, :R.GAUSS_PREFIX] - series[:, :R.GAUSS_PREFIX]).max() < 1e-12
    print(f"analytic {sde}: ratio {min(ratios):.4f} .. {max(ratios):.4f}")
    assert lo <= min(ratios) < lo + 2e-4 and hi - 2e-4 < max(ratios) <= hi, ratios


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_restatement_without_the_final_replacement(sde):
    free, series, _ = R.gaussian_conditional(sde, SDES[sde], 0, n=256, final_replace=False)
    assert np.abs(free[:, :R.GAUSS_PREFIX] - series[:, :R.GAUSS_PREFIX]).max() > 1e-6  # y_eps still carries sigma(eps) z
