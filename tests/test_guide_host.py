"""CPU-side tests of guided conditional sampling (no GPU): the new C-ABI symbols are exported and bound consistently with
include/ffd.h, every argument error and refusal comes back before any device work, ``ffd_host_guide_coef`` agrees with
float64, the Python surface refuses what it cannot run, and the restatement the GPU tests judge the kernels by
(tests/guide_restatement.py) has the properties guidance rests on: its gradient is autograd's, the mixture's closed-form
VJP is autograd's and symmetric, scale = 0 is the unguided trajectory, and on a two-mode forecast guidance moves the
posterior mode share towards the exact one where replacement stays at the prior."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cond_restatement as CR
import guide_restatement as GR
import mixture_restatement as M
import ode_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_guide_seed", "ffd_guide_combine", "ffd_host_guide_coef", "ffd_mixture_vjp_work_floats",
               "ffd_mixture_score_vjp", "ffd_train_bind_params", "ffd_train_input_vjp", "ffd_sample_batch_guided")
SDES = {"vp": M.VP, "ve": M.VE}


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _header_decl(name):
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"^(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared in include/ffd.h"
    return m.group(1), [" ".join(re.sub(r"/\*.*?\*/", "", p).split()) for p in m.group(2).split(",")]


def _ctype_of(param):
    if "*" in param or "[" in param:
        return "pointer"
    return {"double": C.c_double, "float": C.c_float, "int": C.c_int, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "size_t": C.c_size_t}[param.split()[-2]]


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
            assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_guide_cfg_layout_and_documents():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} ffd_guide_cfg;", header)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl).strip()
        if decl:
            fields += [f.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in N.GuideCfg._fields_] == ["scale", "obs_var", "rho", "replace", "reserved"]
    assert C.sizeof(N.GuideCfg) == 3 * 8 + 2 * 4
    assert [getattr(N.GuideCfg, f).offset for f in fields] == [0, 8, 16, 24, 28]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in integration, f"{name} is missing from INTEGRATION.md"
    make = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "Makefile")).read()
    assert "ffd_guide.hip" in make


# ---------------------------------------------------------------- argument errors: no device work ----
P_ = 0x1000  # dummies, never dereferenced
X_, S_, O_, M_, D_, G_, U_, V_, H_, W_ = (P_ * k for k in range(1, 11))


def _desc(kind=0):
    from fastfourierdiffusion_amd import _native as N

    return N.SdeDesc(kind, 0, 0.1, 20.0)


def _seed(lib, sde="default", x=X_, s=S_, obs=O_, mask=M_, std=None, g=G_, t=0.5, obs_batch=2, domain=0, B=2, L=5, Cn=3,
          u=U_, v=V_, loss=None, x0=None, kind=0):
    desc = _desc(kind)
    return lib.ffd_guide_seed(C.byref(desc) if sde == "default" else sde, x, s, obs, mask, std, g, t, obs_batch, domain, B, L,
                              Cn, u, v, loss, x0, None)


def test_guide_seed_refuses_bad_arguments_without_a_device(lib):
    for bad in (dict(sde=None), dict(x=None), dict(s=None), dict(obs=None), dict(mask=None), dict(g=None), dict(u=None),
                dict(v=None), dict(B=0), dict(L=0), dict(Cn=0), dict(B=-1), dict(obs_batch=0), dict(obs_batch=3),
                dict(domain=2), dict(domain=-1), dict(domain=1, std=D_), dict(t=float("nan")), dict(t=float("inf")),
                dict(t=-0.1), dict(u=X_), dict(v=S_), dict(u=O_), dict(v=M_), dict(u=G_), dict(v=U_), dict(x0=X_),
                dict(x0=U_), dict(x0=V_), dict(std=D_, u=D_),
                dict(loss=None, x=None), dict(x0=None, s=None), dict(std=None, obs=None)):  # the optional ones may be null
        assert _seed(lib, **bad) == -1, bad
    for L in (1, 4097, 5000, 8192):  # FFD_ERR_UNSUPPORTED after the argument checks, as ffd_cond_project
        assert _seed(lib, L=L) == -2, L
        assert _seed(lib, L=L, obs=None) == -1, L
    assert _seed(lib, kind=7) == -2 and _seed(lib, kind=7, domain=1) == -2 and _seed(lib, kind=7, x=None) == -1


def test_guide_combine_refuses_bad_arguments_without_a_device(lib):
    def combine(s=S_, u=U_, j=V_, alpha=0.9, coef=2.0, out=S_, n=16):
        return lib.ffd_guide_combine(s, u, j, alpha, coef, out, n, None)

    for bad in (dict(s=None), dict(u=None), dict(j=None), dict(out=None), dict(n=0), dict(alpha=0.0), dict(alpha=float("nan")),
                dict(alpha=float("inf")), dict(coef=float("nan")), dict(coef=float("inf"))):
        assert combine(**bad) == -1, bad


def test_mixture_vjp_refuses_bad_arguments_without_a_device(lib):
    def vjp(sde="default", x=X_, t=S_, ts=0, mu=O_, lw=M_, var=None, g=G_, v=V_, out=U_, B=2, K=3, L=5, Cn=3, work=W_,
            floats=None, kind=0):
        desc = _desc(kind)
        floats = lib.ffd_mixture_vjp_work_floats(B, K, L, Cn) if floats is None else floats
        return lib.ffd_mixture_score_vjp(C.byref(desc) if sde == "default" else sde, x, t, ts, mu, lw, var, g, v, out, B, K, L, Cn,
                                         work, floats, None)

    for bad in (dict(sde=None), dict(x=None), dict(t=None), dict(mu=None), dict(lw=None), dict(g=None), dict(v=None),
                dict(out=None), dict(work=None), dict(B=0), dict(K=0), dict(L=0), dict(Cn=0), dict(ts=2), dict(ts=-1),
                dict(floats=1)):
        assert vjp(**bad) == -1, bad
    assert vjp(kind=7) == -2 and vjp(L=1025, Cn=1) == -2 and vjp(L=513, Cn=2) == -2
    # the work query: slices of 512 components, per (slice, row) the maximum, two sums and two weighted sums
    assert lib.ffd_mixture_vjp_work_floats(2, 3, 5, 3) == 2 * (2 * 15 + 3)
    assert lib.ffd_mixture_vjp_work_floats(7, 513, 8, 1) == 2 * 7 * (2 * 8 + 3)
    assert lib.ffd_mixture_vjp_work_floats(2, 3, 1025, 1) == 0 and lib.ffd_mixture_vjp_work_floats(0, 3, 5, 3) == 0
    assert lib.ffd_mixture_vjp_work_floats(2, 3, 5, 3) > lib.ffd_mixture_work_floats(2, 3, 5, 3)


def _train(lib, kind, bind="params"):
    """A training object (without a device its creation fails after the tensors are listed: binding still works)."""
    from fastfourierdiffusion_amd import _native as N

    desc = N.ModelDesc(kind, 1, 12, 24, 4 if kind == N.FFD_MODEL_TRANSFORMER else 1, 2, 64, 0, 0.1, 20.0, 1, 1e-5)
    h = C.c_void_p()
    assert lib.ffd_train_create(C.byref(h), C.byref(desc), 0.0, 0) == (0 if torch.cuda.is_available() else -4)
    d, io, F = 24, 12, 64
    sizes = {"time_encoder.W": 12, "time_encoder.dense.weight": d * d, "time_encoder.dense.bias": d}
    if kind == N.FFD_MODEL_MLP:
        sizes.update({"embedder.weight": d * io, "embedder.bias": d, "unembedder.weight": io * d, "unembedder.bias": io})
        for i in range(2):
            sizes.update({f"backbone.{i}.0.weight": F * d, f"backbone.{i}.0.bias": F, f"backbone.{i}.3.weight": d * F,
                          f"backbone.{i}.3.bias": d})
    else:
        sizes.update({"pos_encoder.embedding.weight": 12 * d, "embedder.weight": d, "embedder.bias": d, "unembedder.weight": d,
                      "unembedder.bias": 1})
        for i in range(2):
            p = f"backbone.layers.{i}."
            sizes.update({p + "self_attn.in_proj_weight": 3 * d * d, p + "self_attn.in_proj_bias": 3 * d,
                          p + "self_attn.out_proj.weight": d * d, p + "self_attn.out_proj.bias": d, p + "linear1.weight": F * d,
                          p + "linear1.bias": F, p + "linear2.weight": d * F, p + "linear2.bias": d, p + "norm1.weight": d,
                          p + "norm1.bias": d, p + "norm2.weight": d, p + "norm2.bias": d})
    for name, n in sizes.items():
        if bind == "params":
            assert lib.ffd_train_bind_params(h, name.encode(), P_, n) == 0, name
        elif bind == "full":
            assert lib.ffd_train_bind(h, name.encode(), P_, 2 * P_, 3 * P_, 4 * P_, n) == 0, name
    return h, sizes


@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_parameter_only_binding_refuses_training_without_a_device(lib, kind):
    from fastfourierdiffusion_amd import _native as N

    k = N.FFD_MODEL_MLP if kind == "mlp" else N.FFD_MODEL_TRANSFORMER
    h, sizes = _train(lib, k, bind=None)
    try:
        assert lib.ffd_train_bind_params(None, b"embedder.bias", P_, 24) == -1
        assert lib.ffd_train_bind_params(h, None, P_, 24) == -1 and lib.ffd_train_bind_params(h, b"embedder.bias", None, 24) == -1
        assert lib.ffd_train_bind_params(h, b"no.such.tensor", P_, 24) == -1
        assert lib.ffd_train_bind_params(h, b"embedder.bias", P_, 23) == -1
        # nothing bound yet: the VJP needs its tensors (FFD_ERR_STATE), then a forward
        assert lib.ffd_train_input_vjp(h, X_, S_, 2, None) == -3 and b"not bound" in lib.ffd_train_last_error(h)
    finally:
        lib.ffd_train_destroy(h)
    h, sizes = _train(lib, k, bind="params")
    try:
        cfg = N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1)
        batch = (X_, None, S_, O_, M_, None, 0, 0, 0, D_, 2)
        assert lib.ffd_train_loss_grad(h, *batch, None) == -3
        assert b"ffd_train_bind_params" in lib.ffd_train_last_error(h)
        assert lib.ffd_train_step(h, *batch, C.byref(cfg), None) == -3
        assert lib.ffd_train_adamw(h, D_, C.byref(cfg), None) == -3
        assert lib.ffd_train_grad_sqnorm(h, D_, None) == -3
        # the argument errors still come first
        assert lib.ffd_train_loss_grad(h, None, None, S_, O_, M_, None, 0, 0, 0, D_, 2, None) == -1
        # no forward has run: the VJP has no activations to go through
        assert lib.ffd_train_input_vjp(h, X_, S_, 2, None) == -3 and b"no forward" in lib.ffd_train_last_error(h)
        for bad in ((None, S_, 2), (X_, None, 2), (X_, X_, 2), (X_, S_, 0)):
            assert lib.ffd_train_input_vjp(h, *bad, None) == -1, bad
        assert lib.ffd_train_input_vjp(None, X_, S_, 2, None) == -1
        # binding one tensor fully does not make the object trainable; binding all of them does (its contract is kept)
        name, n = "embedder.bias", sizes["embedder.bias"]
        assert lib.ffd_train_bind(h, name.encode(), P_, 2 * P_, 3 * P_, 4 * P_, n) == 0
        assert lib.ffd_train_grad_sqnorm(h, D_, None) == -3
        assert lib.ffd_train_bind(h, name.encode(), P_, None, 3 * P_, 4 * P_, n) == -1  # ffd_train_bind's own refusal
    finally:
        lib.ffd_train_destroy(h)


def test_sample_batch_guided_refuses_a_null_context(lib):
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    cond = N.CondCfg(O_, M_, None, 1, N.FFD_COND_TIME, 1, 0)
    guide = N.GuideCfg(1.0, 1e-2, 1.0, 0, 0)
    assert lib.ffd_sample_batch_guided(None, None, X_, 1, ts, 3, 0.5, 0, 2, 0, 0, None, C.byref(cond), C.byref(guide), None,
                                       None) == -1


# ---------------------------------------------------------------- the host coefficient ----
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_host_guide_coef_against_float64(lib, sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    a, b = (kw["beta_min"], kw["beta_max"]) if sde == "vp" else (kw["sigma_min"], kw["sigma_max"])
    desc = N.SdeDesc(N.FFD_SDE_VP if sde == "vp" else N.FFD_SDE_VE, 0, a, b)
    out = (C.c_double * 3)()
    for t in (1.0, 0.5, 0.05, 1e-3, 1e-5, float(np.float32(0.3))):
        for scale, obs_var, rho in ((1.0, 1e-2, 1.0), (0.5, 0.25, 0.0), (2.0, 0.0, 3.0), (0.0, 1.0, 1.0)):
            assert lib.ffd_host_guide_coef(C.byref(desc), t, scale, obs_var, rho, out) == 0
            want = GR.coefficients(sde, kw, t, scale, obs_var, rho)
            np.testing.assert_allclose(list(out), want, rtol=1e-14, atol=0)
            mc, sigma = CR.coefficients(sde, kw, t)  # the (alpha, sigma) of ffd_cond_project
            assert math.isclose(out[0], mc, rel_tol=1e-15) and math.isclose(out[1], sigma * sigma, rel_tol=1e-14)
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 1, 1, 1), (inf, 1, 1, 1), (-0.1, 1, 1, 1), (0.5, nan, 1, 1), (0.5, -1, 1, 1), (0.5, inf, 1, 1),
                (0.5, 1, nan, 1), (0.5, 1, -1e-3, 1), (0.5, 1, 1, nan), (0.5, 1, 1, -1), (0.5, 1, 1, inf),
                (0.5, 1, 0, 0)):  # the last: a zero denominator
        assert lib.ffd_host_guide_coef(C.byref(desc), *bad, out) == -1, bad
    assert lib.ffd_host_guide_coef(None, 0.5, 1, 1, 1, out) == -1 and lib.ffd_host_guide_coef(C.byref(desc), 0.5, 1, 1, 1, None) == -1
    if sde == "ve":  # at t = 0 a VP marginal has sigma = 0: obs_var = 0 leaves no denominator
        vp = N.SdeDesc(N.FFD_SDE_VP, 0, 0.1, 20.0)
        assert lib.ffd_host_guide_coef(C.byref(vp), 0.0, 1, 0, 1, out) == -1
    unknown = N.SdeDesc(7, 0, a, b)
    assert lib.ffd_host_guide_coef(C.byref(unknown), 0.5, 1, 1, 1, out) == -2
    assert lib.ffd_host_guide_coef(C.byref(unknown), nan, 1, 1, 1, out) == -1


# ---------------------------------------------------------------- the Python surface ----
class _Model:
    """The attributes DiffusionSampler reads before any device work."""
    n_channels, max_len, cache = 1, 8, None
    device = torch.device("cpu")

    def __init__(self, sch, kind):
        self.noise_scheduler, self._kind = sch, kind

    def enable_caching(self, **kw):
        self.cache = object()


def test_python_surface_and_refusals():
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    g = Guidance()
    assert (g.scale, g.obs_var, g.rho, g.replace) == (1.0, 1e-2, 1.0, False)
    for bad in (dict(scale=-1.0), dict(scale=float("nan")), dict(obs_var=-1e-3), dict(rho=float("inf")), dict(rho="1"),
                dict(scale=True), dict(obs_var=0.0, rho=0.0)):
        with pytest.raises(ValueError):
            Guidance(**bad)
    assert "overshoot" in Guidance.__doc__  # the docstring says what too small an obs_var does

    obs, mask = torch.zeros(8, 1), torch.ones(8)
    model = lambda kind: _Model(VPScheduler(), kind)  # noqa: E731
    refused = [
        (DiffusionSampler(model(N.FFD_MODEL_LSTM), 4), {}),
        (DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4, corrector_steps=1), {}),
        (DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4, solver="ode_heun"), {}),
        (DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4, solver="dpmpp_2m"), {}),
        (DiffusionSampler(model(N.FFD_MODEL_TRANSFORMER), 4, use_cache=True), {}),
        (DiffusionSampler(model(N.FFD_MODEL_MLP), 4, use_fresca=True), {}),
        (DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4), dict(resample=2, jump=2)),
    ]
    for s, kw in refused:
        with pytest.raises(NotImplementedError):
            s.sample_conditional(obs, mask, 4, 3, guidance=g, **kw)
        with pytest.raises(NotImplementedError):
            s.impute(obs, mask, 4, 3, guidance=g, **kw)
    s = DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4)
    with pytest.raises(TypeError):
        s.sample_conditional(obs, mask, 4, 3, guidance=dict(scale=1.0))
    with pytest.raises(TypeError):
        s.sample_conditional(obs, mask, 4, 3, guide=g)  # guidance is the one extension keyword
    with pytest.raises(ValueError):  # None: today's path and today's refusals
        DiffusionSampler(model(N.FFD_MODEL_MIXTURE), 4, solver="ode_heun").sample_conditional(obs, mask, 4, 3, guidance=None)

    # SDE.denoise: Tweedie's estimate with the coefficients of the guidance kernels
    for sch, sde in ((VPScheduler(fourier_noise_scaling=True), "vp"), (VEScheduler(fourier_noise_scaling=True), "ve")):
        sch.set_noise_scaling(8)
        x, sc = torch.randn(3, 8, 2, dtype=torch.float64), torch.randn(3, 8, 2, dtype=torch.float64)
        alpha, s2, lam = sch.guide_coeffs(0.3, 2.0, 0.04, 1.0)
        assert (alpha, s2, lam) == pytest.approx(GR.coefficients(sde, SDES[sde], 0.3, 2.0, 0.04, 1.0), rel=1e-14)
        want = (x + s2 * (sch.G.double() ** 2)[None, :, None] * sc) / alpha
        assert torch.allclose(sch.denoise(sc, 0.3, x), want, rtol=1e-12, atol=0)
        with pytest.raises(ValueError):
            sch.denoise(sc[:, :4], 0.3, x)


class _Lib:
    """Stands in for libffd under DiffusionSampler._sample: records the guided loop calls."""

    def __init__(self, slab):
        self.slab, self.calls = slab, []

    def ffd_sample_batch_guided(self, hdl, net, x, B, ts, n_steps, h, first, n_run, seed, off, z, cond, guide, loss, stream):
        zs = None
        if z:
            zs = np.frombuffer(C.string_at(z, 4 * self.slab * n_run * 2), np.float32).reshape(n_run, 2, -1)[..., 0].copy()
        c, g = cond._obj, guide._obj
        self.calls.append(dict(net=net, B=B, first=first, n_run=n_run, off=off, z=zs, obs_batch=c.obs_batch, domain=c.domain,
                               final=c.final_replace, guide=(g.scale, g.obs_var, g.rho, g.replace)))
        return 0

    def ffd_sample_batch_cond(self, *a):
        raise AssertionError("the guided path must not take the replacement entry")

    def __getattr__(self, name):
        return lambda *a: 0


def test_sampler_hands_the_guided_loop_its_draws_in_order(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    L, Cn, batch, steps = 8, 1, 4, 5
    m = _Model(VPScheduler(), N.FFD_MODEL_MIXTURE)
    m.num_training_steps, m.scale_noise, m.eval = steps, False, lambda: None
    lib = _Lib(batch * L * Cn)
    m._ctx = lambda: type("Ctx", (), {"lib": lib, "handle": None})()
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    s = DiffusionSampler(m, batch, z_chunk_steps=4)
    monkeypatch.setattr(s, "sample_prior", lambda batch_size, _sample_offset=0: torch.zeros(batch_size, L, Cn))
    s.inject_noise(np.full((batch, L, Cn), float(v), np.float32) for v in range(1000))
    s.sample_conditional(torch.zeros(L, Cn), torch.ones(L), 2 * batch, steps, guidance=Guidance(0.5, 0.04, 2.0, True),
                         final_replace=False)
    calls = lib.calls
    assert [c["net"] for c in calls] == [None] * len(calls)  # the mixture needs no network object
    assert all(c["guide"] == (0.5, 0.04, 2.0, 1) and c["domain"] == N.FFD_COND_TIME and c["final"] == 0 for c in calls)
    for b in range(2):  # per batch: chunks of two steps (four draws), the predictor's draw then the projection's
        mine = [c for c in calls if c["off"] == b * batch]
        assert [(c["first"], c["n_run"]) for c in mine] == [(0, 2), (2, 2), (4, 1)]
        z = np.concatenate([c["z"] for c in mine]).reshape(-1)
        assert z.tolist() == [float(v) for v in range(b * 2 * steps, (b + 1) * 2 * steps)]


# ---------------------------------------------------------------- the restatement ----
@pytest.mark.parametrize("L", [7, 8, 12, 187])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_restated_gradient_is_autograds(sde, L):
    """u = d loss / d x0hat at odd and even L, both domains, with and without std; and without W the frequency-domain
    gradient is wrong by O(1)."""
    rng = np.random.default_rng(L)
    B, Cn, t, kw = 3, 2, 0.3, SDES[sde]
    G = M.fourier_G(L)
    for domain, use_std in (("frequency", False), ("frequency", True), ("time", False)):
        x, s, obs = (rng.standard_normal((B, L, Cn)) for _ in range(3))
        mask = (rng.random((B, L, Cn)) < 0.5).astype(np.float64)
        std = rng.uniform(0.5, 2.0, (L, Cn)) if use_std else None
        u, v, loss, x0 = GR.seed(sde, kw, t, x, s, obs, mask, G, std, domain)
        alpha, s2, _ = GR.coefficients(sde, kw, t)
        c = s2 * (G.astype(np.float64) ** 2)[None, :, None]
        np.testing.assert_allclose(x0, (x + c * s) / alpha, rtol=1e-14)
        np.testing.assert_allclose(v, c * u, rtol=1e-14)
        xh = torch.tensor(x0, requires_grad=True)
        lt = GR.loss_torch(sde, kw, t, xh, obs, mask, std, domain)
        grad = torch.autograd.grad(lt.sum(), xh)[0].numpy()
        np.testing.assert_allclose(loss, lt.detach().numpy(), rtol=1e-12)
        assert np.abs(u - grad).max() <= 1e-12 * np.abs(grad).max()
        if domain == "frequency":
            plain = u / GR.adjoint_weights(L)[None, :, None]  # dft alone, without the layout's weights
            assert np.abs(plain - grad).max() > 0.1 * np.abs(grad).max()
    # a zero mask: exact zeros
    u, v, loss, _ = GR.seed(sde, kw, t, x, s, obs, np.zeros_like(mask), G, None, "frequency", np.float32)
    assert not u.any() and not v.any() and not loss.any()


@pytest.mark.parametrize("shape", [(4, 8, 1, 3), (5, 20, 3, 17), (2, 7, 2, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_mixture_vjp_formula_is_autograds_and_symmetric(sde, shape):
    kw = SDES[sde]
    rng = np.random.default_rng(sum(shape))
    for t in (1.0, 0.5, 1e-3):
        for v_mode in (0, 1):
            x, mu, lw, var, G = M.make_case(shape, sde, t, v_mode)
            v, w = rng.standard_normal(x.shape), rng.standard_normal(x.shape)
            jv = GR.mixture_vjp(sde, kw, x, t, mu, lw, var, G, v)
            ref = GR.mixture_vjp_autograd(sde, kw, x, t, mu, lw, var, G, v)
            assert np.abs(jv - ref).max() <= 1e-11 * np.abs(ref).max(), (t, v_mode)
            # the fp32 evaluation in the kernel's order (the GPU tests' bar): the same quantity, and with one component
            # the two products of the covariance round alike -- J^T v = -v / c to the last bit
            ordered = GR.mixture_vjp_ordered(sde, kw, x, t, mu, lw, var, G, v)
            assert np.abs(ordered - ref).max() <= 2e-3 * np.abs(ref).max(), (t, v_mode)
            if shape[3] == 1:
                c32 = M._coeffs(sde, kw, t, x.shape[0], var, G, x.shape[1], x.shape[2], np.float32)[1]
                assert np.array_equal(ordered, -(v.astype(np.float32) * (np.float32(1.0) / c32)))
            jw = GR.mixture_vjp(sde, kw, x, t, mu, lw, var, G, w)
            a, b = (jv * w).reshape(x.shape[0], -1).sum(-1), (v * jw).reshape(x.shape[0], -1).sum(-1)  # <Jv, w> = <v, Jw>
            assert np.abs(a - b).max() <= 1e-10 * max(np.abs(a).max(), np.abs(b).max()), (t, v_mode)


@pytest.mark.parametrize("case", GR.VJP_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_vjp_cases_stay_clear_of_the_relu_kink(sde, case):
    """The chosen seeds satisfy the no-kink rule for every network case of test_guide_gpu.py; and on the CPU the fp32
    autograd VJP of the same forward sits within 1e-5 of the float64 one (the device's bar is 3 x this error)."""
    model, sd, xn, t, v = GR.vjp_case_setup(case, sde)
    GR.vjp_assert_no_kink(case, sd, xn, t, model.noise_scheduler.G.numpy(), case["name"])
    s64, g64 = GR.network_vjp(GR.network_forward(case, sd, t), xn, v)
    s32, g32 = GR.network_vjp(GR.network_forward(case, sd, t, torch.float32), xn, v, torch.float32)
    assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max() and np.abs(s32 - s64).max() <= 1e-5 * np.abs(s64).max()


def _two_mode(sde, seed, n=512, steps=100):
    kw = SDES[sde]
    mu, lw, var = GR.two_mode_mixture()
    obs, mask = GR.two_mode_observation()
    G = np.ones(GR.TWO_L, np.float32)
    ts, h = R.grid(steps)
    rng = np.random.default_rng(seed)
    x0 = (kw["sigma_max"] if sde == "ve" else 1.0) * rng.standard_normal((n, GR.TWO_L, 1))
    zs = rng.standard_normal((steps, 2, n, GR.TWO_L, 1))
    replaced = CR.cond_integrate(sde, kw, x0, M.score_fn(sde, kw, mu, lw, var, G), lambda i, k, p: zs[i, p], ts, h, G, 0, 0.16,
                                 obs, mask, None, "time", True)
    guide = dict(scale=1.0, obs_var=GR.TWO_BW ** 2, rho=1.0)
    guided, losses = GR.guided_integrate(sde, kw, x0, GR.mixture_score_vjp_fn(sde, kw, mu, lw, var, G), lambda i, p: zs[i, p],
                                         ts, h, G, obs, mask, guide, None, "time", False, True)
    return GR.two_mode_share(replaced), GR.two_mode_share(guided), losses


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_two_mode_forecast_guidance_moves_the_mode_share_towards_the_exact_one(sde):
    exact = GR.two_mode_exact_share()
    assert 0.95 < exact < 0.98
    replaced, guided, losses = _two_mode(sde, seed=0)
    print(f"two-mode forecast {sde}: exact {exact:.3f} replacement {replaced:.3f} guided {guided:.3f}")
    assert abs(guided - exact) < abs(replaced - exact)
    assert guided - replaced > 3 * 0.022  # ... by more than the share's sampling error (512 samples: 0.022)
    assert losses.shape == (100, 512) and np.isfinite(losses).all()


@pytest.mark.parametrize("domain", CR.DOMAINS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_scale_zero_is_the_unguided_trajectory(sde, domain):
    kw = SDES[sde]
    shape, steps = (3, 12, 2, 5), 6
    x, mu, lw, var, G = M.make_case(shape, sde, 1.0, 1, fourier=domain == "frequency")
    rng = np.random.default_rng(5)
    obs, mask = rng.standard_normal((1, 12, 2)), (rng.random((1, 12, 2)) < 0.5).astype(np.float64)
    zs = rng.standard_normal((steps, 2) + x.shape)
    ts, h = R.grid(steps)
    fn = GR.mixture_score_vjp_fn(sde, kw, mu, lw, var, G)
    guide = dict(scale=0.0, obs_var=0.04, rho=1.0)
    for dtype in (np.float64, np.float32):
        sf = M.score_fn(sde, kw, mu, lw, var, G, dtype)
        for final in (True, False):
            want = CR.cond_integrate(sde, kw, x, sf, lambda i, k, p: zs[i, p], ts, h, G, 0, 0.16, obs, mask, None, domain, final,
                                     dtype=dtype)
            got, _ = GR.guided_integrate(sde, kw, x, GR.mixture_score_vjp_fn(sde, kw, mu, lw, var, G, dtype),
                                         lambda i, p: zs[i, p], ts, h, G, obs, mask, guide, None, domain, True, final, dtype)
            assert np.array_equal(got, want), (dtype, final)
    # and without the projection it is the plain Euler-Maruyama run; a split run is the run
    import pc_restatement as P

    plain = P.pc_integrate(sde, kw, x, M.score_fn(sde, kw, mu, lw, var, G), lambda i, k: zs[i, 0], ts, h, G, 0, 0.16)
    got, _ = GR.guided_integrate(sde, kw, x, fn, lambda i, p: zs[i, p], ts, h, G, obs, mask, guide, None, domain, False, False)
    assert np.array_equal(got, plain)
    on = dict(scale=1.0, obs_var=0.04, rho=1.0)
    whole, lw_ = GR.guided_integrate(sde, kw, x, fn, lambda i, p: zs[i, p], ts, h, G, obs, mask, on, None, domain, True, True)
    a, la = GR.guided_integrate(sde, kw, x, fn, lambda i, p: zs[i, p], ts, h, G, obs, mask, on, None, domain, True, True,
                                first=0, n_run=2)
    b, lb = GR.guided_integrate(sde, kw, a, fn, lambda i, p: zs[i, p], ts, h, G, obs, mask, on, None, domain, True, True,
                                first=2, n_run=4)
    assert np.array_equal(b, whole) and np.array_equal(np.concatenate([la, lb]), lw_)
