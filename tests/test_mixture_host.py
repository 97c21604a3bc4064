"""CPU-side tests of the closed-form Gaussian-mixture score backbone (no GPU): the C surface and its argument checks, the
Python surface (MixtureScoreModule, from_data, state_dict, checkpoint round trip), and the numpy restatement
(tests/mixture_restatement.py) against facts it does not share code with -- a finite-difference gradient of its own
log-density, the one-Gaussian analytic score, the reason for the difference form, and the last-step amplification of the
reference's Euler-Maruyama under an exact score."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mixture_restatement as M
import ode_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ------------------------------------------------------------------ the C surface ----
def test_symbols_constant_and_header(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    assert re.search(r"FFD_MODEL_MIXTURE\s*=\s*3", header) and N.FFD_MODEL_MIXTURE == 3
    for name in ("ffd_mixture_score", "ffd_mixture_work_floats", "ffd_host_mixture_check", "ffd_mixture_tiling"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name)
    for key in ("mixture.means", "mixture.log_weights", "mixture.variance"):
        assert key in header
    rt, kt, sl, dmax = (C.c_int() for _ in range(4))
    assert lib.ffd_mixture_tiling(C.byref(rt), C.byref(kt), C.byref(sl), C.byref(dmax)) == 0
    assert (rt.value, kt.value) == (16, 16) and sl.value % kt.value == 0
    assert dmax.value >= 1024  # ECG 187 x 1 and NASA 251 x 4 fit
    assert lib.ffd_mixture_tiling(None, None, None, None) == 0


def test_work_floats(lib):
    sl, dmax = C.c_int(), C.c_int()
    lib.ffd_mixture_tiling(None, None, C.byref(sl), C.byref(dmax))
    S = sl.value
    assert lib.ffd_mixture_work_floats(7, 1, 8, 1) == 7 * (8 + 2)
    assert lib.ffd_mixture_work_floats(7, S, 8, 3) == 7 * (24 + 2)
    assert lib.ffd_mixture_work_floats(7, S + 1, 8, 3) == 2 * 7 * (24 + 2)
    assert lib.ffd_mixture_work_floats(512, 87554, 187, 1) == -(-87554 // S) * 512 * 189
    assert lib.ffd_mixture_work_floats(2, 5, 251, 4) > 0
    for bad in ((0, 1, 8, 1), (1, 0, 8, 1), (1, 1, 0, 1), (1, 1, 8, 0), (1, 1, dmax.value + 1, 1), (1, 1, 513, 2)):
        assert lib.ffd_mixture_work_floats(*bad) == 0, bad


def test_operator_argument_errors(lib):
    """Every refusal comes before any device work: none of these pointers is a device pointer."""
    from fastfourierdiffusion_amd import _native as N

    sde = N.SdeDesc(N.FFD_SDE_VP, 0, 0.1, 20.0)
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    B, K, L, Cn = 2, 3, 8, 1
    need = lib.ffd_mixture_work_floats(B, K, L, Cn)

    def call(sde_=sde, x=p, t=p, stride=0, mu=p, lw=p, var=p, G=p, out=p, B=B, K=K, L=L, Cn=Cn, work=p, wf=need):
        return lib.ffd_mixture_score(C.byref(sde_) if sde_ is not None else None, x, t, stride, mu, lw, var, G, out, B, K, L,
                                     Cn, work, wf, None)

    for kw in (dict(sde_=None), dict(x=None), dict(t=None), dict(mu=None), dict(lw=None), dict(G=None), dict(out=None),
               dict(work=None), dict(B=0), dict(K=0), dict(L=0), dict(Cn=0), dict(stride=2), dict(stride=-1),
               dict(wf=need - 1)):
        assert call(**kw) == INVALID, kw
    assert call(sde_=N.SdeDesc(7, 0, 0.1, 20.0)) == UNSUPPORTED
    assert call(L=1025, wf=1 << 30) == UNSUPPORTED      # L * C over the limit
    assert call(L=513, Cn=2, wf=1 << 30) == UNSUPPORTED


def test_host_mixture_check(lib):
    K, L, Cn = 3, 4, 2
    mu = np.ones((K, L, Cn), np.float32)
    lw = np.log(np.full(K, 1.0 / K)).astype(np.float32)
    var = np.zeros((L, Cn), np.float32)

    def chk(mu=mu, lw=lw, var=var, K=K, L=L, Cn=Cn):
        return lib.ffd_host_mixture_check(fptr(mu), fptr(lw), fptr(var) if var is not None else None, K, L, Cn)

    assert chk() == 0 and chk(var=None) == 0
    one_off = lw.copy()
    one_off[1] = -np.inf
    assert chk(lw=one_off) == 0  # an ignored component is fine
    for v in (np.nan, np.inf, -np.inf):
        bad = mu.copy()
        bad[1, 2, 1] = v
        assert chk(mu=bad) == INVALID
    for v in (-1e-3, np.nan, np.inf):
        bad = var.copy()
        bad[3, 0] = v
        assert chk(var=bad) == INVALID
    for v in (np.nan, np.inf):
        bad = lw.copy()
        bad[2] = v
        assert chk(lw=bad) == INVALID
    assert chk(lw=np.full(K, -np.inf, np.float32)) == INVALID
    assert chk(K=0) == INVALID
    big = np.zeros((1, 1025, 1), np.float32)
    assert lib.ffd_host_mixture_check(fptr(big), fptr(lw), None, 1, 1025, 1) == UNSUPPORTED


def _create(lib, K=3, L=8, Cn=1, kind=3):
    from fastfourierdiffusion_amd import _native as N

    desc = N.ModelDesc(kind, Cn, L, 0, 0, 0, K, 0, 0.1, 20.0, 1, 1e-5)
    h = C.c_void_p()
    rc = lib.ffd_create(C.byref(h), C.byref(desc), 0)
    return rc, h


def test_context_refusals_before_device_work(lib):
    """Shape refusals of ffd_create, the weight names and sizes, a missing tensor and the cache: all decided on the host
    (without a device the context is returned for its error message and its weight table is already bound)."""
    rc, h = _create(lib, K=0)
    assert rc == INVALID, lib.ffd_last_error(h)
    lib.ffd_destroy(h)
    for L, Cn in ((1025, 1), (513, 2), (251, 5)):
        rc, h = _create(lib, L=L, Cn=Cn)
        assert rc == UNSUPPORTED and b"limit" in lib.ffd_last_error(h)
        lib.ffd_destroy(h)
    rc, h = _create(lib, K=3, L=8, Cn=2)
    assert rc == (0 if torch.cuda.is_available() else -4), lib.ffd_last_error(h)
    buf = np.zeros(64, np.float32)
    assert lib.ffd_load_weight(h, b"mixture.scales", buf.ctypes.data, 3) == INVALID     # unknown mixture.* name
    assert b"unexpected parameter" in lib.ffd_last_error(h)
    assert lib.ffd_load_weight(h, b"embedder.weight", buf.ctypes.data, 3) == INVALID    # no network parameters
    assert lib.ffd_load_weight(h, b"mixture.means", buf.ctypes.data, 3 * 8 * 2 - 1) == INVALID
    assert lib.ffd_load_weight(h, b"mixture.log_weights", buf.ctypes.data, 4) == INVALID
    assert lib.ffd_load_weight(h, b"mixture.variance", buf.ctypes.data, 8) == INVALID
    assert lib.ffd_finalize_weights(h) == INVALID and b"missing parameter 'mixture.means'" in lib.ffd_last_error(h)
    assert lib.ffd_cache_enable(h, None) == UNSUPPORTED
    lib.ffd_destroy(h)


# ------------------------------------------------------------------ the Python surface ----
def _sch(sde="vp", L=8):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    s = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=True)
    s.set_noise_scaling(L)
    return s


def test_module_surface_and_from_data(tmp_path):
    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule, ScoreModule

    assert pkg.MixtureScoreModule is MixtureScoreModule and issubclass(MixtureScoreModule, ScoreModule)
    assert MixtureScoreModule._kind == N.FFD_MODEL_MIXTURE
    K, L, Cn = 5, 8, 2
    g = torch.Generator().manual_seed(0)
    X = torch.randn(K, L, Cn, generator=g)
    m = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=_sch(L=L), means=X)
    assert list(m.state_dict()) == ["mixture.means", "mixture.log_weights", "mixture.variance"]
    assert not hasattr(m, "embedder") and not hasattr(m, "backbone")
    assert torch.allclose(m.mixture.log_weights, torch.full((K,), -math.log(K)))
    assert torch.equal(m.mixture.variance, torch.zeros(L, Cn)) and torch.equal(m.mixture.means, X)
    assert m.device.type == "cpu" and m.n_components == K
    d = m._desc()
    assert (d.kind, d.n_channels, d.max_len, d.dim_feedforward, d.fourier_noise_scaling) == (3, Cn, L, K, 1)
    with pytest.raises(AttributeError):
        m.enable_caching()
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    with pytest.raises(N.FFDError):  # no CPU path
        m(DiffusableBatch(X=torch.zeros(2, L, Cn), timesteps=torch.ones(2)))

    bw = torch.rand(L, Cn, generator=g) + 0.1
    w = torch.tensor([1.0, 2.0, 3.0, 0.0, 4.0])
    f = MixtureScoreModule.from_data(X, _sch("ve", L), bandwidth=bw, weights=w, num_training_steps=50)
    assert torch.allclose(f.mixture.variance, bw * bw) and f.num_training_steps == 50
    assert torch.allclose(f.mixture.log_weights.exp(), w / w.sum()) and f.mixture.log_weights[3] == -float("inf")
    f2 = MixtureScoreModule.from_data(X, _sch(L=L), bandwidth=0.2)
    assert torch.allclose(f2.mixture.variance, torch.full((L, Cn), 0.04)) and f2.mixture.means.shape == (K, L, Cn)
    assert (f2.max_len, f2.n_channels) == (L, Cn)

    for bad in (dict(means=X[:, :-1]), dict(means=X[0]), dict(log_weights=torch.zeros(K + 1)),
                dict(variance=torch.zeros(L)), dict(variance=-torch.ones(L, Cn)),
                dict(variance=torch.full((L, Cn), float("nan"))), dict(log_weights=torch.full((K,), -float("inf"))),
                dict(log_weights=torch.tensor([0.0, float("inf"), 0, 0, 0])), dict(means=X * float("nan"))):
        kw = dict(n_channels=Cn, max_len=L, noise_scheduler=_sch(L=L), means=X)
        kw.update(bad)
        with pytest.raises(ValueError):
            MixtureScoreModule(**kw)
    with pytest.raises(ValueError):
        MixtureScoreModule.from_data(X, _sch(L=L), bandwidth=torch.ones(L))
    with pytest.raises(NotImplementedError):
        MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler="ddpm", means=X)

    # load_from_checkpoint on a synthesised file
    path = tmp_path / "mixture.ckpt"
    torch.save({"hyper_parameters": {"n_channels": Cn, "max_len": L, "noise_scheduler": _sch("ve", L),
                                     "num_training_steps": 77, "lr_max": 1e-3},
                "state_dict": f.state_dict()}, path)
    r = MixtureScoreModule.load_from_checkpoint(path)
    assert r.num_training_steps == 77 and type(r.noise_scheduler).__name__ == "VEScheduler"
    for k, v in f.state_dict().items():
        assert torch.equal(r.state_dict()[k], v), k


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("v_mode", [0, 1], ids=["v0", "v>0"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_score_is_the_gradient_of_log_pt(sde, v_mode):
    """float64 score == central finite differences of log p_t, to 1e-6 relative."""
    kw = M.sde_kwargs(sde)
    for shape, t in (((4, 8, 1, 3), 0.5), ((5, 20, 3, 17), 0.05), ((2, 8, 1, 3), 1.0)):
        x, mu, lw, var, G = M.make_case(shape, sde, t, v_mode)
        x = x.astype(np.float64)
        s, _, c = M.evaluate(sde, kw, x, t, mu, lw, var, G)
        grad = np.zeros_like(s)
        flat = grad.reshape(x.shape[0], -1)
        for j in range(flat.shape[1]):
            h = 1e-5 * math.sqrt(float(c.reshape(x.shape[0], -1)[0, j]))
            e = np.zeros(flat.shape[1])
            e[j] = h
            e = e.reshape(1, *x.shape[1:])
            flat[:, j] = (M.log_pt(sde, kw, x + e, t, mu, lw, var, G) - M.log_pt(sde, kw, x - e, t, mu, lw, var, G)) / (2 * h)
        assert np.abs(grad - s).max() <= 1e-6 * np.abs(s).max(), (shape, t)


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_one_component_is_the_analytic_gaussian(sde):
    kw = M.sde_kwargs(sde)
    L = 20
    G = R.fourier_G(L)
    x = R.gaussian_start(L)
    var = np.full((L, 1), R.DATA_STD ** 2)
    for t in M.TIMES:
        s = M.score(sde, kw, x, t, np.zeros((1, L, 1)), np.zeros(1), var, G)
        want = R.gaussian_score(sde, kw, G)(x, float(np.float32(t)))
        assert np.abs(s - want).max() <= 1e-12 * np.abs(want).max()


def grid_cases():
    for sde in ("vp", "ve"):
        for shape in M.SHAPES:
            for t in M.TIMES:
                for v_mode in (0, 1):
                    yield sde, shape, t, v_mode


def test_difference_form_holds_and_expanded_form_fails():
    """The reason for the form.  fp32 difference form: the displacement stays within 6e-7 of max(|x|, alpha |mu|) of the
    float64 value on the whole grid (measured: 3.7e-7); the fp32 expanded (GEMM) form exceeds 2e-6 at every t <= 0.05
    with v = 0, VP and VE (the worst of the four shapes at that time; measured 3.9e-6 at VP t = 0.05 up to 1.7e-4 at VP
    t = 1e-5; the 8-coordinate shape alone has too few terms to show it)."""
    worst_diff, worst_exp = 0.0, {}
    for sde, shape, t, v_mode in grid_cases():
        kw = M.sde_kwargs(sde)
        x, mu, lw, var, G = M.make_case(shape, sde, t, v_mode)
        al = M.alpha_sigma2(sde, kw, t)[0]
        _, d64, _ = M.evaluate(sde, kw, x, t, mu, lw, var, G)
        _, d32, _ = M.evaluate(sde, kw, x, t, mu, lw, var, G, np.float32)
        e = M.displacement_error(d32, d64, x, mu, al)
        worst_diff = max(worst_diff, e)
        assert e <= 6e-7, (sde, shape, t, v_mode, e)
        if v_mode == 0 and t <= 0.05:
            _, dx, _ = M.evaluate(sde, kw, x, t, mu, lw, var, G, np.float32, form="expanded")
            worst_exp[(sde, t)] = max(worst_exp.get((sde, t), 0.0), M.displacement_error(dx, d64, x, mu, al))
    print(f"difference form worst {worst_diff:.2e}; expanded form worst per (sde, t): {worst_exp}")
    assert len(worst_exp) == 6
    for key, ex in worst_exp.items():
        assert ex > 2e-6, (key, ex)


def _em_run(sde, means, var, N, seed, B=16):
    """float64 Euler-Maruyama under the exact score of the uniform mixture: the state before and after the last step."""
    kw = M.sde_kwargs(sde)
    K, L, Cn = means.shape
    G = M.fourier_G(L)
    lw = np.full(K, -math.log(K))
    ts, h = R.grid(N)
    rng = np.random.default_rng(seed)
    x = G[None, :, None] * rng.standard_normal((B, L, Cn)) * (kw["sigma_max"] if sde == "ve" else 1.0)
    before = None
    for i in range(N):
        before = x
        s = M.score(sde, kw, x, ts[i], means, lw, var, G)
        x = M.em_step(sde, kw, x, s, G, ts[i], h, rng.standard_normal(x.shape))
    return before, x, ts, h, G


def _nearest(x, means):
    return np.sqrt(((x[:, None] - means[None]) ** 2).reshape(x.shape[0], means.shape[0], -1).sum(-1)).min(-1)


def test_mode_weight_case_on_the_cpu():
    """The seed of test_mixture_gpu.test_mode_weights_end_to_end: float64, numpy draws, 2048 samples, 200 steps --
    0.80 / 1.19 / 1.72 binomial standard deviations from the weights 0.2 / 0.3 / 0.5."""
    x, mu = M.mode_run("vp")
    dev = M.mode_sigmas(x, mu)
    print(f"mode weights, float64 restatement: {dev}")
    assert (dev < 3.0).all(), dev


def test_vp_last_step_amplification():
    """Known property of the reference algorithm under an exact score (documented, not fixed): with v = 0 under VP,
    Euler-Maruyama takes a step AT t = eps = 1e-5, where dt beta G^2 / c is about 100 at N = 1000 (1 would land on the
    posterior mean), so the last step throws the sample off the data; at N = 50 it is about 2000.  A bandwidth > 0
    bounds c from below and removes it; the ODE solvers never evaluate at eps; VE is unaffected."""
    L, K = 8, 3
    means = 2.0 * np.random.default_rng(5).standard_normal((K, L, 1))
    ts, h = R.grid(1000)
    G = M.fourier_G(L)
    gain = M.last_step_gain("vp", M.VP, None, G, ts[-1], h)
    assert 90.0 < gain < 110.0, gain
    assert M.last_step_gain("vp", M.VP, np.full((L, 1), 0.04), G, ts[-1], h) < 0.01
    assert M.last_step_gain("ve", M.VE, None, G, ts[-1], h) < 20.0 * M.last_step_gain("ve", M.VE, None, G, ts[-2], h)
    before, after, *_ = _em_run("vp", means, None, 1000, seed=1)
    d0, d1 = _nearest(before, means), _nearest(after, means)
    print(f"VP v=0 N=1000: distance to the nearest mean before the last step {d0.max():.3f}, after {d1.max():.3f}")
    assert d1.max() > 1.0 and d1.max() > 10.0 * d0.max()
    _, after50, *_ = _em_run("vp", means, None, 50, seed=1)
    assert np.abs(after50).max() > 50.0
    # with a bandwidth the same run ends on the data, and so do VE and the ODE
    var = np.full((L, 1), 0.04)
    _, smooth, *_ = _em_run("vp", means, var, 1000, seed=1)
    assert _nearest(smooth, means).max() < 5.0 * math.sqrt(0.04 * L)
    _, ve, *_ = _em_run("ve", means, None, 1000, seed=1)
    assert _nearest(ve, means).max() < 0.5
    x0 = G[None, :, None] * np.random.default_rng(2).standard_normal((16, L, 1))
    lw = np.full(K, -math.log(K))
    ts, h = R.grid(1000)  # (Euler: its last evaluation is at the grid's last-but-one point, never at eps)
    ode = R.integrate("ode_euler", "vp", M.VP, x0, M.score_fn("vp", M.VP, means, lw, None, G), ts, h, G)
    print(f"VP v=0 N=1000 ode_euler: distance to the nearest mean {_nearest(ode, means).max():.3f}")
    assert _nearest(ode, means).max() < 0.3
