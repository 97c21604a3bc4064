"""GPU tests of the closed-form Gaussian-mixture score: the operator ``ffd_mixture_score``, the backbone
``FFD_MODEL_MIXTURE`` behind the context, and ``MixtureScoreModule`` through the public sampler and loss.

1. the operator against the float64 restatement (tests/mixture_restatement.py) on its grid and on the edge shapes of the
   kernel's tiling; the bar is on the displacement score * c64:
       <= max(2e-6, 3 x the fp32 difference-form restatement's own error on that case) x max(|x|, alpha |mu|);
2. exact and degenerate cases; 3. independence of batching, per-sample times, run-to-run identity;
4. through the context, bit for bit against the operator; 5. trajectories of DiffusionSampler against the float64
   restatement (1e-5 of the max-norm); 6. the analytic Gaussian case through the public sampler; 7. the validation loss;
8. mode weights end to end; 9. Philox shards.
"""
import ctypes as C_
import math

import numpy as np
import pytest
import torch

import cond_restatement as CR
import mixture_restatement as M
import multistep_restatement as MS
import ode_restatement as R
import pc_restatement as P
from conftest import rel_err
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6    # the floor of a single operator's bar (the other operators' floor)
TOL_TRAJ = 1e-5  # a trajectory, of the max-norm (the project's trajectory contract)
TOL_SCORE = 1e-5  # test_loss_gpu's score tolerance in its MLP loss bar
SDES = {"vp": M.VP, "ve": M.VE}
ODE_SOLVERS = ("ode_euler", "ode_heun", "ode_ab2", "dpmpp_2m")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def tiling(lib):
    v = [C_.c_int() for _ in range(4)]
    assert lib.ffd_mixture_tiling(*(C_.byref(i) for i in v)) == 0
    return tuple(i.value for i in v)  # row tile, component tile, slice, max dim


def run_op(lib, sde, kw, x, t, means, lw, var, G, per_sample=False):
    """ffd_mixture_score on numpy inputs -> numpy score.  t: a float (shared, stride 0) or, per_sample, an array (B,)."""
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn = x.shape
    K = means.shape[0]
    a, b = (kw["beta_min"], kw["beta_max"]) if sde == "vp" else (kw["sigma_min"], kw["sigma_max"])
    desc = N.SdeDesc(N.FFD_SDE_VP if sde == "vp" else N.FFD_SDE_VE, 0, a, b)
    xd, md, ld, Gd = dev(x), dev(means), dev(lw), dev(G)
    vd = dev(var) if var is not None else None
    td = dev(np.asarray(t, np.float32).reshape(-1))
    assert td.numel() == (B if per_sample else 1)
    n = lib.ffd_mixture_work_floats(B, K, L, Cn)
    assert n > 0
    work = torch.empty(n, device="cuda", dtype=torch.float32)
    out = torch.empty_like(xd)
    rc = lib.ffd_mixture_score(C_.byref(desc), xd.data_ptr(), td.data_ptr(), 1 if per_sample else 0, md.data_ptr(),
                               ld.data_ptr(), vd.data_ptr() if vd is not None else None, Gd.data_ptr(), out.data_ptr(), B, K,
                               L, Cn, work.data_ptr(), n, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


WORST = {}


def check_case(lib, sde, shape, t, v_mode, fourier, what):
    kw = SDES[sde]
    x, mu, lw, var, G = M.make_case(shape, sde, t, v_mode, fourier)
    al = M.alpha_sigma2(sde, kw, t)[0]
    _, d64, c64 = M.evaluate(sde, kw, x, t, mu, lw, var, G)
    _, d32, _ = M.evaluate(sde, kw, x, t, mu, lw, var, G, np.float32)
    own = M.displacement_error(d32, d64, x, mu, al)
    got = run_op(lib, sde, kw, x, t, mu, lw, var, G)
    assert np.isfinite(got).all()
    err = M.displacement_error(got.astype(np.float64) * c64, d64, x, mu, al)
    bar = max(TOL_OP, 3.0 * own)
    WORST[what] = max(WORST.get(what, 0.0), err)
    print(f"{what} {sde} {shape} t={t} v={v_mode} fourier={fourier}: device {err:.2e} restatement {own:.2e} bar {bar:.2e}")
    assert err <= bar, (sde, shape, t, v_mode, err, bar)


# ------------------------------------------------------------------ 1. operator ----
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_vs_float64_on_the_grid(lib, sde, fourier, shape):
    """Largest device error measured on the grid: see DESIGN.md section 5."""
    for t in M.TIMES:
        for v_mode in (0, 1):
            check_case(lib, sde, shape, t, v_mode, fourier, "grid")


def edge_shapes():
    RT, KT, SL = 16, 16, 512  # asserted against ffd_mixture_tiling in the test
    return [(3, 8, 1, 1), (3, 8, 2, KT - 1), (3, 8, 2, KT), (3, 8, 2, KT + 1), (3, 8, 1, SL - 1), (3, 8, 1, SL),
            (3, 8, 1, SL + 1), (2, 6, 1, 2 * SL + 3), (1, 8, 1, 3), (RT - 1, 5, 1, 3), (RT, 5, 1, 3), (RT + 1, 5, 1, 3),
            (2, 251, 4, 5), (3, 7, 8, 5), (2, 512, 1, 5), (2, 64, 1, 5), (2, 65, 1, 5), (2, 192, 1, 5), (2, 193, 1, 5),
            (2, 256, 1, 5), (2, 257, 1, 5), (2, 513, 1, 5)]


@pytest.mark.parametrize("shape", edge_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_operator_edge_shapes(lib, shape):
    """K = 1; K at the component tile -1 / exact / +1; K across the slice boundary; B = 1 and at the row tile +-1; L C at the
    limit; C = 8; L = 512; and L C across every instance boundary of the kernel (64, 192, 256, 512 coordinates)."""
    assert tiling(lib)[:3] == (16, 16, 512)
    check_case(lib, "vp", shape, 0.05, 0, True, "edge")
    check_case(lib, "ve", shape, 0.5, 1, False, "edge")


# ------------------------------------------------------------------ 2. exact and degenerate cases ----
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_one_component_is_elementwise(lib, sde):
    kw = SDES[sde]
    for shape, t, v_mode in (((5, 20, 3, 1), 0.5, 1), ((3, 187, 1, 1), 1e-3, 0), ((2, 8, 1, 1), 1.0, 1)):
        x, mu, lw, var, G = M.make_case(shape, sde, t, v_mode)
        # the operator's own coefficients: alpha and sigma^2 formed in double and ROUNDED ONCE to fp32 (at small t the
        # displacement alpha mu - x cancels, and alpha's last fp32 bit is 6e-8 |mu| against |d| ~ sigma)
        al, s2 = (float(np.float32(v)) for v in M.alpha_sigma2(sde, kw, t))
        v = 0.0 if var is None else var.astype(np.float64)
        c = al * al * v + s2 * (G.astype(np.float64) ** 2)[:, None]
        want = (al * mu[0].astype(np.float64)[None] - x) / c[None]
        got = run_op(lib, sde, kw, x, t, mu, lw, var, G)
        assert rel_err(got, want) <= 1e-6, (shape, t)


def test_far_component_is_ignored_and_inf_weight_changes_nothing(lib):
    sde, kw, t = "vp", M.VP, 0.5
    x, mu, lw, var, G = M.make_case((4, 20, 3, 2), sde, t, 1)
    mu[1] = mu[0] + np.float32(1e3 / math.sqrt(60))   # two components 1e3 apart
    x = (M.alpha_sigma2(sde, kw, t)[0] * mu[0][None] + 0.3 * np.random.default_rng(3).standard_normal(x.shape)).astype(np.float32)
    both = run_op(lib, sde, kw, x, t, mu, np.log(np.float32([0.5, 0.5])), var, G)
    near = run_op(lib, sde, kw, x, t, mu[:1], np.zeros(1, np.float32), var, G)
    assert rel_err(both, near) <= 1e-6
    # a -inf-weight component, appended so that the tile count is unchanged: bit for bit the mixture without it
    x, mu, lw, var, G = M.make_case((4, 20, 3, 6), sde, t, 1)
    base = run_op(lib, sde, kw, x, t, mu[:5], lw[:5], var, G)
    lw6 = lw.copy()
    lw6[5] = -np.inf
    assert np.array_equal(run_op(lib, sde, kw, x, t, mu, lw6, var, G), base)
    # ... and in front of a whole slice of its own
    big = np.concatenate([mu[:5], np.repeat(mu[5:], 512 + 3, 0)])
    lwb = np.concatenate([lw[:5], np.full(515, -np.inf, np.float32)])
    assert rel_err(run_op(lib, sde, kw, x, t, big, lwb, var, G), base) <= 1e-6


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_rows_far_from_every_mean_stay_finite(lib, sde):
    """Rows 1e4 noise deviations from every mean: logits near -1e8 L C / 2, no NaN or Inf, and the nearest component
    wins."""
    kw, t = SDES[sde], 0.5
    x, mu, lw, var, G = M.make_case((4, 20, 3, 17), sde, t, 0)
    al, s2 = M.alpha_sigma2(sde, kw, t)
    c = s2 * (G.astype(np.float64) ** 2)[:, None] * np.ones((20, 3))
    x = (al * mu[3][None] + 1e4 * np.sqrt(c)[None] * np.sign(np.random.default_rng(4).standard_normal(x.shape))).astype(np.float32)
    got = run_op(lib, sde, kw, x, t, mu, lw, var, G)
    assert np.isfinite(got).all()
    s64, _, _ = M.evaluate(sde, kw, x, t, mu, lw, var, G)
    assert rel_err(got, s64) <= 1e-5


# ------------------------------------------------------------------ 3. independence of batching ----
@pytest.mark.parametrize("shape", [(7, 20, 3, 17), (7, 187, 1, 70), (7, 8, 1, 515)], ids=lambda s: "x".join(map(str, s)))
def test_rows_are_independent_and_runs_repeat(lib, shape):
    sde, kw, t = "vp", M.VP, 0.05
    x, mu, lw, var, G = M.make_case(shape, sde, t, 1)
    whole = run_op(lib, sde, kw, x, t, mu, lw, var, G)
    assert np.array_equal(run_op(lib, sde, kw, x, t, mu, lw, var, G), whole)  # two runs
    split = np.concatenate([run_op(lib, sde, kw, x[:3], t, mu, lw, var, G), run_op(lib, sde, kw, x[3:], t, mu, lw, var, G)])
    assert np.array_equal(split, whole)
    ones = np.concatenate([run_op(lib, sde, kw, x[i:i + 1], t, mu, lw, var, G) for i in range(7)])
    assert np.array_equal(ones, whole)
    # per-sample times: row by row the shared-time result
    ts = np.float32([1.0, 0.5, 0.05, 1e-3, 1e-5, 0.5, 0.7])
    per = run_op(lib, sde, kw, x, ts, mu, lw, var, G, per_sample=True)
    for i in range(7):
        assert np.array_equal(per[i], run_op(lib, sde, kw, x, float(ts[i]), mu, lw, var, G)[i]), i


# ------------------------------------------------------------------ 4. through the context ----
def scheduler(sde, L, fourier=True, N=None, kw=None):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=fourier, **(kw or SDES[sde]))
    sch.set_noise_scaling(L)
    if N is not None:
        sch.set_timesteps(N)
    return sch


def module(sde, mu, lw, var, fourier=True, kw=None):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    K, L, Cn = mu.shape
    sch = scheduler(sde, L, fourier, kw=kw)
    m = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=None if var is None else torch.from_numpy(var),
                           fourier_noise_scaling=fourier)
    return m.cuda().eval(), sch


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_context_forwards_equal_the_operator(lib, sde):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    kw = SDES[sde]
    x, mu, lw, var, G = M.make_case((5, 20, 3, 17), sde, 0.5, 1)
    m, sch = module(sde, mu, lw, var)
    assert np.array_equal(sch.G.numpy(), G)
    ctx = m._ctx()
    xd = dev(x)
    out = torch.empty_like(xd)
    for t in (1.0, 0.05, 1e-5):
        assert lib.ffd_score_forward(ctx.handle, xd.data_ptr(), t, out.data_ptr(), 5, stream()) == 0
        assert np.array_equal(out.cpu().numpy(), run_op(lib, sde, kw, x, t, mu, lw, var, G))
    ts = np.float32([1.0, 0.5, 0.05, 1e-3, 1e-5])
    want = run_op(lib, sde, kw, x, ts, mu, lw, var, G, per_sample=True)
    assert lib.ffd_score_forward_ts(ctx.handle, xd.data_ptr(), dev(ts).data_ptr(), out.data_ptr(), None, 5, -1, stream()) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    got = m(DiffusableBatch(X=xd, timesteps=torch.from_numpy(ts)))
    assert np.array_equal(got.cpu().numpy(), want)
    # no cache for this kind; the bookkeeping names the kernel
    assert lib.ffd_score_forward_cached(ctx.handle, xd.data_ptr(), 0.5, out.data_ptr(), None, 5, 0, stream()) == -2
    assert lib.ffd_cache_enable(ctx.handle, None) == -2
    fl, by = C_.c_double(), C_.c_double()
    name = lib.ffd_kernel_work(ctx.handle, N.K_ATTN, 5, 0, C_.byref(fl), C_.byref(by))
    assert name == b"k_mixture_part + k_mixture_merge" and fl.value == 7.0 * 5 * 17 * 60
    assert lib.ffd_flops_per_sample_step(ctx.handle, 0) == 7.0 * 17 * 60
    assert lib.ffd_kernel_work(ctx.handle, N.K_SDE, 5, 0, None, None) == b"k_sde_step"  # never a fused tail
    assert lib.ffd_kernel_work(ctx.handle, N.K_EMBED, 5, 0, None, None) is None


# ------------------------------------------------------------------ 5. trajectories ----
TRAJ_SHAPES = [(6, 8, 1, 5), (5, 20, 3, 17)]
FRESCA = dict(low_scale=0.9, high_scale=1.2, cutoff_ratio=0.4, cutoff_strategy="spatial")


def traj_case(shape, sde, v_mode):
    """A mixture with well-spread means (data scale 1), its module and the float64 score function."""
    B, L, Cn, K = shape
    rng = np.random.default_rng(40 + L + K)
    mu = rng.standard_normal((K, L, Cn)).astype(np.float32)
    lw = np.log(rng.dirichlet(np.full(K, 2.0))).astype(np.float32)
    var = M.variance(L, Cn, v_mode)
    m, sch = module(sde, mu, lw, var)
    return m, sch, M.score_fn(sde, SDES[sde], mu, lw, var, sch.G.numpy())


def start(sde, z0, G):
    return O.prior(torch.from_numpy(z0), torch.from_numpy(G), SDES[sde]["sigma_max"] if sde == "ve" else None).numpy()


def noise(shape, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape).astype(np.float32) for _ in range(n)]


@pytest.mark.parametrize("v_mode", [0, 1], ids=["v0", "v>0"])
@pytest.mark.parametrize("solver", ODE_SOLVERS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("shape", TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ode_trajectories_vs_float64(lib, shape, sde, solver, v_mode):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    B, L, Cn, K = shape
    N = 21
    m, sch, fn = traj_case(shape, sde, v_mode)
    z0 = noise((B, L, Cn), 1, 900 + K)[0]
    s = DiffusionSampler(score_model=m, sample_batch_size=B, solver=solver)
    s.inject_noise([z0])
    out = s.sample(num_samples=B, num_diffusion_steps=N)
    ts, h = O.timesteps(N)
    G = sch.G.numpy()
    integ = R.integrate if solver in ("ode_euler", "ode_heun") else MS.integrate
    ref = integ(solver, sde, SDES[sde], start(sde, z0, G), fn, ts.numpy(), float(h), G)
    err = rel_err(out, ref)
    print(f"trajectory {shape} {sde} {solver} v={v_mode}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err


EM_CASES = [(sde, v, n_corr) for sde, v in (("vp", 1), ("ve", 1), ("ve", 0)) for n_corr in (0, 1)]


@pytest.mark.parametrize("sde,v_mode,n_corr", EM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_euler_maruyama_and_corrector_trajectories_vs_float64(lib, shape, sde, v_mode, n_corr):
    """50 steps, injected noise.  VP Euler-Maruyama runs with v > 0 only: with v = 0 its last step is the pathological one
     and amplifies rounding to 4 - 8e-6."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    B, L, Cn, K = shape
    N, snr = 50, 0.16
    m, sch, fn = traj_case(shape, sde, v_mode)
    zs = noise((B, L, Cn), 1 + N * (n_corr + 1), 950 + K)
    s = DiffusionSampler(score_model=m, sample_batch_size=B, corrector_steps=n_corr, snr=snr)
    s.inject_noise(zs)
    out = s.sample(num_samples=B, num_diffusion_steps=N)
    ts, h = O.timesteps(N)
    G = sch.G.numpy()
    ref = P.pc_integrate(sde, SDES[sde], start(sde, zs[0], G), fn, lambda i, k: zs[1 + i * (n_corr + 1) + k], ts.numpy(),
                         float(h), G, n_corr, snr)
    err = rel_err(out, ref)
    print(f"trajectory {shape} {sde} EM n_corr={n_corr} v={v_mode}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err


@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("shape", TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_time_masked_conditional_trajectory_vs_float64(lib, shape, sde):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    B, L, Cn, K = shape
    N, snr, n_corr = 50, 0.16, 1
    m, sch, fn = traj_case(shape, sde, 1)
    rng = np.random.default_rng(70 + K)
    series = rng.standard_normal((1, L, Cn)).astype(np.float32)
    mask = np.zeros((1, L, Cn), np.float32)
    mask[:, : L // 3] = 1.0
    zs = noise((B, L, Cn), 1 + N * (n_corr + 1) * 2, 960 + K)
    s = DiffusionSampler(score_model=m, sample_batch_size=B, corrector_steps=n_corr, snr=snr)
    s.inject_noise(zs)
    out = s.sample_conditional(torch.from_numpy(series[0]), torch.from_numpy(mask[0]), B, N, domain="time",
                               final_replace=True)
    ts, h = O.timesteps(N)
    G = sch.G.numpy()
    ref = CR.cond_integrate(sde, SDES[sde], start(sde, zs[0], G), fn, lambda i, k, p: zs[1 + (i * (n_corr + 1) + k) * 2 + p],
                            ts.numpy(), float(h), G, n_corr, snr, series, mask, None, "time", True)
    err = rel_err(out, ref)
    print(f"conditional trajectory {shape} {sde}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_fresca_trajectory_vs_float64(lib, sde):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    shape = TRAJ_SHAPES[1]
    B, L, Cn, K = shape
    N = 21
    m, sch, fn = traj_case(shape, sde, 1)
    z0 = noise((B, L, Cn), 1, 905)[0]
    s = DiffusionSampler(score_model=m, sample_batch_size=B, solver="ode_euler", use_fresca=True,
                         fresca_low_scale=FRESCA["low_scale"], fresca_high_scale=FRESCA["high_scale"],
                         fresca_cutoff_ratio=FRESCA["cutoff_ratio"], fresca_cutoff_strategy=FRESCA["cutoff_strategy"])
    s.inject_noise([z0])
    out = s.sample(num_samples=B, num_diffusion_steps=N)

    def scaled(x, t, k=0):
        sc = torch.from_numpy(fn(x, t, k)).to(torch.float64)
        return O.fresca(sc, timestep=t, num_steps=N, **FRESCA).numpy()

    ts, h = O.timesteps(N)
    G = sch.G.numpy()
    ref = R.integrate("ode_euler", sde, SDES[sde], start(sde, z0, G), scaled, ts.numpy(), float(h), G)
    err = rel_err(out, ref)
    print(f"FreSca trajectory {sde}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err


# ------------------------------------------------------------------ 6. the analytic Gaussian case ----
@pytest.mark.parametrize("solver", ODE_SOLVERS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_analytic_gaussian_through_the_public_sampler(lib, sde, solver):
    """K = 1, mu = 0, v = 1.5^2, injected prior: sample() reproduces the float64 restatement's error at N = 17 / 33 / 65
    within 2 % and shows the solver's order (test_ode_gpu's and test_multistep_gpu's assertions on the bare operators)."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from oracle import cases

    kw, L = {"vp": cases.VP, "ve": cases.VE}[sde], 20  # the schedulers of test_ode_gpu's analytic case
    z0 = R.gaussian_start(L).astype(np.float32)
    mu, lw, var = np.zeros((1, L, 1), np.float32), np.zeros(1, np.float32), np.full((L, 1), R.DATA_STD ** 2, np.float32)
    m, sch = module(sde, mu, lw, var, kw=kw)
    G64 = sch.G.numpy().astype(np.float64)
    x1 = O.prior(torch.from_numpy(z0), sch.G, kw["sigma_max"] if sde == "ve" else None).numpy().astype(np.float64)
    integ = R.integrate if solver in ("ode_euler", "ode_heun") else MS.integrate
    errs, want = [], []
    for N in (17, 33, 65):
        s = DiffusionSampler(score_model=m, sample_batch_size=z0.shape[0], solver=solver)
        s.inject_noise([z0])
        out = s.sample(num_samples=z0.shape[0], num_diffusion_steps=N).numpy()
        ts, h = R.grid(N)
        exact = R.gaussian_exact(sde, kw, x1, 1.0, float(ts[-1]), G64)
        errs.append(R.rel_max_err(out, exact))
        ref = integ(solver, sde, kw, x1, R.gaussian_score(sde, kw, G64), ts, h, G64)
        want.append(R.rel_max_err(ref, exact))
    print(f"gaussian {sde} {solver}: device {errs} restatement {want}")
    for e, w in zip(errs, want):
        assert abs(e - w) <= 0.02 * w, (errs, want)
    lo, hi = (1.8, 2.2) if solver == "ode_euler" else (3.5, 5.0) if solver == "ode_heun" else (3.0, 5.5)
    for a, b in zip(errs, errs[1:]):
        assert lo <= a / b <= hi, errs


# ------------------------------------------------------------------ 7. validation loss ----
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_validation_loss_vs_float64(lib, sde):
    from test_loss_host import loss_f64, perturb_f64

    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    kw = SDES[sde]
    B, L, Cn, K = 5, 20, 3, 17
    _, mu, lw, var, G = M.make_case((B, L, Cn, K), sde, 0.5, 1)
    m, sch = module(sde, mu, lw, var)
    rng = np.random.default_rng(11)
    x0 = mu[rng.integers(0, K, B)]
    z = rng.standard_normal((B, L, Cn)).astype(np.float32)
    t = torch.tensor([0.3, 0.5, 0.7, 0.9, 1.0])
    mc, sigma = (v.numpy() for v in sch.marginal_coeffs(t))
    xn = perturb_f64(x0, z, mc, sigma, G).astype(np.float32)
    score = M.score(sde, kw, xn, t.numpy(), mu, lw, var, G)
    zd = dev(z)
    for lwt in (0, 1):
        ref = loss_f64(score, z, sigma, G, lwt, 1)
        std = (sigma[:, None] * G[None, :]).astype(np.float64)[:, :, None]
        r = score + z / std
        om = std ** 2 if lwt else 1.0
        sens = (om * np.abs(r)).reshape(B, -1).sum(1) / (om * r * r).reshape(B, -1).sum(1)
        tol = float(np.max(2 * TOL_SCORE * np.abs(score).max() * sens)) + TOL_OP
        m.likelihood_weighting = bool(lwt)
        m.training_loss_fn, m.validation_loss_fn = m.set_loss_fn()
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch, "randn_like", lambda x, **k: zd)
            loss = float(m.validation_step(DiffusableBatch(X=dev(x0), timesteps=t.cuda()), 0))
        err = abs(loss - ref.mean()) / ref.mean()
        print(f"mixture {sde} lw={lwt}: loss {loss:.8e} restatement {ref.mean():.8e} rel {err:.2e} (tol {tol:.2e})")
        assert err <= tol


# ------------------------------------------------------------------ 8. mode weights ----
def test_mode_weights_end_to_end(lib):
    """2048 Philox draws, 200 Euler-Maruyama steps, three well-separated components with weights 0.2 / 0.3 / 0.5 (L = 8,
    v = 0.04): the nearest-component frequencies are within 4.5 binomial standard deviations of the weights.  The float64
    restatement with numpy draws of the same count (M.mode_run, VP, seed 3) gives 0.80 / 1.19 / 1.72 standard
    deviations, inside 3: test_mixture_host.test_mode_weight_case_on_the_cpu asserts it."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    mu, lw, var = M.mode_mixture()
    m, sch = module("vp", mu, lw, var)
    s = DiffusionSampler(score_model=m, sample_batch_size=M.MODE_N, rng="philox", seed=M.MODE_SEED)
    out = s.sample(num_samples=M.MODE_N, num_diffusion_steps=M.MODE_STEPS).numpy()
    dev_ = M.mode_sigmas(out, mu)
    print(f"mode frequencies: deviations in binomial standard deviations {dev_}")
    assert (dev_ <= 4.5).all(), dev_


# ------------------------------------------------------------------ 9. shards ----
@pytest.mark.parametrize("solver", ["euler_maruyama", "ode_heun", "dpmpp_2m"])
def test_philox_shards_agree(lib, solver):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    m, sch, fn = traj_case((6, 20, 3, 17), "vp", 1)

    def run(B, **kw):
        return DiffusionSampler(score_model=m, sample_batch_size=B, solver=solver, rng="philox", seed=5, **kw).sample(B, 21)

    full = run(6)
    parts = torch.cat([run(3, sample_offset=o) for o in (0, 3)])
    assert not torch.equal(full[:3], full[3:])
    assert rel_err(parts, full) < TOL_TRAJ
