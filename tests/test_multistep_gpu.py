"""GPU tests of the linear multistep ODE solvers (``ode_ab2``, ``dpmpp_2m``).

1. the context-free operator against the float64 restatement (tests/multistep_restatement.py), with and without history;
2. the analytic Gaussian case with the device's operator: the restatement's errors and second order;
3. whole trajectories of ``DiffusionSampler.sample`` (the fused loop ``ffd_sample_batch_ode``) against the oracle's score
   network + the fp32 restatement of the update, TOL_TRAJ, over the tail paths of test_ode_gpu's model set (fused
   scalar / quad / ragged tile, stand-alone, LSTM, MLP, FreSca, E2-CRF cache);
4. properties: fused == stand-alone tail bit for bit, run-to-run and call-splitting bit-identity at every split point,
   the FFD_ERR_STATE cases of a continued trajectory, shard invariance under philox, the sampler's output contract,
   ``reverse_diffusion_step`` walked over the grid.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import multistep_restatement as M
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O
from test_multistep_host import GAUSS_N, gaussian_errors, interval_cases
from test_ode_gpu import (TOL_TRAJ, TRAJ_MODELS, TRAJ_N, _tune_defaults, build, ffd, oracle_score_fn, sampler_for,  # noqa: F401
                          scheduler)

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6  # a single operator, of the output's max-norm; or three times the fp32 restatement's own error
SOLVERS = M.METHODS
SDES = {"vp": cases.VP, "ve": cases.VE}


# ------------------------------------------------------------------ 1. operator ----
@pytest.mark.parametrize("shape", [(3, 21, 1), (3, 21, 3), (3, 20, 4), (2, 187, 1), (3, 21, 20)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_vs_float64_restatement(ffd, sde, fourier, shape):
    """Bar: max(2e-6, 3 x the fp32 restatement's own error against float64) of the output's max-norm, for x and for the
    history (3 x: the margin the conditional-sampling tests give operation-order differences).  Measured maxima over
    all cases: x 1.63e-7, history 1.35e-7."""
    B, L, Cn = shape
    sch = scheduler(sde, fourier, L, N=12)
    points, h = interval_cases(12)
    assert h == float(sch.step_size)
    G = sch.G.numpy()
    rng = np.random.default_rng(2000 + 7 * L + Cn)
    x, s, hp = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    xd, sd_, hd = (torch.from_numpy(a).cuda() for a in (x, s, hp))
    worst = [0.0, 0.0]
    for method in SOLVERS:
        for tp, t, tn in points:
            for have in (False, True):
                out, hist = sch.ode_multistep_step(model_output=sd_, timestep=t, timestep_next=tn, sample=xd, method=method,
                                                   history=hd if have else None, timestep_prev=tp if have else None)
                coef = M.coefficients(method, sde, SDES[sde], t, tn, h, tp if have else None)
                x64, q64 = M.step(coef, x, s, G, hp if have else None)
                x32, q32 = M.step(coef, x, s, G, hp if have else None, dtype=np.float32)
                for k, (got, r64, r32) in enumerate(((out.prev_sample, x64, x32), (hist, q64, q32))):
                    err, bar = rel_err(got.cpu(), r64), max(TOL_OP, 3.0 * rel_err(r32, r64))
                    worst[k] = max(worst[k], err)
                    assert err < bar, (method, t, have, "x" if k == 0 else "hist", err, bar)
    print(f"operator {sde} {'fourier' if fourier else 'unit'} {shape}: max rel err x {worst[0]:.3e} hist {worst[1]:.3e}")
    for a, b in ((xd, x), (sd_, s), (hd, hp)):  # inputs untouched
        assert torch.equal(a.cpu(), torch.from_numpy(b))


def test_first_interval_does_not_read_the_history(ffd):
    """have_prev == 0 writes the history only: a buffer of NaN leaves no trace."""
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    for shape in ((3, 21, 3), (3, 20, 4)):  # scalar and quad kernel
        B, L, Cn = shape
        sch = scheduler("vp", True, L, N=12)
        rng = np.random.default_rng(5)
        x, s = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(2))
        want, hist = sch.ode_multistep_step(s, 0.5, 0.25, x, "dpmpp_2m")
        x2 = x.clone()
        h2 = torch.full_like(x, float("nan"))
        coef = (C_.c_double * 5)(*sch.multistep_coefficients("dpmpp_2m", 0.5, 0.25))
        assert lib.ffd_ode_multistep_step(x2.data_ptr(), s.data_ptr(), sch._G_on(x.device).data_ptr(), h2.data_ptr(), coef, 0,
                                          B, L, Cn, N.current_stream_ptr(x.device)) == 0
        assert torch.equal(x2, want.prev_sample) and torch.equal(h2, hist)


# ------------------------------------------------------------ 2. analytic Gaussian ----
@pytest.fixture(scope="module")
def gaussian_reference():
    """float64 restatement errors at N = 17 / 33 / 65, computed once."""
    return {(sde, method): gaussian_errors(sde, method) for sde in SDES for method in SOLVERS}


@pytest.mark.parametrize("method", SOLVERS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_analytic_gaussian_error_and_order(ffd, gaussian_reference, sde, method):
    """Data N(0, 1.5^2) per coordinate: the score is -x / var(t) and the ODE's flow map is x sqrt(var(t) / var(1)).
    float64 restatement, relative max error at N = 17 / 33 / 65:
        VP AB2 8.92e-3 2.40e-3 6.18e-4   VP DPM++ 8.82e-2 2.14e-2 5.41e-3
        VE AB2 1.61e-3 5.08e-4 1.40e-4   VE DPM++ 2.60e-3 5.53e-4 1.28e-4"""
    kw = SDES[sde]
    L = 20
    x0 = M.gaussian_start(L)
    errs = []
    for N in GAUSS_N:
        sch = scheduler(sde, True, L, N)
        assert np.array_equal(sch.G.numpy(), M.fourier_G(L))
        ts = [float(t) for t in sch.timesteps]
        G64 = sch.G.numpy().astype(np.float64)
        x = torch.from_numpy(x0.astype(np.float32)).cuda()
        hist = None
        for i in range(N - 1):
            inv_var = torch.from_numpy((1.0 / M.gaussian_var(sde, kw, ts[i], G64)).astype(np.float32)).cuda()[None, :, None]
            out, hist = sch.ode_multistep_step(model_output=-x * inv_var, timestep=ts[i], timestep_next=ts[i + 1], sample=x,
                                               method=method, history=hist, timestep_prev=ts[i - 1] if i else None)
            x = out.prev_sample
        errs.append(M.rel_max_err(x.cpu().numpy(), M.gaussian_exact(sde, kw, x0, 1.0, ts[-1], G64)))
    want = gaussian_reference[(sde, method)]
    print(f"gaussian {sde} {method}: device {errs} restatement {want}")
    for e, w in zip(errs, want):
        assert abs(e - w) <= 0.02 * w, (errs, want)
    for a, b in zip(errs, errs[1:]):
        assert 3.0 <= a / b <= 5.5, errs


# ------------------------------------------------------------------ 3. trajectories ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("name", sorted(TRAJ_MODELS))
def test_trajectory_vs_oracle(ffd, name, sde, solver):
    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, sde)
    B, L, Cn, N = c["B"], c["L"], c["C"], TRAJ_N
    z0 = next(synthetic.noise_stream((B, L, Cn), 1, 900 + len(name)))
    sampler = sampler_for(m, c, solver)
    sampler.inject_noise([z0])
    out = sampler.sample(num_samples=B, num_diffusion_steps=N)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu"

    ts, h = O.timesteps(N)
    G = O.noise_scaling(L, True)
    x0 = O.prior(torch.from_numpy(z0), G, SDES[sde]["sigma_max"] if sde == "ve" else None).numpy()
    table = O.KVTable(c["NL"], L) if "cache" in c else None
    ref = M.integrate(solver, sde, SDES[sde], x0, oracle_score_fn(c, sd, N, table), ts.numpy(), float(h), G.numpy(),
                      dtype=np.float32)
    err = rel_err(out, ref)
    print(f"trajectory {name} {sde} {solver}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err
    if table is not None:
        st = m._native_cache_stats()
        assert (st.recompute_count, st.cache_hit_count) == (table.recompute_count, table.cache_hit_count)
        assert st.recompute_count == L * c["NL"] and st.cache_hit_count == (N - 2) * L * c["NL"]
        assert st.table_allocated == 1 and m.cache.current_step == N - 2
        m.disable_caching()


# ------------------------------------------------------------------ 4. properties ----
def _run(m, c, solver, z0=None, **kw):
    s = sampler_for(m, c, solver, **kw)
    if z0 is not None:
        s.inject_noise([z0])
    return s.sample(num_samples=c["B"], num_diffusion_steps=TRAJ_N)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_c4_quad", "lstm_d16"])
def test_fused_tail_equals_standalone_tail_and_runs_repeat(ffd, name, solver):
    from fastfourierdiffusion_amd import _native

    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, "vp")
    z0 = next(synthetic.noise_stream((c["B"], c["L"], c["C"]), 1, 31))
    lib = _native.lib()
    ctx = m._ctx()
    fused = _run(m, c, solver, z0)
    flops, nbytes = C_.c_double(), C_.c_double()
    tail = lib.ffd_kernel_work(ctx.handle, _native.K_SDE, c["B"], 0, C_.byref(flops), C_.byref(nbytes))
    rows = c["B"] * c["L"]
    assert tail == b"k_unembed_multistep" and nbytes.value == 4.0 * rows * (c["d"] + 4 * c["C"]), (tail, nbytes.value)
    assert torch.equal(_run(m, c, solver, z0), fused)             # two identical runs: bit-identical
    assert torch.equal(_run(m, c, solver, z0, seed=1234), fused)  # no draw depends on the seed
    assert lib.ffd_tune(b"fuse_tail", 0) == 0
    plain = _run(m, c, solver, z0)
    tail = lib.ffd_kernel_work(ctx.handle, _native.K_SDE, c["B"], 0, C_.byref(flops), C_.byref(nbytes))
    assert tail == b"k_multistep_step" and nbytes.value == 20.0 * rows * c["C"] and flops.value == 0.0, tail
    assert torch.equal(plain, fused)  # the same score tile and the same update: bit for bit
    assert torch.equal(_run(m, c, solver, z0), plain)


def _loop(m, c, sde_grid_n=TRAJ_N):
    """(run(x, first, count, solver code, B), the grid) on the model's native context."""
    from fastfourierdiffusion_amd import _native as N

    sch = m.noise_scheduler
    sch.set_timesteps(sde_grid_n)
    ts_c = (C_.c_float * sde_grid_n)(*sch.timesteps.tolist())
    h = float(sch.step_size)
    ctx = m._ctx()
    stream = N.current_stream_ptr(m.device)

    def run(x, first, count, sol, B=c["B"]):
        return ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), B, ts_c, sde_grid_n, h, first, count, sol, 0, 0, stream)

    return run, ctx


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_c20_unfused"])
def test_call_splitting_at_every_point(ffd, name, solver):
    """A 6-interval trajectory cut at every point (1 | 5: the first-order interval, then history) gives the single
    call's bits; so do three calls; the FFD_K_SDE class counts one tail launch per interval."""
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import MULTISTEP_SOLVERS

    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, "ve")
    B, L, Cn, n = c["B"], c["L"], c["C"], 7
    run, ctx = _loop(m, c, n)
    code = MULTISTEP_SOLVERS[solver]
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 77))).cuda()
    one = x0.clone()
    assert ctx.lib.ffd_kernel_timing_begin(ctx.handle, 1 << N.K_SDE, 64) == 0
    assert run(one, 0, n - 1, code) == 0
    assert ctx.lib.ffd_kernel_timing_end(ctx.handle) == 0
    ms, launches = C_.c_float(), C_.c_int()
    assert ctx.lib.ffd_kernel_timing_get(ctx.handle, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
    assert launches.value == n - 1
    assert not torch.equal(one, x0) and bool(torch.isfinite(one).all())
    for cut in range(0, n):  # 0 | 6 and 6 | 0 hold an empty call
        two = x0.clone()
        assert run(two, 0, cut, code) == 0 and run(two, cut, n - 1 - cut, code) == 0
        assert torch.equal(one, two), cut
    three = x0.clone()
    assert run(three, 0, 2, code) == 0 and run(three, 2, 1, code) == 0 and run(three, 3, 3, code) == 0
    assert torch.equal(one, three)
    # the history matters: the same second call after a first-order restart differs
    other = x0.clone()
    assert run(other, 0, 3, code) == 0
    mid = other.clone()
    assert run(other, 3, 3, code) == 0 and torch.equal(other, one)
    assert run(mid, 0, 0, code) == 0  # an empty call at 0 starts a new trajectory: no history is kept
    assert run(mid, 3, 3, code) == -3


@pytest.mark.parametrize("solver", SOLVERS)
def test_continuing_without_the_matching_history_is_a_state_error(ffd, solver):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import MULTISTEP_SOLVERS

    c = dict(TRAJ_MODELS["tf_d24_ragged"], B=4)
    m, sch, sd = build(c, "vp")
    B, L, Cn, n = c["B"], c["L"], c["C"], TRAJ_N
    run, ctx = _loop(m, c, n)
    code = MULTISTEP_SOLVERS[solver]
    other = MULTISTEP_SOLVERS[[s for s in SOLVERS if s != solver][0]]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 79))).cuda()
    keep = x.clone()
    STATE = -3
    assert run(x, 3, 2, code) == STATE  # a fresh context
    assert b"multistep" in ctx.lib.ffd_last_error(ctx.handle)
    assert run(x, 0, 3, N.FFD_SOLVER_ODE_EULER) == 0 and run(x, 3, 2, code) == STATE  # after an Euler call
    assert run(x, 0, 3, N.FFD_SOLVER_ODE_HEUN) == 0 and run(x, 3, 2, code) == STATE
    assert run(x, 0, 3, other) == 0 and run(x, 3, 2, code) == STATE  # the other multistep solver's history
    x.copy_(keep)
    assert run(x, 0, 3, code) == 0
    after3 = x.clone()
    assert run(x, 4, 2, code) == STATE and run(x, 2, 2, code) == STATE  # the call ended at interval 3
    assert run(x[:2], 3, 2, code, B=2) == STATE  # another B
    assert torch.equal(x, after3)  # refused before any device work
    assert run(x, 3, 2, code) == 0  # the refusals left the history in place
    assert run(x, 5, 1, code) == 0
    assert run(x, 6, 1, N.FFD_SOLVER_ODE_EULER) == 0 and run(x, 7, 1, code) == STATE  # Euler dropped it
    # after ffd_sample_batch
    x.copy_(keep)
    assert run(x, 0, 3, code) == 0
    ts_c = (C_.c_float * n)(*sch.timesteps.tolist())
    assert ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), B, ts_c, n, float(sch.step_size), 3, 1, 1, 0, None, 0, 0,
                                    N.current_stream_ptr(m.device)) == 0
    assert run(x, 3, 2, code) == STATE
    # the loop keeps refusing what it refused
    for bad in (N.FFD_SOLVER_EULER_MARUYAMA, N.FFD_SOLVER_PC, 7):
        assert run(x, 0, 1, bad) == -1
    assert run(x, 0, n, code) == -1 and run(x, 0, 2, code) == 0


@pytest.mark.parametrize("solver", SOLVERS)
def test_philox_prior_shards_agree(ffd, solver):
    c = dict(TRAJ_MODELS["tf_d24_ragged"], B=6)
    m, sch, sd = build(c, "vp")
    full = _run(m, c, solver, rng="philox", seed=5)
    half = dict(c, B=3)
    parts = torch.cat([_run(m, half, solver, rng="philox", seed=5, sample_offset=o) for o in (0, 3)])
    assert not torch.equal(full[:3], full[3:])
    assert rel_err(parts, full) < TOL_TRAJ
    # two batches of one sample() call: the second starts without the first one's history
    two = sampler_for(m, half, solver, rng="philox", seed=5).sample(num_samples=6, num_diffusion_steps=TRAJ_N)
    assert torch.equal(two, parts)


@pytest.mark.parametrize("solver", SOLVERS)
def test_sampler_output_contract(ffd, solver):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = TRAJ_MODELS["tf_d24_ragged"]
    m, sch, sd = build(c, "vp")
    torch.manual_seed(3)
    out = DiffusionSampler(m, 4, solver=solver).sample(8, 12)  # two batches, torch prior
    assert tuple(out.shape) == (8, c["L"], c["C"]) and out.device.type == "cpu" and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        DiffusionSampler(m, 4, solver=solver).sample(4, 1)  # a one-point grid has no interval


@pytest.mark.parametrize("solver", SOLVERS)
def test_reverse_diffusion_step_walks_the_grid_like_sample(ffd, solver):
    """The single-step API keeps the history between consecutive calls: walked over the grid it equals ``sample``; a call
    that does not continue the previous one is the first-interval form."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = TRAJ_MODELS["tf_d24_ragged"]
    m, sch, sd = build(c, "vp")
    B, L, Cn, N = c["B"], c["L"], c["C"], TRAJ_N
    z0 = next(synthetic.noise_stream((B, L, Cn), 1, 78))
    want = _run(m, c, solver, z0)
    sampler = DiffusionSampler(m, B, solver=solver)
    sampler.inject_noise([z0])
    X = sampler.sample_prior(B)
    sch.set_timesteps(N)

    def step(X, i, s=sampler):
        t = float(sch.timesteps[i])
        return s.reverse_diffusion_step(DiffusableBatch(X=X, y=None, timesteps=torch.full((B,), t, device="cuda")))

    states = [X]
    for i in range(N - 1):
        states.append(step(states[-1], i))
    assert rel_err(states[-1].cpu(), want) < TOL_TRAJ
    # interval 4 from the same state, out of sequence (a fresh sampler; after interval 7): the first-interval form
    ref = M.integrate(solver, "vp", cases.VP, states[4].cpu().numpy(), oracle_score_fn(c, sd, N), sch.timesteps.numpy(),
                      float(sch.step_size), sch.G.numpy(), dtype=np.float32, first=4, n_run=1)
    for s in (DiffusionSampler(m, B, solver=solver), sampler):
        out = step(states[4], 4, s)
        assert rel_err(out.cpu(), ref) < TOL_TRAJ
        assert not torch.equal(out, states[5])
    for bad in (float(sch.timesteps[-1]), 0.123):
        batch = DiffusableBatch(X=X, y=None, timesteps=torch.full((B,), bad, device="cuda"))
        with pytest.raises(ValueError):
            sampler.reverse_diffusion_step(batch)
