"""GPU tests of the probability-flow ODE solvers (``ode_euler``, ``ode_heun``).

1. the three context-free operators against the float64 restatement (tests/ode_restatement.py), TOL_OP;
2. the analytic Gaussian case: signs, the factor 1/2 and the order of convergence, independent of any network;
3. whole trajectories of ``DiffusionSampler.sample`` (the fused loop ``ffd_sample_batch_ode``) against the oracle's score
   network + the fp32 restatement of the update, TOL_TRAJ, over every tail path (fused scalar / quad / ragged tile,
   stand-alone, LSTM, MLP, FreSca, E2-CRF cache);
4. properties: fused == stand-alone tail, run-to-run and call-splitting bit-identity, seed independence, shard
   invariance under philox, the sampler's output contract, the introspection entries.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import ode_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6    # a single operator, of the output's max-norm (the bar of test_step_golden's family)
TOL_TRAJ = 1e-5  # a trajectory, of the max-norm (the project's trajectory contract)
SOLVERS = ("ode_euler", "ode_heun")
SDES = {"vp": cases.VP, "ve": cases.VE}


@pytest.fixture(scope="module")
def ffd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    _native.lib()
    return pkg


@pytest.fixture(autouse=True)
def _tune_defaults():
    from fastfourierdiffusion_amd import _native

    yield
    _native.lib().ffd_tune(b"reset", 0)


def scheduler(sde, fourier, L, N=None):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=fourier, **SDES[sde])
    sch.set_noise_scaling(L)
    if N is not None:
        sch.set_timesteps(N)
    return sch


# ------------------------------------------------------------------ 1. operators ----
@pytest.mark.parametrize("shape", [(3, 21, 1), (3, 21, 3), (3, 20, 4), (2, 187, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operators_vs_float64_restatement(ffd, sde, fourier, shape):
    B, L, Cn = shape
    sch = scheduler(sde, fourier, L, N=12)
    h = float(sch.step_size)
    G = sch.G.numpy()
    rng = np.random.default_rng(1000 + 7 * L + Cn)
    x, s, s2 = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    xd, sd_, s2d = (torch.from_numpy(a).cuda() for a in (x, s, s2))
    for t in (1.0, 0.5, 1e-5):
        tn = t - h if t > h else t  # the corrector's time: the interval's end (any valid time at the grid's last point)
        out = sch.ode_step(model_output=sd_, timestep=t, sample=xd).prev_sample
        assert rel_err(out.cpu(), R.euler_step(sde, SDES[sde], t, x, s, G, h)) < TOL_OP
        xp, d1 = sch.ode_heun_predict(model_output=sd_, timestep=t, sample=xd)
        xp64, d164 = R.heun_predict(sde, SDES[sde], t, x, s, G, h)
        assert rel_err(xp.cpu(), xp64) < TOL_OP and rel_err(d1.cpu(), d164) < TOL_OP
        assert torch.equal(xp, out)  # the predictor's state is the Euler step
        out = sch.ode_heun_correct(model_output_pred=s2d, timestep_next=tn, sample=xd, sample_pred=xp, drift=d1).prev_sample
        # judged from the device's own xp / d1, so that the bound is this operator's alone
        ref = R.heun_correct(sde, SDES[sde], tn, x, xp.cpu().numpy(), s2, d1.cpu().numpy(), G, h)
        assert rel_err(out.cpu(), ref) < TOL_OP
    assert torch.equal(xd.cpu(), torch.from_numpy(x))  # inputs untouched


# ------------------------------------------------------------ 2. analytic Gaussian ----
@pytest.fixture(scope="module")
def gaussian_reference():
    """float64 restatement errors at N = 17 / 33 / 65, computed once."""
    out = {}
    G = R.fourier_G(20)
    x0 = R.gaussian_start()
    for sde, kw in SDES.items():
        for solver in SOLVERS:
            errs = []
            for N in (17, 33, 65):
                ts, h = R.grid(N)
                x = R.integrate(solver, sde, kw, x0, R.gaussian_score(sde, kw, G), ts, h, G)
                errs.append(R.rel_max_err(x, R.gaussian_exact(sde, kw, x0, 1.0, float(ts[-1]), G)))
            out[(sde, solver)] = errs
    return out


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_analytic_gaussian_error_and_order(ffd, gaussian_reference, sde, solver):
    """Data N(0, 1.5^2) per coordinate: the score is -x / var(t) and the ODE's flow map is x sqrt(var(t) / var(1)).
    float64 restatement, relative max error at N = 17 / 33 / 65:
        VP Heun 3.93e-3 9.31e-4 2.27e-4   VP Euler 3.24e-2 1.61e-2 8.05e-3
        VE Heun 4.78e-3 1.10e-3 2.63e-4   VE Euler 9.96e-2 4.77e-2 2.34e-2"""
    kw = SDES[sde]
    L = 20
    x0 = R.gaussian_start(L)
    errs = []
    for N in (17, 33, 65):
        sch = scheduler(sde, True, L, N)
        assert np.array_equal(sch.G.numpy(), R.fourier_G(L))
        ts = sch.timesteps
        G64 = sch.G.numpy().astype(np.float64)
        inv_var = [torch.from_numpy((1.0 / R.gaussian_var(sde, kw, float(t), G64)).astype(np.float32)).cuda()[None, :, None]
                   for t in ts]
        x = torch.from_numpy(x0.astype(np.float32)).cuda()
        for i in range(N - 1):
            t, tn = float(ts[i]), float(ts[i + 1])
            score = -x * inv_var[i]
            if solver == "ode_euler":
                x = sch.ode_step(model_output=score, timestep=t, sample=x).prev_sample
            else:
                xp, d1 = sch.ode_heun_predict(model_output=score, timestep=t, sample=x)
                x = sch.ode_heun_correct(model_output_pred=-xp * inv_var[i + 1], timestep_next=tn, sample=x, sample_pred=xp,
                                         drift=d1).prev_sample
        errs.append(R.rel_max_err(x.cpu().numpy(), R.gaussian_exact(sde, kw, x0, 1.0, float(ts[-1]), G64)))
    want = gaussian_reference[(sde, solver)]
    print(f"gaussian {sde} {solver}: device {errs} restatement {want}")
    for e, w in zip(errs, want):
        assert abs(e - w) <= 0.02 * w, (errs, want)
    lo, hi = (3.5, 5.0) if solver == "ode_heun" else (1.8, 2.2)
    for a, b in zip(errs, errs[1:]):
        assert lo <= a / b <= hi, errs


# ------------------------------------------------------------------ 3. trajectories ----
def to_t(sd):
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


TRAJ_N = 12
_TF24 = dict(kind="transformer", d=24, H=4, NL=2)
TRAJ_MODELS = {
    "tf_d24_ragged": dict(_TF24, L=21, C=3, B=3),                                 # M = 63: ragged last 16-row tile
    "tf_d72_ecg": dict(kind="transformer", d=72, H=12, NL=2, L=187, C=1, B=4),
    "tf_c4_quad": dict(_TF24, L=20, C=4, B=3),                                    # float4 quads, M = 60
    "tf_c20_unfused": dict(_TF24, L=21, C=20, B=3),                               # C > 16: stand-alone tail
    "lstm_d16": dict(kind="lstm", d=16, H=1, NL=2, L=21, C=3, B=3),
    "mlp": dict(kind="mlp", d=8, H=1, NL=2, L=20, C=3, B=4, d_mlp=512),            # unfused by backbone
    "tf_d24_fresca": dict(_TF24, L=21, C=3, B=3, fresca=dict(low_scale=0.9, high_scale=1.2, cutoff_ratio=0.4,
                                                             cutoff_strategy="spatial")),
    "tf_d24_cache": dict(_TF24, L=21, C=3, B=3, cache=dict(K=5, R=10)),
}


def build(c, sde, fourier=True):
    """(model on the device, scheduler, state dict as CPU tensors)"""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule

    sch = scheduler(sde, fourier, c["L"])
    common = dict(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"])
    if c["kind"] == "lstm":
        m = LSTMScoreModule(fourier_noise_scaling=fourier, **common)
        sd = synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=146)
    elif c["kind"] == "mlp":
        m = MLPScoreModule(d_mlp=c["d_mlp"], **common)
        sd = synthetic.mlp_state_dict(c["C"], c["L"], c["d"], c["d_mlp"], c["NL"], seed=149)
    else:
        m = ScoreModule(fourier_noise_scaling=fourier, n_head=c["H"], **common)
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=142)
    sd = to_t(sd)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sch, sd


def oracle_score_fn(c, sd, N, table=None):
    """score_fn(x, t, k) for R.integrate: the oracle's network (+ FreSca); with the cache the gate on the predictor
    evaluations (k = 0, one global step per interval) and an empty recompute set on the corrector's (k = 1)."""
    state = {"gstep": 0}

    def fn(x, t, k):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        tt = torch.full((xt.shape[0],), t, dtype=torch.float32)
        if c["kind"] == "lstm":
            s = O.lstm_score_forward(xt, tt, sd, c["NL"])
        elif c["kind"] == "mlp":
            s = O.mlp_score_forward(xt, tt, sd, c["NL"])
        elif table is not None:
            rec = [] if k == 1 else O.gate(state["gstep"], c["L"], c["cache"]["K"], c["cache"]["R"])
            state["gstep"] += k == 0
            s = O.score_forward(xt, tt, sd, c["NL"], c["H"], table, rec)
        else:
            s = O.score_forward(xt, tt, sd, c["NL"], c["H"])
        if "fresca" in c:
            s = O.fresca(s, timestep=t, num_steps=N, **c["fresca"])
        return s.numpy()

    return fn


def sampler_for(m, c, solver, **kw):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    if "fresca" in c:
        f = c["fresca"]
        kw.update(use_fresca=True, fresca_low_scale=f["low_scale"], fresca_high_scale=f["high_scale"],
                  fresca_cutoff_ratio=f["cutoff_ratio"], fresca_cutoff_strategy=f["cutoff_strategy"])
    if "cache" in c:
        kw.update(use_cache=True, cache_kwargs=dict(c["cache"]))
    return DiffusionSampler(score_model=m, sample_batch_size=c["B"], solver=solver, **kw)


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
    ref = R.integrate(solver, sde, SDES[sde], x0, oracle_score_fn(c, sd, N, table), ts.numpy(), float(h), G.numpy(),
                      dtype=np.float32)
    err = rel_err(out, ref)
    print(f"trajectory {name} {sde} {solver}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err
    if table is not None:
        st = m._native_cache_stats()
        assert (st.recompute_count, st.cache_hit_count) == (table.recompute_count, table.cache_hit_count)
        evals = (N - 1) * (2 if solver == "ode_heun" else 1)
        assert st.recompute_count == L * c["NL"] and st.cache_hit_count == (evals - 1) * L * c["NL"]
        assert st.table_allocated == 1 and m.cache.current_step == N - 2
        k, v = m.cache_tables()
        assert rel_err(k.cpu(), table.k) < TOL_TRAJ and rel_err(v.cpu(), table.v) < TOL_TRAJ
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
    tail = lib.ffd_kernel_work(ctx.handle, _native.K_SDE, c["B"], 0, None, None)
    assert tail.startswith(b"k_unembed_ode<" + (b"heun" if solver == "ode_heun" else b"euler")), tail
    assert torch.equal(_run(m, c, solver, z0), fused)             # two identical runs: bit-identical
    assert torch.equal(_run(m, c, solver, z0, seed=1234), fused)  # no draw depends on the seed
    assert lib.ffd_tune(b"fuse_tail", 0) == 0
    plain = _run(m, c, solver, z0)
    tail = lib.ffd_kernel_work(ctx.handle, _native.K_SDE, c["B"], 0, None, None)
    assert tail.startswith(b"k_ode_step<"), tail
    assert rel_err(plain, fused) < TOL_OP


@pytest.mark.parametrize("solver", SOLVERS)
def test_philox_prior_shards_agree(ffd, solver):
    c = dict(TRAJ_MODELS["tf_d24_ragged"], B=6)
    m, sch, sd = build(c, "vp")
    full = _run(m, c, solver, rng="philox", seed=5)
    half = dict(c, B=3)
    parts = torch.cat([_run(m, half, solver, rng="philox", seed=5, sample_offset=o) for o in (0, 3)])
    assert not torch.equal(full[:3], full[3:])
    assert rel_err(parts, full) < TOL_TRAJ


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
def test_call_splitting_and_introspection(ffd, solver):
    """Intervals [0, 5) + [5, 11) in two calls equal one call of 11, bit for bit; the loop refuses what lies outside the
    grid; the FFD_K_SDE timing class counts one tail launch per score evaluation."""
    from fastfourierdiffusion_amd import _native as N

    c = TRAJ_MODELS["tf_d24_ragged"]
    m, sch, sd = build(c, "ve")
    B, L, Cn, n = c["B"], c["L"], c["C"], TRAJ_N
    sch.set_timesteps(n)
    ts_c = (C_.c_float * n)(*sch.timesteps.tolist())
    h = float(sch.step_size)
    ctx = m._ctx()
    lib, hdl = ctx.lib, ctx.handle
    code = N.FFD_SOLVER_ODE_HEUN if solver == "ode_heun" else N.FFD_SOLVER_ODE_EULER
    stream = N.current_stream_ptr(m.device)
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 77))).cuda()

    def run(x, first, count, sol=code, n_steps=n, step=h):
        return lib.ffd_sample_batch_ode(hdl, x.data_ptr(), B, ts_c, n_steps, step, first, count, sol, 0, 0, stream)

    one = x0.clone()
    assert lib.ffd_kernel_timing_begin(hdl, 1 << N.K_SDE, 64) == 0
    assert run(one, 0, n - 1) == 0
    assert lib.ffd_kernel_timing_end(hdl) == 0
    ms, launches = C_.c_float(), C_.c_int()
    assert lib.ffd_kernel_timing_get(hdl, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
    assert launches.value == (n - 1) * (2 if solver == "ode_heun" else 1)
    two = x0.clone()
    assert run(two, 0, 5) == 0 and run(two, 5, 6) == 0
    assert torch.equal(one, two) and not torch.equal(one, x0)
    # argument errors: nothing is launched, x stays as it is
    keep = two.clone()
    for bad in (dict(first=0, count=n), dict(first=6, count=6), dict(first=-1, count=2), dict(first=0, count=-1),
                dict(first=0, count=1, sol=N.FFD_SOLVER_EULER_MARUYAMA), dict(first=0, count=1, sol=7),
                dict(first=0, count=0, n_steps=1), dict(first=0, count=1, step=0.0)):
        assert run(two, **bad) == -1, bad
    assert lib.ffd_sample_batch_ode(hdl, None, B, ts_c, n, h, 0, 1, code, 0, 0, stream) == -1
    assert lib.ffd_sample_batch_ode(hdl, two.data_ptr(), B, None, n, h, 0, 1, code, 0, 0, stream) == -1
    assert lib.ffd_sample_batch_ode(hdl, two.data_ptr(), 0, ts_c, n, h, 0, 1, code, 0, 0, stream) == -1
    assert torch.equal(two, keep)


def test_cache_is_refused_on_lstm_and_mlp(ffd):
    from fastfourierdiffusion_amd import _native as N

    for name in ("lstm_d16", "mlp"):
        c = TRAJ_MODELS[name]
        m, sch, sd = build(c, "vp")
        sch.set_timesteps(TRAJ_N)
        ts_c = (C_.c_float * TRAJ_N)(*sch.timesteps.tolist())
        x = torch.zeros((c["B"], c["L"], c["C"]), device="cuda")
        ctx = m._ctx()
        rc = ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), c["B"], ts_c, TRAJ_N, float(sch.step_size), 0, 1,
                                          N.FFD_SOLVER_ODE_HEUN, 1, 0, N.current_stream_ptr(m.device))
        assert rc == -2, rc  # FFD_ERR_UNSUPPORTED


@pytest.mark.parametrize("solver", SOLVERS)
def test_reverse_diffusion_step_honours_the_solver(ffd, solver):
    """The single-step API: one interval of ``sample``'s loop; Heun makes two model calls and needs a grid point."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = TRAJ_MODELS["tf_d24_ragged"]
    m, sch, sd = build(c, "vp")
    B, L, Cn, N = c["B"], c["L"], c["C"], TRAJ_N
    sch.set_timesteps(N)
    x0 = next(synthetic.noise_stream((B, L, Cn), 1, 78))
    sampler = DiffusionSampler(m, B, solver=solver)
    i = 4
    t = sch.timesteps[i]
    batch = DiffusableBatch(X=torch.from_numpy(x0).cuda(), y=None, timesteps=torch.full((B,), float(t), device="cuda"))
    out = sampler.reverse_diffusion_step(batch)
    ref = R.integrate(solver, "vp", cases.VP, x0, oracle_score_fn(c, sd, N), sch.timesteps.numpy(), float(sch.step_size),
                      sch.G.numpy(), dtype=np.float32, first=i, n_run=1)
    assert rel_err(out.cpu(), ref) < TOL_TRAJ
    if solver == "ode_heun":
        for bad in (float(sch.timesteps[-1]), 0.123):
            batch = DiffusableBatch(X=torch.from_numpy(x0).cuda(), y=None, timesteps=torch.full((B,), bad, device="cuda"))
            with pytest.raises(ValueError):
                sampler.reverse_diffusion_step(batch)
