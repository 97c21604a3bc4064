"""GPU tests of predictor-corrector sampling: the Langevin corrector ``ffd_langevin_step`` / ``SDE.step_correct`` and the
loop ``ffd_sample_batch_pc`` / ``DiffusionSampler(corrector_steps=...)``.

1. the operator against the float64 restatement (tests/pc_restatement.py), TOL_OP, x and eps;
2. zero scores: eps = 0, the sample untouched, no NaN;
3. the Philox contract: the update regenerates the draw the norms measured;
4. bit-identity: run to run, fused / stand-alone tail, a sample alone or in a batch, one call or several;
5. n_corrector = 0 is the existing loop bit for bit;
6. whole trajectories against the oracle's score network + the fp32 restatement, TOL_TRAJ, over every tail path, LSTM,
   MLP, FreSca and the E2-CRF cache; the single-step API;
7. stationarity on the analytic Gaussian case with the device's own draws;
8. shard invariance of the "sample" norm, batch dependence of the "batch" norm.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import pc_restatement as P
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6    # a single operator, of the output's max-norm (the project's single-operator bar)
TOL_TRAJ = 1e-5  # a trajectory, of the max-norm (the project's trajectory contract)
SDES = {"vp": cases.VP, "ve": cases.VE}
NORMS = ("batch", "sample")
TAG0 = 0x80000000
SNR = 0.16


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


def correct(sch, x, s, t, norm, z=None, **kw):
    """(x', eps) of one corrector step on device tensors"""
    out, eps = sch.step_correct(s, x, SNR, t, noise=z, norm=norm, return_step_sizes=True, **kw)
    return out.prev_sample, eps


# ------------------------------------------------------------------ 1. operator ----
OP_SHAPES = [(3, 21, 1), (3, 21, 3), (3, 20, 4), (2, 187, 1), (1, 5, 1), (2, 512, 8)]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_vs_float64_restatement(ffd, sde, fourier, shape, norm):
    """Ragged rows, the quad path, fewer elements than a wave, several reduction passes (L > 256), B = 1; on the
    12-point grid VP's alpha is clamped to 0 at t = 1 (the output IS the input) and 0.086 at t = 0.5."""
    B, L, Cn = shape
    sch = scheduler(sde, fourier, L, N=12)
    h = float(sch.step_size)
    G = sch.G.numpy()
    rng = np.random.default_rng(2000 + 7 * L + Cn)
    x, s, z = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    xd, sd_, zd = (torch.from_numpy(a).cuda() for a in (x, s, z))
    for t in (1.0, 0.5, 1e-5):
        out, eps = correct(sch, xd, sd_, t, norm, zd)
        ref, eps64 = P.langevin_step(sde, SDES[sde], t, x, s, z, G, h, SNR, norm)
        if P.alpha(sde, SDES[sde], t, h) == 0.0:
            assert sde == "vp" and t == 1.0
            assert torch.equal(out, xd) and not eps.any()
            continue
        e_x = rel_err(out.cpu(), ref)
        e_eps = float(np.max(np.abs(eps.cpu().numpy().astype(np.float64) - eps64) / eps64))
        print(f"operator {sde} {shape} {norm} t={t}: x {e_x:.2e} eps {e_eps:.2e}")
        assert e_x < TOL_OP and e_eps < TOL_OP
        if norm == "batch":
            assert len(set(eps.tolist())) == 1
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(sd_.cpu(), torch.from_numpy(s))  # inputs untouched


# ------------------------------------------------------------------ 2. zero score ----
@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4)], ids=lambda s: "x".join(map(str, s)))
def test_zero_scores_leave_the_sample_alone(ffd, shape):
    B, L, Cn = shape
    sch = scheduler("ve", True, L, N=12)
    h = float(sch.step_size)
    rng = np.random.default_rng(7)
    x, s, z = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    s[1] = 0.0
    xd, sd_, zd = (torch.from_numpy(a).cuda() for a in (x, s, z))
    out, eps = correct(sch, xd, sd_, 0.5, "sample", zd)
    ref, eps64 = P.langevin_step("ve", cases.VE, 0.5, x, s, z, sch.G.numpy(), h, SNR, "sample")
    assert float(eps[1]) == 0.0 and torch.equal(out[1], xd[1])
    assert bool(torch.isfinite(out).all()) and rel_err(out.cpu(), ref) < TOL_OP and eps64[0] > 0 and eps64[2] > 0
    for seed in (None, 3):  # injected and device draws
        out, eps = correct(sch, xd, torch.zeros_like(sd_), 0.5, "batch", zd if seed is None else None,
                           **({} if seed is None else dict(seed=seed)))
        assert torch.equal(out, xd) and not eps.any()
    out, eps = correct(sch, xd, torch.zeros_like(sd_), 0.5, "sample", zd)
    assert torch.equal(out, xd) and not eps.any()


# ------------------------------------------------------------------ 3. Philox ----
def reconstruct_w(x, s, out, eps, G):
    """w = (x' - x - eps u) / sqrt(2 eps) in float64 from the device's fp32 results, (B, L, C)"""
    x, s, out = (a.cpu().numpy().astype(np.float64) for a in (x, s, out))
    e = eps.cpu().numpy().astype(np.float64)[:, None, None]
    G = np.asarray(G, np.float64)[None, :, None]
    return (out - x - e * (G * G * s)) / np.sqrt(2.0 * e)


@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4), (2, 187, 1)], ids=lambda s: "x".join(map(str, s)))
def test_update_regenerates_the_draw_the_norms_measured(ffd, shape):
    """With z = NULL, eps comes from stage 1's draw and the update from stage 3's: ||w|| reconstructed from x' must be
    the n_w that eps implies (sample norm, VE: n_w = n_u sqrt(eps / 2) / snr).  Tolerance: x' carries two fp32 roundings
    (1.2e-7 |x'|), divided by sqrt(2 eps) ~ 0.5 against |w| ~ 0.7, i.e. <~ 1e-6 of the norm; 1e-5 is held."""
    B, L, Cn = shape
    sch = scheduler("ve", True, L, N=12)
    G = sch.G.numpy().astype(np.float64)
    rng = np.random.default_rng(11)
    x, s = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(2))
    out, eps = correct(sch, x, s, 0.5, "sample", seed=9, sample_offset=3, tag=TAG0 + 5)
    w = reconstruct_w(x, s, out, eps, G)
    n_w = np.sqrt((w * w).reshape(B, -1).sum(axis=1))
    u = G[None, :, None] ** 2 * s.cpu().numpy().astype(np.float64)
    n_u = np.sqrt((u * u).reshape(B, -1).sum(axis=1))
    implied = n_u * np.sqrt(eps.cpu().numpy().astype(np.float64) / 2.0) / SNR
    print(f"philox {shape}: n_w {n_w} implied {implied}")
    assert np.max(np.abs(n_w - implied) / implied) < 1e-5
    # equal (seed, tag, sample_offset): the same draw; another tag, seed or offset: another
    again, _ = correct(sch, x, s, 0.5, "sample", seed=9, sample_offset=3, tag=TAG0 + 5)
    assert torch.equal(again, out)
    for other in (dict(seed=9, sample_offset=3, tag=TAG0 + 6), dict(seed=10, sample_offset=3, tag=TAG0 + 5),
                  dict(seed=9, sample_offset=4, tag=TAG0 + 5), dict(seed=9, sample_offset=3, tag=5)):
        o2, e2 = correct(sch, x, s, 0.5, "sample", **other)
        w2 = reconstruct_w(x, s, o2, e2, G)
        assert np.abs(w2 - w).max() > 0.1, other
    # counting is by the global sample index
    shifted, e_s = correct(sch, x, s, 0.5, "sample", seed=9, sample_offset=4, tag=TAG0 + 5)
    w_s = reconstruct_w(x, s, shifted, e_s, G)
    assert np.allclose(w_s[:-1], w[1:], atol=1e-5)  # sample b at offset 4 is sample b + 1 at offset 3


def test_device_draw_moments(ffd):
    """z = w / G over 4096 x 20 draws: mean and variance within 5 standard errors (the band of test_loss_gpu.py)."""
    shape = (4096, 20, 1)
    sch = scheduler("ve", True, 20, N=12)
    g = torch.Generator().manual_seed(1)
    x, s = (torch.randn(shape, generator=g).cuda() for _ in range(2))
    out, eps = correct(sch, x, s, 0.5, "batch", seed=21, tag=TAG0)
    z = (reconstruct_w(x, s, out, eps, sch.G.numpy()) / sch.G.numpy().astype(np.float64)[None, :, None]).ravel()
    n = z.size
    print(f"philox: mean {z.mean():+.3e} (se {n ** -0.5:.1e}), var {z.var():.5f} (se {(2 / n) ** 0.5:.1e})")
    assert abs(z.mean()) <= 5 * n ** -0.5
    assert abs(z.var() - 1.0) <= 5 * (2.0 / n) ** 0.5


# ------------------------------------------------------------------ models ----
def to_t(sd):
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


TRAJ_N = 6
_TF24 = dict(kind="transformer", d=24, H=4, NL=2)
TRAJ_MODELS = {
    "tf_d72_c1_scalar": dict(kind="transformer", d=72, H=12, NL=2, L=187, C=1, B=3),
    "tf_c4_quad": dict(_TF24, L=20, C=4, B=3),                                    # float4 quads, M = 60
    "tf_d24_ragged": dict(_TF24, L=21, C=3, B=3),                                 # M = 63: ragged last 16-row tile
    "tf_d24_unfused": dict(_TF24, L=21, C=3, B=3, fuse_tail=0),
    "lstm_d16": dict(kind="lstm", d=16, H=1, NL=2, L=21, C=3, B=3),
    "mlp": dict(kind="mlp", d=8, H=1, NL=2, L=20, C=3, B=3, d_mlp=512),
    "tf_d24_fresca": dict(_TF24, L=21, C=3, B=3, fresca=dict(low_scale=0.9, high_scale=1.2, cutoff_ratio=0.4,
                                                             cutoff_strategy="spatial")),
    "tf_d24_cache": dict(_TF24, L=21, C=3, B=3, cache=dict(K=5, R=2)),
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
    """score_fn(x, t, k) for P.pc_integrate: the oracle's network (+ FreSca); with the cache the gate on a step's first
    evaluation (k = 0, one global step per reverse step) and an empty recompute set on the later ones."""
    state = {"gstep": 0}

    def fn(x, t, k):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        tt = torch.full((xt.shape[0],), t, dtype=torch.float32)
        if c["kind"] == "lstm":
            s = O.lstm_score_forward(xt, tt, sd, c["NL"])
        elif c["kind"] == "mlp":
            s = O.mlp_score_forward(xt, tt, sd, c["NL"])
        elif table is not None:
            rec = O.gate(state["gstep"], c["L"], c["cache"]["K"], c["cache"]["R"]) if k == 0 else []
            state["gstep"] += k == 0
            s = O.score_forward(xt, tt, sd, c["NL"], c["H"], table, rec)
        else:
            s = O.score_forward(xt, tt, sd, c["NL"], c["H"])
        if "fresca" in c:
            s = O.fresca(s, timestep=t, num_steps=N, **c["fresca"])
        return s.numpy()

    return fn


def sampler_for(m, c, **kw):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    if "fresca" in c:
        f = c["fresca"]
        kw.update(use_fresca=True, fresca_low_scale=f["low_scale"], fresca_high_scale=f["high_scale"],
                  fresca_cutoff_ratio=f["cutoff_ratio"], fresca_cutoff_strategy=f["cutoff_strategy"])
    if "cache" in c:
        kw.update(use_cache=True, cache_kwargs=dict(c["cache"]))
    return DiffusionSampler(score_model=m, sample_batch_size=c["B"], **kw)


def draws(c, n_corr, seed, N=TRAJ_N):
    """the prior's draw, then n_corr + 1 per step"""
    return list(synthetic.noise_stream((c["B"], c["L"], c["C"]), 1 + N * (n_corr + 1), seed))


def stepwise(m, c, sampler, zs, N=TRAJ_N):
    """The same trajectory through the single-step API, the cache driven as the reference's loop drives it."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    sch = m.noise_scheduler
    sch.set_timesteps(N)
    sampler.inject_noise(zs)
    X = sampler.sample_prior(c["B"])
    if "cache" in c:
        m.cache.reset()
    for j in range(N):
        rec = None
        if "cache" in c:
            m.cache.current_step = j
            rec = set(O.gate(j, c["L"], c["cache"]["K"], c["cache"]["R"]))
        batch = DiffusableBatch(X=X, y=None, timesteps=torch.full((c["B"],), float(sch.timesteps[j]), device="cuda"))
        X = sampler.reverse_diffusion_step(batch, step=j, recompute_tokens=rec)
    return X.cpu()


# ------------------------------------------------------------------ 6. trajectories ----
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("n_corr", [1, 2])
@pytest.mark.parametrize("name", sorted(TRAJ_MODELS))
def test_trajectory_vs_oracle(ffd, name, n_corr, norm):
    """VE (alpha = 1: every corrector step moves x); the VP clamp has its own case below."""
    _trajectory(name, "ve", n_corr, norm)


@pytest.mark.parametrize("norm", NORMS)
def test_trajectory_vs_oracle_vp(ffd, norm):
    """VP on 6 points: alpha = 0 for t >= 0.4 (inert correctors, x untouched), 0.18 at t = 0.2, 0.98 at t = 1e-5."""
    _trajectory("tf_d24_ragged", "vp", 2, norm)


def _trajectory(name, sde, n_corr, norm):
    from fastfourierdiffusion_amd import _native

    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, sde)
    B, L, Cn, N = c["B"], c["L"], c["C"], TRAJ_N
    if "fuse_tail" in c:
        assert _native.lib().ffd_tune(b"fuse_tail", c["fuse_tail"]) == 0
    zs = draws(c, n_corr, 900 + len(name))
    sampler = sampler_for(m, c, corrector_steps=n_corr, snr=SNR, corrector_norm=norm)
    sampler.inject_noise(zs)
    out = sampler.sample(num_samples=B, num_diffusion_steps=N)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu"
    tail = _native.lib().ffd_kernel_work(m._ctx().handle, _native.K_SDE, B, 0, None, None)
    fusable = c["kind"] != "mlp" and "fresca" not in c and c.get("fuse_tail", 1)
    assert tail.startswith(b"k_unembed_mfma<sde> + k_lv_" if fusable else b"k_sde_step + k_lv_"), tail

    ts, h = O.timesteps(N)
    G = O.noise_scaling(L, True)
    x0 = O.prior(torch.from_numpy(zs[0]), G, SDES[sde]["sigma_max"] if sde == "ve" else None).numpy()
    table = O.KVTable(c["NL"], L) if "cache" in c else None
    ref = P.pc_integrate(sde, SDES[sde], x0, oracle_score_fn(c, sd, N, table), lambda i, k: zs[1 + i * (n_corr + 1) + k],
                         ts.numpy(), float(h), G.numpy(), n_corr, SNR, norm, dtype=np.float32)
    err = rel_err(out, ref)
    print(f"trajectory {name} {sde} n_corr={n_corr} {norm}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err
    kept = None
    if table is not None:
        st = m._native_cache_stats()
        assert (st.recompute_count, st.cache_hit_count) == (table.recompute_count, table.cache_hit_count)
        evals = N * (n_corr + 1)  # the first evaluation of step 0 recomputes everything, every other one is a pure hit
        assert st.recompute_count == L * c["NL"] and st.cache_hit_count == (evals - 1) * L * c["NL"]
        assert st.table_allocated == 1 and m.cache.current_step == N - 1
        k, v = m.cache_tables()
        assert rel_err(k.cpu(), table.k) < TOL_TRAJ and rel_err(v.cpu(), table.v) < TOL_TRAJ
        kept = (k.cpu(), v.cpu(), m.cache.crf_cache.cpu())
    # the single-step API: the same model calls (ffd_score_forward_cached sizes gate(j), then 0s) in the same order
    single = stepwise(m, c, sampler, zs)
    err = rel_err(single, out)
    print(f"  reverse_diffusion_step: rel err {err:.3e}")
    assert err < TOL_TRAJ, err
    if kept is not None:
        st2 = m._native_cache_stats()
        assert (st2.recompute_count, st2.cache_hit_count) == (table.recompute_count, table.cache_hit_count)
        k, v = m.cache_tables()
        assert rel_err(k.cpu(), kept[0]) < TOL_TRAJ and rel_err(v.cpu(), kept[1]) < TOL_TRAJ
        assert rel_err(m.cache.crf_cache.cpu(), kept[2]) < TOL_TRAJ  # captured from the step's FIRST evaluation
        m.disable_caching()


# ------------------------------------------------------------------ 4. bit-identity ----
def _run(m, c, zs=None, **kw):
    s = sampler_for(m, c, **kw)
    if zs is not None:
        s.inject_noise(zs)
    return s.sample(num_samples=c["B"], num_diffusion_steps=TRAJ_N)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_c4_quad", "tf_d72_c1_scalar"])
def test_runs_repeat_and_fused_tail_equals_standalone_tail(ffd, name, norm):
    from fastfourierdiffusion_amd import _native

    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, "ve")
    lib = _native.lib()
    kw = dict(corrector_steps=2, snr=SNR, corrector_norm=norm)
    zs = draws(c, 2, 31)
    res = {}
    for fuse in (1, 0):
        assert lib.ffd_tune(b"fuse_tail", fuse) == 0
        res[(fuse, "inject")] = _run(m, c, zs, **kw)
        res[(fuse, "philox")] = _run(m, c, rng="philox", seed=5, **kw)
        assert torch.equal(_run(m, c, zs, **kw), res[(fuse, "inject")])
        assert torch.equal(_run(m, c, rng="philox", seed=5, **kw), res[(fuse, "philox")])
    for how in ("inject", "philox"):
        assert bool(torch.isfinite(res[(1, how)]).all())
        assert torch.equal(res[(1, how)], res[(0, how)]), how
    assert not torch.equal(res[(1, "inject")], res[(1, "philox")])
    assert not torch.equal(_run(m, c, rng="philox", seed=6, **kw), res[(1, "philox")])


@pytest.mark.parametrize("shape", [(5, 20, 4), (5, 21, 3), (5, 187, 1)], ids=lambda s: "x".join(map(str, s)))
def test_sample_norm_does_not_depend_on_the_batch(ffd, shape):
    """Sample b alone (B = 1, sample_offset = b) against sample b inside B = 5: eps and x' bit for bit, with injected
    and with device draws.  Offsets 1 .. 3 are no multiple of 4; at (21, 3) the element offset 63 b is none either and
    a sample's first Philox block straddles its neighbour."""
    B, L, Cn = shape
    sch = scheduler("ve", True, L, N=12)
    rng = np.random.default_rng(13)
    x, s, z = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(3))
    full_i, eps_i = correct(sch, x, s, 0.5, "sample", z)
    full_p, eps_p = correct(sch, x, s, 0.5, "sample", seed=4, tag=TAG0 + 1)
    for b in range(B):
        one = slice(b, b + 1)
        o, e = correct(sch, x[one].contiguous(), s[one].contiguous(), 0.5, "sample", z[one].contiguous())
        assert torch.equal(o[0], full_i[b]) and float(e[0]) == float(eps_i[b]), b
        o, e = correct(sch, x[one].contiguous(), s[one].contiguous(), 0.5, "sample", seed=4, sample_offset=b, tag=TAG0 + 1)
        assert torch.equal(o[0], full_p[b]) and float(e[0]) == float(eps_p[b]), b
    # a misaligned view of the same data takes the scalar kernels: the same bits
    pad = torch.empty(s.numel() + 1, device="cuda")
    o, e = correct(sch, x, pad[1:].view(shape).copy_(s), 0.5, "sample", z)
    assert torch.equal(o, full_i) and torch.equal(e, eps_i)


def _pc_call(m, sch, x, first, count, n_corr, norm, z=None, n_steps=TRAJ_N, snr=SNR, step=None, seed=9, off=5, B=None,
             cache=0):
    from fastfourierdiffusion_amd import _native as N

    ctx = m._ctx()
    ts_c = (C_.c_float * len(sch.timesteps))(*sch.timesteps.tolist())
    return ctx.lib.ffd_sample_batch_pc(ctx.handle, x.data_ptr() if x is not None else None, x.shape[0] if B is None else B,
                                       ts_c, n_steps, float(sch.step_size) if step is None else step, first, count, n_corr,
                                       snr, norm, seed, off, z.data_ptr() if z is not None else None, cache, 0,
                                       N.current_stream_ptr(m.device))


@pytest.mark.parametrize("norm", [0, 1], ids=NORMS)
def test_call_splitting_errors_and_introspection(ffd, norm):
    """Steps [0, 2) + [2, 3) + [3, 6) in three calls equal one call of 6, bit for bit, with device and with injected draws;
    the FFD_K_SDE timing class counts one entry per score evaluation; argument errors launch nothing."""
    from fastfourierdiffusion_amd import _native as N

    c = TRAJ_MODELS["tf_d24_ragged"]
    m, sch, sd = build(c, "ve")
    B, L, Cn, n = c["B"], c["L"], c["C"], TRAJ_N
    sch.set_timesteps(n)
    ctx = m._ctx()
    lib, hdl = ctx.lib, ctx.handle
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 77))).cuda()
    zs = torch.from_numpy(np.stack(list(synthetic.noise_stream((B, L, Cn), n * 3, 78)))).cuda()  # (n, 3, B, L, C) flat
    for z in (None, zs):
        one = x0.clone()
        assert lib.ffd_kernel_timing_begin(hdl, 1 << N.K_SDE, 64) == 0
        assert _pc_call(m, sch, one, 0, n, 2, norm, z) == 0
        assert lib.ffd_kernel_timing_end(hdl) == 0
        ms, launches = C_.c_float(), C_.c_int()
        assert lib.ffd_kernel_timing_get(hdl, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
        assert launches.value == n * 3
        two = x0.clone()
        for first, count in ((0, 2), (2, 1), (3, 3)):
            assert _pc_call(m, sch, two, first, count, 2, norm, None if z is None else z[first * 3:]) == 0
        assert torch.equal(one, two) and not torch.equal(one, x0) and bool(torch.isfinite(one).all())
    keep = two.clone()
    for bad in (dict(first=0, count=n + 1), dict(first=4, count=3), dict(first=-1, count=2), dict(first=0, count=-1),
                dict(first=0, count=1, n_corr=-1), dict(first=0, count=1, snr=0.0), dict(first=0, count=1, snr=-0.1),
                dict(first=0, count=1, norm=2), dict(first=0, count=1, norm=-1), dict(first=0, count=1, step=0.0),
                dict(first=0, count=0, n_steps=0), dict(first=0, count=1, B=0),
                dict(first=0, count=0, n_corr=0x40000000, n_steps=6)):  # 6 * 2^30 tags do not fit below 2^31
        args = dict(n_corr=2, norm=norm)
        args.update(bad)
        assert _pc_call(m, sch, two, **args) == -1, bad
    assert _pc_call(m, sch, None, 0, 1, 2, norm, B=B) == -1
    assert torch.equal(two, keep)
    for name in ("lstm_d16", "mlp"):  # the cache is the transformer's
        c2 = TRAJ_MODELS[name]
        m2, sch2, _ = build(c2, "ve")
        sch2.set_timesteps(n)
        x = torch.zeros((c2["B"], c2["L"], c2["C"]), device="cuda")
        assert _pc_call(m2, sch2, x, 0, 1, 1, norm, cache=1) in (-2, -3), name  # FFD_ERR_UNSUPPORTED, or _STATE: never enabled


# ------------------------------------------------------------------ 5. n_corrector = 0 ----
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_c4_quad", "tf_d24_cache", "lstm_d16"])
def test_no_corrector_is_the_existing_loop(ffd, name):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = TRAJ_MODELS[name]
    m, sch, sd = build(c, "vp")
    B, L, Cn, n = c["B"], c["L"], c["C"], TRAJ_N
    zs = draws(c, 0, 41)
    base = dict(use_cache=True, cache_kwargs=dict(c["cache"])) if "cache" in c else {}
    for kw in (dict(), dict(rng="philox", seed=8, sample_offset=3)):
        outs = []
        for extra in (dict(), dict(corrector_steps=0, snr=0.3, corrector_norm="sample")):
            s = DiffusionSampler(m, B, **base, **kw, **extra)
            if not kw:
                s.inject_noise(zs)
            outs.append(s.sample(B, n))
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    if "cache" in c:
        m.disable_caching()
    sch.set_timesteps(n)
    ctx = m._ctx()
    ts_c = (C_.c_float * n)(*sch.timesteps.tolist())
    x0 = torch.from_numpy(zs[0]).cuda()
    z = torch.from_numpy(np.stack(zs[1:])).cuda()
    for zz in (None, z):
        a, b = x0.clone(), x0.clone()
        assert ctx.lib.ffd_sample_batch(ctx.handle, a.data_ptr(), B, ts_c, n, float(sch.step_size), 0, n, 9, 5,
                                        zz.data_ptr() if zz is not None else None, 0, 0, N.current_stream_ptr(m.device)) == 0
        assert _pc_call(m, sch, b, 0, n, 0, 0, zz) == 0
        assert torch.equal(a, b) and not torch.equal(a, x0)


def test_plain_entry_is_the_shared_loop_under_every_option(ffd):
    """ffd_sample_batch, ffd_sample_batch_pc(n_corrector = 0) and ffd_sample_batch_cond(cond = NULL) with the cache
    (K = 5, R = 2), the CRF capture (``last`` every 2nd step, a 2-slot ring every step: step 4 goes to both) and FreSca all
    on: the state, both capture buffers and the cache statistics agree bit for bit, with device and with injected draws,
    under fuse_tail 1 and 0; steps [0, 2) + [2, 3) + [3, 6) equal one call of 6; FFD_K_SDE counts one launch per step."""
    from fastfourierdiffusion_amd import _native as N

    c = dict(_TF24, L=21, C=3, B=3)
    m, sch, sd = build(c, "vp")
    m.enable_caching(K=5, R=2)
    B, L, Cn, n = c["B"], c["L"], c["C"], TRAJ_N
    sch.set_timesteps(n)
    ctx = m._ctx()
    lib, hdl, stream = ctx.lib, ctx.handle, N.current_stream_ptr(m.device)
    ts_c = (C_.c_float * n)(*sch.timesteps.tolist())
    h = float(sch.step_size)
    fresca = N.FrescaCfg(0.9, 1.2, 0.4, 0, n)
    assert lib.ffd_fresca_enable(hdl, C_.byref(fresca)) == 0
    crf_shape = (c["NL"], L, c["d"])
    last = torch.empty(crf_shape, device="cuda")
    ring = torch.empty((2,) + crf_shape, device="cuda")
    cap = N.CrfCaptureCfg(ring.data_ptr(), 2, 1, last.data_ptr(), 2, 0)
    assert lib.ffd_cache_crf_capture(hdl, C_.byref(cap)) == 0
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 77))).cuda()
    zs = torch.from_numpy(np.stack(list(synthetic.noise_stream((B, L, Cn), n, 78)))).cuda()

    def ptr(t):
        return t.data_ptr() if t is not None else None

    entries = {
        "plain": lambda x, first, count, z: lib.ffd_sample_batch(hdl, x.data_ptr(), B, ts_c, n, h, first, count, 9, 5, ptr(z),
                                                                 1, first, stream),
        "pc": lambda x, first, count, z: lib.ffd_sample_batch_pc(hdl, x.data_ptr(), B, ts_c, n, h, first, count, 0, SNR, 0, 9,
                                                                 5, ptr(z), 1, first, stream),
        "cond": lambda x, first, count, z: lib.ffd_sample_batch_cond(hdl, x.data_ptr(), B, ts_c, n, h, first, count, 0, SNR,
                                                                     0, 9, 5, ptr(z), 1, first, None, stream),
    }

    def run(entry, z, cuts, count_launches=False):
        """(state, last, ring, statistics) after the calls [cuts[k], cuts[k + 1]) from a reset cache"""
        assert lib.ffd_cache_reset(hdl) == 0
        last.fill_(float("nan"))
        ring.fill_(float("nan"))
        x = x0.clone()
        if count_launches:
            assert lib.ffd_kernel_timing_begin(hdl, 1 << N.K_SDE, 64) == 0
        for first, end in zip(cuts[:-1], cuts[1:]):
            assert entries[entry](x, first, end - first, None if z is None else z[first:]) == 0
        if count_launches:
            assert lib.ffd_kernel_timing_end(hdl) == 0
            ms, launches = C_.c_float(), C_.c_int()
            assert lib.ffd_kernel_timing_get(hdl, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
            assert launches.value == n
        st = N.CacheStats()
        assert lib.ffd_cache_stats_get(hdl, C_.byref(st)) == 0
        return x, last.clone(), ring.clone(), (st.recompute_count, st.cache_hit_count, st.current_step, st.table_allocated)

    def same(a, b):
        return all(torch.equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]

    res = {}
    for fuse in (1, 0):
        assert lib.ffd_tune(b"fuse_tail", fuse) == 0
        for how, z in (("philox", None), ("inject", zs)):
            one = run("plain", z, (0, n), count_launches=True)
            assert all(bool(torch.isfinite(t).all()) for t in one[:3]) and not torch.equal(one[0], x0)
            # the gate recomputes every token at global step 0 and none at steps 1..5 (the periodic refresh is 500 apart)
            assert one[3] == (L * c["NL"], (n - 1) * L * c["NL"], n - 1, 1), one[3]
            for entry in entries:
                assert same(one, run(entry, z, (0, n))), (fuse, how, entry)
                assert same(one, run(entry, z, (0, 2, 3, n))), (fuse, how, entry, "split")
            res[(fuse, how)] = one
    for how in ("philox", "inject"):  # (FreSca reads the whole score: both settings take the stand-alone tail)
        assert same(res[(1, how)], res[(0, how)]), how
    assert not torch.equal(res[(1, "philox")][0], res[(1, "inject")][0])


# ------------------------------------------------------------------ 7. stationarity ----
# tests/test_pc_host.py RECORDED_BAND (the restatement's 8-seed min / max), widened on each side by its own width: a
# wrong factor 2 (0.52 / 2.02 VE, 0.58 / 1.62 VP) or a wrong power of G (0.75 / 0.82) stays outside, another RNG inside
STATIONARY_BAND = {"ve": (1.0182 - 0.0129, 1.0311 + 0.0129), "vp": (0.9942 - 0.0166, 1.0108 + 0.0166)}


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_stationary_on_the_gaussian_case_with_device_draws(ffd, sde):
    kw = SDES[sde]
    L, n = P.GAUSS_L, P.GAUSS_SAMPLES
    sch = scheduler(sde, True, L, N=P.GAUSS_N)
    assert np.array_equal(sch.G.numpy(), P.fourier_G(L))
    var = P.gaussian_var(sde, kw, P.GAUSS_T, sch.G.numpy().astype(np.float64))
    var_d = torch.from_numpy(var.astype(np.float32)).cuda()[None, :, None]
    inv_var = torch.from_numpy((1.0 / var).astype(np.float32)).cuda()[None, :, None]
    g = torch.Generator().manual_seed(17)
    x = torch.randn((n, L, 1), generator=g).cuda() * var_d.sqrt()
    for k in range(P.GAUSS_STEPS):
        x = sch.step_correct(-x * inv_var, x, P.GAUSS_SNR, P.GAUSS_T, norm="batch", seed=23, tag=TAG0 + k).prev_sample
    ratio = float(((x.double() ** 2).mean(dim=(0, 2)).cpu().numpy() / var).mean())
    lo, hi = STATIONARY_BAND[sde]
    print(f"stationarity {sde}: variance ratio {ratio:.4f} (band {lo:.4f} .. {hi:.4f})")
    assert lo <= ratio <= hi, ratio


# ------------------------------------------------------------------ 8. shards ----
def test_sample_norm_is_shard_invariant_batch_norm_is_not(ffd):
    c = dict(TRAJ_MODELS["tf_d24_ragged"], B=4)
    m, sch, sd = build(c, "ve")
    half = dict(c, B=2)
    kw = dict(corrector_steps=2, snr=SNR, rng="philox", seed=5)
    full = _run(m, c, corrector_norm="sample", **kw)
    parts = torch.cat([_run(m, half, corrector_norm="sample", sample_offset=o, **kw) for o in (0, 2)])
    assert not torch.equal(full[:2], full[2:])
    err = rel_err(parts, full)
    print(f"shards, sample norm: rel err {err:.3e}")
    assert err < TOL_TRAJ
    full_b = _run(m, c, corrector_norm="batch", **kw)
    parts_b = torch.cat([_run(m, half, corrector_norm="batch", sample_offset=o, **kw) for o in (0, 2)])
    err_b = rel_err(parts_b, full_b)
    print(f"shards, batch norm: rel err {err_b:.3e}")
    assert err_b > TOL_TRAJ  # beyond rounding: the step size is a batch statistic
    # the noise itself: a shard's corrector draws are the whole batch's, bit for bit (and so are eps and x')
    shape = (4, 21, 3)
    sch2 = scheduler("ve", True, 21, N=12)
    rng = np.random.default_rng(3)
    x, s = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(2))
    whole, eps = correct(sch2, x, s, 0.5, "sample", seed=5, sample_offset=0, tag=TAG0 + 7)
    w = reconstruct_w(x, s, whole, eps, sch2.G.numpy())
    for o in (0, 2):
        part, e = correct(sch2, x[o:o + 2].contiguous(), s[o:o + 2].contiguous(), 0.5, "sample", seed=5, sample_offset=o,
                          tag=TAG0 + 7)
        assert torch.equal(part, whole[o:o + 2]) and torch.equal(e, eps[o:o + 2])
        assert np.array_equal(reconstruct_w(x[o:o + 2], s[o:o + 2], part, e, sch2.G.numpy()), w[o:o + 2])
