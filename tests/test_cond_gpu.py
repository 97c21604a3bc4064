"""GPU tests of conditional sampling by replacement: the operator ``ffd_cond_project`` / ``SDE.cond_project`` and the loop
``ffd_sample_batch_cond`` / ``DiffusionSampler.sample_conditional`` / ``impute``.

1. the frequency-domain operator against the float64 restatement (tests/cond_restatement.py), bar: max(TOL_OP, 3 x the
   error of the same composite in fp32 on the CPU);   2. the time-domain operator, TOL_OP;
3. exact cases (mask 0, noiseless mask 1, observed points);   4. independence of the fill at unobserved points;
5. the Philox contract and shard invariance;   6. bit-identity;   7. the unconditional paths are what they were;
8. whole trajectories against the oracle's score network + the fp32 restatement, TOL_TRAJ;
9. the analytic Gaussian case with the device's own draws;   10. ``impute`` end to end.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import cond_restatement as R
import ode_restatement as ODE
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O
from test_cond_host import RECORDED_BAND
from test_pc_gpu import (SNR, TRAJ_MODELS, _TF24, _tune_defaults, build, ffd, oracle_score_fn, sampler_for,  # noqa: F401
                         scheduler)

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6    # a single operator, of the output's max-norm (the project's single-operator bar)
TOL_TRAJ = 1e-5  # a trajectory, of the max-norm (the project's trajectory contract)
SDES = {"vp": cases.VP, "ve": cases.VE}
TAG0 = R.TAG0
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def masks(shape, rng):
    """random 0/1, a prefix, one fractional"""
    B, L, Cn = shape
    prefix = np.zeros(shape, np.float32)
    prefix[:, :max(1, L // 2)] = 1.0
    return {"random": (rng.random(shape) < 0.5).astype(np.float32), "prefix": prefix,
            "fractional": rng.random(shape).astype(np.float32)}


# ---- the same composite in fp32 on the CPU (torch.fft): what fp32 arithmetic costs on these inputs ----
def _unpack(xf):
    L = xf.shape[1]
    n_re = L // 2 + 1
    im = torch.zeros_like(xf[:, :n_re])
    im[:, 1:1 + (L - n_re)] = xf[:, n_re:]
    return torch.complex(xf[:, :n_re], im)


def _pack(X, L):
    return torch.cat([X.real, X.imag[:, 1:(L + 1) // 2]], dim=1)


def cpu_fp32_composite(sde, t, x, obs, mask, z, G, std, noiseless):
    mc, sigma = R.coefficients(sde, SDES[sde], t, noiseless)
    x, obs, mask, z = (torch.from_numpy(np.asarray(a, np.float32)) for a in (x, obs, mask, z))
    L = x.shape[1]
    y = obs if noiseless else np.float32(mc) * obs + (np.float32(sigma) * torch.from_numpy(G)[None, :, None]) * z
    d = y - x
    if std is not None:
        d = d * torch.from_numpy(std)[None]
    w = torch.fft.irfft(_unpack(d), n=L, dim=1, norm="ortho")
    X = _pack(torch.fft.rfft(mask * w, dim=1, norm="ortho"), L)
    if std is not None:
        X = X / torch.from_numpy(std)[None]
    return (x + X).numpy()


# ------------------------------------------------------------------ 1. operator ----
OP_SHAPES = [(1, 2, 1), (1, 5, 1), (3, 21, 1), (3, 21, 3), (3, 20, 4), (2, 187, 1), (1, 1031, 2), (2, 16, 4), (2, 64, 3),
             (2, 512, 8), (1, 4096, 3)]


@pytest.mark.parametrize("shape", OP_SHAPES, ids=ids)
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_vs_float64_restatement(ffd, sde, fourier, shape):
    """std given / NULL x obs_batch 1 / B x t in {1, 0.5, 1e-5} and noiseless, injected z; the three masks rotate over the
    16 settings.  The composite chains two transforms, so its bar is measured: the same composite in fp32 on the CPU
    (torch.fft) against float64, times 3 because the summation orders differ, and never below TOL_OP."""
    B, L, Cn = shape
    sch = scheduler(sde, fourier, L)
    G = sch.G.numpy()
    rng = np.random.default_rng(3000 + 7 * L + Cn)
    x, z, series = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    std = rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32)
    mk = masks(shape, rng)
    xd, zd = dev(x), dev(z)
    kept, worst, n = [], (0.0, 0.0), 0
    for sd in (std, None):
        for ob in (1, B):
            for t, noiseless in ((1.0, False), (0.5, False), (1e-5, False), (0.5, True)):
                name = ("random", "prefix", "fractional")[n % 3]
                n += 1
                mask = mk[name][:ob]
                obs = R.dft(series[:ob] * mask, np.float32) if sd is None else (R.dft(series[:ob] * mask) / sd).astype(np.float32)
                od, md, sdd = dev(obs), dev(mask), (dev(sd) if sd is not None else None)
                out = sch.cond_project(xd, od, md, t, std=sdd, noise=zd, noiseless=noiseless).prev_sample
                ref = R.project(sde, SDES[sde], t, x, obs, mask, z, G, sd, noiseless=noiseless)
                e_dev = rel_err(out.cpu(), ref)
                e_cpu = rel_err(cpu_fp32_composite(sde, t, x, obs, mask, z, G, sd, noiseless), ref)
                worst = max(worst, (e_dev, e_cpu))
                assert e_dev <= max(TOL_OP, 3.0 * e_cpu), (name, sd is not None, ob, t, noiseless, e_dev, e_cpu)
                kept.append((od, obs, md, mask, sdd, sd))
    print(f"operator {sde} {'fourier' if fourier else 'unit'} {shape}: device {worst[0]:.2e}, CPU fp32 {worst[1]:.2e}")
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(zd.cpu(), torch.from_numpy(z))  # inputs untouched
    for od, obs, md, mask, sdd, sd in kept:
        assert torch.equal(od.cpu(), torch.from_numpy(obs)) and torch.equal(md.cpu(), torch.from_numpy(mask))
        assert sdd is None or torch.equal(sdd.cpu(), torch.from_numpy(sd))


# ------------------------------------------------------------------ 2. time domain ----
@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4), (1, 1, 1)], ids=ids)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_time_domain_operator(ffd, sde, shape):
    B, L, Cn = shape
    sch = scheduler(sde, False, L)
    rng = np.random.default_rng(4000 + L)
    x, z, obs = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    for name, mask in masks(shape, rng).items():
        for ob in (1, B):
            for t, noiseless in ((1.0, False), (0.5, False), (1e-5, False), (0.5, True)):
                out = sch.cond_project(dev(x), dev(obs[:ob]), dev(mask[:ob]), t, domain="time", noise=dev(z),
                                       noiseless=noiseless).prev_sample
                ref = R.project(sde, SDES[sde], t, x, obs[:ob], mask[:ob], z, sch.G.numpy(), domain="time",
                                noiseless=noiseless)
                assert rel_err(out.cpu(), ref) < TOL_OP, (name, ob, t, noiseless)


# ------------------------------------------------------------------ 3. exact cases ----
EXACT_SHAPES = [(3, 21, 3), (3, 20, 4), (2, 16, 4), (2, 64, 3)]


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=ids)
def test_zero_mask_leaves_the_state_alone(ffd, shape):
    B, L, Cn = shape
    sch = scheduler("ve", True, L)
    rng = np.random.default_rng(5)
    x, z, obs = (dev(rng.standard_normal(shape)) for _ in range(3))
    zero = torch.zeros_like(x)
    std = dev(rng.uniform(0.5, 2.0, (L, Cn)))
    for domain in ("frequency", "time"):
        for kw in (dict(noise=z), dict(seed=3, sample_offset=2), dict(noiseless=True)):
            for sd in ((std, None) if domain == "frequency" else (None,)):
                out = sch.cond_project(x, obs, zero, 0.5, std=sd, domain=domain, **kw).prev_sample
                assert torch.equal(out, x), (domain, kw.keys())


@pytest.mark.parametrize("shape", EXACT_SHAPES + [(2, 187, 1)], ids=ids)
def test_noiseless_replacement_returns_the_observation(ffd, shape):
    """mask 1: the observation itself; a 0/1 mask: idft of the result is the observed series at the observed points and
    idft(x) at the others.  Bar of section 1 (the CPU's fp32 error of the same composite)."""
    B, L, Cn = shape
    sch = scheduler("ve", False, L)
    G = sch.G.numpy()
    rng = np.random.default_rng(6)
    x, series = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    obs = R.dft(series, np.float32)
    ones = np.ones(shape, np.float32)
    out = sch.cond_project(dev(x), dev(obs), dev(ones), 0.5, noiseless=True).prev_sample.cpu().numpy()
    bar = max(TOL_OP, 3.0 * rel_err(cpu_fp32_composite("ve", 0.5, x, obs, ones, x, G, None, True), obs.astype(np.float64)))
    assert rel_err(out, obs) <= bar
    mask = (rng.random(shape) < 0.5).astype(np.float32)
    obs_m = R.dft(series * mask, np.float32)
    out = sch.cond_project(dev(x), dev(obs_m), dev(mask), 0.5, noiseless=True).prev_sample.cpu().numpy()
    want = np.where(mask == 1, series.astype(np.float64), R.idft(x))
    bar = max(TOL_OP, 3.0 * rel_err(R.idft(cpu_fp32_composite("ve", 0.5, x, obs_m, mask, x, G, None, True)), want))
    assert rel_err(R.idft(out), want) <= bar


# ------------------------------------------------------------------ 4. fill independence ----
@pytest.mark.parametrize("shape", EXACT_SHAPES + [(2, 187, 1)], ids=ids)
def test_fill_at_unobserved_points_does_not_matter(ffd, shape):
    B, L, Cn = shape
    sch = scheduler("vp", True, L)
    rng = np.random.default_rng(8)
    x, z, series, f1, f2 = (rng.standard_normal(shape).astype(np.float32) for _ in range(5))
    mask = (rng.random(shape) < 0.5).astype(np.float32)
    std = rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32)
    outs, cpus = [], []
    for fill in (f1, f2):
        obs = (R.dft(series * mask + fill * (1 - mask)) / std).astype(np.float32)
        outs.append(sch.cond_project(dev(x), dev(obs), dev(mask), 0.5, std=dev(std), noise=dev(z)).prev_sample.cpu().numpy())
        cpus.append((cpu_fp32_composite("vp", 0.5, x, obs, mask, z, sch.G.numpy(), std, False),
                     R.project("vp", cases.VP, 0.5, x, obs, mask, z, sch.G.numpy(), std)))
    bar = max(TOL_OP, 3.0 * max(rel_err(a, b) for a, b in cpus))
    e = rel_err(outs[0], outs[1])
    print(f"fill independence {shape}: {e:.2e} (bar {bar:.2e})")
    assert e <= bar


# ------------------------------------------------------------------ 5. Philox ----
def sde_step_draw(sch, shape, seed, offset, tag):
    """the draw ffd_sde_step's stream gives: VE, x = 0, score = 0: x' = sqrt(h) (cs G) z"""
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn = shape
    x, s = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    desc = sch._desc()
    h = 0.25
    assert N.lib().ffd_sde_step(C_.byref(desc), x.data_ptr(), s.data_ptr(), sch._G_on(x.device).data_ptr(), 0.5, h, None, seed,
                                offset, tag, B, L, Cn, N.current_stream_ptr(x.device)) == 0
    _, cs = ODE.coefficients("ve", cases.VE, 0.5)
    return x.cpu().numpy().astype(np.float64) / (np.sqrt(h) * cs * sch.G.numpy().astype(np.float64)[None, :, None])


@pytest.mark.parametrize("domain", R.DOMAINS)
@pytest.mark.parametrize("shape", [(4, 21, 3), (4, 20, 4), (2, 187, 1), (2, 16, 4), (2, 64, 3)], ids=ids)
def test_device_draws_are_the_sde_step_stream_and_shard_invariant(ffd, shape, domain):
    """mask 1, x = obs = 0 (VE): the output is sigma G z up to the transforms' rounding, so z can be read off it; it is
    the draw ffd_sde_step makes under the same (seed, tag, offset)."""
    B, L, Cn = shape
    sch = scheduler("ve", True, L)
    G = sch.G.numpy().astype(np.float64)[None, :, None]
    _, sigma = R.coefficients("ve", cases.VE, 0.5)
    zero, ones = torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda")
    seed, off, tag = 9, 3, 7
    out = sch.cond_project(zero, zero, ones, 0.5, domain=domain, seed=seed, sample_offset=off, tag=tag).prev_sample
    z = out.cpu().numpy().astype(np.float64) / (float(np.float32(sigma)) * G)
    want = sde_step_draw(sch, shape, seed, off, tag)
    assert np.abs(want).max() > 2.0
    if domain == "time":
        # no transform: out = (sigma G) z, two fp32 roundings, against ffd_sde_step's sqrt(h) ((cs G) z), h = 1/4, two
        # roundings and cs rounded to fp32: a few 2^-24 of each draw, whatever its size
        assert np.all(np.abs(z - want) <= 1e-6 * np.abs(want)), (np.abs(z - want) / np.abs(want)).max()
    else:  # the two transforms add their rounding, relative to the slab's max-norm (|z| up to ~4)
        assert np.abs(z - want).max() < 2e-5, np.abs(z - want).max()
    for other in (dict(seed=10, sample_offset=off, tag=tag), dict(seed=seed, sample_offset=off + 1, tag=tag),
                  dict(seed=seed, sample_offset=off, tag=TAG0)):
        o2 = sch.cond_project(zero, zero, ones, 0.5, domain=domain, **other).prev_sample
        assert (o2 - out).abs().max() > 0.1 * float(sigma)
    # a shard draws what the unsharded call draws: bit for bit with a real state, observation and mask
    rng = np.random.default_rng(12)
    x, obs, mask = dev(rng.standard_normal(shape)), dev(rng.standard_normal(shape)), dev(rng.random(shape) < 0.5)
    whole = sch.cond_project(x, obs, mask, 0.5, domain=domain, seed=seed, sample_offset=off, tag=TAG0 + 4).prev_sample
    h = B // 2
    for o in (0, h):
        part = sch.cond_project(x[o:o + h].contiguous(), obs[o:o + h].contiguous(), mask[o:o + h].contiguous(), 0.5,
                                domain=domain, seed=seed, sample_offset=off + o, tag=TAG0 + 4).prev_sample
        assert torch.equal(part, whole[o:o + h])


# ------------------------------------------------------------------ 6. bit-identity ----
@pytest.mark.parametrize("shape", [(5, 21, 3), (5, 20, 4), (5, 187, 1), (5, 16, 4), (5, 64, 3)], ids=ids)
def test_operator_repeats_and_a_sample_does_not_depend_on_its_batch(ffd, shape):
    B, L, Cn = shape
    sch = scheduler("vp", True, L)
    rng = np.random.default_rng(13)
    x, z, obs = (dev(rng.standard_normal(shape)) for _ in range(3))
    mask, std = dev(rng.random(shape) < 0.5), dev(rng.uniform(0.5, 2.0, (L, Cn)))
    for ob in (1, B):
        o_, m_ = obs[:ob].contiguous(), mask[:ob].contiguous()
        full_i = sch.cond_project(x, o_, m_, 0.5, std=std, noise=z).prev_sample
        full_p = sch.cond_project(x, o_, m_, 0.5, std=std, seed=4, tag=TAG0 + 1).prev_sample
        assert torch.equal(sch.cond_project(x, o_, m_, 0.5, std=std, noise=z).prev_sample, full_i)  # run to run
        assert torch.equal(sch.cond_project(x, o_, m_, 0.5, std=std, seed=4, tag=TAG0 + 1).prev_sample, full_p)
        for b in range(B):
            one = slice(b, b + 1)
            ob1, mb1 = (o_, m_) if ob == 1 else (o_[one].contiguous(), m_[one].contiguous())
            o = sch.cond_project(x[one].contiguous(), ob1, mb1, 0.5, std=std, noise=z[one].contiguous()).prev_sample
            assert torch.equal(o[0], full_i[b]), (ob, b)
            o = sch.cond_project(x[one].contiguous(), ob1, mb1, 0.5, std=std, seed=4, sample_offset=b, tag=TAG0 + 1).prev_sample
            assert torch.equal(o[0], full_p[b]), (ob, b)
    # a misaligned view of the same data takes the scalar kernels: the same bits
    pad = torch.empty(z.numel() + 1, device="cuda")
    o = sch.cond_project(x, obs, mask, 0.5, std=std, noise=pad[1:].view(shape).copy_(z)).prev_sample
    assert torch.equal(o, sch.cond_project(x, obs, mask, 0.5, std=std, noise=z).prev_sample)


COND_N = 12
COND_MODELS = dict(TRAJ_MODELS, tf_pow2_quad=dict(_TF24, L=16, C=4, B=3))


def cond_inputs(c, seed, per_sample=False, std=True):
    """(obs (1 | B, L, C) in the diffused domain, prefix mask, std or None) as fp32 numpy"""
    rng = np.random.default_rng(seed)
    n = c["B"] if per_sample else 1
    series = rng.standard_normal((n, c["L"], c["C"])).astype(np.float32)
    mask = np.zeros_like(series)
    mask[:, :(2 * c["L"]) // 3] = 1.0
    sd = rng.uniform(0.5, 2.0, (c["L"], c["C"])).astype(np.float32) if std else None
    return series, mask, sd


def _cond_call(m, sch, x, first, count, n_corr, cfg, z=None, n_steps=COND_N, seed=9, off=5, norm=0, B=None):
    from fastfourierdiffusion_amd import _native as N

    ctx = m._ctx()
    ts_c = (C_.c_float * len(sch.timesteps))(*sch.timesteps.tolist())
    return ctx.lib.ffd_sample_batch_cond(ctx.handle, x.data_ptr(), x.shape[0] if B is None else B, ts_c, n_steps,
                                         float(sch.step_size), first, count, n_corr, SNR, norm, seed, off,
                                         z.data_ptr() if z is not None else None, 0, 0,
                                         C_.byref(cfg) if cfg is not None else None, N.current_stream_ptr(m.device))


@pytest.mark.parametrize("domain", [0, 1], ids=R.DOMAINS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_pow2_quad"])
def test_loop_repeats_splits_and_fused_tail_equals_standalone_tail(ffd, name, domain):
    """One call of 12 steps against [0, 5) + [5, 6) + [6, 12), device and injected draws, final_replace on; the fused
    predictor tail against the stand-alone one; the FFD_K_SDE class counts every update and every projection; argument
    errors launch nothing."""
    from fastfourierdiffusion_amd import _native as N

    c = COND_MODELS[name]
    m, sch, sd = build(c, "ve")
    B, L, Cn, n = c["B"], c["L"], c["C"], COND_N
    sch.set_timesteps(n)
    lib, hdl = m._ctx().lib, m._ctx().handle
    series, mask, std = cond_inputs(c, 21, std=domain == 0)
    obs = series if domain == 1 else (R.dft(series * mask) / std).astype(np.float32)
    od, md, sdd = dev(obs), dev(mask), (dev(std) if std is not None else None)
    cfg = N.CondCfg(od.data_ptr(), md.data_ptr(), sdd.data_ptr() if sdd is not None else None, 1, domain, 1, 0)
    x0 = dev(next(synthetic.noise_stream((B, L, Cn), 1, 77)))
    zs = dev(np.stack(list(synthetic.noise_stream((B, L, Cn), n * 4, 78))))  # (n, 2, 2, B, L, C) flat
    res = {}
    for fuse in (1, 0):
        assert lib.ffd_tune(b"fuse_tail", fuse) == 0
        for how, z in (("philox", None), ("inject", zs)):
            one = x0.clone()
            assert lib.ffd_kernel_timing_begin(hdl, 1 << N.K_SDE, 128) == 0
            assert _cond_call(m, sch, one, 0, n, 1, cfg, z) == 0
            assert lib.ffd_kernel_timing_end(hdl) == 0
            ms, launches = C_.c_float(), C_.c_int()
            assert lib.ffd_kernel_timing_get(hdl, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
            assert launches.value == n * 4 + 1  # per step 2 updates + 2 projections; the final replacement
            again = x0.clone()
            assert _cond_call(m, sch, again, 0, n, 1, cfg, z) == 0
            two = x0.clone()
            for first, count in ((0, 5), (5, 1), (6, 6)):
                assert _cond_call(m, sch, two, first, count, 1, cfg, None if z is None else z[first * 4:]) == 0
            assert torch.equal(one, again) and torch.equal(one, two) and bool(torch.isfinite(one).all())
            res[(fuse, how)] = one
    for how in ("philox", "inject"):
        assert torch.equal(res[(1, how)], res[(0, how)]), how
    assert not torch.equal(res[(1, "philox")], res[(1, "inject")])
    keep = two.clone()
    bad_cfgs = [N.CondCfg(None, md.data_ptr(), None, 1, domain, 1, 0), N.CondCfg(od.data_ptr(), None, None, 1, domain, 1, 0),
                N.CondCfg(od.data_ptr(), md.data_ptr(), None, 2, domain, 1, 0), N.CondCfg(od.data_ptr(), md.data_ptr(), None, 1, 2, 1, 0),
                N.CondCfg(od.data_ptr(), md.data_ptr(), md.data_ptr(), 1, 1, 1, 0), N.CondCfg(two.data_ptr(), md.data_ptr(), None, 1, domain, 1, 0),
                N.CondCfg(od.data_ptr(), two.data_ptr(), None, 1, domain, 1, 0)]
    for bad in bad_cfgs:
        assert _cond_call(m, sch, two, 0, 1, 1, bad) == -1
    for bad in (dict(first=0, count=n + 1), dict(first=-1, count=2), dict(first=0, count=1, n_corr=-1),
                dict(first=0, count=1, norm=2), dict(first=0, count=1, B=0), dict(first=0, count=1, z=two),
                dict(first=0, count=0, n_corr=0x15555555)):  # 12 * (n_corr + 1) tags do not fit below 2^30
        args = dict(n_corr=1, cfg=cfg)
        args.update(bad)
        assert _cond_call(m, sch, two, **args) == -1, bad
    assert torch.equal(two, keep)


def test_loop_refuses_a_length_outside_the_frequency_domain_set(ffd):
    """The model's L = 4100 is past the projection's 4096: FFD_ERR_UNSUPPORTED before any launch (x is left as it is),
    after the FFD_ERR_INVALID checks."""
    from fastfourierdiffusion_amd import _native as N

    c = dict(kind="lstm", d=16, H=1, NL=1, L=4100, C=1, B=1)
    m, sch, sd = build(c, "ve")
    sch.set_timesteps(COND_N)
    x = dev(np.random.default_rng(1).standard_normal((1, 4100, 1)))
    keep = x.clone()
    obs, mask = torch.zeros_like(x), torch.zeros_like(x)
    cfg = N.CondCfg(obs.data_ptr(), mask.data_ptr(), None, 1, N.FFD_COND_FREQUENCY, 1, 0)
    assert _cond_call(m, sch, x, 0, 1, 0, cfg) == -2
    assert _cond_call(m, sch, x, 0, 1, 0, N.CondCfg(None, mask.data_ptr(), None, 1, N.FFD_COND_FREQUENCY, 1, 0)) == -1
    assert torch.equal(x, keep)


# ------------------------------------------------------------------ 7. unchanged paths ----
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_c4_quad", "lstm_d16"])
def test_unconditional_paths_are_what_they_were(ffd, name):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from test_pc_gpu import _pc_call

    c = COND_MODELS[name]
    m, sch, sd = build(c, "vp")
    B, L, Cn, n = c["B"], c["L"], c["C"], 6
    sch.set_timesteps(n)
    x0 = dev(next(synthetic.noise_stream((B, L, Cn), 1, 41)))
    for n_corr in (0, 2):
        z = dev(np.stack(list(synthetic.noise_stream((B, L, Cn), n * (n_corr + 1), 42))))
        for zz in (None, z):  # cond == NULL is ffd_sample_batch_pc
            a, b = x0.clone(), x0.clone()
            assert _pc_call(m, sch, a, 0, n, n_corr, 0, zz, n_steps=n) == 0
            assert _cond_call(m, sch, b, 0, n, n_corr, None, zz, n_steps=n) == 0
            assert torch.equal(a, b) and not torch.equal(a, x0)
    zero = torch.zeros(L, Cn)
    for n_corr in (0, 1):  # an all-zero mask adds exact zeros after every update
        for domain in R.DOMAINS:
            kw = dict(rng="philox", seed=8, sample_offset=3, corrector_steps=n_corr, snr=SNR)
            base = DiffusionSampler(m, B, **kw).sample(B, n)
            got = DiffusionSampler(m, B, **kw).sample_conditional(torch.randn(L, Cn), zero, B, n, domain=domain,
                                                                  final_replace=False)
            assert torch.equal(base, got) and bool(torch.isfinite(base).all()), (n_corr, domain)


# ------------------------------------------------------------------ 8. trajectories ----
TRAJ = [(name, n_corr, "frequency", n_corr == 1)
        for name in ("tf_d24_ragged", "tf_d24_unfused", "tf_c4_quad", "tf_pow2_quad", "lstm_d16", "mlp", "tf_d24_fresca",
                     "tf_d24_cache") for n_corr in (0, 1)]
TRAJ += [("tf_d24_ragged", 1, "time", True), ("tf_c4_quad", 0, "time", False), ("lstm_d16", 1, "time", False),
         ("tf_d72_c1_scalar", 0, "frequency", True)]


@pytest.mark.parametrize("name,n_corr,domain,final", TRAJ, ids=lambda v: str(v))
def test_trajectory_vs_oracle(ffd, monkeypatch, name, n_corr, domain, final):
    """12 steps, VE, injected draws: per update its own draw, then its projection's.  Frequency domain: the observation
    is per sample with std when there is a corrector, shared without std otherwise."""
    from fastfourierdiffusion_amd import _native
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = COND_MODELS[name]
    sde = "ve"
    m, sch, sd = build(c, sde)
    B, L, Cn, N = c["B"], c["L"], c["C"], COND_N
    if "fuse_tail" in c:
        assert _native.lib().ffd_tune(b"fuse_tail", c["fuse_tail"]) == 0
    series, mask, std = cond_inputs(c, 60 + len(name), per_sample=n_corr == 1, std=domain == "frequency" and n_corr == 1)
    obs = series if domain == "time" else R.dft(series * mask)
    obs = (obs / std if std is not None else obs).astype(np.float32)
    zs = list(synthetic.noise_stream((B, L, Cn), 1 + N * (n_corr + 1) * 2, 950 + len(name)))
    kw = dict(corrector_steps=n_corr, snr=SNR)
    call = dict(domain=domain, final_replace=final, feature_std=torch.from_numpy(std) if std is not None else None)
    sampler = sampler_for(m, c, **kw)
    sampler.inject_noise(zs)
    o_t, m_t = (torch.from_numpy(a if n_corr == 1 else a[0]) for a in (obs, mask))
    out = sampler.sample_conditional(o_t, m_t[:, :1] if n_corr == 0 else m_t, B, N, **call)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu"

    ts, h = O.timesteps(N)
    G = O.noise_scaling(L, True)
    x0 = O.prior(torch.from_numpy(zs[0]), G, SDES[sde]["sigma_max"]).numpy()
    table = O.KVTable(c["NL"], L) if "cache" in c else None
    ref = R.cond_integrate(sde, SDES[sde], x0, oracle_score_fn(c, sd, N, table),
                           lambda i, k, p: zs[1 + (i * (n_corr + 1) + k) * 2 + p], ts.numpy(), float(h), G.numpy(), n_corr, SNR,
                           obs, mask, std, domain, final, dtype=np.float32)
    err = rel_err(out, ref)
    print(f"trajectory {name} n_corr={n_corr} {domain} final={final}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err
    if table is not None:
        st = m._native_cache_stats()
        assert (st.recompute_count, st.cache_hit_count) == (table.recompute_count, table.cache_hit_count)
    if n_corr == 0:  # the single-step API: cond_project after reverse_diffusion_step (whose predictor draws randn_like)
        sch.set_timesteps(N)
        sampler.inject_noise(zs)
        monkeypatch.setattr(torch, "randn_like", lambda like: sampler._next_injected(like.shape, like.device))
        X = sampler.sample_prior(B)
        if "cache" in c:
            m.cache.reset()
        od, md = dev(obs), dev(mask)
        for j in range(N):
            rec = None
            if "cache" in c:
                m.cache.current_step = j
                rec = set(O.gate(j, L, c["cache"]["K"], c["cache"]["R"]))
            t = float(sch.timesteps[j])
            X = sampler.reverse_diffusion_step(DiffusableBatch(X=X, y=None, timesteps=torch.full((B,), t, device="cuda")),
                                               step=j, recompute_tokens=rec)
            X = sch.cond_project(X, od, md, t, domain=domain, noise=sampler._next_injected(X.shape, X.device)).prev_sample
        if final:
            X = sch.cond_project(X, od, md, float(sch.timesteps[-1]), domain=domain, noiseless=True).prev_sample
        err = rel_err(X.cpu(), out)
        print(f"  single-step API: rel err {err:.3e}")
        assert err < TOL_TRAJ, err
    if "cache" in c:
        m.disable_caching()


# ------------------------------------------------------------------ 9. analytic case ----
@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_analytic_gaussian_case_with_device_draws(ffd, sde):
    """White data (tests/cond_restatement.py): 4096 samples conditioned on a prefix of a fixed series, 150 steps with one
    corrector.  The margin is the PC stationarity test's: the float64 restatement's recorded 8-seed band
    (tests/test_cond_host.py), widened on each side by its own width."""
    from fastfourierdiffusion_amd.utils.fourier import idft

    kw = SDES[sde]
    L, n, N = R.GAUSS_L, R.GAUSS_SAMPLES, R.GAUSS_STEPS
    sch = scheduler(sde, True, L, N=N)
    G64 = sch.G.numpy().astype(np.float64)
    series, mask = R.gaussian_series(L)
    obs, md = dev(R.dft(series * mask)), dev(mask)
    g = torch.Generator().manual_seed(17)
    Gd = sch.G.cuda()[None, :, None]
    x = torch.randn((n, L, 1), generator=g).cuda() * Gd * (kw["sigma_max"] if sde == "ve" else 1.0)
    torch.manual_seed(18)
    for i in range(N):
        t = float(sch.timesteps[i])
        inv_var = dev(1.0 / R.white_var(sde, kw, t, G64))[None, :, None]
        x = sch.step_correct(-x * inv_var, x, R.GAUSS_SNR, t, norm="batch", seed=23, tag=0x80000000 + i).prev_sample
        x = sch.cond_project(x, obs, md, t, seed=23, tag=TAG0 + 2 * i).prev_sample
        x = sch.step(-x * inv_var, t, x).prev_sample
        x = sch.cond_project(x, obs, md, t, seed=23, tag=TAG0 + 2 * i + 1).prev_sample
    x = sch.cond_project(x, obs, md, float(sch.timesteps[-1]), noiseless=True).prev_sample
    xt = idft(x).cpu().numpy().astype(np.float64)
    ratio, worst = R.unobserved_stats(xt, mask)
    lo, hi = RECORDED_BAND[sde]
    lo, hi = lo - (hi - lo), hi + (hi - lo)
    seen = xt[:, :R.GAUSS_PREFIX]
    e_obs = float(np.abs(seen - series[:, :R.GAUSS_PREFIX]).max() / np.abs(xt).max())
    print(f"analytic {sde}: variance ratio {ratio:.4f} (band {lo:.4f} .. {hi:.4f}), worst mean {worst:.2f} se, observed {e_obs:.2e}")
    assert e_obs <= TOL_OP  # the operator bar
    assert lo <= ratio <= hi, ratio
    assert worst < 5.0, worst


# ------------------------------------------------------------------ 10. impute ----
def test_impute_end_to_end(ffd):
    """(2, 187, 1) with dataset statistics, a forecast (prefix mask): time-domain series come back, the observed points
    reproduced.  Four chained transforms of at most TOL_OP each: TOL_TRAJ of the max-norm is held."""
    c = dict(TRAJ_MODELS["tf_d72_c1_scalar"], B=2)
    m, sch, sd = build(c, "vp")
    B, L, Cn = 2, 187, 1
    rng = np.random.default_rng(31)
    series = torch.from_numpy(rng.standard_normal((B, L, Cn)).astype(np.float32))
    mean = torch.from_numpy(rng.standard_normal((L, Cn)).astype(np.float32))
    std = torch.from_numpy(rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32))
    mask = torch.zeros(L)
    mask[:100] = 1.0
    sampler = sampler_for(m, c, rng="philox", seed=3, corrector_steps=1, snr=SNR)
    out = sampler.impute(series, mask, B, 6, feature_mean=mean, feature_std=std)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu" and bool(torch.isfinite(out).all())
    err = float((out[:, :100] - series[:, :100]).abs().max() / out.abs().max())
    print(f"impute: observed points {err:.2e} of the max-norm; unobserved spread {float(out[:, 100:].std()):.3f}")
    assert err < TOL_TRAJ
    assert float((out[:, 100:] - series[:, 100:]).abs().max()) > 1e-3  # the rest is sampled, not copied
    again = sampler_for(m, c, rng="philox", seed=3, corrector_steps=1, snr=SNR).impute(series, mask, B, 6, feature_mean=mean,
                                                                                     feature_std=std)
    assert torch.equal(out, again)
    plain = sampler_for(m, c, rng="philox", seed=3).impute(series[0], mask, B, 6)  # one series, no statistics
    assert tuple(plain.shape) == (B, L, Cn)
    assert float((plain[:, :100] - series[:1, :100]).abs().max() / plain.abs().max()) < TOL_TRAJ
