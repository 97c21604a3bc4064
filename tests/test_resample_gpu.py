"""GPU tests of resampled conditional sampling: the operator ``ffd_forward_transition`` / ``SDE.forward_transition`` and
the loop ``ffd_sample_batch_resample`` / ``DiffusionSampler.sample_conditional(resample=, jump=)`` / ``impute``.

1. the operator against the float64 restatement (tests/resample_restatement.py), injected and device draws, TOL_OP;
2. exact cases: s == t, run to run, alone / in a batch, shards, ``ffd_sde_step``'s stream, scalar == float4 kernel;
3. the loop: ``resample=1`` is ``ffd_sample_batch_cond``, every split point of a U = 12 run, launches, argument errors;
4. whole trajectories against the oracle's score network + the fp32 restatement, TOL_TRAJ;
5. the analytic white-data case through the public sampler;   6. the two-mode forecast;   7. ``impute`` end to end.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import resample_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O
from test_cond_gpu import COND_MODELS, cond_inputs, dev, sde_step_draw
from test_pc_gpu import SNR, _tune_defaults, build, ffd, oracle_score_fn, sampler_for, scheduler  # noqa: F401
from test_resample_host import RESAMPLED_WHITE_BAND, TWO_MODE_BAND

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6    # a single operator, of the output's max-norm (the project's single-operator bar)
TOL_TRAJ = 1e-5  # a trajectory, of the max-norm (the project's trajectory contract)
SDES = {"vp": cases.VP, "ve": cases.VE}
TAG0 = R.TAG0
CR = R.CR
ids = lambda s: "x".join(map(str, s))  # noqa: E731
# (s, t): from 0 (the marginal), inside the grid, a short hop next to eps, the whole range
TIMES = [(0.0, 1.0), (0.25, 0.5), (1e-5, 0.2), (0.8, 0.8000001), (1e-5, 1.0)]


# ------------------------------------------------------------------ 1. operator ----
OP_SHAPES = [(3, 187, 1), (2, 64, 4), (3, 5, 3), (1, 1, 1)]  # scalar; float4; scalar at an odd element offset; one element


@pytest.mark.parametrize("shape", OP_SHAPES, ids=ids)
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_vs_float64_restatement(ffd, sde, fourier, shape):
    """Injected z, and device draws at sample_offset 1 (element offset L C: 15 for (3, 5, 3), odd) read back from
    ``ffd_sde_step``'s stream as tests/test_cond_gpu.py reads them."""
    B, L, Cn = shape
    sch = scheduler(sde, fourier, L)
    G = sch.G.numpy()
    rng = np.random.default_rng(7000 + 7 * L + Cn)
    x, z = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    xd, zd = dev(x), dev(z)
    seed, off, tag = 11, 1, TAG0 + 3
    z_dev = sde_step_draw(scheduler("ve", fourier, L), shape, seed, off, tag)
    worst = [0.0, 0.0]
    for s, t in TIMES:
        out = sch.forward_transition(xd, s, t, noise=zd).prev_sample
        e = rel_err(out.cpu(), R.forward_transition(sde, SDES[sde], s, t, x, z, G))
        out = sch.forward_transition(xd, s, t, seed=seed, sample_offset=off, tag=tag).prev_sample
        e_dev = rel_err(out.cpu(), R.forward_transition(sde, SDES[sde], s, t, x, z_dev, G))
        worst = [max(worst[0], e), max(worst[1], e_dev)]
        assert e < TOL_OP and e_dev < TOL_OP, (s, t, e, e_dev)
    print(f"transition {sde} {'fourier' if fourier else 'unit'} {shape}: injected {worst[0]:.2e}, device draws {worst[1]:.2e}")
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(zd.cpu(), torch.from_numpy(z))  # inputs untouched


# ------------------------------------------------------------------ 2. exact cases ----
@pytest.mark.parametrize("shape", OP_SHAPES + [(5, 20, 4)], ids=ids)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_operator_exact_cases(ffd, sde, shape):
    B, L, Cn = shape
    sch = scheduler(sde, True, L)
    rng = np.random.default_rng(21)
    x, z = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    x.flat[0] = -0.0
    xd, zd = dev(x), dev(z)
    # s == t: bit-identical, the sign of a zero included, whatever the draw
    for kw in (dict(noise=zd), dict(seed=3, sample_offset=2)):
        for t in (0.0, 1e-5, 0.5, 1.0):
            out = sch.forward_transition(xd, t, t, **kw).prev_sample
            assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32)), (kw.keys(), t)
    s, t = 0.25, 0.5
    full_i = sch.forward_transition(xd, s, t, noise=zd).prev_sample
    full_p = sch.forward_transition(xd, s, t, seed=4, sample_offset=3, tag=TAG0 + 1).prev_sample
    assert not torch.equal(full_i, xd) and not torch.equal(full_p, full_i)
    assert torch.equal(sch.forward_transition(xd, s, t, noise=zd).prev_sample, full_i)  # run to run
    assert torch.equal(sch.forward_transition(xd, s, t, seed=4, sample_offset=3, tag=TAG0 + 1).prev_sample, full_p)
    for b in range(B):  # alone against in a batch; a shard draws what the whole call draws
        one = slice(b, b + 1)
        o = sch.forward_transition(xd[one].contiguous(), s, t, noise=zd[one].contiguous()).prev_sample
        assert torch.equal(o[0], full_i[b]), b
        o = sch.forward_transition(xd[one].contiguous(), s, t, seed=4, sample_offset=3 + b, tag=TAG0 + 1).prev_sample
        assert torch.equal(o[0], full_p[b]), b
    h = B // 2
    if h:
        for o in (0, h):
            part = sch.forward_transition(xd[o:o + h].contiguous(), s, t, seed=4, sample_offset=3 + o, tag=TAG0 + 1).prev_sample
            assert torch.equal(part, full_p[o:o + h])
    for other in (dict(seed=5, sample_offset=3, tag=TAG0 + 1), dict(seed=4, sample_offset=4, tag=TAG0 + 1),
                  dict(seed=4, sample_offset=3, tag=TAG0 + 2)):
        assert not torch.equal(sch.forward_transition(xd, s, t, **other).prev_sample, full_p)
    # a misaligned view of the same draws takes the scalar kernel: the same bits
    pad = torch.empty(zd.numel() + 1, device="cuda")
    assert torch.equal(sch.forward_transition(xd, s, t, noise=pad[1:].view(shape).copy_(zd)).prev_sample, full_i)


@pytest.mark.parametrize("shape", [(4, 21, 3), (4, 20, 4), (2, 187, 1)], ids=ids)
def test_device_draws_are_the_sde_step_stream(ffd, shape):
    """x = 0 (VE): the output is (sg G) z, two fp32 roundings, against ffd_sde_step's sqrt(h) ((cs G) z): a few 2^-24 of
    each draw, whatever its size (the bar of tests/test_cond_gpu.py's time-domain case)."""
    B, L, Cn = shape
    sch = scheduler("ve", True, L)
    G = sch.G.numpy().astype(np.float64)[None, :, None]
    _, sg = R.transition_coefficients("ve", cases.VE, 0.25, 0.5)
    seed, off, tag = 9, 3, 7
    out = sch.forward_transition(torch.zeros(shape, device="cuda"), 0.25, 0.5, seed=seed, sample_offset=off, tag=tag).prev_sample
    z = out.cpu().numpy().astype(np.float64) / (float(np.float32(sg)) * G)
    want = sde_step_draw(sch, shape, seed, off, tag)
    assert np.abs(want).max() > 2.0
    assert np.all(np.abs(z - want) <= 1e-6 * np.abs(want)), (np.abs(z - want) / np.abs(want)).max()


# ------------------------------------------------------------------ 3. the loop ----
LOOP_N = 6


def _res_call(m, sch, x, first, count, n_corr, cfg, z=None, n_steps=LOOP_N, jump=2, resample=2, seed=9, off=5, norm=0,
              B=None):
    from fastfourierdiffusion_amd import _native as N

    ctx = m._ctx()
    ts_c = (C_.c_float * len(sch.timesteps))(*sch.timesteps.tolist())
    return ctx.lib.ffd_sample_batch_resample(ctx.handle, x.data_ptr(), x.shape[0] if B is None else B, ts_c, n_steps,
                                             float(sch.step_size), first, count, jump, resample, n_corr, SNR, norm, seed, off,
                                             z.data_ptr() if z is not None else None,
                                             C_.byref(cfg) if cfg is not None else None, N.current_stream_ptr(m.device))


def _loop_setup(name, domain, sde="ve"):
    from fastfourierdiffusion_amd import _native as N

    c = COND_MODELS[name]
    m, sch, sd = build(c, sde)
    sch.set_timesteps(LOOP_N)
    series, mask, std = cond_inputs(c, 21, std=domain == 0)
    obs = series if domain == 1 else (CR.dft(series * mask) / std).astype(np.float32)
    keep = (dev(obs), dev(mask), dev(std) if std is not None else None)
    cfg = N.CondCfg(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr() if std is not None else None, 1, domain, 1, 0)
    return c, m, sch, cfg, keep


@pytest.mark.parametrize("domain", [0, 1], ids=CR.DOMAINS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_pow2_quad", "lstm_d16"])
def test_resample_1_is_the_conditional_loop_bit_for_bit(ffd, name, domain):
    from test_cond_gpu import _cond_call

    c, m, sch, cfg, keep = _loop_setup(name, domain)
    shape = (c["B"], c["L"], c["C"])
    x0 = dev(next(synthetic.noise_stream(shape, 1, 77)))
    for n_corr in (0, 1):
        zs = dev(np.stack(list(synthetic.noise_stream(shape, LOOP_N * (n_corr + 1) * 2, 78))))
        for z in (None, zs):
            for jump in (1, 4, 9):
                a, b = x0.clone(), x0.clone()
                assert _cond_call(m, sch, a, 0, LOOP_N, n_corr, cfg, z, n_steps=LOOP_N) == 0
                assert _res_call(m, sch, b, 0, LOOP_N, n_corr, cfg, z, jump=jump, resample=1) == 0
                assert torch.equal(a, b) and not torch.equal(a, x0) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("domain", [0, 1], ids=CR.DOMAINS)
@pytest.mark.parametrize("name", ["tf_d24_ragged", "tf_pow2_quad"])
def test_loop_splits_launches_and_argument_errors(ffd, name, domain):
    """N = 6, r = 2, j = 2: U = 12 visits, 3 transitions.  Every split point [0, p) + [p, 12) against the one call,
    device and injected draws (the slab pointer of a call starts at its first visit); the FFD_K_SDE class counts every
    update, projection and transition and the final replacement; argument errors launch nothing."""
    from fastfourierdiffusion_amd import _native as N

    c, m, sch, cfg, keep = _loop_setup(name, domain)
    lib, hdl = m._ctx().lib, m._ctx().handle
    shape = (c["B"], c["L"], c["C"])
    n_corr, U = 1, 12
    assert lib.ffd_host_resample_visits(LOOP_N, 2, 2) == U
    x0 = dev(next(synthetic.noise_stream(shape, 1, 77)))
    total = R.n_slabs(LOOP_N, 2, 2, n_corr)
    assert total == U * 4 + 3
    zs = dev(np.stack(list(synthetic.noise_stream(shape, total, 79))))
    res = {}
    for how, z in (("philox", None), ("inject", zs)):
        one = x0.clone()
        assert lib.ffd_kernel_timing_begin(hdl, 1 << N.K_SDE, 128) == 0
        assert _res_call(m, sch, one, 0, U, n_corr, cfg, z) == 0
        assert lib.ffd_kernel_timing_end(hdl) == 0
        ms, launches = C_.c_float(), C_.c_int()
        assert lib.ffd_kernel_timing_get(hdl, N.K_SDE, C_.byref(ms), C_.byref(launches)) == 0
        assert launches.value == U * 4 + 3 + 1
        again = x0.clone()
        assert _res_call(m, sch, again, 0, U, n_corr, cfg, z) == 0
        assert torch.equal(one, again) and bool(torch.isfinite(one).all())
        for p in range(0, U + 1):  # (p = 0 and p = U: an empty call on either side)
            two = x0.clone()
            assert _res_call(m, sch, two, 0, p, n_corr, cfg, z) == 0
            z2 = None if z is None or p == U else z[R.n_slabs(LOOP_N, 2, 2, n_corr, 0, p):]
            assert _res_call(m, sch, two, p, U - p, n_corr, cfg, z2) == 0
            assert torch.equal(one, two), (how, p)
        res[how] = one
    assert not torch.equal(res["philox"], res["inject"])
    plain = x0.clone()  # resampling changes the result
    assert _res_call(m, sch, plain, 0, LOOP_N, n_corr, cfg, None, resample=1) == 0
    assert not torch.equal(plain, res["philox"])
    # fused predictor tail against the stand-alone one
    assert lib.ffd_tune(b"fuse_tail", 0) == 0
    unfused = x0.clone()
    assert _res_call(m, sch, unfused, 0, U, n_corr, cfg, None) == 0
    assert torch.equal(unfused, res["philox"])
    two = res["inject"].clone()
    keep_x = two.clone()
    od, md = keep[0], keep[1]
    bad_cfgs = [None, N.CondCfg(None, md.data_ptr(), None, 1, domain, 1, 0), N.CondCfg(od.data_ptr(), None, None, 1, domain, 1, 0),
                N.CondCfg(od.data_ptr(), md.data_ptr(), None, 2, domain, 1, 0), N.CondCfg(od.data_ptr(), md.data_ptr(), None, 1, 2, 1, 0),
                N.CondCfg(two.data_ptr(), md.data_ptr(), None, 1, domain, 1, 0)]
    for bad in bad_cfgs:  # cond == NULL is refused: resampling an unconditional sampler buys nothing
        assert _res_call(m, sch, two, 0, 1, 1, bad) == -1
    for bad in (dict(first=0, count=U + 1), dict(first=-1, count=2), dict(first=U, count=1), dict(first=7, count=6),
                dict(first=0, count=-1), dict(first=0, count=1, jump=0), dict(first=0, count=1, resample=0),
                dict(first=0, count=1, jump=-2), dict(first=0, count=1, n_corr=-1), dict(first=0, count=1, norm=2),
                dict(first=0, count=1, B=0), dict(first=0, count=1, z=two), dict(first=0, count=LOOP_N + 1, resample=1),
                dict(first=0, count=0, n_corr=0x1FFFFFF0 // U)):  # 12 * (n_corr + 1) tags reach 0xE0000000
        args = dict(n_corr=1, cfg=cfg)
        args.update(bad)
        assert _res_call(m, sch, two, **args) == -1, bad
    assert _res_call(m, sch, two, 0, 0, 0x1FFFFFF0 // U - 1, cfg) == 0  # the largest corrector count that fits
    assert torch.equal(two, keep_x)


# ------------------------------------------------------------------ 4. trajectories ----
TRAJ = [(name, "ve", n_corr, domain, r, j)
        for name in ("tf_d24_ragged", "tf_d24_unfused", "lstm_d16")
        for n_corr in (0, 1) for domain in CR.DOMAINS for r, j in ((2, 1), (2, 2), (3, 4), (2, 9))]
TRAJ += [("tf_c4_quad", "ve", 1, "frequency", 2, 2), ("tf_c4_quad", "ve", 0, "time", 3, 4),
         ("tf_pow2_quad", "ve", 1, "frequency", 3, 4)]
# VP: the transition's a < 1 inside the loop (VE has a = 1), over every (r, j), both domains, with and without a corrector
TRAJ += [("tf_d24_ragged", "vp", n_corr, domain, r, j)
         for n_corr in (0, 1) for domain in CR.DOMAINS for r, j in ((2, 1), (2, 2), (3, 4), (2, 9))]
TRAJ += [("tf_d24_unfused", "vp", 1, "frequency", 2, 2), ("lstm_d16", "vp", 0, "time", 3, 4),
         ("lstm_d16", "vp", 1, "frequency", 2, 9), ("tf_c4_quad", "vp", 1, "frequency", 2, 1)]


@pytest.mark.parametrize("name,sde,n_corr,domain,r,j", TRAJ, ids=lambda v: str(v))
def test_trajectory_vs_oracle(ffd, name, sde, n_corr, domain, r, j):
    """6 steps, VE and VP, injected draws in execution order (per visit each update's draw and its projection's, then the
    transition's), the public sampler against the fp32 restatement driving the oracle's network."""
    from fastfourierdiffusion_amd import _native

    c = COND_MODELS[name]
    m, sch, sd = build(c, sde)
    B, L, Cn, N = c["B"], c["L"], c["C"], LOOP_N
    if "fuse_tail" in c:
        assert _native.lib().ffd_tune(b"fuse_tail", c["fuse_tail"]) == 0
    series, mask, std = cond_inputs(c, 60 + len(name), per_sample=n_corr == 1, std=domain == "frequency" and n_corr == 1)
    obs = series if domain == "time" else CR.dft(series * mask)
    obs = (obs / std if std is not None else obs).astype(np.float32)
    zs = list(synthetic.noise_stream((B, L, Cn), 1 + R.n_slabs(N, j, r, n_corr), 950 + len(name)))
    sampler = sampler_for(m, c, corrector_steps=n_corr, snr=SNR, z_chunk_steps=7)  # several calls per run
    sampler.inject_noise(zs)
    out = sampler.sample_conditional(torch.from_numpy(obs), torch.from_numpy(mask), B, N, resample=r, jump=j, domain=domain,
                                     feature_std=torch.from_numpy(std) if std is not None else None)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu"
    with pytest.raises(StopIteration):
        next(sampler._injected)  # every draw was consumed

    ts, h = O.timesteps(N)
    G = O.noise_scaling(L, True)
    x0 = O.prior(torch.from_numpy(zs[0]), G, SDES[sde]["sigma_max"] if sde == "ve" else None).numpy()
    noise_fn, trans_fn = R.flat_noise(zs[1:], N, j, r, n_corr)
    ref = R.resample_integrate(sde, SDES[sde], x0, oracle_score_fn(c, sd, N), noise_fn, trans_fn, ts.numpy(), float(h),
                               G.numpy(), n_corr, SNR, obs, mask, j, r, std, domain, True, dtype=np.float32)
    err = rel_err(out, ref)
    print(f"trajectory {name} {sde} n_corr={n_corr} {domain} r={r} j={j}: rel err {err:.3e}")
    assert err < TOL_TRAJ, err


# ------------------------------------------------------------------ 5. analytic white-data case ----
def _mixture(sde, mu, lw, var, fourier):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    K, L, Cn = mu.shape
    sch = scheduler(sde, fourier, L)
    m = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=torch.from_numpy(var), fourier_noise_scaling=fourier)
    return m.cuda().eval()


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_analytic_white_data_case(ffd, sde):
    """White data (tests/cond_restatement.py), where replacement is exact, so resampling must leave the statistics alone:
    one Gaussian of variance DATA_STD^2 G_l^2 behind the mixture backbone IS the white score.  4096 samples, 50 steps,
    r = 3, j = 2, one corrector, the device's own draws.  The observed prefix comes back to the operator bar; the
    unobserved variance lies in the float64 restatement's 8-seed band for this very loop
    (tests/test_resample_host.py), as recorded, without a margin."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.fourier import idft

    L, n = CR.GAUSS_L, CR.GAUSS_SAMPLES
    G = R.fourier_G(L).astype(np.float64)
    var = (R.DATA_STD ** 2 * G * G)[:, None].astype(np.float32)
    m = _mixture(sde, np.zeros((1, L, 1), np.float32), np.zeros(1, np.float32), var, True)
    series, mask = CR.gaussian_series(L)
    obs = torch.from_numpy(CR.dft(series * mask).astype(np.float32))
    s = DiffusionSampler(m, n, rng="philox", seed=23, corrector_steps=1, snr=CR.GAUSS_SNR)
    x = s.sample_conditional(obs, torch.from_numpy(mask.astype(np.float32)), n, R.WHITE_STEPS, resample=R.WHITE_RESAMPLE,
                             jump=R.WHITE_JUMP, domain="frequency")
    xt = idft(x.cuda()).cpu().numpy().astype(np.float64)
    ratio, worst = CR.unobserved_stats(xt, mask)
    lo, hi = RESAMPLED_WHITE_BAND[sde]
    e_obs = float(np.abs(xt[:, :CR.GAUSS_PREFIX] - series[:, :CR.GAUSS_PREFIX]).max() / np.abs(xt).max())
    print(f"white data {sde} r=3 j=2: variance ratio {ratio:.4f} (band {lo:.4f} .. {hi:.4f}), worst mean {worst:.2f} se, "
          f"observed {e_obs:.2e}")
    assert e_obs <= TOL_OP
    assert lo <= ratio <= hi, ratio
    assert worst < 5.0, worst


# ------------------------------------------------------------------ 6. the two-mode forecast ----
def test_two_mode_forecast_through_the_public_sampler(ffd):
    """tests/resample_restatement.py's two-mode case (exact right-mode probability 0.9) behind MixtureScoreModule:
    20 steps, r = 5, j = 2, philox, 4000 samples.  The right-mode fraction lies in the restatement's 8-seed band widened
    by 3 binomial standard deviations of 4000 draws, and above the device's own replacement run at 100 steps (the
    same 100 score evaluations)."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    mu, lw, var, obs, mask = R.two_mode_mixture()
    m = _mixture("vp", mu, lw, var, False)
    n = R.TWO_MODE_SAMPLES
    o, k = torch.from_numpy(obs[0]), torch.from_numpy(mask[0])
    again = DiffusionSampler(m, n, rng="philox", seed=5).sample_conditional(o, k, n, 20, resample=5, jump=2, domain="time")
    plain = DiffusionSampler(m, n, rng="philox", seed=5).sample_conditional(o, k, n, 100, domain="time")
    f_again, f_plain = R.right_mode_fraction(again.numpy()), R.right_mode_fraction(plain.numpy())
    lo, hi = TWO_MODE_BAND["resampled"]
    sd3 = 3.0 * np.sqrt(hi * (1.0 - hi) / n)
    print(f"two-mode: resampled {f_again:.4f} (band {lo - sd3:.4f} .. {hi + sd3:.4f}), replacement at 100 steps {f_plain:.4f}")
    # final_replace in the time domain: x + 1 (1 - x), two fp32 roundings next to 1
    assert float((again[:, :R.TWO_MODE_PREFIX] - 1.0).abs().max()) <= 2.0 ** -22
    assert lo - sd3 <= f_again <= hi + sd3, f_again
    assert f_again > f_plain, (f_again, f_plain)


# ------------------------------------------------------------------ 7. impute ----
def test_impute_with_resampling_end_to_end(ffd):
    """L = 16, C = 4, a forecast (prefix mask) with dataset statistics: time-domain series come back and the observed
    points are reproduced as they are without resampling (four chained transforms of at most TOL_OP each: TOL_TRAJ of the
    max-norm, the bar of tests/test_cond_gpu.py's impute test)."""
    c = COND_MODELS["tf_pow2_quad"]
    m, sch, sd = build(c, "vp")
    B, L, Cn = c["B"], c["L"], c["C"]
    rng = np.random.default_rng(31)
    series = torch.from_numpy(rng.standard_normal((B, L, Cn)).astype(np.float32))
    mean = torch.from_numpy(rng.standard_normal((L, Cn)).astype(np.float32))
    std = torch.from_numpy(rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32))
    mask = torch.zeros(L)
    mask[:9] = 1.0
    kw = dict(rng="philox", seed=3, corrector_steps=1, snr=SNR)
    out = sampler_for(m, c, **kw).impute(series, mask, B, 6, resample=2, jump=2, feature_mean=mean, feature_std=std)
    base = sampler_for(m, c, **kw).impute(series, mask, B, 6, feature_mean=mean, feature_std=std)
    assert tuple(out.shape) == (B, L, Cn) and out.device.type == "cpu" and bool(torch.isfinite(out).all())
    err = float((out[:, :9] - series[:, :9]).abs().max() / out.abs().max())
    err_base = float((base[:, :9] - series[:, :9]).abs().max() / base.abs().max())
    print(f"impute r=2 j=2: observed points {err:.2e} of the max-norm (without resampling {err_base:.2e})")
    assert err < TOL_TRAJ and err_base < TOL_TRAJ
    assert float((out[:, 9:] - series[:, 9:]).abs().max()) > 1e-3  # the rest is sampled, not copied
    assert not torch.equal(out, base)
    again = sampler_for(m, c, **kw).impute(series, mask, B, 6, resample=2, jump=2, feature_mean=mean, feature_std=std)
    assert torch.equal(out, again)
    same = sampler_for(m, c, **kw).impute(series, mask, B, 6, resample=1, jump=5, feature_mean=mean, feature_std=std)
    assert torch.equal(same, base)  # resample = 1 is the replacement path
