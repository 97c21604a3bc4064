"""Device tests of the log-likelihood through the probability-flow ODE (``-m gpu``): the three operators of
csrc/ffd_loglik.hip against tests/loglik_restatement.py, the loop entry ``ffd_loglik_batch`` on the closed-form mixture
(where float64 knows the answer), on the device's own Philox probes, on the three networks, over call splits and shards,
and ``DiffusionSampler.log_likelihood`` in use.

Bars.  An fp32 result is held to ``max(2e-6 x the sum of the |terms| it adds, 3 x the error of the fp32 restatement
against the float64 one)``: the first is the rounding of the number format, the second the rounding the operation order
itself allows.  Every test prints what it measured."""
import ctypes as C_
import itertools
import math

import numpy as np
import pytest
import torch

import loglik_restatement as LL
import lstm_restatement as LS
import mixture_restatement as M
import ode_restatement as R
import transformer_restatement as TR
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

SDES = {"vp": M.VP, "ve": M.VE}
EPS = 1e-3          # the marginal the likelihoods are taken at
POINT_SEED = 2      # tests/test_loglik_host.py: chosen on the restatement alone
SHAPES = [(3, 8, 1), (5, 20, 3), (4, 187, 1), (2, 33, 4)]
EULER, PREDICT, CORRECT = 0, 1, 2
INVALID, UNSUPPORTED, STATE = -1, -2, -3


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


def desc(sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    return N.SdeDesc(0, 0, kw["beta_min"], kw["beta_max"]) if sde == "vp" else N.SdeDesc(1, 0, kw["sigma_min"], kw["sigma_max"])


def bar(mass, e32):
    return np.maximum(2e-6 * np.asarray(mass), 3.0 * np.asarray(e32))


# ------------------------------------------------------------------ 1. the prior ----
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prior_logp(lib, shape, sde, fourier):
    B, L, Cn = shape
    kw = SDES[sde]
    G = M.fourier_G(L, fourier)
    rng = np.random.default_rng(L * Cn + B)
    x = ((kw["sigma_max"] if sde == "ve" else 1.0) * G[None, :, None] * rng.standard_normal(shape)).astype(np.float32)
    d = desc(sde)

    def run(xs):
        out = torch.empty(xs.shape[0], dtype=torch.float64, device="cuda")
        xd, Gd = dev(xs), dev(G)
        assert lib.ffd_prior_logp(C_.byref(d), xd.data_ptr(), Gd.data_ptr(), out.data_ptr(), xs.shape[0], L, Cn, stream()) == 0
        return out.cpu().numpy()

    got = run(x)
    want = LL.prior_logp(sde, kw, x, G)
    e32 = np.abs(LL.prior_logp(sde, kw, x, G, np.float32) - want)
    mass = np.abs(LL.prior_terms(sde, kw, x, G)).reshape(B, -1).sum(-1)
    err = np.abs(got - want)
    print(f"prior {shape} {sde} fourier={fourier}: err {err.max():.3e} fp32 restatement {e32.max():.3e} "
          f"bar {bar(mass, e32).min():.3e}")
    assert np.all(err <= bar(mass, e32)), (err, bar(mass, e32))
    half = (B + 1) // 2  # a batch split in two: the same bits per sample
    assert np.array_equal(np.concatenate([run(x[:half]), run(x[half:])]), got)


# ------------------------------------------------------------------ 2. the perturbation ----
def run_perturb(lib, x, G, h, k, probes=None, seed=0, offset=0, tag0=0):
    B, L, Cn = x.shape
    out = torch.full((1 + 2 * k, B, L, Cn), float("nan"), device="cuda")
    p = dev(probes) if probes is not None else None
    xd, Gd = dev(x), dev(G)
    assert lib.ffd_loglik_perturb(xd.data_ptr(), Gd.data_ptr(), float(h), k, p.data_ptr() if p is not None else None, seed,
                                  offset, tag0, out.data_ptr(), B, L, Cn, stream()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_perturb_bit_for_bit(lib, shape, k):
    B, L, Cn = shape
    rng = np.random.default_rng(7 * L + k)
    x = rng.standard_normal(shape).astype(np.float32)
    G = M.fourier_G(L)
    h = LL.fd_step("vp", M.VP, 0.3, 1e-2)
    signs = rng.choice([-1.0, 1.0], (k,) + shape).astype(np.float32)
    anyv = rng.standard_normal((k,) + shape).astype(np.float32) * 3.0  # injected non-+-1 probes pass through
    for probes in (signs, anyv):
        assert np.array_equal(run_perturb(lib, x, G, h, k, probes), LL.perturb(x, probes, G, h, np.float32))


@pytest.mark.parametrize("seed", [5, (0x9E3779B9 << 32) | 7], ids=["seed_lo", "seed_hi_lo"])
def test_perturb_philox_probes_element_by_element(lib, seed):
    """per = L C = 33 elements per sample: sample offsets 0 .. 3 put the first element at offsets 0 .. 3 modulo 4 (every
    slot of a Philox block), and the batch runs across many block boundaries."""
    shape = (3, 33, 1)
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    G = M.fourier_G(33)
    h, k = np.float32(0.125), 3
    for offset in (0, 1, 2, 3, 2 ** 33 + 1):
        for e in (0, 5):
            tag0 = LL.tag_probe(e, k, 0)
            want = LL.perturb(x, LL.philox_probes(seed, e, k, offset, shape), G, h, np.float32)
            assert np.array_equal(run_perturb(lib, x, G, h, k, None, seed, offset, tag0), want), (offset, e)


# ------------------------------------------------------------------ 3. the tail ----
def run_tail(lib, sde, stage, x, xp, d1, score, G, t, dt, h, k, probes, delta, v1, seed=0, offset=0, tag0=0):
    """-> (x, xp, d1, delta, v1, v) after the launch, as numpy"""
    B, L, Cn = x.shape
    d = desc(sde)
    xd, xpd, d1d = dev(x), dev(xp), dev(d1)
    dl = torch.from_numpy(np.asarray(delta, np.float64).copy()).cuda()
    v1d = torch.from_numpy(np.asarray(v1, np.float64).copy()).cuda()
    vo = torch.empty(B, dtype=torch.float64, device="cuda")
    p = dev(probes) if probes is not None else None
    sc, Gd = dev(score), dev(G)
    rc = lib.ffd_loglik_tail(C_.byref(d), stage, xd.data_ptr(), xpd.data_ptr(), d1d.data_ptr(), sc.data_ptr(),
                             Gd.data_ptr(), float(t), float(dt), float(h), k, p.data_ptr() if p is not None else None,
                             seed, offset, tag0, dl.data_ptr(), v1d.data_ptr(), vo.data_ptr(), B, L, Cn, stream())
    assert rc == 0
    return tuple(a.cpu().numpy() for a in (xd, xpd, d1d, dl, v1d, vo))


TAIL_SHAPES = [(3, 8, 1), (5, 20, 3), (2, 33, 4), (3, 1, 1), (2, 187, 4)]  # C % 4 != 0 and == 0, L C = 1, 748 = 3 waves' worth


def tail_case(shape, sde, k, seed):
    B, L, Cn = shape
    rng = np.random.default_rng(seed)
    f = np.float32
    x, xp, d1 = (rng.standard_normal(shape).astype(f) for _ in range(3))
    score = rng.standard_normal((1 + 2 * k,) + shape).astype(f)
    probes = rng.choice([-1.0, 1.0], (k,) + shape).astype(f)
    delta, v1 = rng.standard_normal(B) * 10.0, rng.standard_normal(B) * 100.0
    t = float(np.float32(0.37))
    return x, xp, d1, score, probes, delta, v1, t, 0.01, LL.fd_step(sde, SDES[sde], t, 1e-2)


@pytest.mark.parametrize("stage", [EULER, PREDICT, CORRECT], ids=["euler", "predict", "correct"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tail_vs_float64(lib, shape, sde, stage):
    B, L, Cn = shape
    k, kw, G = 3, SDES[sde], M.fourier_G(shape[1])
    x, xp, d1, score, probes, delta, v1, t, dt, h = tail_case(shape, sde, k, 31 * L + Cn + stage)
    got = run_tail(lib, sde, stage, x, xp, d1, score, G, t, dt, h, k, probes, delta, v1)
    want = LL.tail(stage, sde, kw, t, dt, x, xp, d1, score, probes, G, h, delta, v1)
    w32 = LL.tail(stage, sde, kw, t, dt, x, xp, d1, score, probes, G, h, delta, v1, np.float32)
    # the state: 2e-6 of its scale
    for i, name in ((0, "x"), (1, "xp"), (2, "d1")):
        ref = np.asarray(want[i], np.float64)
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(got[i] - ref).max() <= 2e-6 * scale, (name, np.abs(got[i] - ref).max())
    # v and the increment of delta: the terms' mass over 2 h k, or what the fp32 order itself costs
    mass = np.abs(LL.trace_terms(score, probes, G)).sum(axis=(0, 2)) / (2.0 * float(h) * k)
    vbar = bar(mass, np.abs(w32[5] - want[5]))
    verr = np.abs(got[5] - want[5])
    print(f"tail {shape} {sde} stage {stage}: v err {verr.max():.3e} (|v| {np.abs(want[5]).max():.3e}) bar {vbar.min():.3e}")
    assert np.all(verr <= vbar), (verr, vbar)
    inc_got, inc_want = got[3] - delta, np.asarray(want[3]) - delta
    step = dt if stage == EULER else 0.5 * dt
    assert np.all(np.abs(inc_got - inc_want) <= step * vbar + 1e-12 * np.abs(delta))
    if stage == PREDICT:
        assert np.array_equal(got[3], delta) and np.array_equal(got[4], got[5]) and np.array_equal(got[0], x)
    else:
        assert np.array_equal(got[4], v1)


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_tail_zero_score_and_determinism(lib, sde):
    shape, k = (4, 187, 4), 2
    B, L, Cn = shape
    kw, G = SDES[sde], M.fourier_G(L)
    x, xp, d1, score, probes, delta, v1, t, dt, h = tail_case(shape, sde, k, 77)
    a, _ = R.coefficients(sde, kw, t)
    got = run_tail(lib, sde, EULER, x, xp, d1, np.zeros_like(score), G, t, dt, h, k, probes, delta, v1)
    assert np.array_equal(got[5], np.full(B, a * (L * Cn)))  # a zero score stack: v = a L C exactly
    # identical bits from run to run, and for a sample moved within the batch (and into a smaller one)
    one = run_tail(lib, sde, CORRECT, x, xp, d1, score, G, t, dt, h, k, probes, delta, v1)
    two = run_tail(lib, sde, CORRECT, x, xp, d1, score, G, t, dt, h, k, probes, delta, v1)
    for a_, b_ in zip(one, two):
        assert np.array_equal(a_, b_)
    perm = np.array([2, 0, 3])
    moved = run_tail(lib, sde, CORRECT, x[perm], xp[perm], d1[perm], score[:, perm], G, t, dt, h, k, probes[:, perm],
                     delta[perm], v1[perm])
    for a_, b_ in zip(one, moved):
        assert np.array_equal(a_[perm], b_)
    # the Philox path regenerates what the perturbation drew: the restated probes, injected, give the same bits
    seed, offset, tag0 = 99, 7, LL.tag_probe(3, k, 0)
    drawn = run_tail(lib, sde, EULER, x, xp, d1, score, G, t, dt, h, k, None, delta, v1, seed, offset, tag0)
    fed = run_tail(lib, sde, EULER, x, xp, d1, score, G, t, dt, h, k, LL.philox_probes(seed, 3, k, offset, shape), delta, v1)
    for a_, b_ in zip(drawn, fed):
        assert np.array_equal(a_, b_)


def test_operator_argument_errors_on_device_pointers(lib):
    """(the refusals that need real buffers to tell apart from the null-pointer ones: aliasing and the size limit)"""
    d = desc("vp")
    buf = torch.zeros(4096, device="cuda")
    dbl = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, q = buf.data_ptr(), dbl.data_ptr()
    G = buf.data_ptr() + 4 * 2048
    # perturb: the stack may not share an address with x
    assert lib.ffd_loglik_perturb(p, G, 0.1, 1, None, 0, 0, 0, p + 4 * 8, 2, 8, 1, None) == INVALID
    assert lib.ffd_loglik_perturb(p, G, 0.1, 1, None, 0, 0, 0, p + 4 * 1024, 2, 2 ** 15, 2 ** 14, None) == UNSUPPORTED
    # tail: x aliasing the score stack, x_pred aliasing x
    sc = p + 4 * 1024
    assert lib.ffd_loglik_tail(C_.byref(d), EULER, sc, None, None, sc, G, 0.5, 0.01, 0.1, 1, None, 0, 0, 0, q, None, None,
                               2, 8, 1, None) == INVALID
    assert lib.ffd_loglik_tail(C_.byref(d), PREDICT, p, p, p + 4 * 64, sc, G, 0.5, 0.01, 0.1, 1, None, 0, 0, 0, q, q + 256,
                               None, 2, 8, 1, None) == INVALID
    assert lib.ffd_loglik_tail(C_.byref(d), CORRECT, p, p + 4 * 64, p + 4 * 128, sc, G, 0.5, 0.01, 0.1, 1, None, 0, 0, 0, q, q,
                               None, 2, 8, 1, None) == INVALID  # delta == v1


# ------------------------------------------------------------------ the mixture cases ----
def scheduler(sde, L, fourier=True, eps=EPS, kw=None):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=fourier, eps=eps, **(kw or SDES[sde]))
    sch.set_noise_scaling(L)
    return sch


def mixture_module(sde, mu, lw, var):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    K, L, Cn = mu.shape
    sch = scheduler(sde, L)
    m = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=None if var is None else torch.from_numpy(var),
                           fourier_noise_scaling=True)
    return m.cuda().eval(), sch


def sampler(m, B, **kw):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    return DiffusionSampler(score_model=m, sample_batch_size=B, **kw)


def cycle_probes(probes):
    """the slabs of one probe set, over and over: every evaluation of a run takes the same (k, B, L, C) set"""
    return itertools.cycle(list(probes))


class ModeCase:
    """The mode mixture (tests/mixture_restatement.py), points of its eps-marginal, and the two restatements."""

    def __init__(self, sde, B):
        self.sde, self.kw = sde, SDES[sde]
        self.mu, self.lw, self.var = M.mode_mixture()
        self.L = self.mu.shape[1]
        self.G = M.fourier_G(self.L)
        self.x0 = LL.eps_marginal_points(sde, self.kw, self.mu, self.lw, self.var, self.G, EPS, B, POINT_SEED)
        self.m, self.sch = mixture_module(sde, self.mu, self.lw, self.var)
        assert np.array_equal(self.sch.G.numpy(), self.G)

    def score_fn(self, dtype=np.float64):
        return M.score_fn(self.sde, self.kw, self.mu, self.lw, self.var, self.G, dtype)

    def log_pt(self, x, t):
        return M.log_pt(self.sde, self.kw, x, t, self.mu, self.lw, self.var, self.G)

    def restate(self, solver, n, dtype=np.float64, stats=None, **kw):
        ts, _ = R.grid(n + 1, EPS)
        return LL.integrate(solver, self.sde, self.kw, self.x0, self.score_fn(dtype), ts, self.G, dtype=dtype, stats=stats, **kw)


# ------------------------------------------------------------------ 4. the exact answer ----
@pytest.mark.parametrize("n", [100, 200])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_mixture_exact_answer_heun(lib, sde, n):
    B = 16
    c = ModeCase(sde, B)
    pr = LL.exact_probes(B, c.L, 1)
    s = sampler(c.m, B)
    s.inject_noise(cycle_probes(pr))
    out = s.log_likelihood(torch.from_numpy(c.x0), n + 1, solver="ode_heun", n_probes=c.L, return_latent=True)
    stats = {}
    x64, d64 = c.restate("ode_heun", n, n_probes=c.L, probes=lambda e: pr, stats=stats)
    x32, d32 = c.restate("ode_heun", n, np.float32, n_probes=c.L, probes=lambda e: pr)
    dbar = bar(stats["abs"], np.abs(d32 - d64))
    derr = np.abs(out.delta.numpy() - d64)
    xerr = np.abs(out.latent.numpy() - x64).max()
    xbar = max(2e-6 * np.abs(x64).max(), 3.0 * np.abs(x32 - x64).max())
    own = np.abs(d64 - (c.log_pt(c.x0, EPS) - c.log_pt(x64, 1.0)))  # the restatement's discretisation error
    exact = np.abs(out.delta.numpy() - (c.log_pt(c.x0, EPS) - c.log_pt(out.latent.numpy(), 1.0)))
    print(f"exact answer {sde} {n} intervals: delta err {derr.max():.3e} (fp32 restatement {np.abs(d32 - d64).max():.3e}, "
          f"mass {stats['abs'].max():.3e}, bar {dbar.min():.3e}); latent err {xerr:.3e} (bar {xbar:.3e}); against log_pt "
          f"{exact.max():.3e} (the restatement's own {own.max():.3e})")
    assert np.all(derr <= dbar), (derr, dbar)
    assert xerr <= xbar
    assert np.all(exact <= own + dbar)
    # end to end: logp = prior_logp + delta to the last bit of the float64 sum; the prior is the density of the latent
    assert torch.equal(out.logp, out.prior_logp + out.delta)
    assert torch.equal(out.bpd, -out.logp / (c.L * math.log(2.0)))
    pl = LL.prior_logp(sde, c.kw, out.latent.numpy(), c.G)
    assert np.abs(out.prior_logp.numpy() - pl).max() <= 2e-6 * np.abs(LL.prior_terms(sde, c.kw, out.latent.numpy(), c.G)).sum(
        axis=(1, 2)).max() + 1e-6


def test_mixture_exact_answer_euler(lib):
    B, n, sde = 16, 100, "vp"
    c = ModeCase(sde, B)
    pr = LL.exact_probes(B, c.L, 1)
    s = sampler(c.m, B)
    s.inject_noise(cycle_probes(pr))
    out = s.log_likelihood(torch.from_numpy(c.x0), n + 1, solver="ode_euler", n_probes=c.L, return_latent=True)
    stats = {}
    x64, d64 = c.restate("ode_euler", n, n_probes=c.L, probes=lambda e: pr, stats=stats)
    x32, d32 = c.restate("ode_euler", n, np.float32, n_probes=c.L, probes=lambda e: pr)
    dbar = bar(stats["abs"], np.abs(d32 - d64))
    derr = np.abs(out.delta.numpy() - d64)
    print(f"euler {sde}: delta err {derr.max():.3e} bar {dbar.min():.3e}")
    assert np.all(derr <= dbar)
    assert np.abs(out.latent.numpy() - x64).max() <= max(2e-6 * np.abs(x64).max(), 3.0 * np.abs(x32 - x64).max())


# ------------------------------------------------------------------ 5. Hutchinson on the device's own draws ----
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_hutchinson_on_device_draws(lib, sde):
    B, n, seed = 256, 100, 11
    c = ModeCase(sde, B)
    X = torch.from_numpy(c.x0)
    one = sampler(c.m, B, rng="philox", seed=seed).log_likelihood(X, n + 1, n_probes=1).delta.numpy()
    four = sampler(c.m, B, rng="philox", seed=seed).log_likelihood(X, n + 1, n_probes=4).delta.numpy()
    pr = LL.exact_probes(B, c.L, 1)
    s = sampler(c.m, B)
    s.inject_noise(cycle_probes(pr))
    exact = s.log_likelihood(X, n + 1, n_probes=c.L).delta.numpy()
    # per sample: the restatement fed the restated Philox probes
    stats = {}
    _, d64 = c.restate("ode_heun", n, n_probes=1, probes=None, seed=seed, stats=stats)
    _, d32 = c.restate("ode_heun", n, np.float32, n_probes=1, probes=None, seed=seed)
    dbar = bar(stats["abs"], np.abs(d32 - d64))
    derr = np.abs(one - d64)
    dev1, dev4 = one - exact, four - exact
    se = dev1.std(ddof=1) / math.sqrt(B)
    rms1, rms4 = math.sqrt((dev1 ** 2).mean()), math.sqrt((dev4 ** 2).mean())
    print(f"hutchinson {sde}: per-sample err {derr.max():.3e} (bar {dbar.min():.3e}); mean deviation {dev1.mean() / se:+.2f} "
          f"standard errors; rms {rms1:.3f} (1 probe), {rms4:.3f} (4 probes), ratio {rms4 / rms1:.3f}")
    assert np.all(derr <= dbar), (derr.max(), dbar.min())
    assert abs(dev1.mean()) <= 4.0 * se
    assert rms4 <= 0.6 * rms1


# ------------------------------------------------------------------ 6. the networks ----
# The networks carry random weights: their "score" is O(1) whatever x is, so under the standard VE (sigma_max = 50) the
# ODE's drift cs(t)^2 s / 2 of up to 2e4 moves x by thousands per interval of an 8-interval grid, x_T reaches 1e8, and the
# fp32 oracle and the float64 judge -- restatement against restatement, on the CPU, no device involved -- end 17 .. 126
# nats apart on |delta| of 450 .. 820: that case measures the instability of an explicit solver on a meaningless drift,
# not a kernel.  sigma_max = 5 keeps x_T at 11 .. 34 and the two restatements 3e-5 .. 1e-4 nats apart.
NET_SDES = {"vp": M.VP, "ve": dict(sigma_min=0.01, sigma_max=5.0)}
# "draws": how many draws of (x0, probes) the yardstick -- the fp32 oracle's error against the float64 judge -- is taken over,
# seeds seed .. seed + draws - 1, all on the CPU; the device runs the first.  One draw where a case sums hundreds of terms.
# At the LSTM's smallest accepted shape (d_model 8, one layer, L C = 2) the yardstick is a maximum over three samples of
# two-coordinate traces and moves by a factor of five with the draw (VE, six draws: 9e-6 .. 4e-5 nats), so it is taken over
# six fixed draws there.
NETS = {
    "transformer": dict(kind="transformer", d=16, H=4, NL=2, L=20, C=3, B=3, seed=111, draws=1),
    "lstm": dict(kind="lstm", d=8, H=1, NL=2, L=20, C=3, B=3, seed=104, draws=1),
    "lstm_smallest": dict(kind="lstm", d=8, H=1, NL=1, L=2, C=1, B=3, seed=104, draws=6),
    "mlp": dict(kind="mlp", d=8, H=1, NL=2, L=20, C=3, B=3, d_mlp=64, seed=103, draws=1),
}


def build_net(c, sde):
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule

    sch = scheduler(sde, c["L"], kw=NET_SDES[sde])
    common = dict(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"])
    if c["kind"] == "lstm":
        m = LSTMScoreModule(fourier_noise_scaling=True, **common)
        sd = synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=146)
    elif c["kind"] == "mlp":
        m = MLPScoreModule(d_mlp=c["d_mlp"], **common)
        sd = synthetic.mlp_state_dict(c["C"], c["L"], c["d"], c["d_mlp"], c["NL"], seed=149)
    else:
        m = ScoreModule(fourier_noise_scaling=True, n_head=c["H"], **common)
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=142)
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sch, sd


def net_score_fns(c, sd):
    """(the oracle's fp32 forward, the float64 judge) as score_fn(x, t, k)"""
    def f32(x, t, k=0):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        tt = torch.full((xt.shape[0],), t, dtype=torch.float32)
        if c["kind"] == "lstm":
            return O.lstm_score_forward(xt, tt, sd, c["NL"]).numpy()
        if c["kind"] == "mlp":
            return O.mlp_score_forward(xt, tt, sd, c["NL"]).numpy()
        return O.score_forward(xt, tt, sd, c["NL"], c["H"]).numpy()

    def f64(x, t, k=0):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        tt = torch.full((xt.shape[0],), t, dtype=torch.float32)
        if c["kind"] == "lstm":
            return LS.lstm_score_forward64(xt, tt, sd, c["NL"])[0].numpy()
        if c["kind"] == "mlp":
            return O.mlp_score_forward(xt, tt.to(torch.float64), TR.sd64(sd), c["NL"]).numpy()
        return TR.score_forward64(xt, tt, sd, c["NL"], c["H"]).numpy()

    return f32, f64


def net_draw(c, seed, n, k):
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((c["B"], c["L"], c["C"])).astype(np.float32)
    return x0, rng.choice([-1.0, 1.0], (2 * n, k, c["B"], c["L"], c["C"])).astype(np.float32)


@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_networks_vs_oracle_and_float64_judge(lib, name, sde):
    """latent: within 1e-5 of the max-norm of the fp32 restatement driven by the oracle's forward.  delta: within
    max(3 x E, 2e-6 x the sum of |dt v|) of the float64 judge, E = the fp32 oracle's error against the judge over the
    case's draws -- the bar of every other test in this file, fixed on the CPU before the device runs.
    Recorded, device / the oracle on the device's draw: transformer 5.0e-5 / 7.3e-5 (VP), 4.2e-5 / 6.4e-5 (VE); LSTM
    20 x 3 1.1e-5 / 1.9e-5, 6.6e-5 / 9.7e-5; MLP 4.5e-5 / 4.8e-5, 2.1e-4 / 1.9e-4.  LSTM at its smallest shape (|delta| 7.8 /
    7.6): VP 7.4e-6 / 3.1e-6, E over the six draws 8.6e-6, bar 2.6e-5; VE 1.7e-5 / 4.5e-6, E over the six draws 5.7e-5, bar
    1.7e-4 -- on the device's draw alone 3 x 4.5e-6 = 1.3e-5 and 2e-6 x 7.6 = 1.5e-5 both lie below the device's 1.7e-5,
    which is why one draw is no yardstick there: the device's error sits inside the oracle's own range over the draws."""
    c = NETS[name]
    B, L, Cn, n, k = c["B"], c["L"], c["C"], 8, 2
    m, sch, sd = build_net(c, sde)
    f32, f64 = net_score_fns(c, sd)
    ts, _ = R.grid(n + 1, EPS)
    G = sch.G.numpy()
    runs = []
    for i in range(c["draws"]):
        x0, probes = net_draw(c, c["seed"] + i, n, k)
        stats = {}
        x32, d32 = LL.integrate("ode_heun", sde, NET_SDES[sde], x0, f32, ts, G, n_probes=k, probes=probes, dtype=np.float32)
        x64, d64 = LL.integrate("ode_heun", sde, NET_SDES[sde], x0, f64, ts, G, n_probes=k, probes=probes, stats=stats)
        runs.append((x0, probes, x32, d64, float(np.abs(d32 - d64).max()), float(stats["abs"].max())))
    x0, probes, x32, d64, own_err, mass = runs[0]
    oracle_err = max(r[4] for r in runs)
    dbar = max(3.0 * oracle_err, 2e-6 * mass)
    s = sampler(m, B)
    s.inject_noise(iter(probes.reshape((-1, B, L, Cn))))
    out = s.log_likelihood(torch.from_numpy(x0), n + 1, n_probes=k, return_latent=True)
    lat = rel_err(out.latent.numpy(), x32)
    dev_err = np.abs(out.delta.numpy() - d64).max()
    print(f"network {name} {sde}: latent rel err {lat:.3e}; delta: device against the float64 judge {dev_err:.3e}, fp32 "
          f"oracle against it {own_err:.3e} on this draw, {oracle_err:.3e} over {c['draws']} draw(s), bar {dbar:.3e} "
          f"(|delta| {np.abs(d64).max():.3e})")
    assert lat < 1e-5, lat
    assert dev_err <= dbar, (dev_err, oracle_err, dbar)


# ------------------------------------------------------------------ 7. splits and shards ----
def loop_call(lib, ctx, x, delta, ts, first, n_run, solver, k, fd_rel=1e-2, probes=None, seed=0, offset=0):
    tsc = (C_.c_float * len(ts))(*[float(t) for t in ts])
    return lib.ffd_loglik_batch(ctx.handle, x.data_ptr(), delta.data_ptr(), x.shape[0], tsc, len(ts), first, n_run, solver, k,
                                fd_rel, probes.data_ptr() if probes is not None else None, seed, offset, stream())


@pytest.mark.parametrize("inject", [False, True], ids=["philox", "injected"])
def test_splits_reproduce_the_single_call(lib, inject):
    B, n, k = 5, 6, 2
    c = ModeCase("vp", B)
    ctx = c.m._ctx()
    ts, _ = R.grid(n + 1, EPS)
    probes = dev(np.random.default_rng(3).choice([-1.0, 1.0], (2 * n, k, B, c.L, 1))) if inject else None
    slab = k * B * c.L

    def run(cuts):
        x, delta = dev(c.x0), torch.zeros(B, dtype=torch.float64, device="cuda")
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p = probes.reshape(-1)[2 * lo * slab:] if inject else None
            assert loop_call(lib, ctx, x, delta, ts, lo, hi - lo, 2, k, probes=p, seed=21, offset=4) == 0
        return x.cpu().numpy(), delta.cpu().numpy()

    whole = run([0, n])
    again = run([0, n])
    assert np.array_equal(whole[0], again[0]) and np.array_equal(whole[1], again[1])  # two runs are bit-identical
    for cut in range(1, n):
        part = run([0, cut, n])
        assert np.array_equal(part[0], whole[0]) and np.array_equal(part[1], whole[1]), cut
    assert np.all(np.isfinite(whole[1])) and np.abs(whole[1]).max() > 0


def test_philox_shards_agree(lib):
    B, n, k, seed = 6, 6, 1, 33
    c = ModeCase("ve", B)
    ctx = c.m._ctx()
    ts, _ = R.grid(n + 1, EPS)

    def run(lo, hi, offset):
        x, delta = dev(c.x0[lo:hi]), torch.zeros(hi - lo, dtype=torch.float64, device="cuda")
        assert loop_call(lib, ctx, x, delta, ts, 0, n, 2, k, seed=seed, offset=offset) == 0
        return x.cpu().numpy(), delta.cpu().numpy()

    whole = run(0, B, 10)
    a, b = run(0, 3, 10), run(3, B, 13)
    # the probes of a shard are the unsharded call's, bit for bit (the perturbation shows them)
    h = LL.fd_step("ve", c.kw, float(ts[-1]), 1e-2)
    full = run_perturb(lib, c.x0, c.G, h, k, None, seed, 10, LL.tag_probe(0, k, 0))
    part = run_perturb(lib, c.x0[3:], c.G, h, k, None, seed, 13, LL.tag_probe(0, k, 0))
    assert np.array_equal(full[:, 3:], part)
    got = np.concatenate([a[1], b[1]])
    stats = {}
    _, d64 = c.restate("ode_heun", n, n_probes=k, probes=None, seed=seed, sample_offset=10, stats=stats)
    _, d32 = c.restate("ode_heun", n, np.float32, n_probes=k, probes=None, seed=seed, sample_offset=10)
    dbar = bar(stats["abs"], np.abs(d32 - d64))
    print(f"shards: |sharded - whole| {np.abs(got - whole[1]).max():.3e}, whole against float64 {np.abs(whole[1] - d64).max():.3e}, "
          f"bar {dbar.min():.3e}")
    assert np.all(np.abs(whole[1] - d64) <= dbar) and np.all(np.abs(got - d64) <= dbar)


def test_loop_entry_argument_errors(lib):
    """Every refusal comes before any device work: x and delta stay as they are."""
    from fastfourierdiffusion_amd import _native as N

    B, n = 2, 4
    c = ModeCase("vp", B)
    ctx = c.m._ctx()
    ts, _ = R.grid(n + 1, EPS)
    x, delta = dev(c.x0), torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    keep = x.clone()

    def call(first=0, n_run=n, solver=2, k=1, fd_rel=1e-2, grid=ts, xx=x, dd=delta, Bc=B):
        tsc = (C_.c_float * len(grid))(*[float(t) for t in grid])
        return lib.ffd_loglik_batch(ctx.handle, xx.data_ptr() if xx is not None else None,
                                    dd.data_ptr() if dd is not None else None, Bc, tsc, len(grid), first, n_run, solver, k,
                                    fd_rel, None, 0, 0, stream())

    for kw in (dict(xx=None), dict(dd=None), dict(Bc=0), dict(k=0), dict(solver=0), dict(solver=4), dict(fd_rel=0.0),
               dict(fd_rel=-1.0), dict(fd_rel=float("nan")), dict(fd_rel=float("inf")), dict(first=-1), dict(n_run=n + 1),
               dict(first=2, n_run=n - 1), dict(grid=ts[:1], n_run=0), dict(grid=ts[::-1].copy()),
               dict(grid=np.float32([1.0, 0.5, 0.5, 0.2, 0.1]))):
        assert call(**kw) == INVALID, kw
    assert lib.ffd_loglik_batch(None, x.data_ptr(), delta.data_ptr(), B, None, 0, 0, 0, 2, 1, 1e-2, None, 0, 0, None) == INVALID
    # the end of the probes' tag family: e n_probes + m reaches 0x0FFFFFF0 (one interval is asked for, none runs)
    big = np.linspace(1.0, EPS, 1001).astype(np.float32)
    k_over = -(-LL.LIMIT_LOGLIK // (2 * 999 + 1))
    assert not LL.run_fits("ode_heun", 999, 1, k_over) and call(grid=big, first=999, n_run=1, k=k_over) == INVALID
    assert call(k=2 ** 28) == UNSUPPORTED  # (1 + 2 k) B L C reaches 2^31
    cfg = N.FrescaCfg(0.9, 1.2, 0.4, 0, 0)
    assert lib.ffd_fresca_enable(ctx.handle, C_.byref(cfg)) == 0
    assert call() == STATE and b"FreSca" in lib.ffd_last_error(ctx.handle)
    assert lib.ffd_fresca_disable(ctx.handle) == 0
    assert torch.equal(x, keep) and torch.all(delta == 7.0)
    assert call(n_run=0) == 0 and torch.equal(x, keep) and torch.all(delta == 7.0)  # an empty run is allowed
    assert call() == 0 and not torch.equal(x, keep)  # delta is accumulated, not zeroed
    fresh = torch.zeros(B, dtype=torch.float64, device="cuda")
    assert call(xx=keep.clone(), dd=fresh) == 0
    assert torch.all((delta - (fresh + 7.0)).abs() <= 1e-12 * (7.0 + fresh.abs()))


def test_cache_is_refused_by_the_sampler_and_untouched_by_the_entry(lib):
    c = NETS["transformer"]
    m, sch, sd = build_net(c, "vp")
    s = sampler(m, c["B"], use_cache=True, cache_kwargs=dict(K=5, R=10))
    X = torch.zeros(c["B"], c["L"], c["C"])
    with pytest.raises(ValueError, match="use_cache"):
        s.log_likelihood(X, 5)
    # the entry has no cache argument: on a context with the cache enabled it runs the uncached forward and leaves the
    # cache's counters as they are
    ctx = m._ctx()
    before = m._native_cache_stats()
    ts, _ = R.grid(5, EPS)
    x, delta = X.cuda(), torch.zeros(c["B"], dtype=torch.float64, device="cuda")
    assert loop_call(lib, ctx, x, delta, ts, 0, 4, 2, 1) == 0
    after = m._native_cache_stats()
    assert (after.recompute_count, after.cache_hit_count) == (before.recompute_count, before.cache_hit_count)
    m.disable_caching()
    x2, delta2 = X.cuda(), torch.zeros(c["B"], dtype=torch.float64, device="cuda")
    assert loop_call(lib, ctx, x2, delta2, ts, 0, 4, 2, 1) == 0
    assert torch.equal(x, x2) and torch.equal(delta, delta2)


# ------------------------------------------------------------------ 8. use ----
def test_anomaly_scores_on_a_from_data_mixture(lib):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    L, Cn, bw = 24, 2, 0.1
    rng = np.random.default_rng(8)
    tgrid = np.linspace(0.0, 1.0, L)[None, :, None]
    data = (np.sin(2 * np.pi * (tgrid * rng.uniform(1.0, 3.0, (64, 1, 1)) + rng.uniform(0, 1, (64, 1, Cn))))
            + 0.05 * rng.standard_normal((64, L, Cn))).astype(np.float32)
    sch = scheduler("vp", L)
    m = MixtureScoreModule.from_data(torch.from_numpy(data), sch, bandwidth=bw).cuda().eval()
    al, s2 = M.alpha_sigma2("vp", M.VP, EPS)
    G = sch.G.numpy().astype(np.float64)
    noise = np.sqrt(s2) * G[None, :, None] * rng.standard_normal((8, L, Cn))
    held_in = (al * data[:8] + noise).astype(np.float32)
    shifted = (al * (data[:8] + 3.0 * bw) + noise).astype(np.float32)  # three bandwidths per coordinate
    s = sampler(m, 5, rng="philox", seed=1)  # 16 series in batches of 5: the remainder gets its numbers too
    out = s.log_likelihood(torch.from_numpy(np.concatenate([held_in, shifted])), 51, n_probes=4)
    assert tuple(out.logp.shape) == (16,) and out.logp.dtype == torch.float64 and out.latent is None
    assert torch.all(torch.isfinite(out.bpd)) and torch.all(torch.isfinite(out.logp))
    print("held-in logp", out.logp[:8].numpy().round(1), "shifted", out.logp[8:].numpy().round(1))
    assert torch.all(out.logp[8:] < out.logp[:8])
    with pytest.raises(ValueError, match="use_fresca"):
        sampler(m, 5, use_fresca=True).log_likelihood(torch.from_numpy(held_in), 51)


def test_torch_rng_draws_rademacher_probes_in_chunks(lib):
    """rng="torch": seeded runs repeat, and the chunking of the hand-over does not change the draws."""
    B, n = 4, 6
    c = ModeCase("vp", B)
    X = torch.from_numpy(c.x0)
    outs = []
    for chunk in (50, 3):
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        outs.append(sampler(c.m, B, z_chunk_steps=chunk).log_likelihood(X, n + 1, n_probes=2).delta)
    assert torch.equal(outs[0], outs[1]) and torch.all(torch.isfinite(outs[0]))
