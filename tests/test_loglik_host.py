"""CPU-side tests of the log-likelihood through the probability-flow ODE (no GPU): the C surface and every argument error
raised before device work, the Python refusals, the result object and the remainder rule, the probes' stream tags at and
beyond their limit, and the numpy restatement (tests/loglik_restatement.py) against the mixture's closed-form log-density
``mixture_restatement.log_pt`` -- an answer it shares no code with.

The points of the accuracy checks are draws of the mode mixture's eps-marginal under ``POINT_SEED``.  The errors' maxima
over 16 points move by a factor of two with the draw (seeds 0 .. 9: 0.014 .. 0.029 for VP at 100 intervals); the seed
is fixed by this restatement alone, on the CPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import loglik_restatement as LL
import mixture_restatement as M
import ode_restatement as R
import philox_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
EPS, POINT_SEED = 1e-3, 2
SYMBOLS = ("ffd_host_loglik_h", "ffd_prior_logp", "ffd_loglik_perturb", "ffd_loglik_tail", "ffd_loglik_batch")


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


# ------------------------------------------------------------------ the C surface ----
def test_symbols_constants_and_header(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name)
        # the binding takes as many arguments as the declaration
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(N.SIGNATURES[name][1]) == decl.count(",") + 1, name
    assert re.search(r"FFD_LOGLIK_EULER = 0, FFD_LOGLIK_PREDICT = 1, FFD_LOGLIK_CORRECT = 2", header)
    assert (N.FFD_LOGLIK_EULER, N.FFD_LOGLIK_PREDICT, N.FFD_LOGLIK_CORRECT) == (0, 1, 2)
    assert "0xF0000000" in header and "0x0FFFFFF0" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in integration, name


def sde_desc(kind=0):
    from fastfourierdiffusion_amd import _native as N

    return N.SdeDesc(kind, 0, 0.1, 20.0) if kind != 1 else N.SdeDesc(1, 0, 0.01, 50.0)


def test_host_step_matches_the_restatement(lib):
    out = C.c_float()
    for kind, sde in ((0, "vp"), (1, "ve")):
        d = sde_desc(kind)
        for t in (1e-5, 1e-3, 0.37, 1.0):
            for fd_rel in (1e-1, 1e-2, 1e-4):
                assert lib.ffd_host_loglik_h(C.byref(d), t, fd_rel, C.byref(out)) == 0
                assert out.value == float(LL.fd_step(sde, M.sde_kwargs(sde), t, fd_rel)), (sde, t, fd_rel)
    d = sde_desc(0)
    for bad in (dict(sde=None), dict(out=None), dict(t=-0.1), dict(t=float("nan")), dict(t=float("inf")), dict(fd_rel=0.0),
                dict(fd_rel=-1e-2), dict(fd_rel=float("nan")), dict(fd_rel=float("inf")), dict(sde=sde_desc(7)),
                dict(t=0.0)):  # (sigma(0) = 0 for VP: no step)
        kw = dict(sde=d, t=0.5, fd_rel=1e-2, out=out)
        kw.update(bad)
        assert lib.ffd_host_loglik_h(C.byref(kw["sde"]) if kw["sde"] is not None else None, kw["t"], kw["fd_rel"],
                                     C.byref(kw["out"]) if kw["out"] is not None else None) == INVALID, bad


def test_operator_argument_errors(lib):
    """Every refusal comes before any device work: none of these pointers is a device pointer."""
    buf = np.zeros(1 << 16, np.float32)
    p = buf.ctypes.data
    x, xp, d1, sc, G, pr = p, p + 4096, p + 8192, p + 16384, p + 65536, p + 131072
    dl, v1, vo = p + 200000, p + 204096, p + 208192
    d = sde_desc(0)
    B, L, Cn, k = 2, 8, 1, 2

    def prior(sde=d, x=x, G=G, out=dl, B=B, L=L, Cn=Cn):
        return lib.ffd_prior_logp(C.byref(sde) if sde is not None else None, x, G, out, B, L, Cn, None)

    for kw in (dict(sde=None), dict(x=None), dict(G=None), dict(out=None), dict(B=0), dict(L=0), dict(Cn=0), dict(B=-3),
               dict(sde=sde_desc(7)), dict(out=x), dict(out=x + 8), dict(out=G)):
        assert prior(**kw) == INVALID, kw
    assert prior(B=2 ** 15, L=2 ** 15, Cn=2) == UNSUPPORTED

    def perturb(x=x, G=G, h=0.1, k=k, probes=pr, out=sc, B=B, L=L, Cn=Cn):
        return lib.ffd_loglik_perturb(x, G, h, k, probes, 0, 0, 0, out, B, L, Cn, None)

    for kw in (dict(x=None), dict(G=None), dict(out=None), dict(B=0), dict(L=0), dict(Cn=0), dict(k=0), dict(k=-1),
               dict(h=0.0), dict(h=-0.1), dict(h=float("nan")), dict(h=float("inf")), dict(out=x), dict(out=x + 4 * 15),
               dict(out=pr - 4), dict(out=G)):
        assert perturb(**kw) == INVALID, kw
    assert perturb(probes=None, k=2 ** 20, B=64, L=8, Cn=2) == UNSUPPORTED  # (1 + 2 k) B L C = 2^31 + ...
    assert perturb(probes=None, B=2 ** 14, L=2 ** 14, Cn=2) == UNSUPPORTED

    def tail(sde=d, stage=0, x=x, xp=xp, d1=d1, sc=sc, G=G, t=0.5, dt=0.01, h=0.1, k=k, probes=pr, delta=dl, v1=v1, vo=vo,
             B=B, L=L, Cn=Cn):
        return lib.ffd_loglik_tail(C.byref(sde) if sde is not None else None, stage, x, xp, d1, sc, G, t, dt, h, k, probes, 0,
                                   0, 0, delta, v1, vo, B, L, Cn, None)

    for stage in (0, 1, 2):
        for kw in (dict(sde=None), dict(x=None), dict(sc=None), dict(G=None), dict(B=0), dict(L=0), dict(Cn=0), dict(k=0),
                   dict(h=0.0), dict(h=float("nan")), dict(h=float("inf")), dict(dt=0.0), dict(dt=-0.01),
                   dict(dt=float("nan")), dict(dt=float("inf")), dict(dt=1e-60), dict(t=-1.0), dict(t=float("nan")),
                   dict(sde=sde_desc(7)), dict(x=sc), dict(x=sc + 4 * 40), dict(x=pr), dict(vo=x), dict(vo=G), dict(vo=sc), dict(vo=pr)):
            assert tail(stage=stage, **kw) == INVALID, (stage, kw)
    for kw in (dict(stage=3), dict(stage=-1), dict(stage=0, delta=None), dict(stage=2, delta=None), dict(stage=1, xp=None),
               dict(stage=1, d1=None), dict(stage=1, v1=None), dict(stage=2, xp=None), dict(stage=2, d1=None),
               dict(stage=2, v1=None), dict(stage=1, xp=x), dict(stage=1, d1=x), dict(stage=1, d1=xp), dict(stage=2, xp=sc),
               dict(stage=2, delta=v1), dict(stage=2, delta=x), dict(stage=1, v1=d1), dict(stage=0, delta=G),
               dict(stage=2, delta=G), dict(stage=1, v1=G), dict(stage=2, v1=sc)):
        assert tail(**kw) == INVALID, kw
    assert tail(stage=0, probes=None, k=2 ** 20, B=64, L=8, Cn=2) == UNSUPPORTED
    # the loop entry without a context
    assert lib.ffd_loglik_batch(None, x, dl, B, None, 0, 0, 0, 2, 1, 1e-2, None, 0, 0, None) == INVALID


# ------------------------------------------------------------------ the Python surface ----
def cpu_mixture(sde="vp", use_cache=False, **kw):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    mu, lw, var = M.mode_mixture()
    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=True, eps=EPS, **M.sde_kwargs(sde))
    sch.set_noise_scaling(mu.shape[1])
    m = MixtureScoreModule(n_channels=1, max_len=mu.shape[1], noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=torch.from_numpy(var))
    s = DiffusionSampler(score_model=m, sample_batch_size=5, **kw)
    s.use_cache = use_cache  # (the mixture has no cache to enable: the refusal reads the sampler's flag)
    return s


def test_python_refusals_come_before_device_work():
    """The model lives on the CPU: anything that got as far as the device would raise FFDError, not ValueError."""
    X = torch.zeros(7, 8, 1)
    ok = cpu_mixture()
    for kw, match in ((dict(solver="euler_maruyama"), "solver"), (dict(solver="ode_ab2"), "solver"),
                      (dict(n_probes=0), "n_probes"), (dict(n_probes=1.5), "n_probes"), (dict(n_probes=True), "n_probes"),
                      (dict(fd_rel=0.0), "fd_rel"), (dict(fd_rel=-1e-2), "fd_rel"), (dict(fd_rel=float("inf")), "fd_rel"),
                      (dict(fd_rel=float("nan")), "fd_rel"), (dict(num_diffusion_steps=1), "two points")):
        with pytest.raises(ValueError, match=match):
            ok.log_likelihood(X, **{"num_diffusion_steps": 10, **kw})
    for bad in (torch.zeros(8, 1), torch.zeros(7, 9, 1), torch.zeros(7, 8, 2), torch.zeros(0, 8, 1), torch.zeros(1, 7, 8, 1)):
        with pytest.raises(ValueError, match="X must be"):
            ok.log_likelihood(bad, 10)
    with pytest.raises(ValueError, match="use_cache"):
        cpu_mixture(use_cache=True).log_likelihood(X, 10)
    with pytest.raises(ValueError, match="use_fresca"):
        cpu_mixture(use_fresca=True).log_likelihood(X, 10)
    # the sampler's own solver and corrector are not consulted: this one gets past every refusal, to the device
    from fastfourierdiffusion_amd._native import FFDError

    with pytest.raises(FFDError):
        cpu_mixture(solver="dpmpp_2m").log_likelihood(X, 10)
    with pytest.raises(FFDError):
        cpu_mixture(corrector_steps=2).log_likelihood(X, 10)


def test_prior_logp_refuses_a_length_the_noise_scaling_was_not_set_for():
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    sch = VPScheduler(fourier_noise_scaling=True)
    with pytest.raises(ValueError, match="set_noise_scaling"):
        sch.prior_logp(torch.zeros(2, 8, 1))
    sch.set_noise_scaling(8)
    for bad in (torch.zeros(2, 9, 1), torch.zeros(2, 7, 3)):
        with pytest.raises(ValueError, match="set_noise_scaling"):
            sch.prior_logp(bad)
    with pytest.raises(ValueError, match="B, L, C"):
        sch.prior_logp(torch.zeros(8, 1))


def test_result_object_and_remainder_rule():
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler, LogLikelihood

    prior = torch.tensor([-10.0, -11.5, -9.25], dtype=torch.float64)
    delta = torch.tensor([3.0, 0.125, -2.0], dtype=torch.float64)
    out = LogLikelihood.from_parts(prior, delta, 8, 2)
    assert out._fields == ("logp", "prior_logp", "delta", "bpd", "latent")
    assert torch.equal(out.logp, prior + delta) and out.logp.dtype == torch.float64 and out.latent is None
    assert torch.equal(out.bpd, -(prior + delta) / (16 * math.log(2.0)))
    lat = torch.zeros(3, 8, 2)
    assert LogLikelihood.from_parts(prior, delta, 8, 2, lat).latent is lat
    # every series gets a number: the remainder is a batch of its own
    f = DiffusionSampler._likelihood_batches
    assert f(16, 5) == [(0, 5), (5, 5), (10, 5), (15, 1)]
    assert f(5, 5) == [(0, 5)] and f(3, 5) == [(0, 3)] and f(10, 5) == [(0, 5), (5, 5)]
    for n, b in ((1, 1), (7, 3), (512, 50)):
        assert sum(size for _, size in f(n, b)) == n


# ------------------------------------------------------------------ the tag plan ----
def test_probe_tags_at_and_beyond_their_limit():
    assert LL.TAG_PROBE0 == 0xF0000000 and LL.LIMIT_LOGLIK == 0x0FFFFFF0
    last = LL.LIMIT_LOGLIK - 1  # the largest e n_probes + m a run may reach
    assert LL.tag_probe(0, 1, 0) == 0xF0000000 and LL.tag_probe(last, 1, 0) == 0xFFFFFFEF
    assert LL.tag_probe(last, 1, 0) < min(P.RESERVED)  # clear of the loss's and the prior's tags
    assert LL.tag_probe(5, 4, 3) == 0xF0000000 + 23 and LL.tag_probe(2 * 7 + 1, 3, 2) == 0xF0000000 + 47
    # distinct (evaluation, probe) pairs have distinct tags
    tags = {LL.tag_probe(e, 3, m) for e in range(40) for m in range(3)}
    assert len(tags) == 120 and min(tags) == 0xF0000000
    # at the limit and beyond: Euler's e = j, Heun's e = 2 j + 1
    assert LL.run_fits("ode_euler", 0, LL.LIMIT_LOGLIK, 1) and not LL.run_fits("ode_euler", 0, LL.LIMIT_LOGLIK + 1, 1)
    assert LL.run_fits("ode_heun", 0, LL.LIMIT_LOGLIK // 2, 1) and not LL.run_fits("ode_heun", 0, LL.LIMIT_LOGLIK // 2 + 1, 1)
    assert LL.run_fits("ode_heun", 999, 1, 134217) and not LL.run_fits("ode_heun", 999, 1, 134218)  # 2000 k - 1 < limit
    assert LL.run_fits("ode_heun", 5, 0, 10 ** 9)  # an empty run draws nothing
    # the family overlaps the transitions' (0xE0000000 + q) from q = 2^28 on: the two entries never draw in one run
    assert P.tag_transition((1 << 28) - 1) < LL.TAG_PROBE0 == P.tag_transition(1 << 28)
    assert LL.TAG_PROBE0 > P.tag_projection(0, 0, 0) and LL.TAG_PROBE0 > P.tag_corrector(0, 0, 1)


def test_rademacher_probes_are_bit_31_of_the_philox_words():
    seed, tag, g0, n = (0xABCDEF01 << 32) | 17, LL.tag_probe(3, 2, 1), 4 * 11 + 3, 41
    got = LL.rademacher(seed, tag, g0, n)
    first, nb, skip = P._span(g0, n)
    words = np.stack(P._blocks(seed, tag, first, nb), axis=1).reshape(-1)[skip:skip + n]
    assert np.array_equal(got, np.where(words >= np.uint64(1 << 31), -1.0, 1.0))
    big = LL.rademacher(5, LL.tag_probe(0, 1, 0), 0, 1 << 16)
    assert set(np.unique(big)) == {-1.0, 1.0} and abs(big.mean()) < 4.0 / 256.0  # 4 standard errors
    shard = LL.philox_probes(5, 7, 2, 3, (2, 33, 1))
    whole = LL.philox_probes(5, 7, 2, 0, (5, 33, 1))
    assert np.array_equal(whole[:, 3:], shard)


# ------------------------------------------------------------------ the restatement against the closed form ----
class Mode:
    def __init__(self, sde, n):
        self.sde, self.kw = sde, M.sde_kwargs(sde)
        self.mu, self.lw, self.var = M.mode_mixture()
        self.L = self.mu.shape[1]
        self.G = M.fourier_G(self.L)
        self.x0 = LL.eps_marginal_points(sde, self.kw, self.mu, self.lw, self.var, self.G, EPS, n, POINT_SEED)
        self.score = M.score_fn(sde, self.kw, self.mu, self.lw, self.var, self.G)

    def trace(self, x, t):
        return LL.mixture_trace(self.sde, self.kw, x, t, self.mu, self.lw, self.var, self.G)

    def log_pt(self, x, t):
        return M.log_pt(self.sde, self.kw, x, t, self.mu, self.lw, self.var, self.G)

    def error(self, xT, delta):
        return np.abs(delta - (self.log_pt(self.x0, EPS) - self.log_pt(xT, 1.0)))


def test_closed_form_trace_is_the_divergence_of_the_score():
    """against a float64 central difference of mixture_restatement.score, coordinate by coordinate"""
    for sde in ("vp", "ve"):
        c = Mode(sde, 4)
        for t in (EPS, 0.2, 1.0):
            x = c.x0.astype(np.float64) * (1.0 if t == EPS else 0.5)
            h = 1e-5 * LL.sigma(sde, c.kw, t)
            tr = np.zeros(4)
            for l in range(c.L):
                e = np.zeros_like(x)
                e[:, l, 0] = h
                tr += c.G[l].astype(np.float64) ** 2 * (c.score(x + e, t) - c.score(x - e, t))[:, l, 0] / (2 * h)
            want = c.trace(x, t)
            assert np.allclose(tr, want, rtol=1e-6, atol=1e-6 * np.abs(want).max()), (sde, t)


@pytest.mark.parametrize("sde,bound", [("vp", 0.02), ("ve", 0.09)])
def test_heun_error_against_log_pt_and_its_order(sde, bound):
    c = Mode(sde, 16)
    pr = LL.exact_probes(16, c.L, 1)
    err, fd_gap = {}, {}
    for n in (100, 200):
        ts, _ = R.grid(n + 1, EPS)
        xT, d = LL.integrate("ode_heun", sde, c.kw, c.x0, c.score, ts, c.G, n_probes=c.L, probes=lambda e: pr)
        err[n] = c.error(xT, d).max()
        _, d_exact = LL.integrate_exact("ode_heun", sde, c.kw, c.x0, c.score, c.trace, ts, c.G)
        fd_gap[n] = np.abs(d - d_exact).max()
    print(f"{sde}: Heun error {err[100]:.4f} (100 intervals) {err[200]:.4f} (200), ratio {err[100] / err[200]:.2f}; exact-trace "
          f"probes against the closed-form trace {fd_gap[100]:.2e} / {fd_gap[200]:.2e} nats")
    assert err[100] < bound
    assert 3.5 <= err[100] / err[200] <= 4.5
    assert fd_gap[100] <= 2e-4 and fd_gap[200] <= 2e-4


def test_euler_is_first_order_and_far_worse():
    c = Mode("vp", 16)
    pr = LL.exact_probes(16, c.L, 1)
    ts, _ = R.grid(201, EPS)
    xT, d = LL.integrate("ode_euler", "vp", c.kw, c.x0, c.score, ts, c.G, n_probes=c.L, probes=lambda e: pr)
    xH, dH = LL.integrate("ode_heun", "vp", c.kw, c.x0, c.score, ts, c.G, n_probes=c.L, probes=lambda e: pr)
    assert c.error(xT, d).max() > 10.0 * c.error(xH, dH).max()


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_hutchinson_is_unbiased_within_its_spread(sde):
    """one fresh Rademacher probe per evaluation, numpy's default_rng(11): |mean deviation from the exact-divergence
    run| <= 4 standard errors of its own spread"""
    n_pts, n = 256, 100
    c = Mode(sde, n_pts)
    ts, _ = R.grid(n + 1, EPS)
    rng = np.random.default_rng(11)
    _, d_exact = LL.integrate_exact("ode_heun", sde, c.kw, c.x0, c.score, c.trace, ts, c.G)
    _, d = LL.integrate("ode_heun", sde, c.kw, c.x0, c.score, ts, c.G, n_probes=1,
                        probes=lambda e: rng.choice([-1.0, 1.0], (1, n_pts, c.L, 1)).astype(np.float32))
    dev = d - d_exact
    se = dev.std(ddof=1) / math.sqrt(n_pts)
    print(f"{sde}: Hutchinson rms {math.sqrt((dev ** 2).mean()):.3f} nats, mean deviation {dev.mean() / se:+.2f} standard errors")
    assert abs(dev.mean()) <= 4.0 * se
    assert 0.05 < math.sqrt((dev ** 2).mean()) < 0.5  # (0.19 VP, 0.24 VE)


def test_prior_restatement_is_the_gaussian_log_density():
    rng = np.random.default_rng(0)
    for sde in ("vp", "ve"):
        kw = M.sde_kwargs(sde)
        G = M.fourier_G(20)
        sp = kw["sigma_max"] if sde == "ve" else 1.0
        x = sp * rng.standard_normal((3, 20, 2))
        var = (sp * G.astype(np.float64)[None, :, None]) ** 2
        want = (-0.5 * x * x / var - 0.5 * np.log(2.0 * math.pi * var)).reshape(3, -1).sum(-1)
        assert np.allclose(LL.prior_logp(sde, kw, x, G), want, rtol=1e-13)
        assert np.abs(LL.prior_logp(sde, kw, x, G, np.float32) - want).max() < 2e-6 * np.abs(want).max()


def test_split_runs_of_the_restatement_agree():
    c = Mode("vp", 3)
    ts, _ = R.grid(7, EPS)
    whole = LL.integrate("ode_heun", "vp", c.kw, c.x0, c.score, ts, c.G, n_probes=2, seed=9, sample_offset=4)
    x, d = LL.integrate("ode_heun", "vp", c.kw, c.x0, c.score, ts, c.G, n_probes=2, seed=9, sample_offset=4, n_run=2)
    x, d = LL.integrate("ode_heun", "vp", c.kw, x, c.score, ts, c.G, n_probes=2, seed=9, sample_offset=4, first=2, delta=d)
    assert np.array_equal(whole[0], x) and np.array_equal(whole[1], d)
