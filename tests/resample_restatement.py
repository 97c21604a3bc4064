"""Numpy restatement of resampled conditional sampling (support module of test_resample_host.py / test_resample_gpu.py).

"Time travel" (RePaint, Lugmayr et al. 2022) on top of conditional sampling by replacement (cond_restatement.py): the N
reverse steps of the grid are cut into blocks [0, j), [j, 2j), ... (the last may be shorter, j > N is one block), every
block is run r times, and between two passes of the block [i0, e) the whole state is diffused FORWARD from
s = ts[e] (0 when e == N) to t = ts[i0] with the SDE's exact transition kernel (include/ffd.h, ffd_forward_transition):

    x_t = a x_s + (sg G_l) z
    VP: a = exp(lmc(t) - lmc(s)), sg = sqrt(-expm1(2 (lmc(t) - lmc(s))));   VE: a = 1, sg = sqrt(sigma(t)^2 - sigma(s)^2)

with lmc and sigma as in cond_restatement.coefficients.  No projection follows a transition.  U = r N visits,
(r - 1) ceil(N / j) transitions; a transition belongs to the visit it follows.

``dtype=np.float64`` evaluates this in double precision.  ``dtype=np.float32`` follows libffd's operation order: the
coefficients rounded once from double, then x' = (a x) + ((sg G) z) with one fp32 rounding per product / sum; with a
rounded sg of 0 no draw is used and x' = a x, and with a == 1 as well x is returned as it is.
"""
import math

import numpy as np

import cond_restatement as CR
import mixture_restatement as MR
from cond_restatement import DATA_STD, dft, fourier_G, grid, idft, rel_max_err  # noqa: F401  (re-exported helpers)

TAG0 = 0xE0000000


def transition_coefficients(sde, sde_kwargs, s, t):
    """(a, sg) in double, the operations in ffd_host_transition_coef's order."""
    s, t = float(s), float(t)
    assert 0.0 <= s <= t
    if s == t:
        return 1.0, 0.0
    if sde == "vp":
        a, b = sde_kwargs["beta_min"], sde_kwargs["beta_max"]
        lt = -0.25 * t * t * (b - a) - 0.5 * t * a
        ls = -0.25 * s * s * (b - a) - 0.5 * s * a
        d = lt - ls
        return math.exp(d), math.sqrt(-math.expm1(2.0 * d))
    a, b = sde_kwargs["sigma_min"], sde_kwargs["sigma_max"]
    st = a * math.pow(b / a, t)
    ss = a * math.pow(b / a, s)
    vt = st * st
    vs = ss * ss
    return 1.0, math.sqrt(max(vt - vs, 0.0))


def forward_transition(sde, sde_kwargs, s, t, x, z, G, dtype=np.float64):
    dt = np.dtype(dtype).type
    a, sg = transition_coefficients(sde, sde_kwargs, s, t)
    x = np.asarray(x, dtype)
    if dt(sg) == 0:
        return x if dt(a) == 1 else dt(a) * x
    return dt(a) * x + (dt(sg) * np.asarray(G, dtype)[None, :, None]) * np.asarray(z, dtype)


def visits(n_steps, jump, resample):
    """The schedule as a list of (grid index, back_to): back_to = -1, or the index the state is re-noised to after the
    visit.  Written as the loops the text above describes (libffd computes a visit in closed form)."""
    assert n_steps >= 1 and jump >= 1 and resample >= 1
    out = []
    for i0 in range(0, n_steps, jump):
        e = min(i0 + jump, n_steps)
        for p in range(resample):
            for i in range(i0, e):
                out.append((i, i0 if i == e - 1 and p < resample - 1 else -1))
    return out


def n_slabs(n_steps, jump, resample, n_corrector, first=0, n_run=None):
    """(B, L, C) slabs of injected noise that visits [first, first + n_run) consume."""
    sched = visits(n_steps, jump, resample)
    n_run = len(sched) - first if n_run is None else n_run
    return sum(2 * (n_corrector + 1) + (b >= 0) for _, b in sched[first:first + n_run])


def flat_noise(zs, n_steps, jump, resample, n_corrector):
    """(noise_fn(u, k, p), transition_noise_fn(u)) reading the flat list ``zs`` in libffd's execution order."""
    sched = visits(n_steps, jump, resample)
    start = np.concatenate([[0], np.cumsum([2 * (n_corrector + 1) + (b >= 0) for _, b in sched])])
    return (lambda u, k, p: zs[start[u] + 2 * k + p]), (lambda u: zs[start[u] + 2 * (n_corrector + 1)])


def resample_integrate(sde, sde_kwargs, x, score_fn, noise_fn, transition_noise_fn, ts, step_size, G, n_corrector, snr, obs,
                       mask, jump, resample, std=None, domain="frequency", final_replace=True, norm="batch",
                       dtype=np.float64, first=0, n_run=None):
    """Visits [first, first + n_run) of the schedule.  A visit is one step of ``cond_restatement.cond_integrate`` at its
    grid index; ``noise_fn(u, k, p)`` is the draw of update k of VISIT u (p = 0) or of its projection (p = 1),
    ``transition_noise_fn(u)`` the draw of the transition behind visit u.  ``final_replace``: a noiseless projection
    after the schedule's last visit."""
    sched = visits(len(ts), jump, resample)
    n_run = len(sched) - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    for u in range(first, first + n_run):
        i, back_to = sched[u]
        x = CR.cond_integrate(sde, sde_kwargs, x, score_fn, lambda _i, k, p: noise_fn(u, k, p), ts, step_size, G, n_corrector,
                              snr, obs, mask, std, domain, False, norm, dtype, first=i, n_run=1)
        if back_to >= 0:
            s = float(ts[i + 1]) if i + 1 < len(ts) else 0.0
            x = forward_transition(sde, sde_kwargs, s, float(ts[back_to]), x, transition_noise_fn(u), G, dtype)
    if final_replace and n_run > 0 and first + n_run == len(sched):
        x = CR.project(sde, sde_kwargs, float(ts[-1]), x, obs, mask, None, G, std, domain, True, dtype)
    return x


# ---- the analytic white-data case of cond_restatement under the resampled loop: replacement is exact there, so
# resampling must leave the statistics where they are ----
WHITE_STEPS, WHITE_RESAMPLE, WHITE_JUMP = 50, 3, 2  # 150 visits: the cost of cond_restatement's 150-step case


def gaussian_conditional(sde, sde_kwargs, seed, jump=WHITE_JUMP, resample=WHITE_RESAMPLE, n_corrector=1, L=CR.GAUSS_L,
                         n=CR.GAUSS_SAMPLES, steps=WHITE_STEPS, snr=CR.GAUSS_SNR, final_replace=True):
    """``cond_restatement.gaussian_conditional`` through ``resample_integrate``: (time-domain samples, series, mask)."""
    rng = np.random.default_rng(seed)
    G = fourier_G(L).astype(np.float64)
    ts, h = grid(steps)
    series, mask = CR.gaussian_series(L)
    obs = dft(series * mask)
    prior_scale = sde_kwargs["sigma_max"] if sde == "ve" else 1.0
    x = prior_scale * G[None, :, None] * rng.standard_normal((n, L, 1))
    draw = lambda *a: rng.standard_normal((n, L, 1))  # noqa: E731  (consumed in execution order)
    x = resample_integrate(sde, sde_kwargs, x, CR.white_score(sde, sde_kwargs, G), draw, draw, ts, h, G, n_corrector, snr,
                           obs, mask, jump, resample, final_replace=final_replace)
    return idft(x), series, mask


# ---- the two-mode forecast: time domain, VP 0.1 / 20, L = 8, G = 1; four components with means +-1 on the first four
# points and +-1 on the last four, weights 0.45 (+ +), 0.05 (+ -), 0.05 (- +), 0.45 (- -), variance 0.05.  The first four
# points are observed at +1: the exact probability that the last four sit at +1 is 0.45 / (0.45 + 0.05) = 0.9.
# Replacement draws the noised prefix independently of the rest and undershoots it. ----
TWO_MODE_VP = {"beta_min": 0.1, "beta_max": 20.0}
TWO_MODE_L, TWO_MODE_PREFIX, TWO_MODE_SAMPLES, TWO_MODE_EXACT = 8, 4, 4000, 0.9


def two_mode_mixture():
    """(means (4, 8, 1), log-weights (4,), variance (8, 1)) as fp32, and the observation / prefix mask (1, 8, 1)."""
    mu = np.zeros((4, TWO_MODE_L, 1), np.float32)
    for i, (head, tail) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        mu[i, :TWO_MODE_PREFIX, 0], mu[i, TWO_MODE_PREFIX:, 0] = head, tail
    log_w = np.log(np.array([0.45, 0.05, 0.05, 0.45])).astype(np.float32)
    var = np.full((TWO_MODE_L, 1), 0.05, np.float32)
    obs = np.ones((1, TWO_MODE_L, 1), np.float32)
    mask = np.zeros((1, TWO_MODE_L, 1), np.float32)
    mask[:, :TWO_MODE_PREFIX] = 1.0
    return mu, log_w, var, obs, mask


def right_mode_fraction(x):
    """The fraction of completions whose last four points sit at the +1 mode."""
    return float((np.asarray(x, np.float64)[:, TWO_MODE_PREFIX:, 0].mean(axis=1) > 0).mean())


def two_mode_run(seed, steps, resample=1, jump=1, n_corrector=0, snr=0.16, n=TWO_MODE_SAMPLES):
    """The float64 run on numpy draws; returns the right-mode fraction."""
    mu, log_w, var, obs, mask = two_mode_mixture()
    G = np.ones(TWO_MODE_L)
    ts, h = grid(steps)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, TWO_MODE_L, 1))
    draw = lambda *a: rng.standard_normal((n, TWO_MODE_L, 1))  # noqa: E731
    x = resample_integrate("vp", TWO_MODE_VP, x, MR.score_fn("vp", TWO_MODE_VP, mu, log_w, var, G), draw, draw, ts, h, G,
                           n_corrector, snr, obs, mask, jump, resample, domain="time")
    return right_mode_fraction(x)
