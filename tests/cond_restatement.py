"""Numpy restatement of conditional sampling by replacement (support module of test_cond_host.py / test_cond_gpu.py).

Song et al. 2021, Appendix I.2 (score_sde's ``get_inpaint_update_fn``): after every state update of a predictor-corrector
step at time t the observation, noised to the forward SDE's marginal at t,

    y_t = mc obs + (sigma G_l) z
    VP: lmc = -0.25 t^2 (b - a) - 0.5 t a, mc = exp(lmc), sigma = sqrt(-expm1(2 lmc));   VE: mc = 1, sigma = a (b / a)^t
    noiseless: mc = 1, sigma = 0

replaces the observed part of the state.  The mask lives on the time axis; libffd blends in difference form
(include/ffd.h, ffd_cond_project):

    frequency domain:  x <- x + dft( mask (.) idft( (y_t - x) (.) std ) ) / std       (x, obs: packed ortho spectra)
    time domain:       x <- x + mask (.) (y_t - x)

``dft`` / ``idft`` are ``np.fft.rfft`` / ``irfft`` with ``norm="ortho"`` in the reference's packing (fourier.py:8-94):
rows 0 .. L/2 hold Re X_k, the rows behind them Im X_k for k = 1 .. ceil(L/2) - 1.

``dtype=np.float64`` evaluates this in double precision.  ``dtype=np.float32`` follows libffd's operation order: the
coefficients rounded once from double, one fp32 rounding per product / sum (sg = sigma G, y = mc obs + sg z, d = y - x,
d std; w = idft / sqrt(L) rounded, m = mask w; X rounded, X / std, x + X).  The transforms themselves run in numpy's
float64 and are rounded to fp32 where the kernel holds fp32 values, so the butterflies' own rounding (a few 1e-7 of the
max-norm) is not restated.  x, obs, mask and z are (B, L, C) (obs and mask may be (1, L, C)); G is (L,); std (L, C).
"""
import math

import numpy as np

import pc_restatement as P
from ode_restatement import DATA_STD, fourier_G, grid, rel_max_err  # noqa: F401  (re-exported helpers)

DOMAINS = ("frequency", "time")
TAG0 = 0xC0000000


def dft(x, dtype=np.float64):
    x = np.asarray(x, np.float64)
    L = x.shape[1]
    X = np.fft.rfft(x, axis=1, norm="ortho")
    return np.concatenate([X.real, X.imag[:, 1:(L + 1) // 2]], axis=1).astype(dtype)


def idft(xf, dtype=np.float64):
    xf = np.asarray(xf, np.float64)
    L = xf.shape[1]
    n_re = L // 2 + 1
    im = np.zeros_like(xf[:, :n_re])
    im[:, 1:1 + (L - n_re)] = xf[:, n_re:]
    return np.fft.irfft(xf[:, :n_re] + 1j * im, n=L, axis=1, norm="ortho").astype(dtype)


def coefficients(sde, sde_kwargs, t, noiseless=False):
    """(mc, sigma) in double."""
    if noiseless:
        return 1.0, 0.0
    t = float(t)
    if sde == "vp":
        a, b = sde_kwargs["beta_min"], sde_kwargs["beta_max"]
        lmc = -0.25 * t * t * (b - a) - 0.5 * t * a
        return math.exp(lmc), math.sqrt(-math.expm1(2.0 * lmc))
    a, b = sde_kwargs["sigma_min"], sde_kwargs["sigma_max"]
    return 1.0, a * (b / a) ** t


def noised_observation(sde, sde_kwargs, t, obs, z, G, noiseless=False, dtype=np.float64):
    dt = np.dtype(dtype).type
    mc, sigma = coefficients(sde, sde_kwargs, t, noiseless)
    obs = np.asarray(obs, dtype)
    if noiseless:
        return obs
    sg = dt(sigma) * np.asarray(G, dtype)[None, :, None]
    return dt(mc) * obs + sg * np.asarray(z, dtype)


def project(sde, sde_kwargs, t, x, obs, mask, z, G, std=None, domain="frequency", noiseless=False, dtype=np.float64):
    """One replacement step; z is ignored when ``noiseless``."""
    assert domain in DOMAINS and not (domain == "time" and std is not None)
    x = np.asarray(x, dtype)
    mask = np.asarray(mask, dtype)
    y = noised_observation(sde, sde_kwargs, t, obs, z, G, noiseless, dtype)
    d = y - x
    if domain == "time":
        return x + mask * d
    if std is not None:
        std = np.asarray(std, dtype)[None]
        d = d * std
    w = idft(d, dtype)
    X = dft(mask * w, dtype)
    if std is not None:
        X = X / std
    return x + X


def cond_integrate(sde, sde_kwargs, x, score_fn, noise_fn, ts, step_size, G, n_corrector, snr, obs, mask, std=None,
                   domain="frequency", final_replace=True, norm="batch", dtype=np.float64, first=0, n_run=None):
    """Reverse steps [first, first + n_run) of the grid ``ts``: the predictor-corrector step of pc_restatement with one
    projection at t_i behind every update.  ``score_fn(x, t, k)`` as there; ``noise_fn(i, k, p)`` is the draw of update k
    of step i (p = 0) or of its projection (p = 1).  ``final_replace``: a noiseless projection after the grid's last
    step."""
    n_run = len(ts) - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    for i in range(first, first + n_run):
        t = float(ts[i])
        for k in range(n_corrector + 1):
            s = score_fn(x, t, k)
            if k < n_corrector:
                x, _ = P.langevin_step(sde, sde_kwargs, t, x, s, noise_fn(i, k, 0), G, step_size, snr, norm, dtype)
            else:
                x = P.em_step(sde, sde_kwargs, t, x, s, noise_fn(i, k, 0), G, step_size, dtype)
            x = project(sde, sde_kwargs, t, x, obs, mask, noise_fn(i, k, 1), G, std, domain, False, dtype)
    if final_replace and n_run > 0 and first + n_run == len(ts):
        x = project(sde, sde_kwargs, float(ts[-1]), x, obs, mask, None, G, std, domain, True, dtype)
    return x


# ---- the analytic case: data WHITE IN TIME, N(0, DATA_STD^2) per time point.  Its packed ortho spectrum has variance
# DATA_STD^2 G_l^2 with the Fourier G, so the marginal at t is N(0, v(t) G_l^2), v = mc^2 DATA_STD^2 + sigma^2, in the
# spectrum and white N(0, v(t)) in time: observed and unobserved time points are independent at every t, replacement
# sampling is exact, and the unobserved points of a sample end with variance DATA_STD^2 (up to the discretisation). ----
GAUSS_L, GAUSS_SAMPLES, GAUSS_STEPS, GAUSS_SNR, GAUSS_PREFIX = 20, 4096, 150, 0.16, 8


def white_var(sde, sde_kwargs, t, G, s=DATA_STD):
    mc, sigma = coefficients(sde, sde_kwargs, t)
    G = np.asarray(G, np.float64)
    return (mc * mc * s * s + sigma * sigma) * G * G


def white_score(sde, sde_kwargs, G, s=DATA_STD):
    return lambda x, t, k=0: -np.asarray(x, np.float64) / white_var(sde, sde_kwargs, t, G, s)[None, :, None]


def gaussian_series(L=GAUSS_L, seed=100):
    """the fixed series the analytic case conditions on, (1, L, 1), and its prefix mask"""
    series = DATA_STD * np.random.default_rng(seed).standard_normal((1, L, 1))
    mask = np.zeros((1, L, 1))
    mask[:, :GAUSS_PREFIX] = 1.0
    return series, mask


def gaussian_conditional(sde, sde_kwargs, seed, n_corrector=1, L=GAUSS_L, n=GAUSS_SAMPLES, steps=GAUSS_STEPS,
                         snr=GAUSS_SNR, final_replace=True):
    """Run the float64 restatement on its own draws; returns (time-domain samples (n, L, 1), series, mask)."""
    rng = np.random.default_rng(seed)
    G = fourier_G(L).astype(np.float64)
    ts, h = grid(steps)
    series, mask = gaussian_series(L)
    obs = dft(series * mask)
    prior_scale = sde_kwargs["sigma_max"] if sde == "ve" else 1.0
    x = prior_scale * G[None, :, None] * rng.standard_normal((n, L, 1))
    x = cond_integrate(sde, sde_kwargs, x, white_score(sde, sde_kwargs, G), lambda i, k, p: rng.standard_normal((n, L, 1)),
                       ts, h, G, n_corrector, snr, obs, mask, final_replace=final_replace)
    return idft(x), series, mask


def unobserved_stats(xt, mask):
    """(mean over unobserved positions of sample variance / DATA_STD^2, largest |position mean| in standard errors)"""
    free = np.asarray(mask)[0, :, 0] == 0
    v = np.asarray(xt, np.float64)[:, free, 0]
    ratio = float((v.var(axis=0) / DATA_STD ** 2).mean())
    se = v.std(axis=0) / math.sqrt(v.shape[0])
    return ratio, float(np.abs(v.mean(axis=0) / se).max())
