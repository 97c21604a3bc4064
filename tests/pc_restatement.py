"""Numpy restatement of predictor-corrector sampling (support module of test_pc_host.py / test_pc_gpu.py).

Forward SDE  dx = f(x,t) dt + g(t) diag(G) dw  as in ode_restatement.py.  One Langevin corrector step at time t on sample
b with the score s and a draw z ~ N(0, I) (include/ffd.h, ffd_langevin_step):

    u = G_l^2 s,  w = G_l z,  n_u[b] = ||u[b]||,  n_w[b] = ||w[b]||
    eps[b] = 2 alpha (snr n_w[b] / n_u[b])^2                   norm = "sample"
    eps[b] = 2 alpha (snr mean_b(n_w) / mean_b(n_u))^2         norm = "batch"
    x <- x + eps[b] u + sqrt(2 eps[b]) w
    alpha = 1 (VE), max(1 - beta(t) step_size, 0) (VP);  n_u == 0: eps = 0

and one reverse step i of the sampler is n_corrector of these at t_i, each on its own score evaluation, followed by the
Euler-Maruyama predictor at t_i on another one.

``dtype=np.float64`` evaluates this in double precision.  ``dtype=np.float32`` follows libffd's operation order: one fp32
rounding per product / sum (g2 = G G, u = g2 s, w = G z, x' = (x + eps u) + se w), the norms from the fp32 squares
summed in float64, eps rounded once to fp32 and se = fp32(sqrt(2 eps)) from the rounded eps.  (The float64 sums here
run in numpy's order, the device's in its fixed tree: the difference is far below the fp32 rounding of eps.)
x, the score and z are (B, L, C); G is (L,).
"""
import numpy as np

import ode_restatement as R
from ode_restatement import DATA_STD, fourier_G, gaussian_var, grid, rel_max_err  # noqa: F401  (re-exported helpers)

NORMS = ("batch", "sample")


def alpha(sde, sde_kwargs, t, step_size):
    if sde != "vp":
        return 1.0
    beta = sde_kwargs["beta_min"] + float(t) * (sde_kwargs["beta_max"] - sde_kwargs["beta_min"])
    return max(1.0 - beta * float(step_size), 0.0)


def langevin_step(sde, sde_kwargs, t, x, score, z, G, step_size, snr, norm="batch", dtype=np.float64, _noise_factor=2.0,
                  _g_power=2):
    """(x', eps (B,) float64 holding the values the update used).  ``_noise_factor`` / ``_g_power`` exist for the host
    test's deliberately wrong variants (noise sqrt(_noise_factor eps), u = G^_g_power s)."""
    assert norm in NORMS
    x, score, z = (np.asarray(a, dtype) for a in (x, score, z))
    Gc = np.asarray(G, dtype)[None, :, None]
    g2 = Gc * Gc if _g_power == 2 else Gc ** _g_power
    u = g2 * score
    w = Gc * z
    B = x.shape[0]
    n_u = np.sqrt((u * u).astype(np.float64).reshape(B, -1).sum(axis=1))
    n_w = np.sqrt((w * w).astype(np.float64).reshape(B, -1).sum(axis=1))
    if norm == "batch":
        n_u = np.full(B, n_u.sum() / B)
        n_w = np.full(B, n_w.sum() / B)
    a = alpha(sde, sde_kwargs, t, step_size)
    eps = np.zeros(B, np.float64)
    ok = n_u > 0
    r = (float(snr) * n_w[ok]) / n_u[ok]
    eps[ok] = (2.0 * a) * (r * r)
    eps = eps.astype(dtype).astype(np.float64)  # fp32: rounded once
    se = np.sqrt(_noise_factor * eps).astype(dtype)
    e = eps.astype(dtype)[:, None, None]
    out = (x + e * u) + se[:, None, None] * w
    out[eps == 0] = x[eps == 0]  # such a sample is not touched
    return out, eps


def em_step(sde, sde_kwargs, t, x, score, z, G, step_size, dtype=np.float64):
    """The reverse Euler-Maruyama step in the reference's operation order (oracle.ffd_oracle.vp_step / ve_step)."""
    dt = np.dtype(dtype).type
    a, cs = R.coefficients(sde, sde_kwargs, t)
    x, score, z = (np.asarray(v, dtype) for v in (x, score, z))
    g = dt(cs) * np.asarray(G, dtype)[None, :, None]
    gs = (g * g) * score
    drift = dt(a) * x - gs if sde == "vp" else -gs
    h = dt(step_size)
    return (x - drift * h) + np.sqrt(h) * (g * z)


def pc_integrate(sde, sde_kwargs, x, score_fn, noise_fn, ts, step_size, G, n_corrector, snr, norm="batch",
                 dtype=np.float64, first=0, n_run=None):
    """Reverse steps [first, first + n_run) of the grid ``ts`` (default: all).  ``score_fn(x, t, k)`` returns the k-th
    score evaluation of a step (k = 0 .. n_corrector; the last one is the predictor's), ``noise_fn(i, k)`` the draw
    that evaluation's update consumes."""
    n_run = len(ts) - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    for i in range(first, first + n_run):
        t = float(ts[i])
        for k in range(n_corrector):
            x, _ = langevin_step(sde, sde_kwargs, t, x, score_fn(x, t, k), noise_fn(i, k), G, step_size, snr, norm, dtype)
        x = em_step(sde, sde_kwargs, t, x, score_fn(x, t, n_corrector), noise_fn(i, n_corrector), G, step_size, dtype)
    return x


# ---- the analytic case: data N(0, DATA_STD^2) per coordinate; the marginal at t is N(0, var_l(t)), score -x / var ----
GAUSS_T, GAUSS_L, GAUSS_SAMPLES, GAUSS_STEPS, GAUSS_SNR, GAUSS_N = 0.5, 20, 4096, 150, 0.16, 12


def gaussian_stationary_ratio(sde, sde_kwargs, seed, norm="batch", L=GAUSS_L, C=1, n=GAUSS_SAMPLES, steps=GAUSS_STEPS,
                              snr=GAUSS_SNR, **wrong):
    """Start n samples at the exact marginal of time GAUSS_T, run ``steps`` corrector steps on the analytic score and
    return (mean over positions of the sample variance / exact variance, the last step's mean eps)."""
    rng = np.random.default_rng(seed)
    G = fourier_G(L)
    var = gaussian_var(sde, sde_kwargs, GAUSS_T, G)[None, :, None]
    _, h = grid(GAUSS_N)
    x = rng.standard_normal((n, L, C)) * np.sqrt(var)
    eps = None
    for _ in range(steps):
        x, eps = langevin_step(sde, sde_kwargs, GAUSS_T, x, -x / var, rng.standard_normal(x.shape), G, h, snr, norm,
                               **wrong)
    ratio = (x * x).mean(axis=(0, 2)) / var[0, :, 0]
    return float(ratio.mean()), float(eps.mean())


def gaussian_expected_ratio(sde, sde_kwargs, eps, L=GAUSS_L):
    """x' = (1 - a_l) x + sqrt(2 eps) G_l z with a_l = eps G_l^2 / var_l has the stationary variance var_l / (1 - a_l / 2):
    the mean over positions of 1 / (1 - eps G_l^2 / (2 var_l))."""
    G = fourier_G(L).astype(np.float64)
    var = gaussian_var(sde, sde_kwargs, GAUSS_T, G)
    return float((1.0 / (1.0 - eps * G * G / (2.0 * var))).mean())
