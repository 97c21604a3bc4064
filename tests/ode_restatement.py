"""Numpy restatement of the probability-flow ODE solvers (support module of test_ode_host.py / test_ode_gpu.py).

Forward SDE  dx = f(x,t) dt + g(t) diag(G) dw  with  f = -beta(t) x / 2 (VP), 0 (VE);  g = sqrt(beta(t)) (VP), the
reference's ``sqrt_derivative`` (VE).  Probability-flow drift

    d(x, t) = f(x, t) - (g(t) G_l)^2 s(x, t) / 2

and one interval from t_i down to t_{i+1} = t_i - dt:

    euler:  x <- x - d(x, t_i) dt
    heun :  d1 = d(x, t_i);  xp = x - d1 dt;  d2 = d(xp, t_{i+1});  x <- x - ((d1 + d2) / 2) dt

``dtype=np.float64`` evaluates this in double precision; ``dtype=np.float32`` follows libffd's operation order with one
fp32 rounding per product / sum (g = cs G, g2 = g g, gs = g2 s, hgs = 0.5 gs, d = a x - hgs), the coefficients a and
cs rounded from their double values as ``sde_params`` does.  x and the score are (B, L, C); G is (L,).
"""
import math

import numpy as np


def coefficients(sde, sde_kwargs, t):
    """(a, cs) in double: f = a x and g = cs at time t."""
    t = float(t)
    if sde == "vp":
        beta = sde_kwargs["beta_min"] + t * (sde_kwargs["beta_max"] - sde_kwargs["beta_min"])
        return -0.5 * beta, math.sqrt(beta)
    lo, hi = sde_kwargs["sigma_min"], sde_kwargs["sigma_max"]
    return 0.0, lo * math.sqrt(2.0 * math.log(hi / lo)) * (hi / lo) ** t


def drift(sde, sde_kwargs, t, x, score, G, dtype=np.float64):
    a, cs = coefficients(sde, sde_kwargs, t)
    dt = np.dtype(dtype).type
    x, score = np.asarray(x, dtype), np.asarray(score, dtype)
    g = dt(cs) * np.asarray(G, dtype)[None, :, None]
    g2 = g * g
    gs = g2 * score
    hgs = dt(0.5) * gs
    return dt(a) * x - hgs if sde == "vp" else -hgs


def euler_step(sde, sde_kwargs, t, x, score, G, step_size, dtype=np.float64):
    d = drift(sde, sde_kwargs, t, x, score, G, dtype)
    return np.asarray(x, dtype) - d * np.dtype(dtype).type(step_size)


def heun_predict(sde, sde_kwargs, t, x, score, G, step_size, dtype=np.float64):
    """(xp, d1)"""
    d1 = drift(sde, sde_kwargs, t, x, score, G, dtype)
    return np.asarray(x, dtype) - d1 * np.dtype(dtype).type(step_size), d1


def heun_correct(sde, sde_kwargs, t_next, x, x_pred, score_pred, d1, G, step_size, dtype=np.float64):
    dt = np.dtype(dtype).type
    d2 = drift(sde, sde_kwargs, t_next, x_pred, score_pred, G, dtype)
    return np.asarray(x, dtype) - (dt(0.5) * (np.asarray(d1, dtype) + d2)) * dt(step_size)


def integrate(solver, sde, sde_kwargs, x, score_fn, ts, step_size, G, dtype=np.float64, first=0, n_run=None):
    """Walk intervals [first, first + n_run) of the grid ``ts`` (default: all len(ts) - 1).  ``score_fn(x, t, k)`` returns
    the score at (x, t); k = 0 for the evaluation at an interval's start, 1 for Heun's second one."""
    assert solver in ("ode_euler", "ode_heun")
    n_run = len(ts) - 1 - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    for i in range(first, first + n_run):
        t, tn = float(ts[i]), float(ts[i + 1])
        s = score_fn(x, t, 0)
        if solver == "ode_euler":
            x = euler_step(sde, sde_kwargs, t, x, s, G, step_size, dtype)
        else:
            xp, d1 = heun_predict(sde, sde_kwargs, t, x, s, G, step_size, dtype)
            x = heun_correct(sde, sde_kwargs, tn, x, xp, score_fn(xp, tn, 1), d1, G, step_size, dtype)
    return x


# ---- the analytic case: data N(0, s^2) per coordinate, so every marginal is Gaussian and the score is -x / var(t) ----
DATA_STD = 1.5


def gaussian_var(sde, sde_kwargs, t, G, s=DATA_STD):
    """Variance per position (L,) of the marginal at time t."""
    G = np.asarray(G, np.float64)
    if sde == "vp":
        b0, b1 = sde_kwargs["beta_min"], sde_kwargs["beta_max"]
        m2 = math.exp(2.0 * (-0.25 * t * t * (b1 - b0) - 0.5 * t * b0))
        return m2 * s * s + (1.0 - m2) * G * G
    sigma = sde_kwargs["sigma_min"] * (sde_kwargs["sigma_max"] / sde_kwargs["sigma_min"]) ** t
    return s * s + sigma * sigma * G * G


def gaussian_score(sde, sde_kwargs, G, s=DATA_STD):
    return lambda x, t, k=0: -np.asarray(x, np.float64) / gaussian_var(sde, sde_kwargs, t, G, s)[None, :, None]


def gaussian_exact(sde, sde_kwargs, x_start, t_start, t_end, G, s=DATA_STD):
    """The ODE's exact flow map between two times: x sqrt(var(t_end) / var(t_start))."""
    r = np.sqrt(gaussian_var(sde, sde_kwargs, t_end, G, s) / gaussian_var(sde, sde_kwargs, t_start, G, s))
    return np.asarray(x_start, np.float64) * r[None, :, None]


def fourier_G(L):
    """SDE.set_noise_scaling with fourier_noise_scaling=True, in the reference's fp32 operation order."""
    G = np.full(L, np.float32(1.0 / math.sqrt(2.0)), np.float32)
    G[0] = np.float32(G[0] * np.float32(math.sqrt(2.0)))
    if L % 2 == 0:
        G[L // 2] = np.float32(G[L // 2] * np.float32(math.sqrt(2.0)))
    return G


def gaussian_start(L=20, n=4, seed=0):
    """The start samples of the analytic case: n draws of N(0, 1) per coordinate, (n, L, 1)."""
    return np.random.default_rng(seed).standard_normal((n, L, 1))


def grid(N, eps=1e-5):
    """fp32 linspace(1, eps, N) and its fp32 step size, as SDE.set_timesteps makes them."""
    import torch

    ts = torch.linspace(1.0, eps, N)
    return ts.numpy().copy(), float(ts[0] - ts[1])


def rel_max_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())
