"""Numpy restatement of the linear multistep ODE solvers (support module of test_multistep_host.py /
test_multistep_gpu.py): ``ode_ab2`` (Adams-Bashforth 2 on the probability-flow drift) and ``dpmpp_2m`` (DPM-Solver++ 2M,
the exponential two-step form on the data prediction).  One score evaluation per interval, second order.

Both are one operation.  With the interval's *history quantity*

    q = qa x + qb G_l^2 s

(the drift d(x, t) of ode_restatement for AB2, the data prediction (x + sigma^2 G_l^2 s) / alpha for DPM++) the update is

    x <- x + (cxm1 x + cn q + cp q_prev),    hist <- q

and the solvers differ in the five coefficients (qa, qb, cxm1, cn, cp) alone:

    ode_ab2   qa = a(t), qb = -cs(t)^2 / 2 (``ode_restatement.coefficients``), cxm1 = 0,
              cn = -1.5 h, cp = 0.5 h with history; cn = -h, cp = 0 without (an Euler interval); h = step_size
    dpmpp_2m  alpha, sigma of the marginal at t (without G), lambda = log(alpha / sigma), h = lambda(t_next) - lambda(t),
              r = (lambda(t) - lambda(t_prev)) / h, c = -alpha(t_next) expm1(-h):
              qa = 1 / alpha, qb = sigma^2 / alpha, cxm1 = sigma(t_next) / sigma(t) - 1,
              cn = c (1 + 1 / (2 r)), cp = -c / (2 r) with history; cn = c, cp = 0 without

``coefficients`` evaluates them in float64 (expm1 / log1p where near-equal numbers would be subtracted).
``dtype=np.float64`` steps with them as they are; ``dtype=np.float32`` follows libffd's operation order, the coefficients
rounded once and every product / sum its own fp32 rounding:

    g2 = G G, u = g2 s, q = (qa x) + (qb u), inc = (cxm1 x) + (cn q), [inc = inc + (cp q_prev)], x = x + inc.

x, the score and the history are (B, L, C); G is (L,).
"""
import math

import numpy as np

import ode_restatement as O
from ode_restatement import (DATA_STD, fourier_G, gaussian_exact, gaussian_score, gaussian_start, gaussian_var,  # noqa: F401
                             grid, rel_max_err)

METHODS = ("ode_ab2", "dpmpp_2m")


def log_alpha_sigma(sde, sde_kwargs, t):
    """(log alpha, log sigma) of the forward marginal at t, in double."""
    t = float(t)
    if sde == "vp":
        b0, b1 = sde_kwargs["beta_min"], sde_kwargs["beta_max"]
        la = -0.25 * t * t * (b1 - b0) - 0.5 * t * b0
        return la, 0.5 * math.log(-math.expm1(2.0 * la))
    lo, hi = sde_kwargs["sigma_min"], sde_kwargs["sigma_max"]
    return 0.0, math.log(lo) + t * math.log(hi / lo)


def coefficients(method, sde, sde_kwargs, t, t_next, step_size, t_prev=None):
    """(qa, qb, cxm1, cn, cp) in double; ``t_prev=None``: the first interval of a trajectory (no history)."""
    assert method in METHODS
    if method == "ode_ab2":
        a, cs = O.coefficients(sde, sde_kwargs, t)
        h = float(step_size)
        cn, cp = (-h, 0.0) if t_prev is None else (-1.5 * h, 0.5 * h)
        return a, -0.5 * cs * cs, 0.0, cn, cp
    la, ls = log_alpha_sigma(sde, sde_kwargs, t)
    lan, lsn = log_alpha_sigma(sde, sde_kwargs, t_next)
    h = (lan - lsn) - (la - ls)
    c = -math.exp(lan) * math.expm1(-h)
    if t_prev is None:
        cn, cp = c, 0.0
    else:
        lap, lsp = log_alpha_sigma(sde, sde_kwargs, t_prev)
        r = ((la - ls) - (lap - lsp)) / h
        cn, cp = c * (1.0 + 1.0 / (2.0 * r)), -c / (2.0 * r)
    return math.exp(-la), math.exp(2.0 * ls - la), math.expm1(lsn - ls), cn, cp


def step(coef, x, score, G, hist=None, dtype=np.float64):
    """(x_new, q): one interval with the five coefficients ``coef``; ``hist=None`` takes the first-interval form."""
    f = np.dtype(dtype).type
    qa, qb, cxm1, cn, cp = (f(v) for v in coef)
    x, score = np.asarray(x, dtype), np.asarray(score, dtype)
    Gl = np.asarray(G, dtype)[None, :, None]
    g2 = Gl * Gl
    u = g2 * score
    q = qa * x + qb * u
    inc = cxm1 * x + cn * q
    if hist is not None:
        inc = inc + cp * np.asarray(hist, dtype)
    else:
        assert float(cp) == 0.0
    return x + inc, q


def integrate(method, sde, sde_kwargs, x, score_fn, ts, step_size, G, dtype=np.float64, first=0, n_run=None, hist=None):
    """Walk intervals [first, first + n_run) of the grid ``ts`` (default: all len(ts) - 1) with one evaluation
    ``score_fn(x, t, 0)`` per interval.  ``hist``: the history a trajectory continued at ``first`` > 0 brings along;
    None starts without.  Returns x (``integrate_with_history``: also the last q)."""
    return integrate_with_history(method, sde, sde_kwargs, x, score_fn, ts, step_size, G, dtype, first, n_run, hist)[0]


def integrate_with_history(method, sde, sde_kwargs, x, score_fn, ts, step_size, G, dtype=np.float64, first=0, n_run=None,
                           hist=None):
    n_run = len(ts) - 1 - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    for i in range(first, first + n_run):
        t_prev = float(ts[i - 1]) if hist is not None else None
        coef = coefficients(method, sde, sde_kwargs, float(ts[i]), float(ts[i + 1]), step_size, t_prev)
        x, hist = step(coef, x, score_fn(x, float(ts[i]), 0), G, hist, dtype)
    return x, hist


# ---- the delta-data case: every sample is x0, so x_t = alpha x0 + sigma G eps and the score is linear in x ----
def delta_score(sde, sde_kwargs, G, x0):
    G2 = (np.asarray(G, np.float64) ** 2)[None, :, None]

    def fn(x, t, k=0):
        la, ls = log_alpha_sigma(sde, sde_kwargs, t)
        return -(np.asarray(x, np.float64) - math.exp(la) * x0) / (math.exp(2.0 * ls) * G2)

    return fn


def delta_exact(sde, sde_kwargs, x_start, t_start, t_end, x0):
    """The ODE's flow map on the delta case: the noise part of x scales with sigma, the data part with alpha."""
    la0, ls0 = log_alpha_sigma(sde, sde_kwargs, t_start)
    la1, ls1 = log_alpha_sigma(sde, sde_kwargs, t_end)
    return math.exp(la1) * x0 + math.exp(ls1 - ls0) * (np.asarray(x_start, np.float64) - math.exp(la0) * x0)
