"""Numpy restatement of the closed-form Gaussian-mixture score (support module of test_mixture_host.py /
test_mixture_gpu.py; include/ffd.h ffd_mixture_score).

Data distribution p_0 = sum_i w_i N(mu_i, diag(v)); forward marginal x_t = alpha(t) x_0 + sigma(t) G_l z:

    c_lc    = alpha^2 v_lc + sigma^2 G_l^2
    logit_i = log w_i - 1/2 sum_lc (x_lc - alpha mu_i,lc)^2 / c_lc
    r       = softmax_i(logit)
    d_lc    = alpha sum_i r_i mu_i,lc - x_lc            (the displacement)
    score   = d / c

``t`` is the fp32 grid value widened to double; alpha and sigma^2 are formed in float64 (VP: sigma^2 = -expm1(2 log
alpha)) and rounded once to ``dtype``.  ``form="difference"`` subtracts, then squares; ``form="expanded"`` evaluates
|x|^2 - 2 x . alpha mu + |alpha mu|^2 (the GEMM form, which cancels catastrophically at small t: kept to pin the reason
for the other one).  x (B, L, C), means (K, L, C), log_w (K), var (L, C) or None, G (L,), t a scalar or (B,).
"""
import math

import numpy as np

VP = {"beta_min": 0.1, "beta_max": 20.0}
VE = {"sigma_min": 0.01, "sigma_max": 50.0}
SHAPES = [(4, 8, 1, 3), (5, 20, 3, 17), (4, 187, 1, 70), (3, 33, 4, 130)]  # (B, L, C, K)
TIMES = [1.0, 0.5, 0.05, 1e-3, 1e-5]


def sde_kwargs(sde):
    return VP if sde == "vp" else VE


def alpha_sigma2(sde, kw, t):
    """(alpha, sigma^2) in double at the fp32 value of t; arrays for an array t."""
    t = np.asarray(np.asarray(t, np.float32), np.float64)
    if sde == "vp":
        la = -0.25 * t * t * (kw["beta_max"] - kw["beta_min"]) - 0.5 * t * kw["beta_min"]
        return np.exp(la), -np.expm1(2.0 * la)
    sg = kw["sigma_min"] * (kw["sigma_max"] / kw["sigma_min"]) ** t
    return np.ones_like(t), sg * sg


def fourier_G(L, fourier=True):
    G = np.ones(L, np.float32)
    if fourier:
        G = np.full(L, np.float32(1.0 / math.sqrt(2.0)), np.float32)
        G[0] = np.float32(G[0] * np.float32(math.sqrt(2.0)))
        if L % 2 == 0:
            G[L // 2] = np.float32(G[L // 2] * np.float32(math.sqrt(2.0)))
    return G


def _coeffs(sde, kw, t, B, var, G, L, C, dtype):
    al, s2 = alpha_sigma2(sde, kw, t)
    al = np.broadcast_to(np.asarray(al, dtype), (B,)).reshape(B, 1, 1)
    s2 = np.broadcast_to(np.asarray(s2, dtype), (B,)).reshape(B, 1, 1)
    v = np.zeros((L, C), dtype) if var is None else np.asarray(var, dtype)
    g = np.asarray(G, dtype).reshape(1, L, 1)
    c = (al * al) * v[None] + s2 * (g * g)
    return al, c.astype(dtype)


def evaluate(sde, kw, x, t, means, log_w, var, G, dtype=np.float64, form="difference"):
    """(score, d, c) in ``dtype``; c is (B, L, C)."""
    x = np.asarray(x, dtype)
    mu = np.asarray(means, dtype)
    lw = np.asarray(log_w, dtype)
    B, L, C = x.shape
    K = mu.shape[0]
    al, c = _coeffs(sde, kw, t, B, var, G, L, C, dtype)
    ic = (dtype(1.0) / c).astype(dtype)
    half = dtype(0.5)
    if form == "difference":
        diff = x[:, None] - al[:, None] * mu[None]                       # (B, K, L, C)
        q = (diff * (diff * ic[:, None])).reshape(B, K, -1).sum(-1, dtype=dtype)
    else:
        am = al[:, None] * mu[None]
        xx = (x * x * ic).reshape(B, -1).sum(-1, dtype=dtype)[:, None]
        xm = np.einsum("bj,bkj->bk", (x * ic).reshape(B, -1), am.reshape(B, K, -1)).astype(dtype)
        mm = (am * am * ic[:, None]).reshape(B, K, -1).sum(-1, dtype=dtype)
        q = (xx - dtype(2.0) * xm + mm).astype(dtype)
    with np.errstate(invalid="ignore"):
        logit = (lw[None] - half * q).astype(dtype)
    m = logit.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, dtype(0.0))
    p = np.exp(logit - m).astype(dtype)
    r = (p / p.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    mean = np.einsum("bk,kj->bj", r, mu.reshape(K, -1)).astype(dtype).reshape(B, L, C)
    d = (al * mean - x).astype(dtype)
    return (d * ic).astype(dtype), d, c


def score(sde, kw, x, t, means, log_w, var, G, dtype=np.float64, form="difference"):
    return evaluate(sde, kw, x, t, means, log_w, var, G, dtype, form)[0]


def score_fn(sde, kw, means, log_w, var, G, dtype=np.float64):
    """``score_fn(x, t, k)`` for ode_restatement.integrate and the pc / cond / multistep restatements."""
    return lambda x, t, k=0: score(sde, kw, x, t, means, log_w, var, G, dtype)


def log_pt(sde, kw, x, t, means, log_w, var, G):
    """log p_t(x) per row, float64 (log-weights need not be normalised: the constant drops out of the gradient)."""
    x = np.asarray(x, np.float64)
    mu = np.asarray(means, np.float64)
    B, L, C = x.shape
    al, c = _coeffs(sde, kw, t, B, var, G, L, C, np.float64)
    diff = x[:, None] - al[:, None] * mu[None]
    logit = np.asarray(log_w, np.float64)[None] - 0.5 * (diff * diff / c[:, None]).reshape(B, mu.shape[0], -1).sum(-1)
    m = logit.max(-1, keepdims=True)
    return (m[:, 0] + np.log(np.exp(logit - m).sum(-1))) - 0.5 * np.log(2.0 * math.pi * c).reshape(B, -1).sum(-1)


def variance(L, C, mode, seed=0):
    """``mode`` 0: None (v = 0, the empirical distribution); 1: about 0.04 U(0.5, 2) per coordinate."""
    if not mode:
        return None
    return (0.04 * np.random.default_rng(1000 + seed).uniform(0.5, 2.0, (L, C))).astype(np.float32)


def make_case(shape, sde, t, v_mode, fourier=True, seed=0):
    """A case of the grid: fp32 arrays x, means, log_w, var (or None), G.  Half the means (the odd ones) sit about two
    noise standard deviations -- of the marginal at this t -- from their even neighbour: the NEAR-TIE construction, which
    keeps two softmax weights of comparable size at every t.  Rows of x are draws of the marginal around a random mean."""
    B, L, C, K = shape
    kw = sde_kwargs(sde)
    rng = np.random.default_rng(seed + 7919 * (L * C + K))
    G = fourier_G(L, fourier)
    var = variance(L, C, v_mode, seed)
    al, s2 = alpha_sigma2(sde, kw, t)
    v = np.zeros((L, C)) if var is None else var.astype(np.float64)
    c = al * al * v + s2 * (G.astype(np.float64) ** 2)[:, None]
    means = rng.standard_normal((K, L, C))
    for i in range(1, K, 2):
        u = rng.standard_normal((L, C))
        u /= np.sqrt((u * u).sum())
        means[i] = means[i - 1] + 2.0 * u * np.sqrt(c) / al  # |alpha (mu_i - mu_{i-1})| / sqrt(c) = 2
    log_w = np.log(rng.dirichlet(np.full(K, 2.0)))
    pick = rng.integers(0, K, B)
    x = al * means[pick] + np.sqrt(c)[None] * rng.standard_normal((B, L, C))
    f = np.float32
    return x.astype(f), means.astype(f), log_w.astype(f), var, G


def displacement_error(d, d64, x, means, alpha):
    """max |d - d64| over max(|x|, alpha |mu|): the form the bars are stated in."""
    scale = max(float(np.abs(np.asarray(x, np.float64)).max()), float(np.max(alpha)) * float(np.abs(means).max()))
    return float(np.abs(np.asarray(d, np.float64) - d64).max()) / scale


def em_step(sde, kw, x, s, G, t, dt, z):
    """One reverse Euler-Maruyama step (sde.py:129-165, 215-246) in float64."""
    t = float(np.float32(t))
    g = np.asarray(G, np.float64)[None, :, None]
    if sde == "vp":
        beta = kw["beta_min"] + t * (kw["beta_max"] - kw["beta_min"])
        drift = -0.5 * beta * x - beta * g * g * s
        diff = math.sqrt(beta) * g
    else:
        r = kw["sigma_max"] / kw["sigma_min"]
        cs = kw["sigma_min"] * math.sqrt(2.0 * math.log(r)) * r ** t
        drift = -(cs * g) ** 2 * s
        diff = cs * g
    return x - drift * dt + diff * math.sqrt(dt) * z


# ---- mode weights end to end: three well-separated components, weights 0.2 / 0.3 / 0.5 ----
MODE_W = np.array([0.2, 0.3, 0.5])
MODE_N, MODE_STEPS, MODE_SEED = 2048, 200, 3


def mode_mixture(L=8):
    """(means (3, L, 1), log-weights, variance): the means are 6 sqrt(L) and 6 sqrt(L / 2) apart, 30 and more bandwidths."""
    mu = np.zeros((3, L, 1), np.float32)
    mu[0, :, 0], mu[1, :, 0], mu[2, :, 0] = 3.0, -3.0, 3.0 * np.where(np.arange(L) % 2 == 0, 1.0, -1.0)
    return mu, np.log(MODE_W).astype(np.float32), np.full((L, 1), 0.04, np.float32)


def mode_sigmas(x, mu):
    """|nearest-component frequency - weight| in binomial standard deviations, per component."""
    x = np.asarray(x, np.float64)
    near = ((x[:, None] - mu[None]) ** 2).reshape(x.shape[0], 3, -1).sum(-1).argmin(-1)
    freq = np.bincount(near, minlength=3) / x.shape[0]
    return np.abs(freq - MODE_W) / np.sqrt(MODE_W * (1 - MODE_W) / x.shape[0])


def mode_run(sde, seed=MODE_SEED, n=MODE_N, steps=MODE_STEPS):
    """The float64 Euler-Maruyama run of the mode-weight case on numpy draws."""
    kw = sde_kwargs(sde)
    mu, lw, var = mode_mixture()
    G = fourier_G(mu.shape[1])
    ts = np.linspace(1.0, 1e-5, steps).astype(np.float32)
    h = float(ts[0] - ts[1])
    rng = np.random.default_rng(seed)
    x = G[None, :, None] * rng.standard_normal((n,) + mu.shape[1:]) * (kw["sigma_max"] if sde == "ve" else 1.0)
    for t in ts:
        x = em_step(sde, kw, x, score(sde, kw, x, t, mu, lw, var, G), G, t, h, rng.standard_normal(x.shape))
    return x, mu


def last_step_gain(sde, kw, var, G, t, dt):
    """dt g(t)^2 G_l^2 / c_lc at time t: how far one Euler-Maruyama step moves a sample along its displacement (1 lands
    on the posterior mean; far above 1 overshoots it).  Returns the largest over the coordinates."""
    al, s2 = alpha_sigma2(sde, kw, t)
    g2 = np.asarray(G, np.float64) ** 2
    v = 0.0 if var is None else np.asarray(var, np.float64)
    c = al * al * v + (s2 * g2)[:, None]
    tt = float(np.float32(t))
    if sde == "vp":
        gg = kw["beta_min"] + tt * (kw["beta_max"] - kw["beta_min"])
    else:
        r = kw["sigma_max"] / kw["sigma_min"]
        gg = (kw["sigma_min"] * math.sqrt(2.0 * math.log(r)) * r ** tt) ** 2
    return float((dt * gg * g2[:, None] / c).max())
