"""Numpy restatement of the log-likelihood through the probability-flow ODE (support module of test_loglik_host.py /
test_loglik_gpu.py; include/ffd.h ffd_loglik_tail, ffd_loglik_batch, ffd_prior_logp).

Drift d(x, t) = a(t) x - (cs(t) G_l)^2 s(x, t) / 2 (ode_restatement.drift).  Along the ODE's solution from eps up to 1

    log p_eps(x(eps)) = log p_1(x(1)) + integral of v dt,    v = a(t) L C - cs(t)^2 tr(diag(G^2) ds/dx) / 2

with the trace estimated from probes eps_1 .. eps_k (k, B, L, C): w = G_l eps, h = fp32(fd_rel sigma(t)),

    tr = sum_m sum_lc w_m (s(x + h w_m) - s(x - h w_m)) / ((2 h) k).

The descending grid ``ts`` is walked from its last point to its first: interval j runs from ts[n-1-j] to ts[n-2-j], its
width the difference of the two fp32 values in double.  Euler: x += d dt, delta += dt v.  Heun: d1, v1 at (x, t);
xp = x + d1 dt; d2, v2 at (xp, t_next); x += (d1 + d2) / 2 dt, delta += dt / 2 (v1 + v2).

``dtype=np.float64`` evaluates everything in double (h stays the fp32 value: it is a parameter of the definition).
``dtype=np.float32`` follows libffd's operation order: one fp32 rounding per product / sum of w, hw, x+-, diff, term and of
the state update (the coefficients a, cs rounded from double, the width rounded to fp32 there); the terms are summed in
float64 and tr, v, delta are float64 in both modes.  x and scores are (B, L, C), G is (L,).
"""
import math

import numpy as np

import mixture_restatement as M
import ode_restatement as R
import philox_restatement as P

TAG_PROBE0 = 0xF0000000
LIMIT_LOGLIK = 0x0FFFFFF0  # ffd_loglik_batch: the largest e * n_probes + m of a run stays below it
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ------------------------------------------------------------------ coefficients ----
def sigma(sde, kw, t):
    """the marginal's standard deviation without G at time t, in double"""
    t = float(t)
    if sde == "vp":
        return math.sqrt(-math.expm1(2.0 * (-0.25 * t * t * (kw["beta_max"] - kw["beta_min"]) - 0.5 * t * kw["beta_min"])))
    return kw["sigma_min"] * (kw["sigma_max"] / kw["sigma_min"]) ** t


def fd_step(sde, kw, t, fd_rel):
    """h = fd_rel sigma(t), rounded once to fp32 (ffd_host_loglik_h)"""
    return np.float32(fd_rel * sigma(sde, kw, t))


# ------------------------------------------------------------------ probes ----
def tag_probe(e, n_probes, m):
    """probe m of divergence evaluation e (Euler: e = j; Heun: e = 2 j and 2 j + 1)"""
    return (TAG_PROBE0 + int(e) * int(n_probes) + int(m)) & 0xFFFFFFFF


def run_fits(solver, first, n_run, n_probes):
    """does a run of intervals [first, first + n_run) keep its tags inside the family?"""
    if n_run <= 0:
        return True
    e_max = 2 * (first + n_run - 1) + 1 if solver == "ode_heun" else first + n_run - 1
    return e_max * n_probes + (n_probes - 1) < LIMIT_LOGLIK


def rademacher(seed, tag, g0, n):
    """+1 / -1 of global elements g0 .. g0 + n - 1 under (seed, tag): bit 31 of slot g & 3 of Philox block g >> 2"""
    first, nb, skip = P._span(g0, n)
    words = np.stack(P._blocks(seed, tag, first, nb), axis=1).reshape(-1)[skip:skip + int(n)]
    return np.where((words >> np.uint64(31)) & np.uint64(1), -1.0, 1.0).astype(np.float32)


def philox_probes(seed, e, n_probes, sample_offset, shape):
    """the (n_probes, B, L, C) probes of divergence evaluation e of a call at ``sample_offset``"""
    B, L, Cn = shape
    return np.stack([rademacher(seed, tag_probe(e, n_probes, m), int(sample_offset) * L * Cn, B * L * Cn).reshape(shape)
                     for m in range(n_probes)])


def exact_probes(B, L, Cn):
    """eps_j = sqrt(D) e_j, j = 0 .. D - 1 (D = L C): Hutchinson's sum is then the exact trace.  (D, B, L, C) fp32."""
    D = L * Cn
    eye = (math.sqrt(D) * np.eye(D)).reshape(D, 1, L, Cn)
    return np.ascontiguousarray(np.broadcast_to(eye, (D, B, L, Cn))).astype(np.float32)


# ------------------------------------------------------------------ one divergence evaluation ----
def perturb(x, eps, G, h, dtype=np.float64):
    """the stacked batch (1 + 2 k, B, L, C): x, then x + h w_m, x - h w_m per probe"""
    x = np.asarray(x, dtype)
    w = np.asarray(G, dtype)[None, None, :, None] * np.asarray(eps, dtype)
    hw = dtype(h) * w
    out = np.empty((1 + 2 * eps.shape[0],) + x.shape, dtype)
    out[0], out[1::2], out[2::2] = x, x[None] + hw, x[None] - hw
    return out


def trace_terms(score_stack, eps, G, dtype=np.float64):
    """(k, B, L C) terms w (s+ - s-) in ``dtype``, widened to float64"""
    s = np.asarray(score_stack, dtype)
    w = np.asarray(G, dtype)[None, None, :, None] * np.asarray(eps, dtype)
    term = w * (s[1::2] - s[2::2])
    return term.astype(np.float64).reshape(term.shape[0], term.shape[1], -1)


def divergence_term(sde, kw, t, score_stack, eps, G, h, dtype=np.float64):
    """v (B,) float64 from the scores of the stacked batch"""
    terms = trace_terms(score_stack, eps, G, dtype)
    k, _, D = terms.shape
    tr = terms.sum(axis=(0, 2)) / ((2.0 * float(np.float32(h))) * k)
    a, cs = R.coefficients(sde, kw, t)
    return a * D + (-0.5 * (cs * cs)) * tr


def evaluate(sde, kw, x, t, score_fn, G, eps, h, dtype=np.float64, which=0):
    """(score at x (B, L, C), v (B,)): one score evaluation at the stacked batch"""
    stack = perturb(x, eps, G, h, dtype)
    s = np.asarray(score_fn(stack.reshape((-1,) + stack.shape[2:]), t, which), dtype).reshape(stack.shape)
    return s[0], divergence_term(sde, kw, t, s, eps, G, h, dtype)


def tail(stage, sde, kw, t, dt, x, xp, d1, score_stack, eps, G, h, delta, v1, dtype=np.float64):
    """One tail launch (ffd_loglik_tail) on copies: returns (x, xp, d1, delta, v1, v).  stage 0 Euler, 1 predict,
    2 correct (score_stack at xp and t = the interval's end)."""
    T = np.dtype(dtype).type
    s = np.asarray(score_stack, dtype)
    v = divergence_term(sde, kw, t, s, eps, G, h, dtype)
    fdt = T(np.float32(dt)) if dtype == np.float32 else T(dt)
    x = np.asarray(x, dtype)
    if stage == 2:
        d2 = R.drift(sde, kw, t, np.asarray(xp, dtype), s[0], G, dtype)
        return x + (T(0.5) * (np.asarray(d1, dtype) + d2)) * fdt, xp, d1, delta + (0.5 * dt) * (v1 + v), v1, v
    d = R.drift(sde, kw, t, x, s[0], G, dtype)
    if stage == 1:
        return x, x + d * fdt, d, delta, v, v
    return x + d * fdt, xp, d1, delta + dt * v, v1, v


# ------------------------------------------------------------------ the loop ----
def integrate(solver, sde, kw, x, score_fn, ts, G, n_probes=1, fd_rel=1e-2, probes=None, seed=0, sample_offset=0,
              dtype=np.float64, first=0, n_run=None, delta=None, stats=None):
    """Intervals [first, first + n_run) of the upward walk (default: all len(ts) - 1).  ``probes``: None (the Philox plan
    under ``seed`` / ``sample_offset``), a callable e -> (k, B, L, C) of the trajectory's evaluation ordinal, or an array
    (evaluations of this call, k, B, L, C) in consumption order.  Returns (x, delta (B,) float64).  ``stats`` (a dict):
    stats["abs"] receives, per sample, the sum of |dt v| (Heun: |dt v1 / 2| + |dt v2 / 2|) over the run -- the
    "sum of |terms|" the device tests' bars are stated in."""
    assert solver in ("ode_euler", "ode_heun")
    n = len(ts)
    n_run = n - 1 - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    B = x.shape[0]
    delta = np.zeros(B) if delta is None else np.asarray(delta, np.float64).copy()
    per = 2 if solver == "ode_heun" else 1
    zero = np.zeros(B)
    mass = np.zeros(B)

    def eps_of(ev):
        if probes is None:
            return philox_probes(seed, first * per + ev, n_probes, sample_offset, x.shape)
        return probes(first * per + ev) if callable(probes) else probes[ev]

    for j in range(n_run):
        lo = n - 1 - (first + j)
        t, tn = float(ts[lo]), float(ts[lo - 1])
        dt = tn - t
        if solver == "ode_euler":
            e0, h0 = eps_of(j), fd_step(sde, kw, t, fd_rel)
            stack = perturb(x, e0, G, h0, dtype)
            s = score_fn(stack.reshape((-1,) + x.shape[1:]), t, 0).reshape(stack.shape)
            x, _, _, delta, _, v = tail(0, sde, kw, t, dt, x, None, None, s, e0, G, h0, delta, zero, dtype)
            mass += np.abs(dt * v)
            continue
        e0, e1 = eps_of(2 * j), eps_of(2 * j + 1)
        h0, h1 = fd_step(sde, kw, t, fd_rel), fd_step(sde, kw, tn, fd_rel)
        stack = perturb(x, e0, G, h0, dtype)
        s = score_fn(stack.reshape((-1,) + x.shape[1:]), t, 0).reshape(stack.shape)
        _, xp, d1, _, v1, _ = tail(1, sde, kw, t, dt, x, None, None, s, e0, G, h0, delta, zero, dtype)
        stack = perturb(xp, e1, G, h1, dtype)
        s = score_fn(stack.reshape((-1,) + x.shape[1:]), tn, 1).reshape(stack.shape)
        x, _, _, delta, _, v2 = tail(2, sde, kw, tn, dt, x, xp, d1, s, e1, G, h1, delta, v1, dtype)
        mass += np.abs(0.5 * dt * v1) + np.abs(0.5 * dt * v2)
    if stats is not None:
        stats["abs"] = mass
    return x, delta


def integrate_exact(solver, sde, kw, x, score_fn, trace_fn, ts, G):
    """The same walk in float64 with the EXACT divergence: ``trace_fn(x, t)`` returns tr(diag(G^2) ds/dx) per row."""
    n = len(ts)
    x = np.asarray(x, np.float64)
    delta = np.zeros(x.shape[0])
    D = x.shape[1] * x.shape[2]

    def dv(xx, t):
        a, cs = R.coefficients(sde, kw, t)
        return R.drift(sde, kw, t, xx, score_fn(xx, t, 0), G), a * D - 0.5 * cs * cs * trace_fn(xx, t)

    for j in range(n - 1):
        t, tn = float(ts[n - 1 - j]), float(ts[n - 2 - j])
        dt = tn - t
        d1, v1 = dv(x, t)
        if solver == "ode_euler":
            x, delta = x + d1 * dt, delta + dt * v1
            continue
        d2, v2 = dv(x + d1 * dt, tn)
        x, delta = x + 0.5 * (d1 + d2) * dt, delta + 0.5 * dt * (v1 + v2)
    return x, delta


# ------------------------------------------------------------------ the prior ----
def prior_terms(sde, kw, x, G, dtype=np.float64):
    """log N(x; 0, (sigma_p G_l)^2) per element in ``dtype`` (the logarithm in double, rounded once)"""
    T = np.dtype(dtype).type
    sg = T(kw["sigma_max"] if sde == "ve" else 1.0) * np.asarray(G, dtype)[None, :, None]
    q = np.asarray(x, dtype) / sg
    c = (np.log(sg.astype(np.float64)) + HALF_LOG_2PI).astype(dtype)
    return T(-0.5) * (q * q) - c


def prior_logp(sde, kw, x, G, dtype=np.float64):
    t = prior_terms(sde, kw, x, G, dtype)
    return t.astype(np.float64).reshape(t.shape[0], -1).sum(-1)


# ------------------------------------------------------------------ the mixture's closed-form trace ----
def mixture_trace(sde, kw, x, t, means, log_w, var, G):
    """tr(diag(G^2) ds/dx) of the diffused mixture's score, float64, per row:
    sum_lc G_l^2 (-1 / c + alpha^2 Var_r(mu_lc) / c^2), r the posterior weights of the components.  Its only use is to
    judge the finite difference."""
    x = np.asarray(x, np.float64)
    mu = np.asarray(means, np.float64)
    B, L, Cn = x.shape
    al, c = M._coeffs(sde, kw, t, B, var, G, L, Cn, np.float64)
    diff = x[:, None] - al[:, None] * mu[None]
    logit = np.asarray(log_w, np.float64)[None] - 0.5 * (diff * diff / c[:, None]).reshape(B, mu.shape[0], -1).sum(-1)
    r = np.exp(logit - logit.max(-1, keepdims=True))
    r /= r.sum(-1, keepdims=True)
    mean = np.einsum("bk,klc->blc", r, mu)
    var_r = np.einsum("bk,bklc->blc", r, (mu[None] - mean[:, None]) ** 2)
    g2 = (np.asarray(G, np.float64) ** 2)[None, :, None]
    return (g2 * (-1.0 / c + (al * al) * var_r / (c * c))).reshape(B, -1).sum(-1)


def eps_marginal_points(sde, kw, means, log_w, var, G, eps, n, seed):
    """n draws of the mixture's marginal at time eps, float32 (B, L, C)"""
    rng = np.random.default_rng(seed)
    mu = np.asarray(means, np.float64)
    w = np.exp(np.asarray(log_w, np.float64))
    pick = rng.choice(mu.shape[0], n, p=w / w.sum())
    al, s2 = M.alpha_sigma2(sde, kw, eps)
    v = 0.0 if var is None else np.asarray(var, np.float64)
    c = al * al * v + s2 * (np.asarray(G, np.float64) ** 2)[:, None]
    return (al * mu[pick] + np.sqrt(c)[None] * rng.standard_normal((n,) + mu.shape[1:])).astype(np.float32)
