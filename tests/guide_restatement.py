"""Numpy / torch restatement of guided conditional sampling (support module of test_guide_host.py / test_guide_gpu.py;
include/ffd.h ffd_guide_seed, ffd_guide_combine, ffd_host_guide_coef, ffd_mixture_score_vjp, ffd_train_input_vjp,
ffd_sample_batch_guided).

At time t, with (alpha, sigma) of the forward marginal as in cond_restatement.coefficients and c_l = sigma^2 G_l^2:

    x0hat = (x + c s) / alpha                      s = score(x, t)          (Tweedie)
    r     = mask (x0hat - obs)                     time domain
    r     = mask idft((x0hat - obs) std)           frequency domain (packed ortho spectra; std optional)
    loss  = 1/2 sum r^2                            per sample
    u     = d loss / d x0hat = mask r              time domain
          = std W dft(mask r)                      frequency domain, W = 1 (DC, Nyquist of an even L) | 2 (every other row)
    g     = (u + J^T (c u)) / alpha                J = d s / d x
    s~    = s - lambda g                           lambda = scale / (obs_var + rho sigma^2 / (alpha^2 + sigma^2))

``dtype=np.float64`` evaluates this in double; ``dtype=np.float32`` follows libffd's operation order with the
coefficients rounded once (the transforms run in numpy's float64 and are rounded where the kernel holds fp32 values, as
in cond_restatement).  The VJPs: the mixture's closed form (``mixture_vjp``, any dtype) and float64 autograd through the
restated scores (``mixture_vjp_autograd``, ``network_vjp``)."""
import math

import numpy as np
import torch

import cond_restatement as CR
import mixture_restatement as M
import pc_restatement as P
from cond_restatement import dft, idft


def coefficients(sde, kw, t, scale=1.0, obs_var=1e-2, rho=1.0):
    """(alpha, sigma^2, lambda) in double."""
    t = float(t)
    if sde == "vp":
        a, b = kw["beta_min"], kw["beta_max"]
        lmc = -0.25 * t * t * (b - a) - 0.5 * t * a
        alpha, s2 = math.exp(lmc), -math.expm1(2.0 * lmc)
    else:
        sg = kw["sigma_min"] * (kw["sigma_max"] / kw["sigma_min"]) ** t
        alpha, s2 = 1.0, sg * sg
    return alpha, s2, scale / (obs_var + rho * s2 / (alpha * alpha + s2))


def adjoint_weights(L):
    """W of the packed layout: rows 0 .. L/2 hold Re X_k, the rest Im X_k, k = 1 .. ceil(L/2) - 1."""
    W = np.full(L, 2.0)
    W[0] = 1.0
    if L % 2 == 0:
        W[L // 2] = 1.0
    return W


def seed(sde, kw, t, x, score, obs, mask, G, std=None, domain="frequency", dtype=np.float64):
    """(u, v, loss (B,) float64, x0hat) of one seed; obs and mask may be (1, L, C)."""
    assert domain in CR.DOMAINS and not (domain == "time" and std is not None)
    dt = np.dtype(dtype).type
    alpha, s2, _ = coefficients(sde, kw, t)
    x, score, obs, mask = (np.asarray(a, dtype) for a in (x, score, obs, mask))
    g = np.asarray(G, dtype)[None, :, None]
    c = (dt(s2) * (g * g)).astype(dtype)
    x0hat = ((x + c * score) / dt(alpha)).astype(dtype)
    d = (x0hat - obs).astype(dtype)
    if domain == "time":
        r = (mask * d).astype(dtype)
        u = (mask * r).astype(dtype)
    else:
        if std is not None:
            d = (d * np.asarray(std, dtype)[None]).astype(dtype)
        r = (mask * idft(d, dtype)).astype(dtype)
        u = dft((mask * r).astype(dtype), dtype)
        u = (u * adjoint_weights(x.shape[1]).astype(dtype)[None, :, None]).astype(dtype)
        if std is not None:
            u = (u * np.asarray(std, dtype)[None]).astype(dtype)
    r = np.broadcast_to(r, x.shape)
    loss = 0.5 * (r.astype(np.float64) ** 2).reshape(x.shape[0], -1).sum(-1)
    return np.broadcast_to(u, x.shape).astype(dtype), (c * u).astype(dtype), loss, x0hat


def loss_torch(sde, kw, t, x0hat, obs, mask, std=None, domain="frequency"):
    """The per-sample loss as a float64 torch expression of x0hat (B, L, C): the judge of ``seed``'s u by autograd."""
    d = x0hat - torch.as_tensor(obs, dtype=torch.float64)
    m = torch.as_tensor(mask, dtype=torch.float64)
    if domain == "time":
        r = m * d
    else:
        if std is not None:
            d = d * torch.as_tensor(std, dtype=torch.float64)[None]
        L = d.shape[1]
        n_re = L // 2 + 1
        im = torch.zeros_like(d[:, :n_re])
        im = torch.cat([im[:, :1], d[:, n_re:], im[:, 1 + (L - n_re):]], dim=1)
        r = m * torch.fft.irfft(torch.complex(d[:, :n_re], im), n=L, dim=1, norm="ortho")
    return 0.5 * (r * r).flatten(1).sum(1)


def combine(score, u, jtv, alpha, coef, dtype=np.float64):
    dt = np.dtype(dtype).type
    score, u, jtv = (np.asarray(a, dtype) for a in (score, u, jtv))
    return (score - dt(coef) * ((u + jtv) / dt(alpha))).astype(dtype)


# ---------------------------------------------------------------- the mixture's VJP ----
def mixture_vjp(sde, kw, x, t, means, log_w, var, G, v, dtype=np.float64):
    """J^T v by the closed form: (alpha^2 / c) (sum r mu p - m sum r p) - q, p_i = -(x - alpha mu_i) . q / alpha, q = v / c."""
    x = np.asarray(x, dtype)
    mu = np.asarray(means, dtype)
    B, L, C = x.shape
    K = mu.shape[0]
    al, c = M._coeffs(sde, kw, t, B, var, G, L, C, dtype)
    ic = (dtype(1.0) / c).astype(dtype)
    q = (np.asarray(v, dtype) * ic).astype(dtype)
    diff = x[:, None] - al[:, None] * mu[None]                                   # (B, K, L, C)
    sq = (diff * (diff * ic[:, None])).reshape(B, K, -1).sum(-1, dtype=dtype)
    pp = (diff * q[:, None]).reshape(B, K, -1).sum(-1, dtype=dtype)              # p' = (x - alpha mu) . q
    with np.errstate(invalid="ignore"):
        logit = (np.asarray(log_w, dtype)[None] - dtype(0.5) * sq).astype(dtype)
    mx = logit.max(-1, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, dtype(0.0))
    e = np.exp(logit - mx).astype(dtype)
    r = (e / e.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    muf = mu.reshape(K, -1)
    mean = np.einsum("bk,kj->bj", r, muf).astype(dtype)
    pm = np.einsum("bk,kj->bj", (r * pp).astype(dtype), muf).astype(dtype)
    pbar = (r * pp).sum(-1, keepdims=True, dtype=dtype)
    cov = (pm - mean * pbar).astype(dtype).reshape(B, L, C)
    return (-(al * ic) * cov - q).astype(dtype)


def _fma(a, b, c):
    """fp32 fused multiply-add: one rounding (the double product of two floats is exact)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _sum16(v):
    """ffd_mixture.hip's group16_sum: rotations by 8, 4, 2, 1 over 16 lanes, every stage rounded."""
    v = np.asarray(v, np.float32)
    for h in (8, 4, 2, 1):
        v = (v[:h] + v[h:2 * h]).astype(np.float32)
    return np.float32(v[0])


def mixture_vjp_ordered(sde, kw, x, t, means, log_w, var, G, v, slice_=512, tile=16):
    """The closed form in fp32 IN THE KERNEL'S ORDER, for the bar of the device's error: per row the components in slices
    of 512 and tiles of 16, t = x - alpha mu as one FMA, the squares and p' = t . q as FMA chains over the coordinates, an
    online softmax per tile (the tile's sums by the 16-lane tree), the two weighted sums as FMA chains over the components
    (the matrix cores' accumulation), rescaled at every tile, and the merge of the slices in ascending order, all in fp32.
    Shared time only.  (``mixture_vjp(..., np.float32)`` evaluates the same formula with numpy's pairwise sums.)"""
    f = np.float32
    x = np.asarray(x, f)
    mu = np.asarray(means, f)
    lw = np.asarray(log_w, f)
    B, L, C = x.shape
    K, D = mu.shape[0], L * C
    al, c = M._coeffs(sde, kw, t, B, var, G, L, C, f)
    ic = (f(1.0) / c).astype(f).reshape(B, D)
    al = al.reshape(B)
    xs, vs, muf = x.reshape(B, D), np.asarray(v, f).reshape(B, D), mu.reshape(K, D)
    out = np.zeros((B, D), f)
    for b in range(B):
        q = (vs[b] * ic[b]).astype(f)
        parts = []
        for k0 in range(0, K, slice_):
            k1 = min(K, k0 + slice_)
            tv = _fma(-al[b], muf[k0:k1], xs[b][None])                 # (components of the slice, D)
            sq, pp = np.zeros(k1 - k0, f), np.zeros(k1 - k0, f)
            for j in range(D):                                         # the chains run over the coordinates
                sq = _fma(tv[:, j], (tv[:, j] * ic[b, j]).astype(f), sq)
                pp = _fma(tv[:, j], q[j], pp)
            logits = _fma(f(-0.5), sq, lw[k0:k1])
            m_run, l_run, sp_run = f(-np.inf), f(0.0), f(0.0)
            acc, accp = np.zeros(D, f), np.zeros(D, f)
            for t0 in range(k0, k1, tile):
                n = min(k1, t0 + tile) - t0
                logit, pv = np.full(tile, -np.inf, f), np.zeros(tile, f)
                logit[:n], pv[:n] = logits[t0 - k0:t0 - k0 + n], pp[t0 - k0:t0 - k0 + n]
                m_new = max(m_run, logit.max())
                e = np.zeros(tile, f) if m_new == -np.inf else np.exp((logit - m_new).astype(f)).astype(f)
                sc = f(1.0) if (m_new == -np.inf or m_run == -np.inf) else np.exp(f(m_run - m_new)).astype(f)
                ep = (e * pv).astype(f)
                l_run, sp_run, m_run = _fma(l_run, sc, _sum16(e)), _fma(sp_run, sc, _sum16(ep)), m_new
                acc, accp = (acc * sc).astype(f), (accp * sc).astype(f)
                for i in range(n):
                    acc, accp = _fma(e[i], muf[t0 + i], acc), _fma(ep[i], muf[t0 + i], accp)
            parts.append((m_run, l_run, sp_run, acc, accp))
        Mx = max(p_[0] for p_ in parts)
        lsum, psum, mean, pm = f(0.0), f(0.0), np.zeros(D, f), np.zeros(D, f)
        for m_s, l_s, sp_s, a_s, ap_s in parts:
            w = f(0.0) if m_s == -np.inf else np.exp(f(m_s - Mx)).astype(f)
            lsum, psum = _fma(l_s, w, lsum), _fma(sp_s, w, psum)
            mean, pm = _fma(a_s, w, mean), _fma(ap_s, w, pm)
        inv_l = f(1.0) / lsum if lsum > 0 else f(0.0)
        cov = ((pm * inv_l).astype(f) - ((mean * inv_l).astype(f) * f(psum * inv_l)).astype(f)).astype(f)
        out[b] = ((-(f(al[b]) * ic[b]).astype(f) * cov).astype(f) - (vs[b] * ic[b]).astype(f)).astype(f)
    return out.reshape(B, L, C)


def mixture_score_torch(sde, kw, x, t, means, log_w, var, G):
    """mixture_restatement.score as a float64 torch expression of x."""
    B, L, C = x.shape
    al, c = M._coeffs(sde, kw, t, B, var, G, L, C, np.float64)
    al, c = torch.from_numpy(np.ascontiguousarray(al)), torch.from_numpy(np.ascontiguousarray(c))
    mu = torch.as_tensor(np.asarray(means, np.float64))
    diff = x[:, None] - al[:, None] * mu[None]
    logit = torch.as_tensor(np.asarray(log_w, np.float64))[None] - 0.5 * (diff * diff / c[:, None]).flatten(2).sum(-1)
    r = torch.softmax(logit, dim=-1)
    mean = (r @ mu.flatten(1)).reshape(B, L, C)
    return (al * mean - x) / c


def mixture_vjp_autograd(sde, kw, x, t, means, log_w, var, G, v):
    xt = torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(True)
    s = mixture_score_torch(sde, kw, xt, t, means, log_w, var, G)
    return torch.autograd.grad(s, xt, torch.as_tensor(np.asarray(v, np.float64)))[0].numpy()


# ---------------------------------------------------------------- the networks' VJP ----
def network_vjp(forward, x, v, dtype=torch.float64):
    """(score, J^T v) by autograd through ``forward(x)`` (a torch function of the (B, L, C) input) in ``dtype``."""
    xt = torch.as_tensor(np.asarray(x)).to(dtype).clone().requires_grad_(True)
    s = forward(xt)
    g = torch.autograd.grad(s, xt, torch.as_tensor(np.asarray(v)).to(dtype))[0]
    return s.detach().numpy(), g.numpy()


# ---------------------------------------------------------------- the guided step and loop ----
def guided_score(sde, kw, t, x, obs, mask, G, score_vjp, guide, std=None, domain="frequency", dtype=np.float64):
    """(s~, loss): ``score_vjp(x, t, v)`` -> (s, J^T v) with v = None meaning "the score alone"; guide = dict(scale,
    obs_var, rho)."""
    alpha, _, lam = coefficients(sde, kw, t, guide["scale"], guide["obs_var"], guide["rho"])
    s = np.asarray(score_vjp(x, t, None)[0], dtype)
    u, v, loss, _ = seed(sde, kw, t, x, s, obs, mask, G, std, domain, dtype)
    jtv = np.asarray(score_vjp(x, t, v)[1], dtype)
    return combine(s, u, jtv, alpha, lam, dtype), loss


def guided_integrate(sde, kw, x, score_vjp, noise_fn, ts, step_size, G, obs, mask, guide, std=None, domain="frequency",
                     replace=False, final_replace=True, dtype=np.float64, first=0, n_run=None):
    """Reverse steps [first, first + n_run) of the grid: guided score -> Euler-Maruyama step -> (replace) projection.
    ``noise_fn(i, p)``: the predictor's draw of step i (p = 0) or its projection's (p = 1).  Returns (x, losses
    (n_run, B))."""
    n_run = len(ts) - first if n_run is None else n_run
    x = np.asarray(x, dtype)
    losses = []
    for i in range(first, first + n_run):
        t = float(ts[i])
        s, loss = guided_score(sde, kw, t, x, obs, mask, G, score_vjp, guide, std, domain, dtype)
        losses.append(loss)
        x = P.em_step(sde, kw, t, x, s, noise_fn(i, 0), G, step_size, dtype)
        if replace:
            x = CR.project(sde, kw, t, x, obs, mask, noise_fn(i, 1), G, std, domain, False, dtype)
    if final_replace and n_run > 0 and first + n_run == len(ts):
        x = CR.project(sde, kw, float(ts[-1]), x, obs, mask, None, G, std, domain, True, dtype)
    return x, np.array(losses)


def mixture_score_vjp_fn(sde, kw, means, log_w, var, G, dtype=np.float64):
    def fn(x, t, v):
        if v is None:
            return M.score(sde, kw, x, t, means, log_w, var, G, dtype), None
        return None, mixture_vjp(sde, kw, x, t, means, log_w, var, G, v, dtype)
    return fn


# ---------------------------------------------------------------- the two-mode forecast ----
# Two components in the time domain that share their first TWO_KNOWN points up to a small offset and part ways behind
# them; the observation is component 0's prefix + 0.05.  The exact posterior share of component 0 is closed form (0.966);
# replacement decides the mode while the noised observation says little and stays near the prior weights (0.51 .. 0.56 in
# float64 at 100 steps and 512 samples, VP and VE), guidance at scale 1, rho 1, obs_var = TWO_BW^2 reaches 0.66 .. 0.72.
TWO_L, TWO_KNOWN, TWO_BW = 8, 4, 0.5
TWO_W = np.array([0.5, 0.5])


def two_mode_mixture():
    mu = np.zeros((2, TWO_L, 1), np.float32)
    mu[0, :TWO_KNOWN, 0], mu[1, :TWO_KNOWN, 0] = 0.3, -0.3
    mu[0, TWO_KNOWN:, 0], mu[1, TWO_KNOWN:, 0] = 1.5, -1.5
    return mu, np.log(TWO_W).astype(np.float32), np.full((TWO_L, 1), TWO_BW ** 2, np.float32)


def two_mode_observation():
    mu, _, _ = two_mode_mixture()
    obs = np.zeros((1, TWO_L, 1), np.float32)
    obs[0, :TWO_KNOWN, 0] = mu[0, :TWO_KNOWN, 0] + np.float32(0.05)
    mask = np.zeros((1, TWO_L, 1), np.float32)
    mask[0, :TWO_KNOWN] = 1.0
    return obs, mask


def two_mode_exact_share():
    """P(component 0 | the observed prefix)."""
    mu, lw, var = two_mode_mixture()
    obs, mask = two_mode_observation()
    ll = np.log(TWO_W) - 0.5 * (mask[0] * (obs[0][None] - mu.astype(np.float64)) ** 2 / var[None]).reshape(2, -1).sum(-1)
    p = np.exp(ll - ll.max())
    return float(p[0] / p.sum())


def two_mode_share(x):
    """The share of samples whose free part sits nearer component 0's."""
    return float((np.asarray(x)[:, TWO_KNOWN:, 0].mean(-1) > 0).mean())


# ---------------------------------------------------------------- the networks of the input-VJP and loop tests ----
# TF_TOY; head_dim 8; B L = 85 rows (two 64-row dgrad tiles, the second ragged); L = 1; the MLP's TOY.  Every case runs on
# push_off_kink's weights at its own input, and its xseed is chosen on the CPU so that the no-kink assertion holds under
# VP and VE (tests/test_guide_host.py checks it).
VJP_CASES = (
    dict(name="tf_toy", kind="tf", L=12, C=2, d=24, H=4, F=64, NL=2, B=32, wseed=6, xseed=100),
    dict(name="tf_hd8", kind="tf", L=16, C=1, d=16, H=2, F=32, NL=1, B=2, wseed=21, xseed=100),
    dict(name="tf_85rows", kind="tf", L=17, C=3, d=60, H=12, F=128, NL=2, B=5, wseed=12, xseed=100),
    dict(name="tf_L1", kind="tf", L=1, C=1, d=8, H=2, F=64, NL=1, B=1, wseed=19, xseed=100),
    dict(name="mlp_toy", kind="mlp", L=12, C=2, d=24, F=64, NL=2, B=32, wseed=5, xseed=100),
)


def network_forward(c, sd, t, dtype=torch.float64):
    """``forward(x)`` of the case's network at the per-sample times ``t`` in ``dtype`` (the oracle's forward; the
    transformer's positional rows renormalised beforehand, as train_restatement does)."""
    import train_restatement as TR
    from oracle import ffd_oracle as O

    tt = torch.as_tensor(np.asarray(t)).to(dtype)
    if c["kind"] == "mlp":
        s = TR.cast(sd, dtype)
        return lambda x: O.mlp_score_forward(x, tt, s, c["NL"])
    s = TR.cast(TR.renormed(sd), dtype)

    def forward(x):
        with TR._Recorded():
            return O.score_forward(x, tt, s, c["NL"], c["H"])
    return forward


def vjp_case_setup(c, sde):
    """(model on the CPU with the pushed weights, its state dict, the input xn, the times t, the cotangent v), fp32."""
    import train_restatement as TR

    model = (TR.mlp_model if c["kind"] == "mlp" else TR.tf_model)(c, sde)
    sch = model.noise_scheduler
    x0, t, mc, sigma, z = TR.case_inputs(c, sch)
    G = sch.G.numpy()
    xn = (mc[:, None, None] * x0 + (sigma[:, None] * G[None, :])[:, :, None] * z).astype(np.float32)
    sd = vjp_push(c, dict(model.state_dict()), xn, t, G)
    model.load_state_dict(sd)
    v = np.random.default_rng(c["xseed"] + 1).standard_normal(xn.shape).astype(np.float32)
    return model, {k: v_.detach().clone() for k, v_ in model.state_dict().items()}, xn, t, v


def _as_input(xn):
    """train_restatement's (mc, sigma, z) under which its perturbation returns xn itself."""
    B = xn.shape[0]
    return np.ones(B, np.float32), np.zeros(B, np.float32), np.zeros_like(xn)


def vjp_push(c, sd, xn, t, G):
    import train_restatement as TR

    mc, sigma, z = _as_input(xn)
    if c["kind"] == "mlp":
        return TR.push_off_kink(sd, c["NL"], xn, t, mc, sigma, G, z)
    return TR.tf_push_off_kink(sd, c["NL"], c["H"], xn, t, mc, sigma, G, z)


def vjp_assert_no_kink(c, sd, xn, t, G, what=""):
    import train_restatement as TR

    mc, sigma, z = _as_input(xn)
    if c["kind"] == "mlp":
        return TR.assert_no_kink(sd, c["NL"], xn, t, mc, sigma, G, z, what)
    return TR.tf_assert_no_kink(sd, c["NL"], c["H"], xn, t, mc, sigma, G, z, what)
