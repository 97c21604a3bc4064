"""GPU tests of guided conditional sampling: the networks' input VJP ``ffd_train_input_vjp``, the mixture's
``ffd_mixture_score_vjp``, the guidance operators ``ffd_guide_seed`` / ``ffd_guide_combine`` and the loop
``ffd_sample_batch_guided`` / ``DiffusionSampler.sample_conditional(guidance=...)`` / ``impute(guidance=...)``.

The bar throughout is the project's: max(2e-6 x the quantity's max-norm, 3 x the error of the same arithmetic in fp32 on
the CPU against float64); trajectories: max(1e-5, 3 x the fp32 restatement's trajectory error) of the max-norm.  Every
test prints what it measured (DESIGN.md section 6 records the values).
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import cond_restatement as CR
import guide_restatement as GR
import mixture_restatement as M
import train_restatement as TR
from conftest import rel_err
from oracle import ffd_oracle as O
from test_cond_gpu import OP_SHAPES, _pack, _unpack, masks

pytestmark = pytest.mark.gpu

TOL_OP, TOL_TRAJ = 2e-6, 1e-5
SDES = {"vp": M.VP, "ve": M.VE}
ids = lambda s: "x".join(map(str, s))  # noqa: E731


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


def sde_desc(sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    a, b = (kw["beta_min"], kw["beta_max"]) if sde == "vp" else (kw["sigma_min"], kw["sigma_max"])
    return N.SdeDesc(N.FFD_SDE_VP if sde == "vp" else N.FFD_SDE_VE, 0, a, b)


def bar(own, floor=TOL_OP):
    return max(floor, 3.0 * own)


# ------------------------------------------------------------------ 1. the networks' input VJP ----
class Net:
    """A native training object on a module's parameters: ``full`` binds gradients and moments too (filled with a
    sentinel), otherwise the parameter-only binding."""

    def __init__(self, lib, model, full=False):
        self.lib, self.model, self.h = lib, model, C_.c_void_p()
        desc = model._desc()
        assert lib.ffd_train_create(C_.byref(self.h), C_.byref(desc), 0.0, torch.cuda.current_device()) == 0, self.error()
        self.extra = {}
        for name, p in model.named_parameters():
            if full:
                bufs = [torch.full_like(p, 3.25) for _ in range(3)] if p.requires_grad else [None] * 3
                self.extra[name] = bufs
                rc = lib.ffd_train_bind(self.h, name.encode(), p.data_ptr(), *(b.data_ptr() if b is not None else None for b in bufs),
                                        p.numel())
            else:
                rc = lib.ffd_train_bind_params(self.h, name.encode(), p.data_ptr(), p.numel())
            assert rc == 0, (name, self.error())

    def error(self):
        return self.lib.ffd_train_last_error(self.h).decode()

    def forward(self, x, t):
        out = torch.empty_like(x)
        rc = self.lib.ffd_train_forward(self.h, x.data_ptr(), t.data_ptr(), out.data_ptr(), x.shape[0], stream())
        assert rc == 0, self.error()
        return out

    def vjp(self, v, B=None):
        out = torch.empty_like(v)
        return self.lib.ffd_train_input_vjp(self.h, v.data_ptr(), out.data_ptr(), v.shape[0] if B is None else B, stream()), out

    def state(self):
        tensors = [p for _, p in self.model.named_parameters()] + [b for bufs in self.extra.values() for b in bufs if b is not None]
        return [t.detach().clone() for t in tensors], tensors

    def close(self):
        torch.cuda.synchronize()
        self.lib.ffd_train_destroy(self.h)


@pytest.mark.parametrize("case", GR.VJP_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_input_vjp_vs_float64_autograd(lib, sde, case):
    model, sd, xn, t, v = GR.vjp_case_setup(case, sde)
    G = model.noise_scheduler.G.numpy()
    GR.vjp_assert_no_kink(case, sd, xn, t, G, case["name"])  # for every case: none is skipped
    s64, g64 = GR.network_vjp(GR.network_forward(case, sd, t), xn, v)
    s32, g32 = GR.network_vjp(GR.network_forward(case, sd, t, torch.float32), xn, v, torch.float32)
    model = model.cuda()
    xd, td, vd = dev(xn), dev(t), dev(v)
    for full in (False, True):
        net = Net(lib, model, full)
        try:
            rc, _ = net.vjp(vd)
            assert rc == -3 and "no forward" in net.error()  # FFD_ERR_STATE without a forward
            score = net.forward(xd, td)
            before, tensors = net.state()  # (the forward has renormalised the positional rows in place, as torch's lookup does)
            rc, dx = net.vjp(vd)
            assert rc == 0, net.error()
            torch.cuda.synchronize()
            for was, now in zip(before, tensors):  # parameters, gradient buffers and moments: bit-unchanged
                assert torch.equal(was, now)
            assert torch.equal(vd.cpu(), torch.from_numpy(v))
            e_s, own_s = rel_err(score.cpu(), s64), rel_err(s32, s64)
            e_g, own_g = rel_err(dx.cpu(), g64), rel_err(g32, g64)
            print(f"input VJP {case['name']} {sde} full={full}: score {e_s:.2e} (CPU fp32 {own_s:.2e}), "
                  f"VJP {e_g:.2e} (CPU fp32 {own_g:.2e}, bar {bar(own_g):.2e})")
            assert e_s <= bar(own_s) and e_g <= bar(own_g)
            rc2, dx2 = net.vjp(vd)  # run to run
            assert rc2 == 0 and torch.equal(dx2, dx)
            assert net.vjp(vd, B=xn.shape[0] + 1)[0] == -3 and "another batch size" in net.error()  # FFD_ERR_STATE: B differs
            from fastfourierdiffusion_amd import _native as N

            cfg = N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1)
            B = xn.shape[0]
            per, one = torch.zeros(B, device="cuda", dtype=torch.float64), torch.ones(B, device="cuda")
            batch = (xd.data_ptr(), None, td.data_ptr(), one.data_ptr(), one.data_ptr(), None, 0, 0, 0, per.data_ptr(), B)
            if full:  # the activations of ffd_train_loss_grad serve too; an AdamW update ends their validity (last: it moves
                # the parameters)
                assert lib.ffd_train_loss_grad(net.h, *batch, stream()) == 0, net.error()
                rc, dx3 = net.vjp(vd)
                assert rc == 0 and torch.isfinite(dx3).all()
                assert lib.ffd_train_adamw(net.h, None, C_.byref(N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.0, 1)), stream()) == 0
                assert net.vjp(vd)[0] == -3 and "no forward" in net.error()
                net.forward(xd, td)
                assert net.vjp(vd)[0] == 0
            if not full:  # the training calls on a parameter-only binding: FFD_ERR_STATE before any device work
                assert lib.ffd_train_loss_grad(net.h, *batch, stream()) == -3
                assert lib.ffd_train_step(net.h, *batch, C_.byref(cfg), stream()) == -3
                assert lib.ffd_train_adamw(net.h, per.data_ptr(), C_.byref(cfg), stream()) == -3
                assert lib.ffd_train_grad_sqnorm(net.h, per.data_ptr(), stream()) == -3
                torch.cuda.synchronize()
                for was, now in zip(before, tensors):
                    assert torch.equal(was, now)
                assert not per.any()
        finally:
            net.close()


# ------------------------------------------------------------------ 2. the mixture's VJP ----
def run_vjp(lib, sde, x, t, means, lw, var, G, v, per_sample=False):
    B, L, Cn = x.shape
    K = means.shape[0]
    desc = sde_desc(sde)
    xd, md, ld, Gd, vd = dev(x), dev(means), dev(lw), dev(G), dev(v)
    vard = dev(var) if var is not None else None
    td = dev(np.asarray(t, np.float32).reshape(-1))
    n = lib.ffd_mixture_vjp_work_floats(B, K, L, Cn)
    assert n > 0
    work = torch.empty(n, device="cuda", dtype=torch.float32)
    out = torch.empty_like(xd)
    rc = lib.ffd_mixture_score_vjp(C_.byref(desc), xd.data_ptr(), td.data_ptr(), 1 if per_sample else 0, md.data_ptr(),
                                   ld.data_ptr(), vard.data_ptr() if vard is not None else None, Gd.data_ptr(), vd.data_ptr(),
                                   out.data_ptr(), B, K, L, Cn, work.data_ptr(), n, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(vd.cpu(), torch.from_numpy(np.asarray(v, np.float32)))
    return out.cpu().numpy()


def vjp_cotangent(x, seed):
    """A cotangent of the size guidance feeds: v = c u with u of order one, i.e. of the order of c; here c-free and of
    order one, which the linear map does not care about."""
    return np.random.default_rng(seed).standard_normal(x.shape).astype(np.float32)


MIX_K = (1, 15, 16, 17, 511, 512, 513)
MIX_LC = ((3, 1), (16, 4), (187, 1), (256, 4))  # L C = 3, 64, 187, 1024


@pytest.mark.parametrize("LC", MIX_LC, ids=ids)
@pytest.mark.parametrize("K", MIX_K)
def test_mixture_vjp_vs_float64(lib, K, LC):
    """Small t (a tight softmax) and large t, v = 0 and v > 0, VP and VE; one component with log w = -inf where K > 1.
    The CPU's fp32 error is that of the restatement IN THE KERNEL'S ORDER (GR.mixture_vjp_ordered: components in tiles of
    16 through an online softmax, FMA chains): at t = 1e-3 the covariance is a difference of two products that agree to
    sigma / alpha of their size, and what fp32 keeps of it depends on the order the weighted sums run in -- 2.2e-5 in this
    order against 5.4e-6 with numpy's pairwise sums at K = 15, L C = 3; and a chain over 513 components loses more than a
    pairwise sum at any t (3.9e-6 against 1.0e-6 at K = 513, L C = 3, t = 0.5).  tests/test_guide_host.py holds that
    restatement to float64 and to the exact one-component case."""
    L, Cn = LC
    B = 3
    worst = (0.0, 0.0)
    for sde, t, v_mode in (("vp", 0.5, 1), ("vp", 1e-3, 0), ("ve", 0.05, 1), ("ve", 1.0, 0)):
        kw = SDES[sde]
        x, mu, lw, var, G = M.make_case((B, L, Cn, K), sde, t, v_mode)
        if K > 1:
            lw = lw.copy()
            lw[K // 2] = -np.inf
        v = vjp_cotangent(x, K + L)
        ref = GR.mixture_vjp(sde, kw, x, t, mu, lw, var, G, v)
        own = rel_err(GR.mixture_vjp_ordered(sde, kw, x, t, mu, lw, var, G, v), ref)
        got = run_vjp(lib, sde, x, t, mu, lw, var, G, v)
        assert np.isfinite(got).all()
        err = rel_err(got, ref)
        worst = max(worst, (err, own))
        assert err <= bar(own), (sde, t, v_mode, err, own)
    print(f"mixture VJP K={K} L C={L * Cn}: device {worst[0]:.2e}, CPU fp32 {worst[1]:.2e}")


@pytest.mark.parametrize("shape", [(7, 20, 3, 17), (7, 187, 1, 70), (7, 8, 1, 515)], ids=ids)
def test_mixture_vjp_is_symmetric_repeats_and_rows_are_independent(lib, shape):
    sde, kw, t = "vp", M.VP, 0.05
    x, mu, lw, var, G = M.make_case(shape, sde, t, 1)
    v, w = vjp_cotangent(x, 1), vjp_cotangent(x, 2)
    jv = run_vjp(lib, sde, x, t, mu, lw, var, G, v)
    assert np.array_equal(run_vjp(lib, sde, x, t, mu, lw, var, G, v), jv)  # two runs
    split = np.concatenate([run_vjp(lib, sde, x[:3], t, mu, lw, var, G, v[:3]), run_vjp(lib, sde, x[3:], t, mu, lw, var, G, v[3:])])
    assert np.array_equal(split, jv)
    ones = np.concatenate([run_vjp(lib, sde, x[i:i + 1], t, mu, lw, var, G, v[i:i + 1]) for i in range(7)])
    assert np.array_equal(ones, jv)
    ts = np.float32([1.0, 0.5, 0.05, 1e-3, 1e-5, 0.5, 0.7])  # per-sample times: row by row the shared-time result
    per = run_vjp(lib, sde, x, ts, mu, lw, var, G, v, per_sample=True)
    for i in range(7):
        assert np.array_equal(per[i], run_vjp(lib, sde, x, float(ts[i]), mu, lw, var, G, v)[i]), i
    # <J v, w> = <v, J w> per row, within the bar of the two products
    jw = run_vjp(lib, sde, x, t, mu, lw, var, G, w)
    j64v, j64w = (GR.mixture_vjp(sde, kw, x, t, mu, lw, var, G, c) for c in (v, w))
    j32v, j32w = (GR.mixture_vjp_ordered(sde, kw, x, t, mu, lw, var, G, c) for c in (v, w))
    dot = lambda a, b: (np.asarray(a, np.float64) * b).reshape(7, -1).sum(-1)  # noqa: E731
    scale = (np.abs(j64v).reshape(7, -1).max(-1) * np.abs(w).reshape(7, -1).sum(-1))
    own = np.abs(dot(j32v, w) - dot(v, j32w)) / scale
    err = np.abs(dot(jv, w) - dot(v, jw)) / scale
    print(f"mixture VJP symmetry {shape}: device {err.max():.2e}, CPU fp32 {own.max():.2e}")
    assert err.max() <= bar(own.max())


# ------------------------------------------------------------------ 3. the seed and the combination ----
def run_seed(lib, sde, t, x, score, obs, mask, G, std, domain, want_loss=True, want_x0=True):
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn = x.shape
    desc = sde_desc(sde)
    xd, sd, od, md, Gd = dev(x), dev(score), dev(obs), dev(mask), dev(G)
    stdd = dev(std) if std is not None else None
    u, v, x0 = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    loss = torch.full((B,), 7.0, device="cuda", dtype=torch.float64)
    rc = lib.ffd_guide_seed(C_.byref(desc), xd.data_ptr(), sd.data_ptr(), od.data_ptr(), md.data_ptr(),
                            stdd.data_ptr() if stdd is not None else None, Gd.data_ptr(), float(t), obs.shape[0],
                            N.FFD_COND_FREQUENCY if domain == "frequency" else N.FFD_COND_TIME, B, L, Cn, u.data_ptr(),
                            v.data_ptr(), loss.data_ptr() if want_loss else None, x0.data_ptr() if want_x0 else None, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for a, b in ((xd, x), (sd, score), (od, obs), (md, mask)):  # inputs untouched
        assert torch.equal(a.cpu(), torch.from_numpy(np.asarray(b, np.float32)))
    return u.cpu().numpy(), v.cpu().numpy(), loss.cpu().numpy(), x0.cpu().numpy()


def cpu_fp32_seed(sde, t, x, score, obs, mask, G, std):
    """The frequency-domain seed in fp32 on the CPU (torch.fft): what fp32 arithmetic costs on these inputs."""
    alpha, s2, _ = GR.coefficients(sde, SDES[sde], t)
    x, score, obs, mask = (torch.from_numpy(np.asarray(a, np.float32)) for a in (x, score, obs, mask))
    L = x.shape[1]
    g = torch.from_numpy(G)[None, :, None]
    c = np.float32(s2) * (g * g)
    d = (x + c * score) / np.float32(alpha) - obs
    if std is not None:
        d = d * torch.from_numpy(std)[None]
    r = mask * torch.fft.irfft(_unpack(d), n=L, dim=1, norm="ortho")
    u = _pack(torch.fft.rfft(mask * r, dim=1, norm="ortho"), L) * torch.from_numpy(GR.adjoint_weights(L).astype(np.float32))[None, :, None]
    if std is not None:
        u = u * torch.from_numpy(std)[None]
    r = r.expand(x.shape)
    return u.expand(x.shape).numpy(), (c * u).expand(x.shape).numpy(), 0.5 * (r.double() ** 2).flatten(1).sum(1).numpy()


@pytest.mark.parametrize("shape", OP_SHAPES, ids=ids)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_seed_vs_float64_restatement(lib, sde, shape):
    """The eleven shapes of the projection tests; std given / NULL x obs_batch 1 / B x t in {1, 0.5, 1e-5}, Fourier and unit
    G alternating, the three masks rotating.  u, v, the loss and x0hat against float64."""
    B, L, Cn = shape
    kw = SDES[sde]
    rng = np.random.default_rng(5000 + 7 * L + Cn)
    x, score, series = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    std = rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32)
    mk = masks(shape, rng)
    worst, n = [0.0] * 6, 0
    for sd in (std, None):
        for ob in (1, B):
            for t in (1.0, 0.5, 1e-5):
                G = M.fourier_G(L, fourier=n % 2 == 0)
                mask = mk[("random", "prefix", "fractional")[n % 3]][:ob]
                n += 1
                obs = CR.dft(series[:ob] * mask, np.float32) if sd is None else (CR.dft(series[:ob] * mask) / sd).astype(np.float32)
                u, v, loss, x0 = run_seed(lib, sde, t, x, score, obs, mask, G, sd, "frequency")
                ru, rv, rl, rx0 = GR.seed(sde, kw, t, x, score, obs, mask, G, sd, "frequency")
                cu, cv, cl = cpu_fp32_seed(sde, t, x, score, obs, mask, G, sd)
                errs = (rel_err(u, ru), rel_err(cu, ru), rel_err(v, rv), rel_err(cv, rv), float(np.abs(loss - rl).max() / rl.max()),
                        float(np.abs(cl - rl).max() / rl.max()))
                worst = [max(a, b) for a, b in zip(worst, errs)]
                assert errs[0] <= bar(errs[1]) and errs[2] <= bar(errs[3]) and errs[4] <= bar(errs[5]), (sd is not None, ob, t, errs)
                assert rel_err(x0, rx0) <= TOL_OP
    print(f"seed {sde} {shape}: u {worst[0]:.2e} (CPU fp32 {worst[1]:.2e}), v {worst[2]:.2e} ({worst[3]:.2e}), "
          f"loss {worst[4]:.2e} ({worst[5]:.2e})")


@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4), (1, 1, 1), (2, 187, 1)], ids=ids)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_seed_time_domain_is_the_fp32_restatement_bit_for_bit(lib, sde, shape):
    """Pointwise, every operation its own rounding: with a 0 / 1 mask (and with a fractional one) the device gives the bits
    of the fp32 restatement; the loss against float64."""
    B, L, Cn = shape
    kw = SDES[sde]
    rng = np.random.default_rng(6000 + L)
    x, score, obs = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    for name, mask in masks(shape, rng).items():
        for ob in (1, B):
            for t in (1.0, 0.5, 1e-5):
                G = M.fourier_G(L, fourier=ob == 1)
                u, v, loss, x0 = run_seed(lib, sde, t, x, score, obs[:ob], mask[:ob], G, None, "time")
                ru, rv, rl, rx0 = GR.seed(sde, kw, t, x, score, obs[:ob], mask[:ob], G, None, "time", np.float32)
                assert np.array_equal(u, ru) and np.array_equal(v, rv) and np.array_equal(x0, rx0), (name, ob, t)
                l64 = GR.seed(sde, kw, t, x, score, obs[:ob], mask[:ob], G, None, "time")[2]
                assert np.abs(loss - rl).max() <= 1e-12 * max(rl.max(), 1e-300)  # the fp64 sum of the same fp32 residuals
                assert np.abs(loss - l64).max() <= bar(float(np.abs(rl - l64).max() / l64.max())) * l64.max()


@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4), (2, 16, 4), (2, 64, 3)], ids=ids)
@pytest.mark.parametrize("domain", CR.DOMAINS)
def test_seed_zero_mask_gives_exact_zeros(lib, shape, domain):
    B, L, Cn = shape
    rng = np.random.default_rng(7000 + L)
    x, score, obs = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    u, v, loss, _ = run_seed(lib, "ve", 0.5, x, score, obs, np.zeros(shape, np.float32), M.fourier_G(L), None, domain)
    assert not u.any() and not v.any() and not loss.any()
    # the optional outputs may be left out
    u2, v2, loss2, x02 = run_seed(lib, "ve", 0.5, x, score, obs, np.ones(shape, np.float32), M.fourier_G(L), None, domain,
                                  want_loss=False, want_x0=False)
    assert u2.any() and (loss2 == 7.0).all() and (x02 == 7.0).all()


@pytest.mark.parametrize("shape", [(5, 21, 3), (5, 20, 4), (5, 187, 1), (5, 16, 4), (5, 64, 3)], ids=ids)
@pytest.mark.parametrize("domain", CR.DOMAINS)
def test_seed_repeats_and_a_sample_does_not_depend_on_its_batch(lib, shape, domain):
    B, L, Cn = shape
    rng = np.random.default_rng(8000 + L)
    x, score = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    obs1, mask1 = rng.standard_normal((1, L, Cn)).astype(np.float32), (rng.random((1, L, Cn)) < 0.5).astype(np.float32)
    std = rng.uniform(0.5, 2.0, (L, Cn)).astype(np.float32) if domain == "frequency" else None
    G = M.fourier_G(L)
    whole = run_seed(lib, "vp", 0.3, x, score, obs1, mask1, G, std, domain)
    again = run_seed(lib, "vp", 0.3, x, score, obs1, mask1, G, std, domain)
    tiled = run_seed(lib, "vp", 0.3, x, score, np.repeat(obs1, B, 0), np.repeat(mask1, B, 0), G, std, domain)  # obs_batch = B
    for a, b, c in zip(whole, again, tiled):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for i in (0, B - 1):
        one = run_seed(lib, "vp", 0.3, x[i:i + 1], score[i:i + 1], obs1, mask1, G, std, domain)
        for a, b in zip(whole, one):
            assert np.array_equal(a[i:i + 1], b)


@pytest.mark.parametrize("n", [1, 3, 4, 1021, 4096, 3 * 187 * 5])
def test_combine_vs_float64(lib, n):
    rng = np.random.default_rng(n)
    s, u, j = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    for alpha, coef in ((0.9, 2.5), (1.0, 0.0), (0.1, 100.0)):
        sd, ud, jd = dev(s), dev(u), dev(j)
        out = torch.empty_like(sd)
        assert lib.ffd_guide_combine(sd.data_ptr(), ud.data_ptr(), jd.data_ptr(), alpha, coef, out.data_ptr(), n, stream()) == 0
        want32 = GR.combine(s, u, j, np.float32(alpha), np.float32(coef), np.float32)
        assert np.array_equal(out.cpu().numpy(), want32)  # every operation its own rounding: the restatement's bits
        assert rel_err(out.cpu(), GR.combine(s, u, j, float(np.float32(alpha)), float(np.float32(coef)))) <= TOL_OP
        assert lib.ffd_guide_combine(sd.data_ptr(), ud.data_ptr(), jd.data_ptr(), alpha, coef, sd.data_ptr(), n, stream()) == 0
        assert torch.equal(sd, out)  # in place
        if coef == 0.0:
            assert np.array_equal(out.cpu().numpy(), s)


# ------------------------------------------------------------------ 4. the loop ----
def scheduler(sde, L, fourier=True):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=fourier, **SDES[sde])
    sch.set_noise_scaling(L)
    return sch


def mixture_module(sde, mu, lw, var, fourier=True):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    K, L, Cn = mu.shape
    sch = scheduler(sde, L, fourier)
    m = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=None if var is None else torch.from_numpy(var),
                           fourier_noise_scaling=fourier)
    return m.cuda().eval(), sch


def spread_mixture(L, Cn, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, L, Cn)).astype(np.float32), np.log(rng.dirichlet(np.full(K, 2.0))).astype(np.float32),
            M.variance(L, Cn, 1))


def observation(L, Cn, domain, seed, B=1):
    """(obs in the diffused domain, mask on the time axis): a prefix of a random series."""
    rng = np.random.default_rng(seed)
    series = rng.standard_normal((B, L, Cn)).astype(np.float32)
    mask = np.zeros((B, L, Cn), np.float32)
    mask[:, :max(1, L // 2)] = 1.0
    return (CR.dft(series * mask, np.float32) if domain == "frequency" else series * mask), mask


def guided_call(lib, ctx, net, x, ts, first, n_run, cond, guide, z=None, loss=None, seed=0, offset=0):
    from fastfourierdiffusion_amd import _native as N

    ts_c = (C_.c_float * len(ts))(*[float(v) for v in ts])
    h = float(np.float32(ts[0]) - np.float32(ts[1]))
    rc = lib.ffd_sample_batch_guided(ctx.handle, net, x.data_ptr(), x.shape[0], ts_c, len(ts), h, first, n_run, seed, offset,
                                     z.data_ptr() if z is not None else None, C_.byref(cond), C_.byref(guide),
                                     loss.data_ptr() if loss is not None else None, stream())
    if rc:
        raw = lib.ffd_last_error(ctx.handle)
        return rc, raw.decode() if raw else ""
    return 0, ""


def cond_cfg(obs, mask, domain, final=1, std=None):
    from fastfourierdiffusion_amd import _native as N

    return N.CondCfg(obs.data_ptr(), mask.data_ptr(), std.data_ptr() if std is not None else None, obs.shape[0],
                     N.FFD_COND_FREQUENCY if domain == "frequency" else N.FFD_COND_TIME, final, 0)


@pytest.mark.parametrize("domain", CR.DOMAINS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_scale_zero_with_replace_is_the_replacement_loop_bit_for_bit(lib, sde, domain):
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn, K, steps = 6, 20, 3, 17, 8
    mu, lw, var = spread_mixture(L, Cn, K, 41)
    m, sch = mixture_module(sde, mu, lw, var, fourier=domain == "frequency")
    ctx = m._ctx()
    obs, mask = observation(L, Cn, domain, 42)
    od, md = dev(obs), dev(mask)
    ts = np.linspace(1.0, 1e-5, steps).astype(np.float32)
    rng = np.random.default_rng(43)
    x0 = dev(rng.standard_normal((B, L, Cn)))
    z = dev(rng.standard_normal((steps, 1, 2, B, L, Cn)))
    cond = cond_cfg(od, md, domain)
    ts_c = (C_.c_float * steps)(*ts.tolist())
    h = float(ts[0] - ts[1])
    for zz in (z, None):  # injected and device draws
        want = x0.clone()
        assert lib.ffd_sample_batch_cond(ctx.handle, want.data_ptr(), B, ts_c, steps, h, 0, steps, 0, 0.16, 0, 9, 3,
                                         zz.data_ptr() if zz is not None else None, 0, 0, C_.byref(cond), stream()) == 0
        got = x0.clone()
        loss = torch.zeros(steps, B, device="cuda", dtype=torch.float64)
        rc, msg = guided_call(lib, ctx, None, got, ts, 0, steps, cond, N.GuideCfg(0.0, 0.04, 1.0, 1, 0), zz, loss, seed=9, offset=3)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert bool((loss > 0).all())  # the loss is reported whatever the scale
    # guidance on: not the replacement run
    got = x0.clone()
    assert guided_call(lib, ctx, None, got, ts, 0, steps, cond, N.GuideCfg(1.0, 0.04, 1.0, 1, 0), z)[0] == 0
    assert not torch.equal(got, want)


def test_loop_refusals_come_before_any_device_work(lib):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule

    B, L, Cn, K, steps = 4, 20, 3, 5, 6
    mu, lw, var = spread_mixture(L, Cn, K, 51)
    m, sch = mixture_module("vp", mu, lw, var)
    ctx = m._ctx()
    obs, mask = observation(L, Cn, "frequency", 52)
    od, md = dev(obs), dev(mask)
    ts = np.linspace(1.0, 1e-5, steps).astype(np.float32)
    x = dev(np.random.default_rng(53).standard_normal((B, L, Cn)))
    keep = x.clone()
    ok = N.GuideCfg(1.0, 0.04, 1.0, 0, 0)
    cond = cond_cfg(od, md, "frequency")

    def call(cond_=cond, guide=ok, first=0, n_run=steps, z=None):
        from fastfourierdiffusion_amd import _native as N

        ts_c = (C_.c_float * steps)(*ts.tolist())
        return lib.ffd_sample_batch_guided(ctx.handle, None, x.data_ptr(), B, ts_c, steps, float(ts[0] - ts[1]), first, n_run, 0,
                                           0, z, C_.byref(cond_) if cond_ is not None else None,
                                           C_.byref(guide) if guide is not None else None, None, stream())

    assert call(cond_=None) == -1 and call(guide=None) == -1
    for bad in (N.GuideCfg(-1.0, 0.04, 1.0, 0, 0), N.GuideCfg(float("nan"), 0.04, 1.0, 0, 0), N.GuideCfg(1.0, -0.04, 1.0, 0, 0),
                N.GuideCfg(1.0, 0.04, float("inf"), 0, 0), N.GuideCfg(1.0, 0.0, 0.0, 0, 0)):
        assert call(guide=bad) == -1
    assert call(first=3, n_run=4) == -1 and call(z=x.data_ptr()) == -1
    assert call(cond_=N.CondCfg(od.data_ptr(), md.data_ptr(), None, 3, 0, 1, 0)) == -1  # obs_batch
    assert call(cond_=N.CondCfg(od.data_ptr(), md.data_ptr(), od.data_ptr(), 1, N.FFD_COND_TIME, 1, 0)) == -1  # std in time
    cfg = N.FrescaCfg(0.9, 1.2, 0.4, 0, 0)  # FreSca on: FFD_ERR_STATE
    assert lib.ffd_fresca_enable(ctx.handle, C_.byref(cfg)) == 0
    assert call() == -3 and b"FreSca" in lib.ffd_last_error(ctx.handle)
    assert lib.ffd_fresca_disable(ctx.handle) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, keep)  # nothing ran
    assert call(n_run=0) == 0 and call() == 0
    # the LSTM has no backward: FFD_ERR_UNSUPPORTED; a network without its training object: FFD_ERR_STATE; with another
    # model's: FFD_ERR_INVALID
    torch.manual_seed(0)
    lstm = LSTMScoreModule(n_channels=Cn, max_len=L, noise_scheduler=scheduler("vp", L), d_model=16, num_layers=1).cuda().eval()
    lctx = lstm._ctx()
    ts_c = (C_.c_float * steps)(*ts.tolist())
    args = (x.data_ptr(), B, ts_c, steps, float(ts[0] - ts[1]), 0, steps, 0, 0, None, C_.byref(cond), C_.byref(ok), None, stream())
    assert lib.ffd_sample_batch_guided(lctx.handle, None, *args) == -2
    c = dict(GR.VJP_CASES[4], L=L, C=Cn)
    mlp = TR.mlp_model(c, "vp").cuda().eval()
    mctx = mlp._ctx()
    assert lib.ffd_sample_batch_guided(mctx.handle, None, *args) == -3
    other = Net(lib, TR.mlp_model(dict(c, d=32), "vp").cuda())
    try:
        assert lib.ffd_sample_batch_guided(mctx.handle, other.h, *args) == -1
        assert b"descriptor" in lib.ffd_last_error(mctx.handle)
    finally:
        other.close()


# The trajectory grid.  A guided step computes g = (u + J^T (c u)) / alpha, and for a score the two terms cancel to
# alpha^2 Cov / c of their size -- 5e-5 (VP) and 4e-4 (VE) at t = 1, where fp32 keeps three digits of g whatever the
# kernels do -- while for an UNTRAINED network nothing cancels and the step's gain h g(t)^2 lambda / alpha^2 is 4e4 at
# t = 1 (VP, alpha^2 = 4.5e-5): the float64 restatement of these networks reaches 1e18 within five steps of the full grid
# and fp32 squares overflow.  So the trajectories run the LAST 12 steps of a 40-point grid (t = 0.31 ... 1e-5, alpha^2 >=
# 0.38, sigma_VE <= 0.14) at scale 0.5, where the gain stays below 1 for any Jacobian of order one and fp32 arithmetic is
# meaningful; t = 1 is covered by the operator tests above, the full grid by the bit-identity and two-mode tests below.
TRAJ_GRID, TRAJ_FIRST, TRAJ_RUN = 40, 28, 12


def _trajectory(lib, sde, domain, replace, model, net, score_vjp64, score_vjp32, B, L, Cn, what,
                grid=(TRAJ_GRID, TRAJ_FIRST, TRAJ_RUN), scale=0.5):
    """Steps [first, first + run) of the ``grid``-point grid (default: the last 12 of 40) on injected draws against the
    float64 restatement: the state and the losses; the bar from the fp32 restatement's own trajectory error."""
    TRAJ_GRID, TRAJ_FIRST, TRAJ_RUN = grid
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    G = model.noise_scheduler.G.numpy()
    obs, mask = observation(L, Cn, domain, 77)
    rng = np.random.default_rng(78)
    prior = SDES[sde]["sigma_max"] if sde == "ve" and TRAJ_FIRST == 0 else 1.0  # a run from t = 1 starts at the prior
    x0 = (prior * G[None, :, None] * rng.standard_normal((B, L, Cn))).astype(np.float32)
    z = rng.standard_normal((TRAJ_RUN, 1, 2, B, L, Cn)).astype(np.float32)
    ts, h = O.timesteps(TRAJ_GRID)
    ts = ts.numpy()
    od, md, x, zd = dev(obs), dev(mask), dev(x0), dev(z)
    loss = torch.zeros(TRAJ_RUN, B, device="cuda", dtype=torch.float64)
    rc, msg = guided_call(lib, model._ctx(), net, x, ts, TRAJ_FIRST, TRAJ_RUN, cond_cfg(od, md, domain, int(replace)),
                          N.GuideCfg(scale, 0.04, 1.0, int(replace), 0), zd, loss)
    assert rc == 0, msg
    torch.cuda.synchronize()
    g = dict(scale=scale, obs_var=0.04, rho=1.0)
    args = (ts, float(h), G, obs, mask, g, None, domain, replace, replace)
    draws = lambda i, p: z[i - TRAJ_FIRST, 0, p]  # noqa: E731
    ref, rl = GR.guided_integrate(sde, kw, x0, score_vjp64, draws, *args, first=TRAJ_FIRST, n_run=TRAJ_RUN)
    own, ol = GR.guided_integrate(sde, kw, x0, score_vjp32, draws, *args, dtype=np.float32, first=TRAJ_FIRST, n_run=TRAJ_RUN)
    assert np.abs(ref).max() < 1e3  # no run-away
    err, e32 = rel_err(x.cpu(), ref), rel_err(own, ref)
    lerr, l32 = rel_err(loss.cpu(), rl), rel_err(ol, rl)
    print(f"guided trajectory {what} {sde} {domain} replace={replace}: device {err:.2e} (fp32 restatement {e32:.2e}, bar "
          f"{bar(e32, TOL_TRAJ):.2e}), losses {lerr:.2e} ({l32:.2e})")
    assert err <= bar(e32, TOL_TRAJ) and lerr <= bar(l32, TOL_TRAJ)


@pytest.mark.parametrize("replace", [False, True], ids=["guide", "guide+replace"])
@pytest.mark.parametrize("domain", CR.DOMAINS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_mixture_trajectory_vs_restatement(lib, sde, domain, replace):
    B, L, Cn, K = 5, 20, 3, 17
    mu, lw, var = spread_mixture(L, Cn, K, 61)
    m, sch = mixture_module(sde, mu, lw, var, fourier=domain == "frequency")
    G = sch.G.numpy()
    _trajectory(lib, sde, domain, replace, m, None, GR.mixture_score_vjp_fn(sde, SDES[sde], mu, lw, var, G),
                GR.mixture_score_vjp_fn(sde, SDES[sde], mu, lw, var, G, np.float32), B, L, Cn, "mixture")


def ordered_mixture_fn(sde, mu, lw, var, G):
    """The mixture's fp32 score and VJP for the fp32 restatement of a trajectory, the VJP in the kernel's order."""
    def fn(x, t, v):
        if v is None:
            return M.score(sde, SDES[sde], x, t, mu, lw, var, G, np.float32), None
        return None, GR.mixture_vjp_ordered(sde, SDES[sde], x, t, mu, lw, var, G, v)
    return fn


@pytest.mark.parametrize("replace", [False, True], ids=["guide", "guide+replace"])
@pytest.mark.parametrize("domain", CR.DOMAINS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_mixture_trajectory_on_the_full_grid_vs_restatement(lib, sde, domain, replace):
    """The real 12-step grid, t = 1 ... 1e-5, scale 1, from the prior: for a true score the run does not diverge.  At t = 1
    u + J^T (c u) keeps three to four digits in fp32 (the grid comment above), on the device and in the restatement alike,
    so the bar -- 3 x the fp32 restatement's own trajectory error, its VJP in the kernel's order -- is wide here."""
    B, L, Cn, K = 5, 20, 3, 17
    mu, lw, var = spread_mixture(L, Cn, K, 61)
    m, sch = mixture_module(sde, mu, lw, var, fourier=domain == "frequency")
    G = sch.G.numpy()
    _trajectory(lib, sde, domain, replace, m, None, GR.mixture_score_vjp_fn(sde, SDES[sde], mu, lw, var, G),
                ordered_mixture_fn(sde, mu, lw, var, G), B, L, Cn, "mixture, full grid", grid=(12, 0, 12), scale=1.0)


def network_score_vjp_fn(case, sd, B, dtype):
    def fn(x, t, v):
        fwd = GR.network_forward(case, sd, np.full(B, t, np.float32), dtype)
        if v is None:
            with torch.no_grad():
                return fwd(torch.as_tensor(np.asarray(x)).to(dtype)).numpy(), None
        return GR.network_vjp(fwd, x, v, dtype)
    return fn


@pytest.mark.parametrize("replace", [False, True], ids=["guide", "guide+replace"])
@pytest.mark.parametrize("domain", CR.DOMAINS)
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("name", ["tf_toy", "mlp_toy"])
def test_network_trajectory_vs_restatement(lib, name, sde, domain, replace):
    """The transformer and the MLP at B = 4 on the weights of their VJP case; the time domain runs on the same network."""
    case = dict(next(c for c in GR.VJP_CASES if c["name"] == name), B=4)
    model, sd, _, _, _ = GR.vjp_case_setup(case, sde)
    model = model.cuda().eval()
    B, L, Cn = case["B"], case["L"], case["C"]
    net = Net(lib, model)
    try:
        _trajectory(lib, sde, domain, replace, model, net.h, network_score_vjp_fn(case, sd, B, torch.float64),
                    network_score_vjp_fn(case, sd, B, torch.float32), B, L, Cn, name)
    finally:
        net.close()


@pytest.mark.parametrize("kind", ["mixture", "tf_toy", "mlp_toy"])
def test_sampler_runs_the_native_loop_with_its_own_training_object(lib, kind):
    """``sample_conditional(guidance=...)`` on injected draws gives the bits of the native loop called directly on the same
    prior and draws: the sampler's plumbing, its parameter-only training object included.  The networks run at scale
    1e-6 (the full grid starts at t = 1: see the trajectory grid's comment), the mixture at scale 1."""
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    steps, sde, domain, B = 12, "vp", "frequency", 4
    if kind == "mixture":
        L, Cn = 20, 3
        mu, lw, var = spread_mixture(L, Cn, 17, 91)
        model, _ = mixture_module(sde, mu, lw, var)
        guide = Guidance(1.0, 0.04, 1.0, True)
    else:
        case = dict(next(c for c in GR.VJP_CASES if c["name"] == kind), B=B)
        model, _, _, _, _ = GR.vjp_case_setup(case, sde)
        model = model.cuda().eval()
        L, Cn = case["L"], case["C"]
        guide = Guidance(1e-6, 0.04, 1.0, True)
    obs, mask = observation(L, Cn, domain, 92)
    rng = np.random.default_rng(93)
    zs = [rng.standard_normal((B, L, Cn)).astype(np.float32) for _ in range(1 + 2 * steps)]
    s = DiffusionSampler(score_model=model, sample_batch_size=B, z_chunk_steps=10)
    s.inject_noise(zs)
    out = s.sample_conditional(torch.from_numpy(obs[0]), torch.from_numpy(mask[0]), B, steps, domain=domain, guidance=guide)
    assert torch.isfinite(out).all()
    if kind != "mixture":
        assert s._guide_net is not None and s._guide_net["handle"]
        again = DiffusionSampler(score_model=model, sample_batch_size=B)  # a second sampler owns a second object
        again.inject_noise(zs)
        assert torch.equal(again.sample_conditional(torch.from_numpy(obs[0]), torch.from_numpy(mask[0]), B, steps,
                                                    domain=domain, guidance=guide), out)
    s.inject_noise(zs[:1])
    x = s.sample_prior(B)
    net = Net(lib, model) if kind != "mixture" else None
    try:
        od, md = dev(obs), dev(mask)
        z = dev(np.stack(zs[1:]).reshape(steps, 1, 2, B, L, Cn))
        ts = model.noise_scheduler.timesteps.numpy()
        rc, msg = guided_call(lib, model._ctx(), net.h if net else None, x, ts, 0, steps, cond_cfg(od, md, domain),
                              N.GuideCfg(guide.scale, guide.obs_var, guide.rho, 1, 0), z)
        assert rc == 0, msg
        assert torch.equal(x.cpu(), out)
    finally:
        if net is not None:
            net.close()


@pytest.mark.parametrize("kind", ["mixture", "tf_toy"])
def test_every_split_point_and_a_philox_shard(lib, kind):
    from fastfourierdiffusion_amd import _native as N

    steps, sde, domain = 6, "vp", "frequency"
    if kind == "mixture":
        B, L, Cn = 6, 20, 3
        mu, lw, var = spread_mixture(L, Cn, 17, 71)
        model, sch = mixture_module(sde, mu, lw, var)
        net = None
    else:
        case = dict(next(c for c in GR.VJP_CASES if c["name"] == kind), B=6)
        model, _, _, _, _ = GR.vjp_case_setup(case, sde)
        model = model.cuda().eval()
        B, L, Cn = 6, case["L"], case["C"]
        net = Net(lib, model)
    try:
        ctx = model._ctx()
        h_net = net.h if net is not None else None
        obs, mask = observation(L, Cn, domain, 72)
        od, md = dev(obs), dev(mask)
        cond = cond_cfg(od, md, domain)
        guide = N.GuideCfg(1.0, 0.04, 1.0, 1, 0)
        ts = np.linspace(1.0, 1e-5, steps).astype(np.float32)
        rng = np.random.default_rng(73)
        x0 = dev(rng.standard_normal((B, L, Cn)))
        z = dev(rng.standard_normal((steps, 1, 2, B, L, Cn)))
        for zz in (z, None):
            whole, lw_ = x0.clone(), torch.zeros(steps, B, device="cuda", dtype=torch.float64)
            assert guided_call(lib, ctx, h_net, whole, ts, 0, steps, cond, guide, zz, lw_, seed=5)[0] == 0
            again = x0.clone()
            assert guided_call(lib, ctx, h_net, again, ts, 0, steps, cond, guide, zz, None, seed=5)[0] == 0
            assert torch.equal(again, whole)
            for cut in range(1, steps):  # every split point of the run
                x, ls = x0.clone(), torch.zeros(steps, B, device="cuda", dtype=torch.float64)
                assert guided_call(lib, ctx, h_net, x, ts, 0, cut, cond, guide, zz, ls, seed=5)[0] == 0
                assert guided_call(lib, ctx, h_net, x, ts, cut, steps - cut, cond, guide, zz[cut:] if zz is not None else None,
                                   ls[cut:], seed=5)[0] == 0
                assert torch.equal(x, whole) and torch.equal(ls, lw_), cut
        # a Philox shard: samples [3, 6) as a call of their own draw what the whole batch drew
        part = x0[3:].clone()
        assert guided_call(lib, ctx, h_net, part, ts, 0, steps, cond, guide, None, None, seed=5, offset=3)[0] == 0
        assert rel_err(part.cpu(), whole[3:].cpu()) <= TOL_TRAJ
        if kind == "mixture":  # a row of the mixture does not depend on its batch: the shard's bits
            assert torch.equal(part, whole[3:])
    finally:
        if net is not None:
            net.close()


def test_impute_with_guidance_end_to_end(lib):
    """A spectral mixture: the observed prefix of a series comes back (final_replace), and guided completions sit nearer
    the held-out part than the prior's spread."""
    from fastfourierdiffusion_amd.sampling import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    L, Cn, K, B = 20, 2, 9, 8
    rng = np.random.default_rng(81)
    series = rng.standard_normal((K, L, Cn)).astype(np.float32)
    mu = CR.dft(series, np.float32)
    lw = np.log(np.full(K, 1.0 / K)).astype(np.float32)
    var = np.full((L, Cn), 0.01, np.float32)
    m, sch = mixture_module("vp", mu, lw, var)
    mask = np.zeros((L, Cn), np.float32)
    mask[:L // 2] = 1.0
    s = DiffusionSampler(score_model=m, sample_batch_size=B, rng="philox", seed=3)
    out = s.impute(torch.from_numpy(series[4]), torch.from_numpy(mask), B, 60, guidance=Guidance(1.0, 0.01, 1.0)).numpy()
    assert out.shape == (B, L, Cn) and np.isfinite(out).all()
    assert np.abs(out[:, :L // 2] - series[4][None, :L // 2]).max() <= 1e-4  # the noiseless final replacement
    miss = np.abs(out[:, L // 2:] - series[4][None, L // 2:]).mean()
    print(f"impute with guidance: mean |completion - held-out part| {miss:.3f} (components are 1.1 apart on average)")
    assert miss < 0.5


def test_two_mode_forecast_on_the_device(lib):
    """GR's two-mode forecast with the device's own draws (512 Philox samples, 100 steps, batches of 32): guidance moves the
    share of component 0 towards the exact 0.966 where replacement stays near the prior's 0.5."""
    from fastfourierdiffusion_amd.sampling import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    mu, lw, var = GR.two_mode_mixture()
    obs, mask = GR.two_mode_observation()
    exact = GR.two_mode_exact_share()
    for sde in ("vp", "ve"):
        m, sch = mixture_module(sde, mu, lw, var, fourier=False)
        s = DiffusionSampler(score_model=m, sample_batch_size=32, rng="philox", seed=11)
        args = (torch.from_numpy(obs[0]), torch.from_numpy(mask[0]), 512, 100)
        replaced = GR.two_mode_share(s.sample_conditional(*args, domain="time").numpy())
        guided = GR.two_mode_share(s.sample_conditional(*args, domain="time",
                                                        guidance=Guidance(1.0, GR.TWO_BW ** 2, 1.0)).numpy())
        print(f"two-mode forecast on the device {sde}: exact {exact:.3f} replacement {replaced:.3f} guided {guided:.3f}")
        assert abs(guided - exact) < abs(replaced - exact) and guided - replaced > 3 * 0.022
