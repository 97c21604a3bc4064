"""GPU tests of the score-matching validation loss: the three context-free operators (ffd_sm_draw_times, ffd_sm_perturb,
ffd_sm_loss) against float64 numpy on identical inputs, then ffd_sm_eval_batch / get_sde_loss_fn / validation_step /
evaluate_loss against the reference's recorded losses (tests/golden/g16_losses.npz).

Bounds.  Perturbation: 5e-7 of the max-norm, the project's bar for the SDE step.  Loss kernel: TOL_OP = 2e-6 relative
per sample.  End to end: the `tol` stored with each golden case -- the first-order effect of the score path's own bar
(TOL_SCORE = 1e-5 of the score's max-norm) on the loss, 2 TOL_SCORE max|s| sum om |r| / sum om r^2, plus TOL_OP
(tools/gen_loss_golden.py computes it from the oracle in float64; the MLP test computes the same expression itself).
The comparator never calls the code under test."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import cases, ffd_oracle as O
from test_loss_host import SDE_KW, VARIANTS, loss_f64, perturb_f64

pytestmark = pytest.mark.gpu

TOL_OP, TOL_SCORE, TOL_STEP = 2e-6, 1e-5, 5e-7
SHAPES = [(3, 1, 1), (2, 5, 3), (5, 187, 1), (2, 64, 8), (3, 24, 40), (2, 365, 13)]
# (shape, floats the base pointers are shifted off 16-byte alignment)
PLACED = [(s, 0) for s in SHAPES] + [((2, 64, 8), 1), ((2, 64, 8), 3), ((3, 24, 40), 2)]
placed_id = lambda p: "B{}L{}C{}".format(*p[0]) + (f"+{p[1]}" if p[1] else "")  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def stream():
    from fastfourierdiffusion_amd import _native as N

    return N.current_stream_ptr(torch.device("cuda"))


def dev(a, off=0):
    """A device copy of `a` whose first element lies `off` floats past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, device="cuda", dtype=torch.from_numpy(a).dtype)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def table_G(lib, L):
    G = (C.c_float * L)()
    assert lib.ffd_host_noise_scaling(L, 1, G) == 0
    return np.array(G[:], dtype=np.float32)


def op_inputs(shape, seed=5):
    B, L, Cn = shape
    rng = np.random.default_rng(seed + 1000 * B + L)
    x0 = rng.standard_normal(shape).astype(np.float32)
    z = rng.standard_normal(shape).astype(np.float32)
    score = rng.standard_normal(shape).astype(np.float32)
    sigma = np.geomspace(1e-3, 50.0, B).astype(np.float32)  # the range VE (0.01 .. 50) and VP (<= 1) schedulers reach
    mc = rng.uniform(0.1, 1.0, B).astype(np.float32)
    return x0, z, score, mc, sigma


def run_perturb(lib, x0, mc, sigma, G, z, seed=0, offset=0, off=0):
    B, L, Cn = x0.shape
    # (every device copy stays referenced until the result is back: a freed block could be handed to the next copy)
    bufs = [dev(x0, off), dev(np.zeros_like(x0), off), dev(mc), dev(sigma), dev(G), dev(z, off) if z is not None else None]
    rc = lib.ffd_sm_perturb(*[b.data_ptr() if b is not None else None for b in bufs], seed, offset, B, L, Cn, stream())
    assert rc == 0
    return bufs[1].cpu().numpy()


def run_loss(lib, score, sigma, G, z, lw, rm, seed=0, offset=0, off=0):
    B, L, Cn = score.shape
    out = torch.empty(B, device="cuda", dtype=torch.float64)
    bufs = [dev(score, off), dev(sigma), dev(G), dev(z, off) if z is not None else None]
    rc = lib.ffd_sm_loss(*[b.data_ptr() if b is not None else None for b in bufs], seed, offset, lw, rm, out.data_ptr(),
                         B, L, Cn, stream())
    assert rc == 0
    return out.cpu().numpy()


# ---- operators --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", PLACED, ids=placed_id)
def test_perturb_injected_noise(lib, placed):
    shape, off = placed
    x0, z, _, mc, sigma = op_inputs(shape)
    G = table_G(lib, shape[1])
    got = run_perturb(lib, x0, mc, sigma, G, z, off=off)
    ref = perturb_f64(x0, z, mc, sigma, G)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"perturb {shape}+{off}: {err:.3e} of the max-norm")
    assert err <= TOL_STEP
    assert np.array_equal(got, run_perturb(lib, x0, mc, sigma, G, z, off=off))  # determinism


@pytest.mark.parametrize("placed", PLACED, ids=placed_id)
@pytest.mark.parametrize("lw", [0, 1])
@pytest.mark.parametrize("rm", [1, 0])
def test_loss_kernel(lib, placed, lw, rm):
    shape, off = placed
    _, z, score, _, sigma = op_inputs(shape)
    G = table_G(lib, shape[1])
    got = run_loss(lib, score, sigma, G, z, lw, rm, off=off)
    ref = loss_f64(score, z, sigma, G, lw, rm)
    err = np.abs(got / ref - 1.0).max()
    print(f"loss {shape}+{off} lw={lw} rm={rm}: per-sample relative error {err:.3e}")
    assert err <= TOL_OP
    assert np.array_equal(got, run_loss(lib, score, sigma, G, z, lw, rm, off=off))  # determinism: equal bits
    # the exact score of the perturbation kernel, -z / std, has zero loss
    std = sigma[:, None] * G[None, :]
    at_zero = run_loss(lib, np.zeros_like(score), sigma, G, z, lw, rm, off=off)
    exact = run_loss(lib, -(z / std[:, :, None]), sigma, G, z, lw, rm, off=off)
    print("  loss at score = -z/std over loss at score = 0:", (exact / at_zero).max())
    assert np.all(exact <= 1e-10 * at_zero)


def test_philox_draws_are_standard_normal(lib):
    shape = (8, 512, 256)  # 2^20 elements
    G = table_G(lib, shape[1])
    sigma = np.full(shape[0], 1.5, dtype=np.float32)
    xn = run_perturb(lib, np.zeros(shape, np.float32), np.ones(shape[0], np.float32), sigma, G, None, seed=1234)
    z = xn.astype(np.float64) / (sigma[:, None] * G[None, :]).astype(np.float64)[:, :, None]
    n = z.size
    assert n == 1 << 20
    print(f"philox: mean {z.mean():+.3e} (se {n ** -0.5:.1e}), var {z.var():.5f} (se {(2 / n) ** 0.5:.1e})")
    assert abs(z.mean()) <= 5 * n ** -0.5
    assert abs(z.var() - 1.0) <= 5 * (2.0 / n) ** 0.5


@pytest.mark.parametrize("shape", [(5, 187, 1), (6, 64, 8), (4, 5, 3), (5, 24, 40)], ids=lambda s: "B{}L{}C{}".format(*s))
@pytest.mark.parametrize("offset", [0, 7])
def test_philox_sharding_and_regeneration(lib, shape, offset):
    """A batch split in three with sample_offset draws what the whole batch draws, and ffd_sm_loss(z = NULL)
    regenerates the draws of ffd_sm_perturb: with x0 = 0 the exact score -x_noisy / std^2 has zero loss."""
    B, L, Cn = shape
    x0, _, _, mc, sigma = op_inputs(shape)
    sigma = np.clip(sigma, 1e-2, None)
    G = table_G(lib, L)
    seed = 99
    whole = run_perturb(lib, x0, mc, sigma, G, None, seed=seed, offset=offset)
    cuts = [0, 2, 3, B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = run_perturb(lib, x0[a:b], mc[a:b], sigma[a:b], G, None, seed=seed, offset=offset + a)
        assert np.array_equal(part, whole[a:b]), (a, b)
    assert not np.array_equal(whole, run_perturb(lib, x0, mc, sigma, G, None, seed=seed + 1, offset=offset))
    xn = run_perturb(lib, np.zeros_like(x0), mc, sigma, G, None, seed=seed, offset=offset)
    std = (sigma[:, None] * G[None, :]).astype(np.float64)[:, :, None]
    exact_score = (-(xn.astype(np.float64) / std ** 2)).astype(np.float32)
    for lw in (0, 1):
        at_zero = run_loss(lib, np.zeros_like(xn), sigma, G, None, lw, 1, seed=seed, offset=offset)
        exact = run_loss(lib, exact_score, sigma, G, None, lw, 1, seed=seed, offset=offset)
        print(f"  {shape} offset {offset} lw={lw}: regenerated-draw loss ratio {(exact / at_zero).max():.2e}")
        assert np.all(at_zero > 0) and np.all(exact <= 1e-10 * at_zero)
        # per-sample values depend on the global sample index only
        part = run_loss(lib, exact_score[2:3] * 0, sigma[2:3], G, None, lw, 1, seed=seed, offset=offset + 2)
        assert part[0] == at_zero[2]


def test_draw_times(lib):
    B, eps, T, seed = 65536, 1e-5, 1.0, 4242

    def draw(n, offset):
        t = torch.empty(n, device="cuda", dtype=torch.float32)
        assert lib.ffd_sm_draw_times(t.data_ptr(), n, eps, T, seed, offset, stream()) == 0
        return t.cpu().numpy()

    t = draw(B, 0)
    assert t.min() >= np.float32(eps) and t.max() <= np.float32(T)
    for a, b in [(0, 1000), (1000, 1003), (1003, B)]:
        assert np.array_equal(draw(b - a, a), t[a:b])
    assert np.array_equal(draw(B, 0), t)
    u = (t.astype(np.float64) - eps) / (T - eps)
    print(f"times: mean {u.mean():.5f} var {u.var():.5f}")
    assert abs(u.mean() - 0.5) <= 5 * (1 / 12 / B) ** 0.5
    assert abs(u.var() - 1 / 12) <= 5 * (1 / 180 / B) ** 0.5   # Var((u - 1/2)^2) = 1/80 - 1/144


# ---- end to end -------------------------------------------------------------------------------------------------
_MODELS = {}


def golden_model(g, i, sde):
    """The model of golden case i on the device (one per (case, sde), shared by the tests)."""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    from test_loss_host import case_weights

    if (i, sde) not in _MODELS:
        c, sd = case_weights(g, i)
        sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=True, **SDE_KW[sde])
        sch.set_noise_scaling(c["L"])
        if c["lstm"]:
            m = LSTMScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"])
        else:
            m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"],
                            n_head=c["H"])
        m.load_state_dict(sd, strict=True)
        _MODELS[(i, sde)] = m.cuda().eval()
    return _MODELS[(i, sde)]


@pytest.fixture(params=["default", "attn_small=0,small_path=0"])
def knobs(request, lib):
    if request.param != "default":
        assert lib.ffd_tune(b"attn_small", 0) == 0 and lib.ffd_tune(b"small_path", 0) == 0
    yield request.param
    assert lib.ffd_tune(b"reset", 0) == 0


def check_against_reference(what, got_mean, got_per, ref_loss, ref_per, tol):
    err = abs(got_mean - ref_loss) / ref_loss
    print(f"{what}: loss {got_mean:.8e} reference {ref_loss:.8e} rel {err:.2e} (tol {tol:.2e})")
    assert err <= tol
    if got_per is not None:
        err_p = np.abs(got_per / ref_per - 1.0).max()
        print(f"{what}: per-sample rel {err_p:.2e}")
        assert err_p <= tol


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "c{}_{}_lw{}_rm{}".format(*v))
def test_eval_batch_and_validation_step_match_the_reference(lib, golden, variant, knobs, monkeypatch):
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fastfourierdiffusion_amd.utils.losses import get_sde_loss_fn

    i, sde, lw, rm = variant
    g = golden["g16_losses"]
    key = f"c{i}_{sde}_lw{lw}_rm{rm}"
    ref_loss, ref_per, tol = float(g[key + "_loss"]), g[key + "_per_sample"], float(g[key + "_tol"])
    model = golden_model(g, i, sde)
    x0, t, z = dev(g[f"c{i}_x0"]), dev(g[f"c{i}_t"]), dev(g[f"c{i}_z"])
    B = x0.shape[0]
    # C level: the golden's own coefficient arrays
    ctx = model._ctx()
    mc, sigma = dev(g[f"c{i}_{sde}_mean_coeff"]), dev(g[f"c{i}_{sde}_sigma"])
    per = torch.empty(B, device="cuda", dtype=torch.float64)
    rc = lib.ffd_sm_eval_batch(ctx.handle, x0.data_ptr(), t.data_ptr(), mc.data_ptr(), sigma.data_ptr(), z.data_ptr(), 0,
                               0, lw, rm, per.data_ptr(), B, stream())
    assert rc == 0, lib.ffd_last_error(ctx.handle)
    mm = torch.empty(2, device="cuda", dtype=torch.float64)
    assert lib.ffd_w2_summary(per.data_ptr(), B, mm.data_ptr(), stream()) == 0
    check_against_reference(f"{key} [{knobs}] ffd_sm_eval_batch", float(mm[0]), per.cpu().numpy(), ref_loss, ref_per, tol)
    # Python level: the mirror computes the coefficients on the device; z arrives where the reference draws it
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: z)
    loss_fn = get_sde_loss_fn(model.noise_scheduler, False, reduce_mean=bool(rm), likelihood_weighting=bool(lw))
    batch = DiffusableBatch(X=x0, y=None, timesteps=t)
    loss = loss_fn(model, batch)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
    check_against_reference(f"{key} [{knobs}] loss_fn", float(loss), None, ref_loss, None, tol)
    if rm:
        model.likelihood_weighting = bool(lw)
        model.training_loss_fn, model.validation_loss_fn = model.set_loss_fn()
        assert torch.equal(model.validation_step(batch, 0), loss)


def test_mlp_against_the_float64_restatement(lib):
    """No reference golden exists for the MLP backbone (its block is torchvision.ops.MLP): the comparator is the float64
    restatement on the oracle's MLP forward, the bound the expression of the module docstring."""
    from fastfourierdiffusion_amd.models.score_models import MLPScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler
    from fastfourierdiffusion_amd.utils import synthetic
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fastfourierdiffusion_amd.utils.losses import get_sde_loss_fn

    c = cases.MLP_CASES[0]
    B, L, Cn = c["B"], c["L"], c["C"]
    sd = {k: torch.from_numpy(v) for k, v in
          synthetic.mlp_state_dict(Cn, L, c["d"], c["d_mlp"], c["NL"], seed=c["wseed"]).items()}
    sch = VPScheduler(fourier_noise_scaling=True, **cases.VP)
    sch.set_noise_scaling(L)
    model = MLPScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, d_model=c["d"], d_mlp=c["d_mlp"],
                           num_layers=c["NL"])
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    rng = np.random.default_rng(c["xseed"])
    x0 = rng.standard_normal((B, L, Cn)).astype(np.float32)
    z = rng.standard_normal((B, L, Cn)).astype(np.float32)
    t = torch.tensor([0.3, 0.5, 0.7, 0.9, 1.0])
    mc, sigma = (v.numpy() for v in sch.marginal_coeffs(t))
    G = sch.G.numpy()
    xn = torch.from_numpy(perturb_f64(x0, z, mc, sigma, G).astype(np.float32))
    with torch.no_grad():
        score = O.mlp_score_forward(xn, t, sd, c["NL"]).numpy()
    zd = dev(z)
    for lw in (0, 1):
        ref = loss_f64(score, z, sigma, G, lw, 1)
        std = (sigma[:, None] * G[None, :]).astype(np.float64)[:, :, None]
        r = score + z / std
        om = std ** 2 if lw else 1.0
        sens = (om * np.abs(r)).reshape(B, -1).sum(1) / (om * r * r).reshape(B, -1).sum(1)
        tol = float(np.max(2 * TOL_SCORE * np.abs(score).max() * sens)) + TOL_OP
        loss_fn = get_sde_loss_fn(sch, False, likelihood_weighting=bool(lw))
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch, "randn_like", lambda x, **kw: zd)
            loss = float(loss_fn(model, DiffusableBatch(X=dev(x0), timesteps=t.cuda())))
        err = abs(loss - ref.mean()) / ref.mean()
        print(f"mlp lw={lw}: loss {loss:.8e} restatement {ref.mean():.8e} rel {err:.2e} (tol {tol:.2e})")
        assert err <= tol


def test_evaluate_loss_does_not_depend_on_the_batching(lib, golden):
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    g = golden["g16_losses"]
    model = golden_model(g, 1, "vp")
    model.likelihood_weighting = False
    tol = float(g["c1_vp_lw0_rm1_tol"])
    n = 70
    X = dev(np.random.default_rng(7).standard_normal((n,) + g["c1_x0"].shape[1:]).astype(np.float32))
    whole = evaluate_loss(model, X, batch_size=n, seed=3, _return_noisy=True)
    small = evaluate_loss(model, X, batch_size=16, seed=3, _return_noisy=True)
    assert whole["per_sample"].shape == (1, n) and whole["per_sample"].dtype == torch.float64
    assert whole["timesteps"].shape == (1, n) and whole["loss"].shape == ()
    assert torch.equal(whole["timesteps"], small["timesteps"]) and torch.equal(whole["noisy"], small["noisy"])
    ts = whole["timesteps"].cpu().numpy()
    assert ts.min() >= np.float32(1e-5) and ts.max() <= 1.0 and len(np.unique(ts)) > n // 2
    err = float((small["per_sample"] / whole["per_sample"] - 1).abs().max())
    print(f"evaluate_loss: batch 16 vs 70 per-sample rel {err:.2e} (tol {tol:.2e})")
    assert err <= tol
    assert float(whole["loss"]) == pytest.approx(float(whole["per_sample"].mean()), rel=1e-12)
    halves = [evaluate_loss(model, X[:35], batch_size=35, seed=3, sample_offset=0, _return_noisy=True),
              evaluate_loss(model, X[35:], batch_size=35, seed=3, sample_offset=35, _return_noisy=True)]
    for k in ("timesteps", "noisy"):
        assert torch.equal(torch.cat([h[k] for h in halves], dim=1), whole[k]), k
    joined = torch.cat([h["per_sample"] for h in halves], dim=1)
    assert float((joined / whole["per_sample"] - 1).abs().max()) <= tol
    other = evaluate_loss(model, X, batch_size=n, seed=4, n_draws=2)
    assert other["per_sample"].shape == (2, n)
    assert not torch.equal(other["timesteps"][0], whole["timesteps"][0])
    assert not torch.equal(other["timesteps"][0], other["timesteps"][1])


def test_loss_fn_refuses_cpu_tensors(golden):
    from fastfourierdiffusion_amd._native import FFDError
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    g = golden["g16_losses"]
    model = golden_model(g, 1, "vp")
    with pytest.raises(FFDError):
        model.validation_step(DiffusableBatch(X=torch.from_numpy(g["c1_x0"]), timesteps=torch.from_numpy(g["c1_t"])), 0)
