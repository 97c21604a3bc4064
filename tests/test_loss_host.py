"""CPU-side tests of the score-matching validation loss (no GPU): argument checks of the context-free entry points, the
Python surface, and a float64 restatement of the loss formulas against the reference's recorded losses
(tests/golden/g16_losses.npz, written by tools/gen_loss_golden.py from the unmodified reference)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import cases, ffd_oracle as O

INVALID = -1
SDE_KW = {"vp": cases.VP, "ve": cases.VE}
VARIANTS = [(i, sde, lw, rm) for i in (1, 2, 3, 4) for sde in ("vp", "ve") for lw in (0, 1)
            for rm in ((1, 0) if i == 1 else (1,))]


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def loss_f64(score, z, sigma, G, lw, reduce_mean):
    """The arithmetic of losses.py:68-122 in float64: per-sample losses."""
    std = sigma.astype(np.float64)[:, None] * G.astype(np.float64)[None, :]
    r = score.astype(np.float64) + z.astype(np.float64) / std[:, :, None]
    if lw:
        terms = (std[:, :, None] * r) ** 2
    else:
        terms = (1.0 / np.sum(1.0 / std ** 2, axis=1))[:, None, None] * r ** 2
    terms = terms.reshape(len(r), -1)
    return terms.mean(axis=1) if reduce_mean else 0.5 * terms.sum(axis=1)


def perturb_f64(x0, z, mean_coeff, sigma, G):
    std = sigma.astype(np.float64)[:, None] * G.astype(np.float64)[None, :]
    return mean_coeff.astype(np.float64)[:, None, None] * x0 + std[:, :, None] * z


def case_weights(g, i):
    from fastfourierdiffusion_amd.utils import synthetic

    lstm, L, Cn, d, H, NL, B, wseed = (int(v) for v in g[f"c{i}_shape"])
    sd = synthetic.lstm_state_dict(Cn, L, d, NL, seed=wseed) if lstm else \
        synthetic.transformer_state_dict(Cn, L, d, NL, seed=wseed)
    return dict(lstm=bool(lstm), L=L, C=Cn, d=d, H=H, NL=NL, B=B), {k: torch.from_numpy(v) for k, v in sd.items()}


def test_entry_points_reject_bad_arguments_without_a_device(lib):
    p = 256  # a non-null address; every call below must return before it is used
    assert lib.ffd_sm_draw_times(None, 4, 1e-5, 1.0, 0, 0, None) == INVALID
    assert lib.ffd_sm_draw_times(p, 0, 1e-5, 1.0, 0, 0, None) == INVALID
    assert lib.ffd_sm_draw_times(p, 4, 1.0, 1.0, 0, 0, None) == INVALID   # eps >= T
    assert lib.ffd_sm_draw_times(p, 4, 2.0, 1.0, 0, 0, None) == INVALID
    good = [p, 2 * p, p, p, p, None, 0, 0, 2, 5, 3, None]
    for k in range(5):  # x0, x_noisy, mean_coeff, sigma, G
        a = list(good)
        a[k] = None
        assert lib.ffd_sm_perturb(*a) == INVALID, k
    for k in (8, 9, 10):  # B, L, C
        a = list(good)
        a[k] = 0
        assert lib.ffd_sm_perturb(*a) == INVALID, k
    a = list(good)
    a[1] = a[0]
    assert lib.ffd_sm_perturb(*a) == INVALID  # in place
    good = [p, p, p, None, 0, 0, 0, 1, p, 2, 5, 3, None]
    for k in (0, 1, 2, 8):  # score, sigma, G, per_sample_out
        a = list(good)
        a[k] = None
        assert lib.ffd_sm_loss(*a) == INVALID, k
    for k in (9, 10, 11):
        a = list(good)
        a[k] = 0
        assert lib.ffd_sm_loss(*a) == INVALID, k
    assert lib.ffd_sm_eval_batch(None, p, p, p, p, None, 0, 0, 0, 1, p, 2, None) == INVALID


def test_python_surface():
    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd._native import FFDError

    pkg.install_as_fdiff(force=True)
    from fdiff.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule
    from fdiff.schedulers.sde import VEScheduler, VPScheduler
    from fdiff.utils.dataclasses import DiffusableBatch
    from fdiff.utils.losses import evaluate_loss, get_sde_loss_fn

    sch = VPScheduler(fourier_noise_scaling=True)
    with pytest.raises(NotImplementedError, match="out of scope"):
        get_sde_loss_fn(sch, True)
    with pytest.raises(ValueError):
        get_sde_loss_fn(sch, False, rng="numpy")
    models = [ScoreModule(n_channels=3, max_len=20, noise_scheduler=sch, d_model=24, num_layers=2, n_head=4),
              LSTMScoreModule(n_channels=3, max_len=20, noise_scheduler=sch, d_model=8, num_layers=1),
              MLPScoreModule(n_channels=3, max_len=20, noise_scheduler=sch, d_model=8, d_mlp=16, num_layers=1)]
    batch = DiffusableBatch(X=torch.zeros(2, 20, 3), timesteps=torch.full((2,), 0.5))
    for m in models:
        train_fn, val_fn = m.set_loss_fn()
        assert train_fn is None and callable(val_fn) and callable(m.validation_loss_fn)
        with pytest.raises(FFDError):  # CPU tensors are refused like everywhere else
            m.validation_step(batch, 0)
    with pytest.raises(FFDError):
        evaluate_loss(models[0], torch.zeros(4, 20, 3), batch_size=2)
    # marginal_coeffs are marginal_prob's own per-sample factors
    t = torch.tensor([1e-5, 0.01, 0.3, 0.77, 1.0])
    x = torch.randn(5, 20, 3)
    for s in (sch, VEScheduler(sigma_min=0.01, sigma_max=2.0, fourier_noise_scaling=True)):
        s.set_noise_scaling(20)
        mean, std = s.marginal_prob(x, t)
        mc, sg = s.marginal_coeffs(t)
        assert mc.shape == sg.shape == t.shape
        assert torch.equal(mean, mc.view(-1, 1, 1) * x) and torch.equal(std, sg.view(-1, 1) * s.G)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "c{}_{}_lw{}_rm{}".format(*v))
def test_float64_restatement_reproduces_the_reference_loss(golden, variant):
    """The formulas the device tests use as their comparator, fed the golden inputs and the oracle's score, give the
    loss the unmodified reference returned (within 2e-6: the reference's own fp32 rounding)."""
    i, sde, lw, rm = variant
    g = golden["g16_losses"]
    c, sd = case_weights(g, i)
    x0, t, z = g[f"c{i}_x0"], g[f"c{i}_t"], g[f"c{i}_z"]
    mc, sigma = g[f"c{i}_{sde}_mean_coeff"], g[f"c{i}_{sde}_sigma"]
    G = O.noise_scaling(c["L"], True).numpy()
    xn = torch.from_numpy(perturb_f64(x0, z, mc, sigma, G).astype(np.float32))
    tt = torch.from_numpy(t)
    with torch.no_grad():
        score = O.lstm_score_forward(xn, tt, sd, c["NL"]) if c["lstm"] else O.score_forward(xn, tt, sd, c["NL"], c["H"])
    per = loss_f64(score.numpy(), z, sigma, G, lw, rm)
    key = f"c{i}_{sde}_lw{lw}_rm{rm}"
    ref = float(g[key + "_loss"])
    rel = abs(per.mean() - ref) / ref
    print(f"{key}: restatement {per.mean():.8e} reference {ref:.8e} rel {rel:.2e}")
    assert rel <= 2e-6
    np.testing.assert_allclose(per, g[key + "_per_sample"], rtol=2e-6)
    assert 0 < float(g[key + "_tol"]) <= 2e-4
