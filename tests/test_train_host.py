"""Host checks of the training feature: bindings against the header, argument errors that need no device, the schedule
helper, the Python refusals, and the judge itself (tests/train_restatement.py): its gradient against central finite
differences of its own float64 loss, its AdamW against torch.optim.AdamW, its kink report, and the fall of its own
validation loss on the toy set."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import train_restatement as TR
from conftest import ROOT, rel_err

TRAIN_SYMBOLS = ("ffd_dense_dgrad", "ffd_dense_wgrad", "ffd_dense_wgrad_chunks", "ffd_dense_wgrad_work_bytes",
                 "ffd_sm_loss_grad", "ffd_adamw", "ffd_host_lr_schedule", "ffd_train_create", "ffd_train_destroy",
                 "ffd_train_last_error", "ffd_train_work_bytes", "ffd_train_bind", "ffd_train_forward",
                 "ffd_train_loss_grad", "ffd_train_grad_sqnorm", "ffd_train_adamw", "ffd_train_step", "ffd_sm_draw_times_at",
                 "ffd_layernorm_stats_fwd", "ffd_layernorm_bwd", "ffd_attention_lse_fwd", "ffd_attention_bwd")


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def test_symbols_and_bindings(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    for name in TRAIN_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/ffd.h"
        n_args = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    assert C.sizeof(N.AdamWCfg) == 7 * 8
    srcs = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "Makefile")).read()
    assert "ffd_train.hip" in srcs


def test_argument_errors_need_no_device(lib):
    from fastfourierdiffusion_amd import _native as N

    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.ffd_dense_dgrad(None, p, None, None, p, 4, 4, 4, None) == -1
    assert lib.ffd_dense_dgrad(p, None, None, None, p, 4, 4, 4, None) == -1
    assert lib.ffd_dense_dgrad(p, p, None, None, None, 4, 4, 4, None) == -1
    assert lib.ffd_dense_dgrad(p, p, None, None, p, 4, 4, 4, None) == -1  # dX aliases dY
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.ffd_dense_wgrad(p, p, p, None, *shape, None, 0, None) == -1
        assert lib.ffd_dense_wgrad_work_bytes(*shape) == 0
    assert lib.ffd_dense_wgrad(p, p, p, None, 1 << 20, 1 << 12, 4, None, 0, None) == -2  # M N reaches 2^31
    assert lib.ffd_dense_wgrad(None, p, p, None, 4, 4, 4, None, 0, None) == -1
    assert lib.ffd_dense_wgrad(p, p, p, None, 2000, 4, 4, None, 0, None) == -1  # several chunks need a workspace
    # the chunk plan against its restatement: by rows where the output has tiles enough, finer where it has few
    wide = [lib.ffd_dense_wgrad_chunks(m, 1024, 1024) for m in (0, 1, 1024, 1025, 2560, 1 << 20)]
    assert wide == [0, 1, 1, 2, 3, 64]
    for shape in ((1, 1, 1), (64, 72, 187), (65, 72, 187), (512, 72, 187), (512, 512, 72), (2560, 64, 8), (95744, 2048, 60),
                  (95744, 60, 2048), (1 << 20, 8, 8)):
        assert lib.ffd_dense_wgrad_chunks(*shape) == TR.wgrad_chunks(*shape)[0], shape
    assert lib.ffd_dense_wgrad_chunks(512, 72, 187) == 8 and lib.ffd_dense_wgrad_chunks(95744, 2048, 60) == 64
    # a tile count beyond a grid axis is refused before any device work, not left to the launch
    assert lib.ffd_dense_dgrad(p, p, None, None, C.cast(buf, C.c_void_p).value + 4, 1, 1, 65535 * 64 + 1, None) == -2
    assert lib.ffd_dense_wgrad(p, p, p, None, 1, 65535 * 64 + 1, 1, None, 0, None) == -2
    assert lib.ffd_dense_wgrad_chunks(65536 * 64 + 1, 1, 2) == TR.wgrad_chunks(65536 * 64 + 1, 1, 2)[0] == 64
    # the LayerNorm and attention operators, the indexed time draw
    assert lib.ffd_sm_draw_times_at(p, None, 4, 1e-5, 1.0, 0, 0, None) == -1
    assert lib.ffd_sm_draw_times_at(p, p, 0, 1e-5, 1.0, 0, 0, None) == -1
    assert lib.ffd_sm_draw_times_at(p, p, 4, 1.0, 1.0, 0, 0, None) == -1
    assert lib.ffd_layernorm_stats_fwd(p, p, p, p, p, None, 4, 4, 1e-5, None) == -1
    assert lib.ffd_layernorm_stats_fwd(p, p, p, p, p, p, 0, 4, 1e-5, None) == -1
    assert lib.ffd_layernorm_bwd(p, p, p, p, p, p, None, 4, 4, None) == -1
    assert lib.ffd_layernorm_bwd(p, p, p, p, p, p, p, 4, 0, None) == -1
    assert lib.ffd_attention_lse_fwd(p, p, None, 1, 4, 1, 4, None) == -1
    assert lib.ffd_attention_lse_fwd(p, p, p, 1, 0, 1, 4, None) == -1
    assert lib.ffd_attention_lse_fwd(p, p, p, 1, 513, 1, 4, None) == -2 and lib.ffd_attention_lse_fwd(p, p, p, 1, 4, 1, 9, None) == -2
    assert lib.ffd_attention_bwd(p, p, p, p, None, 1, 4, 1, 4, None) == -1
    assert lib.ffd_attention_bwd(p, p, p, p, p, 1, 4, 1, 4, None) == -1  # dqkv aliases qkv
    pd = C.cast((C.c_double * 4)(), C.c_void_p)
    assert lib.ffd_sm_loss_grad(p, p, p, None, 0, 0, None, 0, pd, None, 2, 2, 2, None) == -1
    assert lib.ffd_sm_loss_grad(p, p, p, None, 0, 0, None, 0, pd, p, 0, 2, 2, None) == -1
    cfg = N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1)
    assert lib.ffd_adamw(p, p, p, None, 4, None, C.byref(cfg), None) == -1
    assert lib.ffd_adamw(p, p, p, p, 0, None, C.byref(cfg), None) == -1
    assert lib.ffd_adamw(p, p, p, p, 4, None, None, None) == -1
    for bad in (dict(step=0), dict(beta1=1.0), dict(lr=-1.0), dict(eps=-1.0), dict(lr=float("nan"))):
        kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_norm=1.0, step=1)
        kw.update(bad)
        assert lib.ffd_adamw(p, p, p, p, 4, None, C.byref(N.AdamWCfg(**kw)), None) == -1, bad


def _create(lib, desc, dropout=0.0):
    h = C.c_void_p()
    rc = lib.ffd_train_create(C.byref(h), C.byref(desc), dropout, 0)
    msg = lib.ffd_train_last_error(h).decode() if h else ""
    if h:
        lib.ffd_train_destroy(h)
    return rc, msg


def test_training_object_refusals(lib):
    from fastfourierdiffusion_amd import _native as N

    mlp = N.ModelDesc(N.FFD_MODEL_MLP, 1, 12, 24, 1, 2, 64, 0, 0.1, 20.0, 1, 1e-5)
    assert lib.ffd_train_create(None, C.byref(mlp), 0.0, 0) == -1
    rc, msg = _create(lib, mlp, dropout=0.1)
    assert rc == -2 and "dropout" in msg
    for kind, word in ((N.FFD_MODEL_LSTM, "kind"), (N.FFD_MODEL_MIXTURE, "kind")):
        rc, msg = _create(lib, N.ModelDesc(kind, 1, 12, 24, 4, 2, 64, 0, 0.1, 20.0, 1, 1e-5))
        assert rc == -2 and word in msg, (kind, msg)
    for bad in (dict(n_channels=0), dict(max_len=0), dict(num_layers=0), dict(d_model=0), dict(dim_feedforward=0)):
        d = N.ModelDesc(N.FFD_MODEL_MLP, 1, 12, 24, 1, 2, 64, 0, 0.1, 20.0, 1, 1e-5)
        for k, v in bad.items():
            setattr(d, k, v)
        assert _create(lib, d)[0] == -1, bad
        assert lib.ffd_train_work_bytes(C.byref(d), 8) == 0
    rc, msg = _create(lib, mlp)
    assert rc == (0 if torch.cuda.is_available() else -4), msg
    tf = lambda **kw: N.ModelDesc(**{**dict(kind=N.FFD_MODEL_TRANSFORMER, n_channels=1, max_len=12, d_model=24, n_head=4,  # noqa: E731
                                            num_layers=2, dim_feedforward=64, sde=0, sde_a=0.1, sde_b=20.0,
                                            fourier_noise_scaling=1, eps=1e-5), **kw})
    assert _create(lib, tf())[0] == (0 if torch.cuda.is_available() else -4)
    assert _create(lib, tf(n_head=5))[0] == -1 and _create(lib, tf(n_head=0))[0] == -1
    assert _create(lib, tf(n_head=2))[0] == -2 and _create(lib, tf(max_len=513))[0] == -2  # head_dim 12; L > 512
    assert _create(lib, tf(), dropout=0.1)[0] == -2
    assert lib.ffd_train_work_bytes(C.byref(tf()), 8) > lib.ffd_train_work_bytes(C.byref(tf(num_layers=1)), 8) > 0
    # the workspace is a function of (B, model): it grows with B and with the depth
    deep = N.ModelDesc(N.FFD_MODEL_MLP, 1, 12, 24, 1, 3, 64, 0, 0.1, 20.0, 1, 1e-5)
    w8, w64 = lib.ffd_train_work_bytes(C.byref(mlp), 8), lib.ffd_train_work_bytes(C.byref(mlp), 64)
    assert 0 < w8 < w64 < lib.ffd_train_work_bytes(C.byref(deep), 64)
    assert lib.ffd_train_work_bytes(C.byref(mlp), 0) == 0 and lib.ffd_train_work_bytes(None, 8) == 0
    for fn in (lib.ffd_train_loss_grad, ):
        assert fn(None, None, None, None, None, None, None, 0, 0, 0, None, 1, None) == -1
    assert lib.ffd_train_grad_sqnorm(None, None, None) == -1 and lib.ffd_train_bind(None, b"x", None, None, None, None, 1) == -1


@pytest.mark.parametrize("total", [1000, 200, 7, 1])
def test_schedule_against_lambdalr(lib, total):
    from fastfourierdiffusion_amd.training import lr_at

    warmup, lr_max = total // 10, 1e-3
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=lr_max)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: TR.lr_lambda(s, warmup, total))
    for step in range(total + 5):  # through the warm-up edge, the last step and beyond
        want = opt.param_groups[0]["lr"]
        got = lr_at(step, lr_max, warmup, total)
        assert abs(got - want) <= 1e-15 + 1e-12 * want, (step, got, want)
        opt.step(), sch.step()
    if warmup:
        assert lr_at(0, lr_max, warmup, total) == 0.0 and lr_at(warmup, lr_max, warmup, total) == lr_max
    assert lr_at(total, lr_max, warmup, total) <= 1e-19 and lr_at(total + 50, lr_max, warmup, total) >= 0.0


@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("lw", [False, True])
def test_judge_gradient_against_finite_differences(sde, lw):
    c = TR.MLP_CASES[0]
    model, sd, (x0, t, mc, sigma, z) = TR.case_setup(c, sde, lw)
    G = model.noise_scheduler.G.numpy()
    _, _, g = TR.mlp_gradients(sd, c["NL"], x0, t, mc, sigma, G, z, lw, torch.float64)
    rng = np.random.default_rng(0)
    s64 = TR.cast(sd, torch.float64)
    f = lambda: float(TR.mlp_loss(s64, c["NL"], x0, t, mc, sigma, G, z, lw, torch.float64)[0])  # noqa: E731
    with torch.no_grad():
        for k in g:
            flat = s64[k].view(-1)
            for i in rng.choice(flat.numel(), size=min(3, flat.numel()), replace=False):
                h = 1e-6 * max(1.0, abs(float(flat[i])))
                keep = float(flat[i])
                flat[i] = keep + h
                up = f()
                flat[i] = keep - h
                dn = f()
                flat[i] = keep
                fd = (up - dn) / (2 * h)
                assert abs(fd - g[k].reshape(-1)[i]) <= 1e-6 * np.abs(g[k]).max() + 1e-5 * abs(fd), (k, int(i))


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_transformer_judge_gradient_against_finite_differences(sde):
    c = TR.TF_CASES[0]
    model, sd, (x0, t, mc, sigma, z) = TR.tf_case_setup(c, sde)
    G = model.noise_scheduler.G.numpy()
    _, _, g = TR.tf_gradients(sd, c["NL"], c["H"], x0, t, mc, sigma, G, z, False, torch.float64)
    assert TR.POS in g and float(np.abs(g[TR.POS]).max()) > 0
    rng = np.random.default_rng(0)
    s64 = TR.cast(TR.renormed(sd), torch.float64)
    f = lambda: float(TR.tf_loss(s64, c["NL"], c["H"], x0, t, mc, sigma, G, z, False, torch.float64)[0])  # noqa: E731
    with torch.no_grad():
        for k in g:
            flat = s64[k].view(-1)
            for i in rng.choice(flat.numel(), size=min(2, flat.numel()), replace=False):
                h = 1e-6 * max(1.0, abs(float(flat[i])))
                keep = float(flat[i])
                flat[i] = keep + h
                up = f()
                flat[i] = keep - h
                dn = f()
                flat[i] = keep
                fd = (up - dn) / (2 * h)
                assert abs(fd - g[k].reshape(-1)[i]) <= 1e-6 * np.abs(g[k]).max() + 1e-5 * abs(fd), (k, int(i))


def test_transformer_cases_are_clear_of_the_kink():
    for i, c in enumerate(TR.TF_CASES):
        for sde in ("vp", "ve"):
            model, sd, _ = TR.tf_case_setup(c, sde)
            for step in range(3 if i < 2 else 1):
                x0, t, mc, sigma, z = TR.case_inputs(c, model.noise_scheduler, step)
                TR.tf_assert_no_kink(sd, c["NL"], c["H"], x0, t, mc, sigma, model.noise_scheduler.G.numpy(), z,
                                     f"{c['name']} {sde} step {step}")


@pytest.mark.parametrize("max_norm", [1.0, 1e9])
def test_judge_adamw_against_torch(max_norm):
    rng = np.random.default_rng(3)
    shapes = [(5, 3), (7,), (2, 2, 2)]
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    mine = [p.detach().clone() for p in ps]
    m, v = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]
    warmup, total, lr_max = 2, 20, 1e-2
    opt = torch.optim.AdamW(ps, lr=lr_max, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: TR.lr_lambda(s, warmup, total))
    clipped = []
    for step in range(6):
        gs = [torch.from_numpy(3.0 * rng.standard_normal(s)) for s in shapes]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step(), sch.step()
        _, coef = TR.clip_coef(gs, max_norm)
        clipped.append(coef < 1.0)
        for p, g, a, b in zip(mine, gs, m, v):
            TR.adamw_step(p, g * coef, a, b, step + 1, lr_max * TR.lr_lambda(step, warmup, total))
    assert all(clipped) == (max_norm == 1.0)
    for p, q in zip(ps, mine):
        assert rel_err(q.numpy(), p.detach().numpy()) < 1e-13
    for p, a, b in zip(ps, m, v):
        assert rel_err(a.numpy(), opt.state[p]["exp_avg"].numpy()) < 1e-13
        assert rel_err(b.numpy(), opt.state[p]["exp_avg_sq"].numpy()) < 1e-13


def test_kink_report_and_the_cases_seeds():
    """The report sees a unit placed on the kink, and every gradient case's inputs are clear of it (for case 0 at the
    three batches of the update test)."""
    for c in TR.MLP_CASES:
        for sde in ("vp", "ve"):
            model, sd, inp = TR.case_setup(c, sde)
            G = model.noise_scheduler.G.numpy()
            for step in range(3 if c is TR.MLP_CASES[0] else 1):
                x0, t, mc, sigma, z = TR.case_inputs(c, model.noise_scheduler, step)
                margin, e32 = TR.assert_no_kink(sd, c["NL"], x0, t, mc, sigma, G, z, f"{c['name']} {sde} step {step}")
                assert 0 < e32 < 1e-4 and margin < 1
    c = TR.MLP_CASES[0]
    model, sd, (x0, t, mc, sigma, z) = TR.case_setup(c, "vp")
    G = model.noise_scheduler.G.numpy()
    xn = TR.perturb(*[torch.from_numpy(a).double() for a in (x0, z, mc, sigma, G)])[0]
    with torch.no_grad():
        a = TR.mlp_forward_with_preacts(xn, torch.from_numpy(t).double(), TR.cast(sd, torch.float64), c["NL"])[1][0]
    bad = {k: v.clone() for k, v in sd.items()}
    bad["backbone.0.0.bias"][3] -= float(a[2, 3])  # unit 3 of block 0 now sits on the kink for row 2
    with pytest.raises(AssertionError, match="pre-activation"):
        TR.assert_no_kink(bad, c["NL"], x0, t, mc, sigma, G, z)
    # the forward with pre-activations is the oracle's forward
    with torch.no_grad():
        s64 = TR.cast(sd, torch.float64)
        from oracle import ffd_oracle as O
        assert torch.equal(TR.mlp_forward_with_preacts(xn, torch.from_numpy(t).double(), s64, c["NL"])[0],
                           O.mlp_score_forward(xn, torch.from_numpy(t).double(), s64, c["NL"]))


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_judge_training_lowers_the_validation_loss(sde):
    """The float64 restatement of the 200-step toy run: the fixed-draw validation loss falls (to 0.73 of its initial
    value under VP and to 0.075 under VE; printed)."""
    c = TR.TOY
    X, Xv = TR.toy_dataset(c["n"], c["L"], c["C"]), TR.toy_dataset(64, c["L"], c["C"], seed=12)
    model = TR.mlp_model(c, sde, total=c["total"], lr_max=c["lr_max"])
    sd, sch = dict(model.state_dict()), model.noise_scheduler
    run, losses, _ = TR.toy_run(sd, c["NL"], sch, False, X, 200, c["B"], c["seed"], c["lr_max"], c["total"] // 10, c["total"],
                                torch.float64)
    v0 = TR.validation_loss(sd, c["NL"], sch, False, Xv, c["seed"])
    v1 = TR.validation_loss(run.state(), c["NL"], sch, False, Xv, c["seed"])
    print(f"{sde}: validation loss {v0:.5f} -> {v1:.5f} ({v1 / v0:.3f}); clipped {sum(x < 1 for x in run.coefs)} of 200 steps")
    assert v1 < v0 and math.isfinite(v1)


def test_python_refusals():
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fastfourierdiffusion_amd.utils.losses import get_sde_loss_fn

    sch = TR.scheduler("vp", 12)
    X = torch.from_numpy(TR.toy_dataset(4, 12, 2))
    batch = DiffusableBatch(X=X, timesteps=torch.full((4,), 0.5))
    with pytest.raises(N.FFDError, match="cpu"):  # the transformer trains, but only on the device
        Trainer(ScoreModule(2, 12, sch, d_model=24, num_layers=1, n_head=4))
    for m in (LSTMScoreModule(2, 12, sch, d_model=8, num_layers=1), MixtureScoreModule(2, 12, sch, means=X)):
        with pytest.raises(NotImplementedError):
            Trainer(m)
        with pytest.raises(NotImplementedError):
            m.training_step(batch, 0)
    mlp = TR.mlp_model(TR.TOY, "vp")
    with pytest.raises(NotImplementedError, match="dropout"):
        Trainer(mlp, dropout=0.1)
    mlp.use_cache = True
    with pytest.raises(NotImplementedError, match="cache"):
        Trainer(mlp)
    mlp.use_cache = False
    mlp.fresca_enabled = True  # FreSca belongs to DiffusionSampler: no attribute of a model switches training off
    with pytest.raises(N.FFDError, match="cpu"):  # a model on the host: no CPU fallback
        Trainer(mlp)
    with pytest.raises(NotImplementedError):  # the closure keeps refusing: the training surface is Trainer
        get_sde_loss_fn(sch, train=True)
    assert mlp.set_loss_fn()[0] is None
