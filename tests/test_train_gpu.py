"""Training on the device (csrc/ffd_train.hip, fastfourierdiffusion_amd/training.py) against the float64 judge of
tests/train_restatement.py.

Bars.  Single operators and whole gradients: max(2e-6, 3 x the error of the same arithmetic in fp32 on the CPU), relative
to the expected array's max-norm (conftest.rel_err), the fp32 error measured inside the test; whole gradients per
parameter tensor.  Runs: 3 x the deviation of the CPU fp32 restatement of the same run, floor 1e-5 (the project's
trajectory bar).  The training forward: the forward bar of tests/transformer_restatement.py.  Every gradient case asserts
first that no hidden unit is near the ReLU kink (train_restatement.assert_no_kink).

The transformer and the MLP train; the LSTM and the mixture are refused (tested here and in test_train_host.py).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import train_restatement as TR
import transformer_restatement as R
from conftest import rel_err
from oracle import ffd_oracle as O
from transformer_restatement import TOL_SCORE, bar as forward_bar

pytestmark = pytest.mark.gpu

SDES = ("vp", "ve")


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else None


def check(what, got, want, e32, floor=2e-6):
    err, tol = rel_err(got, want), TR.bar(e32, floor)
    print(f"{what}: err {err:.2e} fp32-cpu {e32:.2e} bar {tol:.2e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err


# ---- operators ----------------------------------------------------------------------------------------------------------
# (M, N, K): one tile; edges in all three (K = 21 is no multiple of 4); several tiles and reduction stages; the FFN's
# width at few rows
GEMM_SHAPES = [(5, 7, 3), (85, 60, 21), (70, 130, 100), (33, 2048, 60), (130, 72, 187)]


# more than 65 535 row tiles: M lies on grid.x
DGRAD_SHAPES = GEMM_SHAPES + [(65536 * 64 + 1, 1, 2)]


@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=lambda s: "M{}N{}K{}".format(*s))
@pytest.mark.parametrize("mask,res", [(0, 0), (1, 0), (1, 1)])
def test_dense_dgrad(lib, shape, mask, res):
    M, N, K = shape
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    dY, W = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    act = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32) if mask else None
    R = rng.standard_normal((M, K)).astype(np.float32) if res else None

    def ref(dt):
        v = dY.astype(dt) @ W.astype(dt)
        if act is not None:
            v = np.where(act > 0, v, 0)
        return v + R.astype(dt) if R is not None else v

    bufs = [dev(dY), dev(W), dev(act) if mask else None, dev(R) if res else None, torch.zeros(M, K, device="cuda")]
    assert lib.ffd_dense_dgrad(*[ptr(b) for b in bufs], M, N, K, stream()) == 0
    want = ref(np.float64)
    check("dgrad", bufs[4].cpu().numpy(), want, rel_err(ref(np.float32), want))


# ... and several chunks plus a remainder: 40 chunks of 64 rows; 17 chunks, the last of one row; the MLP's embedder at
# B = 512 (8 chunks of 64 rows); an output with tiles enough (18 x 17) to be cut by rows alone: 1024 + 1024 + 952
WGRAD_SHAPES = GEMM_SHAPES + [(2560, 64, 8), (1025, 20, 70), (512, 72, 187), (3000, 1100, 1030)]
# chunks expected for each shape (the rule is restated in train_restatement.wgrad_chunks)
WGRAD_CHUNKS = {(5, 7, 3): 1, (85, 60, 21): 2, (70, 130, 100): 2, (33, 2048, 60): 1, (130, 72, 187): 3, (2560, 64, 8): 40,
                (1025, 20, 70): 17, (512, 72, 187): 8, (3000, 1100, 1030): 3}


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "M{}N{}K{}".format(*s))
@pytest.mark.parametrize("bias", [1, 0])
def test_dense_wgrad(lib, shape, bias):
    M, N, K = shape
    rng = np.random.default_rng(M + 3 * N + 7 * K + 1)
    dY, X = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, K)).astype(np.float32)
    chunks = lib.ffd_dense_wgrad_chunks(M, N, K)
    assert chunks == WGRAD_CHUNKS[shape] == TR.wgrad_chunks(M, N, K)[0]
    nbytes = lib.ffd_dense_wgrad_work_bytes(M, N, K)
    assert (nbytes == 0) == (chunks == 1) and nbytes == (chunks * N * 8 + chunks * N * K * 4 if chunks > 1 else 0)
    work = torch.empty(max(nbytes, 8) // 8, device="cuda", dtype=torch.float64)
    dW = torch.full((N, K), np.nan, device="cuda")
    db = torch.full((N,), np.nan, device="cuda") if bias else None
    a, b = dev(dY), dev(X)
    assert lib.ffd_dense_wgrad(a.data_ptr(), b.data_ptr(), dW.data_ptr(), ptr(db), M, N, K, work.data_ptr(), nbytes,
                               stream()) == 0
    want = dY.astype(np.float64).T @ X.astype(np.float64)
    check("wgrad dW", dW.cpu().numpy(), want, rel_err(dY.T @ X, want))
    if bias:
        wb = dY.astype(np.float64).sum(0)
        check("wgrad db", db.cpu().numpy(), wb, rel_err(dY.sum(0, dtype=np.float32), wb))
    if chunks > 1:  # too small a workspace is an argument error
        assert lib.ffd_dense_wgrad(a.data_ptr(), b.data_ptr(), dW.data_ptr(), ptr(db), M, N, K, work.data_ptr(),
                                   nbytes - 1, stream()) == -1


def table_G(lib, L):
    G = (C.c_float * L)()
    assert lib.ffd_host_noise_scaling(L, 1, G) == 0
    return np.array(G[:], dtype=np.float32)


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 5, 3), (5, 187, 1), (3, 24, 40)], ids=lambda s: "B{}L{}C{}".format(*s))
@pytest.mark.parametrize("lw", [0, 1])
def test_loss_gradient(lib, shape, lw):
    """Injected z: losses bit-equal to ffd_sm_loss, gradient against float64.  Philox z with an index: the same bits as
    the injected run of the draws ffd_sm_perturb makes for those global samples."""
    B, L, Cn = shape
    rng = np.random.default_rng(17 + B + L)
    score, z = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    sigma = np.geomspace(1e-3, 50.0, B).astype(np.float32)
    G = table_G(lib, L)
    ds, dg, dz, dG = dev(score), torch.zeros(shape, device="cuda"), dev(z), dev(G)
    dsig = dev(sigma)
    per, per0 = (torch.empty(B, device="cuda", dtype=torch.float64) for _ in range(2))
    assert lib.ffd_sm_loss_grad(ds.data_ptr(), dsig.data_ptr(), dG.data_ptr(), dz.data_ptr(), 0, 0, None, lw,
                                per.data_ptr(), dg.data_ptr(), B, L, Cn, stream()) == 0
    assert lib.ffd_sm_loss(ds.data_ptr(), dsig.data_ptr(), dG.data_ptr(), dz.data_ptr(), 0, 0, lw, 1, per0.data_ptr(),
                           B, L, Cn, stream()) == 0
    assert torch.equal(per, per0)

    def ref(dt):
        s = torch.from_numpy(score).to(dt).requires_grad_(True)
        std = torch.from_numpy(sigma).to(dt)[:, None] * torch.from_numpy(G).to(dt)[None, :]
        TR.per_sample_loss(s, torch.from_numpy(z).to(dt), std, lw).mean().backward()
        return s.grad.numpy()

    want = ref(torch.float64)
    check("dscore", dg.cpu().numpy(), want, rel_err(ref(torch.float32), want))
    # regenerated draws: rows idx of a 9-sample call at offset 4 under seed 12345
    idx = torch.tensor([(3 * b + 1) % 9 for b in range(B)], device="cuda")
    zall = torch.empty((9, L, Cn), device="cuda")
    ones, zeros = torch.ones(9, device="cuda"), torch.zeros((9, L, Cn), device="cuda")
    Gz = torch.ones(L, device="cuda")  # x_noisy = 0 x0 + (1 * 1) z: the draws themselves
    assert lib.ffd_sm_perturb(zeros.data_ptr(), zall.data_ptr(), zeros.data_ptr(), ones.data_ptr(), Gz.data_ptr(), None,
                              12345, 4, 9, L, Cn, stream()) == 0
    zi = zall[idx].contiguous()
    out = [(torch.empty(B, device="cuda", dtype=torch.float64), torch.zeros(shape, device="cuda")) for _ in range(2)]
    assert lib.ffd_sm_loss_grad(ds.data_ptr(), dsig.data_ptr(), dG.data_ptr(), zi.data_ptr(), 0, 0, None, lw,
                                out[0][0].data_ptr(), out[0][1].data_ptr(), B, L, Cn, stream()) == 0
    assert lib.ffd_sm_loss_grad(ds.data_ptr(), dsig.data_ptr(), dG.data_ptr(), None, 12345, 4, idx.data_ptr(), lw,
                                out[1][0].data_ptr(), out[1][1].data_ptr(), B, L, Cn, stream()) == 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("n", [1, 4097, 20000])
@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
def test_adamw_one_tensor(lib, n, clip):
    from fastfourierdiffusion_amd import _native as N

    rng = np.random.default_rng(n)
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m, v = 0.1 * rng.standard_normal(n).astype(np.float32), 0.01 * rng.random(n).astype(np.float32)
    sq = 9.0 if clip == "active" else 0.25  # the squared norm is an input of the operator: norm 3 clips, 0.5 does not
    max_norm = 0.0 if clip == "off" else 1.0
    step, lr = 7, 3e-4
    _, coef = TR.clip_coef([torch.tensor([np.sqrt(sq)])], max_norm)
    assert (coef < 1.0) == (clip == "active")

    def ref(dt):
        t = [torch.from_numpy(a.copy()).to(dt) for a in (p, g, m, v)]
        TR.adamw_step(t[0], t[1] * coef, t[2], t[3], step, lr)
        return [a.numpy() for a in (t[0], t[2], t[3])]

    bufs = [dev(a) for a in (p, g, m, v)]
    dsq = torch.tensor([sq], device="cuda", dtype=torch.float64)
    cfg = N.AdamWCfg(lr, 0.9, 0.999, 1e-8, 1e-2, max_norm, step)
    assert lib.ffd_adamw(*[b.data_ptr() for b in bufs], n, dsq.data_ptr(), C.byref(cfg), stream()) == 0
    assert torch.equal(bufs[1], dev(g)), "the gradient buffer keeps the unclipped gradient"
    for name, got, w64, w32 in zip(("param", "exp_avg", "exp_avg_sq"), (bufs[0], bufs[2], bufs[3]), ref(torch.float64),
                                   ref(torch.float32)):
        check(f"adamw {name}", got.cpu().numpy(), w64, rel_err(w32, w64))


def test_draw_times_at_are_the_rows_of_draw_times(lib):
    idx = torch.tensor([5, 0, 99, 37, 5, 64], device="cuda")
    full, at = torch.empty(100, device="cuda"), torch.empty(6, device="cuda")
    assert lib.ffd_sm_draw_times(full.data_ptr(), 100, 1e-5, 1.0, 777, 11, stream()) == 0
    assert lib.ffd_sm_draw_times_at(at.data_ptr(), idx.data_ptr(), 6, 1e-5, 1.0, 777, 11, stream()) == 0
    assert torch.equal(at, full[idx])


# ---- LayerNorm and attention operators on their own (the transformer's training path chains them) ---------------------------
@pytest.mark.parametrize("shape", [(1, 8), (85, 60), (130, 72), (2560, 24), (7, 200)], ids=lambda s: "M{}D{}".format(*s))
def test_layernorm_with_statistics_and_its_backward(lib, shape):
    M, D = shape
    rng = np.random.default_rng(M + D)
    x, dy = rng.standard_normal((M, D)).astype(np.float32) * 2 + 0.5, rng.standard_normal((M, D)).astype(np.float32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)

    def ref(dt):
        xt, g, b = (torch.from_numpy(a).to(dt).requires_grad_(True) for a in (x, gamma, beta))
        y = torch.nn.functional.layer_norm(xt, (D,), g, b, 1e-5)
        y.backward(torch.from_numpy(dy).to(dt))
        return [a.detach().numpy() for a in (y, xt.grad, g.grad, b.grad)]

    w64, w32 = ref(torch.float64), ref(torch.float32)
    dx_, dg_, db_ = dev(x), dev(gamma), dev(beta)
    y, xhat, rstd = torch.empty(M, D, device="cuda"), torch.empty(M, D, device="cuda"), torch.empty(M, device="cuda")
    assert lib.ffd_layernorm_stats_fwd(dx_.data_ptr(), dg_.data_ptr(), db_.data_ptr(), y.data_ptr(), xhat.data_ptr(),
                                       rstd.data_ptr(), M, D, 1e-5, stream()) == 0
    ddy, gx, gg, gb = dev(dy), torch.empty(M, D, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    assert lib.ffd_layernorm_bwd(ddy.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), dg_.data_ptr(), gx.data_ptr(),
                                 gg.data_ptr(), gb.data_ptr(), M, D, stream()) == 0
    for what, got, a, b in zip(("y", "dx", "dgamma", "dbeta"), (y, gx, gg, gb), w64, w32):
        check(f"layernorm {what}", got.cpu().numpy(), a, rel_err(b, a))
    x64 = x.astype(np.float64)
    want_rstd = 1.0 / np.sqrt(x64.var(1) + 1e-5)
    check("layernorm rstd", rstd.cpu().numpy(), want_rstd, rel_err(1.0 / np.sqrt(x.var(1) + np.float32(1e-5)), want_rstd))


# (B, L, H, head_dim): every head dimension, L = 1, a length that is no multiple of the 256 threads, the longest length
ATTN_SHAPES = [(3, 5, 2, 4), (5, 17, 12, 5), (4, 33, 12, 6), (2, 16, 12, 2), (2, 16, 8, 3), (2, 64, 6, 8), (2, 300, 2, 8),
               (5, 512, 1, 8), (1, 1, 2, 4), (2, 7, 3, 1)]


# ... and scores far from zero by a shift common to a query row (list E of tests/transformer_restatement.py): dimension 0 of
# each of the twelve heads carries head_plan's constant (+- 150 / 200 log2 units), key staircase or per-query offset
SHIFTED_ATTN_SHAPES = [(2, 33, 12, 5, "shifted"), (2, 187, 12, 5, "shifted"), (2, 33, 12, 6, "shifted"), (2, 187, 12, 6, "shifted")]


def shifted_qkv(qkv, B, L, H, hd):
    """Standard-normal q | k | v rows with dimension 0 of every head's q and k set as shift_state_dict's projections
    would set them."""
    d, qs = H * hd, R.LOG2E / np.sqrt(hd)
    rows = qkv.reshape(B, L, 3 * d)
    stairs = R.e_inputs(torch.zeros(1, L, 2))[0].numpy()  # (L, 2): the staircase and the -1, 0, 1 pattern
    for h, (kind, par) in enumerate(R.head_plan(H)):
        q0, k0 = rows[:, :, h * hd], rows[:, :, d + h * hd]
        if kind == "const":
            q0[:], k0[:] = np.sqrt(abs(par) / qs), np.copysign(np.sqrt(abs(par) / qs), par)
        elif kind == "ramp_k":
            g = np.sqrt(R.E_RAMP_K / qs)
            q0[:], k0[:] = g, g * (stairs[None, :, 0] + par + R.E_NOISE * k0)
        elif kind == "ramp_q":
            g = np.sqrt(R.E_RAMP_Q / qs)
            k0[:], q0[:] = g, g * (stairs[None, :, 1] + R.E_NOISE * q0)
    return qkv


@pytest.mark.parametrize("shape", ATTN_SHAPES + SHIFTED_ATTN_SHAPES,
                         ids=lambda s: "B{}L{}H{}hd{}".format(*s) + ("_shifted" if len(s) > 4 else ""))
def test_attention_with_lse_and_its_backward(lib, shape):
    B, L, H, hd = shape[:4]
    d = H * hd
    rng = np.random.default_rng(B + 3 * L + 5 * H + 7 * hd)
    qkv, dout = rng.standard_normal((B * L, 3 * d)).astype(np.float32), rng.standard_normal((B * L, d)).astype(np.float32)
    if len(shape) > 4:
        qkv = shifted_qkv(qkv, B, L, H, hd)
        s0 = qkv.reshape(B, L, 3, H, hd).astype(np.float64)
        top = np.abs(np.einsum("blhe,bmhe->bhlm", s0[:, :, 0], s0[:, :, 1])).max() * R.LOG2E / np.sqrt(hd)
        assert top > 2 * R.ATTN_T, top

    def ref(dt):
        t = torch.from_numpy(qkv).to(dt).requires_grad_(True)
        q, k, v = (a.reshape(B, L, H, hd).transpose(1, 2) for a in t.split(d, dim=-1))
        s = torch.matmul(q, k.transpose(-2, -1)) / (hd ** 0.5)
        o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B * L, d)
        o.backward(torch.from_numpy(dout).to(dt))
        return [a.detach().numpy() for a in (o, torch.logsumexp(s, dim=-1), t.grad)]

    w64, w32 = ref(torch.float64), ref(torch.float32)
    dq, out, lse = dev(qkv), torch.full((B * L, d), np.nan, device="cuda"), torch.empty(B, H, L, device="cuda")
    assert lib.ffd_attention_lse_fwd(dq.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, hd, stream()) == 0
    dd, dqkv = dev(dout), torch.full((B * L, 3 * d), np.nan, device="cuda")
    assert lib.ffd_attention_bwd(dq.data_ptr(), out.data_ptr(), dd.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), B, L, H, hd,
                                 stream()) == 0
    for what, got, a, b in zip(("out", "lse", "dqkv"), (out, lse, dqkv), w64, w32):
        check(f"attention {what}", got.cpu().numpy(), a, rel_err(b, a))
    assert lib.ffd_attention_lse_fwd(dq.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, 513, 1, 8, stream()) == -2
    assert lib.ffd_attention_bwd(dq.data_ptr(), out.data_ptr(), dd.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), 1, 4, 1, 9,
                                 stream()) == -2


# ---- whole gradients ------------------------------------------------------------------------------------------------------
def make_trainer(model, **kw):
    from fastfourierdiffusion_amd.training import Trainer

    return Trainer(model.cuda(), **kw)


def grads_of(model):
    return {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad}


GRAD_CASES = [(c, sde, lw) for c in TR.MLP_CASES for sde in SDES for lw in ((False, True) if c is TR.MLP_CASES[0] else (False,))]


@pytest.mark.parametrize("case,sde,lw", GRAD_CASES, ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_mlp_whole_gradient(lib, case, sde, lw):
    """Measured on an MI355X: see DESIGN.md section 5 (per-tensor device error over the fp32 CPU autograd's error)."""
    model, sd, (x0, t, mc, sigma, z) = TR.case_setup(case, sde, lw)
    G = model.noise_scheduler.G.numpy()
    margin, e32 = TR.assert_no_kink(sd, case["NL"], x0, t, mc, sigma, G, z, case["name"])
    print(f"kink margin {margin:.2e}, fp32 pre-activation error {e32:.2e}")
    l64, per64, g64 = TR.mlp_gradients(sd, case["NL"], x0, t, mc, sigma, G, z, lw, torch.float64)
    l32, per32, g32 = TR.mlp_gradients(sd, case["NL"], x0, t, mc, sigma, G, z, lw, torch.float32)
    tr = make_trainer(model)
    loss = tr.loss_and_grad(dev(x0), timesteps=dev(t), z=dev(z))
    check("per-sample loss", tr.last_per_sample.cpu().numpy(), per64, rel_err(per32, per64))
    assert abs(float(loss) - l64) <= TR.bar(abs(l32 - l64) / abs(l64)) * abs(l64) + 1e-7 * abs(l64)
    got = grads_of(model)
    assert set(got) == set(g64)
    worst = 0.0
    for k in g64:
        worst = max(worst, check(k, got[k], g64[k], rel_err(g32[k], g64[k])))
    print(f"{case['name']} {sde} lw={lw}: worst per-tensor gradient error {worst:.2e}")
    assert model.time_encoder.W.grad is None


@pytest.mark.parametrize("case", TR.MLP_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("sde", SDES)
def test_training_forward_against_the_inference_forward(lib, case, sde):
    """Both forwards within the float64-judged forward bar on the same weights."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    model, sd, (x0, t, mc, sigma, z) = TR.case_setup(case, sde)
    xn = TR.perturb(*[torch.from_numpy(a) for a in (x0, z, mc, sigma)], model.noise_scheduler.G)[0].numpy()
    with torch.no_grad():
        want = O.mlp_score_forward(torch.from_numpy(xn).double(), torch.from_numpy(t).double(), TR.cast(sd, torch.float64),
                                   case["NL"]).numpy()
        e32 = rel_err(O.mlp_score_forward(torch.from_numpy(xn), torch.from_numpy(t), sd, case["NL"]).numpy(), want)
    tr = make_trainer(model)
    dx, dt = dev(xn), dev(t)
    out = torch.empty_like(dx)
    tr._check(lib.ffd_train_forward(tr.handle, dx.data_ptr(), dt.data_ptr(), out.data_ptr(), case["B"], stream()), "forward")
    inf = model.eval()(DiffusableBatch(X=dx, timesteps=dt))
    for what, got in (("training forward", out), ("inference forward", inf)):
        err = rel_err(got.cpu().numpy(), want)
        print(f"{what}: {err:.2e} (fp32 cpu {e32:.2e}, bar {forward_bar(e32):.2e})")
        assert err <= forward_bar(e32)
    assert TOL_SCORE == 1e-5


# ---- updates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sde,clipped", [("ve", True), ("vp", False)])
def test_three_updates(lib, sde, clipped):
    """Three consecutive steps at the first MLP case from fixed weights with injected t and z: parameters and both moments
    against float64.  VE at init clips at every step, VP never; step 0 runs at lr = 0 (100 warm-up steps): it moves the
    moments only."""
    case = TR.MLP_CASES[0]
    model, sd, _ = TR.case_setup(case, sde)
    sch = model.noise_scheduler
    G = sch.G.numpy()
    runs = {dt: TR.MlpRun(sd, case["NL"], G, False, model.lr_max, model.num_warmup_steps, model.num_training_steps, dt)
            for dt in (torch.float64, torch.float32)}
    tr = make_trainer(model)
    assert tr.lr(0) == 0.0 and model.num_warmup_steps == 100
    losses = []
    for k in range(3):
        x0, t, mc, sigma, z = TR.case_inputs(case, sch, k)
        TR.assert_no_kink(runs[torch.float64].state(), case["NL"], x0, t, mc, sigma, G, z, f"step {k}")
        ref = [runs[dt].step(x0, t, mc, sigma, z) for dt in runs]
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        losses.append((float(tr.step(dev(x0), timesteps=dev(t), z=dev(z))), ref[0]))
        if k == 0:
            assert all(torch.equal(before[n], p) for n, p in model.named_parameters()), "lr = 0 must not move a parameter"
    r64, r32 = runs[torch.float64], runs[torch.float32]
    assert all((c < 1.0) == clipped for c in r64.coefs), r64.norms
    for got, want in losses:
        assert abs(got - want) <= 1e-5 * abs(want)
    for k, p in model.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p.cpu(), sd[k]), "the frozen tensor moved"
            continue
        for what, got, a, b in (("param", p, r64.p[k], r32.p[k]), ("exp_avg", tr.exp_avg[k], r64.m[k], r32.m[k]),
                                ("exp_avg_sq", tr.exp_avg_sq[k], r64.v[k], r32.v[k])):
            a, b = a.detach().numpy(), b.detach().numpy()
            check(f"{k} {what}", got.detach().cpu().numpy(), a, rel_err(b, a))


# ---- the toy runs ---------------------------------------------------------------------------------------------------------
_TOY = {}


def toy(sde):
    """One device run and the float64 / fp32 restatements of the 200-step toy, shared by the tests below."""
    if sde in _TOY:
        return _TOY[sde]
    c = TR.TOY
    X = TR.toy_dataset(c["n"], c["L"], c["C"])
    Xv = TR.toy_dataset(64, c["L"], c["C"], seed=12)
    model = TR.mlp_model(c, sde, total=c["total"], lr_max=c["lr_max"])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sch = model.noise_scheduler
    ref = {}
    for dt in (torch.float64, torch.float32):
        run, losses, snaps = TR.toy_run(sd, c["NL"], sch, False, X, 200, c["B"], c["seed"], c["lr_max"], c["total"] // 10,
                                        c["total"], dt, snapshots=(20, 200))
        ref[dt] = dict(losses=losses, snaps=snaps, val0=TR.validation_loss(sd, c["NL"], sch, False, Xv, c["seed"]),
                       val=TR.validation_loss(snaps[200], c["NL"], sch, False, Xv, c["seed"]))
    tr = make_trainer(model, seed=c["seed"])
    dX = dev(X)
    order = [torch.from_numpy(tr.epoch_order(c["n"], e)).cuda() for e in range(3)]
    loop, at20 = [], None
    for k in range(24):  # three whole epochs by hand; the parameters after step 20
        loop.append(tr.step(dX, index=order[k // 8][(k % 8) * c["B"]:(k % 8 + 1) * c["B"]]))
        if k == 19:
            at20 = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    _TOY[sde] = dict(model=model, tr=tr, X=dX, Xv=dev(Xv), ref=ref, loop=torch.stack(loop).cpu().numpy(), at20=at20, sd=sd)
    return _TOY[sde]


@pytest.mark.parametrize("sde", SDES)
def test_short_run_20_steps(lib, sde):
    """20 steps of the MLP (L = 12, C = 2, d = 24, d_mlp = 64, NL = 2, B = 32) on the two-mode toy set with the device's
    own draws (restated through philox_restatement): loss curve and parameters against float64, bar 3 x the deviation of
    the fp32 restatement, floor 1e-5."""
    T = toy(sde)
    r64, r32 = T["ref"][torch.float64], T["ref"][torch.float32]
    dev32 = rel_err(r32["losses"][:20], r64["losses"][:20])
    assert dev32 < 1e-2, "the fp32 restatement itself turned chaotic: shorten the run"
    check("loss curve", T["loop"][:20], r64["losses"][:20], dev32, floor=1e-5)
    for k, want in r64["snaps"][20].items():
        check(k, T["at20"][k], want, rel_err(r32["snaps"][20][k], want), floor=1e-5)


@pytest.mark.parametrize("sde", SDES)
def test_200_steps_lower_the_validation_loss(lib, sde):
    """fit continues the hand-written loop's 24 steps to 200 (epochs 3 .. 24 of 8 batches).  The fixed-draw validation
    loss against the float64 restatement's, bar 3 x the fp32 restatement's deviation (floor 1e-5); and it fell."""
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    T = toy(sde)
    tr, c = T["tr"], TR.TOY
    if tr.global_step == 24:
        tr.fit(T["X"], batch_size=c["B"], max_epochs=22)
    assert tr.global_step == 200
    r64, r32 = T["ref"][torch.float64], T["ref"][torch.float32]
    val = float(evaluate_loss(T["model"], T["Xv"], 64, seed=c["seed"])["loss"])
    print(f"{sde}: validation loss {r64['val0']:.5f} -> device {val:.5f}, float64 {r64['val']:.5f}, fp32 {r32['val']:.5f}")
    assert r64["val"] < r64["val0"] and val < r64["val0"]
    dev32 = abs(r32["val"] - r64["val"]) / r64["val"]
    assert abs(val - r64["val"]) / r64["val"] <= TR.bar(dev32, floor=1e-5), (val, r64["val"], r32["val"])


# ---- the transformer ----------------------------------------------------------------------------------------------------------
TF_GRAD_CASES = [(c, sde, lw) for i, c in enumerate(TR.TF_CASES) for sde in SDES for lw in ((False, True) if i < 2 else (False,))]


@pytest.mark.parametrize("case,sde,lw", TF_GRAD_CASES, ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_transformer_whole_gradient(lib, case, sde, lw):
    """Every parameter tensor's gradient against float64 autograd of the oracle's score_forward, the positional rows
    renormalised first and treated as the leaf.  Measured on an MI355X: DESIGN.md section 5."""
    model, sd, (x0, t, mc, sigma, z) = TR.tf_case_setup(case, sde, lw)
    NL, H, G = case["NL"], case["H"], model.noise_scheduler.G.numpy()
    margin, e32 = TR.tf_assert_no_kink(sd, NL, H, x0, t, mc, sigma, G, z, case["name"])
    print(f"kink margin {margin:.2e}, fp32 pre-activation error {e32:.2e}")
    if case["name"].startswith("c2_"):  # rows above max_norm are renormalised, rows below are left: both occur at d = 60
        norms = sd[TR.POS].norm(dim=1)
        assert bool((norms > np.sqrt(case["d"])).any()) and bool((norms < np.sqrt(case["d"])).any())
    l64, per64, g64 = TR.tf_gradients(sd, NL, H, x0, t, mc, sigma, G, z, lw, torch.float64)
    l32, per32, g32 = TR.tf_gradients(sd, NL, H, x0, t, mc, sigma, G, z, lw, torch.float32)
    tr = make_trainer(model)
    if case["name"].startswith("c8_"):  # M = 2560 rows: the FFN's wgrads run in several chunks plus a remainder
        M = case["B"] * case["L"]
        assert lib.ffd_dense_wgrad_chunks(M, case["F"], case["d"]) == TR.wgrad_chunks(M, case["F"], case["d"])[0] == 40
        assert tr.work_bytes(case["B"]) > tr.work_bytes(1) > 0
    loss = tr.loss_and_grad(dev(x0), timesteps=dev(t), z=dev(z))
    check("per-sample loss", tr.last_per_sample.cpu().numpy(), per64, rel_err(per32, per64))
    assert abs(float(loss) - l64) <= TR.bar(abs(l32 - l64) / abs(l64)) * abs(l64) + 1e-7 * abs(l64)
    got = grads_of(model)
    assert set(got) == set(g64)
    worst = 0.0
    for k in g64:
        worst = max(worst, check(k, got[k], g64[k], rel_err(g32[k], g64[k])))
    print(f"{case['name']} {sde} lw={lw}: worst per-tensor gradient error {worst:.2e}")
    # the parameter itself now holds the renormalised rows
    assert rel_err(model.pos_encoder.embedding.weight.detach().cpu().numpy(), TR.renormed(sd)[TR.POS].numpy()) < 2e-6


@pytest.mark.parametrize("case", TR.TF_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("sde", SDES)
def test_transformer_training_forward_against_the_inference_forward(lib, case, sde):
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    model, sd, (x0, t, mc, sigma, z) = TR.tf_case_setup(case, sde)
    xn = TR.perturb(*[torch.from_numpy(a) for a in (x0, z, mc, sigma)], model.noise_scheduler.G)[0].numpy()
    with torch.no_grad():
        want = O.score_forward(torch.from_numpy(xn).double(), torch.from_numpy(t).double(), TR.cast(TR.renormed(sd), torch.float64),
                               case["NL"], case["H"]).numpy()
        e32 = rel_err(O.score_forward(torch.from_numpy(xn), torch.from_numpy(t), sd, case["NL"], case["H"]).numpy(), want)
    tr = make_trainer(model)
    dx, dt = dev(xn), dev(t)
    inf = model.eval()(DiffusableBatch(X=dx, timesteps=dt))
    out = torch.empty_like(dx)
    tr._check(lib.ffd_train_forward(tr.handle, dx.data_ptr(), dt.data_ptr(), out.data_ptr(), case["B"], stream()), "forward")
    for what, got in (("training forward", out), ("inference forward", inf)):
        err = rel_err(got.cpu().numpy(), want)
        print(f"{what}: {err:.2e} (fp32 cpu {e32:.2e}, bar {forward_bar(e32):.2e})")
        assert err <= forward_bar(e32)


def test_transformer_training_forward_against_the_inference_forward_on_shifted_scores(lib):
    """A network off the init scale (list E of tests/transformer_restatement.py, head_dim 5, two key tiles): the training
    forward (exact row maximum) and the fused inference forward (reference 0, refreshed) agree with float64 and so with
    each other."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = next(c for c in R.E_CASES if c["name"] == "E_d60_hd5_L33_B3")
    m, rec = c["model"], R.reference(c)[0]
    assert rec["events"]["first_pos"] and rec["events"]["first_neg"] and rec["events"]["later"]
    model = TR.tf_model(dict(L=m["L"], C=m["C"], d=m["d"], H=m["H"], NL=m["NL"], F=m["F"], wseed=1), "vp")
    model.load_state_dict(R.state_dict(m), strict=True)
    tr = make_trainer(model)
    dx, dt = R.inputs(c, 0).cuda(), torch.full((c["B"],), c["t"], dtype=torch.float32, device="cuda")
    inf = model.eval()(DiffusableBatch(X=dx, timesteps=dt))
    out = torch.empty_like(dx)
    tr._check(lib.ffd_train_forward(tr.handle, dx.data_ptr(), dt.data_ptr(), out.data_ptr(), c["B"], stream()), "forward")
    for what, got in (("training forward", out), ("inference forward", inf)):
        err = rel_err(got.cpu().numpy(), rec["score"].numpy())
        print(f"{what}: {err:.2e} (fp32 cpu {rec['e32']:.2e}, bar {forward_bar(rec['e32']):.2e})")
        assert torch.isfinite(got).all() and err <= forward_bar(rec["e32"])


class TfRun(TR.MlpRun):
    """MlpRun with the transformer's loss: the positional rows are renormalised in place before every step."""

    def __init__(self, sd, NL, H, *a, **kw):
        super().__init__(sd, NL, *a, **kw)
        self.H = H

    def step(self, x0, t, mc, sigma, z):
        import math

        with torch.no_grad():
            self.p[TR.POS].copy_(O.renorm_embedding(self.p[TR.POS].detach(), math.sqrt(self.p[TR.POS].shape[1])).to(self.dtype))
        for k, v in self.p.items():
            v.grad = None
            v.requires_grad_(k not in TR.FROZEN)
        loss = TR.tf_loss(self.p, self.NL, self.H, x0, t, mc, sigma, self.G, z, self.lw, self.dtype)[0]
        loss.backward()
        names = list(self.m)
        norm, coef = TR.clip_coef([self.p[k].grad for k in names], self.grad_clip)
        self.norms.append(norm), self.coefs.append(coef)
        lr = self.lr_max * TR.lr_lambda(self.k, self.warmup, self.total)
        with torch.no_grad():
            for k in names:
                TR.adamw_step(self.p[k], self.p[k].grad * coef, self.m[k], self.v[k], self.k + 1, lr, self.betas, self.eps, self.wd)
        self.k += 1
        return float(loss.detach())


@pytest.mark.parametrize("ci", [0, 1])
@pytest.mark.parametrize("sde", SDES)
def test_transformer_three_updates(lib, ci, sde):
    """Three consecutive steps at transformer cases 1 and 2 from fixed weights with injected t and z: parameters and both
    moments against float64.  Step 0 runs at lr = 0 (100 warm-up steps); whether a step clips is read from the float64
    run and printed (VE at init clips, VP does not)."""
    case = TR.TF_CASES[ci]
    model, sd, _ = TR.tf_case_setup(case, sde)
    sch = model.noise_scheduler
    G = sch.G.numpy()
    runs = {dt: TfRun(sd, case["NL"], case["H"], G, False, model.lr_max, model.num_warmup_steps, model.num_training_steps, dt)
            for dt in (torch.float64, torch.float32)}
    tr = make_trainer(model)
    assert tr.lr(0) == 0.0
    for k in range(3):
        x0, t, mc, sigma, z = TR.case_inputs(case, sch, k)
        TR.tf_assert_no_kink(runs[torch.float64].state(), case["NL"], case["H"], x0, t, mc, sigma, G, z, f"step {k}")
        ref = [runs[dt].step(x0, t, mc, sigma, z) for dt in runs]
        got = float(tr.step(dev(x0), timesteps=dev(t), z=dev(z)))
        assert abs(got - ref[0]) <= 1e-5 * abs(ref[0])
    r64, r32 = runs[torch.float64], runs[torch.float32]
    print(f"{case['name']} {sde}: clip coefficients {r64.coefs}")
    assert all(c < 1.0 for c in r64.coefs) == (sde == "ve") or ci == 1
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        for what, got, a, b in (("param", p, r64.p[k], r32.p[k]), ("exp_avg", tr.exp_avg[k], r64.m[k], r32.m[k]),
                                ("exp_avg_sq", tr.exp_avg_sq[k], r64.v[k], r32.v[k])):
            a, b = a.detach().numpy(), b.detach().numpy()
            check(f"{k} {what}", got.detach().cpu().numpy(), a, rel_err(b, a))


_TF_TOY = {}


def tf_toy(sde):
    """The 200-step toy on the named transformer (L = 12, C = 2, d = 24, H = 4, F = 64, NL = 2, B = 32): one device run and
    the float64 / fp32 restatements with the device's own draws."""
    if sde in _TF_TOY:
        return _TF_TOY[sde]
    c = TR.TF_TOY
    X, Xv = TR.toy_dataset(c["n"], c["L"], c["C"]), TR.toy_dataset(64, c["L"], c["C"], seed=12)
    model = TR.tf_model(c, sde, total=c["total"], lr_max=c["lr_max"])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sch = model.noise_scheduler
    G = sch.G.numpy()

    def val(p, dt=torch.float64):
        t, z = TR.device_draws(c["seed"], 0, 64, c["L"], c["C"], sch.eps, sch.T)
        mc, sigma = (v.numpy() for v in sch.marginal_coeffs(torch.from_numpy(t)))
        with torch.no_grad():
            return float(TR.tf_loss(TR.cast(TR.renormed(p), dt), c["NL"], c["H"], Xv, t, mc, sigma, G, z, False, dt)[0])

    ref = {}
    for dt in (torch.float64, torch.float32):
        run = TfRun(sd, c["NL"], c["H"], G, False, c["lr_max"], c["total"] // 10, c["total"], dt)
        losses, snaps, order = [], {}, None
        for k in range(200):
            e, i = divmod(k, 8)
            if i == 0:
                order = TR.epoch_order(c["seed"], e, c["n"])
            idx = order[i * c["B"]:(i + 1) * c["B"]]
            t, z = TR.device_draws(c["seed"], k, c["n"], c["L"], c["C"], sch.eps, sch.T)
            mc, sigma = (v.numpy() for v in sch.marginal_coeffs(torch.from_numpy(t)))
            losses.append(run.step(X[idx], t[idx], mc[idx], sigma[idx], z[idx]))
            if k + 1 in (20, 200):
                snaps[k + 1] = run.state()
        ref[dt] = dict(losses=np.array(losses), snaps=snaps, val0=val(sd), val=val(snaps[200]))
    tr = make_trainer(model, seed=c["seed"])
    dX = dev(X)
    order = [torch.from_numpy(tr.epoch_order(c["n"], e)).cuda() for e in range(3)]
    loop, at20 = [], None
    for k in range(24):
        loop.append(tr.step(dX, index=order[k // 8][(k % 8) * c["B"]:(k % 8 + 1) * c["B"]]))
        if k == 19:
            at20 = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    _TF_TOY[sde] = dict(model=model, tr=tr, X=dX, Xv=dev(Xv), ref=ref, loop=torch.stack(loop).cpu().numpy(), at20=at20)
    return _TF_TOY[sde]


@pytest.mark.parametrize("sde", SDES)
def test_transformer_short_run_20_steps(lib, sde):
    """20 steps (the length the issue names; the fp32 restatement stays far from chaotic) against float64: loss curve and
    parameters, bar 3 x the fp32 restatement's deviation, floor 1e-5."""
    T = tf_toy(sde)
    r64, r32 = T["ref"][torch.float64], T["ref"][torch.float32]
    dev32 = rel_err(r32["losses"][:20], r64["losses"][:20])
    assert dev32 < 1e-2, "the fp32 restatement itself turned chaotic: shorten the run"
    check("loss curve", T["loop"][:20], r64["losses"][:20], dev32, floor=1e-5)
    for k, want in r64["snaps"][20].items():
        check(k, T["at20"][k], want, rel_err(r32["snaps"][20][k], want), floor=1e-5)


@pytest.mark.parametrize("sde", SDES)
def test_transformer_200_steps_lower_the_validation_loss(lib, sde):
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    T = tf_toy(sde)
    tr, c = T["tr"], TR.TF_TOY
    if tr.global_step == 24:
        tr.fit(T["X"], batch_size=c["B"], max_epochs=22)
    assert tr.global_step == 200
    r64, r32 = T["ref"][torch.float64], T["ref"][torch.float32]
    val = float(evaluate_loss(T["model"], T["Xv"], 64, seed=c["seed"])["loss"])
    print(f"{sde}: validation loss {r64['val0']:.5f} -> device {val:.5f}, float64 {r64['val']:.5f} "
          f"({r64['val'] / r64['val0']:.3f}), fp32 {r32['val']:.5f}")
    assert r64["val"] < r64["val0"] and val < r64["val0"]
    dev32 = abs(r32["val"] - r64["val"]) / r64["val"]
    assert abs(val - r64["val"]) / r64["val"] <= TR.bar(dev32, floor=1e-5), (val, r64["val"], r32["val"])


def test_transformer_after_fit_and_bit_identity(lib, tmp_path):
    """fit against a hand-written loop and a second run bit for bit; save -> resume; the trained model through forward
    (the context is invalidated) and the sampler."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = TR.TF_TOY
    X = dev(TR.toy_dataset(c["n"], c["L"], c["C"]))

    def new(seed=3):
        m = TR.tf_model(c, "vp", total=c["total"], lr_max=c["lr_max"])
        return m, make_trainer(m, seed=seed)

    m1, t1 = new()
    batch = DiffusableBatch(X=X[:7].contiguous(), timesteps=torch.linspace(0.1, 1.0, 7).cuda())
    before = m1.eval()(batch).clone()
    h1 = t1.fit(X, batch_size=c["B"], max_epochs=2)["train_loss"]
    m2, t2 = new()
    h2 = []
    for e in range(2):
        order = torch.from_numpy(t2.epoch_order(c["n"], e)).cuda()
        for i in range(0, c["n"], c["B"]):
            h2.append(t2.loss_and_grad(X, index=order[i:i + c["B"]]))
            t2.apply_update(t2.grad_sqnorm())
    assert torch.equal(h1, torch.stack(h2)) and same(params_of(m1), params_of(m2)) and same(t1.exp_avg_sq, t2.exp_avg_sq)
    m3, t3 = new()
    t3.fit(X, batch_size=c["B"], max_epochs=1)
    t3.save_checkpoint(tmp_path / "tf.ckpt")
    m4, t4 = new(seed=9)
    t4.resume(tmp_path / "tf.ckpt")
    assert torch.equal(t4.fit(X, batch_size=c["B"], max_epochs=1)["train_loss"], h1[8:]) and same(params_of(m1), params_of(m4))
    sd = {k: v.detach().cpu() for k, v in m1.state_dict().items()}
    with torch.no_grad():
        want = O.score_forward(batch.X.cpu().double(), batch.timesteps.cpu().double(), TR.cast(TR.renormed(sd), torch.float64),
                               c["NL"], c["H"]).numpy()
        e32 = rel_err(O.score_forward(batch.X.cpu(), batch.timesteps.cpu(), sd, c["NL"], c["H"]).numpy(), want)
    assert rel_err(m1.eval()(batch).cpu().numpy(), want) <= forward_bar(e32)
    assert rel_err(before.cpu().numpy(), want) > 10 * forward_bar(e32), "training must have moved the score"
    x = DiffusionSampler(m1, sample_batch_size=4).sample(num_samples=4, num_diffusion_steps=5)
    assert x.shape == (4, c["L"], c["C"]) and bool(torch.isfinite(x).all())


# ---- bit identity -----------------------------------------------------------------------------------------------------------
def fresh(sde="vp", seed=3, c=None):
    c = TR.TOY if c is None else c
    model = TR.mlp_model(c, sde, total=c.get("total", 1000), lr_max=c.get("lr_max", 1e-3))
    return model, make_trainer(model, seed=seed)


def params_of(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_bit_identity(lib, tmp_path):
    c = TR.TOY
    X = dev(TR.toy_dataset(c["n"], c["L"], c["C"]))
    # run to run; fit against a hand-written loop of step
    m1, t1 = fresh()
    h1 = t1.fit(X, batch_size=c["B"], max_epochs=2)["train_loss"]
    m2, t2 = fresh()
    h2 = []
    for e in range(2):
        order = torch.from_numpy(t2.epoch_order(c["n"], e)).cuda()
        h2 += [t2.step(X, index=order[i:i + c["B"]]) for i in range(0, c["n"], c["B"])]
    assert torch.equal(h1, torch.stack(h2)) and same(params_of(m1), params_of(m2))
    m3, t3 = fresh()
    assert torch.equal(t3.fit(X, batch_size=c["B"], max_epochs=2)["train_loss"], h1) and same(params_of(m1), params_of(m3))
    # the fused step against loss_and_grad + norm + AdamW
    m4, t4 = fresh()
    h4 = []
    for e in range(2):
        order = torch.from_numpy(t4.epoch_order(c["n"], e)).cuda()
        for i in range(0, c["n"], c["B"]):
            h4.append(t4.loss_and_grad(X, index=order[i:i + c["B"]]))
            t4.apply_update(t4.grad_sqnorm())
    assert torch.equal(h1, torch.stack(h4)) and same(params_of(m1), params_of(m4))
    assert same(t1.exp_avg, t4.exp_avg) and same(t1.exp_avg_sq, t4.exp_avg_sq)
    # save -> resume against the uninterrupted run
    m5, t5 = fresh()
    t5.fit(X, batch_size=c["B"], max_epochs=1)
    t5.save_checkpoint(tmp_path / "e0.ckpt")
    m6, t6 = fresh(seed=99)
    torch.manual_seed(1234)
    with torch.no_grad():
        for p in m6.parameters():
            p.copy_(torch.randn_like(p))
    t6.resume(tmp_path / "e0.ckpt")
    assert t6.global_step == 8 and t6.seed == 3
    h6 = t6.fit(X, batch_size=c["B"], max_epochs=1)["train_loss"]
    assert torch.equal(h6, h1[8:]) and same(params_of(m1), params_of(m6)) and same(t1.exp_avg_sq, t6.exp_avg_sq)
    # load_from_checkpoint reads the saved file: the parameters exactly
    from fastfourierdiffusion_amd.models.score_models import MLPScoreModule

    t1.save_checkpoint(tmp_path / "e1.ckpt")
    m7 = MLPScoreModule.load_from_checkpoint(tmp_path / "e1.ckpt")
    assert all(torch.equal(v, m1.state_dict()[k].cpu()) for k, v in m7.state_dict().items())
    assert m7.d_mlp == c["F"] and m7.num_training_steps == c["total"]


def test_a_rows_draw_does_not_depend_on_its_batch(lib):
    c = TR.TOY
    X = dev(TR.toy_dataset(c["n"], c["L"], c["C"]))
    _, tr = fresh()
    a = torch.tensor([5, 17, 200, 3, 64], device="cuda")
    b = torch.tensor([64, 9, 5, 255, 200, 17, 0, 3], device="cuda")
    tr.loss_and_grad(X, index=a)
    pa = tr.last_per_sample.clone()
    tr.loss_and_grad(X, index=b)
    pb = tr.last_per_sample.clone()
    pos = {int(r): i for i, r in enumerate(b.tolist())}
    assert all(pa[i] == pb[pos[int(r)]] for i, r in enumerate(a.tolist()))
    # ... and it is evaluate_loss's draw of that row: the same key, counted by data-set row
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    tr.model.eval()
    ev = evaluate_loss(tr.model, X, 64, seed=tr.seed)["per_sample"][0]
    # (two implementations of the forward, each within 1e-5 of the score; a loss term moves by twice that per unit of
    # |score| / |r|, below 2.5 at the initialisation)
    assert rel_err(pa.cpu().numpy(), ev[a].cpu().numpy()) < 5e-5


# ---- after fit ------------------------------------------------------------------------------------------------------------
def test_the_trained_model_is_what_inference_runs(lib):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = TR.TOY
    X = dev(TR.toy_dataset(c["n"], c["L"], c["C"]))
    model, tr = fresh()
    batch = DiffusableBatch(X=X[:7].contiguous(), timesteps=torch.linspace(0.1, 1.0, 7).cuda())
    before = model.eval()(batch).clone()  # creates the inference context on the initial weights
    tr.fit(X, batch_size=c["B"], max_epochs=3)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want = O.mlp_score_forward(batch.X.cpu().double(), batch.timesteps.cpu().double(), TR.cast(sd, torch.float64),
                                   c["NL"]).numpy()
        e32 = rel_err(O.mlp_score_forward(batch.X.cpu(), batch.timesteps.cpu(), sd, c["NL"]).numpy(), want)
    after = model.eval()(batch)
    assert rel_err(after.cpu().numpy(), want) <= forward_bar(e32)
    assert rel_err(before.cpu().numpy(), want) > 10 * forward_bar(e32), "training must have moved the score"
    x = DiffusionSampler(model, sample_batch_size=4).sample(num_samples=4, num_diffusion_steps=5)
    assert x.shape == (4, c["L"], c["C"]) and bool(torch.isfinite(x).all())


# ---- errors and refusals ----------------------------------------------------------------------------------------------------
def test_argument_errors(lib):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = TR.TOY
    model, tr = fresh()
    X = dev(TR.toy_dataset(8, c["L"], c["C"]))
    t = torch.full((8,), 0.5, device="cuda")
    per = torch.empty(8, device="cuda", dtype=torch.float64)
    good = [tr.handle, X.data_ptr(), None, t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 0, 0, 0, per.data_ptr(), 8]
    cfg = N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1)
    for i in (1, 3, 4, 5, 10):  # null buffers
        bad = list(good)
        bad[i] = None
        assert lib.ffd_train_loss_grad(*bad, stream()) == -1
        assert lib.ffd_train_step(*bad, C.byref(cfg), stream()) == -1
    assert lib.ffd_train_loss_grad(*good[:-1], 0, stream()) == -1
    assert lib.ffd_train_step(*good, None, stream()) == -1
    assert lib.ffd_train_step(*good, C.byref(N.AdamWCfg(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0)), stream()) == -1
    assert lib.ffd_train_grad_sqnorm(tr.handle, None, stream()) == -1
    assert lib.ffd_train_adamw(tr.handle, None, C.byref(cfg), stream()) == -1  # clipping without a norm
    assert lib.ffd_train_bind(tr.handle, b"no.such.tensor", X.data_ptr(), X.data_ptr(), X.data_ptr(), X.data_ptr(), 4) == -1
    assert lib.ffd_train_bind(tr.handle, b"embedder.bias", X.data_ptr(), X.data_ptr(), X.data_ptr(), X.data_ptr(), 5) == -1
    assert lib.ffd_train_bind(tr.handle, b"embedder.bias", X.data_ptr(), None, X.data_ptr(), X.data_ptr(), c["d"]) == -1
    assert b"gradient" in lib.ffd_train_last_error(tr.handle)
    # an object with an unbound tensor refuses the batch (FFD_ERR_STATE) before any device work
    h = C.c_void_p()
    assert lib.ffd_train_create(C.byref(h), C.byref(model._desc()), 0.0, 0) == 0
    assert lib.ffd_train_loss_grad(h, *good[1:], stream()) == -3 and b"not bound" in lib.ffd_train_last_error(h)
    lib.ffd_train_destroy(h)
    assert tr.work_bytes(8) > 0 and tr.work_bytes(64) > tr.work_bytes(8)
    # the Python surface
    with pytest.raises(AssertionError):
        tr.step(X[:, :5].contiguous())
    with pytest.raises(N.FFDError):
        tr.step(X.cpu())
    loss = model.training_step(DiffusableBatch(X=X, timesteps=t), 0)
    assert loss.dim() == 0 and loss.device.type == "cuda" and all(
        p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)


def test_refusals_on_the_device(lib):
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    sch = TR.scheduler("vp", 12)
    X = dev(TR.toy_dataset(4, 12, 2))
    for m in (LSTMScoreModule(2, 12, sch, d_model=8, num_layers=1), MixtureScoreModule(2, 12, sch, means=X.cpu())):
        with pytest.raises(NotImplementedError):
            Trainer(m.cuda())
        with pytest.raises(NotImplementedError):
            m.cuda().training_step(DiffusableBatch(X=X, timesteps=torch.full((4,), 0.5).cuda()), 0)
    with pytest.raises(NotImplementedError):
        Trainer(TR.mlp_model(TR.TOY, "vp").cuda(), dropout=0.1)
