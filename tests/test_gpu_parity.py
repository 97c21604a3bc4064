"""GPU parity tests: the HIP path (through the fdiff-compatible Python surface, which
calls libffd's C ABI) against (a) the golden vectors produced by the unmodified
reference and (b) the CPU oracle on the same seeded inputs.

Tolerances (fp32):
  single operator  : max-abs error <= 2e-6 x output max-norm (FFT, SDE step: 5e-7)
  score evaluation : <= 1e-5 x output max-norm
  trajectories     : <= 1e-5 x max-norm at up to 1000 steps with injected noise
"""
import ctypes as C_
import math
import time

import numpy as np
import pytest
import torch

from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6
TOL_SCORE = 1e-5
TOL_TRAJ = 1e-5


@pytest.fixture(scope="module")
def ffd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):  # the in-tree build normally travels with the snapshot
        from fastfourierdiffusion_amd.build import build

        build()
    _native.lib()  # fail loudly if libffd.so cannot be loaded
    return pkg


def to_t(sd):
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


def make_sd(c):
    if c["kind"] == "lstm":
        return to_t(synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=c["wseed"]))
    return to_t(synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=c["wseed"]))


def make_model(ffd, c):
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if c["sde"] == "vp" else VEScheduler)(fourier_noise_scaling=c["fourier"], **c["sde_kwargs"])
    sch.set_noise_scaling(c["L"])
    if c["kind"] == "lstm":
        m = LSTMScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch,
                            fourier_noise_scaling=c["fourier"], d_model=c["d"], num_layers=c["NL"])
    else:
        m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, fourier_noise_scaling=c["fourier"],
                        d_model=c["d"], num_layers=c["NL"], n_head=c["H"])
    m.load_state_dict(make_sd(c), strict=True)
    return m.cuda().eval(), sch


def batch_of(x, tv):
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    t = torch.full((x.shape[0],), tv, dtype=torch.float32, device=x.device)
    return DiffusableBatch(X=x, y=None, timesteps=t)


# ---------------------------------------------------------------- FFT ------
@pytest.mark.parametrize("case", cases.FFT_CASES, ids=lambda c: f"L{c[0]}C{c[1]}")
def test_fft_golden(ffd, golden, case):
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    L, C, B, seed = case
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, seed))).cuda()
    g = golden["g1_fft"]
    assert rel_err(dft(x).cpu(), g[f"dft_L{L}_C{C}"]) < TOL_OP
    assert rel_err(idft(x).cpu(), g[f"idft_L{L}_C{C}"]) < TOL_OP


@pytest.mark.parametrize("L", [100, 101])
def test_fft_roundtrip_reference_invariant(ffd, L):
    # reference tests/test_utils.py:36-51, same sizes and tolerance
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    torch.manual_seed(0)
    x = torch.randn(100, L, 3, device="cuda")
    assert torch.allclose(x, idft(dft(x)), atol=1e-5)
    assert torch.allclose(x, dft(idft(x)), atol=1e-5)


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 2, 5), (5, 7, 2), (2, 64, 3), (4, 96, 1), (2, 127, 2), (3, 256, 9),
                                   (2, 360, 4), (1, 509, 3), (2, 1024, 2)])
def test_fft_vs_oracle_odd_sizes(ffd, shape):
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    x = torch.from_numpy(next(synthetic.noise_stream(shape, 1, 77)))
    assert rel_err(dft(x.cuda()).cpu(), O.dft(x)) < TOL_OP
    assert rel_err(idft(x.cuda()).cpu(), O.idft(x)) < TOL_OP


def test_fft_host_tensor_roundtrip_and_full_size(ffd):
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    x = torch.from_numpy(next(synthetic.noise_stream((512, 187, 1), 1, 5)))
    y = idft(dft(x))  # CPU tensors are staged through the GPU and come back on the CPU
    assert y.device.type == "cpu" and torch.allclose(x, y, atol=1e-5)
    # BASELINE configs[4] per-GPU shard shape, round trip + Parseval (ortho => energy preserved)
    xs = torch.randn(2048, 512, 8, device="cuda")
    X = dft(xs)
    assert torch.allclose(idft(X), xs, atol=2e-5)
    e_t = (xs.double() ** 2).sum((1, 2))
    w = torch.full((512,), 2.0, device="cuda", dtype=torch.float64)
    w[0] = 1.0
    w[256] = 1.0
    e_f = ((X.double() ** 2) * w.view(1, -1, 1)).sum((1, 2))
    assert torch.allclose(e_t, e_f, rtol=1e-5)


# ------------------------------------------------------------- FreSca ------
@pytest.mark.parametrize("case", cases.FRESCA_CASES, ids=lambda c: c[0])
def test_fresca_golden(ffd, golden, case):
    from fastfourierdiffusion_amd.utils.fresca import apply_fresca_to_score

    name, L, C, B, seed, lo, hi, ratio, strat, tstep, nsteps = case
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, seed))).cuda()
    y = apply_fresca_to_score(x, low_scale=lo, high_scale=hi, cutoff_ratio=ratio, cutoff_strategy=strat,
                              timestep=tstep, num_steps=nsteps)
    assert rel_err(y.cpu(), golden["g6_fresca"][name]) < TOL_OP
    if lo == 1.0 and hi == 1.0:
        assert y is x  # fresca.py:137-138 early exit returns the input itself


def test_fresca_full_batch_properties(ffd):
    """B=512 ECG batch: l = h = s is a pure scaling (linearity of rfft/irfft), and the energy
    cutoff is a batch statistic: permuting the samples permutes the output."""
    from fastfourierdiffusion_amd.utils.fresca import frequency_scale

    x = torch.randn(512, 187, 1, device="cuda")
    y = frequency_scale(x, low_scale=0.75, high_scale=0.75, cutoff_ratio=0.5, cutoff_strategy="energy")
    assert torch.allclose(y, 0.75 * x, atol=2e-6)
    perm = torch.randperm(512, device="cuda")
    a = frequency_scale(x, 1.0, 1.5, 0.5, "energy")
    b = frequency_scale(x[perm], 1.0, 1.5, 0.5, "energy")
    assert rel_err(b.cpu(), a[perm].cpu()) < 1e-6
    with pytest.raises(ValueError):
        frequency_scale(x, 1.0, 1.5, 0.5, "radial")


@pytest.mark.parametrize("case", cases.FRESCA2D_CASES, ids=lambda c: c[0])
def test_fresca2d_golden(ffd, golden, case):
    """frequency_scale on (batch, H, W, channels) (fresca.py:184-213): rfft2 -> radial mask on the bin indices -> irfft2."""
    from fastfourierdiffusion_amd.utils.fresca import frequency_scale

    name, H, W, C, B, seed, lo, hi, ratio, strat = case
    x = torch.from_numpy(next(synthetic.noise_stream((B, H * W, C), 1, seed))).reshape(B, H, W, C).cuda()
    y = frequency_scale(x, low_scale=lo, high_scale=hi, cutoff_ratio=ratio, cutoff_strategy=strat)
    assert rel_err(y.cpu(), golden["g14_fresca2d"][name]) < TOL_OP
    if lo == 1.0 and hi == 1.0:
        assert y is x


def test_fresca2d_properties_and_limits(ffd):
    """l = h = s is a pure scaling; against the oracle at shapes the goldens do not hold (odd H, W = 1, a single row);
    shapes past the kernel's LDS image are NotImplementedError, 5-D input the reference's ValueError (fresca.py:215)."""
    from fastfourierdiffusion_amd.utils.fresca import frequency_scale

    x = torch.randn(3, 20, 28, 2, device="cuda")
    y = frequency_scale(x, low_scale=0.6, high_scale=0.6, cutoff_ratio=0.5, cutoff_strategy="energy")
    assert torch.allclose(y, 0.6 * x, atol=2e-6)
    for shape in ((2, 7, 11, 3), (2, 5, 1, 2), (1, 1, 32, 1), (2, 256, 16, 1), (1, 13, 256, 1)):
        x = torch.randn(*shape)
        for strat, ratio in (("spatial", 0.4), ("energy", 0.55)):
            got = frequency_scale(x.cuda(), 0.9, 1.4, ratio, strat)
            assert rel_err(got.cpu(), O.fresca2d(x, 0.9, 1.4, ratio, strat)) < TOL_OP, (shape, strat)
    with pytest.raises(NotImplementedError):
        frequency_scale(torch.randn(1, 128, 64, 1, device="cuda"), 1.0, 1.5)
    with pytest.raises(NotImplementedError):
        frequency_scale(torch.randn(1, 2, 300, 1, device="cuda"), 1.0, 1.5)
    with pytest.raises(ValueError):
        frequency_scale(torch.randn(1, 2, 3, 4, 5, device="cuda"), 1.0, 1.5)


# ---------------------------------------------------------------- SDE ------
@pytest.mark.parametrize("c", cases.STEP_CASES, ids=lambda c: c["name"])
def test_step_golden(ffd, golden, c):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    g = golden["g3_steps"]
    B, L, C = c["B"], c["L"], c["C"]
    sch = (VPScheduler if c["sde"] == "vp" else VEScheduler)(fourier_noise_scaling=c["fourier"], **c["sde_kwargs"])
    sch.set_noise_scaling(L)
    sch.set_timesteps(c["N"])
    sch.timesteps = torch.from_numpy(golden["g2_tables"][f"ts_N{c['N']}"].copy())  # the grid the golden was made on
    sch.step_size = sch.timesteps[0] - sch.timesteps[1]
    x, s, z = (torch.from_numpy(a).cuda() for a in synthetic.noise_stream((B, L, C), 3, c["seed"]))
    for i in c["idx"]:
        out = sch.step(model_output=s, timestep=sch.timesteps[i].item(), sample=x, noise=z).prev_sample
        assert rel_err(out.cpu(), g[f"{c['name']}_i{i}"]) < 5e-7
    # prior with the same injected draw
    import ctypes as Ct
    from fastfourierdiffusion_amd import _native as N
    xp = torch.empty_like(z)
    desc = sch._desc()
    N.check(N.lib().ffd_prior(Ct.byref(desc), xp.data_ptr(), z.data_ptr(), sch._G_on(z.device).data_ptr(), 0, 0, B, L,
                              C, N.current_stream_ptr(z.device)))
    assert rel_err(xp.cpu(), g[f"{c['name']}_prior"]) < 5e-7


def test_philox_noise_statistics_and_shard_invariance(ffd):
    """On-device draws: N(0,1) moments, and identical values however the batch is sharded."""
    import ctypes as Ct
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    L, C, B = 187, 1, 1024
    sch = VPScheduler(fourier_noise_scaling=False)
    sch.set_noise_scaling(L)
    desc = sch._desc()
    G = sch._G_on(torch.device("cuda", 0))
    full = torch.empty(B, L, C, device="cuda")
    N.check(N.lib().ffd_prior(Ct.byref(desc), full.data_ptr(), None, G.data_ptr(), 1234, 0, B, L, C, None))
    v = full.double()
    assert abs(float(v.mean())) < 0.01 and abs(float(v.var()) - 1.0) < 0.01
    assert abs(float((v ** 4).mean()) - 3.0) < 0.1  # kurtosis of a Gaussian
    # shard into 3 uneven pieces with the matching sample offsets -> bit-identical
    parts, off = [], 0
    for b in (1, 340, 683):
        p = torch.empty(b, L, C, device="cuda")
        N.check(N.lib().ffd_prior(Ct.byref(desc), p.data_ptr(), None, G.data_ptr(), 1234, off, b, L, C, None))
        parts.append(p)
        off += b
    assert torch.equal(torch.cat(parts), full)
    # a different seed or step gives a different stream
    other = torch.empty_like(full)
    N.check(N.lib().ffd_prior(Ct.byref(desc), other.data_ptr(), None, G.data_ptr(), 1235, 0, B, L, C, None))
    assert not torch.equal(other, full)


# ------------------------------------------------------------ encoders -----
def test_encoders_reference_tests(ffd, golden):
    """reference tests/test_transformer.py:18-82 (same sizes, EPS = 1e-5) on the device
    modules, plus the golden time-embedding known answers."""
    from fastfourierdiffusion_amd.models.transformer import GaussianFourierProjection, PositionalEncoding

    max_len, batch_size, d_model, EPS = 20, 16, 5, 1e-5
    torch.manual_seed(42)
    pos = PositionalEncoding(d_model=d_model, max_len=max_len).cuda()
    X = torch.randn((batch_size, max_len, d_model), device="cuda")
    enc = pos(X)
    assert enc.shape == X.shape
    assert torch.max(torch.sum((enc - X) ** 2, dim=-1)) <= d_model + EPS  # max_norm constraint
    assert torch.allclose((enc - X)[3], pos.embedding.weight[:max_len], atol=EPS)
    te = GaussianFourierProjection(d_model=d_model).cuda()
    ts = torch.randint(low=0, high=max_len, size=(batch_size,), device="cuda").float()
    out = te(X, ts)
    proj = ts[:, None].cpu() * te.W[None, :].cpu() * 2 * np.pi
    emb = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)[:, :d_model]
    gt = torch.nn.functional.linear(emb, te.dense.weight.cpu(), te.dense.bias.cpu())
    assert torch.allclose((out - X).cpu(), gt[:, None, :].expand(-1, max_len, -1), atol=EPS * 10)
    # golden known answer (default ECG model weights)
    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    for tv in c["t_values"]:
        t = torch.full((c["B"],), tv, device="cuda")
        got = m.time_encoder(torch.zeros(c["B"], 1, c["d"], device="cuda"), t)[:, 0, :]
        np.testing.assert_allclose(got.cpu().numpy(), golden["g5_models"][f"ecg_temb_t{tv}"], rtol=0, atol=1e-5)
    pe = m.pos_encoder(torch.zeros(1, c["L"], c["d"], device="cuda"))
    for _ in range(3):
        pe = m.pos_encoder(torch.zeros(1, c["L"], c["d"], device="cuda"))
    np.testing.assert_allclose(pe[0].cpu().numpy(), golden["g5_models"]["ecg_pos_fixed"], rtol=0, atol=1e-6)


# -------------------------------------------------------------- models -----
@pytest.fixture(autouse=True)
def _tune_defaults():
    """ffd_tune is process-wide state: every test starts from, and leaves behind, the defaults."""
    yield
    if torch.cuda.is_available():
        from fastfourierdiffusion_amd import _native as N

        assert N.lib().ffd_tune(b"reset", 0) == 0


@pytest.fixture(params=["auto", "large", "rows", "rows_unfused", "unfused", "split"])
def variant(request, ffd):
    """Kernel variants that must all meet the same parity bar: default heuristics (at these small batches: the
    q-/key-split fused attention kernel and the F-split out-proj + FFN pair), "large" (the kernels the heuristics pick
    at large batches, forced: one workgroup per head (pair), k_linear_res_ln + k_ffn_ln), "rows" (the same with the
    large-batch FFN of d_model 72 forced at every size: k_ffn_rows, row-owning waves under the LDS weight ring, with the
    out-projection + LN1 inside it; "rows_unfused": with k_linear_res_ln in front of it instead) and the two-kernel
    projection / attention fallback ("unfused"); and "split": the opt-in FFN on the bf16 matrix cores as a three-part,
    six-term split (fp32-equivalent, csrc/ffd_ffn_split.hip), which has to pass the same goldens at the same tolerance."""
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    if request.param == "split":
        assert lib.ffd_tune(b"ffn_split", 1) == 0
    if request.param == "unfused":
        assert lib.ffd_tune(b"attn_fused", 0) == 0
    if request.param in ("large", "rows", "rows_unfused"):
        assert lib.ffd_tune(b"attn_small", 0) == 0
        assert lib.ffd_tune(b"small_path", 0) == 0
    if request.param in ("rows", "rows_unfused"):
        assert lib.ffd_tune(b"mid_path", 0) == 0 and lib.ffd_tune(b"ffn_rows", 2) == 0
    if request.param == "rows_unfused":
        assert lib.ffd_tune(b"ffn_rows_fuse", 0) == 0
    yield request.param
    lib.ffd_tune(b"reset", 0)


@pytest.mark.parametrize("c", cases.MODEL_CASES, ids=lambda c: c["name"])
def test_model_golden(ffd, golden, c, variant):
    g = golden["g5_models"]
    m, sch = make_model(ffd, c)
    B, L, C = c["B"], c["L"], c["C"]
    name = c["name"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"]))).cuda()
    for tv in c["t_values"]:
        sc = m(batch_of(x, tv))
        assert rel_err(sc.cpu(), g[f"{name}_score_t{tv}"]) < TOL_SCORE, (name, tv)
    if c.get("cache_seq"):
        m.enable_caching(**c.get("cache_kwargs", {}))
        m.cache.reset()
        tv = c["t_values"][0]
        for j, rec in enumerate(c["cache_seq"]):
            xj = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"] + 100 + j))).cuda()
            sc, crf = m(batch_of(xj, tv), recompute_tokens=set(rec), step=j, return_crf=True)
            assert rel_err(sc.cpu(), g[f"{name}_cseq{j}_score"]) < TOL_SCORE, (name, j)
            k, v = m.cache_tables()
            if c.get("dump_table"):
                assert rel_err(k.cpu(), g[f"{name}_cseq{j}_k"]) < TOL_SCORE
                assert rel_err(v.cpu(), g[f"{name}_cseq{j}_v"]) < TOL_SCORE
                assert rel_err(crf.cpu(), g[f"{name}_cseq{j}_crf"]) < TOL_SCORE
            else:
                assert rel_err(k[0, 0].cpu(), g[f"{name}_cseq{j}_k_l0h0"]) < TOL_SCORE
                assert rel_err(v[-1, -1].cpu(), g[f"{name}_cseq{j}_v_lNhN"]) < TOL_SCORE
        st = m.cache.get_cache_stats()
        np.testing.assert_array_equal([st["recompute_count"], st["cache_hit_count"]], g[f"{name}_cstats"])
        m.disable_caching()


def test_model_vs_oracle_ragged_batches(ffd):
    """Batch sizes that do not fill the 16/64/128-row MFMA tiles (B*L % 16 != 0), B=1."""
    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    for B in (1, 3, 7, 70):
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 900 + B)))
        t = torch.full((B,), 0.4, dtype=torch.float32)
        ref = O.score_forward(x, t, sd, c["NL"], c["H"])
        out = m(batch_of(x.cuda(), 0.4))
        assert rel_err(out.cpu(), ref) < TOL_SCORE, B


def test_cached_modes_vs_oracle_batch_across_xcds(ffd, variant):
    """FULL -> PURE -> MIXED -> PURE -> STD-like (n > 0.8 L) with B=19: the fused kernel places samples 0..15 by
    its XCD-aware block remap and 16..18 directly; every sample must see batch element 0's tables (Q1)."""
    c = next(c for c in cases.MODEL_CASES if c["name"] == "reftest")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    B, L, C = 19, c["L"], c["C"]
    m.enable_caching()
    m.cache.reset()
    table = O.KVTable(c["NL"], L)
    for j, n in enumerate([L, 0, 10, 0, L - 3]):
        x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 7000 + j)))
        t = torch.full((B,), 0.55, dtype=torch.float32)
        ref = O.score_forward(x, t, sd, c["NL"], c["H"], table, list(range(n)))
        out = m(batch_of(x.cuda(), 0.55), recompute_tokens=set(range(n)), step=j)
        assert rel_err(out.cpu(), ref) < TOL_SCORE, (j, n)
    m.disable_caching()


@pytest.mark.parametrize("scale", [1.0, 6.0, 40.0])
def test_attention_large_logits_vs_oracle(ffd, scale, variant):
    """Softmax logits far from zero (q/k projection rows scaled up): the fused kernel keeps its max reference at 0
    while |logit| <= 64 (log2 units) and refreshes it beyond -- first-tile and later-tile refreshes, rows whose
    maximum sits in the last key tile -- all must agree with the oracle's exact softmax."""
    c = dict(next(c for c in cases.MODEL_CASES if c["name"] == "ecg"))
    c["NL"] = 2
    sd = make_sd(c)
    d = c["d"]
    for i in range(c["NL"]):
        w = sd[f"backbone.layers.{i}.self_attn.in_proj_weight"]
        bq = sd[f"backbone.layers.{i}.self_attn.in_proj_bias"]
        w[: 2 * d] *= scale
        bq[: 2 * d] *= scale
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    sch = VPScheduler(fourier_noise_scaling=True, **cases.VP)
    sch.set_noise_scaling(c["L"])
    m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=d, num_layers=c["NL"], n_head=c["H"])
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    B = 9
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 8100)))
    t = torch.full((B,), 0.3, dtype=torch.float32)
    ref = O.score_forward(x, t, sd, c["NL"], c["H"])
    out = m(batch_of(x.cuda(), 0.3)).cpu()
    assert torch.isfinite(out).all()
    # logits of magnitude ~1e3 are themselves only known to ~1e-4 in fp32 (every kernel variant and the oracle's
    # own fp32 evaluation differ by ~1.5e-4 there): the check at scale 40 is for finiteness / no lost rows
    assert rel_err(out, ref) < (TOL_SCORE if scale < 10 else 1e-3), scale


# every (d_model, head_dim) pair with kernels in this build, at lengths that exercise 1..many key tiles, odd / even L
_SHAPES = [(72, 12, 187), (60, 12, 50), (48, 12, 33), (64, 8, 100), (32, 4, 64), (16, 4, 20), (24, 8, 45), (24, 4, 20),
           (8, 4, 31), (72, 12, 300), (48, 12, 192), (60, 12, 193), (64, 8, 512), (72, 12, 512), (24, 8, 500)]


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: f"d{s[0]}h{s[1]}L{s[2]}")
def test_supported_shapes_vs_oracle(ffd, shape, variant):
    """No-cache and cached (FULL -> PURE -> MIXED) evaluations against the oracle for every supported head shape."""
    # every variant: "auto" = small-batch kernels, "large" = the large-batch ones, "split" = the bf16x3 FFN, at every
    # (d_model, head_dim) with an instance
    d, H, L = shape
    C, NL, B = 2, 2, 3
    c = dict(kind="transformer", d=d, H=H, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=600 + d + L)
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 9000 + d)))
    t = torch.full((B,), 0.7, dtype=torch.float32)
    out = m(batch_of(x.cuda(), 0.7)).cpu()
    assert rel_err(out, O.score_forward(x, t, sd, NL, H)) < TOL_SCORE
    m.enable_caching()
    m.cache.reset()
    table = O.KVTable(NL, L)
    for j, n in enumerate([L, 0, min(10, L), 0]):
        xj = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 9100 + d + j)))
        ref = O.score_forward(xj, t, sd, NL, H, table, list(range(n)))
        got = m(batch_of(xj.cuda(), 0.7), recompute_tokens=set(range(n)), step=j)
        assert rel_err(got.cpu(), ref) < TOL_SCORE, (j, n)
    m.disable_caching()


def test_forced_q_tile_groups_and_remainder_instances_vs_oracle(ffd):
    """The instances that only ffd_tune "attn_qg" and "ffn_rem" reach.  d_model 72 (two remainder groups in GEMM2) at
    L = 70: three q-tiles, so the heuristics take QG = 3; attn_hpw = 1 keeps the two-heads form (which ignores the knob
    at L <= 192) out of the way.  k_ffn_ln at 48- and 64-row tiles runs with the remainder rows on the 4x4x1 MFMA and
    without."""
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    d, H, L, C, NL, B = 72, 12, 70, 2, 2, 3
    c = dict(kind="transformer", d=d, H=H, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=600 + d + L)
    m, _ = make_model(ffd, c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 9000 + d)))
    ref = O.score_forward(x, torch.full((B,), 0.7, dtype=torch.float32), make_sd(c), NL, H)
    fused = [dict(attn_small=0, attn_hpw=1, attn_qg=qg) for qg in (1, 2)]
    two_kernel = [dict(attn_fused=0, attn_qg=qg) for qg in (1, 2, 3)]
    ffn = [dict(ffn_rows=0, small_path=0, mid_path=0, ffn_height=0, ffn_mb=mb, ffn_rem=rem) for mb in (3, 4) for rem in (0, 1)]
    for knobs in fused + two_kernel + ffn:
        for key, v in knobs.items():
            assert lib.ffd_tune(key.encode(), v) == 0, (key, v)
        out = m(batch_of(x.cuda(), 0.7)).cpu()
        assert lib.ffd_tune(b"reset", 0) == 0
        assert rel_err(out, ref) < TOL_SCORE, knobs


def test_model_full_batch_properties(ffd):
    """BASELINE configs[1] batch (B=512): sample independence (a size-independent
    property of the path) -- every sample of a big batch equals its own B=1 evaluation
    -- plus agreement of a slice with the oracle."""
    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    B = 512
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4242)))
    out = m(batch_of(x.cuda(), 0.6)).cpu()
    assert torch.isfinite(out).all()
    for b in (0, 1, 255, 511):
        one = m(batch_of(x[b:b + 1].cuda(), 0.6)).cpu()
        assert rel_err(out[b:b + 1], one) < 2e-6, b  # tile shape differs (MB=8 vs MB=1) -> same math, other order
    t = torch.full((4,), 0.6, dtype=torch.float32)
    ref = O.score_forward(x[100:104], t, sd, c["NL"], c["H"])
    assert rel_err(out[100:104], ref) < TOL_SCORE


@pytest.mark.parametrize("d,H", [(60, 12), (64, 8), (48, 12)])
def test_rows_kernel_other_d_models_at_size(ffd, d, H):
    """Round 4: k_ffn_rows (row-owning waves under the LDS weight ring, out-projection + LN1 inside) instantiated for
    d_model 60 -- the reference's class default, score_models.py:31 -- 64 and 48.  At the ECG length and B = 512 (the
    production selection there: large M): sample independence, a slice against the oracle, and the same bits for every
    waves-per-workgroup choice, the sliced form to rounding, the F-split kernel it replaces (k_ffn_ln) to rounding."""
    from fastfourierdiffusion_amd import _native as N

    L, C, NL, B = 187, 1, 3, 512
    c = dict(kind="transformer", d=d, H=H, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=700 + d)
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 4400 + d)))
    fl, by = C_.c_double(), C_.c_double()
    name = lib.ffd_kernel_work(m._ctx().handle, N.K_FFN, B, 0, C_.byref(fl), C_.byref(by)).decode()
    assert name.startswith("k_ffn_rows<oproj"), name  # the production selection at this size
    out = m(batch_of(x.cuda(), 0.6))
    assert torch.isfinite(out).all()
    t = torch.full((3,), 0.6, dtype=torch.float32)
    assert rel_err(out[200:203].cpu(), O.score_forward(x[200:203], t, sd, NL, H)) < TOL_SCORE
    for b in (0, 511):
        one = m(batch_of(x[b:b + 1].cuda(), 0.6)).cpu()  # (small-batch kernels: other summation order)
        assert rel_err(out[b:b + 1].cpu(), one) < 2e-6, b
    for nw in (4, 8, 12):
        for fuse in (1, 0):
            assert lib.ffd_tune(b"ffn_rows_nw", nw) == 0 and lib.ffd_tune(b"ffn_rows_fuse", fuse) == 0
            o2 = m(batch_of(x.cuda(), 0.6))
            if fuse:
                assert torch.equal(o2, out), (nw, fuse)
            else:
                assert rel_err(o2.cpu(), out.cpu()) < 2e-6, (nw, fuse)
    assert lib.ffd_tune(b"reset", 0) == 0
    assert lib.ffd_tune(b"rows_slices", 3) == 0 and lib.ffd_tune(b"ffn_rows_nw", 12) == 0
    assert rel_err(m(batch_of(x[:100].contiguous().cuda(), 0.6)).cpu(), out[:100].cpu()) < 2e-6
    assert lib.ffd_tune(b"reset", 0) == 0 and lib.ffd_tune(b"ffn_rows", 0) == 0
    assert rel_err(m(batch_of(x.cuda(), 0.6)).cpu(), out.cpu()) < 2e-6


def test_lstm_full_batch_properties(ffd):
    """BASELINE configs[3] shape at B=128 (32 128 rows: the LDS-staged row-major gate GEMM and two recurrence
    workgroups per CU are in play): sample independence + agreement of a slice with the oracle."""
    c = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    B = 128
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4343)))
    out = m(batch_of(x.cuda(), 0.45)).cpu()
    assert torch.isfinite(out).all()
    for b in (0, 63, 127):
        one = m(batch_of(x[b:b + 1].cuda(), 0.45)).cpu()
        assert rel_err(out[b:b + 1], one) < 2e-6, b
    t = torch.full((2,), 0.45, dtype=torch.float32)
    ref = O.lstm_score_forward(x[40:42], t, sd, c["NL"])
    assert rel_err(out[40:42], ref) < TOL_SCORE


def test_lstm_production_batch_selection(ffd):
    """BASELINE configs[3] shape at the batches the production selection (no ffd_tune here) hands to its two large-batch
    form, the layer wavefront (k_lstm_wave: a 16-sample tile per CU, larger batches in sub-batches of 4096): B = 2048 and
    B = 4352.  Sample independence against small-batch evaluations for three picks, a
    two-sample slice against the oracle, and the kernel class bench.py would report."""
    import ctypes as C

    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    for B, kname in ((2048, b"k_lstm_wave"), (4352, b"k_lstm_wave")):
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4444 + B)))
        out = m(batch_of(x.cuda(), 0.45)).cpu()
        assert torch.isfinite(out).all()
        ctx = m._ctx()
        fl, by = C.c_double(), C.c_double()
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_LSTM_REC, B, 0, C.byref(fl), C.byref(by)) == kname
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_LSTM_REC, 512, 0, C.byref(fl), C.byref(by)) == b"k_lstm_wave"
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_LSTM_REC, 8192, 0, C.byref(fl), C.byref(by)) == b"k_lstm_wave"
        assert fl.value == c["NL"] * 2.0 * 4096 * c["L"] * 8.0 * c["d"] ** 2  # per launch: a sub-batch of 4096
        for b in (0, B // 2 - 1, B - 1):
            one = m(batch_of(x[b:b + 1].cuda(), 0.45)).cpu()
            assert rel_err(out[b:b + 1], one) < 2e-6, (B, b)
        t = torch.full((2,), 0.45, dtype=torch.float32)
        ref = O.lstm_score_forward(x[1500:1502], t, sd, c["NL"])
        assert rel_err(out[1500:1502], ref) < TOL_SCORE, B


@pytest.mark.parametrize("name", ["ecg", "nasa_lstm"])
def test_checkpoint_to_device_to_forward_golden(ffd, golden, tmp_path, name):
    """cmd/sample.py:68-77 / cmd/benchmark_cache.py:141-150: load_from_checkpoint(...) -> .cuda() -> forward.  The
    golden case's state_dict is written as a Lightning-style file (hyper_parameters with the pickled scheduler object +
    state_dict + the cached_backbone.* copies enable_caching leaves in a trained checkpoint), read back with
    weights_only=True, moved to the device and evaluated against the reference's scores for that state_dict (g5).
    (No real trained checkpoint exists in the reference tree: the file is synthesised, the expected output is the
    unmodified reference's.)"""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    c = next(c for c in cases.MODEL_CASES if c["name"] == name)
    assert c["sde"] == "vp"
    sch = VPScheduler(fourier_noise_scaling=c["fourier"], **c["sde_kwargs"])
    sd = dict(make_sd(c))
    hp = dict(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, fourier_noise_scaling=c["fourier"],
              d_model=c["d"], num_layers=c["NL"], num_training_steps=1000, lr_max=1e-3, likelihood_weighting=False)
    cls = LSTMScoreModule
    if c["kind"] != "lstm":
        cls = ScoreModule
        hp["n_head"] = c["H"]
        sd["cached_backbone.0.linear1.weight"] = torch.zeros(3)
    path = tmp_path / "epoch=7-val_loss=0.12.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "pytorch-lightning_version": "2.1.0", "epoch": 7}, path)
    m = cls.load_from_checkpoint(checkpoint_path=str(path), weights_only=False)  # (always read with weights_only=True)
    m.noise_scheduler.set_noise_scaling(c["L"])
    m = m.cuda().eval()
    g = golden["g5_models"]
    x = torch.from_numpy(next(synthetic.noise_stream((c["B"], c["L"], c["C"]), 1, c["xseed"]))).cuda()
    for tv in c["t_values"]:
        assert rel_err(m(batch_of(x, tv)).cpu(), g[f"{name}_score_t{tv}"]) < TOL_SCORE, (name, tv)


def test_errors_are_loud(ffd):
    from fastfourierdiffusion_amd._native import FFDError
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    c = next(c for c in cases.MODEL_CASES if c["name"] == "small")
    m, _ = make_model(ffd, c)
    with pytest.raises(AssertionError):  # wrong shape (score_models.py:87-90)
        m(batch_of(torch.zeros(2, c["L"] + 1, c["C"], device="cuda"), 0.5))
    with pytest.raises(FFDError):  # CPU tensor: no fallback
        m(batch_of(torch.zeros(2, c["L"], c["C"]), 0.5))
    bad = ScoreModule(n_channels=1, max_len=16, noise_scheduler=VPScheduler(), d_model=36, n_head=12).cuda()
    with pytest.raises(NotImplementedError):  # d_model without a kernel
        bad(batch_of(torch.zeros(1, 16, 1, device="cuda"), 0.5))


# --------------------------------------------------------- trajectories ----
@pytest.mark.parametrize("c", cases.TRAJ_CASES, ids=lambda c: c["name"])
def test_traj_golden(ffd, golden, c, variant):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    if variant not in ("auto", "split") and c["N"] >= 1000 and c["use_cache"]:
        pytest.skip("1000-step cached trajectory is run with the default kernels and the split FFN only (suite time)")

    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    nb = max(1, c["num_samples"] // B)
    fk = c.get("fresca")
    fres = {} if fk is None else dict(use_fresca=True, fresca_low_scale=fk["low_scale"],
                                      fresca_high_scale=fk["high_scale"], fresca_cutoff_ratio=fk["cutoff_ratio"],
                                      fresca_cutoff_strategy=fk["cutoff_strategy"])
    sampler = DiffusionSampler(score_model=m, sample_batch_size=B, use_cache=c["use_cache"],
                               cache_kwargs=dict(c.get("cache_kwargs", {})), z_chunk_steps=64, **fres)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), nb * (N + 1), c["zseed"]))
    # the golden trajectory was generated on the timestep grid stored in g2_tables; torch.linspace
    # on this host may differ from it in the last ulp (vector width), so pin the grid.
    ts_golden = torch.from_numpy(golden["g2_tables"][f"ts_N{N}"].copy())
    orig = sch.set_timesteps

    def pinned(n):
        orig(n)
        assert n == N
        sch.timesteps = ts_golden
        sch.step_size = ts_golden[0] - ts_golden[1]

    sch.set_timesteps = pinned
    out = sampler.sample(num_samples=c["num_samples"], num_diffusion_steps=N)
    ref = golden["g7_traj"][c["name"]]
    assert out.device.type == "cpu" and tuple(out.shape) == ref.shape
    err = rel_err(out, ref)
    assert err < TOL_TRAJ, err


def test_reference_unit_test_sizes(ffd):
    """reference tests/test_score_models.py:13-89 and tests/test_schedulers.py:14-18,123-135: the
    d_model=8 / n_head=4 / num_layers=2 models produce (batch, max_len, n_channels) scores and
    (num_samples, max_len, n_channels) samples."""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    for sch in (VPScheduler(), VEScheduler()):
        for cls, kw in ((ScoreModule, dict(n_head=4)), (LSTMScoreModule, {})):
            model = cls(n_channels=3, max_len=20, noise_scheduler=sch, d_model=8, num_layers=2,
                        num_training_steps=10, **kw).cuda()
            sch.set_noise_scaling(20)
            X = torch.randn(5, 20, 3, device="cuda")
            score = model(batch_of(X, 0.5))
            assert score.shape == X.shape and torch.isfinite(score).all()
            samples = DiffusionSampler(score_model=model, sample_batch_size=12).sample(48, 10)
            assert samples.shape == (48, 20, 3) and torch.isfinite(samples).all()


def test_sampler_api_shapes_reference_test(ffd):
    """reference tests/test_sampling.py:21-40: default ScoreModule (d=60, H=12, NL=3),
    sample(48, 10) with batch 12 -> (48, 50, 3), VP and VE, torch-seeded RNG."""
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    for sch in (VPScheduler(), VEScheduler()):
        torch.manual_seed(0)
        model = ScoreModule(n_channels=3, max_len=50, noise_scheduler=sch).cuda()
        sch.set_noise_scaling(max_len=50)
        sampler = DiffusionSampler(score_model=model, sample_batch_size=12)
        samples = sampler.sample(num_samples=48, num_diffusion_steps=10)
        assert samples.shape == (48, 50, 3) and samples.device.type == "cpu"
        assert torch.isfinite(samples).all()
        # same torch seeds -> same samples (drop-in determinism); philox path: shard-invariant
        torch.manual_seed(7)
        a = DiffusionSampler(model, 12).sample(24, 5)
        torch.manual_seed(7)
        b = DiffusionSampler(model, 12).sample(24, 5)
        assert torch.equal(a, b)
        p_full = DiffusionSampler(model, 24, rng="philox", seed=3).sample(24, 5)
        p_half = torch.cat([DiffusionSampler(model, 12, rng="philox", seed=3, sample_offset=o).sample(12, 5)
                            for o in (0, 12)])
        assert rel_err(p_half, p_full) < 2e-6


def test_cache_on_off_and_stats_q5(ffd):
    """cmd/benchmark_cache.py path: cache on vs off differ only through the K/V tables;
    second enable_caching leaves the sampler-visible stats at zero (quirk Q5)."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = next(c for c in cases.TRAJ_CASES if c["name"] == "traj_small_vp_cache")
    m, sch = make_model(ffd, c)
    s1 = DiffusionSampler(m, 2, use_cache=True, cache_kwargs={})
    first = m.cache
    s1.inject_noise(synthetic.noise_stream((2, c["L"], c["C"]), 9, 1))
    s1.sample(2, 8)
    st = first.get_cache_stats()
    assert st["recompute_count"] == c["L"] * c["NL"] and st["cache_hit_count"] == 7 * c["L"] * c["NL"]
    assert st["cache_ratio"] == 0.99
    s2 = DiffusionSampler(m, 2, use_cache=True, cache_kwargs={})
    assert m.cache is not first
    s2.inject_noise(synthetic.noise_stream((2, c["L"], c["C"]), 9, 1))
    s2.sample(2, 8)
    assert m.cache.get_cache_stats()["cache_hit_count"] == 0  # Q5: layers still feed the first cache
    with pytest.raises(TypeError):  # README's random_probe_ratio is not a kwarg (Q6)
        DiffusionSampler(m, 2, use_cache=True, cache_kwargs={"random_probe_ratio": 0.1})


# ------------------------------------------ FreqCa helpers (scope row (f)2/(f)3) ----
TOL_HERMITE = 2e-3  # the reference inverts ridge-regularised normal equations in fp32: conditioning-limited


@pytest.mark.parametrize("case", cases.DECOMP_CASES, ids=lambda c: c[0])
def test_freq_decompose_golden(ffd, golden, case):
    from fastfourierdiffusion_amd.utils.fourier import frequency_decompose_dct, frequency_decompose_fft

    name, B, L, D, seed, ratio = case
    shape = (L, D) if B == 0 else (B, L, D)
    x = torch.from_numpy(next(synthetic.noise_stream(shape, 1, seed))).cuda()
    lo, hi = frequency_decompose_fft(x, ratio)
    g = golden["g10_freqca"]
    assert tuple(lo.shape) == g[f"decomp_{name}_low"].shape and lo.is_cuda
    assert rel_err(lo.cpu(), g[f"decomp_{name}_low"]) < TOL_OP
    assert rel_err(hi.cpu(), g[f"decomp_{name}_high"]) < TOL_OP
    lo2, hi2 = frequency_decompose_dct(x, ratio)  # fourier.py:303: the dct entry returns the fft result
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)


@pytest.mark.parametrize("case", cases.HERMITE_CASES, ids=lambda c: c[0])
def test_hermite_golden(ffd, golden, case):
    from fastfourierdiffusion_amd.utils.fourier import predict_hermite

    name, K, shape, order, ts, target, seed = case
    hist = [torch.from_numpy(a).cuda() for a in synthetic.noise_stream(shape, K, seed)]
    y = predict_hermite(hist, list(ts), target, order)
    assert rel_err(y.cpu(), golden["g10_freqca"][f"hermite_{name}"]) < TOL_HERMITE


@pytest.mark.parametrize("case", cases.DENSITY_CASES, ids=lambda c: f"L{c[0]}C{c[1]}")
def test_spectral_density_golden(ffd, golden, case):
    from fastfourierdiffusion_amd.utils.fourier import spectral_density

    L, C, B, seed, apply = case
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, seed))).cuda()
    y = spectral_density(x, apply_dft=apply)
    assert rel_err(y.cpu(), golden["g10_freqca"][f"density_L{L}_C{C}_{int(apply)}"]) < 2 * TOL_OP


@pytest.mark.parametrize("c", cases.FREQCA_TRAJ_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("chunk", [7, 1000])
def test_freqca_state_golden(ffd, golden, c, chunk):
    """E2CRFCache(use_freqca=True) state after DiffusionSampler.sample: CRF slot, low part, high history,
    timestep history, stats and predict_crf_freqca -- with the loop run in 7-step chunks and in one call."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    nb = max(1, c["num_samples"] // B)
    g, name = golden["g10_freqca"], c["name"]
    sampler = DiffusionSampler(score_model=m, sample_batch_size=B, use_cache=True, cache_kwargs=dict(c["cache_kwargs"]),
                               z_chunk_steps=chunk)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), nb * (N + 1), c["zseed"]))
    ts_golden = torch.from_numpy(g[f"{name}_ts"].copy())
    orig = sch.set_timesteps

    def pinned(n):
        orig(n)
        sch.timesteps = ts_golden
        sch.step_size = ts_golden[0] - ts_golden[1]

    sch.set_timesteps = pinned
    out = sampler.sample(num_samples=c["num_samples"], num_diffusion_steps=N)
    cache = m.cache
    assert rel_err(out, g[f"{name}_out"]) < TOL_TRAJ
    assert rel_err(cache.crf_cache.cpu(), g[f"{name}_crf_cache"]) < TOL_TRAJ
    st = cache.get_cache_stats()
    if cache.use_freqca:
        assert rel_err(cache.crf_low_cache.cpu(), g[f"{name}_low"]) < TOL_TRAJ
        hist = torch.stack([h.cpu() for h in cache.crf_high_history], 0)
        assert tuple(hist.shape) == g[f"{name}_high_hist"].shape
        assert rel_err(hist, g[f"{name}_high_hist"]) < TOL_TRAJ
        np.testing.assert_array_equal(np.array(cache.crf_timestep_history, dtype=np.float64), g[f"{name}_t_hist"])
        assert [st["freq_decomp_count"], st["freq_decomp_skipped"], st["current_step"]] == g[f"{name}_stats"].tolist()
        pred = cache.predict_crf_freqca(c["t_pred"])
        assert rel_err(pred.cpu(), g[f"{name}_pred"]) < TOL_HERMITE
    else:
        assert "freq_decomp_count" not in st and cache.predict_crf_freqca(0.5) is None


# ------------------------------------------ MLPScoreModule (scope row (f)3) ----
def make_mlp(c):
    from fastfourierdiffusion_amd.models.score_models import MLPScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    sch = VPScheduler(fourier_noise_scaling=True, **cases.VP)
    sch.set_noise_scaling(c["L"])
    m = MLPScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], d_mlp=c["d_mlp"],
                       num_layers=c["NL"])
    sd = to_t(synthetic.mlp_state_dict(c["C"], c["L"], c["d"], c["d_mlp"], c["NL"], seed=c["wseed"]))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sch, sd


@pytest.mark.parametrize("c", cases.MLP_CASES, ids=lambda c: c["name"])
def test_mlp_vs_oracle(ffd, c):
    """Parity UNPINNED against the reference (torchvision.ops.MLP is absent from this image): the HIP path is
    compared with the oracle restatement of MLPScoreModule.forward (score_models.py:406-440)."""
    m, sch, sd = make_mlp(c)
    B, L, C = c["B"], c["L"], c["C"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"])))
    for tv in (1.0, 0.37):
        y = m(batch_of(x.cuda(), tv))
        assert tuple(y.shape) == (B, L, C)  # tests/test_score_models.py:58-61
        ref = O.mlp_score_forward(x, torch.full((B,), tv), sd, c["NL"])
        assert rel_err(y.cpu(), ref) < TOL_SCORE
    with pytest.raises(AttributeError):
        m.enable_caching()  # Q9: the reference dereferences backbone.layers, which a ModuleList lacks


def test_mlp_trajectory_vs_oracle(ffd):
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = cases.MLP_CASES[0]
    m, sch, sd = make_mlp(c)
    B, L, C, N = 4, c["L"], c["C"], 12
    sampler = DiffusionSampler(score_model=m, sample_batch_size=B)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), 2 * (N + 1), 77))
    out = sampler.sample(num_samples=2 * B, num_diffusion_steps=N)
    noise = (torch.from_numpy(z) for z in synthetic.noise_stream((B, L, C), 2 * (N + 1), 77))
    ts = sch.timesteps
    ref = O.sample(sd, kind="mlp", n_channels=C, max_len=L, num_layers=c["NL"], n_head=1, sde="vp", sde_kwargs=cases.VP,
                   fourier_noise_scaling=True, num_samples=2 * B, batch_size=B, num_steps=N, noise=noise)
    assert tuple(out.shape) == (2 * B, L, C)
    assert rel_err(out, ref) < TOL_TRAJ


# ------------------------------------------ sampler option matrix vs the oracle ----
@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("use_cache", [False, True])
@pytest.mark.parametrize("fresca", [False, True])
def test_sampler_option_matrix_vs_oracle(ffd, sde, fourier, use_cache, fresca):
    """Every combination of scheduler, noise scaling, E2-CRF cache (R=100 so that a refresh step falls inside) and
    FreSca on the small model, two batches (Q3 cache semantics), against the oracle's sampler on the same draws."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    base = next(c for c in cases.MODEL_CASES if c["name"] == "small")
    c = dict(base, sde=sde, sde_kwargs=cases.VP if sde == "vp" else cases.VE, fourier=fourier)
    m, sch = make_model(ffd, c)
    sd = make_sd(c)
    B, L, C, N, ns = 2, c["L"], c["C"], 104, 4
    fk = dict(low_scale=0.9, high_scale=1.4, cutoff_ratio=0.5, cutoff_strategy="energy") if fresca else None
    fres = {} if fk is None else dict(use_fresca=True, fresca_low_scale=fk["low_scale"], fresca_high_scale=fk["high_scale"],
                                      fresca_cutoff_ratio=fk["cutoff_ratio"], fresca_cutoff_strategy=fk["cutoff_strategy"])
    ck = {"K": 3, "R": 100}
    sampler = DiffusionSampler(score_model=m, sample_batch_size=B, use_cache=use_cache, cache_kwargs=dict(ck),
                               z_chunk_steps=37, **fres)
    nb = ns // B
    sampler.inject_noise(synthetic.noise_stream((B, L, C), nb * (N + 1), 555))
    out = sampler.sample(num_samples=ns, num_diffusion_steps=N)
    noise = (torch.from_numpy(z) for z in synthetic.noise_stream((B, L, C), nb * (N + 1), 555))
    ref = O.sample(sd, kind="transformer", n_channels=C, max_len=L, num_layers=c["NL"], n_head=c["H"], sde=sde,
                   sde_kwargs=c["sde_kwargs"], fourier_noise_scaling=fourier, num_samples=ns, batch_size=B, num_steps=N,
                   noise=noise, use_cache=use_cache, K=ck["K"], R=ck["R"], fresca_kwargs=fk)
    assert tuple(out.shape) == tuple(ref.shape)
    assert rel_err(out, ref) < 2 * TOL_TRAJ, rel_err(out, ref)
    if use_cache:
        m.disable_caching()


@pytest.mark.parametrize("c", cases.EXTRA_TRAJ_CASES, ids=lambda c: c["name"])
def test_extra_traj_golden(ffd, golden, c):
    """G11: VE / time-domain x cache x FreSca combinations against the unmodified reference's output."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    nb = max(1, c["num_samples"] // B)
    fk = c.get("fresca")
    fres = {} if fk is None else dict(use_fresca=True, fresca_low_scale=fk["low_scale"], fresca_high_scale=fk["high_scale"],
                                      fresca_cutoff_ratio=fk["cutoff_ratio"], fresca_cutoff_strategy=fk["cutoff_strategy"])
    sampler = DiffusionSampler(score_model=m, sample_batch_size=B, use_cache=c["use_cache"],
                               cache_kwargs=dict(c.get("cache_kwargs", {})), z_chunk_steps=41, **fres)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), nb * (N + 1), c["zseed"]))
    g = golden["g11_extra_traj"]
    ts_golden = torch.from_numpy(g[c["name"] + "_ts"].copy())
    orig = sch.set_timesteps

    def pinned(n):
        orig(n)
        sch.timesteps = ts_golden
        sch.step_size = ts_golden[0] - ts_golden[1]

    sch.set_timesteps = pinned
    out = sampler.sample(num_samples=c["num_samples"], num_diffusion_steps=N)
    assert rel_err(out, g[c["name"]]) < TOL_TRAJ, rel_err(out, g[c["name"]])
    if c["use_cache"]:
        m.disable_caching()


def test_benchmark_sampling_harness(ffd):
    """T1: the cmd/benchmark_cache.py harness -- same keys, the reference's batching (B=1 -> num_samples batches),
    stats visible on the cache object the harness reads (Q5: zero hits on the sampler-visible object after the
    second enable_caching), cache on/off outputs on the same noise stay finite and close."""
    from fastfourierdiffusion_amd.benchmark import benchmark_sampling

    c = next(c for c in cases.MODEL_CASES if c["name"] == "small")
    m, _ = make_model(ffd, c)
    torch.manual_seed(0)
    off = benchmark_sampling(m, num_samples=3, num_diffusion_steps=12, use_cache=False)
    torch.manual_seed(0)
    on = benchmark_sampling(m, num_samples=3, num_diffusion_steps=12, use_cache=True, cache_kwargs={})
    for r in (off, on):
        assert set(r) == {"elapsed_time", "samples", "cache_stats", "num_samples", "num_diffusion_steps"}
        assert tuple(r["samples"].shape) == (3, c["L"], c["C"]) and r["samples"].device.type == "cpu"
        assert torch.isfinite(r["samples"]).all() and r["elapsed_time"] > 0
    assert off["cache_stats"] == {}
    assert {"cache_hit_ratio", "cache_ratio", "recompute_count", "cache_hit_count", "current_step"} <= set(on["cache_stats"])
    fr = benchmark_sampling(m, num_samples=2, num_diffusion_steps=8, use_cache=True, cache_kwargs={}, use_fresca=True)
    assert torch.isfinite(fr["samples"]).all()
    m.disable_caching()


# ------------------------------------------------------------- round 2 (g12) ----
def _pin_grid(sch, ts_np, N):
    """Golden trajectories were generated on the grid stored next to them (torch.linspace's last ulp depends on the
    host's vector width): make set_timesteps(N) install exactly that grid."""
    ts_golden = torch.from_numpy(np.asarray(ts_np).copy())
    orig = sch.set_timesteps

    def pinned(n):
        orig(n)
        assert n == N
        sch.timesteps = ts_golden
        sch.step_size = ts_golden[0] - ts_golden[1]

    sch.set_timesteps = pinned


@pytest.mark.parametrize("c", cases.MIXED_T_CASES, ids=lambda c: c["name"])
def test_mixed_timesteps_golden(ffd, golden, c):
    """ScoreModule.forward evaluates the time encoder PER SAMPLE (score_models.py:102); the reference's own unit
    test passes torch.randint timesteps (tests/test_score_models.py:70).  Golden from the reference (g12)."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    g = golden["g12_round2"]
    m, _ = make_model(ffd, c)
    B, L, C = c["B"], c["L"], c["C"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"]))).cuda()
    t = torch.tensor(c["t"], dtype=torch.int64 if c["int_t"] else torch.float32).cuda()
    sc = m(DiffusableBatch(X=x, y=None, timesteps=t))
    assert rel_err(sc.cpu(), g[c["name"] + "_score"]) < TOL_SCORE
    # each sample equals its own uniform-time evaluation (the time embedding is indexed by sample, nothing else is)
    for b in (0, B - 1):
        one = m(batch_of(x[b:b + 1].contiguous(), float(c["t"][b])))
        assert rel_err(one.cpu(), sc[b:b + 1].cpu()) < 2e-6
    if c.get("recompute"):
        m.enable_caching()
        m.cache.reset()
        for j, rec in enumerate(c["recompute"]):
            xj = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"] + 100 + j))).cuda()
            sc, crf = m(DiffusableBatch(X=xj, y=None, timesteps=t), recompute_tokens=set(rec), step=j, return_crf=True)
            assert rel_err(sc.cpu(), g[f"{c['name']}_cseq{j}_score"]) < TOL_SCORE, j
            assert rel_err(crf.cpu(), g[f"{c['name']}_cseq{j}_crf"]) < TOL_SCORE, j
        m.disable_caching()


def test_scalar_and_per_sample_time_entry_points_agree(ffd):
    """ffd_score_forward / ffd_score_forward_cached (one t for the batch) and ffd_score_forward_ts (device array of
    equal t) run the same kernels on the same embedding values: bit-identical scores, tables and CRF."""
    import ctypes as C

    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "small")
    m, _ = make_model(ffd, c)
    m.enable_caching()
    ctx = m._ctx()
    B, L, Cn = 3, c["L"], c["C"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 5))).cuda()
    ts = torch.full((B,), 0.37, device="cuda")
    s = N.current_stream_ptr(x.device)
    a, b = torch.empty_like(x), torch.empty_like(x)
    N.check(ctx.lib.ffd_score_forward(ctx.handle, x.data_ptr(), 0.37, a.data_ptr(), B, s), ctx.handle, "fwd")
    N.check(ctx.lib.ffd_score_forward_ts(ctx.handle, x.data_ptr(), ts.data_ptr(), b.data_ptr(), None, B, -1, s), ctx.handle, "fwd_ts")
    assert torch.equal(a, b)
    crf_a = torch.empty(c["NL"], L, c["d"], device="cuda")
    crf_b = torch.empty_like(crf_a)
    for n_rec in (L, 0, 10):
        N.check(ctx.lib.ffd_score_forward_cached(ctx.handle, x.data_ptr(), 0.37, a.data_ptr(), crf_a.data_ptr(), B, n_rec, s),
                ctx.handle, "cached")
        ka, va = m.cache_tables()
        N.check(ctx.lib.ffd_score_forward_ts(ctx.handle, x.data_ptr(), ts.data_ptr(), b.data_ptr(), crf_b.data_ptr(), B, n_rec, s),
                ctx.handle, "cached_ts")
        kb, vb = m.cache_tables()
        assert torch.equal(a, b) and torch.equal(crf_a, crf_b) and torch.equal(ka, kb) and torch.equal(va, vb)
    # a cached forward without ffd_cache_enable, and a bad recompute count, fail loudly
    m.disable_caching()
    with pytest.raises(AssertionError):
        N.check(ctx.lib.ffd_score_forward_ts(ctx.handle, x.data_ptr(), ts.data_ptr(), b.data_ptr(), None, B, L + 1, s),
                ctx.handle, "bad n_rec")


@pytest.mark.parametrize("c", cases.SYN_TRAJ_CASES, ids=lambda c: c["name"])
def test_syn_traj_golden(ffd, golden, c):
    """BASELINE configs[4] shape (L=512, C=8), cached trajectory pinned against the reference."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    g = golden["g12_round2"]
    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    _pin_grid(sch, g[c["name"] + "_ts"], N)
    sampler = DiffusionSampler(m, B, use_cache=True, cache_kwargs=dict(c["cache_kwargs"]))
    sampler.inject_noise(synthetic.noise_stream((B, L, C), max(1, c["num_samples"] // B) * (N + 1), c["zseed"]))
    out = sampler.sample(c["num_samples"], N)
    assert rel_err(out, g[c["name"]]) < TOL_TRAJ


def test_two_samplers_one_model_golden(ffd, golden):
    """cmd/benchmark_cache.py:274-311 builds sampler after sampler on ONE model with different cache kwargs.  The
    gate must follow the current sampler's cache (K, R) although the tables stay bound to the first (Q5)."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = cases.TWO_SAMPLER_CASE
    g = golden["g12_round2"]
    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    _pin_grid(sch, g[c["name"] + "_ts"], N)
    for tag, kw, zs in (("first", c["first_kwargs"], c["zseed1"]), ("second", c["second_kwargs"], c["zseed2"])):
        sampler = DiffusionSampler(m, B, use_cache=True, cache_kwargs=dict(kw))
        sampler.inject_noise(synthetic.noise_stream((B, L, C), max(1, c["num_samples"] // B) * (N + 1), zs))
        out = sampler.sample(c["num_samples"], N)
        assert rel_err(out, g[f"{c['name']}_{tag}"]) < TOL_TRAJ, tag
        st = m.cache.get_cache_stats()
        np.testing.assert_array_equal([st["recompute_count"], st["cache_hit_count"]], g[f"{c['name']}_{tag}_stats"])
    # the R=100 refresh really ran in the second sampling: with the first sampler's gate (R=10 -> interval 500) the
    # same noise gives a different trajectory
    s3 = DiffusionSampler(m, B, use_cache=True, cache_kwargs=dict(c["first_kwargs"]))
    s3.inject_noise(synthetic.noise_stream((B, L, C), max(1, c["num_samples"] // B) * (N + 1), c["zseed2"]))
    assert rel_err(s3.sample(c["num_samples"], N), g[f"{c['name']}_second"]) > 1e-4


def test_torch_rng_draw_order(ffd):
    """rng="torch" (the default) consumes torch's generators where the reference does (sampler.py:217-228 ->
    sde.py:79-87: one CPU torch.randn per batch for the prior; sde.py:241/160: one device randn_like per step), so a
    seeded run equals the injected-noise run fed with the same draws.  PARITY UNPINNED against the reference itself:
    its CPU run consumes the CPU generator for the steps, which no device run can reproduce."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = next(c for c in cases.TRAJ_CASES if c["name"] == "traj_small_vp")
    m, sch = make_model(ffd, c)
    B, L, C, N = 3, c["L"], c["C"], 6
    torch.manual_seed(123)
    a = DiffusionSampler(m, B, z_chunk_steps=4).sample(2 * B, N)
    torch.manual_seed(123)
    draws = []
    like = torch.empty(B, L, C, device="cuda")
    for _ in range(2):
        draws.append(torch.randn(B, L, C).numpy())
        draws += [torch.randn_like(like).cpu().numpy() for _ in range(N)]
    s = DiffusionSampler(m, B)
    s.inject_noise(iter(draws))
    b = s.sample(2 * B, N)
    assert torch.equal(a, b)


def test_cache_benchmark_grid_keys(ffd):
    """run_cache_benchmark = the body of cmd/benchmark_cache.py:159-422: baseline, default cache, cache + FreSca and the
    K / R / tau_0 / freq_decomp_interval / FreSca-h grids on one model, rows keyed like the reference's table."""
    from fastfourierdiffusion_amd.benchmark import ABLATION_GRID, run_cache_benchmark

    c = next(c for c in cases.MODEL_CASES if c["name"] == "small")
    m, _ = make_model(ffd, c)
    rows = run_cache_benchmark(m, num_samples=2, num_diffusion_steps=12)
    keys = {"Config", "Parameter", "Value", "Time (s)", "Speedup", "Time per Sample (s)", "Time per Step (s)",
            "Cache Hit Ratio", "Cache Ratio", "Freq Decomp Count"}
    assert all(set(r) == keys for r in rows)
    assert [r["Config"] for r in rows[:3]] == ["No Cache", "E2-CRF (default)", "E2-CRF + FreSca"]
    assert [r["Config"] for r in rows[3:11]] == ["K=0", "K=3", "K=5", "K=10", "R=5", "R=10", "R=20", "R=50"]
    assert len(rows) == 3 + sum(len(v) for *_, v in ABLATION_GRID)
    assert rows[0]["Speedup"] == 1.0 and all(r["Time (s)"] > 0 for r in rows)
    # only the first cached run's object is bound to the layers (Q5): later configurations read zero hits, as in
    # the reference's recorded ablation ("Hit: 0.0 %", notebooks/ablation_cache_test.ipynb:353-484)
    assert rows[1]["Cache Hit Ratio"] > 0.9 and all(r["Cache Hit Ratio"] == 0.0 for r in rows[2:])
    m.disable_caching()


def test_kernel_timing_and_work_accounting(ffd):
    """ffd_kernel_timing_*: every launch of the selected classes is bracketed by a HIP event pair on the launch
    stream; ffd_kernel_work returns the SURVEY 8(d) figures bench.py's roofline lines are computed from."""
    import ctypes as C

    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, sch = make_model(ffd, c)
    ctx = m._ctx()
    B, L, Cn, NL, d, F = 128, c["L"], c["C"], c["NL"], c["d"], 2048
    x = torch.randn(B, L, Cn, device="cuda")
    sch.set_timesteps(50)
    ts_c = (C.c_float * 50)(*sch.timesteps.tolist())
    s = N.current_stream_ptr(x.device)
    N.check(ctx.lib.ffd_kernel_timing_begin(ctx.handle, 0xFF, 3 * (3 * NL + 3)), ctx.handle, "begin")
    N.check(ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), B, ts_c, 50, float(sch.step_size), 0, 3, 1, 0, None, 0, 0, s),
            ctx.handle, "sample")
    N.check(ctx.lib.ffd_kernel_timing_end(ctx.handle), ctx.handle, "end")
    counts = {}
    for cls in range(8):
        ms, n = C.c_float(), C.c_int()
        N.check(ctx.lib.ffd_kernel_timing_get(ctx.handle, cls, C.byref(ms), C.byref(n)), ctx.handle, "get")
        counts[cls] = n.value
        assert (ms.value > 0) == (n.value > 0)
    assert counts[N.K_FFN] == counts[N.K_ATTN] == 3 * NL
    assert counts[N.K_OUTPROJ] == 0  # at this size the out-projection + LN1 run inside the FFN kernel
    assert counts[N.K_EMBED] == 3 and counts[N.K_LSTM_REC] == 0
    assert counts[N.K_SDE] == 3  # the unembed may be fused into it
    fl, by = C.c_double(), C.c_double()
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_FFN, 512, 0, C.byref(fl), C.byref(by)) == b"k_ffn_rows<oproj>"
    assert fl.value == 4.0 * 512 * L * d * F + 2.0 * 512 * L * d * d  # 56.47 + 0.99 GFLOP at the ECG bench shape
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_OUTPROJ, 512, 0, C.byref(fl), C.byref(by)) is None
    assert ctx.lib.ffd_tune(b"ffn_rows_fuse", 0) == 0
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_FFN, 512, 0, C.byref(fl), C.byref(by)) == b"k_ffn_rows"
    assert fl.value == 4.0 * 512 * L * d * F
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_OUTPROJ, 512, 0, C.byref(fl), C.byref(by)) == b"k_linear_res_ln"
    assert ctx.lib.ffd_tune(b"reset", 0) == 0
    # the sampling loop unembeds inside the step kernel: hidden row + x in, x out
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_SDE, 512, 0, C.byref(fl), C.byref(by)).startswith(b"k_unembed_mfma")
    assert by.value == 4.0 * 512 * L * (d + 2 * Cn)
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_LSTM_REC, 512, 0, C.byref(fl), C.byref(by)) is None
    # small M: the out-projection is absorbed into the F-split FFN pair (csrc/ffd_small.hip)
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_OUTPROJ, 1, 0, C.byref(fl), C.byref(by)) is None
    assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_FFN, 1, 0, C.byref(fl), C.byref(by)).startswith(b"k_oproj_ffn_split")
    assert fl.value == 4.0 * L * d * F + 2.0 * L * d * d

    # a batch sweep of timed forwards: ffd_kernel_work names a class exactly when the forward launched it, and the
    # launch counts are the plan's (one attention / FFN launch per layer; k_linear_res_ln only where named)
    def forward_counts(model, c_, B):
        ctx_ = model._ctx()
        xb = torch.randn(B, c_["L"], c_["C"], device="cuda")
        N.check(ctx_.lib.ffd_kernel_timing_begin(ctx_.handle, 0xFF, 4 * c_["NL"] + 8), ctx_.handle, "begin")
        model(batch_of(xb, 0.5))
        torch.cuda.synchronize()
        N.check(ctx_.lib.ffd_kernel_timing_end(ctx_.handle), ctx_.handle, "end")
        out = {}
        for cls in range(8):
            ms, n = C.c_float(), C.c_int()
            N.check(ctx_.lib.ffd_kernel_timing_get(ctx_.handle, cls, C.byref(ms), C.byref(n)), ctx_.handle, "get")
            name = ctx_.lib.ffd_kernel_work(ctx_.handle, cls, B, 0, C.byref(fl), C.byref(by))
            out[cls] = (name, n.value)
        return out

    for knob in (None, (b"ffn_rows_fuse", 0), (b"ffn_height", 2), (b"ffn_split", 1)):
        if knob:
            assert ctx.lib.ffd_tune(*knob) == 0
        for B in (1, 8, 16, 32, 50, 96, 200, 384, 512):
            got = forward_counts(m, c, B)
            for cls in (N.K_FFN, N.K_ATTN, N.K_OUTPROJ, N.K_LSTM_REC, N.K_LSTM_GATES, N.K_EMBED, N.K_UNEMBED):
                assert (got[cls][0] is not None) == (got[cls][1] > 0), (knob, B, cls, got[cls])
            assert got[N.K_FFN][1] == got[N.K_ATTN][1] == NL, (knob, B, got)
            assert got[N.K_OUTPROJ][1] in (0, NL), (knob, B, got)
        assert ctx.lib.ffd_tune(b"reset", 0) == 0
    # the FFN / attention probes run the planned form at a small and a mid batch
    for B in (8, 96):
        ms = C.c_float()
        N.check(ctx.lib.ffd_bench_ffn(ctx.handle, B, 5, C.byref(ms), None), ctx.handle, "bench_ffn")
        assert ms.value > 0
        ms = C.c_float()
        N.check(ctx.lib.ffd_probe_attn(ctx.handle, B, -1, 0.0, 5, C.byref(ms), None, 0, None, None), ctx.handle, "probe_attn")
        assert ms.value > 0
    cl = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    ml, _ = make_model(ffd, cl)
    for wave in (1, 0):
        assert ml._ctx().lib.ffd_tune(b"lstm_wave", wave) == 0
        for B in (1, 64, 512):
            got = forward_counts(ml, cl, B)
            for cls in (N.K_FFN, N.K_ATTN, N.K_OUTPROJ, N.K_LSTM_REC, N.K_LSTM_GATES):
                assert (got[cls][0] is not None) == (got[cls][1] > 0), (wave, B, cls, got[cls])
            assert got[N.K_LSTM_REC] == ((b"k_lstm_wave", 1) if wave else (b"k_lstm_layer", cl["NL"])), (B, got)
            assert got[N.K_LSTM_GATES][1] == (0 if wave else cl["NL"]), (B, got)
    assert ml._ctx().lib.ffd_tune(b"reset", 0) == 0


@pytest.mark.parametrize("case", cases.AFFINE_FFT_CASES, ids=lambda c: f"L{c[0]}C{c[1]}")
def test_affine_fft_golden(ffd, golden, case):
    """cmd/sample.py:107-113 (X * std + mean, then idft) and datamodules.py:42-62 ((dft(X) - mean) / std), each
    fused into the transform kernel; goldens from the reference's own tensor ops + dft / idft (g12)."""
    from fastfourierdiffusion_amd.utils.fourier import dft, dft_standardize, idft, unstandardize_idft

    L, C, B, seed = case
    x, mean, std = (torch.from_numpy(a) for a in synthetic.noise_stream((B, L, C), 3, seed))
    mean, std = mean[0], std[0].abs() + 0.5
    g = golden["g12_round2"]
    xs = unstandardize_idft(x.cuda(), mean, std)
    assert xs.device.type == "cuda" and rel_err(xs.cpu(), g[f"unstd_idft_L{L}_C{C}"]) < TOL_OP
    xf = dft_standardize(x, mean, std)  # host tensor in -> host tensor out, like dft / idft
    assert xf.device.type == "cpu" and rel_err(xf, g[f"dft_std_L{L}_C{C}"]) < TOL_OP
    # the fused forms equal the two-step forms bit for bit (same kernel, same rounding sequence as the reference's ops)
    assert torch.equal(xs.cpu(), idft((x * std + mean).cuda()).cpu())
    assert torch.equal(xf, (dft(x) - mean) / std)


@pytest.mark.parametrize("shape", [(3, 2, 1), (2, 4, 3), (5, 8, 8), (2, 16, 4), (3, 32, 5), (2, 64, 8), (2, 128, 1),
                                   (3, 1024, 8), (2, 2048, 4), (1, 4096, 3), (2, 512, 72), (2, 256, 40)])
def test_pow2_real_fft_paths_vs_oracle(ffd, shape):
    """Power-of-two lengths run the half-length complex FFT + split kernel (k_rfft_pow2): every radix plan
    (2 | 4 | 4,4 | 8 ... ), the float4 slab path (C % 4 == 0) and the scalar one, channel groups split over
    workgroups when the slab exceeds the CU's LDS, plus FreSca / decomposition on the same path."""
    from fastfourierdiffusion_amd.utils.fourier import dft, frequency_decompose_fft, idft
    from fastfourierdiffusion_amd.utils.fresca import apply_fresca_to_score

    B, L, C = shape
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 1000 + L + C)))
    xf = dft(x.cuda())
    assert rel_err(xf.cpu(), O.dft(x)) < TOL_OP
    assert rel_err(idft(x.cuda()).cpu(), O.idft(x)) < TOL_OP
    assert rel_err(idft(xf).cpu(), x) < 2 * TOL_OP
    if L >= 4 and L <= 1024:
        for strat in ("energy", "spatial"):
            y = apply_fresca_to_score(x.cuda(), low_scale=0.9, high_scale=1.4, cutoff_ratio=0.45, cutoff_strategy=strat)
            assert rel_err(y.cpu(), O.fresca(x, 0.9, 1.4, 0.45, strat, None, None)) < TOL_OP, strat
        lo, hi = frequency_decompose_fft(x.cuda(), 0.3)
        olo, ohi = O.frequency_decompose(x, 0.3)
        assert rel_err(lo.cpu(), olo) < TOL_OP and rel_err(hi.cpu(), ohi) < TOL_OP


@pytest.mark.parametrize("name", ["ecg", "small", "syn", "nasa_lstm"])
def test_fused_unembed_sde_tail_equals_two_kernels(ffd, name):
    """ffd_sample_batch unembeds inside the SDE-step kernel (k_unembed_mfma<D, TailSde>): same MFMA sequence for the
    score, same sde_update, same Philox indexing as unembed + k_step<OpSde> -> bit-identical trajectories, with
    on-device Philox noise and with injected draws, C = 1 / 3 / 4 / 8."""
    import ctypes as C

    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == name)
    m, sch = make_model(ffd, c)
    ctx = m._ctx()
    B, L, Cn = 3, c["L"], c["C"]
    sch.set_timesteps(20)
    ts_c = (C.c_float * 20)(*sch.timesteps.tolist())
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 77))).cuda()
    zs = torch.from_numpy(np.stack(list(synthetic.noise_stream((B, L, Cn), 4, 78)))).cuda()
    s = N.current_stream_ptr(x0.device)
    res = {}
    try:
        for fuse in (1, 0):
            assert ctx.lib.ffd_tune(b"fuse_tail", fuse) == 0
            for z in (None, zs):
                x = x0.clone()
                N.check(ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), B, ts_c, 20, float(sch.step_size), 2, 4, 9, 5,
                                                 z.data_ptr() if z is not None else None, 0, 0, s), ctx.handle, "sample")
                res[(fuse, z is None)] = x
    finally:
        ctx.lib.ffd_tune(b"fuse_tail", 1)
    for philox in (True, False):
        assert torch.isfinite(res[(1, philox)]).all()
        assert torch.equal(res[(1, philox)], res[(0, philox)]), philox


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nasa_lstm", "small_lstm", "refunit_lstm"])
def test_lstm_wavefront_golden(ffd, golden, name):
    """The LSTM layers as a wavefront of (16-sample tile, layer) workgroups in one launch (k_lstm_wave: the production
    selection at every batch) against the reference's
    scores (g5), and against the per-layer kernels (ffd_tune "lstm_wave" = 0)."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == name)
    m, _ = make_model(ffd, c)
    g = golden["g5_models"]
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((c["B"], c["L"], c["C"]), 1, c["xseed"]))).cuda()
    for tv in c["t_values"]:
        assert lib.ffd_tune(b"lstm_wave", 1) == 0
        w = m(batch_of(x, tv)).cpu()
        assert lib.ffd_tune(b"lstm_wave", 0) == 0
        per_layer = m(batch_of(x, tv)).cpu()
        assert rel_err(w, g[f"{name}_score_t{tv}"]) < TOL_SCORE, (name, tv)
        assert rel_err(w, per_layer) < 2e-6, (name, tv)


@pytest.mark.gpu
def test_lstm_wavefront_ragged_batches_and_layer_groups(ffd):
    """k_lstm_wave over batch sizes that leave a ragged last tile, one tile, and more tiles than a launch holds with
    all ten layers (B = 512: 32 tiles x 10 layers on 256 workgroups; B = 1100: 69 tiles -> 3 layers in flight): every
    sample equals its evaluation in a small batch, a slice equals the oracle."""
    c = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    for B in (1, 37, 512, 1100):
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4500 + B)))
        out = m(batch_of(x.cuda(), 0.45)).cpu()
        assert torch.isfinite(out).all()
        for b in sorted({0, B // 2, B - 1}):
            lo = min(b, max(0, B - 2))
            two = m(batch_of(x[lo:lo + 2].cuda(), 0.45)).cpu()
            assert rel_err(out[b:b + 1], two[b - lo:b - lo + 1]) < 2e-6, (B, b)
        n = min(2, B)
        ref = O.lstm_score_forward(x[:n], torch.full((n,), 0.45, dtype=torch.float32), sd, c["NL"])
        assert rel_err(out[:n], ref) < TOL_SCORE, B
        if B in (37, 512):
            # a workgroup walks its tile's layers l0, l0 + per, ...: the same bits as one launch per layer group, and
            # for any number of layers in flight
            from fastfourierdiffusion_amd import _native as N
            lib = N.lib()
            # ... and where the (tile, layer) pairs outnumber the workgroups, for any chunk length of the time-shared
            # form (units of `chunk` cell steps, state handed over through memory; 1 = layers walked whole, 0 = the default choice)
            for per, persist, chunk in ((0, 0, 16), (1, 1, 16), (2, 1, 2), (3, 1, 64), (3, 0, 16), (0, 1, 1), (0, 1, 30),
                                        (2, 1, 1), (3, 1, 0), (4, 1, 0)):
                assert lib.ffd_tune(b"lstm_wave_per", per) == 0 and lib.ffd_tune(b"lstm_wave_persist", persist) == 0
                assert lib.ffd_tune(b"lstm_wave_chunk", chunk) == 0
                assert torch.equal(m(batch_of(x.cuda(), 0.45)).cpu(), out), (B, per, persist, chunk)
            assert lib.ffd_tune(b"reset", 0) == 0


def test_lstm_wavefront_more_layers_than_a_launch_holds(ffd):
    """k_lstm_wave takes up to 16 layers per launch (its argument block): a 19-layer model runs as 16 + 3, the second
    launch on the rows the first one left, time-shared or not -- against the oracle and the per-layer kernels."""
    from fastfourierdiffusion_amd import _native as N

    c = dict(next(c for c in cases.MODEL_CASES if c["name"] == "small_lstm"))
    c["NL"] = 19
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    lib = N.lib()
    for B in (5, 300):
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 5100 + B)))
        assert lib.ffd_tune(b"lstm_wave", 2) == 0
        outs = []
        for per, chunk in ((0, 0), (3, 4), (5, 1)):
            assert lib.ffd_tune(b"lstm_wave_per", per) == 0 and lib.ffd_tune(b"lstm_wave_chunk", chunk) == 0
            outs.append(m(batch_of(x.cuda(), 0.6)).cpu())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), B
        assert lib.ffd_tune(b"reset", 0) == 0 and lib.ffd_tune(b"lstm_wave", 0) == 0
        base = m(batch_of(x.cuda(), 0.6)).cpu()
        assert lib.ffd_tune(b"reset", 0) == 0
        assert rel_err(outs[0], base) < 2e-6, B
        n = min(2, B)
        ref = O.lstm_score_forward(x[:n], torch.full((n,), 0.6, dtype=torch.float32), sd, c["NL"])
        assert rel_err(outs[0][:n], ref) < TOL_SCORE, B


@pytest.mark.parametrize("B", [2048, 8192])
def test_config5_shard_cached_modes_at_size(ffd, B):
    """BASELINE configs[4] per-GPU shard (L = 512, C = 8, transformer d72/H12/NL10) through the E2-CRF modes
    FULL -> PURE -> MIXED -> PURE at B = 2048 and at the full shard size 8192 (98 304 attention workgroups, M = 4.2 M
    rows).  Size-independent properties: the tables come from batch element 0 only (Q1), so every sample of the big
    batch equals its evaluation inside a 3-sample batch that starts with element 0; a 2-sample slice {0, 1} equals the
    oracle; the cache counters equal the reference's per-call increments (caching.py:283,299,396)."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    c = next(c for c in cases.MODEL_CASES if c["name"] == "syn")
    L, C, NL, H = c["L"], c["C"], c["NL"], c["H"]
    sd = make_sd(c)
    seq = [list(range(L)), [], list(range(10)), []]
    picks = [0, B // 2 + 3, B - 1]
    g = torch.Generator().manual_seed(B)
    xs = [torch.randn(B, L, C, generator=g) for _ in seq]
    tv = 0.4

    def run(m, xlist):
        m.enable_caching()
        m.cache.reset()
        outs = []
        for j, (rec, xj) in enumerate(zip(seq, xlist)):
            t = torch.full((xj.shape[0],), tv, device="cuda")
            sc, crf = m(DiffusableBatch(X=xj.cuda(), y=None, timesteps=t), recompute_tokens=set(rec), step=j, return_crf=True)
            outs.append((sc.cpu(), crf.cpu()))
        st = m._first_cache.get_cache_stats()
        m.disable_caching()
        return outs, st

    m, _ = make_model(ffd, c)
    big, st = run(m, xs)
    assert st["recompute_count"] == (L + 10) * NL and st["cache_hit_count"] == (2 * L + (L - 10)) * NL
    m2, _ = make_model(ffd, c)
    small, _ = run(m2, [x[picks] for x in xs])
    for j in range(len(seq)):
        assert torch.isfinite(big[j][0]).all()
        assert rel_err(big[j][0][picks], small[j][0]) < 2e-6, j   # same kernels; tile / workgroup mapping differs
        assert rel_err(big[j][1], small[j][1]) < 2e-6, j          # CRF = element 0's hidden states
    table = O.KVTable(NL, L)
    t2 = torch.full((2,), tv)
    for j, rec in enumerate(seq):
        ref, crf = O.score_forward(xs[j][:2], t2, sd, NL, H, table, rec, return_crf=True)
        assert rel_err(big[j][0][:2], ref) < TOL_SCORE, j
        assert rel_err(big[j][1], crf) < TOL_SCORE, j


def test_ffn_rows_tile_to_wave_assignment_never_shows(ffd):
    """The FFN at large M is k_ffn_rows: row-owning waves (32 rows each, whole hidden dimension) under a CU-shared LDS
    weight ring; by default the out-projection + LN1 run inside it too, from one more ring slot (two-chunk slots).
    Which wave of which workgroup owns a row, and how many chunks a ring slot holds, must not show in the result: the
    ECG B = 512 score is bit-identical for 4 / 8 / 12 waves per workgroup (tiles of 128 / 256 / 384 rows) and for one or
    two chunks per slot in the unfused form, and for
    4 / 8 / 12 waves in the fused form; fused and unfused agree to rounding (other k order in the out-projection); a
    ragged last tile (M = 513 * 187 rows) stays finite and independent; the F-split kernel it replaces (k_ffn_ln,
    other summation order) agrees to rounding."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((513, c["L"], c["C"]), 1, 909))).cuda()
    refs = {}
    for fuse, cfgs in ((0, ((0, 0), (4, 1), (4, 2), (8, 1), (8, 2), (12, 1), (12, 2))),
                       (1, ((0, 0), (4, 2), (8, 2), (12, 2)))):
        outs = {}
        for nw, cps in cfgs:
            assert lib.ffd_tune(b"ffn_rows_fuse", fuse) == 0
            assert lib.ffd_tune(b"ffn_rows_nw", nw) == 0 and lib.ffd_tune(b"ffn_rows_cps", cps) == 0
            outs[(nw, cps)] = m(batch_of(x[:512].contiguous(), 0.3))
        refs[fuse] = outs[(0, 0)]
        for k, v in outs.items():
            assert torch.equal(refs[fuse], v), (fuse, k)
    assert rel_err(refs[0].cpu(), refs[1].cpu()) < 2e-6
    assert lib.ffd_tune(b"reset", 0) == 0
    ref = refs[1]  # the default form
    ragged = m(batch_of(x, 0.3))
    assert torch.isfinite(ragged).all()
    assert torch.equal(ragged[:512], ref)  # a row's result does not depend on the batch around it
    one = m(batch_of(x[512:513].contiguous(), 0.3))  # (B = 1 runs the small-batch kernels: other summation order)
    assert rel_err(ragged[512:513].cpu(), one.cpu()) < 2e-6
    assert lib.ffd_tune(b"ffn_rows", 0) == 0
    old = m(batch_of(x[:512].contiguous(), 0.3))
    assert rel_err(old.cpu(), ref.cpu()) < 2e-6


@pytest.mark.parametrize("name,batches", [("ecg", (24, 96, 130)), ("syn", (30, 48))])
def test_rows_sliced_form_agrees_with_the_other_forms(ffd, name, batches):
    """Mid-size batches run the fused out-proj + FFN kernel over tiles x slices of the hidden dimension (a unit per CU)
    and add the slices' partial rows in order in a reduce / LN2 launch: every (waves, slices) choice agrees with the
    forms it replaces to rounding, is deterministic, and a sample's result does not depend on the batch around it."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == name)
    m, _ = make_model(ffd, c)
    lib = N.lib()
    for B in batches:
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4242 + B))).cuda()
        assert lib.ffd_tune(b"rows_slices", -1) == 0
        ref = m(batch_of(x, 0.4))
        for nw in (8, 12):
            for S in (2, 3, 5, 8, 16):
                if -(-B * c["L"] // (32 * nw)) * S > 256:
                    continue
                assert lib.ffd_tune(b"ffn_rows_nw", nw) == 0 and lib.ffd_tune(b"rows_slices", S) == 0
                assert lib.ffd_tune(b"rows_slices_fuse", 1) == 0  # the out-projection + LN1 inside every unit
                a = m(batch_of(x, 0.4))
                b = m(batch_of(x, 0.4))
                assert torch.equal(a, b), (B, nw, S)
                assert rel_err(a.cpu(), ref.cpu()) < 2e-6, (B, nw, S)
                assert lib.ffd_tune(b"rows_slices_fuse", 2) == 0  # k_linear_res_ln once in front, slices without that slot
                u = m(batch_of(x, 0.4))
                assert torch.equal(u, m(batch_of(x, 0.4))), (B, nw, S)
                assert rel_err(u.cpu(), ref.cpu()) < 2e-6, (B, nw, S)
                assert lib.ffd_tune(b"rows_slices_fuse", 1) == 0
                part = m(batch_of(x[: B // 2].contiguous(), 0.4))  # other tile / unit assignment
                assert rel_err(part.cpu(), a[: B // 2].cpu()) < 2e-6, (B, nw, S)
        assert lib.ffd_tune(b"reset", 0) == 0
        auto = m(batch_of(x, 0.4))
        assert rel_err(auto.cpu(), ref.cpu()) < 2e-6, B


@pytest.mark.parametrize("name,batches", [("ecg", (13, 20, 32, 40, 50, 64)), ("syn", (5, 7, 12, 20)),
                                          ("reftest", (60, 120, 200)), ("small", (150, 300, 500))])
def test_tile_height_form_agrees_with_the_other_forms(ffd, name, batches):
    """Where the 16-row tiles are 1.4 - 3 per CU (ECG: B = 30 ... 65, the reference's default sample_batch_size of 50
    among them) the feed-forward block runs as k_linear_res_ln + k_ffn_ln at 32 / 48 rows per workgroup, one tile per
    CU: equal to the forms it replaces (the small-batch pair, the sliced row-owning kernel, 16- and 64-row tiles) to
    rounding, deterministic, independent of the batch around a sample; forced heights of 1 ... 4 agree as well."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == name)
    m, _ = make_model(ffd, c)
    lib = N.lib()
    for B in batches:
        x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 777 + B))).cuda()
        assert lib.ffd_tune(b"reset", 0) == 0
        a = m(batch_of(x, 0.6))
        assert torch.equal(a, m(batch_of(x, 0.6))), B
        assert lib.ffd_tune(b"ffn_height", 0) == 0
        ref = m(batch_of(x, 0.6))
        assert rel_err(a.cpu(), ref.cpu()) < 2e-6, B
        assert lib.ffd_tune(b"ffn_height", 2) == 0  # the same tiles behind a k_linear_res_ln launch
        u = m(batch_of(x, 0.6))
        assert torch.equal(u, m(batch_of(x, 0.6))) and rel_err(u.cpu(), ref.cpu()) < 2e-6, B
        assert lib.ffd_tune(b"reset", 0) == 0
        part = m(batch_of(x[: B // 2 + 1].contiguous(), 0.6))  # (may be another form: to rounding)
        assert rel_err(part.cpu(), a[: B // 2 + 1].cpu()) < 2e-6, B
        for mb in (1, 2, 3, 4):
            assert lib.ffd_tune(b"small_path", 0) == 0 and lib.ffd_tune(b"rows_slices", -1) == 0
            assert lib.ffd_tune(b"mid_path", 0) == 0 and lib.ffd_tune(b"ffn_rows", 0) == 0 and lib.ffd_tune(b"ffn_mb", mb) == 0
            f = m(batch_of(x, 0.6))
            assert rel_err(f.cpu(), ref.cpu()) < 2e-6, (B, mb)
            part = m(batch_of(x[: B // 2 + 1].contiguous(), 0.6))  # another tile assignment
            assert rel_err(part.cpu(), f[: B // 2 + 1].cpu()) < 2e-6, (B, mb)
        assert lib.ffd_tune(b"reset", 0) == 0
    # the plan itself: B = 50 at the ECG shape is one 48-row tile per CU
    if name == "ecg":
        assert lib.ffd_tune(b"reset", 0) == 0
        fl, by = C_.c_double(), C_.c_double()
        ctx = m._ctx()
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_FFN, 50, 0, C_.byref(fl), C_.byref(by)) == b"k_ffn_ln<oproj>"
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_OUTPROJ, 50, 0, C_.byref(fl), C_.byref(by)) is None
        assert lib.ffd_tune(b"ffn_height", 2) == 0
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_FFN, 50, 0, C_.byref(fl), C_.byref(by)) == b"k_ffn_ln"
        assert ctx.lib.ffd_kernel_work(ctx.handle, N.K_OUTPROJ, 50, 0, C_.byref(fl), C_.byref(by)) == b"k_linear_res_ln"
        assert lib.ffd_tune(b"reset", 0) == 0


def test_lstm_trace_records_every_unit(ffd):
    """ffd_lstm_trace (diagnostics): one record per (chunk, layer, tile) unit of the traced k_lstm_wave launch -- start <=
    start-up done <= end, waits inside the unit's duration, layer l never starts before layer l - 1 of its tile and chunk;
    the traced forward returns the same scores as an untraced one (bit for bit)."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    m, _ = make_model(ffd, c)
    ctx = m._ctx()
    B, NL = 40, c["NL"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 99))).cuda()
    ref = m(batch_of(x, 0.5))
    tiles = -(-B // 16)
    cap = NL * tiles
    N.check(ctx.lib.ffd_lstm_trace(ctx.handle, None, cap, None), ctx.handle, "arm")
    got = m(batch_of(x, 0.5))
    raw = (C_.c_uint64 * (4 * cap))()
    n = C_.c_int()
    N.check(ctx.lib.ffd_lstm_trace(ctx.handle, raw, cap, C_.byref(n)), ctx.handle, "read")
    assert torch.equal(got, ref) and n.value == cap
    r = np.frombuffer(raw, dtype=np.uint64).reshape(cap, 4).astype(np.int64)
    wait = r[:, 3] & ((1 << 48) - 1)
    assert (r[:, 0] > 0).all() and (r[:, 0] <= r[:, 1]).all() and (r[:, 1] <= r[:, 2]).all()
    assert (wait <= r[:, 2] - r[:, 0]).all()
    start = r[:, 0].reshape(NL, tiles)
    assert (start[1:] >= start[:-1] - 100).all()  # (all units of this launch are resident: layers start together, +- 1 us)
    end = r[:, 2].reshape(NL, tiles)
    assert (end[1:] > end[:-1]).all()  # a layer cannot finish before the one it reads from
    assert ctx.lib.ffd_lstm_trace(ctx.handle, raw, cap, C_.byref(n)) != 0  # nothing armed: an error, not stale records


def test_rows_sliced_form_in_rounds(ffd):
    """Round 4: where tiles x slices exceeds the CUs (ECG B = 384: 187 tiles x 4 slices) the sliced form's workgroups walk
    several tiles of their slice: bit-identical with the one-round result of the same slicing wherever both exist (a
    smaller batch whose units fit the chip), equal to the unsliced form to rounding, independent of the batch around a
    sample, and the default plan at B = 384 / 768 is such a multi-round slicing."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((768, c["L"], c["C"]), 1, 777))).cuda()
    for B, nw, S in ((384, 12, 4), (384, 8, 3), (768, 12, 2), (500, 12, 5)):
        xb = x[:B].contiguous()
        assert lib.ffd_tune(b"rows_slices", -1) == 0
        ref = m(batch_of(xb, 0.4))
        assert lib.ffd_tune(b"ffn_rows_nw", nw) == 0 and lib.ffd_tune(b"rows_slices", S) == 0
        assert -(-B * c["L"] // (32 * nw)) * S > 256  # more units than CUs: rounds
        for fuse in (1, 2):  # out-projection inside every unit | k_linear_res_ln once in front
            assert lib.ffd_tune(b"rows_slices_fuse", fuse) == 0
            a = m(batch_of(xb, 0.4))
            assert torch.equal(a, m(batch_of(xb, 0.4))), (B, nw, S, fuse)
            assert rel_err(a.cpu(), ref.cpu()) < 2e-6, (B, nw, S, fuse)
            nfit = (256 // S) * 32 * nw // c["L"]  # samples whose tiles x S units fit the chip in one round
            one_round = m(batch_of(xb[:nfit].contiguous(), 0.4))
            assert torch.equal(one_round, a[:nfit]), (B, nw, S, fuse)  # same slicing, same summation order: the same bits
        assert lib.ffd_tune(b"reset", 0) == 0
    for B in (384, 768):
        xb = x[:B].contiguous()
        auto = m(batch_of(xb, 0.4))
        assert lib.ffd_tune(b"rows_slices", -1) == 0
        assert rel_err(auto.cpu(), m(batch_of(xb, 0.4)).cpu()) < 2e-6, B
        assert lib.ffd_tune(b"reset", 0) == 0


def test_ffn_ln_persistent_grid_equals_one_workgroup_per_tile(ffd):
    """k_ffn_ln (the F-split workgroup; large M of every d_model without a k_ffn_rows instance, selected here with
    ffd_tune "ffn_rows" = 0) walks its tiles with a persistent grid: bit-identical with one workgroup per tile and with
    a 2x grid."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((512, c["L"], c["C"]), 1, 909))).cuda()
    assert lib.ffd_tune(b"ffn_rows", 0) == 0
    outs = {}
    for p in (1, 0, 2):
        assert lib.ffd_tune(b"ffn_persist", p) == 0
        outs[p] = m(batch_of(x, 0.3))
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[1], outs[2])


def test_shard_invariance_with_and_without_batch_statistics(ffd):
    """Philox noise is keyed by the global element index, so two half-batches (sample_offset 0 / B/2) reproduce the
    full batch -- with FreSca off and with its `spatial` cutoff.  FreSca's default `energy` cutoff is a mean over the
    LOCAL batch (fresca.py:150-158): a shard is then the reference run of its own batch, not a slice of the big one
    (documented in sampler.py / sharding.py); the test pins both facts."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = next(c for c in cases.TRAJ_CASES if c["name"] == "traj_small_vp")
    m, _ = make_model(ffd, c)
    B, N = 8, 12

    def run(bs, off, **kw):
        return DiffusionSampler(m, bs, rng="philox", seed=11, sample_offset=off, **kw).sample(bs, N)

    for kw in ({}, dict(use_fresca=True, fresca_cutoff_strategy="spatial", fresca_high_scale=1.4)):
        full = run(B, 0, **kw)
        halves = torch.cat([run(B // 2, 0, **kw), run(B // 2, B // 2, **kw)])
        assert rel_err(halves, full) < 2e-6, kw
    kw = dict(use_fresca=True, fresca_cutoff_strategy="energy", fresca_high_scale=1.4, fresca_cutoff_ratio=0.6)
    full = run(B, 0, **kw)
    lone = DiffusionSampler(m, B // 2, rng="philox", seed=11, sample_offset=B // 2, **kw).sample(B // 2, N)
    assert torch.isfinite(lone).all() and tuple(lone.shape) == (B // 2, c["L"], c["C"])
    # the second half run on its own equals the oracle-defined behaviour of a B/2 batch; it may or may not equal the
    # slice of the big batch (the cutoff index is a batch statistic) -- only finiteness and shape are contractual
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_shards_in_other_kernel_regimes_agree_to_rounding(ffd):
    """A shard can fall into another kernel regime than the whole batch: the ECG batch of 192 samples runs
    k_ffn_rows and one workgroup per head pair; its shards of 48 run the F-sliced mid-batch FFN and shards of 2 the
    F-split small-batch pair and the key-split attention.  Same Philox noise (keyed by global element index), samples
    equal to fp32 rounding -- the statement sampler.py / sharding.py make -- not bit for bit."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    B, N = 192, 6

    def run(bs, off):
        return DiffusionSampler(m, bs, rng="philox", seed=5, sample_offset=off).sample(bs, N)

    full = run(B, 0)
    quarters = torch.cat([run(48, o) for o in range(0, B, 48)])
    assert rel_err(quarters, full) < TOL_TRAJ
    for o in (0, 94, 190):
        assert rel_err(run(2, o), full[o:o + 2]) < TOL_TRAJ, o


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8, 16, 32, 64, 96])
def test_small_batch_split_ffn_matches_large_batch_kernels(ffd, B):
    """Small M (the benchmark_cache.py harness's batch of one): out-proj + LN1 + FFN + LN2 run as an F-split pair of
    launches (csrc/ffd_small.hip) instead of the two large-M kernels.  Same arithmetic, a different fp32 summation
    order over the hidden dimension: the scores agree to 2e-6 relative, the split path is deterministic, and it stays
    within the oracle tolerance on the way (the golden cases all run through it).  B = 1, 2, 3: 16 splits, two 16-unit
    chunks per wave; B = 4: 8 x 4; B = 8: 4 x 8; B = 16: 2 x 16; B = 32: 4 x 8; B = 64: 2 x 16; B = 96: the large-M kernels."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4242))).cuda()
    try:
        assert lib.ffd_tune(b"small_path", 1) == 0
        a = m(batch_of(x, 0.37))
        a2 = m(batch_of(x, 0.37))
        assert lib.ffd_tune(b"small_path", 0) == 0
        b = m(batch_of(x, 0.37))
    finally:
        lib.ffd_tune(b"small_path", 1)
    assert torch.equal(a, a2)
    assert torch.isfinite(a).all()
    assert rel_err(a.cpu(), b.cpu()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("kspl", [2, 4])
def test_small_batch_attention_key_pieces(ffd, kspl):
    """Small batches: each (sample, head) is spread over several workgroups and the key range of a q-tile over
    `kspl` waves whose pieces merge in LDS (csrc/ffd_qkvattn.hip, SPLIT).  Against the one-workgroup-per-head-pair
    kernel on the same inputs, in every cache mode (FULL -> PURE -> MIXED -> PURE), with tables published by the split
    kernel and read by the other and vice versa."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    lib = N.lib()
    L, C = c["L"], c["C"]
    outs = {}
    try:
        for mode in (kspl, 0):
            assert lib.ffd_tune(b"attn_small", mode) == 0
            m, _ = make_model(ffd, c)
            m.enable_caching()
            m.cache.reset()
            res = []
            for j, n in enumerate([L, 0, 37, 0, L - 3]):
                x = torch.from_numpy(next(synthetic.noise_stream((3, L, C), 1, 5100 + j))).cuda()
                res.append(m(batch_of(x, 0.45), recompute_tokens=set(range(n)), step=j))
            m.disable_caching()
            res.append(m(batch_of(x, 0.45)))
            outs[mode] = res
    finally:
        lib.ffd_tune(b"attn_small", 1)
    for a, b in zip(outs[kspl], outs[0]):
        assert torch.isfinite(a).all()
        assert rel_err(a.cpu(), b.cpu()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 64, 512])
def test_ffn_split_bf16x3_against_fp32_kernels(ffd, B):
    """Opt-in ffd_tune("ffn_split", 1): both FFN products on the bf16 matrix cores with every fp32 operand cut into
    three bf16 parts and the six largest cross terms kept (everything down to 2^-24 relative), fp32 accumulation.
    Against the fp32-MFMA kernels on the same inputs the ECG score (10 layers) agrees to 2e-6 relative, i.e. like two
    fp32 summation orders; ragged last tiles (B = 1: 187 rows, B = 5: 935 rows) included; deterministic."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 777))).cuda()
    try:
        ref = m(batch_of(x, 0.41))
        assert lib.ffd_tune(b"ffn_split", 1) == 0
        a = m(batch_of(x, 0.41))
        a2 = m(batch_of(x, 0.41))
    finally:
        lib.ffd_tune(b"ffn_split", 0)
    assert torch.isfinite(a).all() and torch.equal(a, a2)
    assert rel_err(a.cpu(), ref.cpu()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,ns", [(50, 8), (100, 2), (200, 4), (200, 8), (257, 2)])
def test_mid_batch_ffn_over_f_slices_matches_the_persistent_kernel(ffd, B, ns):
    """Mid-size M (the reference's default sample_batch_size = 50, its former 200): the 64-row FFN main loop over NS
    slices of the hidden dimension, partial tiles summed in slice order by k_ffn_reduce_ln (csrc/ffd_small.hip:
    k_ffn_part).  Against k_linear_res_ln + k_ffn_ln on the same inputs: 2e-6 relative, deterministic; B = 257 ends in a
    ragged 64-row tile (48 063 rows)."""
    from fastfourierdiffusion_amd import _native as N

    c = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 2024))).cuda()
    try:
        assert lib.ffd_tune(b"small_path", 0) == 0
        assert lib.ffd_tune(b"mid_path", ns) == 0
        a = m(batch_of(x, 0.6))
        a2 = m(batch_of(x, 0.6))
        assert lib.ffd_tune(b"mid_path", 0) == 0
        b = m(batch_of(x, 0.6))
    finally:
        lib.ffd_tune(b"mid_path", 1)
        lib.ffd_tune(b"small_path", 1)
    assert torch.isfinite(a).all() and torch.equal(a, a2)
    assert rel_err(a.cpu(), b.cpu()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(72, 12, 187), (60, 12, 50), (48, 12, 33), (64, 8, 100), (32, 4, 64), (16, 4, 20), (24, 8, 45),
                                   (8, 4, 31)], ids=lambda s: f"d{s[0]}h{s[1]}L{s[2]}")
def test_f_sliced_ffn_forms_on_every_d_model(ffd, shape):
    """Every d_model instance of the F-sliced FFN kernels (k_ffn_part forced with 2 / 4 / 8 slices, and the 16-row pair)
    against the oracle and against k_linear_res_ln + k_ffn_ln: their chunk loops carry weight fragments in registers
    across iterations, the pattern hipcc 7.2 miscompiled once, so each instantiation is executed."""
    from fastfourierdiffusion_amd import _native as N

    d, H, L = shape
    C, NL, B = 2, 2, 5
    c = dict(kind="transformer", d=d, H=H, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=700 + d + L)
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 9100 + d)))
    t = torch.full((B,), 0.35, dtype=torch.float32)
    ref = O.score_forward(x, t, sd, NL, H)
    lib = N.lib()
    outs = {}
    try:
        for name, (sp, mp) in {"large": (0, 0), "pair16": (1, 0), "part2": (0, 2), "part4": (0, 4), "part8": (0, 8)}.items():
            assert lib.ffd_tune(b"small_path", sp) == 0 and lib.ffd_tune(b"mid_path", mp) == 0
            outs[name] = m(batch_of(x.cuda(), 0.35)).cpu()
    finally:
        lib.ffd_tune(b"small_path", 1)
        lib.ffd_tune(b"mid_path", 1)
    for name, o in outs.items():
        assert rel_err(o, ref) < TOL_SCORE, name
        assert rel_err(o, outs["large"]) < 2e-6, name


# ------------------------------------------------------------------ round 4 ----
@pytest.mark.parametrize("c", cases.ROUND4_TRAJ_CASES, ids=lambda c: c["name"])
def test_round4_traj_golden(ffd, golden, c):
    """G13, pinned against the unmodified reference: BASELINE configs[3] at its full length (NASA charge, LSTM backbone,
    1000 steps, on the production selection k_lstm_wave), the reference's class-default transformer (d_model 60,
    score_models.py:31-33) at the ECG length with and without the cache, and a batch of the reference's default
    sample_batch_size = 50 (cmd/conf/sampler/default.yaml:3) with the cache on."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    g = golden["g13_round4"]
    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    _pin_grid(sch, g[c["name"] + "_ts"], N)
    sampler = DiffusionSampler(m, B, use_cache=c["use_cache"], cache_kwargs=dict(c.get("cache_kwargs", {})), z_chunk_steps=64)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), max(1, c["num_samples"] // B) * (N + 1), c["zseed"]))
    out = sampler.sample(c["num_samples"], N)
    assert tuple(out.shape) == g[c["name"]].shape
    err = rel_err(out, g[c["name"]])
    assert err < TOL_TRAJ, err


@pytest.mark.parametrize("shared", [False, True], ids=["one_unit_per_workgroup", "time_shared_units"])
def test_lstm_wavefront_timeout_is_an_error(ffd, shared):
    """k_lstm_wave's waits on progress words are bounded in time, and a wait that runs out is an ERROR (never a
    fall-through onto stale rows): with one unit's publications withheld (test knob) the launch must drain, the next
    libffd call / ffd_async_status must fail with FFD_ERR_STATE, and the context must work again afterwards."""
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd._native import FFDError

    c = next(c for c in cases.MODEL_CASES if c["name"] == "nasa_lstm")
    m, _ = make_model(ffd, c)
    lib = N.lib()
    B = 37
    x = torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 4500 + B))).cuda()
    good = m(batch_of(x, 0.45)).cpu()
    ctx = m._ctx()
    assert lib.ffd_async_status(ctx.handle) == 0
    if shared:  # (tile, layer) pairs outnumber the workgroups: units of 16 cell steps, state handed over through memory
        assert lib.ffd_tune(b"lstm_wave_per", 2) == 0 and lib.ffd_tune(b"lstm_wave_chunk", 16) == 0
        assert torch.equal(m(batch_of(x, 0.45)).cpu(), good)
    assert lib.ffd_tune(b"lstm_wave_spin_ms", 20) == 0 and lib.ffd_tune(b"lstm_wave_fault", 1) == 0
    t0 = time.time()
    bad = m(batch_of(x, 0.45))  # enqueued; unit 0 = (chunk 0, layer 0, tile 0) never publishes
    torch.cuda.synchronize()
    assert time.time() - t0 < 5.0, "the launch must drain after the first time-out"
    del bad
    assert lib.ffd_tune(b"lstm_wave_fault", 0) == 0
    rc = lib.ffd_async_status(ctx.handle)
    assert rc == -3, rc  # FFD_ERR_STATE
    msg = lib.ffd_last_error(ctx.handle).decode()
    assert "k_lstm_wave" in msg and "invalid" in msg, msg
    assert lib.ffd_async_status(ctx.handle) == 0  # reported once
    # the same failure surfaces at the next entry point when nobody asks
    assert lib.ffd_tune(b"lstm_wave_fault", 1) == 0
    m(batch_of(x, 0.45))
    torch.cuda.synchronize()
    assert lib.ffd_tune(b"lstm_wave_fault", 0) == 0
    with pytest.raises(FFDError, match="k_lstm_wave"):
        m(batch_of(x, 0.45))
    # ... and the context is fine afterwards
    assert torch.equal(m(batch_of(x, 0.45)).cpu(), good)
    assert lib.ffd_async_status(ctx.handle) == 0


def test_failed_workspace_growth_leaves_no_stale_capacity(ffd):
    """A device allocation that fails while a workspace grows (injected: ffd_tune "fail_alloc_after") must come back as
    FFD_ERR_NOMEM and leave the context usable: the capacity that guards the freed buffer reads 0, so the retry -- at
    the same or a smaller batch -- allocates again instead of launching on a null / freed pointer."""
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd._native import FFDError

    lib = N.lib()
    for name in ("small", "small_lstm"):
        c = next(c for c in cases.MODEL_CASES if c["name"] == name)
        m, _ = make_model(ffd, c)
        x = torch.from_numpy(next(synthetic.noise_stream((40, c["L"], c["C"]), 1, 7100))).cuda()
        small = m(batch_of(x[:3], 0.5)).cpu()
        for nth in (1, 2, 3, 4):  # the n-th allocation of the growth to B = 40 fails
            assert lib.ffd_tune(b"fail_alloc_after", nth) == 0
            try:
                out = m(batch_of(x, 0.5)).cpu()  # (fewer than nth allocations were needed: the call succeeds)
            except FFDError as e:
                assert "injected" in str(e), e
                out = None
            assert lib.ffd_tune(b"fail_alloc_after", 0) == 0
            assert torch.equal(m(batch_of(x[:3], 0.5)).cpu(), small), (name, nth)
            full = m(batch_of(x, 0.5)).cpu()
            assert torch.isfinite(full).all() and rel_err(full[:3], small) < 2e-6, (name, nth)
            if out is not None:
                assert torch.equal(out, full)
            m, _ = make_model(ffd, c)  # a fresh context for the next injection point
            small = m(batch_of(x[:3], 0.5)).cpu()


# ------------------------------------------------------- the channel axis (g15) ----
# The kernels choose their code path by the channel count C (csrc/ffd_elem.hip, ffd_api.hip, ffd_fft.hip):
#   embedding    C <= 8: k_embed_reg (float4 x rows only at C = 4 / 8 with 16-B aligned X) | C > 8: k_embed (the
#                transposed weight staged in LDS)
#   unembedding  C <= 16: k_unembed_mfma, lane quad q = 0 .. 3 carries channels 4q .. 4q + 3, float4 stores where
#                C % 4 == 0, scalar ones otherwise | C > 16: k_unembed (16 lanes per row, weight in LDS)
#   sampling     C <= 16: the step is k_unembed_mfma's tail (TailSde), quad or scalar Philox draws | C > 16:
#                k_step_v4<OpSde> (C % 4 == 0) or k_step<OpSde> behind the unembedding
def _channel_branches(C):
    embed = ("reg_xvec" if C in (4, 8) else "reg") if C <= 8 else "lds"
    if C <= 16:
        return f"C{C}-embed_{embed}-unembed_mfma_q{(C - 1) // 4}_{'quad' if C % 4 == 0 else 'scalar'}-fused_tail"
    return f"C{C}-embed_{embed}-unembed_generic-{'sde_step_v4' if C % 4 == 0 else 'sde_step'}"


def _fft_channel_group(L, C):
    """Channels per workgroup of the non-power-of-two FFT kernels (launch_dft / slab_geom): halved until the twiddle
    table and two complex (L x CG) slabs fit in 64 KiB of LDS."""
    CG = C
    while CG > 1 and (L + 2 * L * CG) * 8 > 64 * 1024:
        CG = (CG + 1) // 2
    return CG


def _cached_seq_vs_oracle(m, sd, c, B, tv, seed):
    """FULL -> PURE -> MIXED against the oracle's KV table."""
    L, C = c["L"], c["C"]
    m.enable_caching()
    m.cache.reset()
    table = O.KVTable(c["NL"], L)
    t = torch.full((B,), tv, dtype=torch.float32)
    for j, n in enumerate([L, 0, min(10, L - 1)]):
        xj = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, seed + j)))
        ref = O.score_forward(xj, t, sd, c["NL"], c["H"], table, list(range(n)))
        got = m(batch_of(xj.cuda(), tv), recompute_tokens=set(range(n)), step=j)
        assert rel_err(got.cpu(), ref) < TOL_SCORE, (j, n)
    m.disable_caching()


@pytest.mark.parametrize("c", cases.DATASET_MODEL_CASES, ids=lambda c: f"{c['name']}-{_channel_branches(c['C'])}")
def test_dataset_model_golden(ffd, golden, c, variant):
    """G15: the NASDAQ (252 x 5), MIMIC-III (24 x 40) and US-droughts (365 x 13) shapes with the reference's default
    transformer and its LSTM, against the unmodified reference's scores; the transformer's cached modes against the
    oracle at the same shapes."""
    g = golden["g15_datasets"]
    m, _ = make_model(ffd, c)
    B, L, C = c["B"], c["L"], c["C"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, c["xseed"]))).cuda()
    for tv in c["t_values"]:
        assert rel_err(m(batch_of(x, tv)).cpu(), g[f"{c['name']}_score_t{tv}"]) < TOL_SCORE, tv
    if c["kind"] == "lstm":
        if variant == "auto":  # the per-layer LSTM kernels at L = 24 / 252 / 365 as well
            from fastfourierdiffusion_amd import _native as N

            assert N.lib().ffd_tune(b"lstm_wave", 0) == 0
            for tv in c["t_values"]:
                assert rel_err(m(batch_of(x, tv)).cpu(), g[f"{c['name']}_score_t{tv}"]) < TOL_SCORE, tv
        return
    _cached_seq_vs_oracle(m, make_sd(c), c, B, c["t_values"][0], c["xseed"] + 100)


@pytest.mark.parametrize("c", cases.DATASET_TRAJ_CASES, ids=lambda c: f"{c['name']}-{_channel_branches(c['C'])}")
def test_dataset_traj_golden(ffd, golden, c):
    """G15 trajectories with injected noise: the sampling tail at C = 5 / 13 (unembedding fused into the step kernel,
    scalar draws) and C = 40 (k_unembed + k_step_v4<OpSde>), against the unmodified reference."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    g = golden["g15_datasets"]
    m, sch = make_model(ffd, c)
    B, L, C, N = c["B"], c["L"], c["C"], c["N"]
    _pin_grid(sch, g[c["name"] + "_ts"], N)
    sampler = DiffusionSampler(m, B, use_cache=c["use_cache"], cache_kwargs=dict(c.get("cache_kwargs", {})),
                               z_chunk_steps=16)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), max(1, c["num_samples"] // B) * (N + 1), c["zseed"]))
    out = sampler.sample(c["num_samples"], N)
    assert tuple(out.shape) == g[c["name"]].shape
    err = rel_err(out, g[c["name"]])
    assert err < TOL_TRAJ, err
    if c["use_cache"]:
        m.disable_caching()


@pytest.mark.parametrize("strategy", ["energy", "spatial"])
def test_droughts_fresca_trajectory_vs_oracle(ffd, strategy):
    """FreSca in every step at the droughts shape: the score goes through the generic FFT in two channel groups
    (7 + 6 of 13) and the unfused k_step<OpSde> (C % 4 != 0), against the oracle's sampler on the same draws."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = next(c for c in cases.DATASET_MODEL_CASES if c["name"] == "droughts_tf")
    assert _fft_channel_group(c["L"], c["C"]) == 7
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    B, L, C, N = 2, c["L"], c["C"], 12
    fk = dict(low_scale=0.9, high_scale=1.4, cutoff_ratio=0.45, cutoff_strategy=strategy)
    sampler = DiffusionSampler(m, B, use_fresca=True, fresca_low_scale=fk["low_scale"], fresca_high_scale=fk["high_scale"],
                               fresca_cutoff_ratio=fk["cutoff_ratio"], fresca_cutoff_strategy=strategy)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), N + 1, 187))
    out = sampler.sample(B, N)
    noise = (torch.from_numpy(z) for z in synthetic.noise_stream((B, L, C), N + 1, 187))
    ref = O.sample(sd, kind="transformer", n_channels=C, max_len=L, num_layers=c["NL"], n_head=c["H"], sde="vp",
                   sde_kwargs=cases.VP, fourier_noise_scaling=True, num_samples=B, batch_size=B, num_steps=N, noise=noise,
                   fresca_kwargs=fk)
    assert rel_err(out, ref) < 2 * TOL_TRAJ, rel_err(out, ref)  # (the tolerance of the sampler option matrix)


# C: the first value past each threshold (8 -> 9, 16 -> 17) and every C % 4 on both sides of 8 and of 16
_SWEEP_C = [5, 6, 7, 9, 12, 13, 15, 16, 17, 24, 40]
_SWEEP_MODELS = [dict(kind="transformer", d=24, H=4, NL=2, L=23), dict(kind="transformer", d=72, H=12, NL=2, L=37),
                 dict(kind="lstm", d=24, H=1, NL=2, L=29)]


@pytest.mark.parametrize("C", _SWEEP_C, ids=_channel_branches)
@pytest.mark.parametrize("base", _SWEEP_MODELS, ids=lambda b: f"{b['kind']}_d{b['d']}L{b['L']}")
def test_channel_sweep_vs_oracle(ffd, base, C, variant):
    """Every channel-count branch of the embedding, the unembedding and the sampling tail (see _channel_branches)
    against the oracle: the score forward, the cached FULL -> PURE -> MIXED sequence (transformers), and with the
    default kernels a short injected-noise trajectory (prior + 4 steps, two batches) through the sampling tail."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = dict(base, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=700 + 3 * C + base["d"] + base["L"])
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    B, L, NL = 3, c["L"], c["NL"]
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 7100 + C)))
    t = torch.full((B,), 0.65, dtype=torch.float32)
    ref = O.lstm_score_forward(x, t, sd, NL) if c["kind"] == "lstm" else O.score_forward(x, t, sd, NL, c["H"])
    assert rel_err(m(batch_of(x.cuda(), 0.65)).cpu(), ref) < TOL_SCORE
    if c["kind"] != "lstm":
        _cached_seq_vs_oracle(m, sd, c, B, 0.65, 7200 + C)
    if variant != "auto":
        return
    N, ns = 4, 2 * B
    sampler = DiffusionSampler(m, B)
    sampler.inject_noise(synthetic.noise_stream((B, L, C), 2 * (N + 1), 7300 + C))
    out = sampler.sample(ns, N)
    noise = (torch.from_numpy(z) for z in synthetic.noise_stream((B, L, C), 2 * (N + 1), 7300 + C))
    ref = O.sample(sd, kind=c["kind"], n_channels=C, max_len=L, num_layers=NL, n_head=c["H"], sde="vp",
                   sde_kwargs=cases.VP, fourier_noise_scaling=True, num_samples=ns, batch_size=B, num_steps=N, noise=noise)
    assert rel_err(out, ref) < TOL_TRAJ, rel_err(out, ref)


# (name, model, sample offset): C = 5 / 13 take the fused tail with scalar stores and draws at an element offset
# elem_off = offset * L * C with elem_off % 4 != 0 (115 % 4 = 3; 4745 % 4 = 1); C = 16 takes it with float4 quads in all
# four lane quads; C = 40 has no fused form (k_unembed + k_step_v4<OpSde>)
_TAIL_CASES = [
    ("C5_L23_off1", dict(kind="transformer", d=24, H=4, NL=2, L=23, C=5), 1),
    ("C13_L365_off1", dict(kind="transformer", d=72, H=12, NL=2, L=365, C=13), 1),
    ("C16_L20_off3", dict(kind="lstm", d=24, H=1, NL=2, L=20, C=16), 3),
    ("C40_L24_off1", dict(kind="transformer", d=72, H=12, NL=2, L=24, C=40), 1),
]


@pytest.mark.parametrize("name,base,off", _TAIL_CASES, ids=[t[0] for t in _TAIL_CASES])
def test_fused_tail_at_dataset_channel_counts(ffd, name, base, off):
    """The fused unembedding + SDE step equals the two-kernel tail bit for bit at C = 5 / 13 / 16, with on-device
    Philox draws at an unaligned element offset and with injected draws; at C = 40 the fused form is not planned.
    Every form agrees with the oracle's steps on the injected draws."""
    import ctypes as Ct

    from fastfourierdiffusion_amd import _native as N

    c = dict(base, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=800 + base["C"])
    m, sch = make_model(ffd, c)
    sd = make_sd(c)
    ctx = m._ctx()
    B, L, Cn, n_steps, first, n_run = 3, c["L"], c["C"], 20, 2, 4
    assert (Cn % 4 == 0) or (off * L * Cn) % 4 != 0
    sch.set_timesteps(n_steps)
    ts_c = (Ct.c_float * n_steps)(*sch.timesteps.tolist())
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 81)))
    zs = torch.from_numpy(np.stack(list(synthetic.noise_stream((B, L, Cn), n_run, 82))))
    s = N.current_stream_ptr(torch.device("cuda"))
    fl, by = Ct.c_double(), Ct.c_double()
    res = {}
    try:
        for fuse in (1, 0):
            assert ctx.lib.ffd_tune(b"fuse_tail", fuse) == 0
            kname = ctx.lib.ffd_kernel_work(ctx.handle, N.K_SDE, B, 0, Ct.byref(fl), Ct.byref(by))
            assert kname.startswith(b"k_unembed_mfma") == bool(fuse and Cn <= 16), kname
            for z in (None, zs.cuda()):
                x = x0.cuda()
                N.check(ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), B, ts_c, n_steps, float(sch.step_size), first,
                                                 n_run, 9, off, z.data_ptr() if z is not None else None, 0, 0, s),
                        ctx.handle, "sample")
                res[(fuse, z is None)] = x.cpu()
    finally:
        ctx.lib.ffd_tune(b"fuse_tail", 1)
    for philox in (True, False):
        assert torch.isfinite(res[(1, philox)]).all()
        assert torch.equal(res[(1, philox)], res[(0, philox)]), philox
    assert not torch.equal(res[(1, True)], res[(1, False)])
    G = O.noise_scaling(L, True)
    ts = sch.timesteps.cpu()
    x = x0.clone()
    for j in range(n_run):
        tv = ts[first + j].item()
        t = torch.full((B,), tv, dtype=torch.float32)
        score = O.lstm_score_forward(x, t, sd, c["NL"]) if c["kind"] == "lstm" else O.score_forward(x, t, sd, c["NL"], c["H"])
        x = O.vp_step(x, score, zs[j], tv, G, ts[0] - ts[1], **cases.VP)
    assert rel_err(res[(1, False)], x) < TOL_TRAJ, rel_err(res[(1, False)], x)


@pytest.mark.parametrize("L,C", [(365, 13), (24, 40)], ids=["L365_C13_fused_scalar_draws", "L24_C40_sde_step_v4"])
def test_philox_shards_at_dataset_channel_counts(ffd, L, C):
    """Philox draws are keyed by the global element index: uneven shards at odd sample offsets (elem_off % 4 = 1 and 3
    at C = 13) reproduce the whole batch bit for bit.  The LSTM backbone keeps every shard's forward arithmetic that of
    the whole batch (one 16-sample tile, per-row kernels), so any difference is the noise indexing."""
    import ctypes as Ct

    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = dict(kind="lstm", d=24, H=1, NL=2, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=900 + C)
    m, _ = make_model(ffd, c)
    fl, by = Ct.c_double(), Ct.c_double()
    ctx = m._ctx()
    kname = ctx.lib.ffd_kernel_work(ctx.handle, N.K_SDE, 7, 0, Ct.byref(fl), Ct.byref(by))
    assert kname.startswith(b"k_unembed_mfma") == (C <= 16), kname
    B, Nst = 7, 10

    def run(bs, off):
        return DiffusionSampler(m, bs, rng="philox", seed=23, sample_offset=off).sample(bs, Nst)

    full = run(B, 0)
    assert torch.isfinite(full).all()
    shards = torch.cat([run(1, 0), run(2, 1), run(4, 3)])
    assert torch.equal(shards, full)
    assert not torch.equal(run(4, 2), full[3:])  # a wrong offset draws other noise


_GROUPED_FFT = [(2, 365, 13), (3, 252, 5), (2, 24, 40), (2, 509, 9), (1, 187, 41)]


@pytest.mark.parametrize("shape", _GROUPED_FFT,
                         ids=lambda s: f"B{s[0]}L{s[1]}C{s[2]}-cg{_fft_channel_group(s[1], s[2])}")
def test_generic_fft_channel_groups_vs_oracle(ffd, shape):
    """Non-power-of-two lengths at the dataset shapes.  365 x 13, 509 x 9 and 187 x 41 exceed one workgroup's 64 KiB
    LDS slab and run in channel groups of 7 + 6, 5 + 4 and 21 + 20 (grid .y = 2): dft / idft, FreSca (both cutoffs),
    the frequency decomposition and the standardising wrappers against the fp64 oracle."""
    from fastfourierdiffusion_amd.utils.fourier import dft, dft_standardize, frequency_decompose_fft, idft, unstandardize_idft
    from fastfourierdiffusion_amd.utils.fresca import apply_fresca_to_score

    B, L, C = shape
    CG = _fft_channel_group(L, C)
    if (L, C) in ((365, 13), (509, 9), (187, 41)):
        assert CG < C and C % CG != 0, CG  # grouped, with an uneven last group
    else:
        assert CG == C
    x, mean, std = (torch.from_numpy(a) for a in synthetic.noise_stream((B, L, C), 3, 1300 + L + C))
    mean, std = mean[0], std[0].abs() + 0.5
    assert rel_err(dft(x.cuda()).cpu(), O.dft(x)) < TOL_OP
    assert rel_err(idft(x.cuda()).cpu(), O.idft(x)) < TOL_OP
    for strat in ("energy", "spatial"):
        y = apply_fresca_to_score(x.cuda(), low_scale=0.9, high_scale=1.4, cutoff_ratio=0.45, cutoff_strategy=strat)
        assert rel_err(y.cpu(), O.fresca(x, 0.9, 1.4, 0.45, strat, None, None)) < TOL_OP, strat
    lo, hi = frequency_decompose_fft(x.cuda(), 0.3)
    olo, ohi = O.frequency_decompose(x, 0.3)
    assert rel_err(lo.cpu(), olo) < TOL_OP and rel_err(hi.cpu(), ohi) < TOL_OP
    assert rel_err(unstandardize_idft(x.cuda(), mean, std).cpu(), O.unstandardize_idft(x, mean, std)) < TOL_OP
    assert rel_err(dft_standardize(x.cuda(), mean, std).cpu(), O.dft_standardize(x, mean, std)) < TOL_OP


def _misaligned(x, off):
    """A contiguous device copy of x at storage offset `off` floats: data_ptr() % 16 == 4 * off."""
    buf = torch.zeros(x.numel() + 4, device="cuda")
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("off", [1, 2, 3])
def test_misaligned_inputs_equal_aligned(ffd, off):
    """X not 16-B aligned turns off the float4 x loads of the embedding (C = 4 / 8) and the float4 slab I/O of the
    power-of-two FFT / FreSca kernels.  Those paths read and write the same values in another width and do the same
    arithmetic (the FFT's shape-specialised 512 x 8 instance runs the same passes with the shape as a constant), so
    the results are bit-identical; L = 187 (no float4 path) is the control.  Each also agrees with the oracle."""
    from fastfourierdiffusion_amd.utils.fourier import dft, idft
    from fastfourierdiffusion_amd.utils.fresca import apply_fresca_to_score

    for C, kind in ((4, "transformer"), (8, "transformer"), (8, "lstm")):
        c = dict(kind=kind, d=72, H=12, NL=2, L=50, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=1400 + C)
        m, _ = make_model(ffd, c)
        sd = make_sd(c)
        x = torch.from_numpy(next(synthetic.noise_stream((3, 50, C), 1, 1450 + C)))
        a = m(batch_of(x.cuda(), 0.4))
        b = m(batch_of(_misaligned(x.cuda(), off), 0.4))
        assert torch.equal(a, b), (C, kind)
        t = torch.full((3,), 0.4, dtype=torch.float32)
        ref = O.lstm_score_forward(x, t, sd, 2) if kind == "lstm" else O.score_forward(x, t, sd, 2, 12)
        assert rel_err(b.cpu(), ref) < TOL_SCORE, (C, kind)
    for L, C in ((512, 4), (512, 8), (187, 4)):
        x = torch.from_numpy(next(synthetic.noise_stream((2, L, C), 1, 1500 + L + C)))
        xa = x.cuda()
        xm = _misaligned(xa, off)
        for fn, oracle in ((dft, O.dft), (idft, O.idft)):
            ya, ym = fn(xa), fn(xm)
            assert torch.equal(ya, ym), (L, C, fn.__name__)
            assert rel_err(ym.cpu(), oracle(x)) < TOL_OP
        for strat in ("energy", "spatial"):
            ya = apply_fresca_to_score(xa, low_scale=0.9, high_scale=1.4, cutoff_ratio=0.45, cutoff_strategy=strat)
            ym = apply_fresca_to_score(xm, low_scale=0.9, high_scale=1.4, cutoff_ratio=0.45, cutoff_strategy=strat)
            assert torch.equal(ya, ym), (L, C, strat)
            assert rel_err(ym.cpu(), O.fresca(x, 0.9, 1.4, 0.45, strat, None, None)) < TOL_OP, (L, C, strat)
