"""GPU tests of class-conditional score models and classifier-free guidance (csrc/ffd_class.hip, the context state in
csrc/ffd_api.hip, the training path in csrc/ffd_train.hip, and the Python surface) against the float64 judge of
tests/class_restatement.py: the oracle's own forwards on a one-hot label block.

Bars are the project's: operators, forwards and gradients max(2e-6, 3 x the error of the same arithmetic in fp32 on the
CPU), relative to the expected array's max-norm and measured inside the test; trajectories the same form with the 1e-5
trajectory floor.  3 classes; the labels of a batch cover every class, a repeat, -1 and n_classes (a batch of 3 over its
two label variants).  Shapes: the two transformer shapes of the training tests (L 5 C 1 d 8 H 2 F 64 NL 2 B 3; L 17 C 3
d 60 H 12 F 128 NL 2 B 5: an odd batch, 2 B = 10, B L C = 255 no multiple of 4), the LSTM at the smallest d_model with a
kernel (8) and the MLP toy's network."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

import class_restatement as CL
import cond_restatement as CR
import multistep_restatement as MS
import ode_restatement as R
import pc_restatement as PCR
import resample_restatement as RS
import train_restatement as TR
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic

pytestmark = pytest.mark.gpu

NC = CL.N_CLASSES
GRID, SNR, SEED = 6, 0.16, 11
JUMP, RESAMPLE = 2, 2
MODELS = {
    "tf_d8": dict(kind="transformer", L=5, C=1, d=8, H=2, F=64, NL=2, B=3),
    "tf_d60": dict(kind="transformer", L=17, C=3, d=60, H=12, F=128, NL=2, B=5),
    "lstm_d8": dict(kind="lstm", L=7, C=3, d=8, H=1, F=0, NL=2, B=5),
    "mlp_toy": dict(kind="mlp", L=TR.TOY["L"], C=TR.TOY["C"], d=TR.TOY["d"], H=1, F=TR.TOY["F"], NL=TR.TOY["NL"], B=5),
    # the partition test's shape (tests/test_partition_gpu.py "d24_B5"): eligible for two CU partitions under its knobs
    "tf_d24": dict(kind="transformer", L=24, C=3, d=24, H=4, F=2048, NL=2, B=5),
}
D24_KNOBS = {"ffn_mb": 1, "rows_slices": -1, "small_path": 0, "mid_path": 0, "ffn_height": 0, "attn_small": 0}
FRESCA = dict(low_scale=0.9, high_scale=1.2, cutoff_ratio=0.4, cutoff_strategy="spatial")


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


@pytest.fixture(autouse=True)
def _tune_defaults():
    from fastfourierdiffusion_amd import _native

    yield
    _native.lib().ffd_tune(b"reset", 0)


def N_():
    from fastfourierdiffusion_amd import _native

    return _native


def stream():
    return N_().current_stream_ptr(torch.device("cuda"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(what, got, want, e32, floor=CL.FLOOR_OP):
    err, tol = rel_err(got, want), CL.bar(e32, floor)
    print(f"{what}: err {err:.2e} fp32-cpu {e32:.2e} bar {tol:.2e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err


# ------------------------------------------------------------------------------------------------------ operators ----
@pytest.mark.parametrize("d", [8, 60])
def test_class_temb_against_float64(lib, d):
    B = 5
    rng = np.random.default_rng(d)
    temb, table = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((NC + 1, d)).astype(np.float32)
    dt, dtab = dev(temb), dev(table)
    for variant in (0, 1):
        y = CL.labels_for(B, variant)
        dy = dev(y)
        for stride, stack in ((d, 0), (d, 1), (0, 0), (0, 1)):
            out = torch.full(((2 if stack else 1) * B, d), np.nan, device="cuda")
            assert lib.ffd_class_temb(dt.data_ptr(), stride, dtab.data_ptr(), NC, dy.data_ptr(), B, d, stack, out.data_ptr(),
                                      stream()) == 0
            src = temb if stride else temb[0]
            want = CL.class_temb(src, stride, table, y, B, stack)
            check(f"class_temb stride {stride} stack {stack}", out.cpu().numpy(), want,
                  rel_err(CL.class_temb(src, stride, table, y, B, stack, np.float32), want))
    # no labels: every row null; in place on a per-sample table
    out = torch.empty(B, d, device="cuda")
    assert lib.ffd_class_temb(dt.data_ptr(), d, dtab.data_ptr(), NC, None, B, d, 0, out.data_ptr(), stream()) == 0
    assert np.array_equal(out.cpu().numpy(), CL.class_temb(temb, d, table, None, B, 0, np.float32))
    y = dev(CL.labels_for(B))
    ref = torch.empty(B, d, device="cuda")
    assert lib.ffd_class_temb(dt.data_ptr(), d, dtab.data_ptr(), NC, y.data_ptr(), B, d, 0, ref.data_ptr(), stream()) == 0
    inplace = dt.clone()
    assert lib.ffd_class_temb(inplace.data_ptr(), d, dtab.data_ptr(), NC, y.data_ptr(), B, d, 0, inplace.data_ptr(), stream()) == 0
    assert torch.equal(inplace, ref)


@pytest.mark.parametrize("n", [1, 3, 255, 1024, 4099])
def test_cfg_combine_against_float64_at_every_alignment(lib, n):
    """n % 4 != 0, pointers that are only 4-byte aligned, equal and different 16-byte phases of c and u: the same bits."""
    rng = np.random.default_rng(n)
    c, u = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    for g in (2.5, -1.0, 0.0, 1.0):
        want = CL.cfg_combine(c, u, g)
        e32 = rel_err(CL.cfg_combine(c, u, g, np.float32), want)
        outs = []
        for oc, ou in ((0, 0), (1, 1), (3, 3), (1, 2), (0, 3)):  # offsets in floats from a 256-byte aligned base
            bc, bu = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
            vc, vu = bc[oc:oc + n], bu[ou:ou + n]
            vc.copy_(dev(c)), vu.copy_(dev(u))
            assert vc.data_ptr() % 16 == 4 * oc and vu.data_ptr() % 16 == 4 * ou
            assert lib.ffd_cfg_combine(vc.data_ptr(), vu.data_ptr(), g, n, stream()) == 0
            assert torch.equal(vu.cpu(), torch.from_numpy(u)) and not bc[oc + n:].any() and not bc[:oc].any()
            outs.append(vc.cpu().numpy().copy())
        check(f"cfg_combine n={n} g={g}", outs[0], want, e32)
        assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    if n == 255:  # a prefix's elements do not depend on the length
        a, b = dev(c), dev(c)
        du = dev(u)
        assert lib.ffd_cfg_combine(a.data_ptr(), du.data_ptr(), 2.5, n, stream()) == 0
        assert lib.ffd_cfg_combine(b.data_ptr(), du.data_ptr(), 2.5, 101, stream()) == 0
        assert torch.equal(a[:101], b[:101]) and torch.equal(b[101:].cpu(), torch.from_numpy(c[101:]))


@pytest.mark.parametrize("p", [0.0, 0.1, 1.0])
def test_class_drop_element_by_element(lib, p):
    n, B = 40, 9
    labels = CL.labels_for(n)
    dl = dev(labels)
    for offset in (0, 2, 4097):  # 2: rows 2 .. 10 cross a Philox block (4 rows per block) twice
        out = torch.full((B,), -7, device="cuda", dtype=torch.int32)
        assert lib.ffd_class_drop(dl.data_ptr(), NC, None, B, p, SEED, offset, out.data_ptr(), stream()) == 0
        assert np.array_equal(out.cpu().numpy(), CL.class_drop(labels, NC, None, B, p, SEED, offset))
        idx = np.array([5, 0, 39, 17, 5, 3, 38, 1, 2], np.int64)
        di = dev(idx)
        assert lib.ffd_class_drop(dl.data_ptr(), NC, di.data_ptr(), B, p, SEED, offset, out.data_ptr(), stream()) == 0
        assert np.array_equal(out.cpu().numpy(), CL.class_drop(labels, NC, idx, B, p, SEED, offset))
    big = torch.empty(20000, device="cuda", dtype=torch.int32)
    many = dev((np.arange(20000) % NC).astype(np.int32))
    assert lib.ffd_class_drop(many.data_ptr(), NC, None, 20000, p, SEED, 0, big.data_ptr(), stream()) == 0
    rate = float((big == NC).float().mean())
    assert abs(rate - p) <= 4 * np.sqrt(max(p * (1 - p), 1e-12) / 20000), (p, rate)
    assert lib.ffd_class_drop(None, NC, None, B, p, SEED, 0, out.data_ptr(), stream()) == 0 and bool((out == NC).all())


@pytest.mark.parametrize("d", [8, 60])
def test_class_table_grad_against_float64(lib, d):
    B = 37
    rng = np.random.default_rng(100 + d)
    dtemb = rng.standard_normal((B, d)).astype(np.float32)
    dd = dev(dtemb)
    cases_ = {"every class": CL.labels_for(B), "class 1 absent": np.where(CL.labels_for(B) == 1, 2, CL.labels_for(B)),
              "all null": np.where(np.arange(B) % 2 == 0, -1, NC).astype(np.int32)}
    for what, y in cases_.items():
        out = torch.full((NC + 1, d), np.nan, device="cuda")
        assert lib.ffd_class_table_grad(dd.data_ptr(), dev(y.astype(np.int32)).data_ptr(), NC, B, d, out.data_ptr(), stream()) == 0
        want = CL.table_grad(dtemb, y, NC)
        got = out.cpu().numpy()
        check(f"table_grad {what}", got, want, rel_err(CL.table_grad(dtemb, y, NC, np.float32), want))
        absent = [c for c in range(NC + 1) if not (CL.effective(y, NC) == c).any()]
        assert all(not got[c].any() for c in absent) and (what == "every class") == (not absent)


# ------------------------------------------------------------------------------------------------------- networks ----
@functools.lru_cache(maxsize=None)
def net(name, sde="vp", bias_shift_seed=None):
    """The model on the device with its context, its weights for the judge, the grid and a table of std 0.3.
    bias_shift_seed: the same network with a fixed vector v added to time_encoder.dense.bias (``.v``)."""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule

    c = MODELS[name]
    sch = TR.scheduler(sde, c["L"])
    common = dict(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"])
    if c["kind"] == "lstm":
        m = LSTMScoreModule(**common)
        sd = synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=146)
    elif c["kind"] == "mlp":
        m = MLPScoreModule(d_mlp=c["F"], **common)
        sd = synthetic.mlp_state_dict(c["C"], c["L"], c["d"], c["F"], c["NL"], seed=149)
    else:
        m = ScoreModule(n_head=c["H"], **common)
        if c["F"] != m.dim_feedforward:
            for layer in m.backbone.layers:
                layer.linear1, layer.linear2 = torch.nn.Linear(c["d"], c["F"]), torch.nn.Linear(c["F"], c["d"])
            m.dim_feedforward = c["F"]
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], dim_feedforward=c["F"], seed=142)
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    v = None
    if bias_shift_seed is not None:
        v = (0.3 * np.random.default_rng(bias_shift_seed).standard_normal(c["d"])).astype(np.float32)
        sd["time_encoder.dense.bias"] = sd["time_encoder.dense.bias"] + torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    sch.set_timesteps(GRID)
    ts = sch.timesteps.to(torch.float32).numpy().copy()
    table = CL.make_table(NC, c["d"], 7, std=0.3)
    return types.SimpleNamespace(c=c, name=name, sde=sde, kw=TR.SDE_KW[sde], model=m, ctx=m._ctx(), sd=sd, sch=sch,
                                 G=sch.G.numpy().copy(), ts=ts, ts_c=(C.c_float * GRID)(*ts.tolist()), h=float(sch.step_size),
                                 table=table, table_dev=dev(table), v=v, keep=None)


def enable(n, labels, g=1.0, table=None):
    N = N_()
    tab = n.table_dev if table is None else table
    host = None if labels is None else np.ascontiguousarray(labels, np.int32)
    y = None if host is None else dev(host)
    cfg = N.ClassCfg(tab.data_ptr(), y.data_ptr() if y is not None else None, host.ctypes.data if host is not None else None, NC,
                     len(host) if host is not None else 0, g, 0)
    N.check(n.ctx.lib.ffd_class_enable(n.ctx.handle, C.byref(cfg)), n.ctx.handle, "ffd_class_enable")
    n.keep = (tab, y)  # the library reads both live


def disable(n):
    assert n.ctx.lib.ffd_class_disable(n.ctx.handle) == 0
    n.keep = None


def forward_ts(n, x, t):
    out = torch.full_like(x, np.nan)
    N_().check(n.ctx.lib.ffd_score_forward_ts(n.ctx.handle, x.data_ptr(), t.data_ptr(), out.data_ptr(), None, x.shape[0], -1,
                                              stream()), n.ctx.handle, "ffd_score_forward_ts")
    return out


def forward_inputs(c, seed=5):
    rng = np.random.default_rng(seed + c["d"])
    return (rng.standard_normal((c["B"], c["L"], c["C"])).astype(np.float32), rng.uniform(0.05, 1.0, c["B"]).astype(np.float32))


FORWARD_NETS = ["tf_d8", "tf_d60", "lstm_d8", "mlp_toy"]


@pytest.mark.parametrize("sde", ["vp", "ve"])
@pytest.mark.parametrize("name", FORWARD_NETS)
def test_forward_against_the_float64_judge(lib, name, sde):
    n = net(name, sde)
    c = n.c
    x, t = forward_inputs(c)
    dx, dt = dev(x), dev(t)
    try:
        for variant in (0, 1):
            y = CL.labels_for(c["B"], variant)
            enable(n, y, g=7.0)  # (the forward entries take the conditional branch whatever the scale)
            got = forward_ts(n, dx, dt).cpu().numpy()
            want = CL.forward_np(c["kind"], x, t, n.sd, n.table, y, c["NL"], c["H"])
            e32 = rel_err(CL.forward_np(c["kind"], x, t, n.sd, n.table, y, c["NL"], c["H"], torch.float32), want)
            check(f"{name} {sde} forward, labels {y.tolist()}", got, want, e32)
        enable(n, None)
        null = forward_ts(n, dx, dt).cpu().numpy()
        want = CL.forward_np(c["kind"], x, t, n.sd, n.table, None, c["NL"], c["H"])
        check(f"{name} {sde} forward, no labels", null, want,
              rel_err(CL.forward_np(c["kind"], x, t, n.sd, n.table, None, c["NL"], c["H"], torch.float32), want))
        assert rel_err(got, null) > 1e-3  # the labels matter at this table
    finally:
        disable(n)


@pytest.mark.parametrize("name", FORWARD_NETS)
def test_forward_bit_identities_and_the_constant_table(lib, name):
    n = net(name)
    c = n.c
    x, t = forward_inputs(c)
    dx, dt = dev(x), dev(t)
    plain = forward_ts(n, dx, dt)
    y = CL.labels_for(c["B"], 1)
    try:
        # a zero table is the plain network at the same times
        enable(n, y, table=torch.zeros(NC + 1, c["d"], device="cuda"))
        assert torch.equal(forward_ts(n, dx, dt), plain)
        # a sample's row does not depend on the other samples' labels
        enable(n, y)
        mixed = forward_ts(n, dx, dt)
        assert not torch.equal(mixed, plain)
        for b in range(c["B"]):
            enable(n, np.full(c["B"], y[b], np.int32))
            assert torch.equal(forward_ts(n, dx, dt)[b], mixed[b]), b
        # a table whose rows all equal v is the network with v added to the time encoder's bias
        shifted = net(name, "vp", 77)
        enable(n, y, table=dev(np.tile(shifted.v, (NC + 1, 1))))
        got = forward_ts(n, dx, dt).cpu().numpy()
    finally:
        disable(n)
    other = forward_ts(shifted, dx, dt).cpu().numpy()
    want = CL.forward_np(c["kind"], x, t, shifted.sd, np.zeros_like(n.table), None, c["NL"], c["H"])
    e32 = rel_err(CL.forward_np(c["kind"], x, t, shifted.sd, np.zeros_like(n.table), None, c["NL"], c["H"], torch.float32), want)
    check(f"{name} constant table vs float64", got, want, e32)
    check(f"{name} constant table vs the shifted bias on the device", got, other, e32)


def test_validation_loss_takes_the_conditional_branch(lib):
    """ffd_sm_eval_batch with the state on: the per-sample losses of the judge's conditional score (injected z)."""
    n = net("tf_d60")
    c = n.c
    rng = np.random.default_rng(3)
    x0, z = (rng.standard_normal((c["B"], c["L"], c["C"])).astype(np.float32) for _ in range(2))
    t = rng.uniform(0.05, 1.0, c["B"]).astype(np.float32)
    mc, sigma = (v.numpy() for v in n.sch.marginal_coeffs(torch.from_numpy(t)))
    y = CL.labels_for(c["B"])
    out = torch.empty(c["B"], device="cuda", dtype=torch.float64)
    bufs = [dev(a) for a in (x0, t, mc, sigma, z)]
    enable(n, y, g=0.0)
    try:
        N_().check(lib.ffd_sm_eval_batch(n.ctx.handle, *[b.data_ptr() for b in bufs], 0, 0, 0, 1, out.data_ptr(), c["B"], stream()),
                   n.ctx.handle, "ffd_sm_eval_batch")
    finally:
        disable(n)

    def ref(dt):
        cast = lambda a: torch.as_tensor(a).to(dt)  # noqa: E731
        xn, std = TR.perturb(cast(x0), cast(z), cast(mc), cast(sigma), cast(n.G))
        with torch.no_grad():
            s = CL.forward(c["kind"], xn, cast(t), TR.cast(n.sd, dt), cast(n.table), y, c["NL"], c["H"], dt)
        return TR.per_sample_loss(s, cast(z), std, False).numpy()

    want = ref(torch.float64)
    check("per-sample validation loss", out.cpu().numpy(), want, rel_err(ref(torch.float32), want))


# ---------------------------------------------------------------------------------------------------------- loops ----
ENTRIES = ("em", "ode_euler", "ode_heun", "ode_ab2", "dpmpp_2m", "pc", "cond", "resample")
SOLVER = {"ode_euler": 1, "ode_heun": 2, "ode_ab2": 4, "dpmpp_2m": 5}


def iterations(entry):
    return GRID - 1 if entry in SOLVER else GRID * RESAMPLE if entry == "resample" else GRID


def slabs_per_iteration(entry):
    if entry in SOLVER:
        return [0] * iterations(entry)
    if entry == "resample":
        return [2 + (b >= 0) for _, b in RS.visits(GRID, JUMP, RESAMPLE)]
    return [1 if entry == "em" else 2] * GRID


@functools.lru_cache(maxsize=None)
def loop_inputs(name, entry):
    """(x0, the injected draws in consumption order, obs, mask) as fp32 numpy; read-only"""
    c = MODELS[name]
    shape = (c["B"], c["L"], c["C"])
    rng = np.random.default_rng(1000 + len(entry) + c["d"])
    x0 = rng.standard_normal(shape).astype(np.float32)
    zs = [rng.standard_normal(shape).astype(np.float32) for _ in range(sum(slabs_per_iteration(entry)))]
    obs = rng.standard_normal((1, c["L"], c["C"])).astype(np.float32)
    mask = np.zeros((1, c["L"], c["C"]), np.float32)
    mask[:, :c["L"] // 2] = 1.0
    return x0, zs, obs, mask


def device_run(n, entry, splits):
    """The entry over the iteration ranges ``splits`` = [(first, count), ...], in place on the prior -> numpy"""
    N = N_()
    lib, h = n.ctx.lib, n.ctx.handle
    x0, zs, obs, mask = loop_inputs(n.name, entry)
    x, dobs, dmask = dev(x0), dev(obs), dev(mask)
    B = x.shape[0]
    per = slabs_per_iteration(entry)
    start = np.concatenate([[0], np.cumsum(per)]).astype(int)
    cond = N.CondCfg(dobs.data_ptr(), dmask.data_ptr(), None, 1, N.FFD_COND_TIME, 1, 0)
    for first, count in splits:
        z = torch.stack([dev(a) for a in zs[start[first]:start[first + count]]]) if start[first + count] > start[first] else None
        zp = z.data_ptr() if z is not None else None
        grid = (h, x.data_ptr(), B, n.ts_c, GRID, n.h, first, count)
        if entry == "em":
            rc = lib.ffd_sample_batch(*grid, SEED, 0, zp, 0, 0, stream())
        elif entry in SOLVER:
            rc = lib.ffd_sample_batch_ode(*grid, SOLVER[entry], 0, 0, stream())
        elif entry == "pc":
            rc = lib.ffd_sample_batch_pc(*grid, 1, SNR, N.FFD_LANGEVIN_NORM_BATCH, SEED, 0, zp, 0, 0, stream())
        elif entry == "cond":
            rc = lib.ffd_sample_batch_cond(*grid, 0, SNR, N.FFD_LANGEVIN_NORM_BATCH, SEED, 0, zp, 0, 0, C.byref(cond), stream())
        else:
            rc = lib.ffd_sample_batch_resample(*grid, JUMP, RESAMPLE, 0, SNR, N.FFD_LANGEVIN_NORM_BATCH, SEED, 0, zp, C.byref(cond),
                                               stream())
        N.check(rc, h, entry)
        torch.cuda.synchronize()  # (z is released next)
    parts = C.c_int(0)
    assert lib.ffd_partition_status(h, C.byref(parts)) == 0 and parts.value == 1  # class loops run single-stream
    return x.cpu().numpy()


def judge_run(n, entry, score_fn, dtype):
    x0, zs, obs, mask = loop_inputs(n.name, entry)
    a = (n.sde, n.kw, x0)
    if entry == "em":
        return PCR.pc_integrate(*a, score_fn, lambda i, k: zs[i], n.ts, n.h, n.G, 0, SNR, "batch", dtype)
    if entry in ("ode_euler", "ode_heun"):
        return R.integrate(entry, *a, score_fn, n.ts, n.h, n.G, dtype)
    if entry in MS.METHODS:
        return MS.integrate(entry, *a, score_fn, n.ts, n.h, n.G, dtype)
    if entry == "pc":
        return PCR.pc_integrate(*a, score_fn, lambda i, k: zs[2 * i + k], n.ts, n.h, n.G, 1, SNR, "batch", dtype)
    if entry == "cond":
        return CR.cond_integrate(*a, score_fn, lambda i, k, p: zs[2 * i + p], n.ts, n.h, n.G, 0, SNR, obs, mask, None, "time", True,
                                 "batch", dtype)
    noise, trans = RS.flat_noise(zs, GRID, JUMP, RESAMPLE, 0)
    return RS.resample_integrate(*a, score_fn, noise, trans, n.ts, n.h, n.G, 0, SNR, obs, mask, JUMP, RESAMPLE, None, "time", True,
                                 "batch", dtype)


@functools.lru_cache(maxsize=None)
def loop_reference(name, sde, entry, g, variant=0, fresca=False):
    """(the float64 trajectory's end: s_c and s_u from the judge, combined and stepped in float64; the error of the same
    run in fp32 on the CPU against it).  Computed once, shared by the fused and the unfused case; read-only."""
    n = net(name, sde)
    c = n.c
    y = CL.labels_for(c["B"], variant)
    out = []
    for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        fn = CL.guided_score_fn(c["kind"], n.sd, n.table, y, g, c["NL"], c["H"], dt, FRESCA if fresca else None, GRID)
        out.append(judge_run(n, entry, fn, npdt))
    return out[0], rel_err(out[1], out[0])


LOOP_CASES = [("tf_d8", "vp", e, g, 1) for e in ENTRIES for g in (1.0, 0.0, 2.5)]
LOOP_CASES += [("tf_d8", "vp", e, 2.5, 0) for e in ENTRIES]
LOOP_CASES += [("tf_d8", "ve", "em", 2.5, 1), ("tf_d8", "ve", "dpmpp_2m", 2.5, 1)]
LOOP_CASES += [("tf_d60", "vp", e, 2.5, f) for e in ("em", "ode_heun", "dpmpp_2m", "cond") for f in (1, 0)]
LOOP_CASES += [("lstm_d8", "vp", "em", g, 1) for g in (1.0, 0.0, 2.5)] + [("lstm_d8", "vp", "ode_heun", 2.5, f) for f in (1, 0)]
LOOP_CASES += [("mlp_toy", "vp", "em", g, 1) for g in (1.0, 0.0, 2.5)] + [("mlp_toy", "vp", "ode_ab2", 2.5, 1)]


@pytest.mark.parametrize("name,sde,entry,g,fuse", LOOP_CASES,
                         ids=lambda v: str(v) if not isinstance(v, float) else f"g{v}")
def test_loop_against_the_float64_trajectory(lib, name, sde, entry, g, fuse):
    """Each case: the whole run against float64; a second run and a run split over two calls bit for bit."""
    n = net(name, sde)
    # (a batch of 3 sees every class in its first label variant, the repeat, -1 and n_classes in its second)
    variant = 1 if name == "tf_d8" and (g == 0.0 or entry in ("pc", "cond", "resample")) else 0
    y = CL.labels_for(n.c["B"], variant)
    want, e32 = loop_reference(name, sde, entry, g, variant)
    assert lib.ffd_tune(b"fuse_tail", fuse) == 0
    n_it = iterations(entry)
    enable(n, y, g)
    try:
        whole = device_run(n, entry, [(0, n_it)])
        again = device_run(n, entry, [(0, n_it)])
        split = device_run(n, entry, [(0, 2), (2, n_it - 2)])
    finally:
        disable(n)
    assert np.isfinite(whole).all()
    assert np.array_equal(whole, again), "two runs differ"
    assert np.array_equal(whole, split), "a run split over two calls differs"
    check(f"{name} {sde} {entry} g={g} fuse={fuse}", whole, want, e32, CL.FLOOR_TRAJ)


def test_fused_and_unfused_tails_and_the_labels_matter(lib):
    """The two tails agree within the trajectory bar; another label vector and another scale move the samples."""
    n = net("tf_d60")
    y = CL.labels_for(n.c["B"])
    outs = {}
    try:
        for fuse in (1, 0):
            assert lib.ffd_tune(b"fuse_tail", fuse) == 0
            enable(n, y, 2.5)
            outs[fuse] = device_run(n, "em", [(0, GRID)])
        assert lib.ffd_tune(b"fuse_tail", 1) == 0
        enable(n, CL.labels_for(n.c["B"], 1), 2.5)
        other_labels = device_run(n, "em", [(0, GRID)])
        enable(n, y, 1.0)
        other_scale = device_run(n, "em", [(0, GRID)])
    finally:
        disable(n)
    _, e32 = loop_reference("tf_d60", "vp", "em", 2.5)
    check("fused against unfused tail", outs[1], outs[0], e32, CL.FLOOR_TRAJ)
    assert rel_err(other_labels, outs[1]) > 1e-3 and rel_err(other_scale, outs[1]) > 1e-3


def test_loop_with_fresca(lib):
    N = N_()
    n = net("tf_d8")
    want, e32 = loop_reference("tf_d8", "vp", "em", 2.5, 0, True)
    cfg = N.FrescaCfg(FRESCA["low_scale"], FRESCA["high_scale"], FRESCA["cutoff_ratio"], 0, GRID)
    assert n.ctx.lib.ffd_fresca_enable(n.ctx.handle, C.byref(cfg)) == 0
    enable(n, CL.labels_for(n.c["B"]), 2.5)
    try:
        got = device_run(n, "em", [(0, GRID)])
    finally:
        disable(n)
        assert n.ctx.lib.ffd_fresca_disable(n.ctx.handle) == 0
    check("tf_d8 em g=2.5 with FreSca", got, want, e32, CL.FLOOR_TRAJ)
    plain, _ = loop_reference("tf_d8", "vp", "em", 2.5)
    assert rel_err(want, plain) > 1e-3  # FreSca did something


def plan_forms(n, B):
    N = N_()
    info = N.PartitionInfo()
    assert n.ctx.lib.ffd_partition_plan(n.ctx.handle, B, N.FFD_SOLVER_EULER_MARUYAMA, C.byref(info)) == 0
    w = info.whole
    return (info.whole_planned, w.ffn, w.attn, w.nw, w.cps, w.mb, w.persist, w.hpw, w.qg, w.kspl, w.one_per_tile)


@pytest.mark.parametrize("name", FORWARD_NETS)
def test_all_null_labels_under_guidance_are_the_unconditional_run(lib, name):
    """s_u + g (s_c - s_u) with every label null: the g = 0 run.  Bit for bit where the stacked batch of 2 B rows is
    planned to the kernel forms of B rows (then a row's bits are the same in both, and c - u is exactly 0); within the bar
    otherwise.  Which case a shape is, is asserted."""
    n = net(name)
    B = n.c["B"]
    try:
        enable(n, None, 0.0)
        uncond = device_run(n, "em", [(0, GRID)])
        enable(n, np.full(B, -1, np.int32), 2.5)
        guided = device_run(n, "em", [(0, GRID)])
    finally:
        disable(n)
    at_b, at_2b = plan_forms(n, B), plan_forms(n, 2 * B)
    same_forms = bool(at_b[0]) and at_b == at_2b
    print(f"{name}: plan at B {at_b}, at 2B {at_2b}")
    assert same_forms == {"tf_d8": True, "tf_d60": True, "lstm_d8": False, "mlp_toy": False}[name]
    if same_forms:
        assert np.array_equal(guided, uncond)
    else:
        _, e32 = loop_reference(name, "vp", "em", 0.0, 1 if name == "tf_d8" else 0)
        check(f"{name} all-null g=2.5 against g=0", guided, uncond, e32, CL.FLOOR_TRAJ)


def test_class_conditioned_loops_stay_single_stream(lib):
    """At a shape and knobs where the plain loop runs as two CU partitions (device draws), the class-conditioned loop
    reports one and gives the bits of "partitions" = 0."""
    N = N_()
    n = net("tf_d24")
    B, L, Cn = n.c["B"], n.c["L"], n.c["C"]
    x0 = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, 1234))).cuda()

    def run(partitions):
        assert lib.ffd_tune(b"reset", 0) == 0
        for k, v in dict(D24_KNOBS, partitions=partitions).items():
            assert lib.ffd_tune(k.encode(), v) == 0, k
        x = x0.clone()
        N.check(lib.ffd_sample_batch(n.ctx.handle, x.data_ptr(), B, n.ts_c, GRID, n.h, 1, 3, SEED, 5, None, 0, 0, stream()),
                n.ctx.handle, "ffd_sample_batch")
        parts = C.c_int(0)
        assert lib.ffd_partition_status(n.ctx.handle, C.byref(parts)) == 0
        torch.cuda.synchronize()
        return parts.value, x

    assert run(2)[0] == 2  # the plain loop does partition here
    for g in (1.0, 2.5):
        enable(n, CL.labels_for(B), g)
        try:
            p2, x2 = run(2)
            p0, x0_ = run(0)
        finally:
            disable(n)
        assert (p2, p0) == (1, 1) and torch.equal(x2, x0_) and bool(torch.isfinite(x2).all())
    assert run(2)[0] == 2  # and partitions again once the state is off


def test_refusals_on_the_device(lib):
    N = N_()
    n = net("tf_d8")
    B = n.c["B"]
    x = torch.zeros(B, n.c["L"], n.c["C"], device="cuda")
    out = torch.empty_like(x)
    delta = torch.zeros(B, device="cuda", dtype=torch.float64)
    h = n.ctx.handle
    assert lib.ffd_cache_enable(h, C.byref(N.CacheCfg(5, 10))) == 0
    enable(n, CL.labels_for(B), 2.5)
    try:
        grid = (h, x.data_ptr(), B, n.ts_c, GRID, n.h, 0, 1)
        assert lib.ffd_sample_batch(*grid, SEED, 0, None, 1, 0, stream()) == -3 and b"class" in lib.ffd_last_error(h)
        assert lib.ffd_sample_batch_ode(*grid, 2, 1, 0, stream()) == -3
        assert lib.ffd_score_forward(h, x.data_ptr(), 0.5, out.data_ptr(), B, stream()) == -3
        assert lib.ffd_score_forward_cached(h, x.data_ptr(), 0.5, out.data_ptr(), None, B, 0, stream()) == -3
        t = torch.full((B,), 0.5, device="cuda")
        assert lib.ffd_score_forward_ts(h, x.data_ptr(), t.data_ptr(), out.data_ptr(), None, B, 2, stream()) == -3
        assert lib.ffd_loglik_batch(h, x.data_ptr(), delta.data_ptr(), B, n.ts_c, GRID, 0, 1, 1, 1, 1e-2, None, 0, 0, stream()) == -3
        cond = N.CondCfg(out.data_ptr(), out.data_ptr(), None, 1, N.FFD_COND_TIME, 1, 0)
        guide = N.GuideCfg(1.0, 1.0, 0.0, 0, 0)
        assert lib.ffd_sample_batch_guided(h, None, *grid[1:], SEED, 0, None, C.byref(cond), C.byref(guide), None, stream()) == -3
        wrong = (h, x.data_ptr(), B - 1, n.ts_c, GRID, n.h, 0, 1)  # n_labels != B
        assert lib.ffd_sample_batch(*wrong, SEED, 0, None, 0, 0, stream()) == -1
        assert lib.ffd_score_forward_ts(h, x.data_ptr(), t.data_ptr(), out.data_ptr(), None, B - 1, -1, stream()) == -1
        assert not x.any()  # nothing ran
        assert lib.ffd_sample_batch(*grid, SEED, 0, None, 0, 0, stream()) == 0  # and the state itself works
    finally:
        disable(n)
        assert lib.ffd_cache_disable(h) == 0
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    mix = MixtureScoreModule(n_channels=1, max_len=5, noise_scheduler=TR.scheduler("vp", 5), means=torch.zeros(2, 5, 1)).cuda()
    mctx = mix._ctx()
    cfg = N.ClassCfg(n.table_dev.data_ptr(), None, None, NC, 0, 1.0, 0)
    assert lib.ffd_class_enable(mctx.handle, C.byref(cfg)) == -2


# ------------------------------------------------------------------------------------------------------- training ----
def make_trainer(model, **kw):
    from fastfourierdiffusion_amd.training import Trainer

    return Trainer(model.cuda(), **kw)


def grads_of(model):
    return {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad}


GRAD_PARAMS = [(c, sde, p) for c in CL.GRAD_CASES for sde in ("vp", "ve") for p in CL.P_UNCOND]


@pytest.mark.parametrize("case,sde,p", GRAD_PARAMS, ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_whole_gradient_with_classes(lib, case, sde, p):
    """Every parameter tensor's gradient, the table's included, against float64 autograd through the one-hot judge, with
    injected times and noise; the dropped labels are the restated drop's under the trainer's key.  Measured on an MI355X:
    worst per-tensor error 6.3e-6 .. 9.7e-6 (c1), 8.0e-6 / 3.7e-5 (c2, VP / VE), 6.5e-6 .. 9.5e-6 (the MLP toy): the CPU fp32
    autograd's own error."""
    model, sd, table, (x0, t, mc, sigma, z), labels, eff = CL.grad_case_setup(case, sde, p)
    kind, NL, H, G = case["kind"], case["NL"], case["H"], model.noise_scheduler.G.numpy()
    margin, e32 = CL.kink_report(kind, sd, table, NL, H, x0, t, mc, sigma, G, z, eff)
    print(f"kink margin {margin:.2e}, fp32 pre-activation error {e32:.2e}, pushed weights: {case['push']}")
    assert margin > TR.KINK_MARGIN * e32
    dropped = (eff == NC) & (CL.effective(labels, NC) != NC)
    assert dropped.any() == (p > 0) and (p == 0 or not dropped.all()), "the case must see kept and dropped labels"
    l64, per64, g64 = CL.gradients(kind, sd, table, NL, H, x0, t, mc, sigma, G, z, eff, False, torch.float64)
    l32, per32, g32 = CL.gradients(kind, sd, table, NL, H, x0, t, mc, sigma, G, z, eff, False, torch.float32)
    tr = make_trainer(model, seed=CL.TRAIN_SEED, p_uncond=p)
    loss = tr.loss_and_grad(dev(x0), timesteps=dev(t), z=dev(z), labels=labels)
    check("per-sample loss", tr.last_per_sample.cpu().numpy(), per64, rel_err(per32, per64))
    assert abs(float(loss) - l64) <= TR.bar(abs(l32 - l64) / abs(l64)) * abs(l64) + 1e-7 * abs(l64)
    got = grads_of(model)
    assert set(got) == set(g64) and CL.TABLE in got
    worst = 0.0
    for k in g64:
        worst = max(worst, check(k, got[k], g64[k], rel_err(g32[k], g64[k])))
    print(f"{case['name']} {sde} p_uncond={p}: worst per-tensor gradient error {worst:.2e}")
    absent = [c for c in range(NC + 1) if not (CL.effective(eff, NC) == c).any()]
    assert all(not got[CL.TABLE][c].any() for c in absent)


class ClassRun:
    """The reference's update restated for the class-conditional transformer in ``dtype`` on the CPU (TR.MlpRun's
    arithmetic; the positional rows renormalised in place before every step, as the device does)."""

    def __init__(self, sd, table, c, G, lr_max, warmup, total, dtype):
        self.p = TR.cast(dict(sd, **{CL.TABLE: torch.as_tensor(table)}), dtype)
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items() if k not in TR.FROZEN}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items() if k not in TR.FROZEN}
        self.c, self.G, self.dtype, self.lr_max, self.warmup, self.total = c, G, dtype, lr_max, warmup, total
        self.k, self.coefs = 0, []

    def step(self, x0, t, mc, sigma, z, eff):
        import math

        from oracle import ffd_oracle as O

        c = self.c
        with torch.no_grad():
            self.p[TR.POS].copy_(O.renorm_embedding(self.p[TR.POS].detach(), math.sqrt(c["d"])).to(self.dtype))
        for k, v in self.p.items():
            v.grad = None
            v.requires_grad_(k not in TR.FROZEN)
        s = {k: v for k, v in self.p.items() if k != CL.TABLE}
        loss = CL.loss(c["kind"], s, self.p[CL.TABLE], c["NL"], c["H"], x0, t, mc, sigma, self.G, z, eff, False, self.dtype)[0]
        loss.backward()
        names = list(self.m)
        _, coef = TR.clip_coef([self.p[k].grad for k in names], 1.0)
        self.coefs.append(coef)
        lr = self.lr_max * TR.lr_lambda(self.k, self.warmup, self.total)
        with torch.no_grad():
            for k in names:
                TR.adamw_step(self.p[k], self.p[k].grad * coef, self.m[k], self.v[k], self.k + 1, lr)
        self.k += 1
        return float(loss.detach())


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_three_clipped_updates_with_classes(lib, sde):
    """Three consecutive steps with injected t and z and p_uncond = 0.5: parameters and both moments, the table's among
    them (clip and decay included), against float64 AdamW."""
    case, p = CL.UPDATE_CASE, 0.5
    model, sd, table, _, labels, _ = CL.grad_case_setup(case, sde, p)
    sch = model.noise_scheduler
    G = sch.G.numpy()
    runs = {dt: ClassRun(sd, table, case, G, model.lr_max, model.num_warmup_steps, model.num_training_steps, dt)
            for dt in (torch.float64, torch.float32)}
    tr = make_trainer(model, seed=CL.TRAIN_SEED, p_uncond=p)
    for k in range(3):
        x0, t, mc, sigma, z = TR.case_inputs(case, sch, k)
        eff = CL.class_drop(labels, NC, None, case["B"], p, (CL.TRAIN_SEED + k * TR.DRAW_STRIDE) & ((1 << 64) - 1), 0)
        r64 = runs[torch.float64]
        now = {kk: v.detach().float() for kk, v in r64.p.items() if kk != CL.TABLE}
        margin, e32 = CL.kink_report(case["kind"], now, r64.p[CL.TABLE].detach().float().numpy(), case["NL"], case["H"], x0, t, mc,
                                     sigma, G, z, eff)
        assert margin > TR.KINK_MARGIN * e32, f"step {k}"
        ref = [runs[dt].step(x0, t, mc, sigma, z, eff) for dt in runs]
        got = float(tr.step(dev(x0), timesteps=dev(t), z=dev(z), labels=labels))
        assert abs(got - ref[0]) <= 1e-5 * abs(ref[0])
    r64, r32 = runs[torch.float64], runs[torch.float32]
    print(f"{case['name']} {sde}: clip coefficients {r64.coefs}")
    for k, prm in model.named_parameters():
        if not prm.requires_grad:
            continue
        for what, got, a, b in (("param", prm, r64.p[k], r32.p[k]), ("exp_avg", tr.exp_avg[k], r64.m[k], r32.m[k]),
                                ("exp_avg_sq", tr.exp_avg_sq[k], r64.v[k], r32.v[k])):
            a, b = a.detach().numpy(), b.detach().numpy()
            check(f"{k} {what}", got.detach().cpu().numpy(), a, rel_err(b, a))


def params_of(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def two_class_data(n=256, seed=11):
    """TR.toy_dataset's two modes with the mode as the label: class 0 = + the pattern, class 1 = - the pattern."""
    c = TR.TF_TOY
    rng = np.random.default_rng(seed)
    l = np.arange(c["L"])[:, None]
    pattern = np.sin(2 * np.pi * (l + 1) / c["L"] + 0.7 * np.arange(c["C"])[None, :])
    y = (rng.random(n) < 0.5).astype(np.int32)
    X = (np.where(y == 0, 1.0, -1.0)[:, None, None] * pattern[None] + 0.1 * rng.standard_normal((n, c["L"], c["C"])))
    return X.astype(np.float32), y, pattern


TOY_LR, TOY_SAMPLER_STEPS = 2e-2, 100


def new_toy(seed=3, p_uncond=0.1):
    """TR.TF_TOY's network with two classes.  lr_max = 2e-2 (TF_TOY's 1e-3 leaves a 200-step model whose samples are
    noise: sized on the CPU, see test_200_steps_give_samples_of_the_requested_class)."""
    c = TR.TF_TOY
    m = CL.tf_class_model(c, "vp", total=c["total"], lr_max=TOY_LR, n_classes=2)
    return m, make_trainer(m, seed=seed, p_uncond=p_uncond)


def test_fit_hand_loop_and_resume_bit_for_bit(lib, tmp_path):
    c = TR.TF_TOY
    Xn, yn, _ = two_class_data()
    X, y = dev(Xn), torch.from_numpy(yn)
    m1, t1 = new_toy()
    h1 = t1.fit(X, batch_size=c["B"], max_epochs=2, labels=y, X_val=X[:64], labels_val=y[:64])
    assert h1["val_loss"].shape == (2,) and bool(torch.isfinite(h1["val_loss"]).all())
    h1 = h1["train_loss"]
    m2, t2 = new_toy()
    h2 = []
    for e in range(2):
        order = torch.from_numpy(t2.epoch_order(c["n"], e)).cuda()
        for i in range(0, c["n"], c["B"]):
            h2.append(t2.loss_and_grad(X, index=order[i:i + c["B"]], labels=y))
            t2.apply_update(t2.grad_sqnorm())
    assert torch.equal(h1, torch.stack(h2)) and same(params_of(m1), params_of(m2)) and same(t1.exp_avg_sq, t2.exp_avg_sq)
    m3, t3 = new_toy()
    t3.fit(X, batch_size=c["B"], max_epochs=1, labels=y)
    t3.save_checkpoint(tmp_path / "c.ckpt")
    m4, t4 = new_toy(seed=9, p_uncond=0.7)
    t4.resume(tmp_path / "c.ckpt")
    assert t4.p_uncond == 0.1 and t4.seed == 3
    assert torch.equal(t4.fit(X, batch_size=c["B"], max_epochs=1, labels=y)["train_loss"], h1[8:])
    assert same(params_of(m1), params_of(m4))
    # the labels do reach the loss: other labels, another curve; and a model without classes takes none
    m5, t5 = new_toy()
    h5 = t5.fit(X, batch_size=c["B"], max_epochs=1, labels=1 - y)["train_loss"]
    assert not torch.equal(h5, h1[:8])
    plain = make_trainer(TR.tf_model(c, "vp"))
    with pytest.raises(AssertionError):
        plain.step(X[:4].contiguous(), labels=y[:4])


def test_training_forward_with_labels_against_the_context(lib):
    """ffd_train_forward (the labels as they are, no dropout even at p_uncond = 1) and the inference context on the same
    parameters, both within the forward bar of the float64 judge."""
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch

    case = CL.GRAD_CASES[1]
    model, sd, table, (x0, t, mc, sigma, z), labels, _ = CL.grad_case_setup(case, "vp", 0.0)
    xn = TR.perturb(*[torch.from_numpy(a) for a in (x0, z, mc, sigma)], model.noise_scheduler.G)[0].numpy()
    want = CL.forward_np("transformer", xn, t, TR.renormed(sd), table, labels, case["NL"], case["H"])
    e32 = rel_err(CL.forward_np("transformer", xn, t, TR.renormed(sd), table, labels, case["NL"], case["H"], torch.float32), want)
    tr = make_trainer(model, p_uncond=1.0)
    dx, dt = dev(xn), dev(t)
    inf = model.eval()(DiffusableBatch(X=dx, y=torch.from_numpy(labels), timesteps=dt))
    tr._set_labels(torch.from_numpy(labels), dx)
    out = torch.empty_like(dx)
    tr._check(lib.ffd_train_forward(tr.handle, dx.data_ptr(), dt.data_ptr(), out.data_ptr(), case["B"], stream()), "forward")
    check("training forward", out.cpu().numpy(), want, e32)
    check("inference forward", inf.cpu().numpy(), want, e32)
    null = model(DiffusableBatch(X=dx, timesteps=dt))  # y None: the null class
    check("inference forward, y None", null.cpu().numpy(),
          CL.forward_np("transformer", xn, t, TR.renormed(sd), table, None, case["NL"], case["H"]), e32)


_TOY = {}


def trained_toy():
    """200 steps on the two well-separated classes, once."""
    if not _TOY:
        c = TR.TF_TOY
        Xn, yn, pattern = two_class_data()
        m, t = new_toy()
        hist = t.fit(dev(Xn), batch_size=c["B"], max_epochs=25, labels=torch.from_numpy(yn))["train_loss"]
        assert t.global_step == 200
        _TOY.update(model=m, trainer=t, pattern=pattern, loss=hist.cpu().numpy())
    return _TOY


def test_200_steps_give_samples_of_the_requested_class(lib):
    """A sign check, not a quality bar: the samples drawn with label k lie nearer class k's mean (+- the pattern) than
    the other's, on average over 64 samples per label.  The run was sized on the CPU with the fp32 judge alone (the same
    200 steps, then 100 Euler-Maruyama steps on numpy draws): mean squared distance to the own / the other class's mean
    12.2 / 41.4 and 17.2 / 35.7 at g = 1, 4.8 / 52.0 and 5.7 / 49.1 at g = 2; at TF_TOY's lr_max = 1e-3 the samples of a
    200-step model are noise (323 / 327).  Measured on an MI355X (Philox draws): 12.1 / 41.7 and 15.0 / 38.8 at g = 1,
    4.4 / 53.4 and 8.1 / 47.4 at g = 2."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    T = trained_toy()
    assert np.isfinite(T["loss"]).all() and T["loss"][-8:].mean() < T["loss"][:8].mean()
    s = DiffusionSampler(T["model"], sample_batch_size=64, rng="philox", seed=5)
    mean = {0: T["pattern"], 1: -T["pattern"]}
    for g in (1.0, 2.0):
        x = s.sample(128, TOY_SAMPLER_STEPS, labels=torch.cat([torch.zeros(64), torch.ones(64)]).long(), guidance_scale=g).numpy()
        assert x.shape == (128, 12, 2) and np.isfinite(x).all()
        for k in (0, 1):
            xs = x[64 * k:64 * (k + 1)]
            own = ((xs - mean[k]) ** 2).sum((1, 2)).mean()
            other = ((xs - mean[1 - k]) ** 2).sum((1, 2)).mean()
            print(f"g={g} label {k}: mean squared distance to its class {own:.3f}, to the other {other:.3f}")
            assert own < other, (g, k, own, other)


def test_sampler_labels_end_to_end_and_from_a_checkpoint(lib, tmp_path):
    """sample(labels=...) over two batches is the two native runs on the label slices (bit for bit); a model reloaded from
    the trainer's checkpoint samples the same bits; impute(labels=...) runs and returns the observed points."""
    from fastfourierdiffusion_amd.models.score_models import ClassConditionalScoreModule
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    c = TR.TF_TOY
    Xn, yn, pattern = two_class_data()
    torch.manual_seed(21)  # (the default FFN width: load_from_checkpoint rebuilds the module from its constructor arguments)
    m = ClassConditionalScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=TR.scheduler("vp", c["L"]), n_classes=2,
                                    d_model=c["d"], num_layers=c["NL"], n_head=c["H"], num_training_steps=200, lr_max=TOY_LR)
    trainer = make_trainer(m, seed=3)
    trainer.fit(dev(Xn), batch_size=c["B"], max_epochs=2, labels=torch.from_numpy(yn))
    labels = torch.tensor([0, 1, 1, -1, 2, 0, 1, 0])

    def draw(model, **kw):
        s = DiffusionSampler(model, sample_batch_size=4, rng="philox", seed=5)
        return s.sample(8, GRID, labels=labels, **kw)

    a = draw(m, guidance_scale=1.5)
    assert a.shape == (8, c["L"], c["C"]) and bool(torch.isfinite(a).all())
    halves = [DiffusionSampler(m, sample_batch_size=4, rng="philox", seed=5, sample_offset=4 * i).sample(
        4, GRID, labels=labels[4 * i:4 * i + 4], guidance_scale=1.5) for i in range(2)]
    assert torch.equal(a, torch.cat(halves))
    assert not torch.equal(a, draw(m, guidance_scale=1.0)) and not torch.equal(draw(m), draw(m, guidance_scale=0.0))
    assert torch.equal(draw(m, guidance_scale=0.0),
                       DiffusionSampler(m, sample_batch_size=4, rng="philox", seed=5).sample(8, GRID, guidance_scale=0.0))
    trainer.save_checkpoint(tmp_path / "toy.ckpt")
    back = ClassConditionalScoreModule.load_from_checkpoint(tmp_path / "toy.ckpt", map_location="cuda")
    assert back.n_classes == 2 and torch.equal(back.class_embedding.weight, m.class_embedding.weight)
    assert torch.equal(draw(back, guidance_scale=1.5), a)
    series = torch.from_numpy(pattern.astype(np.float32))
    mask = torch.zeros(c["L"])
    mask[:6] = 1.0
    s = DiffusionSampler(m, sample_batch_size=4, rng="philox", seed=5)
    out = s.impute(series, mask, 4, GRID, labels=torch.tensor([0, 0, 1, 1]), guidance_scale=1.5)
    assert out.shape == (4, c["L"], c["C"]) and bool(torch.isfinite(out).all())
    assert float((out[:, :6] - series[None, :6]).abs().max()) < 1e-4
    with pytest.raises(NotImplementedError):
        s.log_likelihood(a, GRID, labels=labels)


def test_sampler_with_injected_noise_against_the_float64_trajectory(lib):
    """DiffusionSampler.sample on a class-conditional module: two batches with their label slices, against the judge."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    case = CL.GRAD_CASES[0]
    model = CL.tf_class_model(case, "vp").cuda().eval()
    with torch.no_grad():
        model.class_embedding.weight.copy_(dev(CL.make_table(NC, case["d"], 7, std=0.3)))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k != CL.TABLE}
    table = model.class_embedding.weight.detach().cpu().numpy()
    B, L, Cn = case["B"], case["L"], case["C"]
    labels = np.concatenate([CL.labels_for(B, 0), CL.labels_for(B, 1)])
    rng = np.random.default_rng(2)
    draws = [rng.standard_normal((B, L, Cn)).astype(np.float32) for _ in range(2 * (GRID + 1))]
    s = DiffusionSampler(model, sample_batch_size=B)
    s.inject_noise(draws)
    got = s.sample(2 * B, GRID, labels=labels, guidance_scale=2.5).numpy()
    sch = model.noise_scheduler
    ts, h, G = sch.timesteps.to(torch.float32).numpy(), float(sch.step_size), sch.G.numpy()
    for i in range(2):
        zs = draws[i * (GRID + 1):(i + 1) * (GRID + 1)]
        out = []
        for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            fn = CL.guided_score_fn("transformer", sd, table, labels[i * B:(i + 1) * B], 2.5, case["NL"], case["H"], dt)
            x0 = zs[0].astype(npdt) * G.astype(npdt)[None, :, None]  # the VP prior: G z
            out.append(PCR.pc_integrate("vp", TR.SDE_KW["vp"], x0, fn, lambda j, k: zs[1 + j], ts, h, G, 0, SNR, "batch", npdt))
        check(f"sampler batch {i}", got[i * B:(i + 1) * B], out[0], rel_err(out[1], out[0]), CL.FLOOR_TRAJ)
