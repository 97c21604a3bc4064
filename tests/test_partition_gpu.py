"""The sampling loops as two CU partitions (ffd_tune "partitions"): the same bits as the single-stream path and as two
separate calls on the halves; the ineligible cases stay on the caller's stream; the caller's stream sees the result."""
import ctypes as C

import pytest
import torch

from fastfourierdiffusion_amd import _native as N
from fastfourierdiffusion_amd.models.score_models import ScoreModule
from fastfourierdiffusion_amd.schedulers.sde import VPScheduler
from fastfourierdiffusion_amd.utils import synthetic

pytestmark = pytest.mark.gpu

STEPS, GRID, SEED, OFFSET = 3, 8, 42, 5
# the same kernel instances whatever the batch and the CU budget: the row-owning FFN at 4 waves (128-row tiles), no
# small- / mid-batch or sliced forms, one attention form
ECG_KNOBS = {"ffn_rows": 2, "ffn_rows_nw": 4, "rows_slices": -1, "small_path": 0, "mid_path": 0, "ffn_height": 0, "attn_small": 0}
# d_model 24 has no row-owning FFN: k_ffn_ln at 16-row tiles, which keeps no partial rows in a shared workspace either
D24_KNOBS = {"ffn_mb": 1, "rows_slices": -1, "small_path": 0, "mid_path": 0, "ffn_height": 0, "attn_small": 0}
SHAPES = {"ecg_B2": ("ecg", 2), "ecg_B3": ("ecg", 3), "ecg_B8": ("ecg", 8), "d24_B5": ("d24", 5)}
MODELS = {"ecg": dict(L=187, C=1, d=72, H=12, NL=2, knobs=ECG_KNOBS), "d24": dict(L=24, C=3, d=24, H=4, NL=2, knobs=D24_KNOBS)}
_built = {}


@pytest.fixture(autouse=True)
def _knobs_back():
    yield
    N.lib().ffd_tune(b"reset", 0)


def model(kind):
    if kind not in _built:
        c = MODELS[kind]
        sch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=42)
        m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"], n_head=c["H"])
        sch.set_noise_scaling(c["L"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        sch.set_timesteps(GRID)
        _built[kind] = (m.cuda().eval(), (C.c_float * GRID)(*sch.timesteps.tolist()), float(sch.step_size))
    return _built[kind]


def prior(kind, B):
    c = MODELS[kind]
    return torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, 1234))).cuda()


def tune(knobs, partitions):
    lib = N.lib()
    assert lib.ffd_tune(b"reset", 0) == 0
    for k, v in dict(knobs, partitions=partitions).items():
        assert lib.ffd_tune(k.encode(), v) == 0, k


def run(kind, x, entry, partitions, offset=OFFSET, knobs=None, use_cache=0, stream=None):
    """STEPS steps of `entry` in place on x; returns the partitions the library reports."""
    m, ts, h = model(kind)
    ctx = m._ctx()
    tune(MODELS[kind]["knobs"] if knobs is None else knobs, partitions)
    s = N.current_stream_ptr(x.device) if stream is None else stream
    if entry == "sde":
        rc = ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, 1, STEPS, SEED, offset, None,
                                      use_cache, 1 if use_cache else 0, s)
    else:
        rc = ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, 1, STEPS, N.FFD_SOLVER_ODE_EULER,
                                          use_cache, 1 if use_cache else 0, s)
    N.check(rc, ctx.handle, entry)
    parts = C.c_int(0)
    assert ctx.lib.ffd_partition_status(ctx.handle, C.byref(parts)) == 0
    return parts.value


@pytest.mark.parametrize("entry", ["sde", "ode_euler"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_partitioned_bits_equal_single_stream_and_separate_halves(shape, entry):
    kind, B = SHAPES[shape]
    x0 = prior(kind, B)
    one, two = x0.clone(), x0.clone()
    assert run(kind, one, entry, 0) == 1
    assert run(kind, two, entry, 2) == 2            # the partitioned path did run
    torch.cuda.synchronize()
    assert torch.isfinite(one).all() and not torch.equal(one, x0)
    assert torch.equal(two, one)
    nb0 = (B + 1) // 2                              # two calls on the halves, with their global sample offsets
    a, b = x0[:nb0].clone(), x0[nb0:].clone()
    assert run(kind, a, entry, 0) == 1 and run(kind, b, entry, 0, offset=OFFSET + nb0) == 1
    assert torch.equal(torch.cat([a, b]), two)


def test_below_the_threshold_the_single_stream_path_runs():
    """One sample cannot be halved; and under the default knobs a batch of 8 takes the small-batch FFN pair, whose
    partial rows share a workspace: "partitions" = 1 and 2 both leave it on the caller's stream."""
    x0 = prior("ecg", 1)
    one, two = x0.clone(), x0.clone()
    assert run("ecg", one, "sde", 0) == 1 and run("ecg", two, "sde", 2) == 1
    assert torch.equal(one, two)
    x0 = prior("ecg", 8)
    ref = x0.clone()
    assert run("ecg", ref, "sde", 0, knobs={}) == 1
    for p in (1, 2):
        got = x0.clone()
        assert run("ecg", got, "sde", p, knobs={}) == 1
        assert torch.equal(got, ref)
    small = x0.clone()  # the pinned row-owning form is eligible, but 8 samples do not fill half the chip: auto declines
    assert run("ecg", small, "sde", 1) == 1


def test_cache_and_fresca_energy_stay_single_stream():
    m, _, _ = model("ecg")
    ctx = m._ctx()
    x0 = prior("ecg", 8)
    assert ctx.lib.ffd_cache_enable(ctx.handle, C.byref(N.CacheCfg(5, 10))) == 0
    try:
        outs = []
        for p in (0, 2):
            assert ctx.lib.ffd_cache_reset(ctx.handle) == 0
            x = x0.clone()
            assert run("ecg", x, "sde", p, use_cache=1) == 1
            outs.append(x)
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], x0)
    finally:
        assert ctx.lib.ffd_cache_disable(ctx.handle) == 0
    assert ctx.lib.ffd_fresca_enable(ctx.handle, C.byref(N.FrescaCfg(1.0, 1.5, 0.5, 1, 0))) == 0  # strategy 1: energy
    try:
        outs = []
        for p in (0, 2):
            x = x0.clone()
            assert run("ecg", x, "sde", p) == 1
            outs.append(x)
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], x0)
    finally:
        assert ctx.lib.ffd_fresca_disable(ctx.handle) == 0
    x = x0.clone()
    assert run("ecg", x, "sde", 2) == 2  # and the context partitions again afterwards


def test_work_enqueued_behind_the_call_sees_the_final_samples():
    """The join puts both halves in front of whatever the caller enqueues next on ITS stream: a copy made there, awaited
    through that stream alone, holds the final samples."""
    x0 = prior("ecg", 8)
    ref = x0.clone()
    assert run("ecg", ref, "sde", 0) == 1
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    x = x0.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert run("ecg", x, "sde", 2, stream=st.cuda_stream) == 2
        seen = x.clone()
    st.synchronize()
    assert torch.equal(seen, ref)
