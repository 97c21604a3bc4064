"""GPU tests of the loop iterations and launcher branches of the sampling tails that no other test reaches.

1. *Second tile of a wave.*  The fused unembed tail (``k_unembed_mfma<D, Tail>``) runs at most 2048 x 4 waves of 16 rows:
   a wave takes a second tile, and computes from the registers it prefetched under the first, only when B L > 131072.
   A one-layer d = 8 transformer at L = 64, B = 2052 has 131328 rows, so 16 waves loop.  Every tail form must give the
   bits of the stand-alone unembedding + step kernel (``fuse_tail`` 0).
2. *Second grid-stride pass.*  The pointwise step kernels (``k_step_v4<Op>`` / ``k_step<Op>``) run at most 4096 x 256
   threads, one float4 (or four scalars) each: 4,194,304 elements on the float4 path.  (1026, 1024, 4) and (1368, 1024, 3)
   hold 4,202,496 elements; every context-free operator on the whole batch must give the bits of its calls on chunks of
   128 samples (524,288 / 393,216 elements: below every cap), the drawing ones with ``sample_offset`` per chunk.
3. *The launcher's float4 conditions*, at small shapes: a misaligned z and odd element offsets change the kernel form,
   never the bits.
"""
import ctypes as C_

import pytest
import torch

from fastfourierdiffusion_amd.utils import synthetic
from test_ode_gpu import _tune_defaults, build, ffd, sampler_for, scheduler  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ 1. second tile of a wave ----
WAVE_MODEL = dict(kind="transformer", d=8, H=2, NL=1, L=64, B=2052)  # 131328 rows > 2048 x 4 x 16
# (solver, draws, grid points): two steps / two intervals each, so that the multistep tail runs both of its forms
WAVE_RUNS = [("euler_maruyama", "inject", 2), ("euler_maruyama", "philox", 2), ("ode_euler", None, 3), ("ode_heun", None, 3),
             ("dpmpp_2m", None, 3)]


@pytest.mark.parametrize("solver,draws,n", WAVE_RUNS, ids=[f"{s}-{d}" if d else s for s, d, _ in WAVE_RUNS])
@pytest.mark.parametrize("Cn", [1, 4], ids=["C1_ragged", "C4_quad"])
def test_second_tile_of_a_wave_fused_equals_standalone(ffd, Cn, solver, draws, n):
    from fastfourierdiffusion_amd import _native

    c = dict(WAVE_MODEL, C=Cn)
    assert c["B"] * c["L"] > 2048 * 4 * 16
    m, sch, sd = build(c, "vp")
    lib = _native.lib()
    shape = (c["B"], c["L"], Cn)
    noise = list(synthetic.noise_stream(shape, n + 1, 51)) if draws != "philox" else None

    def run():
        s = sampler_for(m, c, solver, **(dict(rng="philox", seed=9) if draws == "philox" else {}))
        if noise is not None:
            s.inject_noise(noise)
        return s.sample(num_samples=c["B"], num_diffusion_steps=n)

    fused = run()
    tail = lib.ffd_kernel_work(m._ctx().handle, _native.K_SDE, c["B"], 0, None, None)
    assert tail.startswith(b"k_unembed_"), tail
    assert lib.ffd_tune(b"fuse_tail", 0) == 0
    plain = run()
    tail = lib.ffd_kernel_work(m._ctx().handle, _native.K_SDE, c["B"], 0, None, None)
    assert not tail.startswith(b"k_unembed_"), tail
    assert bool(torch.isfinite(fused).all())
    assert torch.equal(fused, plain)


# ------------------------------------------------------ 2. second grid-stride pass ----
SEED, T, SNR = 11, 0.5, 0.16


def operator_inputs(shape, seed=5, misaligned_z=False):
    """x, score, z, xp, d1, hist of ``shape`` on the device.  ``misaligned_z`` adds ``z_off``: the same draws one float
    into a buffer (a 4-byte aligned view: the float4 path must refuse it)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = {k: torch.randn(shape, device="cuda", generator=g) for k in ("x", "score", "z", "xp", "d1", "hist")}
    if misaligned_z:
        buf = torch.empty(t["z"].numel() + 4, device="cuda")
        buf[1:-3].copy_(t["z"].reshape(-1))
        t["z_off"] = buf[1:-3].view(shape)
    return t


def run_operator(name, sch, t, lo, hi, draws="inject", offset=0, z_key="z"):
    """Operator ``name`` on samples [lo, hi) of the inputs ``t``; global sample index ``offset`` + lo.  Returns the
    tuple of its outputs.  ``draws``: "inject" (z from ``t[z_key]``) or "device" (Philox under SEED)."""
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    B, (_, L, Cn) = hi - lo, t["x"].shape
    dev = t["x"].device
    G, stream, desc = sch._G_on(dev).data_ptr(), N.current_stream_ptr(dev), sch._desc()
    h = float(sch.step_size)
    new = {k: t[k][lo:hi].clone() for k in ("x", "xp", "d1", "hist")}
    sc = t["score"][lo:hi].data_ptr()
    z = t[z_key][lo:hi].data_ptr() if draws == "inject" else None
    off, d = offset + lo, C_.byref(desc)
    x = new["x"]
    if name == "sde_step":
        rc, out = lib.ffd_sde_step(d, x.data_ptr(), sc, G, T, h, z, SEED, off, 3, B, L, Cn, stream), (x,)
    elif name in ("forward_transition", "forward_transition_noiseless"):
        t_to = 0.6 if name == "forward_transition" else 0.2
        rc, out = lib.ffd_forward_transition(d, x.data_ptr(), G, 0.2, t_to, z, SEED, off, 0xE0000001, B, L, Cn, stream), (x,)
    elif name == "ode_step":
        rc, out = lib.ffd_ode_step(d, x.data_ptr(), sc, G, T, h, B, L, Cn, stream), (x,)
    elif name == "ode_heun_predict":
        xp, d1 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        rc = lib.ffd_ode_heun_predict(d, x.data_ptr(), sc, G, T, h, xp.data_ptr(), d1.data_ptr(), B, L, Cn, stream)
        out = (xp, d1, x)
    elif name == "ode_heun_correct":
        rc = lib.ffd_ode_heun_correct(d, x.data_ptr(), new["xp"].data_ptr(), sc, new["d1"].data_ptr(), G, T - h, h, B, L, Cn,
                                      stream)
        out = (x,)
    elif name in ("multistep_first", "multistep_prev"):
        have = name == "multistep_prev"
        coef = (C_.c_double * 5)(*sch.multistep_coefficients("dpmpp_2m", T, T - h, T + h if have else None))
        hist = new["hist"] if have else torch.full_like(x, float("nan"))
        rc = lib.ffd_ode_multistep_step(x.data_ptr(), sc, G, hist.data_ptr(), coef, int(have), B, L, Cn, stream)
        out = (x, hist)
    elif name == "prior":
        x.fill_(float("nan"))
        rc, out = lib.ffd_prior(d, x.data_ptr(), z, G, SEED, off, B, L, Cn, stream), (x,)
    elif name == "langevin":
        work = torch.empty(int(lib.ffd_langevin_work_bytes(B, L)) // 8 + 1, device=dev, dtype=torch.float64)
        eps = torch.empty(B, device=dev)
        rc = lib.ffd_langevin_step(d, x.data_ptr(), sc, G, T, h, SNR, N.FFD_LANGEVIN_NORM_SAMPLE, z, SEED, off, 0x80000002, B,
                                   L, Cn, eps.data_ptr(), work.data_ptr(), stream)
        out = (x, eps)
    else:
        raise KeyError(name)
    assert rc == 0, (name, rc)
    return out


DRAWING = ("sde_step", "forward_transition", "prior", "langevin")
OPERATORS = [(op, dr) for op in DRAWING for dr in ("inject", "device")] + [
    ("forward_transition_noiseless", "inject")] + [
    (op, None) for op in ("ode_step", "ode_heun_predict", "ode_heun_correct", "multistep_first", "multistep_prev")]
CHUNK = 128


@pytest.fixture(scope="module", params=[(1026, 1024, 4), (1368, 1024, 3)], ids=["vec_1026x1024x4", "scalar_1368x1024x3"])
def big_inputs(request):
    shape = request.param
    assert shape[0] * shape[1] * shape[2] == 4202496 > 4096 * 256 * 4
    assert CHUNK * shape[1] * shape[2] <= 4096 * 256  # one pass of every kernel form, float4 or scalar
    return operator_inputs(shape)


@pytest.mark.parametrize("op,draws", OPERATORS, ids=[f"{o}-{d}" if d else o for o, d in OPERATORS])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_second_grid_stride_pass_equals_chunked_calls(ffd, big_inputs, sde, op, draws):
    t = big_inputs
    B, L, _ = t["x"].shape
    sch = scheduler(sde, True, L, N=12)
    keep = {k: v.clone() for k, v in t.items()}
    whole = run_operator(op, sch, t, 0, B, draws or "inject")
    parts = [run_operator(op, sch, t, lo, min(lo + CHUNK, B), draws or "inject") for lo in range(0, B, CHUNK)]
    for k, w in enumerate(whole):
        assert bool(torch.isfinite(w).all()), (op, k)
        assert torch.equal(w, torch.cat([p[k] for p in parts])), (op, k)
    if op == "forward_transition_noiseless":  # s == t: nothing is launched
        assert torch.equal(whole[0], t["x"])  # x keeps its bits
    elif op != "ode_heun_predict":  # (its x is an input)
        assert not torch.equal(whole[0][-2:], t["x"][-2:])  # the last samples, beyond the first pass, moved
    for k, v in keep.items():  # inputs untouched
        assert torch.equal(t[k], v), k


# ------------------------------------------------------ 3. the launcher's float4 conditions ----
@pytest.mark.parametrize("op", DRAWING)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_misaligned_z_gives_the_float4_bits(ffd, sde, op):
    """C % 4 == 0 with z one float off a 16-byte boundary: the launcher takes the scalar kernel, whose bits are the
    float4 kernel's."""
    shape = (3, 20, 4)
    t = operator_inputs(shape, misaligned_z=True)
    assert t["z_off"].data_ptr() % 16 == 4 and t["z"].data_ptr() % 16 == 0 and torch.equal(t["z_off"], t["z"])
    sch = scheduler(sde, True, shape[1], N=12)
    vec = run_operator(op, sch, t, 0, shape[0], "inject", offset=5)
    off = run_operator(op, sch, t, 0, shape[0], "inject", offset=5, z_key="z_off")
    for k, w in enumerate(vec):
        assert torch.equal(w, off[k]), (op, k)


@pytest.mark.parametrize("op", DRAWING)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_odd_element_offsets_draw_what_the_whole_batch_draws(ffd, sde, op):
    """L C = 63: samples 1 and 3 start at odd global elements, so their first draws are the tail of a Philox block.
    Every sample on its own (``sample_offset`` = base + b) gives the whole call's bits, from base 0 and from base 1."""
    shape = (5, 21, 3)
    t = operator_inputs(shape)
    sch = scheduler(sde, True, shape[1], N=12)
    for base in (0, 1):
        whole = run_operator(op, sch, t, 0, shape[0], "device", offset=base)
        parts = [run_operator(op, sch, t, b, b + 1, "device", offset=base) for b in range(shape[0])]
        for k, w in enumerate(whole):
            assert torch.equal(w, torch.cat([p[k] for p in parts])), (op, base, k)
    assert not torch.equal(whole[0], run_operator(op, sch, t, 0, shape[0], "device", offset=0)[0])  # the offset counts
