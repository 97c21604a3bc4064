"""GPU tests of the LSTM kernels (csrc/ffd_lstm.hip) at every d_model instance, at the length edges and with
saturated gates, through the Python surface (helpers of test_gpu_parity.py).

Forms: "wave" is the default selection (k_lstm_wave<D>, weights packed by k_pack_lstm_wave<D>, D in 16 .. 72),
"per_layer" is ffd_tune "lstm_wave" = 0 (k_linear + k_lstm_layer<D, BT>, all of FFD_D_LIST).  Every test asserts through
ffd_kernel_work that the form it means to run is the one planned.

What differs between the instances (and why the shapes are what they are):
  * k_lstm_wave shares NT = D/4 unit tiles over four waves: d = 60 (NT = 15) is the one instance whose last wave holds
    fewer tiles than the register arrays (the `tt < ntw` masks and the clamps of the kernel and the pack), d = 16 gives
    every wave exactly one tile and leaves three of the four input-role waves without a row slot (their `nld` is 0),
    d = 64 fills the 256 row slots exactly, d = 72 alone has two slots per thread;
  * the state block of the time-chunked form (16 D + 4 NTW 64 floats) and the pack sizes are per-D arithmetic:
    lstm_wave_per = 1 forces the hand-over through it at every D;
  * k_lstm_layer pads the per-lane k-slice to whole float4: d = 60 is the padded case with one sample per workgroup,
    d = 16 .. 64 the unpadded ones;
  * the wavefront requests rows tb .. tb+3 before its first barrier, prefetches three steps ahead and publishes from
    t >= tb + 2: L = 1 .. 4 walks every `t + k < te` guard, an odd L in the chunked form ends on a unit of one step;
  * the fast activations rcp(1 + exp2(s x)) are fed, besides init-scale pre-activations, gates far in saturation and at
    the exp2 overflow edge (tests/lstm_restatement.py), judged against float64.

Batches: B = 1 (a partial tile), 16 (an exact tile), 17 (a second tile with one live row), 35 (three tiles, the last
ragged)."""
import ctypes as C_
import functools

import pytest
import torch

import lstm_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import ffd_oracle as O
from test_gpu_parity import TOL_SCORE, _tune_defaults, batch_of, ffd, make_model, make_sd  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TOL_FORMS = 2e-6  # two kernel forms / two batchings of one sample (tests/test_gpu_parity.py)
KERNEL = {"wave": b"k_lstm_wave", "per_layer": b"k_lstm_layer"}
FORMS = ("wave", "per_layer")
T_INIT = 0.45


def _lib():
    from fastfourierdiffusion_amd import _native as N

    return N.lib()


def select(m, form, B):
    """Select `form` (the default, or the per-layer kernels) and assert that it is what the plan runs at batch B."""
    from fastfourierdiffusion_amd import _native as N

    if form == "per_layer":
        assert _lib().ffd_tune(b"lstm_wave", 0) == 0
    ctx = m._ctx()
    fl, by = C_.c_double(), C_.c_double()
    name = ctx.lib.ffd_kernel_work(ctx.handle, N.K_LSTM_REC, B, 0, C_.byref(fl), C_.byref(by))
    assert name == KERNEL[form], (form, B, name)


def run(m, x, tv=T_INIT):
    return m(batch_of(x.cuda(), tv)).cpu()


def init_case(d, L):
    return R.lstm_case(d, 3, L, 3, 900 + d)


@functools.lru_cache(maxsize=None)
def init_reference(d, L, B):
    """(input, fp32 oracle score) of the init-scale model of d_model d at length L: computed once, read-only."""
    c = init_case(d, L)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, c["C"]), 1, 950 + d + 7 * L)))
    ref = O.lstm_score_forward(x, torch.full((B,), T_INIT, dtype=torch.float32), make_sd(c), c["NL"])
    return x, ref


# ------------------------------------------------------------------ (a) every d_model against the oracle
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", R.WAVE_D, ids=lambda d: f"d{d}")
def test_every_d_model_vs_oracle(ffd, d, form):
    """NL = 3, L = 37, C = 3 at B = 1, 16, 17, 35 against the fp32 oracle; a sample of the B = 35 batch equals its
    evaluation in a batch of two."""
    m, _ = make_model(ffd, init_case(d, 37))
    x, ref = init_reference(d, 37, 35)
    worst = 0.0
    for B in (1, 16, 17, 35):
        select(m, form, B)
        out = run(m, x[:B].contiguous())
        assert torch.isfinite(out).all(), (d, form, B)
        e = rel_err(out, ref[:B])
        worst = max(worst, e)
        print(f"(a) d={d} {form} B={B}: rel_err vs oracle {e:.2e}")
        assert e < TOL_SCORE, (d, form, B, e)
    for b in (0, 16, 34):
        lo = min(b, 33)
        two = run(m, x[lo:lo + 2].contiguous())
        assert rel_err(out[b:b + 1], two[b - lo:b - lo + 1]) < TOL_FORMS, (d, form, b)
    print(f"(a) d={d} {form}: largest rel_err {worst:.2e}")


@pytest.mark.parametrize("d", R.WAVE_D, ids=lambda d: f"d{d}")
def test_the_two_forms_agree_at_every_d_model(ffd, d):
    m, _ = make_model(ffd, init_case(d, 37))
    x, _ref = init_reference(d, 37, 35)
    for B in (1, 16, 17, 35):
        xb = x[:B].contiguous()
        select(m, "wave", B)
        w = run(m, xb)
        select(m, "per_layer", B)
        p = run(m, xb)
        assert _lib().ffd_tune(b"reset", 0) == 0
        e = rel_err(w, p)
        print(f"(a) d={d} B={B}: wave vs per_layer {e:.2e}")
        assert e < TOL_FORMS, (d, B, e)


# ------------------------------------------------------------------ (b) every schedule of the wavefront
SCHEDULES = ((0, 0, 16), (1, 1, 16), (2, 1, 2), (1, 1, 36), (3, 1, 0), (0, 1, 1))  # (per, persist, chunk)


@pytest.mark.parametrize("d", R.WAVE_D, ids=lambda d: f"d{d}")
def test_wavefront_schedules_are_bit_identical_at_every_d_model(ffd, d):
    """B = 35, L = 37, NL = 3: a launch per layer group, layers walked whole, and the time-chunked form (chunk 16 ends
    on a unit of 5 steps, chunk 36 on a unit of 1 step, chunk 2 hands the state over 18 times; per = 1 sends every
    hand-over through the per-D state block) give the bits of the default schedule."""
    lib = _lib()
    m, _ = make_model(ffd, init_case(d, 37))
    x, ref = init_reference(d, 37, 35)
    select(m, "wave", 35)
    out = run(m, x)
    assert rel_err(out, ref) < TOL_SCORE, d
    for per, persist, chunk in SCHEDULES:
        assert lib.ffd_tune(b"lstm_wave_per", per) == 0 and lib.ffd_tune(b"lstm_wave_persist", persist) == 0
        assert lib.ffd_tune(b"lstm_wave_chunk", chunk) == 0
        select(m, "wave", 35)
        assert torch.equal(run(m, x), out), (d, per, persist, chunk)


# ------------------------------------------------------------------ (c) short and odd lengths
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", (16, 60, 72), ids=lambda d: f"d{d}")
@pytest.mark.parametrize("L", (1, 2, 3, 4, 5, 16, 17), ids=lambda L: f"L{L}")
def test_short_and_odd_lengths_vs_oracle(ffd, L, d, form):
    """B = 17, NL = 3.  The wavefront's units of fewer than four steps: the row requests `tb + k < te`, the wait for
    min(tb + 4, te) published rows, the last row's store from ring slot s2; chunk 2 with one layer in flight makes every
    unit two steps long (one step at the end of an odd L) and must give the same bits.  max_len = 1 is a supported
    length (one cell step from the zero state)."""
    lib = _lib()
    B = 17
    m, _ = make_model(ffd, init_case(d, L))
    x, ref = init_reference(d, L, B)
    select(m, form, B)
    out = run(m, x)
    assert torch.isfinite(out).all()
    e = rel_err(out, ref)
    print(f"(c) d={d} L={L} {form}: rel_err vs oracle {e:.2e}")
    assert e < TOL_SCORE, (d, L, form, e)
    if form == "wave" and L >= 4:
        assert lib.ffd_tune(b"lstm_wave_chunk", 2) == 0 and lib.ffd_tune(b"lstm_wave_per", 1) == 0
        select(m, form, B)
        assert torch.equal(run(m, x), out), (d, L)


# ------------------------------------------------------------------ (d) saturated gates, judged in float64
def _sat_params():
    for c in R.SAT_CASES:
        for form in FORMS:
            if form == "wave" and c["d"] not in R.WAVE_D:
                continue  # d_model 8 has the per-layer kernels only
            yield pytest.param(c, form, id=f"{c['name']}-{form}")


@pytest.mark.parametrize("c,form", list(_sat_params()))
def test_saturated_gates_vs_float64(ffd, c, form):
    """Gate biases from the saturating pattern (6 of 11 values beyond |20|, two of them at the exp2 overflow edge of
    sigmoid_fast / tanh_fast; the edge case holds every gate there): the output is finite and within
    max(TOL_SCORE, 4 e_ref) of the float64 restatement, e_ref being the fp32 oracle's own error on that case."""
    ref64, share, e_ref = R.sat_reference(c["name"])
    assert share >= 0.40, (c["name"], share)
    m, _ = make_model(ffd, c)
    m.load_state_dict(R.sat_state_dict(c), strict=True)
    select(m, form, c["B"])
    out = run(m, R.sat_input(c), R.T_SAT)
    assert torch.isfinite(out).all(), (c["name"], form)
    e = rel_err(out, ref64)
    print(f"(d) {c['name']} {form}: rel_err vs float64 {e:.2e} (e_ref {e_ref:.2e}, share {share:.3f}, bound {R.sat_bound(e_ref):.1e})")
    assert e <= R.sat_bound(e_ref), (c["name"], form, e, e_ref)
