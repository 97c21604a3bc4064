"""The static score bound of the fused attention kernels and the scalar-base ring DMA of k_ffn_rows, through the C ABI
(helpers of test_gpu_parity.py).

Layers whose weights bound every attention score within the kernels' threshold (ffd_host_attn_score_bound, evaluated
by ffd_finalize_weights) run instances without the per-launch bound.  A static bound is never smaller than the measured
one, so wherever it holds the measured test would have passed too and the same arithmetic runs: knob "attn_static_bound"
on and off must give the same bits -- in every kernel form, in a layer that falls back, with K/V tables (which force
the measuring form) and along a trajectory.  k_ffn_rows now issues its ring's LDS-DMA pieces from a scalar base: every
form of it must still be independent of the waves-per-workgroup choice and match the oracle."""
import ctypes as C_

import pytest
import torch

from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O
from test_gpu_parity import TOL_SCORE, _tune_defaults, batch_of, ffd, make_model, make_sd  # noqa: F401  (fixtures)
from test_hot_loop_vector_cuts import model_from, tune

pytestmark = pytest.mark.gpu

ECG = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")      # d72 / hd6: two-heads kernel, split forms
SMALL = next(c for c in cases.MODEL_CASES if c["name"] == "small")  # d24 / hd6: one head per workgroup only
T = 0.4


def attn_name(m, B):
    from fastfourierdiffusion_amd import _native as N

    fl, by = C_.c_double(), C_.c_double()
    return N.lib().ffd_kernel_work(m._ctx().handle, N.K_ATTN, B, 0, C_.byref(fl), C_.byref(by)).decode()


def on_off(m, x, **knobs):
    """The score with the static bound on and off under `knobs`; asserts the static form is planned exactly when on."""
    outs = []
    for on in (1, 0):
        tune(reset=0)
        tune(attn_static_bound=on, **knobs)
        assert attn_name(m, x.shape[0]) == ("k_qkv_attention<static bound>" if on else "k_qkv_attention")
        outs.append(m(batch_of(x, T)))
    tune(reset=0)
    return outs


# (case, L, B, knobs): the two-heads kernel at the flagship length (q-tile groups of 3), at L = 70 (groups of 2, a ragged
# key tile) and L = 17 (one live token in the last 16-token tile); the same lengths in the default small-batch split
# form; B = 1: the kv | q pack and the plain split form; one head per workgroup (two q-tile groups of 3) at d72 and d24
SHAPES = [
    ("ecg", 187, 3, dict(attn_small=0)), ("ecg", 70, 2, dict(attn_small=0)), ("ecg", 17, 2, dict(attn_small=0)),
    ("ecg", 187, 3, {}), ("ecg", 70, 2, {}), ("ecg", 17, 2, {}),
    ("ecg", 187, 1, {}), ("ecg", 187, 1, dict(attn_kvq=0)),
    ("ecg", 187, 3, dict(attn_small=0, attn_hpw=1)),
    ("small", 20, 3, dict(attn_small=0)), ("small", 20, 3, {}),
]


@pytest.mark.parametrize("name,L,B,knobs", SHAPES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else str(v))
def test_static_bound_on_equals_off_and_matches_oracle(ffd, name, L, B, knobs):
    c = dict(ECG if name == "ecg" else SMALL, L=L)
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, c["C"]), 1, 6200 + L + B)))
    ref = O.score_forward(x, torch.full((B,), T, dtype=torch.float32), sd, c["NL"], c["H"])
    on, off = on_off(m, x.cuda(), **knobs)
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)
    err = rel_err(on.cpu(), ref)
    print(f"{name} L={L} B={B} {knobs}: rel err vs oracle {err:.3e}")
    assert err < TOL_SCORE, err


def test_layer_over_the_threshold_falls_back_alone(ffd):
    """in_proj_weight x 2 in one layer puts its static bound near 170: that layer measures its bound per launch as
    before (the doubled weights' real scores stay small), the others stay static; same bits as with the knob off."""
    B = 3
    sd = make_sd(ECG)
    sd["backbone.layers.5.self_attn.in_proj_weight"] *= 2.0
    m = model_from(sd, ECG)
    x = torch.from_numpy(next(synthetic.noise_stream((B, ECG["L"], ECG["C"]), 1, 6300)))
    ref = O.score_forward(x, torch.full((B,), T, dtype=torch.float32), sd, ECG["NL"], ECG["H"])
    for knobs in (dict(attn_small=0), {}):
        on, off = on_off(m, x.cuda(), **knobs)
        assert torch.equal(on, off), knobs
        assert rel_err(on.cpu(), ref) < TOL_SCORE, knobs
    # every layer over the threshold: nothing static is planned
    sd = make_sd(ECG)
    for i in range(ECG["NL"]):
        sd[f"backbone.layers.{i}.self_attn.in_proj_weight"] *= 2.0
    m = model_from(sd, ECG)
    assert attn_name(m, B) == "k_qkv_attention"
    ref = O.score_forward(x, torch.full((B,), T, dtype=torch.float32), sd, ECG["NL"], ECG["H"])
    assert rel_err(m(batch_of(x.cuda(), T)).cpu(), ref) < TOL_SCORE


def test_cached_modes_on_equals_off(ffd):
    """FULL -> PURE -> MIXED -> PURE at B = 3, six steps: FULL runs the static instances, the modes that read the K/V
    tables the measuring ones (table rows are projections of another step's hidden state)."""
    B, L, C = 3, ECG["L"], ECG["C"]
    m, _ = make_model(ffd, ECG)
    xs = [torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 6400 + j))).cuda() for j in range(6)]
    runs = {}
    for on in (1, 0):
        tune(reset=0)
        tune(attn_static_bound=on)
        m.enable_caching()
        m.cache.reset()
        runs[on] = [m(batch_of(xs[j], T), recompute_tokens=set(range(n)), step=j)
                    for j, n in enumerate([L, 0, 10, 0, 10, 0])]
        m.disable_caching()
    tune(reset=0)
    for j, (a, b) in enumerate(zip(runs[1], runs[0])):
        assert torch.isfinite(a).all() and torch.equal(a, b), j


def test_trajectory_on_equals_off(ffd):
    """20 sampler steps of the ECG model at B = 4 with injected noise."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    B, L, C, N = 4, ECG["L"], ECG["C"], 20
    m, _ = make_model(ffd, ECG)
    outs = {}
    for on in (1, 0):
        tune(reset=0)
        tune(attn_static_bound=on)
        sampler = DiffusionSampler(score_model=m, sample_batch_size=B, use_cache=False)
        sampler.inject_noise(synthetic.noise_stream((B, L, C), N + 1, 6500))
        outs[on] = sampler.sample(num_samples=B, num_diffusion_steps=N)
    tune(reset=0)
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[1], outs[0])


@pytest.mark.parametrize("d,H,NL", [(72, 12, 10), (60, 12, 3)], ids=["d72", "d60"])
@pytest.mark.parametrize("B", [3, 50])
def test_ffn_rows_forms_independent_of_waves_and_match_oracle(ffd, d, H, NL, B):
    """k_ffn_rows at M = 3 x 187 and 50 x 187 rows (ragged last wave tiles): the fused and the unfused form each give the
    same bits at 4 / 8 / 12 waves per workgroup (the ring pieces a wave fetches change with the count), the sliced form
    is deterministic, and the forms agree to rounding with each other (other summation order) and with the oracle."""
    L, C = 187, 1
    c = dict(kind="transformer", d=d, H=H, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=42 if d == 72 else 760)
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 6600 + d + B)))
    nref = min(B, 3)
    ref = O.score_forward(x[:nref], torch.full((nref,), T, dtype=torch.float32), sd, NL, H)
    base = dict(attn_small=0, small_path=0, mid_path=0, ffn_height=0, ffn_rows=2)  # k_ffn_rows itself at this M
    forms = {}
    for fuse in (1, 0):
        outs = []
        for nw in (4, 8, 12):
            tune(reset=0)
            tune(rows_slices=-1, ffn_rows_fuse=fuse, ffn_rows_nw=nw, **base)
            outs.append(m(batch_of(x.cuda(), T)))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), fuse
        forms[f"fuse{fuse}"] = outs[0]
    for sfuse in (1, 2):
        tune(reset=0)
        tune(rows_slices=3, rows_slices_fuse=sfuse, ffn_rows_nw=8, **base)
        a = m(batch_of(x.cuda(), T))
        assert torch.equal(a, m(batch_of(x.cuda(), T))), sfuse
        forms[f"sliced{sfuse}"] = a
    tune(reset=0)
    for k, v in forms.items():
        assert torch.isfinite(v).all(), k
        err = rel_err(v[:nref].cpu(), ref)
        print(f"k_ffn_rows d={d} B={B} {k}: rel err vs oracle {err:.3e}")
        assert err < TOL_SCORE, (k, err)
        assert rel_err(v.cpu(), forms["fuse1"].cpu()) < 2e-6, k
