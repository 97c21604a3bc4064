"""The two vector-instruction cuts in the flagship hot loops, through the C ABI (helpers of test_gpu_parity.py):

  * k_ffn_rows takes its relu as an integer max on the bit pattern (one instruction per element instead of a
    canonicalising float max + the max itself): negatives, -0.0 and +0.0 pre-activations must all come out as +0.0 and
    the layer must still match the oracle, with the same bits for every waves-per-workgroup choice;
  * the two-heads fused attention kernel projects its four remainder features (36 = 2 x 16 + 4) on the 4x4x1 matrix form
    from the x registers the wave already holds: checked against the oracle and against the two-kernel fallback at
    lengths whose last 16-token tile has one live token (tokens past L are clamped inside the tile).
"""
import pytest
import torch

from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O
from test_gpu_parity import TOL_SCORE, _tune_defaults, batch_of, ffd, make_model, make_sd  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ECG = next(c for c in cases.MODEL_CASES if c["name"] == "ecg")
RELU_LAYER = 4
T = 0.4


def tune(**knobs):
    from fastfourierdiffusion_amd import _native as N

    for k, v in knobs.items():
        assert N.lib().ffd_tune(k.encode(), v) == 0, (k, v)


def model_from(sd, c):
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    sch = VPScheduler(fourier_noise_scaling=c["fourier"], **c["sde_kwargs"])
    sch.set_noise_scaling(c["L"])
    m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, fourier_noise_scaling=c["fourier"],
                    d_model=c["d"], num_layers=c["NL"], n_head=c["H"])
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def relu_edge_sd():
    """ECG weights with one layer's linear1 overwritten: units [0, 1000) four times the weights and b1 = -0.5 (most
    pre-activations negative, a few units wide of zero on both sides), units [1000, 1300) zero weights with b1 = +0.0
    and units [1300, 1500) zero weights with b1 = -0.0 (pre-activations exactly +0.0, and -0.0 where the products 0 * x
    are all negative zeros); the rest untouched.  The blocks are not aligned to the kernel's 32-unit chunks."""
    sd = make_sd(ECG)
    w = sd[f"backbone.layers.{RELU_LAYER}.linear1.weight"]
    b = sd[f"backbone.layers.{RELU_LAYER}.linear1.bias"]
    w[:1000] *= 4.0
    b[:1000] = -0.5
    w[1000:1500] = 0.0
    b[1000:1300] = 0.0
    b[1300:1500] = -0.0
    assert torch.signbit(b[1300:1500]).all() and not torch.signbit(b[1000:1300]).any()
    return sd


@pytest.fixture(scope="module")
def relu_case():
    B = 3  # 561 rows: full 32-row wave tiles and a ragged one at 4, 8 and 12 waves per workgroup
    sd = relu_edge_sd()
    x = torch.from_numpy(next(synthetic.noise_stream((B, ECG["L"], ECG["C"]), 1, 5100)))
    ref = O.score_forward(x, torch.full((B,), T, dtype=torch.float32), sd, ECG["NL"], ECG["H"])
    # the oracle's own output for these weights: a usable reference
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0.0
    return sd, x, ref


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "unfused"])
def test_ffn_rows_relu_edges(ffd, relu_case, fuse):
    sd, x, ref = relu_case
    m = model_from(sd, ECG)
    outs = {}
    for nw in (4, 8, 12):
        # k_ffn_rows itself at this small M: no small-M pair, no F slices, no sliced form of it
        tune(attn_small=0, small_path=0, mid_path=0, rows_slices=-1, ffn_rows=2, ffn_rows_fuse=fuse, ffn_rows_nw=nw)
        out = m(batch_of(x.cuda(), T))
        assert torch.isfinite(out).all(), nw
        err = rel_err(out.cpu(), ref)
        print(f"k_ffn_rows relu edges, fuse={fuse} nw={nw}: rel err vs oracle {err:.3e}")
        assert err < TOL_SCORE, (nw, err)
        outs[nw] = out
    assert torch.equal(outs[4], outs[8]) and torch.equal(outs[4], outs[12])
    tune(reset=0)


@pytest.mark.parametrize("L", [17, 33, 187])
def test_two_heads_projection_remainder_features(ffd, L):
    """L = 17 and 33 leave a 16-token tile with one live token; 187 is the flagship length (a tile with 11)."""
    c = dict(ECG, L=L)
    B = 2
    m, _ = make_model(ffd, c)
    sd = make_sd(c)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, c["C"]), 1, 5200 + L)))
    ref = O.score_forward(x, torch.full((B,), T, dtype=torch.float32), sd, c["NL"], c["H"])
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0.0
    outs = {}
    # the default fused attention at this batch (its small-batch split form), the two-heads-per-workgroup kernel the
    # large batches run (the one with the remainder features), and the two-kernel fallback
    for name, knobs in (("default", {}), ("two_heads", dict(attn_small=0)), ("two_kernel", dict(attn_fused=0))):
        tune(reset=0)
        tune(**knobs)
        out = m(batch_of(x.cuda(), T))
        assert torch.isfinite(out).all(), name
        err = rel_err(out.cpu(), ref)
        print(f"attention L={L} {name}: rel err vs oracle {err:.3e}")
        assert err < TOL_SCORE, (name, err)
        outs[name] = out.cpu()
    # the pair's tolerance in the variant tests: each form within TOL_SCORE of the same reference
    for name in ("default", "two_heads"):
        err = rel_err(outs[name], outs["two_kernel"])
        print(f"attention L={L} {name} vs two_kernel: rel err {err:.3e}")
        assert err < TOL_SCORE, (name, err)
    tune(reset=0)
