"""Float64 restatement of LSTMScoreModule.forward (score_models.py:486-511) and the saturated-gate cases built on it.
Shared by tests/test_lstm_restatement_host.py and tests/test_lstm_shapes_gpu.py; torch on the CPU only, no device, and
no code of the library: the embedding is the oracle's ``_embed`` on float64 tensors, the residual stack is an explicit
cell loop (gate order i, f, g, o; zero initial state), the unembedding one matrix product.

Saturation comes from the gate biases, with the weights left at init scale: scaled recurrent weights make the
recurrence chaotic (x16: the fp32 oracle itself is 2e-4 .. 3e-1 off float64), and no kernel can be judged there.
``bias_ih`` of every layer is drawn per element from SAT_PATTERN, which puts 6 of 11 gates beyond |20| (sigmoid and
tanh are then 0 / 1 / -1 to fp32 rounding), two of them at the exp2 overflow edge of the fast activations of
csrc/ffd_lstm.hip (|x| = 88: 2^(88 / ln 2) is the last finite power, 100 overflows), and leaves ``bias_hh`` as
generated.  With these inputs the fp32 oracle stays within 5.5e-6 of float64."""
import functools

import numpy as np
import torch

from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

TOL_SCORE = 1e-5
SAT_PATTERN = (-100.0, -88.0, -30.0, -8.0, -2.0, 0.0, 2.0, 8.0, 30.0, 88.0, 100.0)
EDGE_PATTERN = (-88.0, 88.0, -100.0, 100.0)  # every gate fully open or fully closed, at the overflow edge
SAT_LIMIT = 20.0
ALL_D = (8, 16, 24, 32, 48, 60, 64, 72)   # FFD_D_LIST: the k_lstm_layer<D, BT> instances
WAVE_D = (16, 24, 32, 48, 60, 64, 72)     # the k_lstm_wave<D> / k_pack_lstm_wave<D> instances


def lstm_case(d, NL, L, C, wseed, **extra):
    """A model description in the form tests/test_gpu_parity.py's make_model / make_sd take."""
    return dict(kind="lstm", d=d, H=1, NL=NL, L=L, C=C, sde="vp", sde_kwargs=cases.VP, fourier=True, wseed=wseed, **extra)


def saturate_biases(sd, num_layers, d, pattern=SAT_PATTERN):
    """A copy of the state dict with every layer's ``bias_ih`` drawn per element from ``pattern``
    (``rng.integers`` over the list, PCG64(77 + d)); everything else as generated."""
    rng = np.random.Generator(np.random.PCG64(77 + d))
    vals = np.asarray(pattern, dtype=np.float32)
    out = dict(sd)
    for i in range(num_layers):
        out[f"backbone.{i}.bias_ih_l0"] = torch.from_numpy(vals[rng.integers(0, len(vals), size=4 * d)])
    return out


def lstm_score_forward64(x, t, sd, num_layers):
    """-> (score (B, L, C) float64, share of gate pre-activations with |value| > SAT_LIMIT over all layers and steps)."""
    sd = {k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}
    x, t = x.to(torch.float64), t.to(torch.float64)
    d = sd["embedder.weight"].shape[0]
    h = O._embed(x, t, sd, d, with_pos=False)
    B, L, _ = h.shape
    n_sat = n_all = 0
    for i in range(num_layers):
        p = f"backbone.{i}."
        w_ih, w_hh = sd[p + "weight_ih_l0"], sd[p + "weight_hh_l0"]
        b = sd[p + "bias_ih_l0"] + sd[p + "bias_hh_l0"]
        hs = torch.zeros(B, d, dtype=torch.float64)
        cs = torch.zeros(B, d, dtype=torch.float64)
        out = torch.empty_like(h)
        for s in range(L):
            pre = h[:, s] @ w_ih.T + hs @ w_hh.T + b  # (B, 4d): i, f, g, o
            n_sat += int((pre.abs() > SAT_LIMIT).sum())
            n_all += pre.numel()
            gi, gf, gg, go = pre[:, :d], pre[:, d:2 * d], pre[:, 2 * d:3 * d], pre[:, 3 * d:]
            cs = cs / (1.0 + torch.exp(-gf)) + torch.tanh(gg) / (1.0 + torch.exp(-gi))
            hs = torch.tanh(cs) / (1.0 + torch.exp(-go))
            out[:, s] = hs
        h = h + out
    return h @ sd["unembedder.weight"].T + sd["unembedder.bias"], n_sat / n_all


# The saturated cases of the device test (d): every d_model at NL = 2, L = 37, C = 3, B = 19, the full-depth shape of
# cmd/conf/score_model/lstm.yaml, and one case with every gate at the overflow edge (d = 60: the ragged tile shares).
T_SAT = 0.45
SAT_CASES = [lstm_case(d, 2, 37, 3, 700 + d, name=f"sat_d{d}", B=19, xseed=800 + d, pattern=SAT_PATTERN) for d in ALL_D]
SAT_CASES.append(lstm_case(72, 10, 251, 4, 791, name="sat_d72_nl10_L251", B=3, xseed=891, pattern=SAT_PATTERN))
SAT_CASES.append(lstm_case(60, 2, 37, 3, 792, name="edge_d60", B=19, xseed=892, pattern=EDGE_PATTERN))


def sat_state_dict(c):
    sd = {k: torch.from_numpy(v.copy()) for k, v in synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=c["wseed"]).items()}
    return saturate_biases(sd, c["NL"], c["d"], c["pattern"])


def sat_input(c):
    return torch.from_numpy(next(synthetic.noise_stream((c["B"], c["L"], c["C"]), 1, c["xseed"])))


@functools.lru_cache(maxsize=None)
def sat_reference(name):
    """-> (float64 score, saturation share, e_ref = the fp32 oracle's error against it relative to its max-norm);
    computed once per case and shared by the tests (treat the tensors as read-only)."""
    c = next(c for c in SAT_CASES if c["name"] == name)
    sd, x = sat_state_dict(c), sat_input(c)
    t = torch.full((c["B"],), T_SAT, dtype=torch.float32)
    ref64, share = lstm_score_forward64(x, t, sd, c["NL"])
    o32 = O.lstm_score_forward(x, t, sd, c["NL"]).to(torch.float64)
    e_ref = float((o32 - ref64).abs().max() / ref64.abs().max())
    return ref64, share, e_ref


def sat_bound(e_ref):
    """Four times the reference's own fp32 error, floored at the score bar (the rule of the spectral goldens)."""
    return max(TOL_SCORE, 4.0 * e_ref)
