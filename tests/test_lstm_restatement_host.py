"""CPU checks of tests/lstm_restatement.py: the float64 restatement is the function the oracle computes (init scale,
every d_model), and the saturated cases of tests/test_lstm_shapes_gpu.py are what they claim to be -- they saturate,
and the fp32 oracle is still a judge there (within TOL_SCORE of float64)."""
import pytest
import torch

import lstm_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import ffd_oracle as O


@pytest.mark.parametrize("d", R.ALL_D)
def test_restatement_equals_the_oracle_at_init_scale(d):
    NL, L, C, B = 3, 37, 3, 5
    sd = {k: torch.from_numpy(v) for k, v in synthetic.lstm_state_dict(C, L, d, NL, seed=600 + d).items()}
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, C), 1, 650 + d)))
    t = torch.full((B,), 0.6, dtype=torch.float32)
    ref64, share = R.lstm_score_forward64(x, t, sd, NL)
    assert ref64.dtype == torch.float64 and ref64.shape == (B, L, C)
    assert share == 0.0, share  # init scale: no gate near saturation
    e_cell, e_stock = rel_err(O.lstm_score_forward(x, t, sd, NL), ref64), rel_err(O.lstm_score_forward_stock(x, t, sd, NL), ref64)
    print(f"d={d}: explicit oracle {e_cell:.2e}, stock nn.LSTM {e_stock:.2e} off float64")
    assert e_cell < R.TOL_SCORE and e_stock < R.TOL_SCORE, (d, e_cell, e_stock)


def test_pattern_is_the_one_documented():
    assert R.SAT_PATTERN == (-100.0, -88.0, -30.0, -8.0, -2.0, 0.0, 2.0, 8.0, 30.0, 88.0, 100.0)
    assert sum(abs(v) > R.SAT_LIMIT for v in R.SAT_PATTERN) == 6
    c = R.SAT_CASES[0]
    plain = {k: torch.from_numpy(v) for k, v in synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=c["wseed"]).items()}
    sat = R.sat_state_dict(c)
    for k in plain:
        if k.endswith("bias_ih_l0"):
            assert set(sat[k].tolist()) <= set(R.SAT_PATTERN) and len(set(sat[k].tolist())) > 4, k
        else:
            assert torch.equal(sat[k], plain[k]), k  # weights and bias_hh as generated


@pytest.mark.parametrize("name", [c["name"] for c in R.SAT_CASES])
def test_saturated_cases_saturate_and_the_oracle_still_judges(name):
    ref64, share, e_ref = R.sat_reference(name)
    print(f"{name}: share of |pre-activation| > {R.SAT_LIMIT:g}: {share:.3f}, fp32 oracle off float64: {e_ref:.2e}, "
          f"max-norm {float(ref64.abs().max()):.2f}")
    assert torch.isfinite(ref64).all()
    assert share >= 0.40, (name, share)  # 6 of 11 pattern values: ~0.55 expected (1.0 for the edge pattern)
    assert e_ref < R.TOL_SCORE, (name, e_ref)
