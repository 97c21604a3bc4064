"""Host checks of tests/transformer_restatement.py: the float64 judge of the transformer shape tests is pinned to the
reference goldens that tests/test_oracle_golden.py holds the fp32 oracle to, the case lists are what they claim to be,
and on every case of every list the fp32 oracle's own deviation e32 from the judge is at most E32_LIMIT = 2.5e-6 -- so
max(TOL_SCORE, 4 e32), the bar of tests/test_transformer_shapes_gpu.py, is its 1e-5 floor everywhere and no case can hide
behind the maximum.  Nothing of the device enters."""
import math

import numpy as np
import pytest
import torch

import transformer_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

TOL_GOLDEN = 1e-5  # 5 x the single-kernel tolerance: what test_oracle_golden.py allows the fp32 oracle on these goldens
TRANSFORMER_GOLDENS = [c for c in cases.MODEL_CASES if c["kind"] == "transformer"]


@pytest.mark.parametrize("c", TRANSFORMER_GOLDENS, ids=lambda c: c["name"])
def test_judge_against_the_reference_goldens(golden, c):
    """Positional rows, time embedding, the uncached score at every golden time, the cached sequence with its tables and
    counters: the outputs of the unmodified reference."""
    g = golden["g5_models"]
    sd = {k: torch.from_numpy(v.copy()) for k, v in
          synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=c["wseed"]).items()}
    B, L, Cn, d, H, name = c["B"], c["L"], c["C"], c["d"], c["H"], c["name"]
    s64 = R.sd64(sd)
    pos = R.renorm_rows64(s64["pos_encoder.embedding.weight"], math.sqrt(d))
    np.testing.assert_allclose(pos.numpy(), g[f"{name}_pos_fixed"], rtol=0, atol=1e-6)
    x = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, c["xseed"])))
    for tv in c["t_values"]:
        t = torch.full((B,), tv, dtype=torch.float32)
        np.testing.assert_allclose(R.time_embedding64(t, sd, s64, d).numpy(), g[f"{name}_temb_t{tv}"], rtol=0, atol=1e-5)
        assert rel_err(R.score_forward64(x, t, sd, c["NL"], H), g[f"{name}_score_t{tv}"]) < TOL_GOLDEN
    table = R.Table64(c["NL"], H, L, d // H)
    t = torch.full((B,), c["t_values"][0], dtype=torch.float32)
    for j, rec in enumerate(c["cache_seq"]):
        assert list(rec) == list(range(len(rec)))  # (prefixes: the only sets the gate produces)
        xj = torch.from_numpy(next(synthetic.noise_stream((B, L, Cn), 1, c["xseed"] + 100 + j)))
        sc = R.score_forward64(xj, t, sd, c["NL"], H, table, len(rec))
        assert rel_err(sc, g[f"{name}_cseq{j}_score"]) < TOL_GOLDEN, j
        if c.get("dump_table"):
            assert rel_err(table.k, g[f"{name}_cseq{j}_k"]) < TOL_GOLDEN
            assert rel_err(table.v, g[f"{name}_cseq{j}_v"]) < TOL_GOLDEN
        else:
            assert rel_err(table.k[0, 0], g[f"{name}_cseq{j}_k_l0h0"]) < TOL_GOLDEN
            assert rel_err(table.v[-1, -1], g[f"{name}_cseq{j}_v_lNhN"]) < TOL_GOLDEN
    np.testing.assert_array_equal(np.array([table.recompute_count, table.cache_hit_count]), g[f"{name}_cstats"])


def test_time_embedding_argument_is_fp32():
    """With the argument in float64 the judge would sit ~6e-6 from every fp32 implementation: the widened fp32 argument
    keeps the oracle's time embedding within fp32 rounding of the judge's."""
    m = R.model(72, 6, 45)
    sd = R.state_dict(m)
    t = torch.full((3,), R.T_EVAL, dtype=torch.float32)
    j = R.time_embedding64(t, sd, R.sd64(sd), 72)
    o = O.time_embedding(t, sd["time_encoder.W"], sd["time_encoder.dense.weight"], sd["time_encoder.dense.bias"], 72)
    assert rel_err(o, j) < 1e-6
    arg64 = t.double()[:, None] * sd["time_encoder.W"].double()[None, :] * 2 * np.pi
    emb = torch.cat([torch.sin(arg64), torch.cos(arg64)], -1)[:, :72]
    exact = torch.nn.functional.linear(emb, sd["time_encoder.dense.weight"].double(), sd["time_encoder.dense.bias"].double())
    assert rel_err(exact, j) > 1e-6  # the two specifications are distinguishable


def test_case_lists_are_what_they_claim():
    assert len(R.ACCEPTED_PAIRS) == 32 and len(R.FUSED_PAIRS) == 9 and len(R.TWO_KERNEL_PAIRS) == 23
    assert set(R.FUSED_PAIRS) <= set(R.ACCEPTED_PAIRS)
    assert R.ROWS_D == (72, 64, 60, 48)
    # all 18 k_attention_mfma<HD, QG> instances, each with and without tables (every sequence has both)
    inst = {(c["model"]["d"] // c["model"]["H"], c["qg"]) for c in R.A_CASES if "qg" in c}
    assert inst == {(hd, qg) for hd in R.HD_LIST for qg in (1, 2, 3)}
    for c in R.A_CASES:
        assert None in c["seq"] and 0 in c["seq"] and c["model"]["L"] in c["seq"]
    # the cache's mode boundaries (cache_mode of ffd_api.hip: n > 0.8 L is STD-like)
    assert [n for n in R.D_SEQ70 if n and n > 0.8 * 70] == [70, 57] and 56 in R.D_SEQ70
    assert [n for n in R.D_SEQ187 if n and n > 0.8 * 187] == [187, 150] and 149 in R.D_SEQ187
    assert [n for n in R.D_SEQ50 if n and n > 0.8 * 50] == [50, 41] and 40 in R.D_SEQ50
    assert R.short_seq(1) == (None, 1, 0) and R.short_seq(2) == (None, 2, 0, 1, 0)
    assert R.short_seq(5) == (None, 5, 0, 4, 0, 1, 0) and R.short_seq(8) == (None, 8, 0, 6, 0, 1, 0, 7)
    # FFN widths below, at and above the three-slot ring, slot counts no slicing divides, and the batches of the tile heights
    assert {c["model"]["F"] for c in R.B_CASES if c["model"]["d"] == 72} == {64, 128, 192, 256, 320, 1024, 4096}
    assert R.small_splits(135, 256, 640) == 2 and R.small_splits(135, 192, 640) == 0 and R.small_splits(135, 4096, 640) == 16
    for fam in R.FFN_FAMILIES:
        for d in R.STD_HD:
            for Fw in (64, 128, 192, 256, 320, 1024, 4096):
                forms = R.ffn_forms(fam, d, Fw, 135)
                assert forms and all(name is None or name.startswith("k_") for _, name in forms)
    assert R.ffn_forms("ffn_split", 72, 192, 135) == [(dict(ffn_split=1), None)]


@pytest.mark.parametrize("which", sorted(R.ALL_CASES))
def test_fp32_oracle_error_against_the_judge(which):
    """e32 on every evaluation of every case of the list: reported, and at most E32_LIMIT."""
    worst, worst_at, lo = 0.0, None, 1.0
    for c in R.ALL_CASES[which]:
        for j, rec in enumerate(R.reference(c)):
            assert torch.isfinite(rec["score"]).all()
            lo = min(lo, rec["e32"])
            if rec["e32"] > worst:
                worst, worst_at = rec["e32"], (c["name"], j, rec["n"])
            if "score_identity" in rec:  # L = 1: the softmax weight of the only key is 1
                assert rel_err(rec["score_identity"], rec["score"]) < 1e-14, c["name"]
    print(f"list {which}: {len(R.ALL_CASES[which])} cases, e32 {lo:.2e} .. {worst:.2e} (largest at {worst_at})")
    assert worst <= R.E32_LIMIT, (which, worst, worst_at)
    assert R.bar(worst) == R.TOL_SCORE
