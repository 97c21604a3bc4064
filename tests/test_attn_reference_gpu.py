"""GPU tests of the fused attention kernels (k_qkv_attention, k_qkv_attention_mh) where their softmax reference leaves
zero, on list E of tests/transformer_restatement.py, judged by its float64 restatement.

The kernels run the online softmax against a reference m_ref that starts at 0 and moves only when a 32-key tile's largest
score is more than T = 64 log2 units from it; networks at the init scale never get there.  The E models shift every score
of a query row by a common amount (which softmax does not see: the fp32 oracle stays within 2.5e-6 of float64, so the
bar is the 1e-5 of every other list): first-tile references upwards and downwards, later-tile refreshes, several in one
row, the maximum in the last key tile, 32-query tiles of which only some rows carry a reference (ref_on with m_ref = 0
lanes), two-heads workgroups of which one head is bounded, and key pieces of the split form that meet in the merge with
different references.  tests/test_attn_reference_host.py certifies on the CPU that every case shows the events it names.

Every case runs the uncached evaluation, then FULL -> PURE -> MIXED -> PURE (the table-reading launches meet non-zero
references), in every attention form of its pair, with run_case's assertions unchanged: a finite score within
max(1e-5, 4 e32) of float64, the tables within 1e-5, the counters, the planned kernel.  The static-bound form must not be
planned: the weights of these models bound nothing within T.  The two pairs without a fused kernel run the same inputs
through k_attention_mfma, whose running maximum starts at -inf: the control that tells an input problem from a kernel
problem.

Not observable here, by design: the factor corr = 2^-delta that rescales what a row accumulated before a later-tile
refresh.  By then those terms are at most 2^-64 of the row, so a wrong finite factor is invisible in fp32; only a
non-finite one would show."""
import pytest

import transformer_restatement as R
from test_gpu_parity import _tune_defaults, batch_of, ffd  # noqa: F401  (fixtures)
from test_transformer_shapes_gpu import WORST, model_of, planned, run_case, set_knobs

pytestmark = pytest.mark.gpu


def pair_of(c):
    m = c["model"]
    return m["d"], m["d"] // m["H"]


def run_form(c, form, knobs, label):
    """One form of one case: never the static-bound instances; then every assertion of run_case."""
    from fastfourierdiffusion_amd import _native as N

    d, hd = pair_of(c)
    two = form == "two_kernel" or (d, hd) not in R.FUSED_PAIRS
    mod = model_of(c)
    set_knobs(knobs)
    for hit in (0, 1):
        name = planned(mod, N.K_ATTN, c["B"], hit)
        assert "<static bound>" not in name, (c["name"], label, name)
    which = f"E d{d} hd{hd} {form}"
    run_case(which, c, knobs, attn=R.K_TWO_KERNEL if two else R.K_FUSED, label=label)
    return WORST[which]


@pytest.mark.parametrize("c", R.E_CASES, ids=lambda c: c["name"])
def test_shifted_scores_vs_float64(ffd, c):
    """Every form the case lists (the split forms at B = 1, the others at B = 3)."""
    for form in c["forms"]:
        run_form(c, form, R.ATTN_FORMS[form], form)


@pytest.mark.parametrize("c", R.E_QG_CASES, ids=lambda c: c["name"])
def test_shifted_scores_with_forced_q_tile_groups_vs_float64(ffd, c):
    """L = 187, one head per workgroup: one, two and three q-tiles per wave share ref_on."""
    for qg in (1, 2, 3):
        run_form(c, "one_head", dict(R.ATTN_FORMS["one_head"], attn_qg=qg), f"one_head attn_qg={qg}")
