"""GPU tests of the transformer kernels at the accepted shapes the rest of the suite never runs, through the Python
surface (which calls libffd's C ABI), judged by the float64 restatement of tests/transformer_restatement.py.

  A  every (d_model, head_dim) pair WITHOUT a fused in-projection + attention kernel (23 of the 32 accepted pairs; derived
     from FFD_D_LIST x FFD_HD_LIST minus FFD_QKV_LIST): k_linear_hm + k_attention_mfma + k_kv_store, without the cache and
     through FULL / PURE / MIXED / STD-like steps; all 18 k_attention_mfma<HD, QG> instances, with and without tables.
  B  dim_feedforward 64 ... 4096: fewer ring slots than k_ffn_rows' ring is deep (64, 128), exactly as many (192), slot
     counts no slicing divides (192, 320), one chunk per k_ffn_ln wave (64); the default plan and every FFN form forced by
     its knobs.  Where a form cannot take the width the plan must name another form, or the call fail loudly.  At
     F = 64, 128, 192 also 98 550 rows, so that workgroups walk several tiles and the weight rings wrap.
  C  L = 1 ... 8 (a lane half of a score tile without a live key; up to 32 samples in a projection tile) in every
     attention form; at L = 1 attention is the identity on v.
  D  recomputed prefixes ending on both sides of the 16-token and 32-key tile edges and of 0.8 L.

Every case asserts: a finite score within max(TOL_SCORE, 4 e32) of the judge's max-norm (e32: the fp32 oracle's own
deviation from the judge; tests/test_transformer_restatement_host.py holds it under 2.5e-6, so the bar is 1e-5); with the
cache on, after every evaluation, cache_tables() within TOL_SCORE of the judge's tables and exact hit / recompute
counters; and, through ffd_kernel_work, that the form the case means to run is the one planned."""
import ctypes as C_
import functools

import pytest
import torch

import transformer_restatement as R
from conftest import rel_err
from test_gpu_parity import _tune_defaults, batch_of, ffd  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
WORST = {}  # list -> largest device error seen (printed per test; DESIGN section 5 quotes them)


def _lib():
    from fastfourierdiffusion_amd import _native as N

    return N.lib()


@functools.lru_cache(maxsize=None)
def _model(mkey):
    """One module per model description (the forms of one shape share it)."""
    from torch import nn

    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    m = dict(mkey, sde_kwargs=R.cases.VP)
    sch = VPScheduler(fourier_noise_scaling=m["fourier"], **m["sde_kwargs"])
    sch.set_noise_scaling(m["L"])
    mod = ScoreModule(n_channels=m["C"], max_len=m["L"], noise_scheduler=sch, fourier_noise_scaling=m["fourier"],
                      d_model=m["d"], num_layers=m["NL"], n_head=m["H"])
    if m["F"] != mod.dim_feedforward:  # the backbone at that width, before the first forward creates the native context
        layer = nn.TransformerEncoderLayer(d_model=m["d"], nhead=m["H"], dim_feedforward=m["F"], batch_first=True)
        mod.backbone = nn.TransformerEncoder(encoder_layer=layer, num_layers=m["NL"])
        mod.dim_feedforward = m["F"]
    mod.load_state_dict(R.state_dict(m), strict=True)
    return mod.cuda().eval()


def model_of(c):
    return _model(tuple(sorted((k, v) for k, v in c["model"].items() if k != "sde_kwargs")))


def set_knobs(knobs):
    lib = _lib()
    assert lib.ffd_tune(b"reset", 0) == 0
    for key, v in knobs.items():
        assert lib.ffd_tune(key.encode(), v) == 0, (key, v)


def planned(mod, cls, B, cache_hit=0):
    fl, by = C_.c_double(), C_.c_double()
    name = _lib().ffd_kernel_work(mod._ctx().handle, cls, B, cache_hit, C_.byref(fl), C_.byref(by))
    return name.decode() if name else None


def assert_plan(mod, B, attn=None, ffn=None):
    """The FFD_K_ATTN name (with and without a pure cache hit), the FFD_K_FFN name and the FFD_K_OUTPROJ launch that goes
    with it, under the knobs now set."""
    from fastfourierdiffusion_amd import _native as N

    if attn is not None:
        for hit in (0, 1):
            name = planned(mod, N.K_ATTN, B, hit)
            assert name == attn or (attn == R.K_FUSED and name.startswith(attn)), (attn, name, hit)
    if ffn is not None:
        assert planned(mod, N.K_FFN, B) == ffn, (ffn, planned(mod, N.K_FFN, B))
        assert planned(mod, N.K_OUTPROJ, B) == (None if ffn in R.OPROJ_INSIDE else "k_linear_res_ln"), ffn


def run_case(which, c, knobs, attn=None, ffn=None, label=""):
    """The case's evaluations under ``knobs``; every assertion of the module docstring.  -> largest score error."""
    mod, ref, B, L = model_of(c), R.reference(c), c["B"], c["model"]["L"]
    set_knobs(knobs)
    assert_plan(mod, B, attn, ffn)
    if mod.cache is None:  # (once per module: the tables stay bound to the first cache; evaluations without
        mod.enable_caching()  # recompute_tokens take the uncached path whether caching is enabled or not)
    mod.cache.reset()
    worst = 0.0
    for j, rec in enumerate(ref):
        x, n = R.inputs(c, j).cuda(), rec["n"]
        out = (mod(batch_of(x, c["t"])) if n is None else mod(batch_of(x, c["t"]), recompute_tokens=set(range(n)), step=j)).cpu()
        where = (c["name"], label, j, n)
        assert torch.isfinite(out).all(), where
        e = rel_err(out, rec["score"])
        worst = max(worst, e)
        assert e <= R.bar(rec["e32"]), (where, e, rec["e32"])
        if L == 1:
            assert rel_err(out, rec["score_identity"]) <= R.bar(rec["e32"]), where
        if n is not None:
            k, v = mod.cache_tables()
            assert rel_err(k.cpu(), rec["k"]) <= R.TOL_SCORE and rel_err(v.cpu(), rec["v"]) <= R.TOL_SCORE, where
            st = mod.cache.get_cache_stats()
            assert (st["recompute_count"], st["cache_hit_count"]) == (rec["recompute"], rec["hits"]), where
    assert _lib().ffd_tune(b"reset", 0) == 0
    WORST[which] = max(WORST.get(which, 0.0), worst)
    print(f"({which}) {c['name']} {label}: largest rel_err vs float64 {worst:.2e} (list so far {WORST[which]:.2e})")
    return worst


# ------------------------------------------------------------------ A: the pairs without a fused kernel
def test_the_pairs_without_a_fused_kernel_are_23():
    """A new fused instance moves a pair out of list A visibly."""
    assert len(R.ACCEPTED_PAIRS) == 32 and len(R.TWO_KERNEL_PAIRS) == 23
    assert len([c for c in R.A_CASES if c["name"].startswith("pair_")]) == 23


@pytest.mark.parametrize("c", R.A_CASES, ids=lambda c: c["name"])
def test_two_kernel_attention_vs_float64(ffd, c):
    """k_linear_hm + k_attention_mfma (+ k_kv_store, the q-only k_linear_hm, the table modes of the attention kernel)."""
    if "attn_qg" in c["knobs"]:
        assert -(-c["model"]["L"] // 32) > 1  # (one q-tile ignores the knob)
    run_case("A", c, c["knobs"], attn=R.K_TWO_KERNEL)


# ------------------------------------------------------------------ B: dim_feedforward
def _b_params():
    for c in R.B_CASES:
        for fam in R.FFN_FAMILIES:
            yield pytest.param(c, fam, id=f"{c['name']}-{fam}")
    for c in R.B_HEIGHT_CASES:
        for fam in ("default", "ffn_ln_oproj", "ffn_height2"):
            yield pytest.param(c, fam, id=f"{c['name']}-{fam}")


@pytest.mark.parametrize("c,family", list(_b_params()))
def test_ffn_forms_at_every_width_vs_float64(ffd, c, family):
    m = c["model"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for knobs, name in R.ffn_forms(family, m["d"], m["F"], c["B"] * m["L"], cus):
        label = " ".join(f"{k}={v}" for k, v in knobs.items()) or "default"
        if name is not None:
            run_case("B", c, knobs, ffn=name, label=label)
            continue
        # the form cannot take the width: the call fails loudly, at once, and leaves the model usable
        set_knobs(knobs)
        with pytest.raises(NotImplementedError, match=r"status -2\): ffn_split"):  # FFD_ERR_UNSUPPORTED
            model_of(c)(batch_of(R.inputs(c, 0).cuda(), c["t"]))
        run_case("B", c, {}, label="after the refused call")


@pytest.mark.parametrize("c", R.B_TILE_CASES, ids=lambda c: c["name"] + "-several_tiles_per_workgroup")
def test_ring_wraps_with_fewer_slots_than_the_ring_is_deep_vs_float64(ffd, c):
    """98 550 rows: every k_ffn_rows workgroup (unfused, fused, one-chunk slots, sliced in rounds) walks several tiles of
    1 ... 4 slots through its three- / four-slot ring, and k_ffn_ln's persistent workgroups wrap their last weight
    prefetch to the next tile's first chunk at 1 / 2 / 3 chunks per wave."""
    assert torch.cuda.get_device_properties(0).multi_processor_count * 384 < c["B"] * c["model"]["L"]
    for knobs, name in R.tile_forms(c["model"]["F"]):
        run_case("B", c, knobs, ffn=name, label=" ".join(f"{k}={v}" for k, v in knobs.items()))


# ------------------------------------------------------------------ C: short sequences
def _c_params():
    for d, hd in R.C_PAIRS:
        for L in R.C_LENGTHS:
            yield pytest.param(d, hd, L, id=f"d{d}_hd{hd}_L{L}")


@pytest.mark.parametrize("d,hd,L", list(_c_params()))
def test_short_sequences_vs_float64(ffd, d, hd, L):
    """B = 1, 3, 33 in every attention form that is a distinct launch for the pair."""
    for c in (c for c in R.C_CASES if c["model"]["d"] == d and c["model"]["H"] == d // hd and c["model"]["L"] == L):
        for form in R.attn_forms_for(d, hd):
            two = form == "two_kernel" or (d, hd) not in R.FUSED_PAIRS
            run_case("C", c, R.ATTN_FORMS[form], attn=R.K_TWO_KERNEL if two else R.K_FUSED, label=form)


# ------------------------------------------------------------------ D: where the prefix ends
def _d_params():
    for c in R.D_CASES:
        m = c["model"]
        for form in c.get("forms", R.attn_forms_for(m["d"], m["d"] // m["H"])):
            yield pytest.param(c, form, id=f"{c['name']}-{form}-n" + "_".join(str(n) for n in c["seq"][1:]))


@pytest.mark.parametrize("c,form", list(_d_params()))
def test_prefix_ends_at_tile_edges_vs_float64(ffd, c, form):
    """The tables are batch element 0's: the error is taken over all five samples."""
    run_case("D", c, R.ATTN_FORMS[form], attn=R.K_TWO_KERNEL if form == "two_kernel" else R.K_FUSED, label=form)
