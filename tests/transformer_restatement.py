"""Float64 restatement of ScoreModule.forward (score_models.py:79-194) with and without the E2-CRF cache, and the case
lists of the transformer shape tests.  Shared by tests/test_transformer_restatement_host.py and
tests/test_transformer_shapes_gpu.py; torch on the CPU only, no device, no code of the library.

The judge follows the definitions oracle/ffd_oracle.py states: embedding, positional rows renormalised to sqrt(d) (the
fixed point of nn.Embedding(max_norm)), Gaussian Fourier time embedding, post-norm encoder layers (softmax(q k^T /
sqrt(hd)) v, out-projection, LayerNorm eps 1e-5, ReLU FFN), the four cached layer modes (FULL / STD-like / PURE / MIXED,
cached_transformer.py:139-305) over a float64 K/V table of its own, unembedding.  The oracle's dtype-generic pieces
(``_layer_params``, ``_split_heads``, ``_post_attention``) are called on float64 tensors; torch's default dtype is
never touched.

One thing is specification and not arithmetic: the time embedding's ARGUMENT is ((t W) 2) pi in fp32, product by
product (transformer.py:77-91, k_time_embed) -- W has magnitudes of ~30, so the fp32 products differ from the exact
ones by ~6e-6, which sin / cos pass on undiminished.  The judge computes that argument in fp32, widens it and evaluates
sin / cos and everything after in float64.

The bar of the device tests is ``bar(e32) = max(TOL_SCORE, 4 e32)`` of the judge's max-norm, e32 being the fp32 oracle's
own deviation from the judge on the same case (the rule of tests/lstm_restatement.py); the host test holds e32 under
E32_LIMIT on every case, so the bar is its floor everywhere.

Case lists (plain data; a case = model dict, batch, input seed, time, the evaluations ``seq`` -- None: without the
cache, n: cached with the prefix {0 .. n-1} recomputed -- and the ffd_tune knobs):
  A_CASES  every (d_model, head_dim) pair without a fused in-projection + attention kernel, k_attention_mfma's instances
  B_CASES  dim_feedforward from one ring slot to 64, every FFN form
  C_CASES  L = 1 .. 8
  D_CASES  prefix lengths at the tile edges and at 0.8 L
  E_CASES  attention scores far from the fused kernels' softmax reference 0, by a shift common to each query row, with
           the float64 certificate score_events64 of what the kernels' reference rule meets (tests/test_attn_reference_*.py)
"""
import functools
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from fastfourierdiffusion_amd.utils import synthetic
from oracle import cases
from oracle import ffd_oracle as O

TOL_SCORE = 1e-5
E32_LIMIT = 2.5e-6
T_EVAL = 0.7
NL, C = 2, 2
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastfourierdiffusion_amd", "csrc")


def bar(e32):
    return max(TOL_SCORE, 4.0 * e32)


# ---------------------------------------------------------------------------------------------- the float64 judge
class Table64:
    """K/V tables (NL, H, L, hd) float64 holding batch element 0's projections, and the two counters (caching.py:88-91,
    283, 299, 396)."""

    def __init__(self, num_layers, n_head, max_len, hd):
        self.k = torch.zeros(num_layers, n_head, max_len, hd, dtype=torch.float64)
        self.v = torch.zeros(num_layers, n_head, max_len, hd, dtype=torch.float64)
        self.recompute_count = 0
        self.cache_hit_count = 0


def sd64(sd):
    return {k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}


def renorm_rows64(w, max_norm, max_iter=8):
    """Rows with |w| > max_norm scaled by max_norm / (|w| + 1e-7), to the fixed point (torch embedding_renorm_)."""
    w = w.clone()
    for _ in range(max_iter):
        norms = w.norm(2, dim=1)
        mask = norms > max_norm
        if not bool(mask.any()):
            break
        w[mask] = w[mask] * (max_norm / (norms[mask] + 1e-7))[:, None]
    return w


def time_embedding64(t, sd, s64, d):
    """The argument in fp32 (see the module docstring), sin / cos / dense in float64."""
    arg = (t.to(torch.float32)[:, None] * torch.as_tensor(sd["time_encoder.W"]).to(torch.float32)[None, :] * 2 * np.pi)
    assert arg.dtype == torch.float32
    arg = arg.to(torch.float64)
    emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)[:, :d]
    return F.linear(emb, s64["time_encoder.dense.weight"], s64["time_encoder.dense.bias"])


def _attention64(q, k, v, softmax_one):
    if softmax_one:  # one key: its weight is 1 whatever the score
        assert k.shape[-2] == 1
        return v.expand(-1, -1, q.shape[-2], -1).clone()
    s = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    return torch.matmul(torch.softmax(s, dim=-1), v)


def layer64(src, p, H, layer, table, n, softmax_one=False, probe=None):
    """One encoder layer; table None: the plain layer, else the cached mode of |recompute| = n (a prefix).  ``probe``, if
    given, is called with (layer, q, k) -- the (B, H, L, hd) queries and the keys the attention runs on."""
    B, L, d = src.shape
    hd = d // H
    wq, wk, wv = p["in_w"].split(d, dim=0)
    bq, bk, bv = p["in_b"].split(d, dim=0)
    heads = lambda x: O._split_heads(x, H)  # noqa: E731
    q = heads(F.linear(src, wq, bq))
    if table is None or n == L or n > 0.8 * L:
        k_own = heads(F.linear(src, wk, bk))
        if probe is not None:
            probe(layer, q, k_own)
        out = O._post_attention(src, _attention64(q, k_own, heads(F.linear(src, wv, bv)), softmax_one), p)
        if table is not None and n == L:  # FULL: K, V of the layer OUTPUT, batch element 0
            table.k[layer] = heads(F.linear(out, wk, bk))[0]
            table.v[layer] = heads(F.linear(out, wv, bv))[0]
            table.recompute_count += L
        return out
    k_full = table.k[layer].unsqueeze(0).expand(B, -1, -1, -1).clone()
    v_full = table.v[layer].unsqueeze(0).expand(B, -1, -1, -1).clone()
    table.cache_hit_count += L - n
    if n > 0:  # MIXED: the prefix from the layer INPUT, per sample; batch element 0's rows go into the table
        k_full[:, :, :n] = heads(F.linear(src[:, :n], wk, bk))
        v_full[:, :, :n] = heads(F.linear(src[:, :n], wv, bv))
        table.k[layer][:, :n] = k_full[0, :, :n]
        table.v[layer][:, :n] = v_full[0, :, :n]
        table.recompute_count += n
    if probe is not None:
        probe(layer, q, k_full)
    return O._post_attention(src, _attention64(q, k_full, v_full, softmax_one), p)


def score_forward64(x, t, sd, num_layers, n_head, table=None, n=None, softmax_one=False, probe=None):
    """-> score (B, L, C) float64.  x (B, L, C), t (B,) fp32; ``table`` / ``n`` select the cached path; ``probe``: layer64."""
    s64 = sd64(sd)
    d = s64["embedder.weight"].shape[0]
    h = F.linear(x.to(torch.float64), s64["embedder.weight"], s64["embedder.bias"])
    h = h + renorm_rows64(s64["pos_encoder.embedding.weight"], math.sqrt(d))[None, : x.shape[1], :]
    h = h + time_embedding64(t, sd, s64, d)[:, None, :]
    for i in range(num_layers):
        h = layer64(h, O._layer_params(s64, i), n_head, i, table if n is not None else None, n, softmax_one, probe)
    return F.linear(h, s64["unembedder.weight"], s64["unembedder.bias"])


# ---------------------------------------------------------------------------------------------- shapes of the build
def _macro_list(fname, macro, which=r"X2?"):
    """The (...) argument tuples of ``#define macro(...) X(a[, b]) ...`` in a csrc file."""
    with open(os.path.join(_CSRC, fname)) as f:
        line = next(ln for ln in f if ln.startswith(f"#define {macro}("))
    body = line.split(")", 1)[1]
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(which + r"\(([\d, ]+)\)", body)]


D_LIST = tuple(v[0] for v in _macro_list("ffd_internal.h", "FFD_D_LIST"))
HD_LIST = tuple(v[0] for v in _macro_list("ffd_internal.h", "FFD_HD_LIST"))
FUSED_PAIRS = tuple(_macro_list("ffd_qkvattn.hip", "FFD_QKV_LIST"))  # (d_model, head_dim) with a k_qkv_attention instance
TWO_HEAD_PAIRS = tuple(_macro_list("ffd_qkvattn.hip", "FFD_QKV_LIST", "X2"))  # ... with a two-heads-per-workgroup instance
ACCEPTED_PAIRS = tuple((d, hd) for d in D_LIST for hd in HD_LIST if d % hd == 0)
TWO_KERNEL_PAIRS = tuple(p for p in ACCEPTED_PAIRS if p not in FUSED_PAIRS)
ROWS_D = (72, 64, 60, 48)  # d_model values with a k_ffn_rows instance (FFD_ROWS_D_LIST)


# ---------------------------------------------------------------------------------------------- cases
def model(d, hd, L, Fw=2048):
    return dict(kind="transformer", d=d, H=d // hd, NL=NL, L=L, C=C, F=Fw, sde="vp", sde_kwargs=cases.VP, fourier=True,
                wseed=5000 + 7 * d + 131 * hd + L + Fw // 64)


def case(name, m, B, seq, knobs=None, **extra):
    return dict(name=name, model=m, B=B, xseed=9000 + 3 * m["d"] + m["L"] + 17 * B, t=T_EVAL, seq=tuple(seq),
                knobs=dict(knobs or {}), **extra)


def cached_seq(L):
    """FULL, PURE, MIXED just past a 16-token tile, MIXED at 0.8 L (still MIXED), STD-like (no store)."""
    return (None, L, 0, min(17, L), 0, int(0.8 * L), 0, L - 3)


# A: every pair without a fused kernel at L = 45 (two q-tiles, a ragged last key tile), B = 3 (135 rows: k_linear_hm's
# 32-row tiles straddle samples and end ragged); one pair per head_dim at L = 20, 70 (QG 1, 3 by the heuristic) and with
# attn_qg forced at L = 45 and 300 (q-tile counts the group size does not divide; ten groups on four waves)
A_SEQ45 = (None, 45, 0, 17, 0, 36, 0, 42)
HD_PAIRS = ((72, 2), (48, 3), (24, 4), (60, 5), (48, 6), (72, 8))  # (60, 5) has a fused kernel: run under attn_fused = 0
A_CASES = [case(f"pair_d{d}_hd{hd}_L45", model(d, hd, 45), 3, A_SEQ45, dict(attn_fused=0) if (d, hd) in FUSED_PAIRS else {})
           for d, hd in TWO_KERNEL_PAIRS]
for _d, _hd in HD_PAIRS:
    _kn = dict(attn_fused=0) if (_d, _hd) in FUSED_PAIRS else {}
    for _L, _qg in ((20, 1), (70, 3)):
        A_CASES.append(case(f"hd{_hd}_QG{_qg}_heuristic_d{_d}_L{_L}", model(_d, _hd, _L), 3, cached_seq(_L), _kn, qg=_qg))
    for _L in (45, 300):
        for _qg in (1, 2, 3):
            A_CASES.append(case(f"hd{_hd}_QG{_qg}_forced_d{_d}_L{_L}", model(_d, _hd, _L), 3, cached_seq(_L),
                                dict(_kn, attn_qg=_qg), qg=_qg))

# B: the FFN widths.  Only the model, batch and the uncached evaluation are data here; the knob sets of the forms are
# ffn_forms() below (they depend on the width)
STD_HD = {72: 6, 60: 5, 48: 4, 64: 8, 32: 8, 16: 4, 24: 3, 8: 2}  # head dims of tests/test_gpu_parity.py's _SHAPES
B_WIDTHS = {d: (64, 128, 192, 256, 320, 1024, 4096) if d in (72, 60) else (64, 192, 320) for d in STD_HD}
B_HEIGHT_BATCHES = (50, 183)  # 141 / 515 16-row tiles: one 16-row, one 48-row k_ffn_ln tile per CU (ffn_height_plan at 256 CUs)
B_CASES = [case(f"d{d}_F{Fw}_B{B}", model(d, STD_HD[d], 45, Fw), B, (None,))
           for d in STD_HD for Fw in B_WIDTHS[d] for B in ((3, 19) if d == 72 else (3,))]
B_HEIGHT_CASES = [case(f"d{d}_F{Fw}_B{B}", model(d, STD_HD[d], 45, Fw), B, (None,))
                  for d in (72, 60) for Fw in B_WIDTHS[d] for B in B_HEIGHT_BATCHES if B == 50 or Fw <= 320]


# Several tiles per workgroup at the narrow widths: where a ring wraps.  B = 2190 at L = 45 is 98 550 rows: 257 tiles of
# 384 rows for k_ffn_rows' one 12-wave workgroup per CU (770 tiles of 128 rows at four waves), 1540 64-row tiles for
# k_ffn_ln's persistent grid of two workgroups per CU (256 CUs) -- so the slot a workgroup prefetches past its tile's end
# is the next tile's first, with fewer slots per tile than the ring is deep (k_ffn_rows: 1 / 2 / 3 chunk slots at F = 64 /
# 128 / 192, one more with the out-projection slot) and k_ffn_ln's last prefetch wrapping at 1 / 2 / 3 chunks per wave
B_TILE_BATCH = 2190
B_TILE_CASES = [case(f"d72_F{Fw}_B{B_TILE_BATCH}", model(72, 6, 45, Fw), B_TILE_BATCH, (None,)) for Fw in (64, 128, 192)]


def tile_forms(Fw):
    """[(knobs, FFD_K_FFN name)] of B_TILE_CASES: every k_ffn_rows form whose workgroups walk several tiles, and the
    persistent k_ffn_ln."""
    off = dict(small_path=0, mid_path=0, ffn_height=0)
    forms = [(dict(off, ffn_rows=2, rows_slices=-1, ffn_rows_fuse=fuse, ffn_rows_nw=nw), K_ROWS_OP if fuse else K_ROWS)
             for fuse in (0, 1) for nw in (4, 12)]
    forms.append((dict(off, ffn_rows=2, rows_slices=-1, ffn_rows_cps=1, ffn_rows_nw=4), K_ROWS))
    if Fw // 64 >= 2:  # the sliced form in rounds, one or two slots per slice
        forms += [(dict(off, rows_slices=2, rows_slices_fuse=fuse, ffn_rows_nw=12), K_SL_OP if fuse == 1 else K_SL) for fuse in (1, 2)]
    forms += [(dict(ONLY_LN, ffn_mb=4, ffn_rem=rem), K_LN) for rem in (0, 1)]
    return forms


def small_splits(M, Fw, cap):
    """F splits of the small-M pair under a workgroup cap (small_path_splits): the largest power of two ns <= 16 that
    divides F / 64, keeps tiles x ns under the cap and leaves 2, 4, 8 or 16 chunks per wave; 0: the pair cannot take F."""
    tiles = -(-M // 16)
    for ns in (16, 8, 4, 2):
        if (Fw // 64) % ns == 0 and tiles * ns <= cap and Fw // (64 * ns) in (2, 4, 8, 16):
            return ns
    return 0


K_LN, K_LN_OP, K_SMALL, K_PART, K_SPLIT = "k_ffn_ln", "k_ffn_ln<oproj>", "k_oproj_ffn_split + k_ffn_reduce_ln", "k_ffn_part", "k_ffn_ln_split"
K_ROWS, K_ROWS_OP = "k_ffn_rows", "k_ffn_rows<oproj>"
K_SL, K_SL_OP = "k_ffn_rows<sliced> + k_rows_reduce_ln", "k_ffn_rows<oproj, sliced> + k_rows_reduce_ln"
OPROJ_INSIDE = (K_LN_OP, K_SMALL, K_ROWS_OP, K_SL_OP)  # the others run behind k_linear_res_ln
ONLY_LN = dict(ffn_rows=0, small_path=0, mid_path=0, ffn_height=0)  # k_ffn_ln behind k_linear_res_ln, whatever M
FFN_FAMILIES = ("default", "ffn_ln", "ffn_ln_oproj", "ffn_height2", "ffn_persist0", "ffn_rows", "ffn_rows_sliced", "ffn_part",
                "ffn_small", "ffn_split")


def height_plan(M, cus):
    """16-row tiles per k_ffn_ln workgroup where there are 0.55 - 3 of them per CU (ffn_height_plan), else 0."""
    t16 = -(-M // 16)
    if 20 * t16 >= 11 * cus and t16 <= cus:
        return 1
    if 4 * t16 >= 5 * cus and t16 <= 2 * cus:
        return 2
    return 3 if 2 * cus < t16 <= 3 * cus else 0


def ffn_forms(family, d, Fw, M, cus=256):
    """[(knobs, FFD_K_FFN name the plan must give | None: the call must fail with FFD_ERR_UNSUPPORTED)] of a family at
    (d_model, F) and M rows, for a chip of ``cus`` compute units.  Where a form cannot take the width (or, the tile
    heights, the batch) the name is the form the plan falls through to.  At the batches of these lists the default plan
    is the one-launch tile heights where ffn_height_plan gives one, else the small-M pair where it takes F, else k_ffn_ln
    (the sliced k_ffn_rows and the F slices lose their estimates below a few thousand rows)."""
    nslots, ring, hp = Fw // 64, d in ROWS_D, height_plan(M, cus)
    no_height = K_SMALL if small_splits(M, Fw, 5 * cus // 2) or small_splits(M, Fw, 6 * cus) else K_LN
    if family == "default":
        return [({}, K_LN_OP if hp else no_height)]
    if family == "ffn_ln":
        return [(dict(ONLY_LN, ffn_mb=mb, ffn_rem=rem), K_LN) for mb in (1, 2, 3, 4) for rem in (0, 1)]
    if family == "ffn_ln_oproj":
        return [(dict(ffn_height=1, ffn_rem=rem), K_LN_OP if hp else no_height) for rem in (1, 0)]
    if family == "ffn_height2":
        return [(dict(ffn_height=2, ffn_rem=rem), K_LN if hp else no_height) for rem in (1, 0)]
    if family == "ffn_persist0":
        return [(dict(ONLY_LN, ffn_mb=4, ffn_persist=0), K_LN)]
    off = dict(small_path=0, mid_path=0, ffn_height=0)
    if family == "ffn_rows":
        forms = [(dict(off, ffn_rows=2, rows_slices=-1, ffn_rows_fuse=fuse, ffn_rows_nw=nw),
                  (K_ROWS_OP if fuse else K_ROWS) if ring else K_LN) for fuse in (0, 1) for nw in (4, 8, 12)]
        if d == 72:
            forms += [(dict(off, ffn_rows=2, rows_slices=-1, ffn_rows_cps=1, ffn_rows_nw=nw), K_ROWS) for nw in (4, 12)]
        return forms
    if family == "ffn_rows_sliced":
        forms = []
        for S in sorted({2, 3, nslots} - {0, 1}):
            if S > 32:
                continue  # (not a value the knob takes)
            for fuse in (1, 2):
                for nw in (8, 12):
                    ok = ring and S <= min(nslots, 16)
                    forms.append((dict(off, rows_slices=S, rows_slices_fuse=fuse, ffn_rows_nw=nw),
                                  (K_SL_OP if fuse == 1 else K_SL) if ok else K_LN))
        return forms
    if family == "ffn_part":
        return [(dict(small_path=0, ffn_height=0, rows_slices=-1, mid_path=ns), K_PART if nslots % ns == 0 else K_LN)
                for ns in (2, 4, 8)]
    if family == "ffn_small":
        tiles, forms = -(-M // 16), []
        for ns in (16, 8, 4, 2):  # small_wgs = tiles x ns admits exactly ns splits: 2, 4, 8, 16 chunks per wave
            admitted = small_splits(M, Fw, tiles * ns)
            forms.append((dict(small_wgs=tiles * ns, rows_slices=-1, mid_path=0, ffn_height=0), K_SMALL if admitted else K_LN))
        return forms
    if family == "ffn_split":
        return [(dict(ffn_split=1), K_SPLIT if Fw % 128 == 0 else None)]
    raise KeyError(family)


# C: short sequences.  The nine fused pairs and two without a fused kernel; every attention form
ATTN_FORMS = dict(default={}, one_head=dict(attn_small=0, attn_hpw=1), two_heads=dict(attn_small=0, attn_hpw=2),
                  split2=dict(attn_small=2, attn_kvq=0), split2_kvq=dict(attn_small=2, attn_kvq=1),
                  split4=dict(attn_small=4, attn_kvq=0), split4_kvq=dict(attn_small=4, attn_kvq=1),
                  two_kernel=dict(attn_fused=0))
K_TWO_KERNEL, K_FUSED = "k_linear_hm + k_attention_mfma", "k_qkv_attention"  # FFD_K_ATTN names (the fused one: a prefix)


def attn_forms_for(d, hd):
    """The attention forms that are distinct launches for the pair: no fused kernel -> the two-kernel path only; the
    two-heads workgroups and the kv | q pack of the split form exist for some pairs only (the knob is ignored elsewhere)."""
    if (d, hd) not in FUSED_PAIRS:
        return ("default", "two_kernel")
    forms = ["default", "one_head"] + (["two_heads"] if (d, hd) in TWO_HEAD_PAIRS else []) + ["split2", "split4"]
    if 2 * hd <= 16 < 3 * hd:  # attn_kvq_supported
        forms += ["split2_kvq", "split4_kvq"]
    return tuple(forms + ["two_kernel"])


C_PAIRS = FUSED_PAIRS + ((72, 8), (24, 4))
C_LENGTHS = (1, 2, 3, 4, 5, 8)
C_BATCHES = (1, 3, 33)


def short_seq(L):
    """The uncached evaluation, then [L, 0, floor(0.8 L), 0, 1, 0, floor(0.8 L) + 1] without the prefix lengths that repeat
    or leave [0, L] (a zero stays unless it follows a zero): floor(0.8 L) is the last MIXED value, the next one STD-like."""
    out = [None]
    for n in (L, 0, int(0.8 * L), 0, 1, 0, int(0.8 * L) + 1):
        if n > L or (n in out and n != 0) or (n == 0 and out[-1] == 0):
            continue
        out.append(n)
    return tuple(out)


C_CASES = [case(f"d{d}_hd{hd}_L{L}_B{B}", model(d, hd, L), B, short_seq(L)) for d, hd in C_PAIRS for L in C_LENGTHS
           for B in C_BATCHES]

# D: where the recomputed prefix ends.  56 = 0.8 x 70 is MIXED, 57 the first STD-like value; 149 / 150 the same at 187
D_SEQ70 = (None, 70, 0, 1, 0, 15, 16, 17, 0, 31, 32, 33, 0, 55, 56, 57, 0)
D_SEQ187 = (None, 187, 0, 149, 0, 150, 0)
D_SEQ50 = (None, 50, 0, 1, 0, 15, 16, 17, 0, 31, 32, 33, 0, 39, 40, 41, 0)  # 40 = 0.8 x 50
D_CASES = [case("d72_hd6_L70_B5", model(72, 6, 70), 5, D_SEQ70), case("d72_hd6_L187_B5", model(72, 6, 187), 5, D_SEQ187),
           case("d60_hd5_L50_B5", model(60, 5, 50), 5, D_SEQ50, forms=("two_heads",))]

# E: scores far from the fused kernels' softmax reference 0, by a shift COMMON to a query row's scores -- softmax does not
# see it, so the differences stay at the init scale and fp32 and float64 agree as on every other list (e32 under
# E32_LIMIT, held by tests/test_attn_reference_host.py).  A model with ``shift`` (shift_state_dict) has
#   * the embedding's column space to the data alone: positional rows, embedding bias and time embedding are projected
#     onto its orthogonal complement, so that u_c . h = x[..., c] exactly for the dual vectors u_c of the embedding;
#   * per head h, by h mod 6 (h mod 4 where H = 4), in dimension 0 of the head (rows h hd of the q and k blocks):
#       const    q row = k row = 0, biases a and +- a: every score is +- a^2 / sqrt(hd) (+- S in log2 units) plus the rest,
#                in EVERY layer and for table rows too (the bias survives the K projection of another hidden state);
#                S = 200 / 150 (x ``shift``) beyond the threshold T = 64 -- and beyond fp32's exponent range, so that a missing
#                reference overflows or loses the row --, S = 25 within it;
#       ramp_k   (layer 0) q row = 0, q bias g, k row = g u_0, k bias g o: score = 72 (x[key, 0] + o) log2 units, the same for
#                every query; channel 0 of the E inputs is a staircase over the key positions (e_inputs), so the key
#                tiles' maxima rise by 72 > T from one plateau to the next; o = -2 in the second such head starts the row
#                with a NEGATIVE reference;
#       ramp_q   (layer 0) k row = 0, k bias g, q row = g u_1: score = 170 x[query, 1], the same for every key; channel 1 is
#                -1, 0, 1, -1 ... over the positions, so adjacent query rows of one 32-query tile refresh downwards, not
#                at all, upwards;
#       plain    untouched (a head the norm product bounds, next to one it does not).
# The fp32 error of a score grows with its magnitude (an ulp of 1000 log2 units is 6e-5), so the shifts are no larger than
# the events need: with constants of 400 and plateaus of 80 up to 320 the oracle's e32 reached 3.3e-6 on some cases; at
# the values here it is at most 2.1e-6.
# The kernels' rule on these scores is restated by score_events64; each case names the events it must show.
LOG2E = 1.4426950408889634
ATTN_T = 64.0      # ATTN_SCORE_T of csrc/ffd_internal.h
EVENT_MARGIN = 1.0  # an event counts only where every comparison of its row is this far (log2 units) from its threshold
E_STEPS = (32, 66, 170, 500)  # channel 0 rises by 1 there: at a tile edge, inside tile 2, in the last tile of L = 187 and of L = 512
E_NOISE = 0.02     # what is left of the noise in the two channels the ramps read
E_RAMP_K, E_RAMP_Q = 72.0, 170.0  # (170: outside fp32's exponent range on both sides, like the constants)
E_KINDS6 = ("const+", "plain", "const-", "ramp_k", "const_small", "ramp_q")
E_KINDS4 = ("const+", "const-", "ramp_k", "ramp_q")
EVENTS = ("first_pos", "first_neg", "later", "multi", "none", "last_tile_max", "mixed_qtile", "bound_mixed", "split2_merge",
          "split4_merge")


def head_plan(H, shift=1.0):
    """[(kind, parameter)] per head: const -> the signed shift in log2 units, ramp_k -> the plateau offset o."""
    kinds = E_KINDS4 if H < 8 else E_KINDS6
    plan = []
    for h in range(H):
        kind, rep = kinds[h % len(kinds)], h // len(kinds)
        if kind == "const+":
            plan.append(("const", shift * (200.0, 150.0)[rep % 2]))
        elif kind == "const-":
            plan.append(("const", -shift * (200.0, 150.0)[rep % 2]))
        elif kind == "const_small":
            plan.append(("const", (25.0, -25.0)[rep % 2]))
        elif kind == "ramp_k":
            plan.append(("ramp_k", (0.0, -2.0)[rep % 2]))
        else:
            plan.append((kind, 0.0))
    return plan


def shift_state_dict(sd, m):
    """The E model of the comment above, in place on a state dict of fp32 tensors."""
    d, H = m["d"], m["H"]
    hd, qs = d // H, LOG2E / math.sqrt(d // H)
    We = sd["embedder.weight"].double()  # (d, C)
    G = torch.linalg.inv(We.T @ We)
    U = We @ G  # column c: u_c . (We x) = x[c]
    Pc = torch.eye(d, dtype=torch.float64) - We @ G @ We.T  # onto the complement of the embedding's column space
    sd["pos_encoder.embedding.weight"] = (sd["pos_encoder.embedding.weight"].double() @ Pc).float()
    for key in ("embedder.bias", "time_encoder.dense.weight", "time_encoder.dense.bias"):
        sd[key] = (Pc @ sd[key].double()).float()
    for i in range(m["NL"]):
        W, b = sd[f"backbone.layers.{i}.self_attn.in_proj_weight"], sd[f"backbone.layers.{i}.self_attn.in_proj_bias"]
        for h, (kind, par) in enumerate(head_plan(H, m["shift"])):
            rq, rk = h * hd, d + h * hd
            if kind == "const":
                a = math.sqrt(abs(par) / qs)
                W[rq], W[rk], b[rq], b[rk] = 0.0, 0.0, a, math.copysign(a, par)
            elif kind == "ramp_k" and i == 0:
                g = math.sqrt(E_RAMP_K / qs)
                W[rq], b[rq], W[rk], b[rk] = 0.0, g, (g * U[:, 0]).float(), g * par
            elif kind == "ramp_q" and i == 0:
                g = math.sqrt(E_RAMP_Q / qs)
                W[rk], b[rk], W[rq], b[rq] = 0.0, g, (g * U[:, 1]).float(), 0.0
    return sd


def e_inputs(x):
    """Channel 0: the staircase of E_STEPS; channel 1: -1, 0, 1 over the positions; E_NOISE of the noise on top of both."""
    pos = torch.arange(x.shape[1])
    stairs = sum((pos >= s).to(x.dtype) for s in E_STEPS)
    x = x.clone()
    x[..., 0] = E_NOISE * x[..., 0] + stairs
    x[..., 1] = E_NOISE * x[..., 1] + ((pos % 3) - 1).to(x.dtype)
    return x


def _walk(tmax):
    """The kernels' reference rule over the key tiles of one piece.  tmax (..., nt): the tiles' largest score per query row
    -> dict(mref, n (refreshes), first_pos, first_neg, later, sure (every comparison EVENT_MARGIN from its threshold))."""
    shape = tmax.shape[:-1]
    mref, n = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.int64)
    sure = torch.ones(shape, dtype=torch.bool)
    first_pos = first_neg = later = torch.zeros(shape, dtype=torch.bool)
    for t in range(tmax.shape[-1]):
        b = tmax[..., t] - mref
        v = b.abs() if t == 0 else b  # the first tile refreshes on |max| > T, later ones on max > T
        refresh = v > ATTN_T
        sure = sure & ((v - ATTN_T).abs() >= EVENT_MARGIN)
        if t == 0:
            first_pos, first_neg = refresh & (b > 0), refresh & (b < 0)
        else:
            later = later | refresh
        mref = torch.where(refresh, mref + b, mref)
        n = n + refresh
    return dict(mref=mref, n=n, first_pos=first_pos, first_neg=first_neg, later=later, sure=sure)


def tile_maxima(s):
    """(..., Lq, Lk) scores -> (..., Lq, KT): the largest score of each 32-key tile (the ragged last one: its live keys)."""
    Lk = s.shape[-1]
    KT = -(-Lk // 32)
    pad = torch.full(s.shape[:-1] + (KT * 32 - Lk,), -math.inf, dtype=s.dtype)
    return torch.cat([s, pad], dim=-1).reshape(s.shape[:-1] + (KT, 32)).amax(dim=-1)


def row_events(tmax):
    """Event counts of score rows given by their tile maxima (..., Lq, KT), Lq rows making 32-query tiles in order."""
    KT = tmax.shape[-1]
    w = _walk(tmax)
    sure, n = w["sure"], w["n"]
    ev = dict(first_pos=w["first_pos"] & sure, first_neg=w["first_neg"] & sure, later=w["later"] & sure,
              multi=(n >= 2) & sure, none=(n == 0) & sure)
    if KT >= 2:
        ev["last_tile_max"] = tmax[..., -1] >= tmax[..., :-1].amax(dim=-1) + EVENT_MARGIN
    out = {k: int(v.sum()) for k, v in ev.items()}
    Lq = tmax.shape[-2]
    padq = (-Lq) % 32
    tiles = lambda a: torch.cat([a, torch.zeros(a.shape[:-1] + (padq,), dtype=torch.bool)], -1).reshape(a.shape[:-1] + (-1, 32))  # noqa: E731
    out["mixed_qtile"] = int((tiles(ev["none"]).any(-1) & tiles((n >= 1) & sure).any(-1)).sum())
    for kspl in (2, 4):  # the split form: each key piece starts from reference 0 on its own first tile
        kps = -(-KT // kspl)
        pieces = [_walk(tmax[..., p * kps: min(KT, (p + 1) * kps)]) for p in range(kspl) if p * kps < KT]
        hit = torch.zeros(tmax.shape[:-1], dtype=torch.bool)
        for i, a in enumerate(pieces):
            for c in pieces[i + 1:]:
                gap = (a["mref"] - c["mref"]).abs()
                hit = hit | (a["sure"] & c["sure"] & (a["mref"] != 0) & (c["mref"] != 0) & (gap > 0) & (gap < 20.0))
        out[f"split{kspl}_merge"] = int(hit.sum())
    return out


def score_events64(q, k):
    """The events of one layer's attention: q, k (B, H, L, hd) float64 as layer64's probe hands them over.  Scores in the
    kernels' log2 domain, q k^T log2(e) / sqrt(hd); bound_mixed: workgroups of heads (2 g, 2 g + 1) of which one is within
    T by the kernel's product of the largest |q| and the largest |k| (head_bounded) and one is not."""
    qs = LOG2E / math.sqrt(q.shape[-1])
    out = row_events(tile_maxima(torch.matmul(q, k.transpose(-2, -1)) * qs))
    r = qs * q.norm(dim=-1).amax(dim=-1) * k.norm(dim=-1).amax(dim=-1)  # (B, H)
    inside, outside = r <= ATTN_T - EVENT_MARGIN, r >= ATTN_T + EVENT_MARGIN
    H2 = q.shape[1] // 2 * 2
    out["bound_mixed"] = int(((inside[:, 0:H2:2] & outside[:, 1:H2:2]) | (outside[:, 0:H2:2] & inside[:, 1:H2:2])).sum())
    return out


def e_model(d, hd, L, nl=1, shift=1.0):
    return dict(model(d, hd, L), NL=nl, shift=shift)


def e_seq(L):
    """The uncached evaluation, FULL, PURE, MIXED with a prefix of 17 (of 0.8 L where 17 is no longer MIXED), PURE."""
    return (None, L, 0, 17 if 17 <= 0.8 * L else int(0.8 * L), 0)


def e_events(d, hd, L, split):
    """The events a case of the pair at length L must show (split: the forms whose key pieces merge)."""
    ev = ["first_pos", "first_neg", "none", "mixed_qtile"] + (["bound_mixed"] if (d, hd) in TWO_HEAD_PAIRS else [])
    if L > 32:
        ev += ["later", "last_tile_max"] + (["split2_merge", "split4_merge"] if split else [])
    if L > 66:
        ev += ["multi"]
    return tuple(ev)


E_LENGTHS = (17, 33, 70, 187)  # the first key tile is the ragged last one; one live key in the last tile; 3 and 6 tiles
E_LONG_PAIRS = ((72, 6), (64, 8))  # ... and L = 512 (16 tiles; four q-tiles per wave at head_dim 6)
E_NL2_PAIRS = ((60, 5), (24, 3), (72, 6))
E_CONTROL_PAIRS = ((72, 8), (24, 4))  # no fused kernel: k_attention_mfma's running maximum starts at -inf
E_CASES = []
for _d, _hd in FUSED_PAIRS + E_CONTROL_PAIRS:
    _forms = attn_forms_for(_d, _hd)
    _split = tuple(f for f in _forms if f.startswith("split"))
    for _L in E_LENGTHS:
        E_CASES.append(case(f"E_d{_d}_hd{_hd}_L{_L}_B3", e_model(_d, _hd, _L), 3, e_seq(_L),
                            forms=tuple(f for f in _forms if f not in _split), events=e_events(_d, _hd, _L, False)))
        if _split:
            E_CASES.append(case(f"E_d{_d}_hd{_hd}_L{_L}_B1", e_model(_d, _hd, _L), 1, e_seq(_L), forms=_split,
                                events=e_events(_d, _hd, _L, True)))
for _d, _hd in E_LONG_PAIRS:
    E_CASES.append(case(f"E_d{_d}_hd{_hd}_L512_B3", e_model(_d, _hd, 512), 3, e_seq(512), forms=("default", "one_head"),
                        events=e_events(_d, _hd, 512, False)))
for _d, _hd in E_NL2_PAIRS:
    E_CASES.append(case(f"E_d{_d}_hd{_hd}_L70_B3_NL2", e_model(_d, _hd, 70, nl=2), 3, e_seq(70),
                        forms=tuple(f for f in attn_forms_for(_d, _hd) if not f.startswith("split")),
                        events=e_events(_d, _hd, 70, False)))
# the constant shifts five times as large (up to 1000 log2 units), in every form
E_CASES.append(case("E_d72_hd6_L187_B3_shift5", e_model(72, 6, 187, shift=5.0), 3, e_seq(187),
                    forms=("default", "one_head", "two_heads", "two_kernel"), events=e_events(72, 6, 187, False)))
E_CASES.append(case("E_d72_hd6_L187_B1_shift5", e_model(72, 6, 187, shift=5.0), 1, e_seq(187),
                    forms=("split2", "split4", "split2_kvq", "split4_kvq"), events=e_events(72, 6, 187, True)))
E_QG_CASES = [c for c in E_CASES if c["model"]["L"] == 187 and c["B"] == 3 and c["model"]["shift"] == 1.0
              and (c["model"]["d"], c["model"]["d"] // c["model"]["H"]) in FUSED_PAIRS]  # attn_qg 1 / 2 / 3 forced, one_head form

ALL_CASES = dict(A=A_CASES, B=B_CASES + B_HEIGHT_CASES + B_TILE_CASES, C=C_CASES, D=D_CASES, E=E_CASES)


# ---------------------------------------------------------------------------------------------- references
def state_dict(m):
    sd = synthetic.transformer_state_dict(m["C"], m["L"], m["d"], m["NL"], dim_feedforward=m["F"], seed=m["wseed"])
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    return shift_state_dict(sd, m) if "shift" in m else sd


def inputs(c, j):
    m = c["model"]
    x = torch.from_numpy(next(synthetic.noise_stream((c["B"], m["L"], m["C"]), 1, c["xseed"] + j)))
    return e_inputs(x) if "shift" in m else x


@functools.lru_cache(maxsize=None)
def _reference(mkey, B, xseed, t, seq):
    m = dict(mkey)
    m["sde_kwargs"] = cases.VP
    c = dict(model=m, B=B, xseed=xseed)
    sd = state_dict(m)
    L, H, hd = m["L"], m["H"], m["d"] // m["H"]
    tt = torch.full((B,), t, dtype=torch.float32)
    tab64, tab32, tab_id = Table64(m["NL"], H, L, hd), O.KVTable(m["NL"], L), Table64(m["NL"], H, L, hd)
    out = []
    for j, n in enumerate(seq):
        x = inputs(c, j)
        events = {}  # list E: score_events64 summed over the layers, with the largest |score| in log2 units

        def probe(layer, q, k):
            for name, v in score_events64(q, k).items():
                events[name] = events.get(name, 0) + v
            top = float((torch.matmul(q, k.transpose(-2, -1)).abs().max()) * LOG2E / math.sqrt(hd))
            events["max_log2"] = max(events.get("max_log2", 0.0), top)

        s64 = score_forward64(x, tt, sd, m["NL"], H, tab64, n, probe=probe if "shift" in m else None)
        s32 = O.score_forward(x, tt, sd, m["NL"], H, tab32 if n is not None else None, list(range(n)) if n is not None else None)
        rec = dict(n=n, score=s64, e32=float((s32.to(torch.float64) - s64).abs().max() / s64.abs().max()))
        if L == 1:  # attention is the identity on v
            rec["score_identity"] = score_forward64(x, tt, sd, m["NL"], H, tab_id, n, softmax_one=True)
        if events:
            rec["events"] = events
        if n is not None:
            rec.update(k=tab64.k.clone(), v=tab64.v.clone(), recompute=tab64.recompute_count, hits=tab64.cache_hit_count)
            assert (tab32.recompute_count, tab32.cache_hit_count) == (tab64.recompute_count, tab64.cache_hit_count)
        out.append(rec)
    return tuple(out)


def reference(c):
    """Per evaluation of the case: dict(n, score (float64), e32, and with the cache: k, v (the judge's tables after the
    evaluation), recompute, hits; list E: events).  Computed once per (model, batch, inputs, sequence); read-only."""
    mkey = tuple(sorted((k, v) for k, v in c["model"].items() if k != "sde_kwargs"))
    return _reference(mkey, c["B"], c["xseed"], c["t"], c["seq"])
