"""The two-partition sampling loops (ffd_tune "partitions") at the plans and sizes they run at.

Every case asks ffd_partition_plan what the call will do -- the decision, each half's forms for half the CUs and the FFN
grid its launcher computes -- asserts that this is the form the case means to run, and that ffd_partition_status agrees
afterwards.

  1  every eligible form pinned by its knobs so that a half (128 CUs) and the whole batch (256 CUs) plan the same kernel
     instance: "partitions" = 2 gives the bits of "partitions" = 0 and of two single-stream calls on the halves with
     their global sample offsets.  Regime a: an odd batch, one workgroup per tile in both halves.  Regime b: the smallest
     batch at which BOTH halves' FFN grids are the persistent ones sized from the budget (found through the query and
     asserted: 526 for k_ffn_rows at 12 waves), so that workgroups of both halves walk several tiles at the same time.
  2  the default knobs where "partitions" = 1 engages: the decision over B = 340 ... 1100 against a restatement of the
     fill rule and of rows_waves at 128 CUs; the runs at the sweep's picks judged per sample by the float64 walk.
  3  calls: n_run against PART_CHUNK, trajectories continued over calls, workspace growth between partitioned calls,
     DiffusionSampler.
  4  what stays single-stream, and that an eligible call partitions again afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ode_restatement as ODE
import pc_restatement as PC
import philox_restatement as PR
import transformer_restatement as R
from fastfourierdiffusion_amd import _native as N
from fastfourierdiffusion_amd.utils import synthetic
from oracle import ffd_oracle as O

pytestmark = pytest.mark.gpu

STEPS, GRID, SEED, OFFSET = 3, 8, 42, 5
VP = dict(beta_min=0.1, beta_max=20.0)
ENTRY = {"sde": N.FFD_SOLVER_EULER_MARUYAMA, "ode_euler": N.FFD_SOLVER_ODE_EULER}
ENTRIES = sorted(ENTRY)
# no small- / mid-batch or sliced FFN form, no tile heights, no split attention: what is left is pinned by the knobs alone
OFF = dict(rows_slices=-1, small_path=0, mid_path=0, ffn_height=0, attn_small=0)
MODELS = {
    "ecg": dict(L=187, C=1, d=72, H=12, NL=2, F=2048),
    "d64": dict(L=45, C=2, d=64, H=64 // R.STD_HD[64], NL=2, F=2048),
    "d60": dict(L=45, C=2, d=60, H=60 // R.STD_HD[60], NL=2, F=2048),
    "d48": dict(L=45, C=2, d=48, H=48 // R.STD_HD[48], NL=2, F=2048),
    "d24hd4": dict(L=24, C=3, d=24, H=6, NL=2, F=2048),  # (24, 4) has no fused attention kernel
}


def rows(nw, fuse=1, **kw):
    return dict(OFF, ffn_rows=2, ffn_rows_nw=nw, ffn_rows_fuse=fuse, **kw)


def ln(mb, persist=1, **kw):
    return dict(OFF, ffn_rows=0, ffn_mb=mb, ffn_persist=persist, **kw)


ECG_KNOBS = rows(4)


@pytest.fixture(autouse=True)
def _knobs_back():
    yield
    N.lib().ffd_tune(b"reset", 0)


@functools.lru_cache(maxsize=None)
def model(kind):
    """(module on the device, timesteps, step size, state dict on the host, scheduler)"""
    from torch import nn

    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    c = MODELS[kind]
    sch = VPScheduler(fourier_noise_scaling=True, **VP)
    sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], dim_feedforward=c["F"], seed=42)
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"], n_head=c["H"])
    if c["F"] != m.dim_feedforward:
        layer = nn.TransformerEncoderLayer(d_model=c["d"], nhead=c["H"], dim_feedforward=c["F"], batch_first=True)
        m.backbone = nn.TransformerEncoder(encoder_layer=layer, num_layers=c["NL"])
        m.dim_feedforward = c["F"]
    sch.set_noise_scaling(c["L"])
    m.load_state_dict(sd, strict=True)
    sch.set_timesteps(GRID)
    return m.cuda().eval(), (C.c_float * GRID)(*sch.timesteps.tolist()), float(sch.step_size), sd, sch


def prior(kind, B, seed=1234):
    c = MODELS[kind]
    return torch.from_numpy(next(synthetic.noise_stream((B, c["L"], c["C"]), 1, seed))).cuda()


def tune(knobs, partitions):
    lib = N.lib()
    assert lib.ffd_tune(b"reset", 0) == 0
    for k, v in dict(knobs, partitions=partitions).items():
        assert lib.ffd_tune(k.encode(), v) == 0, k


def status(ctx):
    parts = C.c_int(0)
    assert ctx.lib.ffd_partition_status(ctx.handle, C.byref(parts)) == 0
    return parts.value


def call(kind, x, entry, first=1, n_run=STEPS, offset=OFFSET, g0=0, z=None):
    """n_run iterations of `entry` from `first`, in place on x, under the knobs now set -> ffd_partition_status."""
    m, ts, h = model(kind)[:3]
    ctx = m._ctx()
    s = N.current_stream_ptr(x.device)
    if entry == "sde":
        rc = ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, first, n_run, SEED, offset,
                                      z.data_ptr() if z is not None else None, 0, g0, s)
    else:
        rc = ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, first, n_run, ENTRY[entry], 0, g0, s)
    N.check(rc, ctx.handle, entry)
    return status(ctx)


def plan(kind, B, entry="sde"):
    """ffd_partition_plan under the knobs now set"""
    ctx = model(kind)[0]._ctx()
    info = N.PartitionInfo()
    N.check(ctx.lib.ffd_partition_plan(ctx.handle, B, ENTRY.get(entry, entry), C.byref(info)), ctx.handle, "ffd_partition_plan")
    assert (info.half[0].nb, info.half[1].nb, info.whole.nb) == ((B + 1) // 2, B // 2, B)
    return info


def sig(h):
    """the kernel instances of a plan (not its grid)"""
    return (h.ffn.decode(), h.attn.decode(), h.nw, h.cps, h.mb, h.persist, h.hpw, h.qg, h.kspl)


def budget():
    return torch.cuda.get_device_properties(0).multi_processor_count // 2


def assert_wanted(h, want):
    got = dict(ffn=h.ffn.decode(), attn=h.attn.decode(), nw=h.nw, cps=h.cps, mb=h.mb, persist=h.persist, hpw=h.hpw, qg=h.qg,
               kspl=h.kspl, part_floats=h.part_floats)
    for k, v in want.items():
        assert got[k] == v, (k, v, got)


def eligible_plan(kind, B, entry, knobs, want):
    """The knobs with "partitions" = 2: the query says two partitions, both halves and the whole batch plan the wanted
    instance.  -> info"""
    tune(knobs, 2)
    info = plan(kind, B, entry)
    assert info.parts == 2 and info.cu_budget == budget() and info.halves_planned == 1 and info.whole_planned == 1
    for h in info.half:
        assert h.attn.decode() == R.K_FUSED and h.part_floats == 0
        assert_wanted(h, want)
        assert sig(h) == sig(info.whole), (sig(h), sig(info.whole))
    return info


def three_way(kind, B, entry, knobs, want, halves_must_match=True, first=1, n_run=STEPS):
    """"partitions" = 2 == "partitions" = 0 == two single-stream calls on the halves (where a half on its own plans the
    instance the partitioned half runs; halves_must_match: it has to)."""
    info = eligible_plan(kind, B, entry, knobs, want)
    x0 = prior(kind, B)
    one, two = x0.clone(), x0.clone()
    tune(knobs, 0)
    assert plan(kind, B, entry).parts == 1
    assert call(kind, one, entry, first, n_run) == 1
    tune(knobs, 2)
    assert call(kind, two, entry, first, n_run) == info.parts == 2
    torch.cuda.synchronize()
    assert torch.isfinite(one).all() and not torch.equal(one, x0)
    assert torch.equal(two, one)
    tune(knobs, 0)
    nb0 = (B + 1) // 2
    alone = [sig(plan(kind, nb, entry).whole) == sig(h) for nb, h in zip((nb0, B - nb0), info.half)]
    assert all(alone) or not halves_must_match, alone
    if all(alone):
        a, b = x0[:nb0].clone(), x0[nb0:].clone()
        assert call(kind, a, entry, first, n_run) == 1 and call(kind, b, entry, first, n_run, offset=OFFSET + nb0) == 1
        assert torch.equal(torch.cat([a, b]), two)
    return info


# ------------------------------------------------------------------ 0. the query ----
def test_query_argument_errors_and_what_it_leaves_alone():
    m = model("ecg")[0]
    ctx = m._ctx()
    lib, info = ctx.lib, N.PartitionInfo()
    tune(ECG_KNOBS, 2)
    x = prior("ecg", 8)
    assert call("ecg", x, "sde") == 2
    assert lib.ffd_partition_plan(ctx.handle, 8, ENTRY["sde"], None) == -1
    assert lib.ffd_partition_plan(ctx.handle, 0, ENTRY["sde"], C.byref(info)) == -1
    for entry in (-1, 6, 99):
        assert lib.ffd_partition_plan(ctx.handle, 8, entry, C.byref(info)) == -1
    assert status(ctx) == 2  # the query is not a loop call: the status is still the last loop's
    for entry in (N.FFD_SOLVER_ODE_HEUN, N.FFD_SOLVER_PC, N.FFD_SOLVER_ODE_AB2, N.FFD_SOLVER_DPMPP_2M):
        i = plan("ecg", 8, entry)  # these loops never ask
        assert i.parts == 1 and i.halves_planned == 0 and i.whole_planned == 1 and i.whole.ffn.decode() == R.K_ROWS_OP
    i = plan("ecg", 1)
    assert i.parts == 1 and i.halves_planned == 0  # one sample cannot be halved
    tune(ECG_KNOBS, 0)
    i = plan("ecg", 8)
    assert i.parts == 1 and i.halves_planned == 0 and sig(i.whole)[0] == R.K_ROWS_OP
    tune(ECG_KNOBS, 2)
    i = plan("ecg", 8)
    assert i.parts == 2 and [h.nb for h in i.half] == [4, 4] and i.cu_budget == budget()
    assert [(h.ffn_tiles, h.ffn_grid, h.one_per_tile) for h in i.half] == [(6, 6, 1)] * 2  # 748 rows in 128-row tiles
    assert (i.whole.ffn_tiles, i.whole.ffn_grid, i.whole.one_per_tile) == (12, 12, 1)


# ------------------------------------------------------------------ 1. every eligible form, pinned ----
FORMS_A = {}  # id -> (model, B, knobs, what the plan must say, halves on their own must plan the same instance)
for _nw in (4, 8, 12):
    for _fuse in (1, 0):
        FORMS_A[f"rows_nw{_nw}_{'fused' if _fuse else 'unfused'}"] = (
            "ecg", 5, rows(_nw, _fuse), dict(ffn=R.K_ROWS_OP if _fuse else R.K_ROWS, nw=_nw, cps=2), True)
for _nw in (4, 12):
    FORMS_A[f"rows_nw{_nw}_one_chunk_slots"] = ("ecg", 5, rows(_nw, ffn_rows_cps=1), dict(ffn=R.K_ROWS, nw=_nw, cps=1), True)
for _d in (64, 60, 48):
    for _fuse in (1, 0):
        FORMS_A[f"rows_d{_d}_nw8_{'fused' if _fuse else 'unfused'}"] = (
            f"d{_d}", 5, rows(8, _fuse), dict(ffn=R.K_ROWS_OP if _fuse else R.K_ROWS, nw=8, hpw=1 if _d == 64 else 2), True)
for _mb in (1, 2, 3, 4):
    for _p in (1, 0):
        FORMS_A[f"ln_mb{_mb}_persist{_p}"] = ("ecg", 5, ln(_mb, _p), dict(ffn=R.K_LN, mb=_mb, persist=_p), True)
# the tile heights: batches whose halves (128 CUs) and whole (256 CUs) get the same height from ffn_height_plan -- 117 / 106
# and 223 16-row tiles, 176 / 164 and 339, 281 / 269 and 550.  A half on its own at 256 CUs is below the heights' range.
for _B, _mb in ((19, 1), (29, 2), (47, 3)):
    FORMS_A[f"height1_mb{_mb}"] = ("ecg", _B, dict(ffn_height=1), dict(ffn=R.K_LN_OP, mb=_mb, kspl=0), False)
    FORMS_A[f"height2_mb{_mb}"] = ("ecg", _B, dict(ffn_height=2), dict(ffn=R.K_LN, mb=_mb, kspl=0), False)
FORMS_A["attn_two_heads"] = ("ecg", 5, rows(4, attn_hpw=2), dict(hpw=2, qg=3), True)
for _qg, _want in ((0, 3), (1, 1), (2, 2)):
    FORMS_A[f"attn_one_head_qg{_qg}"] = ("ecg", 5, rows(4, attn_hpw=1, attn_qg=_qg), dict(hpw=1, qg=_want), True)
FORMS_A["attn_d64_one_head_qg1"] = ("d64", 5, rows(4, attn_qg=1), dict(hpw=1, qg=1), True)
for _ft in (0, 1):
    FORMS_A[f"fuse_tail{_ft}_rows"] = ("ecg", 5, rows(12, fuse_tail=_ft), dict(ffn=R.K_ROWS_OP, nw=12), True)
    FORMS_A[f"fuse_tail{_ft}_ln"] = ("ecg", 5, ln(4, fuse_tail=_ft), dict(ffn=R.K_LN, mb=4), True)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("form", sorted(FORMS_A))
def test_regime_a_one_workgroup_per_tile_odd_batch(form, entry):
    kind, B, knobs, want, alone = FORMS_A[form]
    assert B % 2 == 1
    info = three_way(kind, B, entry, knobs, want, halves_must_match=alone)
    assert info.half[0].nb == info.half[1].nb + 1
    for h in info.half:
        assert h.one_per_tile == 1 and h.ffn_grid == h.ffn_tiles > 0


# regime b: (knobs, plan, rows per tile, workgroups per CU the launcher fits, smallest B the issue states or None)
FORMS_B = {
    "rows_nw12_fused": (rows(12), dict(ffn=R.K_ROWS_OP, nw=12, cps=2), 384, 1, 526),
    "rows_nw12_unfused": (rows(12, 0), dict(ffn=R.K_ROWS, nw=12, cps=2), 384, 1, 526),
    "rows_nw12_one_chunk_slots": (rows(12, ffn_rows_cps=1), dict(ffn=R.K_ROWS, nw=12, cps=1), 384, 1, 526),
    "rows_nw8_fused": (rows(8), dict(ffn=R.K_ROWS_OP, nw=8, cps=2), 256, 1, None),
    "rows_nw4_fused": (rows(4), dict(ffn=R.K_ROWS_OP, nw=4, cps=2), 128, None, None),
    "rows_nw12_fused_one_head": (rows(12, attn_hpw=1), dict(ffn=R.K_ROWS_OP, nw=12, hpw=1), 384, 1, 526),
    # (263 x 187 score floats in front of the second half: not a multiple of 4)
    "rows_nw12_fused_separate_unembed": (rows(12, fuse_tail=0), dict(ffn=R.K_ROWS_OP, nw=12), 384, 1, 526),
    "ln_mb4_persist1": (ln(4, 1), dict(ffn=R.K_LN, mb=4, persist=1), 64, 2, None),
    "ln_mb4_persist2": (ln(4, 2), dict(ffn=R.K_LN, mb=4, persist=2), 64, 4, None),
}


@functools.lru_cache(maxsize=None)
def smallest_persistent_batch(form):
    """The smallest B at which both halves' FFN grids are the persistent ones (the smaller half decides)."""
    knobs = FORMS_B[form][0]
    tune(knobs, 2)
    for B in range(2, 1400):
        if all(h.one_per_tile == 0 for h in plan("ecg", B).half):
            return B
    raise AssertionError(form)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("form", sorted(FORMS_B))
def test_regime_b_both_halves_walk_several_tiles_per_workgroup(form, entry):
    knobs, want, tile_rows, per_cu, stated = FORMS_B[form]
    B = smallest_persistent_batch(form)
    if stated is not None:
        assert B == stated
    L, cus = MODELS["ecg"]["L"], budget()
    info = three_way("ecg", B, entry, knobs, want)
    for h in info.half:
        assert h.ffn_tiles == -(-h.nb * L // tile_rows) and h.one_per_tile == 0
        assert h.ffn_grid % cus == 0 and h.ffn_tiles > h.ffn_grid  # the grid is sized from the budget, not the device
        if per_cu is not None:
            assert h.ffn_grid == per_cu * cus
    tune(knobs, 2)  # one sample fewer: the smaller half is back to a workgroup per tile
    assert plan("ecg", B - 2, entry).half[1].one_per_tile == 1
    assert info.whole.one_per_tile == 0 and info.whole.ffn_grid == 2 * info.half[0].ffn_grid


# ------------------------------------------------------------------ 2. the default knobs, where auto engages ----
def rows_waves(M, cus):
    """rows_waves (ffd_ffn_rows.hip): the wave count with the least passes x waves per SIMD / efficiency; ties to more waves"""
    eff, best, nw = (0.85, 0.915, 0.938), 0.0, 0
    for i in (2, 1, 0):
        cand = 4 * (i + 1)
        t = float(-(-(-(-M // (32 * cand))) // cus)) * (i + 1) / eff[i]
        if best == 0.0 or t < best * 0.999:
            best, nw = t, cand
    return nw


def auto_engages(info, L):
    """The decision of "partitions" = 1 restated from the halves' reported forms: eligible forms, the row-owning FFN at
    rows_waves' wave count for half the CUs, and every pass of a half's tiles filling at least 0.9 of them."""
    cus, ok = info.cu_budget, True
    for h in info.half:
        ffn, M = h.ffn.decode(), h.nb * L
        is_rows = ffn in (R.K_ROWS, R.K_ROWS_OP)
        assert not is_rows or -(-M // 64) >= 512  # (ffn_rows_selected under the default knobs)
        ok = ok and h.attn.decode() == R.K_FUSED and h.part_floats == 0 and ffn != R.K_SPLIT and is_rows
        if is_rows:
            assert ffn == R.K_ROWS_OP and h.nw == rows_waves(M, cus) and h.ffn_tiles == -(-M // (32 * h.nw))
            last = h.ffn_tiles % cus
            ok = ok and (last == 0 or 10 * last >= 9 * cus)
    return ok


SWEEP = range(340, 1101)


@functools.lru_cache(maxsize=None)
def sweep():
    """B -> (engages, halves' signatures, whole-batch signature) under the default knobs, both entries agreeing"""
    out, L = {}, MODELS["ecg"]["L"]
    tune({}, 1)
    for B in SWEEP:
        infos = [plan("ecg", B, e) for e in ENTRIES]
        for info in infos:
            assert info.halves_planned == 1 and info.cu_budget == budget()
            assert (info.parts == 2) == auto_engages(info, L), (B, info.parts, [sig(h) for h in info.half])
        assert infos[0].parts == infos[1].parts
        out[B] = (infos[0].parts == 2, tuple(sig(h) for h in infos[0].half), sig(infos[0].whole))
    return out


def test_auto_decision_follows_the_fill_rule_over_the_sweep():
    """The reported decision against the restated rule at every B (sweep()).  On MI355X auto engages at B = 350, 474 ... 524,
    666 ... 700 and 998 ... 1050 (printed below; DESIGN.md, section 3 "The loop")."""
    sw = sweep()
    on = [B for B in SWEEP if sw[B][0]]
    runs, start = [], None
    for B in list(SWEEP) + [None]:
        if B is not None and sw[B][0]:
            start = B if start is None else start
        elif start is not None:
            runs.append((start, (B if B is not None else SWEEP[-1] + 1) - 1))
            start = None
    print(f"auto engages at {len(on)} of {len(SWEEP)} batches in [{SWEEP[0]}, {SWEEP[-1]}]: {runs}")
    differ_nw = [B for B in on if sw[B][1][0][2] != sw[B][1][1][2]]
    differ_whole = [B for B in on if any(s != sw[B][2] for s in sw[B][1])]
    print(f"  engaging batches whose halves plan different wave counts: {differ_nw[:8]} ({len(differ_nw)})")
    print(f"  engaging batches whose half plan is not the whole batch's at 256 CUs: {differ_whole[:8]} ({len(differ_whole)})")
    assert 512 in on and any(B % 2 for B in on) and min(on) >= 350  # (a half below 175 samples has no row-owning FFN)
    tune({}, 1)
    for e in ENTRIES:  # a424e4f: 125 tiles of 384 rows on 128 CUs per half
        info = plan("ecg", 512, e)
        assert info.parts == 2
        for h in info.half:
            assert (h.ffn.decode(), h.nw, h.ffn_tiles, h.one_per_tile) == (R.K_ROWS_OP, 12, 125, 1)


def picks():
    """B = 512, the smallest engaging batch, the smallest odd one, and -- where the sweep has them -- the smallest whose
    halves plan different wave counts and the smallest whose half plan is not the whole batch's."""
    sw = sweep()
    on = [B for B in SWEEP if sw[B][0]]
    out = {"B512": 512, "smallest": on[0], "odd": next(B for B in on if B % 2)}
    nw = [B for B in on if sw[B][1][0][2] != sw[B][1][1][2]]
    whole = [B for B in on if any(s != sw[B][2] for s in sw[B][1])]
    if nw:
        out["halves_differ"] = nw[0]
    if whole:
        out["half_is_not_whole"] = whole[0]
    return out


def walk(kind, x0, samples, entry, dtype):
    """STEPS iterations from step 1 of samples `samples` (global offsets OFFSET + b), on the host in `dtype`"""
    _, ts_c, h, sd, _ = model(kind)
    c = MODELS[kind]
    ts, G = np.array(ts_c[:], dtype=np.float32), ODE.fourier_G(c["L"])
    f64 = dtype == np.float64

    def score(x, t, k=0):
        tt = torch.full((x.shape[0],), float(t), dtype=torch.float32)
        if f64:
            return R.score_forward64(torch.from_numpy(np.asarray(x, np.float64)), tt, sd, c["NL"], c["H"]).numpy()
        return O.score_forward(torch.from_numpy(np.asarray(x, np.float32)), tt, sd, c["NL"], c["H"], None, None).numpy()

    x = np.asarray(x0[samples].cpu().numpy(), dtype)
    if entry == "ode_euler":
        return ODE.integrate("ode_euler", "vp", VP, x, score, ts, h, G, dtype, first=1, n_run=STEPS)
    for i in range(1, 1 + STEPS):
        z = np.concatenate([PR.sample_normals(SEED, PR.tag_predictor(i), OFFSET + b, (1, c["L"], c["C"])) for b in samples])
        x = PC.em_step("vp", VP, float(ts[i]), x, score(x, ts[i]), z.astype(dtype), G, h, dtype)
    return x


MEASURED = {}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("pick", ["B512", "smallest", "odd", "halves_differ", "half_is_not_whole"])
def test_auto_runs_within_the_float64_bar(pick, entry):
    """Three steps under the default knobs at the sweep's picks; the six judged samples against the float64 walk at
    max(1e-5, 4 e32) of each sample's max-norm, every sample within that bar of the "partitions" = 0 run.

    Measured on one MI355X (printed per sample; DESIGN.md, section 3 "The loop"): B = 512, 350 and 475; e32 8.5e-8 ...
    2.5e-7, the device 8.1e-8 ... 2.2e-7 against the bar of 1e-5, and the partitioned run equal to the single-stream run
    bit for bit.  The sweep has NO engaging batch in 340 ... 1100 whose halves plan different wave counts or whose half
    plan differs from the whole batch's plan at 256 CUs (a half of nb samples on 128 CUs and 2 nb samples on 256 have
    the same tiles per CU): the ids "halves_differ" and "half_is_not_whole" run such a batch should a later planner
    have one, and say so otherwise."""
    chosen = picks()
    if pick not in chosen:
        print(f"{pick}: no such engaging batch in [{SWEEP[0]}, {SWEEP[-1]}]")
        return
    B = chosen[pick]
    tune({}, 1)
    info = plan("ecg", B, entry)
    assert info.parts == 2 and all(h.ffn.decode() == R.K_ROWS_OP for h in info.half)
    x0 = prior("ecg", B)
    one, two = x0.clone(), x0.clone()
    tune({}, 0)
    assert call("ecg", one, entry) == 1
    tune({}, 1)
    assert call("ecg", two, entry) == 2
    torch.cuda.synchronize()
    nb0 = (B + 1) // 2
    judged = sorted({0, 1, nb0 - 1, nb0, nb0 + 1, B - 1})
    w64, w32 = walk("ecg", x0, judged, entry, np.float64), walk("ecg", x0, judged, entry, np.float32)
    got2, got0 = two[judged].cpu().numpy().astype(np.float64), one[judged].cpu().numpy().astype(np.float64)
    worst_bar = 0.0
    for j, b in enumerate(judged):
        norm = np.abs(w64[j]).max()
        e32, e2, e0 = (float(np.abs(v[j] - w64[j]).max() / norm) for v in (w32, got2, got0))
        print(f"{pick} B={B} {entry} sample {b}: e32 {e32:.2e}, partitioned {e2:.2e}, single-stream {e0:.2e}, bar {R.bar(e32):.2e}")
        MEASURED[(pick, entry, b)] = (e32, e2, e0)
        assert e2 <= R.bar(e32), (b, e2, e0, e32)
        worst_bar = max(worst_bar, R.bar(e32))
    assert torch.isfinite(two).all()
    per_sample = (two - one).abs().flatten(1).max(dim=1).values / one.abs().flatten(1).max(dim=1).values
    print(f"{pick} B={B} {entry}: largest deviation of a sample from the single-stream run {float(per_sample.max()):.2e}")
    assert float(per_sample.max()) <= min(R.bar(MEASURED[(pick, entry, b)][0]) for b in judged)


# ------------------------------------------------------------------ 3. calls ----
CALL_SIZES = {"B8": ("ecg", 8, ECG_KNOBS), "regime_b": ("ecg", None, rows(12))}


def call_size(size):
    kind, B, knobs = CALL_SIZES[size]
    return kind, (smallest_persistent_batch("rows_nw12_fused") if B is None else B), knobs


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("size", sorted(CALL_SIZES))
def test_run_lengths_around_the_chunk_of_two(size, entry):
    kind, B, knobs = call_size(size)
    eligible_plan(kind, B, entry, knobs, {})
    x0 = prior(kind, B)
    for first in (0, 1):
        for n_run in (1, 2, 3, 5):
            one, two = x0.clone(), x0.clone()
            tune(knobs, 0)
            assert call(kind, one, entry, first, n_run) == 1
            tune(knobs, 2)
            assert call(kind, two, entry, first, n_run) == 2
            assert torch.equal(one, two) and not torch.equal(one, x0), (first, n_run)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("size", sorted(CALL_SIZES))
def test_a_trajectory_continued_over_calls(size, entry):
    kind, B, knobs = call_size(size)
    eligible_plan(kind, B, entry, knobs, {})
    x0 = prior(kind, B)
    ref, whole, cut = x0.clone(), x0.clone(), x0.clone()
    tune(knobs, 0)
    assert call(kind, ref, entry, 0, 6, g0=7) == 1
    tune(knobs, 2)
    assert call(kind, whole, entry, 0, 6, g0=7) == 2
    first = 0
    for n in (1, 2, 3):
        assert call(kind, cut, entry, first, n, g0=7 + first) == 2
        first += n
    assert torch.equal(whole, ref) and torch.equal(cut, ref) and not torch.equal(ref, x0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_growth_between_partitioned_calls(entry):
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    c = MODELS["ecg"]
    _, ts, h, sd, _ = model("ecg")
    sch = VPScheduler(fourier_noise_scaling=True, **VP)  # a context of its own, so that its workspace starts empty
    m = ScoreModule(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"], n_head=c["H"])
    sch.set_noise_scaling(c["L"])
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    ctx = m._ctx()
    s = N.current_stream_ptr(m.device)

    def run(x, partitions):
        tune(ECG_KNOBS, partitions)
        if entry == "sde":
            rc = ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, 1, STEPS, SEED, OFFSET, None, 0, 0, s)
        else:
            rc = ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), x.shape[0], ts, GRID, h, 1, STEPS, ENTRY[entry], 0, 0, s)
        N.check(rc, ctx.handle, entry)
        return status(ctx)

    def forward(x):
        out = torch.empty_like(x)
        N.check(ctx.lib.ffd_score_forward(ctx.handle, x.data_ptr(), 0.7, out.data_ptr(), x.shape[0], s), ctx.handle, "forward")
        return out

    want = {}
    for B in (8, 16, 32):  # the single-stream twins, from the shared context
        x = prior("ecg", B, seed=77 + B)
        tune(ECG_KNOBS, 0)
        assert call("ecg", x, entry) == 1
        want[B] = x
    x16 = prior("ecg", 16, seed=5)
    shared = model("ecg")[0]._ctx()
    before = torch.empty_like(x16)
    N.check(shared.lib.ffd_score_forward(shared.handle, x16.data_ptr(), 0.7, before.data_ptr(), 16, s), shared.handle, "forward")
    # the workspace grows in the first call, in the single-stream call of 16 and in the partitioned call of 32; the
    # partitioned call of 16 behind the single-stream one grows the score rows alone (their alignment padding)
    for B, partitions, then_forward in ((8, 2, False), (16, 0, False), (16, 2, True), (8, 2, True), (32, 2, True), (8, 0, True),
                                        (16, 2, True)):
        x = prior("ecg", B, seed=77 + B)
        info = N.PartitionInfo()
        tune(ECG_KNOBS, partitions)
        assert ctx.lib.ffd_partition_plan(ctx.handle, B, ENTRY[entry], C.byref(info)) == 0
        assert run(x, partitions) == info.parts == (2 if partitions else 1)
        assert torch.equal(x, want[B]), (B, partitions)
        if then_forward:  # PartScope put h0 / h1 / attn / score back: the plain forward gives the bits it gave before
            tune(ECG_KNOBS, 0)
            f = forward(x16)
            assert torch.equal(f, before) and torch.isfinite(f).all(), (B, partitions)


@pytest.mark.parametrize("solver", ["euler_maruyama", "ode_euler"])
def test_diffusion_sampler_partitions_with_device_draws(solver):
    """DiffusionSampler at the smallest engaging batch under the default knobs.  With the device's draws (rng="philox")
    and with the Euler ODE solver a batch is one loop call per trajectory and runs as two partitions; the samples are
    within the bar of section 2 of the "partitions" = 0 run.  The default rng="torch" hands its draws over in z_inject,
    which stays single-stream: several loop calls (z_chunk_steps = 2), status 1, the bits of "partitions" = 0."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    m = model("ecg")[0]
    ctx = m._ctx()
    B = picks()["smallest"]
    out = {}
    for partitions in (0, 1):
        tune({}, partitions)
        sampler = DiffusionSampler(m, B, rng="philox", solver=solver)
        out[partitions] = sampler.sample(B, 5)
        assert status(ctx) == 1 + partitions
    m.noise_scheduler.set_timesteps(GRID)
    assert torch.isfinite(out[1]).all() and out[1].shape == (B, MODELS["ecg"]["L"], 1)
    dev = float(((out[1] - out[0]).abs().flatten(1).max(dim=1).values / out[0].abs().flatten(1).max(dim=1).values).max())
    print(f"DiffusionSampler {solver} B={B}: largest deviation of a sample from the single-stream run {dev:.2e}")
    assert dev <= R.TOL_SCORE
    if solver == "euler_maruyama":
        for partitions in (0, 1):
            tune({}, partitions)
            torch.manual_seed(3)
            out[partitions] = DiffusionSampler(m, B, z_chunk_steps=2).sample(B, 5)
            assert status(ctx) == 1
        m.noise_scheduler.set_timesteps(GRID)
        assert torch.equal(out[0], out[1])


# ------------------------------------------------------------------ 4. what must stay single-stream ----
def partitions_again():
    x = prior("ecg", 8)
    tune(ECG_KNOBS, 2)
    assert plan("ecg", 8).parts == 2 and call("ecg", x, "sde") == 2


def both(run, x0):
    """run(x) -> status under "partitions" = 0 and = 2 (the caller's knobs otherwise): status 1, the same bits"""
    outs = []
    for p in (0, 2):
        assert N.lib().ffd_tune(b"partitions", p) == 0
        x = x0.clone()
        assert run(x) == 1, p
        outs.append(x)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all() and not torch.equal(outs[0], x0)


def loop_head(kind, x, first=0, n_run=STEPS):
    m, ts, h = model(kind)[:3]
    return m._ctx(), (m._ctx().handle, x.data_ptr(), x.shape[0], ts, GRID, h, first, n_run), N.current_stream_ptr(x.device)


def entry_case(name):
    """-> run(x) of a call that must stay on the caller's stream although the pinned ECG forms are eligible"""
    c = MODELS["ecg"]
    keep = []  # device buffers the call reads

    def run(x):
        ctx, head, s = loop_head("ecg", x)
        lib, B = ctx.lib, x.shape[0]
        if name == "z_inject":
            keep.append(torch.from_numpy(np.stack(list(synthetic.noise_stream(tuple(x.shape), STEPS, 9)))).cuda())
            rc = lib.ffd_sample_batch(*head, SEED, OFFSET, keep[-1].data_ptr(), 0, 0, s)
        elif name in ("ode_heun", "ode_ab2", "dpmpp_2m"):
            solver = dict(ode_heun=N.FFD_SOLVER_ODE_HEUN, ode_ab2=N.FFD_SOLVER_ODE_AB2, dpmpp_2m=N.FFD_SOLVER_DPMPP_2M)[name]
            rc = lib.ffd_sample_batch_ode(*head, solver, 0, 0, s)
        elif name == "pc":
            rc = lib.ffd_sample_batch_pc(*head, 1, 0.16, N.FFD_LANGEVIN_NORM_SAMPLE, SEED, OFFSET, None, 0, 0, s)
        elif name in ("cond", "resample"):
            keep.extend([torch.zeros((1, c["L"], c["C"]), device="cuda"), torch.zeros((1, c["L"], c["C"]), device="cuda")])
            keep[-1][:, ::3] = 1.0
            cfg = N.CondCfg(keep[-2].data_ptr(), keep[-1].data_ptr(), None, 1, N.FFD_COND_TIME, 0, 0)
            if name == "cond":
                rc = lib.ffd_sample_batch_cond(*head, 0, 0.16, 0, SEED, OFFSET, None, 0, 0, C.byref(cfg), s)
            else:
                rc = lib.ffd_sample_batch_resample(*head, 2, 2, 0, 0.16, 0, SEED, OFFSET, None, C.byref(cfg), s)
        elif name == "loglik":
            keep.append(torch.zeros(B, dtype=torch.float64, device="cuda"))
            rc = lib.ffd_loglik_batch(head[0], head[1], keep[-1].data_ptr(), B, head[3], GRID, 0, STEPS, N.FFD_SOLVER_ODE_EULER, 1,
                                      1e-2, None, SEED, OFFSET, s)
        elif name == "kernel_timing":
            assert lib.ffd_kernel_timing_begin(ctx.handle, 1 << N.K_FFN, 64) == 0
            try:
                rc = lib.ffd_sample_batch(*head, SEED, OFFSET, None, 0, 0, s)
            finally:
                assert lib.ffd_kernel_timing_end(ctx.handle) == 0
        elif name == "fresca_spatial":
            assert lib.ffd_fresca_enable(ctx.handle, C.byref(N.FrescaCfg(1.0, 1.5, 0.5, 0, 0))) == 0
            try:
                rc = lib.ffd_sample_batch(*head, SEED, OFFSET, None, 0, 0, s)
            finally:
                assert lib.ffd_fresca_disable(ctx.handle) == 0
        else:
            raise KeyError(name)
        N.check(rc, ctx.handle, name)
        return status(ctx)

    return run


@pytest.mark.parametrize("name", ["z_inject", "ode_heun", "ode_ab2", "dpmpp_2m", "pc", "cond", "resample", "loglik",
                                  "kernel_timing", "fresca_spatial"])
def test_entries_and_states_that_stay_single_stream(name):
    tune(ECG_KNOBS, 2)
    assert plan("ecg", 8).parts == 2  # the forms are eligible: the entry or the context's state keeps the call whole
    both(entry_case(name), prior("ecg", 8))
    partitions_again()


def other_backbone(kind):
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MixtureScoreModule, MLPScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    L, Cn, d = 24, 2, 32
    sch = VPScheduler(fourier_noise_scaling=True, **VP)
    if kind == "mlp":
        m = MLPScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, d_model=d, d_mlp=64, num_layers=2)
        sd = synthetic.mlp_state_dict(Cn, L, d, 64, 2)
    elif kind == "lstm":
        m = LSTMScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, d_model=d, num_layers=2)
        sd = synthetic.lstm_state_dict(Cn, L, d, 2)
    else:
        means = torch.from_numpy(np.random.default_rng(3).standard_normal((3, L, Cn)).astype(np.float32))
        m, sd = MixtureScoreModule(n_channels=Cn, max_len=L, noise_scheduler=sch, means=means), None
    sch.set_noise_scaling(L)
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    sch.set_timesteps(GRID)
    return m.cuda().eval(), (C.c_float * GRID)(*sch.timesteps.tolist()), float(sch.step_size), (L, Cn)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", ["mlp", "lstm", "mixture"])
def test_other_backbones_stay_single_stream(kind, entry):
    m, ts, h, (L, Cn) = other_backbone(kind)
    ctx = m._ctx()
    x0 = torch.from_numpy(next(synthetic.noise_stream((8, L, Cn), 1, 11))).cuda()
    s = N.current_stream_ptr(x0.device)
    tune({}, 2)
    info = N.PartitionInfo()
    assert ctx.lib.ffd_partition_plan(ctx.handle, 8, ENTRY[entry], C.byref(info)) == 0
    assert (info.parts, info.halves_planned, info.whole_planned, info.cu_budget) == (1, 0, 0, 0)

    def run(x):
        if entry == "sde":
            rc = ctx.lib.ffd_sample_batch(ctx.handle, x.data_ptr(), 8, ts, GRID, h, 1, STEPS, SEED, OFFSET, None, 0, 0, s)
        else:
            rc = ctx.lib.ffd_sample_batch_ode(ctx.handle, x.data_ptr(), 8, ts, GRID, h, 1, STEPS, ENTRY[entry], 0, 0, s)
        N.check(rc, ctx.handle, kind)
        return status(ctx)

    both(run, x0)
    partitions_again()


PLAN_CASES = {  # id -> (model, knobs, what a half's plan must say)
    "two_kernel_attention": ("d24hd4", dict(OFF, ffn_mb=1), dict(attn=R.K_TWO_KERNEL, ffn=R.K_LN)),
    "attn_fused_off": ("ecg", dict(ECG_KNOBS, attn_fused=0), dict(attn=R.K_TWO_KERNEL, ffn=R.K_ROWS_OP)),
    "ffn_split": ("ecg", dict(ECG_KNOBS, ffn_split=1), dict(ffn=R.K_SPLIT)),
    "sliced_rows_forced": ("ecg", dict(rows_slices=2, small_path=0, mid_path=0, ffn_height=0, attn_small=0), dict(ffn=R.K_SL_OP)),
    "f_slices_forced": ("ecg", dict(rows_slices=-1, small_path=0, mid_path=2, ffn_height=0, attn_small=0), dict(ffn=R.K_PART)),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plans_that_stay_single_stream(case, entry):
    kind, knobs, want = PLAN_CASES[case]
    tune(knobs, 2)
    info = plan(kind, 8, entry)
    assert info.parts == 1 and info.halves_planned == 1
    for h in info.half:
        assert_wanted(h, want)
        assert h.attn.decode() != R.K_FUSED or h.part_floats > 0 or h.ffn.decode() == R.K_SPLIT
    both(lambda x: call(kind, x, entry), prior(kind, 8))
    partitions_again()


def test_default_knobs_where_a_half_plans_a_form_with_partial_rows():
    """Under the default knobs, the first batch in 2 ... 400 at which a half plans each FFN form that keeps partial rows
    in the shared workspace (the small-batch pair, the sliced rows, the F slices): "partitions" = 1 and 2 leave the call
    on the caller's stream, with the bits of "partitions" = 0."""
    found = {}
    tune({}, 2)
    for B in range(2, 401):
        info = plan("ecg", B)
        for h in info.half:
            if h.part_floats > 0:
                assert info.parts == 1
                found.setdefault(h.ffn.decode(), B)
    print(f"forms with partial rows under the default knobs, first batch: {found}")
    assert R.K_SMALL in found and len(found) >= 2
    for ffn, B in sorted(found.items()):
        x0 = prior("ecg", B)
        ref = x0.clone()
        tune({}, 0)
        assert call("ecg", ref, "sde") == 1
        for p in (1, 2):
            tune({}, p)
            got = x0.clone()
            assert plan("ecg", B).parts == 1 and call("ecg", got, "sde") == 1
            assert torch.equal(got, ref), (ffn, B, p)
        partitions_again()
