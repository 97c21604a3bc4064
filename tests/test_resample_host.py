"""CPU-side tests of resampled conditional sampling (no GPU): the five new C-ABI symbols are exported and bound like
include/ffd.h, every argument error comes back before any device work, the host coefficients and the visit schedule are
what the restatement (tests/resample_restatement.py) says, the Python surface validates its arguments and hands the loop
its draws in execution order, and the float64 restatement shows the effect resampling is built for on the two-mode
forecast.

The loop's own rejections behind the context check (a visit range outside [0, U], the tag range, cond == NULL with a live
context) need a device and are held by tests/test_resample_gpu.py."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_restatement as R
from oracle import cases
from test_pc_host import _Model, _header_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_host_transition_coef", "ffd_forward_transition", "ffd_host_resample_visits", "ffd_host_resample_visit",
               "ffd_sample_batch_resample")
SDES = {"vp": cases.VP, "ve": cases.VE}
KIND = {"vp": 0, "ve": 1}
C_TYPES = {"double": C.c_double, "float": C.c_float, "int": C.c_int, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _desc(sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    lo, hi = (kw["beta_min"], kw["beta_max"]) if sde == "vp" else (kw["sigma_min"], kw["sigma_max"])
    assert (N.FFD_SDE_VP, N.FFD_SDE_VE) == (KIND["vp"], KIND["ve"])
    return N.SdeDesc(KIND[sde], 0, lo, hi)


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_like_the_header(lib, name):
    from fastfourierdiffusion_amd import _native

    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, re.M), f"{name} is not exported"
    res, args = _native.SIGNATURES[name]
    ret, params = _header_decl(name)
    assert res is C.c_int and ret == "int" and len(args) == len(params), (name, len(args), params)
    for a, p in zip(args, params):
        if "*" in p or "[" in p:  # (an array parameter is a pointer)
            assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is C_TYPES[p.split()[-2]], (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_header_documents_the_tag_row_and_the_contract():
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    assert "0xE0000000 + q" in header and "0x1FFFFFF0" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "0xE0000000" in design  # the tag map of section 3 has the transitions' row


# ---------------------------------------------------------------- argument errors: no device work ----
X_, G_, Z_ = 0x1000, 0x2000, 0x3000  # dummies, never dereferenced


def _transition(lib, sde="default", x=X_, g=G_, s=0.25, t=0.5, z=Z_, B=2, L=5, Cn=3, kind=0):
    from fastfourierdiffusion_amd import _native as N

    desc = N.SdeDesc(kind, 0, 0.1, 20.0)
    return lib.ffd_forward_transition(C.byref(desc) if sde == "default" else sde, x, g, s, t, z, 1, 0, R.TAG0, B, L, Cn, None)


def test_forward_transition_refuses_bad_arguments_without_a_device(lib):
    for bad in (dict(sde=None), dict(x=None), dict(g=None), dict(B=0), dict(L=0), dict(Cn=0), dict(B=-1), dict(t=0.2),
                dict(s=-0.1), dict(s=-1.0, t=-0.5), dict(z=X_), dict(s=math.nan), dict(t=math.nan), dict(t=math.inf),
                dict(z=None, x=None)):  # z may be null: the OTHER argument is refused
        assert _transition(lib, **bad) == -1, bad
    assert _transition(lib, kind=7) == -2 and _transition(lib, kind=7, z=None) == -2
    assert _transition(lib, kind=7, x=None) == -1 and _transition(lib, kind=7, t=0.1) == -1  # INVALID wins


def test_host_helpers_refuse_bad_arguments(lib):
    from fastfourierdiffusion_amd import _native as N

    out = (C.c_double * 2)()
    d = _desc("vp")
    assert lib.ffd_host_transition_coef(None, 0.1, 0.2, out) == -1
    assert lib.ffd_host_transition_coef(C.byref(d), 0.1, 0.2, None) == -1
    for s, t in ((-0.1, 0.2), (0.3, 0.2), (math.nan, 0.2), (0.1, math.nan), (0.1, math.inf), (-math.inf, 0.0)):
        assert lib.ffd_host_transition_coef(C.byref(d), s, t, out) == -1, (s, t)
    bad = N.SdeDesc(7, 0, 0.1, 20.0)
    assert lib.ffd_host_transition_coef(C.byref(bad), 0.1, 0.2, out) == -2
    assert lib.ffd_host_transition_coef(C.byref(bad), 0.3, 0.2, out) == -1  # INVALID wins
    for n, j, r in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 2, 2), (1 << 30, 1, 4)):
        assert lib.ffd_host_resample_visits(n, j, r) == -1, (n, j, r)
    a, b = C.c_int(), C.c_int()
    for n, j, r, u in ((0, 1, 1, 0), (3, 0, 1, 0), (3, 1, 0, 0), (3, 2, 2, -1), (3, 2, 2, 6)):
        assert lib.ffd_host_resample_visit(n, j, r, u, C.byref(a), C.byref(b)) == -1, (n, j, r, u)
    assert lib.ffd_host_resample_visit(3, 2, 2, 0, None, C.byref(b)) == -1
    assert lib.ffd_host_resample_visit(3, 2, 2, 0, C.byref(a), None) == -1
    assert lib.ffd_host_resample_visit(3, 2, 2, 5, C.byref(a), C.byref(b)) == 0


def test_sample_batch_resample_refuses_bad_arguments_without_a_context(lib):
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 3)(1.0, 0.5, 1e-5)
    cfg = N.CondCfg(0x4000, 0x5000, None, 1, N.FFD_COND_FREQUENCY, 1, 0)
    for cond in (None, C.byref(cfg)):
        assert lib.ffd_sample_batch_resample(None, X_, 1, ts, 3, 0.5, 0, 2, 2, 2, 1, 0.16, N.FFD_LANGEVIN_NORM_BATCH, 0, 0, None,
                                             cond, None) == -1


# ---------------------------------------------------------------- coefficients ----
def _coef(lib, sde, s, t):
    out = (C.c_double * 2)()
    d = _desc(sde)
    assert lib.ffd_host_transition_coef(C.byref(d), s, t, out) == 0
    return out[0], out[1]


@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_transition_coefficients(lib, sde):
    """Against the float64 restatement to 1e-15 relative; s == t exactly (1, 0); from s = 0 the VP marginal's (mc, sigma);
    the semigroup property on a 7-point grid to 1e-12."""
    kw = SDES[sde]
    ts = [float(np.float32(v)) for v in np.linspace(1e-5, 1.0, 7)]
    for i, s in enumerate([0.0] + ts):
        assert _coef(lib, sde, s, s) == (1.0, 0.0)
        for t in ([0.0] + ts)[i:]:
            a, sg = _coef(lib, sde, s, t)
            wa, wsg = R.transition_coefficients(sde, kw, s, t)
            assert abs(a - wa) <= 1e-15 * wa and abs(sg - wsg) <= 1e-15 * wsg, (s, t, a, wa, sg, wsg)
    if sde == "vp":
        for t in ts:
            mc, sigma = R.CR.coefficients("vp", kw, t)
            a, sg = _coef(lib, "vp", 0.0, t)
            assert abs(a - mc) <= 1e-15 * mc and abs(sg - sigma) <= 1e-13 * sigma
    for i, r in enumerate(ts):
        for j in range(i, 7):
            for k in range(j, 7):
                s, t = ts[j], ts[k]
                (a_rs, g_rs), (a_st, g_st), (a_rt, g_rt) = _coef(lib, sde, r, s), _coef(lib, sde, s, t), _coef(lib, sde, r, t)
                assert abs(a_rt - a_rs * a_st) <= 1e-12 * a_rt, (r, s, t)
                var = a_st * a_st * g_rs * g_rs + g_st * g_st
                assert abs(g_rt * g_rt - var) <= 1e-12 * max(g_rt * g_rt, 1e-300), (r, s, t)


def test_restatement_operator_is_the_marginal_and_composes():
    """x_0 -> x_t in one transition from s = 0 is cond_restatement's noised observation (VP); two transitions with
    independent draws have the variance of one; fp32 in libffd's order follows float64."""
    rng = np.random.default_rng(0)
    shape = (3, 9, 2)
    x, z = rng.standard_normal(shape), rng.standard_normal(shape)
    G = R.fourier_G(9).astype(np.float64)
    y = R.CR.noised_observation("vp", cases.VP, 0.5, x, z, G)
    assert np.allclose(R.forward_transition("vp", cases.VP, 0.0, 0.5, x, z, G), y, atol=1e-13)
    for sde in ("vp", "ve"):
        assert R.forward_transition(sde, SDES[sde], 0.3, 0.3, x, z, G) is not None
        assert np.array_equal(R.forward_transition(sde, SDES[sde], 0.3, 0.3, x, z, G), x)
        a = R.forward_transition(sde, SDES[sde], 0.2, 0.7, x, z, G)
        b = R.forward_transition(sde, SDES[sde], 0.2, 0.7, np.float32(x), np.float32(z), np.float32(G), dtype=np.float32)
        assert b.dtype == np.float32 and R.rel_max_err(b, a) < 1e-6


# ---------------------------------------------------------------- schedule ----
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("jump", [1, 2, 4, 6, 9])
@pytest.mark.parametrize("n", [1, 6, 7])
def test_visit_schedule(lib, n, jump, r):
    U = lib.ffd_host_resample_visits(n, jump, r)
    assert U == r * n
    step, back = C.c_int(), C.c_int()
    sched = []
    for u in range(U):
        assert lib.ffd_host_resample_visit(n, jump, r, u, C.byref(step), C.byref(back)) == 0
        sched.append((step.value, back.value))
    assert sched == R.visits(n, jump, r)
    assert sorted(s for s, _ in sched) == sorted(list(range(n)) * r)  # every grid index exactly r times
    if r == 1:
        assert sched == [(i, -1) for i in range(n)]  # the identity schedule
    # inside a pass visits ascend by one; a pass ends where the index does not
    transitions = [(u, s, b) for u, (s, b) in enumerate(sched) if b >= 0]
    assert len(transitions) == (r - 1) * math.ceil(n / jump)
    for u in range(1, U):
        prev, cur = sched[u - 1], sched[u]
        if prev[1] >= 0:
            assert cur[0] == prev[1]  # re-noised to the block's first index, which runs next
        else:
            assert cur[0] == prev[0] + 1
    j = min(jump, n)
    for u, s, b in transitions:
        assert b == (s // j) * j and (s == n - 1 or (s + 1) % j == 0)  # a block's last index returns to its first
    assert sched[-1][1] == -1


# ---------------------------------------------------------------- Python surface ----
def test_python_surface_and_argument_checks():
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import SDE, VEScheduler, VPScheduler

    sig = inspect.signature(SDE.forward_transition)
    assert list(sig.parameters)[1:5] == ["sample", "timestep_from", "timestep_to", "noise"]
    assert sig.parameters["noise"].default is None
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        seed=None, sample_offset=0, tag=0xE0000000)
    assert "forward_transition" not in VPScheduler.__dict__ and "forward_transition" not in VEScheduler.__dict__
    for fn in (DiffusionSampler.sample_conditional, DiffusionSampler.impute):
        sig = inspect.signature(fn)
        assert sig.parameters["resample"].default == 1 and sig.parameters["jump"].default == 1

    sch = VPScheduler()
    sch.set_noise_scaling(8)
    x = torch.zeros(2, 8, 1)
    for s, t in ((0.5, 0.4), (-0.1, 0.4)):
        with pytest.raises(ValueError):
            sch.forward_transition(x, s, t)
    a, sg = sch.transition_coeffs(0.25, 0.5)
    assert (a, sg) == R.transition_coefficients("vp", dict(beta_min=sch.beta_0, beta_max=sch.beta_1), 0.25, 0.5)

    m = _Model(VPScheduler())  # L = 8, C = 1
    m.device = torch.device("cpu")
    obs, mask = torch.zeros(8, 1), torch.ones(8)
    for solver in ("ode_euler", "ode_heun", "ode_ab2", "dpmpp_2m"):  # the ODE-solver refusal stays
        with pytest.raises(ValueError):
            DiffusionSampler(m, 4, solver=solver).sample_conditional(obs, mask, 4, 3, resample=2, jump=2)
    s = DiffusionSampler(m, 4)
    for bad in (dict(resample=0), dict(resample=-1), dict(resample=2.0), dict(resample=True), dict(jump=0), dict(jump=1.5),
                dict(jump=None), dict(resample="2")):
        with pytest.raises(ValueError, match="integer >= 1"):
            s.sample_conditional(obs, mask, 4, 3, **bad)
        with pytest.raises(ValueError, match="integer >= 1"):
            s.impute(obs, mask, 4, 3, **bad)


def test_the_cache_is_refused_with_resampling():
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    m = _Model(VPScheduler())
    m.device = torch.device("cpu")
    s = DiffusionSampler(m, 4)
    s.use_cache = True  # (the constructor's use_cache=True needs a real model to enable its cache on)
    obs, mask = torch.zeros(8, 1), torch.ones(8)
    with pytest.raises(ValueError, match="use_cache=True"):
        s.sample_conditional(obs, mask, 4, 3, resample=2)
    with pytest.raises(ValueError, match="use_cache=True"):
        s.impute(obs, mask, 4, 3, resample=3, jump=2)


class _Lib:
    """Stands in for libffd under DiffusionSampler._sample: the host schedule is the real library's, the loop calls are
    recorded with the slabs they were handed."""

    def __init__(self, real, slab):
        self.real, self.slab, self.calls = real, slab, []
        self.ffd_host_resample_visits = real.ffd_host_resample_visits
        self.ffd_host_resample_visit = real.ffd_host_resample_visit

    def ffd_sample_batch_resample(self, hdl, x, B, ts, n_steps, h, first, n_run, jump, resample, n_corr, snr, norm, seed, off,
                                  z, cond, stream):
        zs = None
        if z:
            k = R.n_slabs(n_steps, jump, resample, n_corr, first, n_run)
            zs = np.frombuffer(C.string_at(z, 4 * self.slab * k), np.float32).reshape(k, -1)[:, 0].copy()
        self.calls.append(dict(fn="resample", first=first, n_run=n_run, jump=jump, resample=resample, n_corr=n_corr, off=off,
                               z=zs, final=cond._obj.final_replace))
        return 0

    def ffd_sample_batch_cond(self, hdl, x, B, ts, n_steps, h, first, n_run, n_corr, *rest):
        self.calls.append(dict(fn="cond", first=first, n_run=n_run, n_corr=n_corr))
        return 0

    def __getattr__(self, name):
        return lambda *a: 0


def _stub(lib, monkeypatch, n_steps, inject=True, call=None, **kw):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    L, Cn, batch = 8, 1, 2
    m = _Model(VPScheduler())
    m.device = torch.device("cpu")
    m.num_training_steps = n_steps
    m.scale_noise = True
    m.eval = lambda: None
    stub = _Lib(lib, batch * L * Cn)
    m._ctx = lambda: type("Ctx", (), {"lib": stub, "handle": None})()
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    s = DiffusionSampler(m, batch, **kw)
    monkeypatch.setattr(s, "sample_prior", lambda batch_size, _sample_offset=0: torch.zeros(batch_size, L, Cn))
    if inject:
        s.inject_noise(np.full((batch, L, Cn), float(v), np.float32) for v in range(1000))
    s.sample_conditional(torch.zeros(8, 1), torch.ones(8), batch, n_steps, **(call or {}))
    return stub.calls


def test_call_sequence_draw_count_and_order(lib, monkeypatch):
    """The calls tile the visits [0, U) in order, every call gets exactly the slabs its visits consume -- a visit's
    2 (n_corrector + 1), then its transition's one -- in consumption order, and no call's buffer exceeds z_chunk_steps
    slabs unless a single visit does."""
    for n, r, j, n_corr, chunk in ((5, 2, 2, 1, 9), (5, 3, 4, 0, 5), (6, 2, 9, 0, 50), (3, 2, 1, 1, 1)):
        calls = _stub(lib, monkeypatch, n, corrector_steps=n_corr, z_chunk_steps=chunk, call=dict(resample=r, jump=j))
        assert all(c["fn"] == "resample" and (c["jump"], c["resample"], c["n_corr"]) == (j, r, n_corr) for c in calls)
        firsts = [c["first"] for c in calls]
        assert firsts[0] == 0 and firsts[1:] == [c["first"] + c["n_run"] for c in calls[:-1]]
        assert calls[-1]["first"] + calls[-1]["n_run"] == r * n
        total = R.n_slabs(n, j, r, n_corr)
        assert total == r * n * 2 * (n_corr + 1) + (r - 1) * math.ceil(n / j)
        drawn = np.concatenate([c["z"] for c in calls])
        assert np.array_equal(drawn, np.arange(total, dtype=np.float32))  # in order, none skipped, none left over
        one_visit = 2 * (n_corr + 1) + 1
        assert all(len(c["z"]) <= max(chunk, one_visit) for c in calls)
        if chunk < total:
            assert len(calls) > 1
    calls = _stub(lib, monkeypatch, 5, inject=False, rng="philox", seed=3, sample_offset=7, call=dict(resample=2, jump=2))
    assert len(calls) == 1 and calls[0]["z"] is None and calls[0]["off"] == 7 and calls[0]["n_run"] == 10
    # resample = 1 takes the replacement path, whatever jump is
    calls = _stub(lib, monkeypatch, 5, corrector_steps=1, z_chunk_steps=8, call=dict(resample=1, jump=3))
    assert [(c["fn"], c["first"], c["n_run"]) for c in calls] == [("cond", 0, 2), ("cond", 2, 2), ("cond", 4, 1)]


# ---------------------------------------------------------------- the restatement's recorded bands ----
# right-mode fraction of the two-mode forecast (4000 samples, numpy seeds 0..7, 100 score evaluations each), (min, max)
# as the float64 restatement gives them, rounded outwards to four digits
TWO_MODE_BAND = {"replacement": (0.7222, 0.7435), "resampled": (0.8062, 0.8255)}
# mean over the unobserved positions of (sample variance / DATA_STD^2) on the analytic white-data case under the
# resampled loop (50 steps, r = 3, j = 2, one corrector, snr 0.16, 4096 samples), numpy seeds 0..7, rounded outwards
RESAMPLED_WHITE_BAND = {"ve": (1.0226, 1.0408), "vp": (1.0324, 1.0509)}


@pytest.fixture(scope="module")
def two_mode_runs():
    return {"replacement": [R.two_mode_run(seed, 100) for seed in range(8)],
            "resampled": [R.two_mode_run(seed, 20, resample=5, jump=2) for seed in range(8)]}


def test_two_mode_case_resampling_beats_replacement_at_equal_evaluations(two_mode_runs):
    """4000 samples, 8 seeds, 100 score evaluations each: every seed of (20 steps, r = 5, j = 2) lies above every seed
    of replacement at 100 steps (exact right-mode probability 0.9).  Measured when the feature was specified:
    0.806 - 0.826 against 0.722 - 0.744."""
    plain, again = two_mode_runs["replacement"], two_mode_runs["resampled"]
    bands = f"replacement {min(plain):.3f} - {max(plain):.3f}, resampled {min(again):.3f} - {max(again):.3f}"
    print("two-mode right-mode fraction:", bands)
    assert min(again) > max(plain), bands


@pytest.mark.parametrize("which", ["replacement", "resampled"])
def test_two_mode_recorded_band(two_mode_runs, which):
    """The band tests/test_resample_gpu.py holds the device to IS what the eight seeds give (to its outward rounding)."""
    lo, hi = TWO_MODE_BAND[which]
    got = two_mode_runs[which]
    assert lo <= min(got) < lo + 2e-4 and hi - 2e-4 < max(got) <= hi, got


@pytest.mark.parametrize("sde", ["ve", "vp"])
def test_restatement_white_data_case_under_resampling(sde):
    """White data: replacement is exact, so the resampled loop leaves the statistics where plain replacement has them
    at these 50 steps (variance ratio 1.02 - 1.04, the discretisation's own bias), the observed points come back exactly,
    and the eight seeds' min / max IS the recorded band."""
    lo, hi = RESAMPLED_WHITE_BAND[sde]
    ratios = []
    for seed in range(8):
        xt, series, mask = R.gaussian_conditional(sde, SDES[sde], seed)
        ratio, worst = R.CR.unobserved_stats(xt, mask)
        ratios.append(ratio)
        assert worst < 5.0, (seed, worst)
        assert np.abs(xt[:, :R.CR.GAUSS_PREFIX] - series[:, :R.CR.GAUSS_PREFIX]).max() < 1e-12
    print(f"white data {sde}, resampled: ratio {min(ratios):.4f} .. {max(ratios):.4f}")
    assert lo <= min(ratios) < lo + 2e-4 and hi - 2e-4 < max(ratios) <= hi, ratios
