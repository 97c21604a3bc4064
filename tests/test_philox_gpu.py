"""GPU tests of the on-device noise generator against its float64 restatement (tests/philox_restatement.py), through the
C ABI: every entry that draws with z = NULL is asked for its draws and held to the restated ones, element by element.

Two bars apply to a draw.  IDENTITY, 1e-4 per element: a wrong word, slot, tag, seed half or index moves a draw by O(1).
ACCURACY, 2e-6 x 5.8871 (the single-operator contract of DESIGN.md section 5 applied to the draw's bound): how far the
hardware log2 / sqrt / sin / cos put a draw from the exact Box-Muller value of its words, asserted over one call of 2^20.

1. ``ffd_prior`` with G = 1 returns z itself (1 z is exact): shapes, alignments, seeds, the 2^32 / 2^34 / 2^40 element
   boundaries, each also split into shards bit for bit;   2. the accuracy figures;
3. ``ffd_sde_step``;   4. ``ffd_langevin_step``;   5. ``ffd_cond_project`` and ``ffd_forward_transition``;
6. ``ffd_sm_perturb`` and the draws ``ffd_sm_loss`` regenerates;   7. ``ffd_sm_draw_times`` (bit for bit);
8. the limits the loop entries enforce;
9. the tag plan of the ``ffd_sample_batch*`` entries end to end: a philox run equals the run with the restated draws
   injected in the documented consumption order.

The fused unembed tails have no case of their own: tests/test_tail_forms_gpu.py and
test_gpu_parity.py::test_fused_unembed_sde_tail_equals_two_kernels hold them bit-identical to the stand-alone step under
philox, and the stand-alone step is case 3.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import mixture_restatement as M
import ode_restatement as ODE
import pc_restatement as P
import philox_restatement as PR
import resample_restatement as RS
from conftest import rel_err
from test_mixture_gpu import SDES, lib, module, stream  # noqa: F401  (lib: the module's fixture)
from test_pc_gpu import reconstruct_w

pytestmark = pytest.mark.gpu

IDENTITY = 1e-4
ACCURACY = 2e-6 * PR.Z_MAX  # 1.18e-5
TOL_STEP = 5e-7             # ffd_sde_step / ffd_sm_perturb, of the max-norm (test_gpu_parity.py, test_loss_gpu.py)
TOL_TRAJ = 1e-5             # a trajectory, of the max-norm (the project's trajectory contract)
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def desc(sde):
    from fastfourierdiffusion_amd import _native as N

    kw = SDES[sde]
    a, b = (kw["beta_min"], kw["beta_max"]) if sde == "vp" else (kw["sigma_min"], kw["sigma_max"])
    return N.SdeDesc(N.FFD_SDE_VP if sde == "vp" else N.FFD_SDE_VE, 0, a, b)


def dev(a, shift=0):
    """A device copy of `a` whose first element lies `shift` floats past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, device="cuda", dtype=torch.float32)
    view = buf[shift:shift + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def prior(lib, shape, seed, offset, shift=0):
    """ffd_prior (VP: no scale) with G = 1: the draws themselves, (B, L, C) float32"""
    B, L, Cn = shape
    x = dev(np.full(shape, np.nan, np.float32), shift)
    G = dev(np.ones(L, np.float32))
    d = desc("vp")
    assert lib.ffd_prior(C_.byref(d), x.data_ptr(), None, G.data_ptr(), seed, offset, B, L, Cn, stream()) == 0
    return x.cpu().numpy()


def offset_before(boundary, n, back):
    """the sample offset whose first element is the last multiple of n at least `back` elements below `boundary`"""
    return (boundary - back) // n


# ------------------------------------------------------------------ 1. the prior ----
# (shape, seed, sample offset, floats off 16-byte alignment)
PRIOR_CASES = [
    ((1, 5, 1), 42, 0, 0),            # L C % 4 = 1, B = 1, C = 1
    ((3, 2, 3), 42, 0, 0),            # L C % 4 = 2
    ((3, 5, 3), 42, 0, 0),            # L C % 4 = 3, C = 3
    ((3, 3, 4), 42, 0, 0),            # L C % 4 = 0, C = 4: the float4 kernel
    ((33, 4, 8), 42, 0, 0),           # C = 8, B = 33
    ((3, 3, 13), 42, 0, 0),           # C = 13
    ((33, 2, 40), 42, 0, 0),          # C = 40
    ((3, 300, 4), 42, 0, 0),          # more than one workgroup of float4
    ((3, 1031, 1), 42, 0, 0),         # more than one workgroup of the scalar kernel
    ((3, 5, 3), 42, 3, 0),            # element offset 45: a sample starts in the tail of a block
    ((3, 7, 3), 42, 1, 0),            # element offset 21
    ((3, 3, 4), 42, 5, 1),            # base pointer 4 bytes off: C = 4 through the scalar kernel
    ((3, 3, 4), 42, 5, 2),            # 8 bytes
    ((33, 4, 8), 42, 2, 3),           # 12 bytes
    ((3, 5, 3), 0, 2, 0),
    ((3, 3, 4), 0, 2, 0),
    ((3, 5, 3), 1 << 32, 2, 0),       # only the key's high word is set
    ((3, 3, 4), 1 << 32, 2, 0),
    ((3, 5, 3), (1 << 63) + 5, 2, 0),
    ((3, 3, 4), (1 << 63) + 5, 2, 0),
    ((3, 5, 3), 42, offset_before(1 << 32, 15, 16), 0),   # elements straddle 2^32: the block index crosses 2^30
    ((3, 4, 4), 42, offset_before(1 << 32, 16, 16), 0),
    ((3, 5, 3), 42, offset_before(1 << 34, 15, 4), 0),    # elements straddle 2^34: the high counter word 0 -> 1
    ((3, 4, 4), 42, offset_before(1 << 34, 16, 16), 0),
    ((3, 5, 3), (1 << 63) + 5, offset_before(1 << 40, 15, 20), 0),  # high counter word 63 -> 64
    ((3, 4, 4), (1 << 63) + 5, offset_before(1 << 40, 16, 16), 0),
]


def prior_id(c):
    shape, seed, off, shift = c
    return f"{ids(shape)}-seed{seed:#x}-off{off:#x}" + (f"+{4 * shift}B" if shift else "")


@pytest.mark.parametrize("case", PRIOR_CASES, ids=prior_id)
def test_prior_is_the_restated_draw_and_shards_bit_for_bit(lib, case):
    shape, seed, off, shift = case
    B, L, Cn = shape
    n = L * Cn
    if off > 1 << 20:  # the case is about a boundary: it must lie inside the call
        lo, hi = off * n, (off + B) * n
        assert any(lo < b < hi for b in (1 << 32, 1 << 34, 1 << 40)), (lo, hi)
    got = prior(lib, shape, seed, off, shift)
    want = PR.sample_normals(seed, PR.TAG_PRIOR, off, shape)
    err = float(np.abs(got - want).max())
    print(f"prior {prior_id(case)}: max |z_dev - z_64| {err:.2e}")
    assert np.isfinite(got).all() and err <= IDENTITY
    assert np.abs(want).max() > 1.0  # (not a comparison of zeros)
    cuts = [0, 1, B] if B <= 3 else [0, 1, 16, B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            for s in {shift, 0}:  # a shard at the whole call's alignment, and in an aligned buffer of its own
                assert np.array_equal(prior(lib, (b - a, L, Cn), seed, off + a, s), got[a:b]), (a, b, s)


def test_prior_scale_and_other_streams(lib):
    """VE multiplies by sigma_max; another seed half, offset or (through ffd_sde_step) tag is another stream."""
    shape = (3, 5, 3)
    B, L, Cn = shape
    x = dev(np.zeros(shape, np.float32))
    G = dev(np.ones(L, np.float32))
    d = desc("ve")
    assert lib.ffd_prior(C_.byref(d), x.data_ptr(), None, G.data_ptr(), 42, 2, B, L, Cn, stream()) == 0
    want = SDES["ve"]["sigma_max"] * PR.sample_normals(42, PR.TAG_PRIOR, 2, shape)
    assert np.abs(x.cpu().numpy() - want).max() <= SDES["ve"]["sigma_max"] * IDENTITY
    base = prior(lib, shape, 42, 2)
    for seed, off in ((43, 2), (42 + (1 << 32), 2), (42, 3), (42, 2 + (1 << 34))):
        assert np.abs(prior(lib, shape, seed, off) - base).max() > 0.5, (seed, off)


# ------------------------------------------------------------------ 2. accuracy ----
MILLION = (256, 512, 8)  # 2^20 draws in one call


@pytest.fixture(scope="module")
def million(lib):
    got = prior(lib, MILLION, 42, 0).astype(np.float64).ravel()
    return got, PR.normals(42, PR.TAG_PRIOR, 0, got.size)


def test_a_million_draws_identity(lib, million):
    got, want = million
    assert got.size == 1 << 20 and np.abs(got - want).max() <= IDENTITY
    assert np.abs(got).max() <= PR.Z_MAX * (1 + 1e-6)


def test_a_million_draws_accuracy(lib, million):
    """max |z_dev - z_64| over 2^20 draws against 2e-6 x 5.8871 = 1.18e-5.  Measured on one MI355X: max 7.2e-7, 99.9 %
    quantile 3.2e-7 (cos slots 7.2e-7 / 3.2e-7, sin slots 5.7e-7 / 3.2e-7): the hardware transcendentals need no repair."""
    got, want = million
    e = np.abs(got - want)
    cos, sin = e.reshape(-1, 2)[:, 0], e.reshape(-1, 2)[:, 1]
    for what, v in (("all", e), ("cos slots", cos), ("sin slots", sin)):
        print(f"draw error, {what}: max {v.max():.3e}, 99.9 % quantile {np.quantile(v, 0.999):.3e}, mean {v.mean():.3e}")
    worst = int(np.argmax(e))
    print(f"  worst draw: element {worst}, z_64 {want[worst]:+.6f}, z_dev {got[worst]:+.6f}; bar {ACCURACY:.3e}")
    rel = e / np.maximum(np.abs(want), 1e-30)
    print(f"  relative to the draw, where |z| > 0.1: max {rel[np.abs(want) > 0.1].max():.3e}")
    assert e.max() <= ACCURACY


# ------------------------------------------------------------------ 3. ffd_sde_step ----
@pytest.mark.parametrize("tag", [0, 5])
@pytest.mark.parametrize("shape", [(3, 20, 4), (3, 21, 3)], ids=ids)  # the float4 kernel; the ragged scalar one (offset 126)
@pytest.mark.parametrize("fourier", [True, False], ids=["fourierG", "unitG"])
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_sde_step_draws(lib, sde, fourier, shape, tag):
    """The float64 Euler-Maruyama update with the restated draw in place of z.  Bar: the step's 5e-7 of the max-norm plus
    the draw's share, g sqrt(dt) G_l x the accuracy bar (printed per case)."""
    B, L, Cn = shape
    G = M.fourier_G(L, fourier)
    rng = np.random.default_rng(300 + L + tag)
    x, s = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    t, h, seed, off = 0.5, np.float32(1.0 / 12.0), (1 << 40) + 17, 2
    xd, sd, Gd = dev(x), dev(s), dev(G)
    d = desc(sde)
    assert lib.ffd_sde_step(C_.byref(d), xd.data_ptr(), sd.data_ptr(), Gd.data_ptr(), t, float(h), None, seed, off, tag, B, L,
                            Cn, stream()) == 0
    z = PR.sample_normals(seed, tag, off, shape)
    ref = P.em_step(sde, SDES[sde], t, x, s, z, G, float(h))
    _, cs = ODE.coefficients(sde, SDES[sde], t)
    share = float(cs * np.sqrt(float(h)) * G.max() * ACCURACY)
    err = float(np.abs(xd.cpu().numpy() - ref).max())
    bar = TOL_STEP * float(np.abs(ref).max()) + share
    print(f"sde_step {sde} {'fourier' if fourier else 'unit'} {shape} tag {tag}: abs err {err:.2e}, bar {bar:.2e} "
          f"(draw's share {share:.2e}); of the max-norm {err / np.abs(ref).max():.2e}")
    assert err <= bar
    # the tag is the stream: the other tag's draws are not these
    other = P.em_step(sde, SDES[sde], t, x, s, PR.sample_normals(seed, 5 - tag, off, shape), G, float(h))
    assert np.abs(xd.cpu().numpy() - other).max() > 1e3 * bar


# ------------------------------------------------------------------ 4. ffd_langevin_step ----
@pytest.mark.parametrize("shape", [(3, 21, 3), (3, 20, 4), (2, 187, 1)], ids=ids)
def test_langevin_draws(lib, shape):
    """w = (x' - x - eps u) / sqrt(2 eps) reconstructed as tests/test_pc_gpu.py does, against G z_64 at its 1e-5."""
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn = shape
    G = M.fourier_G(L, True)
    rng = np.random.default_rng(11)
    x, s = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    seed, off, tag = 9, 3, PR.tag_corrector(2, 1, 2)
    xd, sd, Gd = dev(x), dev(s), dev(G)
    x0 = xd.clone()
    eps = torch.empty(B, device="cuda", dtype=torch.float32)
    work = torch.empty(max(lib.ffd_langevin_work_bytes(B, L) // 4, 1) + 4, device="cuda", dtype=torch.float32)
    assert work.data_ptr() % 16 == 0
    d = desc("ve")
    assert lib.ffd_langevin_step(C_.byref(d), xd.data_ptr(), sd.data_ptr(), Gd.data_ptr(), 0.5, 1.0 / 12.0, 0.16,
                                 N.FFD_LANGEVIN_NORM_SAMPLE, None, seed, off, tag, B, L, Cn, eps.data_ptr(), work.data_ptr(),
                                 stream()) == 0
    w = reconstruct_w(x0, sd, xd, eps, G)
    want = G.astype(np.float64)[None, :, None] * PR.sample_normals(seed, tag, off, shape)
    err = float(np.abs(w - want).max())
    print(f"langevin {shape}: max |w - G z_64| {err:.2e}")
    assert float(eps.min()) > 0 and err <= 1e-5


# ------------------------------------------------------------------ 5. projection and transition ----
def scheduler(sde, L, fourier=True):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=fourier, **SDES[sde])
    sch.set_noise_scaling(L)
    return sch


# general length (k_cond_project), power of two with float4 slabs and without, the time domain's float4 / scalar kernels
COND_SHAPES = [(4, 21, 3), (4, 20, 4), (2, 16, 4), (2, 64, 3), (3, 7, 1)]


@pytest.mark.parametrize("domain", ["frequency", "time"])
@pytest.mark.parametrize("shape", COND_SHAPES, ids=ids)
def test_cond_project_draws(lib, shape, domain):
    """mask 1, x = obs = 0 (VE): the output is (sigma G_l) z over the PACKED layout, g = (sample_offset + b) L C + i.
    Time domain: two fp32 roundings on top of the draw.  Frequency domain: the two transforms add their rounding, so
    the recovered draw is held to the identity bar."""
    import cond_restatement as CR

    B, L, Cn = shape
    sch = scheduler("ve", L)
    G = sch.G.numpy().astype(np.float64)[None, :, None]
    _, sigma = CR.coefficients("ve", SDES["ve"], 0.5)
    zero, ones = torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda")
    seed, off, tag = (1 << 63) + 5, 3, PR.tag_projection(4, 1, 1)
    out = sch.cond_project(zero, zero, ones, 0.5, domain=domain, seed=seed, sample_offset=off, tag=tag).prev_sample
    z = out.cpu().numpy().astype(np.float64) / (float(np.float32(sigma)) * G)
    want = PR.sample_normals(seed, tag, off, shape)
    err = np.abs(z - want)
    print(f"cond_project {domain} {shape}: max |z - z_64| {err.max():.2e}")
    if domain == "time":
        assert np.all(err <= ACCURACY + 3 * 2.0 ** -24 * np.abs(want))
    else:
        assert err.max() <= IDENTITY


@pytest.mark.parametrize("shape", [(4, 21, 3), (4, 20, 4), (2, 187, 1)], ids=ids)
def test_forward_transition_draws(lib, shape):
    """x = 0 (VE): the output is (sg G_l) z, two fp32 roundings on top of the draw."""
    B, L, Cn = shape
    sch = scheduler("ve", L)
    G = sch.G.numpy().astype(np.float64)[None, :, None]
    _, sg = RS.transition_coefficients("ve", SDES["ve"], 0.25, 0.5)
    seed, off, tag = 9, 3, PR.tag_transition(2)
    out = sch.forward_transition(torch.zeros(shape, device="cuda"), 0.25, 0.5, seed=seed, sample_offset=off, tag=tag).prev_sample
    z = out.cpu().numpy().astype(np.float64) / (float(np.float32(sg)) * G)
    want = PR.sample_normals(seed, tag, off, shape)
    err = np.abs(z - want)
    print(f"forward_transition {shape}: max |z - z_64| {err.max():.2e}")
    assert np.all(err <= ACCURACY + 3 * 2.0 ** -24 * np.abs(want))


# ------------------------------------------------------------------ 6. ffd_sm_perturb ----
PERTURB = [((2, 5, 3), 0, 0), ((5, 187, 1), 7, 0), ((2, 64, 8), 7, 0), ((3, 24, 40), 0, 0), ((2, 64, 8), 3, 1), ((4, 5, 3), 7, 2)]


@pytest.mark.parametrize("shape,off,shift", PERTURB, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_sm_perturb_draws(lib, shape, off, shift):
    """mean_coeff x0 + sigma G z_64 in float64, at tests/test_loss_gpu.py's 5e-7 of the max-norm"""
    B, L, Cn = shape
    rng = np.random.default_rng(5 + 1000 * B + L)
    x0 = rng.standard_normal(shape).astype(np.float32)
    sigma = np.geomspace(1e-3, 50.0, B).astype(np.float32)
    mc = rng.uniform(0.1, 1.0, B).astype(np.float32)
    G = M.fourier_G(L, True)
    seed = (1 << 40) + 17
    bufs = [dev(x0, shift), dev(np.zeros_like(x0), shift), dev(mc), dev(sigma), dev(G)]
    assert lib.ffd_sm_perturb(*[b.data_ptr() for b in bufs], None, seed, off, B, L, Cn, stream()) == 0
    z = PR.sample_normals(seed, PR.TAG_PERTURB, off, shape)
    ref = mc.astype(np.float64)[:, None, None] * x0 + (sigma.astype(np.float64)[:, None] * G[None, :])[:, :, None] * z
    err = rel_err(bufs[1].cpu().numpy(), ref)
    print(f"sm_perturb {shape} offset {off} +{shift}: {err:.2e} of the max-norm")
    assert err <= TOL_STEP


@pytest.mark.parametrize("lw", [0, 1])
@pytest.mark.parametrize("shape,off,shift", PERTURB, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_sm_loss_regenerates_the_restated_draws(lib, shape, off, shift, lw):
    """ffd_sm_loss with z = NULL walks the quads of the global element index on its own: its per-sample losses against the
    float64 loss of the restated draws, at tests/test_loss_gpu.py's 2e-6 per sample.  The score is O(1 / std) like the
    target, so a wrong draw moves a sample's loss by O(1)."""
    from test_loss_host import loss_f64

    B, L, Cn = shape
    rng = np.random.default_rng(9 + 1000 * B + L)
    sigma = np.geomspace(1e-2, 50.0, B).astype(np.float32)
    G = M.fourier_G(L, True)
    std = (sigma[:, None] * G[None, :])[:, :, None]
    score = (rng.standard_normal(shape) / std).astype(np.float32)
    seed = (1 << 40) + 17
    out = torch.empty(B, device="cuda", dtype=torch.float64)
    bufs = [dev(score, shift), dev(sigma), dev(G)]
    assert lib.ffd_sm_loss(*[b.data_ptr() for b in bufs], None, seed, off, lw, 1, out.data_ptr(), B, L, Cn, stream()) == 0
    z = PR.sample_normals(seed, PR.TAG_PERTURB, off, shape)
    ref = loss_f64(score, z, sigma, G, lw, 1)
    err = float(np.abs(out.cpu().numpy() / ref - 1.0).max())
    wrong = loss_f64(score, PR.sample_normals(seed, PR.TAG_PERTURB, off + 1, shape), sigma, G, lw, 1)
    print(f"sm_loss {shape} offset {off} +{shift} lw={lw}: per-sample relative error {err:.2e}")
    assert err <= 2e-6 and np.abs(wrong / ref - 1.0).min() > 1e-3


# ------------------------------------------------------------------ 7. ffd_sm_draw_times ----
@pytest.mark.parametrize("offset", [0, 1, 2, 3, (1 << 34) - 2, (1 << 40) + 1], ids=lambda o: f"off{o:#x}")
@pytest.mark.parametrize("B", [1, 5, 1027])
def test_draw_times_bit_for_bit(lib, B, offset):
    """t = min(u (T - eps) + eps, T), every step rounded to fp32, u = (w >> 8) 2^-24 of the word of global sample
    sample_offset + b: restated bit for bit."""
    eps, T, seed = 1e-5, 1.0, (1 << 63) + 5
    t = torch.empty(B, device="cuda", dtype=torch.float32)
    assert lib.ffd_sm_draw_times(t.data_ptr(), B, eps, T, seed, offset, stream()) == 0
    u = PR.uniforms(seed, PR.TAG_TIMES, offset, B)
    assert u.dtype == np.float32
    want = np.minimum(u * np.float32(T - eps) + np.float32(eps), np.float32(T))
    assert want.dtype == np.float32 and np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if B > 1000:
        assert len(set(want.tolist())) > B - 3


# ------------------------------------------------------------------ 8. the limits ----
def mixture_model(sde, shape):
    """(module, scheduler, the float64 score function) of a small mixture with well-spread means and v > 0"""
    B, L, Cn, K = shape
    rng = np.random.default_rng(40 + L + K)
    mu = rng.standard_normal((K, L, Cn)).astype(np.float32)
    lw = np.log(rng.dirichlet(np.full(K, 2.0))).astype(np.float32)
    var = M.variance(L, Cn, 1)
    m, sch = module(sde, mu, lw, var)
    return m, sch


def test_loop_entries_enforce_the_limits_of_the_plan(lib):
    """Empty runs (n_run = 0) at each limit and one past it: FFD_OK and FFD_ERR_INVALID.  Ties PR.LIMIT_* -- which
    tests/test_philox_host.py shows to keep the tag families apart -- to what the library accepts."""
    from fastfourierdiffusion_amd import _native as N

    B, L, Cn = 2, 8, 4
    m, sch = mixture_model("ve", (B, L, Cn, 3))
    ctx = m._ctx()
    x = torch.zeros((B, L, Cn), device="cuda")
    obs, mask = torch.zeros((1, L, Cn), device="cuda"), torch.ones((1, L, Cn), device="cuda")
    cfg = N.CondCfg(obs.data_ptr(), mask.data_ptr(), None, 1, N.FFD_COND_TIME, 0, 0)
    s = stream()

    def call(entry, n_steps, n_corr, resample=1):
        ts = (C_.c_float * n_steps)(*np.linspace(1.0, 1e-5, n_steps).tolist())
        head = (ctx.handle, x.data_ptr(), B, ts, n_steps, 0.1, 0, 0)
        if entry == "pc":
            return lib.ffd_sample_batch_pc(*head, n_corr, 0.16, 0, 9, 0, None, 0, 0, s)
        if entry == "cond":
            return lib.ffd_sample_batch_cond(*head, n_corr, 0.16, 0, 9, 0, None, 0, 0, C_.byref(cfg), s)
        return lib.ffd_sample_batch_resample(*head, 1, resample, n_corr, 0.16, 0, 9, 0, None, C_.byref(cfg), s)

    for n_steps in (1, 16):
        assert call("pc", n_steps, PR.LIMIT_PC // n_steps) == 0
        assert call("pc", n_steps, PR.LIMIT_PC // n_steps + 1) == -1
        assert call("cond", n_steps, PR.LIMIT_COND // n_steps - 1) == 0
        assert call("cond", n_steps, PR.LIMIT_COND // n_steps) == -1
        assert call("resample", n_steps, PR.LIMIT_RESAMPLE // n_steps - 1) == 0
        assert call("resample", n_steps, PR.LIMIT_RESAMPLE // n_steps) == -1
        assert call("resample", n_steps, PR.LIMIT_RESAMPLE // (2 * n_steps) - 1, resample=2) == 0
        assert call("resample", n_steps, PR.LIMIT_RESAMPLE // (2 * n_steps), resample=2) == -1
    assert not x.any()


# ------------------------------------------------------------------ 9. the tag plan, end to end ----
N_STEPS = 8
RUNS = {
    "sample": dict(),
    "sample_correctors": dict(n_corr=2),
    "conditional": dict(n_corr=1, cond=True),
    "conditional_no_corrector": dict(n_corr=0, cond=True),
    "resampled": dict(n_corr=1, cond=True, resample=2, jump=3),
    "ode_heun": dict(solver="ode_heun"),
}
WORST = {}


def restated_draws(run, shape, seed, off):
    """the draws of a whole run in the order the loop consumes them, rounded to fp32: the prior's, then per step / visit
    each update's own (correctors in order, then the predictor) with its projection's behind it, then the transition's"""
    zs = [PR.sample_normals(seed, PR.TAG_PRIOR, off, shape)]
    if "solver" not in run:
        sched = PR.schedule_tags(N_STEPS, run.get("n_corr", 0), run.get("cond", False), run.get("jump", 1), run.get("resample", 1))
        zs += [PR.sample_normals(seed, tag, off, shape) for _, tag in sched]
    return [z.astype(np.float32) for z in zs]


@pytest.mark.parametrize("seed,off", [(5, 0), ((1 << 40) + 17, 3)], ids=["seed5", "seed2^40+17-off3"])
@pytest.mark.parametrize("name", sorted(RUNS))
@pytest.mark.parametrize("shape", [(3, 8, 4, 5), (3, 7, 3, 5)], ids=ids)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_philox_run_is_the_run_with_the_restated_draws_injected(lib, sde, shape, name, seed, off):
    """A wrong tag, index or seed half anywhere in the plan gives an O(1) difference; the restated draws rounded to fp32
    differ from the device's by the draw error, so the two runs agree as two roundings of one trajectory do."""
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    run = RUNS[name]
    B, L, Cn, K = shape
    m, sch = mixture_model(sde, shape)
    kw = dict(score_model=m, sample_batch_size=B, corrector_steps=run.get("n_corr", 0), snr=0.16,
              solver=run.get("solver", "euler_maruyama"))
    rng = np.random.default_rng(70 + K + L)
    series = torch.from_numpy(rng.standard_normal((L, Cn)).astype(np.float32))
    mask = torch.zeros((L, Cn))
    mask[: L // 3 + 1] = 1.0

    def go(sampler):
        if run.get("cond"):
            return sampler.sample_conditional(series, mask, B, N_STEPS, run.get("resample", 1), run.get("jump", 1))
        return sampler.sample(num_samples=B, num_diffusion_steps=N_STEPS)

    device = go(DiffusionSampler(rng="philox", seed=seed, sample_offset=off, **kw))
    zs = restated_draws(run, (B, L, Cn), seed, off)
    injected = DiffusionSampler(**kw)
    injected.inject_noise(zs)
    want = go(injected)
    assert next(injected._injected, None) is None  # every restated draw was consumed: the count is the plan's
    err = rel_err(device, want)
    WORST[name] = max(WORST.get(name, 0.0), err)
    print(f"{name} {sde} {shape} seed {seed:#x} offset {off}: rel err {err:.3e} ({len(zs)} draws); worst so far {WORST[name]:.3e}")
    assert bool(torch.isfinite(device).all()) and err < TOL_TRAJ
