"""GPU tests of the Fourier kernels over their whole length range (csrc/ffd_fft.hip, the transform inside
csrc/ffd_spectral.hip), through the Python surface, against float64.

Reference: ``numpy.fft`` on float64 input with ``norm="ortho"``, packed like ``oracle.ffd_oracle.dft`` / ``idft``
(tests/spectral_restatement.py: ``pack_dft`` / ``unpack_idft``; tests/test_fourier_limits_host.py ties the two
references together at L = 509 and 512 -- the oracle's explicit DFT matrices would take 0.5 GB at L = 8192).

Bars: the project's single-operator bar TOL_OP = 2e-6 (max-abs error over the output's max-norm) for dft, idft, the
standardising wrappers, FreSca and the decomposition, 2 TOL_OP for a dft -> idft round trip (tests/test_gpu_parity.py);
k TOL_OP with the per-quantity k of tests/spectral_restatement.py for the spectral consumers.  torch's own fp32 rfft
is 1.7e-7 .. 3.6e-7 off float64 at these lengths on the CPU, so four times the reference's error stays below the floor.

The shapes are the ones the suite did not reach: a single prime radix up to 6823 (one butterfly output is a sum of R
products: a plain fp32 chain is 2e-6 .. 4e-6 off at R >= 2039, the compensated one of stockham() is not), a small factor
times a large prime, many odd passes, more than 64 KiB of dynamic LDS (any length that is not a power of two above 2730),
the longest supported length of either kind, power-of-two channel groups with a short last group, and the persistent
sample loop of k_rfft_pow2 (a workgroup taking a second sample, with and without the register prefetch)."""
import functools
import math

import numpy as np
import pytest
import torch

import spectral_restatement as R
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6
LDS_CAP = 160 * 1024
MAX_MIXED = 6826  # the longest supported length that is not a power of two: 3 L float2 <= 160 KiB


@pytest.fixture(scope="module")
def ffd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):  # the in-tree build normally travels with the snapshot
        from fastfourierdiffusion_amd.build import build

        build()
    _native.lib()  # fail loudly if libffd.so cannot be loaded
    return pkg


# ---- the launch geometry of ffd_fft.hip, restated (a test fails loudly when a rule changes under it) ---------------
def is_pow2(L):
    return L >= 2 and L & (L - 1) == 0


def lds_bytes(L, CG):
    """twiddle table + two slabs of CG channels (fft_lds_bytes)."""
    return 8 * L * (1 + CG if is_pow2(L) else 1 + 2 * CG)


def channel_group(L, C):
    """pow2_cg / the loop of launch_dft: the whole slab when a power of two fits 160 KiB, else halve down to 64 KiB."""
    if is_pow2(L) and lds_bytes(L, C) <= LDS_CAP:
        return C
    CG = C
    while CG > 1 and lds_bytes(L, CG) > 64 * 1024:
        CG = (CG + 1) // 2
    return CG


def group_sizes(L, C):
    CG = channel_group(L, C)
    return [min(CG, C - c0) for c0 in range(0, C, CG)]


def grid_cap(L, C):
    """persistent_blocks: 256 CUs times the workgroups the LDS image lets a CU hold, at most 8."""
    return 256 * min(8, max(1, LDS_CAP // lds_bytes(L, channel_group(L, C))))


def test_geometry_of_the_listed_shapes():
    assert lds_bytes(MAX_MIXED, 1) <= LDS_CAP < lds_bytes(MAX_MIXED + 1, 1)
    assert group_sizes(4095, 3) == [1, 1, 1] and lds_bytes(4095, 1) > 64 * 1024
    assert group_sizes(8192, 3) == [1, 1, 1] and lds_bytes(8192, 1) > 64 * 1024
    assert group_sizes(1024, 21) == [6, 6, 6, 3]  # a short last group
    assert group_sizes(2048, 11) == [3, 3, 3, 2]
    assert group_sizes(4096, 3) == [3] and lds_bytes(4096, 3) > 64 * 1024
    for L in (2731, 4093, 6823, MAX_MIXED):  # any other length above 2730: the hipFuncSetAttribute branch
        assert lds_bytes(L, 1) > 64 * 1024 >= lds_bytes(2730, 1)


# ---- inputs and float64 references, made once per shape --------------------------------------------------------------
def seed_of(B, L, C):
    return 31000 + 7 * L + 13 * C + B


@functools.lru_cache(maxsize=None)
def case(B, L, C):
    """(x fp32, float64 packed dft(x), float64 idft(x)); read-only."""
    x = next(synthetic.noise_stream((B, L, C), 1, seed_of(B, L, C)))
    out = (x, R.pack_dft(x), R.unpack_idft(x))
    for a in out:
        a.setflags(write=False)
    return out


def gpu(a):
    return torch.tensor(np.asarray(a, dtype=np.float32)).cuda()  # a copy: the cached inputs stay read-only


def check_dft_idft(B, L, C):
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    x, fwd, inv = case(B, L, C)
    xd = gpu(x)
    X = dft(xd)
    e_f, e_i = rel_err(X.cpu(), fwd), rel_err(idft(xd).cpu(), inv)
    e_rt = rel_err(idft(X).cpu(), x)
    print(f"({B}, {L}, {C}): dft {e_f:.2e} idft {e_i:.2e} round trip {e_rt:.2e}")
    assert e_f < TOL_OP, ("dft", e_f)
    assert e_i < TOL_OP, ("idft", e_i)
    assert e_rt < 2 * TOL_OP, ("round trip", e_rt)


def check_wrappers(B, L, C):
    from fastfourierdiffusion_amd.utils.fourier import dft_standardize, unstandardize_idft

    x, fwd, _ = case(B, L, C)
    rng = np.random.Generator(np.random.PCG64(seed_of(B, L, C) + 1))
    mean = (0.5 * rng.standard_normal((L, C))).astype(np.float32)
    std = rng.uniform(0.5, 1.5, (L, C)).astype(np.float32)
    m64, s64 = mean.astype(np.float64), std.astype(np.float64)
    got = dft_standardize(gpu(x), torch.from_numpy(mean), torch.from_numpy(std))
    e_f = rel_err(got.cpu(), (fwd - m64) / s64)
    got = unstandardize_idft(gpu(x), torch.from_numpy(mean), torch.from_numpy(std))
    e_i = rel_err(got.cpu(), R.unpack_idft(x.astype(np.float64) * s64 + m64))
    print(f"({B}, {L}, {C}): dft_standardize {e_f:.2e} unstandardize_idft {e_i:.2e}")
    assert e_f < TOL_OP, ("dft_standardize", e_f)
    assert e_i < TOL_OP, ("unstandardize_idft", e_i)


# (B, L, C, also the standardising wrappers)
RANGE_SHAPES = [
    (2, 1021, 3, True), (2, 2039, 2, False), (1, 4093, 1, True), (1, 6823, 1, False),  # one large prime radix
    (1, 3063, 2, False), (2, 4078, 1, False),                                            # 3 * 1021, 2 * 2039
    (2, 6561, 1, False), (2, 6825, 1, True),                                             # 3^8, 3 * 5 * 5 * 7 * 13
    (1, 4095, 3, False),                                                                 # CG = 1 and > 64 KiB of LDS
    (1, MAX_MIXED, 1, False),                                                            # the longest of its kind
    (2, 8192, 1, True), (1, 8192, 3, False),                                             # three one-channel groups
    (2, 1024, 21, False),                                                                # groups 6 + 6 + 6 + 3
]


@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=lambda s: f"B{s[0]}_L{s[1]}_C{s[2]}")
def test_dft_idft_against_float64(ffd, shape):
    B, L, C, wrappers = shape
    if (L, C) == (1024, 21):
        sizes = group_sizes(L, C)
        assert len(set(sizes)) > 1 and sizes[-1] < sizes[0], sizes  # the split is uneven
    check_dft_idft(B, L, C)
    if wrappers:
        check_wrappers(B, L, C)


@pytest.mark.parametrize("shape,cap", [((258, 8192, 1), 256), ((2050, 64, 4), 2048), ((1030, 512, 8), 1024)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"cap{v}")
def test_persistent_sample_loop_against_float64(ffd, shape, cap):
    """More samples than the grid holds: some workgroups of k_rfft_pow2 take a second sample (8192 x 1: no vector path;
    64 x 4: the float4 path with the register prefetch; 512 x 8: the shape-specialised instance)."""
    B, L, C = shape
    assert grid_cap(L, C) == cap < B <= 2 * cap
    assert (C % 4 == 0 and channel_group(L, C) == C and L * C // 4 <= 8 * 256) == (shape != (258, 8192, 1))
    check_dft_idft(B, L, C)


# ---- closed-form inputs ----------------------------------------------------------------------------------------------
CLOSED_L = (2039, 4096, 6825, 8192)
AMP = np.array([1.0, -0.5])  # the two channels carry the same series at these amplitudes (exact in fp32)


def packed(X, L):
    """complex (B, L/2 + 1, C) -> the packed layout (B, L, C)."""
    im = X.imag[:, 1:]
    if L % 2 == 0:
        im = im[:, :-1]
    return np.concatenate([X.real, im], axis=1)


@pytest.mark.parametrize("L", CLOSED_L)
def test_unit_impulse(ffd, L):
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    n0s = (0, 1, L // 2, L - 1)
    x = np.zeros((len(n0s), L, 2))
    k = np.arange(L // 2 + 1)
    X = np.zeros((len(n0s), L // 2 + 1, 2), dtype=np.complex128)
    for b, n0 in enumerate(n0s):
        x[b, n0] = AMP
        phase = -2.0 * np.pi * ((k * n0) % L) / L  # the integer phase reduced exactly
        X[b] = (np.exp(1j * phase) / math.sqrt(L))[:, None] * AMP[None, :]
    want = packed(X, L)
    got = dft(gpu(x)).cpu().numpy().astype(np.float64)
    err = np.max(np.abs(got - want)) * math.sqrt(L)
    back = rel_err(idft(gpu(want)).cpu(), x)
    print(f"L={L}: impulse spectrum off by {err:.2e} of L^-1/2, idft of it off by {back:.2e}")
    assert err < TOL_OP
    assert back < TOL_OP


def coprime_near_a_third(L):
    k = L // 3
    while math.gcd(k, L) != 1:
        k += 1
    return k


@pytest.mark.parametrize("L", CLOSED_L)
def test_single_tone(ffd, L):
    from fastfourierdiffusion_amd.utils.fourier import dft

    k0s = (1, L // 2, coprime_near_a_third(L))
    assert math.gcd(k0s[2], L) == 1 and abs(k0s[2] - L / 3) < 8
    n = np.arange(L)
    x = np.stack([np.cos(2.0 * np.pi * ((k0 * n) % L) / L + 0.3) for k0 in k0s])[:, :, None] * AMP[None, None, :]
    got = dft(gpu(x)).cpu().numpy().astype(np.float64)
    for b, k0 in enumerate(k0s):
        X = np.zeros((1, L // 2 + 1, 2), dtype=np.complex128)
        # a self-paired bin (k0 = L/2, L even) holds both halves of the tone: sqrt(L) cos(0.3), no imaginary part
        X[0, k0] = (math.sqrt(L) * math.cos(0.3) if 2 * k0 == L else 0.5 * math.sqrt(L) * np.exp(0.3j)) * AMP
        want = packed(X, L)[0]
        peak = np.max(np.abs(X[0, k0]))
        at_k0 = np.any(want != 0, axis=1)
        assert at_k0.sum() == (1 if 2 * k0 == L else 2)
        e_bin = np.max(np.abs(got[b][at_k0] - want[at_k0])) / peak
        e_rest = np.max(np.abs(got[b][~at_k0])) / peak
        print(f"L={L} k0={k0}: bin off by {e_bin:.2e}, largest other entry {e_rest:.2e} of the peak")
        assert e_bin < TOL_OP
        assert e_rest < TOL_OP


@pytest.mark.parametrize("L", [L for L in CLOSED_L if L % 2 == 0])
def test_constant_and_alternating_series(ffd, L):
    """The two self-paired rows of the packed layout: X_0 of the constant, X_{L/2} of the alternating series."""
    from fastfourierdiffusion_amd.utils.fourier import dft, idft

    x = np.stack([np.ones(L), (-1.0) ** np.arange(L)])[:, :, None] * AMP[None, None, :]
    want = np.zeros((2, L, 2))
    want[0, 0] = math.sqrt(L) * AMP
    want[1, L // 2] = math.sqrt(L) * AMP
    e_f = rel_err(dft(gpu(x)).cpu(), want)
    e_i = rel_err(idft(gpu(want)).cpu(), x)
    print(f"L={L}: constant / alternating dft {e_f:.2e} idft {e_i:.2e}")
    assert e_f < TOL_OP
    assert e_i < TOL_OP


# ---- FreSca and the decomposition ------------------------------------------------------------------------------------
LOW, HIGH, RATIO = 0.9, 1.4, 0.45
# (B, L, C, seed): the seed is chosen so that the energy cutoff is not a near tie (checked below in float64)
FILTER_SHAPES = [(2, 2039, 1, 41001), (1, 4095, 1, 41022), (1, 4096, 3, 41013), (2, 2048, 11, 41004)]


def irfft64(X, L):
    return np.fft.irfft(X, n=L, axis=1, norm="ortho")


@functools.lru_cache(maxsize=None)
def filter_case(B, L, C, seed):
    x = next(synthetic.noise_stream((B, L, C), 1, seed))
    x.setflags(write=False)
    return x, np.fft.rfft(x.astype(np.float64), axis=1, norm="ortho")


def energy_cutoff(X, ratio):
    """fresca.py:46-58 in float64: Rc = the first bin at which the cumulative batch-mean |X_k| reaches ratio x total;
    also the cumulative shares at Rc - 1 and Rc."""
    share = np.cumsum(np.abs(X).mean(axis=(0, 2)))
    share /= share[-1]
    rc = int(np.argmax(share >= ratio))
    return rc, share[rc - 1], share[rc]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: f"B{s[0]}_L{s[1]}_C{s[2]}")
def test_fresca_against_float64(ffd, shape):
    from fastfourierdiffusion_amd.utils.fresca import frequency_scale

    B, L, C, seed = shape
    x, X = filter_case(*shape)
    nf = L // 2 + 1
    k = torch.arange(nf).float()
    rc, below, at = energy_cutoff(X, RATIO)
    assert 0 < rc < nf - 1 and RATIO - below > 1e-4 and at - RATIO > 1e-4, (rc, below, at)  # no near tie: the fp32
    # cumulative sum of the device picks the same bin
    lows = {"spatial": (k <= RATIO * nf).numpy(), "energy": (k <= rc).numpy()}  # fresca.py:40-43, 54-58
    for strategy, low in lows.items():
        f = np.where(low, np.float32(LOW), np.float32(HIGH)).astype(np.float64)[None, :, None]
        want = irfft64(X * f, L)
        got = frequency_scale(gpu(x), LOW, HIGH, RATIO, strategy)
        err = rel_err(got.cpu(), want)
        print(f"({B}, {L}, {C}) {strategy}: {err:.2e} (Rc = {rc}, shares {below:.5f} / {at:.5f})")
        assert err < TOL_OP, (strategy, err)


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: f"B{s[0]}_L{s[1]}_C{s[2]}")
def test_frequency_decompose_against_float64(ffd, shape):
    from fastfourierdiffusion_amd.utils.fourier import frequency_decompose_fft

    B, L, C, seed = shape
    x, X = filter_case(*shape)
    nf = L // 2 + 1
    n_low = max(1, int(nf * 0.3))  # fourier.py:249
    keep = (np.arange(nf) < n_low)[None, :, None]
    lo, hi = frequency_decompose_fft(gpu(x), 0.3)
    e_lo, e_hi = rel_err(lo.cpu(), irfft64(X * keep, L)), rel_err(hi.cpu(), irfft64(X * ~keep, L))
    print(f"({B}, {L}, {C}) decomposition: low {e_lo:.2e} high {e_hi:.2e}")
    assert e_lo < TOL_OP
    assert e_hi < TOL_OP


# ---- the spectral consumers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6823, 1), (2, 8192, 1)], ids=lambda s: f"B{s[0]}_L{s[1]}_C{s[2]}")
def test_localization_and_profile_against_float64(ffd, shape):
    from fastfourierdiffusion_amd.utils.fourier import localization_metrics
    from fastfourierdiffusion_amd.visualization.spectral_interpretation import spectral_profile

    B, L, C = shape
    x = case(B, L, C)[0]
    got = [t.cpu().numpy() for t in localization_metrics(gpu(x))]
    for name, kk, o, w in zip(("time", "freq"), (1, 3), got, R.localization(x)):
        err = R.rel_to_value(o, w)
        print(f"({B}, {L}, {C}) delocalization {name}: {err:.2e} (bound {kk * R.TOL_OP:.0e})")
        assert err <= kk * R.TOL_OP, (name, err)
    f64 = dict(zip(R.CURVES, R.profile(x)))
    curves = dict(zip(R.CURVES, (t.cpu().numpy() for t in spectral_profile(gpu(x)))))
    for name in R.CURVES:
        err = R.curve_err(name, curves[name], f64, B)
        print(f"({B}, {L}, {C}) {name}: {err:.2e} (bound {R.CURVE_STAGES[name] * R.TOL_OP:.0e})")
        assert err <= R.CURVE_STAGES[name] * R.TOL_OP, (name, err)


def test_smoothing_against_float64_at_a_prime_length(ffd):
    from fastfourierdiffusion_amd.utils.fourier import smooth_frequency

    B, L, C = 2, 2039, 1
    x = case(B, L, C)[0]
    err = rel_err(smooth_frequency(gpu(x), 3.0).cpu(), R.smooth_frequency(x, 3.0))
    print(f"({B}, {L}, {C}) smoothing, sigma 3: {err:.2e} (bound {3 * R.TOL_OP:.0e})")
    assert err <= 3 * R.TOL_OP


# ---- the first refused length ----------------------------------------------------------------------------------------
def test_first_refused_length_raises_and_launches_nothing(ffd):
    from fastfourierdiffusion_amd import _native
    from fastfourierdiffusion_amd.utils.fourier import dft, localization_metrics

    L = MAX_MIXED + 1
    x = torch.zeros(2, L, 1, device="cuda")
    with pytest.raises(NotImplementedError):
        dft(x)
    with pytest.raises(NotImplementedError):
        localization_metrics(x)
    # through the C ABI with scratch of the caller's own sizing: the call returns FFD_ERR_UNSUPPORTED and neither the
    # scratch (where the time-domain rows would go first) nor the outputs are written
    lib = _native.lib()
    assert lib.ffd_localization_work_bytes(2, L, 1) == 0
    nfloat = 2 * L + 2 * (L // 2 + 1) + 2 * 2 * L
    work = torch.full((nfloat,), -7.0, device="cuda")
    out = torch.full((2, 2), -7.0, device="cuda")
    rc = lib.ffd_localization(x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), work.data_ptr(), 4 * nfloat, 2, L, 1,
                              _native.current_stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == -2
    assert bool((work == -7.0).all()) and bool((out == -7.0).all())
