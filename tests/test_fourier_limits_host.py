"""CPU-side tests of the Fourier entry points' length limits (no GPU).

The supported lengths are one predicate (fft_len_supported, csrc/ffd_internal.h) stated in include/ffd.h: a power of two
up to 8192 or any other length up to 6826 for the dft family and the spectral calls, the same set up to 4096 for FreSca
and the decomposition, odd lengths up to 2047 for the smoothing.  Every entry point refuses a length outside its set
with FFD_ERR_UNSUPPORTED before any device call -- the calls below pass dummy pointers on a machine without a device,
so a call that got as far as the HIP runtime would report FFD_ERR_HIP -- and the matching *_work_bytes is 0.

The last test ties the two float64 references of the transform tests together: the numpy.fft packing of
tests/spectral_restatement.py (used for the long lengths of tests/test_fourier_range_gpu.py) against the explicit
DFT matrices of oracle/ffd_oracle.py (too large there)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import spectral_restatement as R
from fastfourierdiffusion_amd.utils import synthetic
from oracle import ffd_oracle as O

OK, INVALID, UNSUPPORTED = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, BIG = 256, 512, 1 << 40  # non-null, 8-byte aligned, distinct addresses; every call must return before using them
MAX_MIXED = 6826               # 3 * 6826 * 8 B = 163 824 B <= 160 KiB < 3 * 6827 * 8 B
FAMILY_REFUSED = (8193, 7001, MAX_MIXED + 1, 8191, 1 << 20)
FILTER_REFUSED = (4097, 8193, 7001, 8192)


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def dft_family(lib):
    """name -> call(L, **overrides) for the four transforms with dummy arguments."""
    def plain(fn):
        return lambda L, src=P, dst=Q, B=2, C=3: fn(src, dst, B, L, C, None)

    def affine(fn):
        return lambda L, src=P, dst=Q, B=2, C=3, mean=P, std=P: fn(src, dst, mean, std, B, L, C, None)

    return {"ffd_dft": plain(lib.ffd_dft), "ffd_idft": plain(lib.ffd_idft),
            "ffd_dft_standardize": affine(lib.ffd_dft_standardize),
            "ffd_unstandardize_idft": affine(lib.ffd_unstandardize_idft)}


def test_header_and_predicate_state_the_same_lengths():
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    internal = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "ffd_internal.h")).read()
    assert "Supported transform lengths" in header
    for figure in ("8192", str(MAX_MIXED), "4096", "2047"):
        assert figure in header[header.index("Supported transform lengths"):], figure
    assert "fft_len_supported" in internal and f"FFT_MAX_MIXED_LEN == {MAX_MIXED}" in internal
    assert 3 * MAX_MIXED * 8 <= 160 * 1024 < 3 * (MAX_MIXED + 1) * 8


@pytest.mark.parametrize("L", FAMILY_REFUSED)
def test_dft_family_refuses_unsupported_lengths_before_any_device_call(lib, L):
    for name, call in dft_family(lib).items():
        assert call(L) == UNSUPPORTED, name
        assert call(L, B=0) == UNSUPPORTED, name  # an empty batch does not hide the length


def test_dft_family_invalid_arguments_at_supported_lengths(lib):
    for L in (1, 509, 4096, MAX_MIXED, 8192):
        for name, call in dft_family(lib).items():
            assert call(L, src=None) == INVALID, (name, L)
            assert call(L, dst=None) == INVALID, (name, L)
            assert call(L, dst=P) == INVALID, (name, L)  # in place
            assert call(L, B=-1) == INVALID, (name, L)
            assert call(L, C=0) == INVALID, (name, L)
            if "standard" in name:
                assert call(L, mean=None) == INVALID, (name, L)
                assert call(L, std=None) == INVALID, (name, L)
    for name, call in dft_family(lib).items():
        assert call(0) == INVALID and call(-5) == INVALID, name
        assert call(MAX_MIXED, B=0) == OK and call(8192, B=0) == OK, name  # nothing to do: no device call either


@pytest.mark.parametrize("L", FILTER_REFUSED)
def test_fresca_and_decomposition_refuse_unsupported_lengths(lib, L):
    # ffd_fresca(in, out, work, B, L, C, low, high, cutoff_ratio, strategy, stream)
    for strategy in (0, 1):
        assert lib.ffd_fresca(P, Q, P, 2, L, 3, 0.9, 1.4, 0.45, strategy, None) == UNSUPPORTED, strategy
    # ffd_freq_decompose(x, low, high, B, L, D, low_freq_ratio, stream)
    assert lib.ffd_freq_decompose(P, Q, 3 * P, 2, L, 3, 0.3, None) == UNSUPPORTED


def test_fresca_and_decomposition_invalid_arguments_at_supported_lengths(lib):
    for L in (2, 2039, 4095, 4096):
        good = [P, Q, P, 2, L, 3, 0.9, 1.4, 0.45, 1, None]
        for k, bad in ((0, None), (1, None), (1, P), (2, None), (3, 0), (5, 0), (9, 2), (9, -1)):
            a = list(good)
            a[k] = bad
            assert lib.ffd_fresca(*a) == INVALID, (L, k, bad)
        good = [P, Q, 3 * P, 2, L, 3, 0.3, None]
        for k, bad in ((0, None), (1, None), (2, None), (1, P), (2, P), (2, Q), (3, 0), (5, 0)):
            a = list(good)
            a[k] = bad
            assert lib.ffd_freq_decompose(*a) == INVALID, (L, k, bad)
    assert lib.ffd_fresca(P, Q, P, 2, 1, 3, 0.9, 1.4, 0.45, 1, None) == INVALID  # L = 1: no frequency axis to cut
    assert lib.ffd_freq_decompose(P, Q, 3 * P, 2, 1, 3, 0.3, None) == INVALID


@pytest.mark.parametrize("L", FAMILY_REFUSED)
def test_spectral_calls_refuse_unsupported_lengths_and_size_no_scratch(lib, L):
    ms = (C.c_float * 9)()
    assert lib.ffd_localization_work_bytes(2, L, 3) == 0
    assert lib.ffd_spectral_profile_work_bytes(2, L, 3) == 0
    assert lib.ffd_smooth_frequency_work_bytes(2, L, 3) == 0
    assert lib.ffd_localization(P, P, P, P, BIG, 2, L, 3, None) == UNSUPPORTED
    assert lib.ffd_localization_bench(P, 1, P, P, P, BIG, 2, L, 3, 1, 1, ms, None) == UNSUPPORTED
    assert lib.ffd_spectral_profile(P, P, P, P, P, P, BIG, 2, L, 3, None) == UNSUPPORTED
    if L % 2:  # an even length is the smoothing's own FFD_ERR_INVALID
        assert lib.ffd_smooth_frequency(P, Q, P, BIG, 2, L, 3, 1.5, None) == UNSUPPORTED


def test_work_bytes_are_zero_for_exactly_the_refused_shapes(lib):
    for L in (1, 5, 2039, 4096, 6823, MAX_MIXED, 8192):
        need = lib.ffd_localization_work_bytes(2, L, 3)
        assert need == 4 * (2 * L * 3 + 2 * (L // 2 + 1) * 3 + 2 * 2 * L), L
        assert lib.ffd_spectral_profile_work_bytes(2, L, 3) > 0, L
        # a supported length with an invalid argument is still FFD_ERR_INVALID
        assert lib.ffd_localization(P, P, P, P, need - 1, 2, L, 3, None) == INVALID, L
        assert lib.ffd_localization(P, None, P, P, BIG, 2, L, 3, None) == INVALID, L
        assert lib.ffd_spectral_profile(P, P, P, P, P, P + 4, BIG, 2, L, 3, None) == INVALID, L  # misaligned scratch
        assert lib.ffd_spectral_profile(P, P, P, P, P, P, 8, 2, L, 3, None) == INVALID, L
    for L in (MAX_MIXED + 1, 7001, 8191, 8193):
        assert lib.ffd_localization_work_bytes(2, L, 3) == 0 and lib.ffd_spectral_profile_work_bytes(2, L, 3) == 0, L
    # the smoothing: odd lengths up to 2047; an even one is refused too (FFD_ERR_INVALID) and sizes nothing
    for L, want in ((1, True), (2039, True), (2047, True), (2049, False), (2038, False), (2, False), (8193, False)):
        got = lib.ffd_smooth_frequency_work_bytes(2, L, 3)
        assert (got == 4 * (L * L + 2 * L * 3)) if want else (got == 0), L
    assert lib.ffd_smooth_frequency(P, Q, P, 4 * (2039 * 2039 + 2 * 2039 * 3) - 1, 2, 2039, 3, 1.5, None) == INVALID
    assert lib.ffd_smooth_frequency(P, Q, P, BIG, 2, 2039, 3, 0.0, None) == INVALID
    # batch and channel limits refuse in the same way at a supported length
    assert lib.ffd_localization_work_bytes((1 << 24) + 1, 5, 1) == 0
    assert lib.ffd_localization(P, P, P, P, BIG, (1 << 24) + 1, 5, 1, None) == UNSUPPORTED
    assert lib.ffd_smooth_frequency_work_bytes(1 << 24, 5, 1 << 16) == 0  # B C > 2^30 series
    assert lib.ffd_smooth_frequency(P, Q, P, BIG, 1 << 24, 5, 1 << 16, 1.5, None) == UNSUPPORTED


@pytest.mark.parametrize("L", (509, 512))
def test_numpy_fft_packing_equals_the_explicit_matrix_oracle(L):
    """Before rounding to fp32, float64 numpy.fft packed like fourier.py:8-94 equals the explicit fp64 DFT sums of
    oracle.ffd_oracle.dft / idft to 1e-12 of the output's max-norm; rounded, the sums are the oracle's own output."""
    x = next(synthetic.noise_stream((3, L, 2), 1, 4242 + L))
    xd = x.astype(np.float64)
    cr, ci = O._dft_mats(L)
    re, im = np.einsum("kn,bnc->bkc", cr, xd), np.einsum("kn,bnc->bkc", ci, xd)
    fwd = np.concatenate([re, im[:, 1:L - (L // 2 + 1) + 1]], axis=1)
    assert np.array_equal(fwd.astype(np.float32), O.dft(torch.from_numpy(x)).numpy())
    got = R.pack_dft(x)
    assert got.shape == fwd.shape == (3, L, 2)
    assert np.max(np.abs(got - fwd)) <= 1e-12 * np.max(np.abs(fwd))
    n_real = L // 2 + 1
    w = np.full(n_real, 2.0)
    w[0] = 1.0
    if L % 2 == 0:
        w[-1] = 1.0
    sre, sim = xd[:, :n_real], np.zeros((3, n_real, 2))
    sim[:, 1:1 + (L - n_real)] = xd[:, n_real:]
    inv = np.einsum("kn,bkc->bnc", cr * w[:, None], sre) + np.einsum("kn,bkc->bnc", ci * w[:, None], sim)
    assert np.array_equal(inv.astype(np.float32), O.idft(torch.from_numpy(x)).numpy())
    got = R.unpack_idft(x)
    assert np.max(np.abs(got - inv)) <= 1e-12 * np.max(np.abs(inv))
    assert np.max(np.abs(R.unpack_idft(R.pack_dft(x)) - xd)) <= 1e-12 * np.max(np.abs(xd))
