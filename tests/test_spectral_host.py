"""CPU-side tests of the localization metrics, the frequency smoothing and the spectral profiles (no GPU): the float64
restatement the device tests compare against reproduces every case of tests/golden/g17_spectral.npz (written by
tools/gen_spectral_golden.py from the unmodified reference), the new entry points are exported, declared and check their
arguments before any device work, and the Python surface resolves through the ``fdiff`` alias."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import spectral_restatement as R

INVALID, UNSUPPORTED = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ffd_localization", "ffd_localization_work_bytes", "ffd_smooth_frequency", "ffd_smooth_frequency_work_bytes",
               "ffd_spectral_profile", "ffd_spectral_profile_work_bytes", "ffd_localization_lds_max_len",
               "ffd_localization_bench"]


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def max_norm_err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("case", R.LOC_CASES, ids=lambda c: R.loc_key(*c))
def test_restatement_reproduces_the_reference_localization_and_profiles(golden, case):
    g = golden["g17_spectral"]
    key = R.loc_key(*case)
    x = g[key + "_x"]
    assert x.shape == (R.LOC_B, case[0], case[1]) and x.dtype == np.float32
    for name, k, f64 in zip(("time", "freq"), (1, 3), R.localization(x)):
        np.testing.assert_allclose(f64, g[f"{key}_f64_{name}"], rtol=1e-12)
        tol = float(g[f"{key}_tol_{name}"])
        err = R.rel_to_value(g[f"{key}_ref_{name}"], f64)
        print(f"{key} {name}: reference off by {err:.2e}, tol {tol:.2e}")
        assert k * R.TOL_OP <= tol <= 2e-5 and 4 * err <= tol
    if case not in R.PROFILE_CASES:
        return
    for B in R.PROFILE_B:
        f64 = dict(zip(R.CURVES, R.profile(x[:B])))
        for name in R.CURVES:
            np.testing.assert_allclose(f64[name], g[f"{key}_B{B}_f64_{name}"], rtol=1e-10)
            tol = float(g[f"{key}_B{B}_tol_{name}"])
            err = R.curve_err(name, g[f"{key}_B{B}_ref_{name}"], f64, B)
            assert R.CURVE_STAGES[name] * R.TOL_OP <= tol <= 2e-5 and 4 * err <= tol, (name, B, err, tol)


@pytest.mark.parametrize("L", R.SMOOTH_L)
def test_restatement_reproduces_the_reference_smoothing(golden, L):
    g = golden["g17_spectral"]
    x = g[f"smooth_L{L}_x"]
    assert x.shape == (R.SMOOTH_B, L, R.SMOOTH_C)
    for sigma in R.SMOOTH_SIGMA:
        key = R.smooth_key(L, sigma)
        f64 = R.smooth_frequency(x, sigma)
        np.testing.assert_allclose(f64, g[key + "_f64"], rtol=1e-10, atol=1e-14)
        tol = float(g[key + "_tol"])
        assert 3 * R.TOL_OP <= tol <= 2e-5 and 4 * max_norm_err(g[key + "_ref"], f64) <= tol
        if L == 1:
            np.testing.assert_array_equal(f64, x.astype(np.float64))  # the identity


def test_restatement_properties():
    # the kernel of an even length has L - 1 rows: the reference's einsum raises (fourier.py:201-214)
    with pytest.raises(AssertionError):
        R.smoothing_kernel(24, 2.0)
    W = R.smoothing_kernel(25, 50.0)
    np.testing.assert_allclose(W.sum(axis=0), 1.0, rtol=1e-13)
    assert np.ptp(W) < 0.04 * W.max()  # near-constant columns
    # an impulse: time delocalization 0, flat spectrum
    for L in (33, 64):
        x = np.zeros((1, L, 2))
        x[0, L // 2, 1] = 3.0
        t, f = R.localization(x)
        assert t[0] == 0.0 and abs(f[0] - R.flat_delocalization(L)) <= 1e-12 * f[0]
    t, f = R.localization(np.zeros((2, 9, 1)))
    assert np.isnan(t).all() and np.isnan(f).all()
    assert np.isnan(R.profile(np.ones((1, 5, 2)))[1]).all()  # B = 1: no spread


def test_new_symbols_are_exported_and_declared(lib):
    from fastfourierdiffusion_amd import _native

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    makefile = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "Makefile")).read()
    assert "ffd_spectral.hip" in makefile
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]


def test_entry_points_reject_bad_arguments_without_a_device(lib):
    p = 256  # a non-null, 8-byte aligned address; every call below must return before it is used
    big = 1 << 40
    # ffd_localization(x, time_out, freq_out, work, work_bytes, B, L, C, stream)
    good = [p, p, p, p, big, 2, 5, 3, None]
    for k in (0, 1, 2, 3):
        a = list(good)
        a[k] = None
        assert lib.ffd_localization(*a) == INVALID, k
    for k in (5, 6, 7):
        a = list(good)
        a[k] = 0
        assert lib.ffd_localization(*a) == INVALID, k
    a = list(good)
    a[6] = 8193
    assert lib.ffd_localization(*a) == UNSUPPORTED
    need = lib.ffd_localization_work_bytes(2, 5, 3)
    assert need == 4 * (2 * 5 * 3 + 2 * 3 * 3 + 2 * 2 * 5)
    a = list(good)
    a[4] = need - 1
    assert lib.ffd_localization(*a) == INVALID
    assert lib.ffd_localization_work_bytes(0, 5, 3) == 0 and lib.ffd_localization_work_bytes(2, 8193, 3) == 0
    # ffd_smooth_frequency(x, out, work, work_bytes, B, L, C, sigma, stream)
    good = [p, 2 * p, p, big, 2, 5, 3, 1.5, None]
    for k in (0, 1, 2):
        a = list(good)
        a[k] = None
        assert lib.ffd_smooth_frequency(*a) == INVALID, k
    for k in (4, 5, 6):
        a = list(good)
        a[k] = 0
        assert lib.ffd_smooth_frequency(*a) == INVALID, k
    for L in (2, 24, 2048):  # even lengths: the reference raises
        a = list(good)
        a[5] = L
        assert lib.ffd_smooth_frequency(*a) == INVALID, L
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        a = list(good)
        a[7] = sigma
        assert lib.ffd_smooth_frequency(*a) == INVALID, sigma
    a = list(good)
    a[1] = a[0]
    assert lib.ffd_smooth_frequency(*a) == INVALID  # in place
    a = list(good)
    a[5] = 2049
    assert lib.ffd_smooth_frequency(*a) == UNSUPPORTED
    need = lib.ffd_smooth_frequency_work_bytes(2, 5, 3)
    assert need == 4 * (5 * 5 + 2 * 5 * 3)
    a = list(good)
    a[3] = need - 1
    assert lib.ffd_smooth_frequency(*a) == INVALID
    assert lib.ffd_smooth_frequency_work_bytes(2, 2049, 3) == 0
    # ffd_spectral_profile(x, spec_mean, spec_se, energy_mean, energy_std, work, work_bytes, B, L, C, stream)
    good = [p, p, p, p, p, p, big, 2, 5, 3, None]
    for k in range(6):
        a = list(good)
        a[k] = None
        assert lib.ffd_spectral_profile(*a) == INVALID, k
    for k in (7, 8, 9):
        a = list(good)
        a[k] = 0
        assert lib.ffd_spectral_profile(*a) == INVALID, k
    a = list(good)
    a[8] = 8193
    assert lib.ffd_spectral_profile(*a) == UNSUPPORTED
    a = list(good)
    a[6] = lib.ffd_spectral_profile_work_bytes(2, 5, 3) - 1
    assert a[6] > 0 and lib.ffd_spectral_profile(*a) == INVALID
    a = list(good)
    a[5] = p + 4  # scratch that is not 8-byte aligned
    assert lib.ffd_spectral_profile(*a) == INVALID
    # ffd_localization_bench(x, n_inputs, time_out, freq_out, work, work_bytes, B, L, C, warmup, iters, ms_out, stream)
    ms = (C.c_float * 9)()
    good = [p, 1, p, p, p, big, 2, 5, 3, 1, 1, ms, None]
    for k, bad in ((0, None), (1, 0), (4, None), (6, 0), (9, -1), (10, 0), (11, None)):
        a = list(good)
        a[k] = bad
        assert lib.ffd_localization_bench(*a) == INVALID, k


def test_lds_limit_of_the_product_kernel(lib):
    """The product kernel keeps a block of 32 rows, each padded to a multiple of 4 plus 2 floats, and 4 x 32 floats of
    minima in at most 144 KiB of LDS: (128 + 32 (4 ceil(L / 4) + 2)) 4 bytes is 147 200 at L = 1144 and 147 712 at 1145.
    tests/test_spectral_gpu.py runs both lengths."""
    def lds_bytes(L):
        return (128 + 32 * (4 * ((L + 3) // 4) + 2)) * 4

    Lmax = lib.ffd_localization_lds_max_len()
    assert Lmax == 1144
    assert lds_bytes(Lmax) <= 144 * 1024 < lds_bytes(Lmax + 1)


def test_python_surface():
    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd._native import FFDError

    pkg.install_as_fdiff(force=True)
    from fdiff.utils.fourier import localization_metrics, smooth_frequency
    from fdiff.visualization.spectral_interpretation import process_dataset, spectral_profile

    with pytest.raises(RuntimeError):  # even max_len, like the reference's einsum
        smooth_frequency(torch.zeros(2, 24, 3), 2.0)
    x = torch.ones(2, 5, 3)
    if torch.cuda.is_available():  # CPU tensors are staged through the device and come back on the CPU
        assert all(t.device.type == "cpu" for t in localization_metrics(x))
        return
    for call in (lambda: localization_metrics(x), lambda: smooth_frequency(x, 2.0), lambda: spectral_profile(x),
                 lambda: process_dataset("d", x)):
        with pytest.raises(FFDError):
            call()
