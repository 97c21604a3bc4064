"""GPU tests of the localization metrics, the frequency smoothing and the spectral profiles (ffd_spectral.hip): every
case of tests/golden/g17_spectral.npz within its recorded bound, through the C ABI and through the Python functions,
and the float64 restatement (tests/spectral_restatement.py) on fresh inputs at the MFMA tile edges.

Fresh inputs have no recorded reference error; their bound is the floor of the recorded ones, k * TOL_OP (k = 1: time
delocalization, energy curves; k = 3: frequency delocalization, density curves, smoothing)."""
import math

import numpy as np
import pytest
import torch

import spectral_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not torch.cuda.is_available():
        pytest.fail("no MI355X visible to torch: the gpu-marked tests need one")
    return _native.lib()


def _stream():
    from fastfourierdiffusion_amd import _native

    return _native.current_stream_ptr(torch.device("cuda"))


def _scratch(nbytes):
    return torch.empty((int(nbytes) + 7) // 8 + 1, dtype=torch.float64, device="cuda")


def c_localization(lib, x):
    """x: numpy (B, L, C) -> (time, freq) numpy fp32 through the C ABI."""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, L, C = xd.shape
    out = torch.full((2, B), -1.0, device="cuda")
    work = _scratch(lib.ffd_localization_work_bytes(B, L, C))
    rc = lib.ffd_localization(xd.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), work.data_ptr(), work.numel() * 8, B, L,
                              C, _stream())
    assert rc == 0, rc
    o = out.cpu().numpy()
    return o[0], o[1]


def c_smooth(lib, x, sigma):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, L, C = xd.shape
    out = torch.full_like(xd, -1.0)
    work = _scratch(lib.ffd_smooth_frequency_work_bytes(B, L, C))
    rc = lib.ffd_smooth_frequency(xd.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel() * 8, B, L, C, float(sigma),
                                  _stream())
    assert rc == 0, rc
    return out.cpu().numpy()


def c_profile(lib, x, extra_bytes=0):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, L, C = xd.shape
    nf = L // 2 + 1
    spec = torch.full((2, nf), -1.0, device="cuda")
    en = torch.full((2, L), -1.0, device="cuda")
    work = _scratch(lib.ffd_spectral_profile_work_bytes(B, L, C) + extra_bytes)
    rc = lib.ffd_spectral_profile(xd.data_ptr(), spec[0].data_ptr(), spec[1].data_ptr(), en[0].data_ptr(), en[1].data_ptr(),
                                  work.data_ptr(), work.numel() * 8, B, L, C, _stream())
    assert rc == 0, rc
    s, e = spec.cpu().numpy(), en.cpu().numpy()
    return dict(zip(R.CURVES, (s[0], s[1], e[0], e[1])))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise(seed, B, L, C):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((B, L, C)).astype(np.float32)


def max_norm_err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(np.max(np.abs(b)), 1e-30))


# ---- the golden cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LOC_CASES, ids=lambda c: R.loc_key(*c))
def test_golden_localization_and_profiles(lib, golden, case):
    from fastfourierdiffusion_amd.utils.fourier import localization_metrics
    from fastfourierdiffusion_amd.visualization.spectral_interpretation import spectral_profile

    g = golden["g17_spectral"]
    key = R.loc_key(*case)
    x = g[key + "_x"]
    got = c_localization(lib, x)
    py = [t.cpu().numpy() for t in localization_metrics(torch.from_numpy(x).cuda())]
    for name, o, p in zip(("time", "freq"), got, py):
        tol = float(g[f"{key}_tol_{name}"])
        err = R.rel_to_value(o, g[f"{key}_f64_{name}"])
        print(f"{key} {name}: device off float64 by {err:.2e} (tol {tol:.2e}), "
              f"off the reference by {R.rel_to_value(o, g[f'{key}_ref_{name}'].astype(np.float64)):.2e}")
        assert err <= tol
        assert np.array_equal(bits(o), bits(p))  # the Python function is the same call
    if case not in R.PROFILE_CASES:
        return
    for B in R.PROFILE_B:
        f64 = {name: g[f"{key}_B{B}_f64_{name}"] for name in R.CURVES}
        got = c_profile(lib, x[:B])
        py = [t.cpu().numpy() for t in spectral_profile(torch.from_numpy(x[:B]))]  # a CPU tensor is staged and comes back
        for name, p in zip(R.CURVES, py):
            tol = float(g[f"{key}_B{B}_tol_{name}"])
            err = R.curve_err(name, got[name], f64, B)
            print(f"{key} B={B} {name}: device off float64 by {err:.2e} (tol {tol:.2e})")
            assert err <= tol
            assert np.array_equal(bits(got[name]), bits(p))


@pytest.mark.parametrize("L", R.SMOOTH_L)
def test_golden_smoothing(lib, golden, L):
    from fastfourierdiffusion_amd.utils.fourier import smooth_frequency

    g = golden["g17_spectral"]
    x = g[f"smooth_L{L}_x"]
    for sigma in R.SMOOTH_SIGMA:
        key = R.smooth_key(L, sigma)
        got = c_smooth(lib, x, sigma)
        tol = float(g[key + "_tol"])
        err = max_norm_err(got, g[key + "_f64"])
        print(f"{key}: device off float64 by {err:.2e} (tol {tol:.2e}), off the reference by "
              f"{max_norm_err(got, g[key + '_ref'].astype(np.float64)):.2e}")
        assert err <= tol
        py = smooth_frequency(torch.from_numpy(x), sigma)
        assert py.device.type == "cpu" and np.array_equal(bits(got), bits(py.numpy()))
        if L == 1:
            assert np.array_equal(bits(got), bits(x))  # the identity, exactly


# ---- fresh inputs at the tile edges -------------------------------------------------------------------------------
FRESH_L = (1, 2, 31, 32, 33, 63, 65, 187, 512)
FRESH_C = (1, 3, 40)
FRESH_B = (1, 3, 33, 70)  # ragged 32-row tiles of the product kernel


@pytest.mark.parametrize("C", FRESH_C)
@pytest.mark.parametrize("L", FRESH_L)
def test_localization_against_float64_on_fresh_inputs(lib, L, C):
    x = noise(9000 + 100 * L + C, max(FRESH_B), L, C)
    x[1::2] *= np.exp(-((np.arange(L) - 0.3 * L) ** 2) / (2 * (L / 10 + 0.5) ** 2))[None, :, None].astype(np.float32)
    f64 = R.localization(x)
    full = c_localization(lib, x)
    for B in FRESH_B:
        got = full if B == max(FRESH_B) else c_localization(lib, x[:B])
        for name, k, o, w, fo in zip(("time", "freq"), (1, 3), got, f64, full):
            err = R.rel_to_value(o, w[:B])
            print(f"L={L} C={C} B={B} {name}: {err:.2e}")
            assert err <= k * R.TOL_OP
            assert np.array_equal(bits(o), bits(fo[:B]))  # a sample does not depend on the rest of the batch


@pytest.mark.parametrize("past", (0, 1), ids=("longest_row_block_in_lds", "first_length_read_from_l2"))
def test_localization_on_both_sides_of_the_lds_limit(lib, past):
    """The library names the longest row whose 32-row block the product kernel keeps in LDS (1144: the largest LDS image,
    147 200 B); one position more takes the kernel that reads the rows from L2."""
    L = lib.ffd_localization_lds_max_len() + past
    assert 512 < L < 8192
    x = noise(9100 + L, 35, L, 2)  # two row blocks, the second ragged
    x[1::2] *= np.exp(-((np.arange(L) - 0.7 * L) ** 2) / (2 * 40.0 ** 2))[None, :, None].astype(np.float32)
    for name, k, o, w in zip(("time", "freq"), (1, 3), c_localization(lib, x), R.localization(x)):
        err = R.rel_to_value(o, w)
        print(f"L={L} {name}: {err:.2e}")
        assert err <= k * R.TOL_OP


@pytest.mark.parametrize("L", (33, 187, 512))
def test_impulse_is_exact_and_shift_invariant(lib, L):
    t0s = (0, L - 1, L // 2)  # the argmin at the first, the last and an interior centre
    x = np.zeros((len(t0s), L, 2), dtype=np.float32)
    for b, t0 in enumerate(t0s):
        x[b, t0, b % 2] = 1.5
    t, f = c_localization(lib, x)
    assert np.array_equal(t, np.zeros(len(t0s), dtype=np.float32))
    flat = R.flat_delocalization(L)
    print(f"L={L}: frequency delocalization of the impulses {f}, flat spectrum {flat}")
    assert np.max(np.abs(f.astype(np.float64) - flat)) / flat <= 3 * R.TOL_OP
    ts, fs = c_localization(lib, np.roll(x, 7, axis=1))
    assert np.array_equal(bits(ts), bits(t))  # exactly 0 wherever the impulse sits
    # The time value is 0 bit for bit wherever the impulse sits.  The frequency value goes through the fp32 dft, where
    # the shifted impulse's spectrum has another phase and cos^2 + sin^2 another rounding: through the power-of-two
    # transform (L = 512) the value still comes out the same bit for bit and is held to that (every kernel on the way
    # is deterministic); through the mixed-radix one (L = 33, 187) it moves in the last place and is held to the bound.
    same = np.array_equal(bits(fs), bits(f))
    print(f"L={L}: shifted impulse, frequency values bitwise equal: {same}")
    if L == 512:
        assert same
    assert R.rel_to_value(fs, f.astype(np.float64)) <= 3 * R.TOL_OP


def test_circular_shift_of_noise_stays_within_the_bound(lib):
    x = noise(9200, 6, 187, 3)
    t, f = c_localization(lib, x)
    for shift in (1, 93, 186):
        ts, fs = c_localization(lib, np.roll(x, shift, axis=1))
        assert R.rel_to_value(ts, t.astype(np.float64)) <= 1 * R.TOL_OP
        assert R.rel_to_value(fs, f.astype(np.float64)) <= 3 * R.TOL_OP


def test_zero_sample_is_nan_and_disturbs_nobody(lib):
    x = noise(9300, 7, 65, 3)
    ref = c_localization(lib, np.delete(x, 3, axis=0))
    x[3] = 0.0
    got = c_localization(lib, x)
    for o, r in zip(got, ref):
        assert np.isnan(o[3])
        assert np.array_equal(bits(np.delete(o, 3)), bits(r))


def test_batch_of_70_equals_its_samples_alone_and_reruns(lib):
    x = noise(9400, 70, 187, 1)
    full = c_localization(lib, x)
    again = c_localization(lib, x)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(full, again))
    alone = [c_localization(lib, x[b:b + 1]) for b in range(70)]
    for d in (0, 1):
        assert np.array_equal(bits(full[d]), bits(np.concatenate([a[d] for a in alone])))


# ---- smoothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,C,B", [(25, 3, 4), (187, 1, 33), (65, 40, 3), (3, 1, 1)])
def test_smoothing_against_float64(lib, L, C, B):
    """sigma = 50: near-constant columns, every output position carries (almost) the same mix of the spectrum.
    sigma = 0.5 is the narrowest kernel, but not the identity: the real and the imaginary part of a harmonic share
    their k (fourier.py:201-206) and so mix with weight 1 at any sigma."""
    x = noise(9500 + L, B, L, C)
    for sigma in (50.0, 0.5):
        got = c_smooth(lib, x, sigma)
        err = max_norm_err(got, R.smooth_frequency(x, sigma))
        print(f"L={L} C={C} B={B} sigma={sigma}: {err:.2e}")
        assert err <= 3 * R.TOL_OP
        assert np.array_equal(bits(got), bits(c_smooth(lib, x, sigma)))
    if L == 25:
        spec = R.pack_dft(c_smooth(lib, x, 50.0))
        assert np.max(np.ptp(spec, axis=1)) <= 0.05 * np.max(np.abs(spec))


def test_smoothing_length_one_and_even_lengths(lib):
    from fastfourierdiffusion_amd.utils.fourier import smooth_frequency

    x = noise(9600, 5, 1, 3)
    assert np.array_equal(bits(c_smooth(lib, x, 2.0)), bits(x))
    with pytest.raises(RuntimeError):
        smooth_frequency(torch.zeros(2, 32, 3, device="cuda"), 2.0)
    xd = torch.zeros(2, 32, 3, device="cuda")
    assert lib.ffd_smooth_frequency(xd.data_ptr(), torch.empty_like(xd).data_ptr(), _scratch(1 << 16).data_ptr(), 1 << 16,
                                    2, 32, 3, 2.0, _stream()) == -1


# ---- profiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (2, 5, 1025))  # 1025 crosses the 1024-sample slab
def test_profile_against_float64(lib, B):
    L, C = 33, 3
    x = noise(9700 + B, B, L, C)
    x *= (1.0 + np.arange(B) % 7)[:, None, None].astype(np.float32)  # the normalisation removes the scale
    f64 = dict(zip(R.CURVES, R.profile(x)))
    got = c_profile(lib, x)
    for name in R.CURVES:
        err = R.curve_err(name, got[name], f64, B)
        print(f"B={B} {name}: {err:.2e}")
        assert err <= R.CURVE_STAGES[name] * R.TOL_OP
    roomy = c_profile(lib, x, extra_bytes=1 << 20)  # the work size offered changes nothing
    assert all(np.array_equal(bits(got[n]), bits(roomy[n])) for n in R.CURVES)


def test_profile_of_one_sample_has_no_spread(lib):
    x = noise(9800, 1, 24, 2)
    got = c_profile(lib, x)
    f64 = dict(zip(R.CURVES, R.profile(x)))
    assert np.isnan(got["spec_se"]).all() and np.isnan(got["energy_std"]).all()
    assert R.rel_to_value(got["spec_mean"], f64["spec_mean"]) <= 3 * R.TOL_OP
    assert R.rel_to_value(got["energy_mean"], f64["energy_mean"]) <= 1 * R.TOL_OP


def test_process_dataset_records(lib):
    import fastfourierdiffusion_amd as pkg

    pkg.install_as_fdiff(force=True)
    from fdiff.visualization.spectral_interpretation import process_dataset

    class Datamodule:
        calls = []

        def prepare_data(self):
            self.calls.append("prepare_data")

        def setup(self):
            self.calls.append("setup")

    B, L, C = 6, 24, 3
    x = noise(9900, B, L, C)
    dm = Datamodule()
    dm.X_train = torch.from_numpy(x)
    tables = process_dataset("ECG", dm)
    assert dm.calls == ["prepare_data", "setup"]
    want = R.records("ECG", x)
    stages = {"Normalized Spectral Density": 3, "Normalized Energy": 1, "Delocalization Time": 1,
              "Delocalization Frequency": 3}
    f64 = dict(zip(R.CURVES, R.profile(x)))
    for got_t, want_t in zip(tables, want):
        assert len(got_t) == len(want_t)
        for gr, wr in zip(got_t, want_t):
            assert list(gr) == list(wr)  # the reference's column names, in its order
            for col, w in wr.items():
                v = gr[col]
                if isinstance(w, str) or col in ("Normalized Frequency", "Normalized Time"):
                    assert v == w, col
                elif col in stages:
                    assert abs(v - w) <= stages[col] * R.TOL_OP * abs(w), col
                elif col == "Delocalization":
                    assert abs(v - w) <= (1 if gr["Domain"] == "Time" else 3) * R.TOL_OP * abs(w)
    for name, table, col in (("spec_se", tables[0], "SE"), ("energy_std", tables[1], "SE")):
        assert R.curve_err(name, [r[col] for r in table], f64, B) <= R.CURVE_STAGES[name] * R.TOL_OP
    assert len(tables[0]) == L // 2 + 1 and len(tables[1]) == L and len(tables[2]) == 2 * B and len(tables[3]) == B
    assert tables[0][-1]["Normalized Frequency"] == 1.0 and tables[1][-1]["Normalized Time"] == 1.0
    # a bare tensor is accepted in place of the datamodule
    assert process_dataset("ECG", torch.from_numpy(x).cuda())[3] == tables[3]
