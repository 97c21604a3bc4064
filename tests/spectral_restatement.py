"""Float64 restatement (numpy: ``np.fft``, explicit sums) of the reference's ``localization_metrics`` /
``smooth_frequency`` (fourier.py:134-216) and of the curves of ``process_dataset``
(spectral_interpretation.py:55-94).  Shared by tests/test_spectral_host.py, tests/test_spectral_gpu.py and
tools/gen_spectral_golden.py; no torch, no device."""
import math

import numpy as np

TOL_OP = 2e-6
EPS = 1e-15  # spectral_interpretation.py:31


def bound(ref_err, k):
    """The bound a device test asserts: 4 x the reference's own fp32 deviation from float64, at least k stages of TOL_OP."""
    return max(4.0 * float(ref_err), k * TOL_OP)


def energy_rows(x):
    """(B, L): per-position energy summed over channels."""
    x = np.asarray(x, dtype=np.float64)
    return (x * x).sum(axis=2)


def density_rows(x):
    """(B, L//2 + 1): spectral density of the ortho real FFT summed over channels (fourier.py:97-131)."""
    X = np.fft.rfft(np.asarray(x, dtype=np.float64), axis=1, norm="ortho")
    return (X.real ** 2 + X.imag ** 2).sum(axis=2)


def mirrored_density_rows(x):
    """(B, L): the density on the full frequency axis (fourier.py:154-159)."""
    L = np.asarray(x).shape[1]
    d = density_rows(x)
    tail = d[:, 1:] if L % 2 != 0 else d[:, 1:-1]
    return np.concatenate([d, tail[:, ::-1]], axis=1)


def cyclic_sq_row(L):
    """cyc(t, 0)^2 = min(t, L - t)^2; the column of centre s is this row rolled by s (no L x L matrix: L goes to 8192)."""
    t = np.arange(L, dtype=np.float64)
    return np.minimum(t, L - t) ** 2


def localization(x):
    """fourier.py:134-182 -> (time delocalization (B), frequency delocalization (B)); 0 / 0 = NaN for a zero sample."""
    L = np.asarray(x).shape[1]
    cyc0 = cyclic_sq_row(L)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for rows in (energy_rows(x), mirrored_density_rows(x)):
            p = rows / rows.sum(axis=1, keepdims=True)
            moments = np.stack([(p * np.roll(cyc0, s)[None, :]).sum(axis=1) for s in range(L)], axis=1)  # (B, L)
            nan = np.isnan(moments).any(axis=1)
            m = np.where(nan, np.nan, np.nanmin(np.where(np.isnan(moments), np.inf, moments), axis=1))
            out.append(m)
    return out[0], out[1]


def flat_delocalization(L):
    """Delocalization of a flat distribution over L positions: sum_t cyc(t, 0)^2 / L."""
    t = np.arange(L, dtype=np.float64)
    return float((np.minimum(t, L - t) ** 2).sum() / L)


def pack_dft(x):
    """fourier.py:8-52: (B, L, C) -> packed ortho spectrum (B, L, C)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[1]
    X = np.fft.rfft(x, axis=1, norm="ortho")
    im = X.imag[:, 1:]
    if L % 2 == 0:
        im = im[:, :-1]
    return np.concatenate([X.real, im], axis=1)


def unpack_idft(xp):
    """fourier.py:55-94."""
    xp = np.asarray(xp, dtype=np.float64)
    B, L, C = xp.shape
    n_real = math.ceil((L + 1) / 2)
    re, im = xp[:, :n_real], xp[:, n_real:]
    zero = np.zeros((B, 1, C))
    im = np.concatenate([zero, im], axis=1)
    if L % 2 == 0:
        im = np.concatenate([im, zero], axis=1)
    return np.fft.irfft(re + 1j * im, n=L, axis=1, norm="ortho")


def smoothing_kernel(L, sigma):
    """fourier.py:196-210 (odd L): the column-normalized Gaussian kernel (L, L)."""
    nyq = L / 2
    k = np.concatenate([np.arange(0, nyq, dtype=np.float64), np.arange(1, nyq, dtype=np.float64)])
    assert len(k) == L, "the reference's kernel has L rows only for odd L"
    g = np.exp(-(((k[:, None] - k[None, :]) / float(sigma)) ** 2) / 2)
    return g / g.sum(axis=0, keepdims=True)


def smooth_frequency(x, sigma):
    """fourier.py:185-216."""
    W = smoothing_kernel(np.asarray(x).shape[1], sigma)
    return unpack_idft(np.einsum("btc,ts->bsc", pack_dft(x), W))


def profile(x):
    """spectral_interpretation.py:55-94 -> (spec_mean, spec_se, energy_mean, energy_std); EPS in the means only,
    unbiased std over the batch (NaN for B = 1), the spectral one divided by sqrt(B)."""
    B = np.asarray(x).shape[0]
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for rows, scale in ((density_rows(x), 1.0 / math.sqrt(B)), (energy_rows(x), 1.0)):
            tot = rows.sum(axis=1, keepdims=True)
            mean = (rows / (EPS + tot)).sum(axis=0) / B
            p = rows / tot
            dev = p - p.sum(axis=0, keepdims=True) / B
            std = np.sqrt((dev * dev).sum(axis=0) / (B - 1)) if B > 1 else np.full(rows.shape[1], np.nan)
            out += [mean, std * scale]
    return tuple(out)


def records(name, x):
    """The four record lists of process_dataset (spectral_interpretation.py:71-141) from the float64 curves."""
    spec_mean, spec_se, energy_mean, energy_std = profile(x)
    loc_t, loc_f = localization(x)
    nf, L = len(spec_mean), len(energy_mean)
    spectral = [{"Dataset": name, "Normalized Frequency": k / (nf - 1), "Normalized Spectral Density": float(spec_mean[k]),
                 "SE": float(spec_se[k])} for k in range(nf)]
    temporal = [{"Dataset": name, "Normalized Time": k / (L - 1), "Normalized Energy": float(energy_mean[k]),
                 "SE": float(energy_std[k])} for k in range(L)]
    loc = [{"Dataset": name, "Delocalization": float(v), "Domain": "Time"} for v in loc_t]
    loc += [{"Dataset": name, "Delocalization": float(v), "Domain": "Frequency"} for v in loc_f]
    joint = [{"Dataset": name, "Delocalization Time": float(a), "Delocalization Frequency": float(b)}
             for a, b in zip(loc_t, loc_f)]
    return spectral, temporal, loc, joint


def rel_to_value(a, b):
    """Largest elementwise |a - b| / |b| over the entries with b != 0 (0 where both are 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = b != 0
    assert np.all(a[~nz] == 0), "an expected zero is not reproduced"
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


CURVES = ("spec_mean", "spec_se", "energy_mean", "energy_std")
CURVE_STAGES = {"spec_mean": 3, "spec_se": 3, "energy_mean": 1, "energy_std": 1}


def curve_err(name, got, f64, B):
    """Error of one curve of `profile` against its float64 value f64 = dict(name -> curve).  The means: elementwise,
    relative to the value.  The spreads: elementwise, relative to the value or, where that is larger, to the mean at that
    position (divided by sqrt(B) for the spectral SE): a spread is a difference of numbers of the mean's size, so its
    rounding error scales with the mean and not with itself -- where two samples happen to agree at a position the
    spread is arbitrarily small and no fp32 evaluation, the reference's included, keeps it to a relative 1e-5."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(f64[name], dtype=np.float64)
    if name == "spec_se":
        scale = np.asarray(f64["spec_mean"], dtype=np.float64) / math.sqrt(B)
    elif name == "energy_std":
        scale = np.asarray(f64["energy_mean"], dtype=np.float64)
    else:
        return rel_to_value(got, want)
    den = np.maximum(np.abs(want), scale)
    nz = den != 0
    assert np.all(got[~nz] == 0), "an expected zero is not reproduced"
    return float(np.max(np.abs(got[nz] - want[nz]) / den[nz])) if nz.any() else 0.0


# ---- the g17 cases (tools/gen_spectral_golden.py writes them, the tests read them) ----
LOC_SHAPES = [(187, 1), (251, 4), (365, 13), (24, 40), (512, 8), (2, 1), (33, 3)]   # (L, C)
TONE_SHAPES = [(187, 1), (512, 8)]
LOC_B = 5
LOC_CASES = [(L, C, kind) for (L, C) in LOC_SHAPES for kind in ("white", "bump")] + [(L, C, "tone") for (L, C) in TONE_SHAPES]
PROFILE_B = (2, 5)
# the tone batches are localization inputs only: the density of their noise-floor bins sits 1e-6 below the tone, where the
# fp32 FFT of the reference itself is 3e-4 off in relative terms
PROFILE_CASES = [case for case in LOC_CASES if case[2] != "tone"]
SMOOTH_L = (1, 3, 25, 187, 251)
SMOOTH_SIGMA = (0.5, 2.0, 50.0)
SMOOTH_B, SMOOTH_C = 3, 2


def loc_key(L, C, kind):
    return f"loc_L{L}_C{C}_{kind}"


def smooth_key(L, sigma):
    return f"smooth_L{L}_s{sigma:g}"
