"""Generate tests/golden/g17_spectral.npz (+ META_g17.txt) by running the UNMODIFIED reference's localization metrics,
frequency smoothing and per-dataset spectral statistics on the CPU.

TEST INFRASTRUCTURE ONLY.  Run where the reference sources are mounted:   python tools/gen_spectral_golden.py
The reference is imported from where it lies (oracle/_ref_import.py); ``fdiff.utils.fourier.localization_metrics`` /
``smooth_frequency`` and ``fdiff.visualization.spectral_interpretation.process_dataset`` are called as they are.  The
last file is loaded without its package's ``__init__`` (which pulls in hydra and the plotting stack) and with inert
``seaborn`` / ``scienceplots`` modules: it only plots with them.  Only arrays are stored.

Cases (tests/spectral_restatement.py lists them): per shape (L, C) a white-noise batch and one multiplied by a Gaussian
bump in time (centre L/2, width L/16), at two shapes a unit tone + 1e-3 noise; B = 5.
  loc_L{L}_C{C}_{kind}_x               the input (B, L, C) fp32
  ..._ref_time, _ref_freq              the reference's fp32 delocalizations
  ..._f64_time, _f64_freq              the float64 restatement
  ..._tol_time, _tol_freq              the bounds the device tests assert
  ..._B{2|5}_ref_{spec_mean,spec_se,energy_mean,energy_std}, _f64_*, _tol_*     the curves of process_dataset on x[:B]
  smooth_L{L}_x; smooth_L{L}_s{sigma}_ref / _f64 / _tol                        smooth_frequency (B = 3, C = 2)

Bounds: ref_err = the reference's own fp32 deviation from the float64 restatement (delocalizations and mean curves: the
largest elementwise error relative to the value; spread curves: relative to the value or to the mean at that position,
whichever is larger, see spectral_restatement.curve_err; smoothing: relative to the max-norm, conftest.rel_err);
tol = max(4 ref_err, k TOL_OP), TOL_OP = 2e-6, k = 1 for the time delocalization and the energy curves (one fp32
stage), k = 3 for the frequency delocalization, the density curves and the smoothing (dft, normalisation or
contraction, product or idft).  The factor 4 covers the different summation orders (blocked / pairwise on the CPU, a
sequential chain over t on the matrix cores).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spectral_restatement as R  # noqa: E402
from oracle._ref_import import REFERENCE_SRC, import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_spectral.npz")
META = os.path.join(ROOT, "tests", "golden", "META_g17.txt")
BAR = 2e-5


def import_process_dataset():
    for name in ("seaborn", "scienceplots"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    plt.style.use = lambda *a, **k: None  # the "science" style comes from scienceplots
    pkg = types.ModuleType("fdiff.visualization")
    pkg.__path__ = [os.path.join(REFERENCE_SRC, "fdiff", "visualization")]
    sys.modules["fdiff.visualization"] = pkg
    from fdiff.visualization.spectral_interpretation import process_dataset

    return process_dataset


class _Datamodule:
    def __init__(self, X):
        self.X_train = X

    def prepare_data(self):
        pass

    def setup(self):
        pass


def make_input(L, C, kind, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((R.LOC_B, L, C))
    t = np.arange(L, dtype=np.float64)
    if kind == "bump":
        x = x * np.exp(-((t - L / 2) ** 2) / (2 * (L / 16) ** 2))[None, :, None]
    elif kind == "tone":
        f = np.array([3, 7, 11, 20, 40])[:, None, None]
        x = np.sin(2 * np.pi * f * t[None, :, None] / L + rng.uniform(0, 2 * np.pi, (R.LOC_B, 1, C))) + 1e-3 * x
    return x.astype(np.float32)


def main() -> None:
    import_reference()
    from fdiff.utils.fourier import localization_metrics, smooth_frequency  # the reference's

    process_dataset = import_process_dataset()
    out, lines = {}, []

    def record(key, ref, f64, k, how):
        ref = np.asarray(ref)
        err = how(ref, f64)
        tol = R.bound(err, k)
        out[key.format("ref")], out[key.format("f64")], out[key.format("tol")] = ref, np.asarray(f64), np.float64(tol)
        lines.append(f"{key.format('*'):44s} ref_err {err:.2e}  tol {tol:.2e}")
        print(lines[-1])
        assert tol <= BAR, (key, tol, "change the case's inputs, not the bar")

    def max_norm(a, b):
        return float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b)))

    for i, (L, C, kind) in enumerate(R.LOC_CASES):
        key = R.loc_key(L, C, kind)
        x = make_input(L, C, kind, 1700 + i)
        out[key + "_x"] = x
        X = torch.from_numpy(x)
        lt, lf = localization_metrics(X)
        ft, ff = R.localization(x)
        record(key + "_{}_time", lt.numpy(), ft, 1, R.rel_to_value)
        record(key + "_{}_freq", lf.numpy(), ff, 3, R.rel_to_value)
        if (L, C, kind) not in R.PROFILE_CASES:
            continue
        for B in R.PROFILE_B:
            spec, temp, loc, joint = (df.to_dict("records") for df in process_dataset("g17", _Datamodule(X[:B])))
            curves = R.profile(x[:B])
            f64 = dict(zip(R.CURVES, curves))
            cols = [(spec, "Normalized Spectral Density"), (spec, "SE"), (temp, "Normalized Energy"), (temp, "SE")]
            for name, (recs, col) in zip(R.CURVES, cols):
                ref = np.array([r[col] for r in recs], dtype=np.float32)
                record(f"{key}_B{B}_{{}}_{name}", ref, f64[name], R.CURVE_STAGES[name],
                       lambda a, b, name=name, B=B: R.curve_err(name, a, f64, B))
            # the localization tables repeat localization_metrics on the same rows
            assert [r["Delocalization Time"] for r in joint] == [float(v) for v in lt[:B]]
    for j, L in enumerate(R.SMOOTH_L):
        x = np.random.Generator(np.random.PCG64(1800 + j)).standard_normal((R.SMOOTH_B, L, R.SMOOTH_C)).astype(np.float32)
        for sigma in R.SMOOTH_SIGMA:
            key = R.smooth_key(L, sigma)
            out[f"smooth_L{L}_x"] = x
            f64 = R.smooth_frequency(x, sigma)
            if L == 1:
                # torch.arange(1, 0.5) raises in the reference (fourier.py:204); numpy's is empty, k = [0], W = [[1]]:
                # the identity, which is what the device computes.  No reference output exists: ref = the float64 value.
                try:
                    smooth_frequency(torch.from_numpy(x), sigma)
                    raise AssertionError("the reference no longer raises at L = 1: record its output")
                except RuntimeError:
                    record(key + "_{}", f64.astype(np.float32), f64, 3, max_norm)
                continue
            ref = smooth_frequency(torch.from_numpy(x), sigma).numpy()
            record(key + "_{}", ref, f64, 3, max_norm)
    np.savez_compressed(OUT, **out)
    with open(META, "w") as f:
        f.write("g17_spectral.npz -- tools/gen_spectral_golden.py, from the unmodified reference "
                "(localization_metrics, smooth_frequency, process_dataset) on the CPU, fp32.\n"
                f"torch {torch.__version__}, numpy {np.__version__}.  tol = max(4 ref_err, k * 2e-6); see the generator.\n\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
