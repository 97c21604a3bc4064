"""Dynamic-time-warping metrics on one MI355X: what they cost and what they say.  Writes profiles/dtw_metrics.json.

    python3 tools/dtw_bench.py [--out profiles/dtw_metrics.json] [--only timing|quality]

Timing.  The cross search ``dtw_neighbours(samples, originals, window)`` at k = 1, at window 0.1 (w = 19 at L = 187, the
W = 32 instance) and at window 0, at the ECG evaluation size (10 000 samples against 87 554 series of 187 points) and at
1024 x 4096 x 187, between device events after a warm-up.  Rates: DP cells of the real band per second, and cells of the
padded band (what the instance computes) against the instruction floor.

The floor.  ``VALU_PER_ROW`` is the number of vector-ALU instructions in the DP-row loop of k_dtw_block<W, C = 1, staged>,
counted in the compiled gfx950 ISA (make lint leaves it in csrc/.isa/ffd_dtw.s: the one basic block holding the
v_min3_i32s; the W = 0 loop is unrolled over 8 rows).  Per cell that is v_sub, v_mul, v_min3_i32, v_add, v_cndmask, and a
few address adds per row.  A wave64 vector instruction holds its SIMD for 4 cycles when the wave issues alone and 2 when
another wave fills the other half (the chip's SIMDs are 32 lanes wide), so
    floor seconds = pairs / 64 lanes * L rows * VALU_PER_ROW * CYCLES / (256 CUs * 4 SIMDs * 2.4e9 Hz)
with CYCLES = 4 (``floor_4``) and 2 (``floor_2``); the LDS reads (one dword per cell), the staging and the merge are not
in it.  The comparison line at the small size is the float64 numpy restatement (tests/dtw_restatement.py) on 16 threads,
run on 128 of the 1024 query rows and scaled by 8.

A whole ``DTWMetrics`` call at 10 000 x 10 000 with the originals' self-search kept (every call after the first) and not
kept (a fresh object per call); the originals' self-search at 87 554 rows once, if the measured rate puts it under a
minute, else what it would take.

Quality.  The sample sets of tools/manifold_bench.py (4096-series four-family target, 1024 samples each; the transformer is
the one profiles/train_quality.json and DESIGN section 6 describe): the six ``DTWMetrics`` numbers at window 0.1."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = {"ecg_eval": (10000, 87554, 187), "1024x4096": (1024, 4096, 187)}
WINDOWS = (0.1, 0)
VALU_PER_ROW = {0: 43 / 8, 4: 51, 8: 90, 16: 174, 32: 342, 64: 879}
SIMDS, CLOCK = 256 * 4, 2.4e9
WHOLE = 10000


def timed(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return {"ms_mean": float(np.mean(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def padded(w):
    return min(p for p in VALU_PER_ROW if p >= w)


def with_rate(entry, nq, nr, L, w):
    pairs, wp = float(nq) * nr, padded(w)
    real = pairs * (L * (2 * w + 1) - w * (w + 1))
    seconds = entry["ms_mean"] * 1e-3
    floor_4 = pairs / 64 * L * VALU_PER_ROW[wp] * 4 / (SIMDS * CLOCK)
    entry.update(window=w, instance=wp, band_cells_per_s=real / seconds, padded_cells_per_s=pairs * L * (2 * wp + 1) / seconds,
                 valu_per_padded_cell=VALU_PER_ROW[wp] / (2 * wp + 1), floor_4_ms=1e3 * floor_4, floor_2_ms=5e2 * floor_4,
                 time_over_floor_4=seconds / floor_4, time_over_floor_2=2 * seconds / floor_4)
    return entry


def series(n, L, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, L, 1, device="cuda", generator=g)


def host_search(X, Y, w, threads=16, rows=8):
    import dtw_restatement as DR

    def part(i0):
        return DR.all_pairs(X[i0:i0 + rows], Y, w, rows_at_once=rows).min(axis=1)

    with ThreadPoolExecutor(threads) as pool:
        return np.concatenate(list(pool.map(part, range(0, X.shape[0], rows))))


def timing(reps):
    from fastfourierdiffusion_amd.sampling.metrics import DTWMetrics
    from fastfourierdiffusion_amd.utils import dtw

    out = {"what": "ms per call between device events: mean / min / max of REPS repetitions after a warm-up; band_cells_per_s "
                   "counts the cells with |i - j| <= w, padded_cells_per_s those of the instance's band; floor_4 / floor_2: the "
                   "DP-row loop's vector instructions alone at 4 / 2 cycles per wave64 instruction on 1024 SIMDs at 2.4 GHz",
           "valu_per_row": VALU_PER_ROW, "reps": reps, "sizes": {}}
    rate = None
    for name, (m, n, L) in SIZES.items():
        X, Y = series(m, L, m), series(n, L, n)
        entry = {"samples": m, "originals": n, "L": L, "C": 1}
        for window in WINDOWS:
            w = dtw.resolve_window(window, L)
            entry[f"cross_search_window_{window:g}"] = with_rate(timed(lambda: dtw.dtw_neighbours(X, Y, w), 1, reps), m, n, L, w)
            print(name, window, json.dumps(entry[f"cross_search_window_{window:g}"]), flush=True)
        if name == "ecg_eval":
            rate = entry["cross_search_window_0.1"]["padded_cells_per_s"]
        else:
            w = dtw.resolve_window(0.1, L)
            Xh, Yh = X[:128].cpu().numpy(), Y.cpu().numpy()
            t0 = time.perf_counter()
            host = host_search(Xh, Yh, w)
            seconds = time.perf_counter() - t0
            dev = dtw.dtw_neighbours(X[:128].contiguous(), Y, w)[0].reshape(-1).cpu().numpy()
            entry["host_float64_numpy"] = {"threads": 16, "query_rows_run": 128, "ms_run": 1e3 * seconds,
                                           "ms_scaled_to_1024_rows": 8e3 * seconds,
                                           "largest_difference_to_device_over_scale": float(np.abs(dev - host).max() / host.max())}
            print(name, json.dumps(entry["host_float64_numpy"]), flush=True)
        out["sizes"][name] = entry
        del X, Y
    # a whole metric call
    X, Y = series(WHOLE, 187, 5), series(WHOLE, 187, 6)
    metric = DTWMetrics(Y, window=0.1)
    values = metric(X)
    out["dtw_metrics_10000x10000"] = {"values_on_two_gaussian_sets": values, "yy_kept": timed(lambda: metric(X), 1, reps),
                                      "yy_not_kept": timed(lambda: DTWMetrics(Y, window=0.1)(X), 1, reps)}
    print("whole call", json.dumps(out["dtw_metrics_10000x10000"]), flush=True)
    del X, Y, metric
    # the originals' self-search at the ECG size
    n, L, w = 87554, 187, 19
    estimate = float(n) * n * L * (2 * padded(w) + 1) / rate
    entry = {"rows": n, "window": w, "estimate_from_the_cross_search_rate_s": estimate}
    if estimate < 60.0:
        Y = series(n, L, 7)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dtw.self_search(Y, w)
        e1.record()
        e1.synchronize()
        entry["measured_once_s"] = 1e-3 * e0.elapsed_time(e1)
    out["originals_self_search_ecg"] = entry
    print("self-search", json.dumps(entry), flush=True)
    return out


def quality():
    import solver_quality as SQ
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import DTWMetrics, ManifoldMetrics
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft
    from manifold_bench import BATCH, BUDGET, EPOCHS_TF, LR_MAX, N_SAMPLES, SEED

    X = SQ.dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    metric = DTWMetrics(X.contiguous(), window=0.1)
    manifold = ManifoldMetrics(X.reshape(X.shape[0], -1).contiguous(), k=5)
    baseline = metric.baseline_metrics

    def score_samples(samples):
        rows = unstandardize_idft(samples.cuda(), mean, std).reshape(samples.shape[0], SQ.L, SQ.CH).contiguous()
        found = metric(rows)
        found["precision"] = manifold(rows.reshape(rows.shape[0], -1))["precision"]
        return {k: float(v) for k, v in found.items()}

    def draw(model):
        s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=SEED,
                             **SQ.SOLVERS["euler_maruyama"][0])
        return s.sample(num_samples=N_SAMPLES, num_diffusion_steps=BUDGET)

    out = {"what": "DTWMetrics (window 0.1 = 19 samples) in the time domain of 1024 samples against the 4096-series four-family "
                   "target, and the precision (k = 5) of the same samples; Euler-Maruyama, 200 score evaluations, VP, Philox "
                   "seed 1", "n_data": SQ.N_DATA, "n_samples": N_SAMPLES, "window": metric.window,
           "baseline_two_halves_of_the_target": baseline, "sets": {}}
    g = torch.Generator().manual_seed(SEED)
    pick = torch.randint(0, SQ.N_DATA, (N_SAMPLES,), generator=g)
    out["sets"]["exact_draws_bandwidth_0.1"] = score_samples(Z.cpu()[pick] + SQ.BANDWIDTH * torch.randn(N_SAMPLES, SQ.L, SQ.CH,
                                                                                                   generator=g))
    print("exact", out["sets"]["exact_draws_bandwidth_0.1"], flush=True)
    sch = SQ.scheduler("vp")
    model = MixtureScoreModule.from_data(Z.cpu(), sch, bandwidth=0.1).cuda().eval()
    out["sets"]["mixture_from_data_bandwidth_0.1"] = score_samples(draw(model))
    print("mixture", out["sets"]["mixture_from_data_bandwidth_0.1"], flush=True)
    steps = EPOCHS_TF * (SQ.N_DATA // BATCH)
    torch.manual_seed(0)
    model = ScoreModule(n_channels=SQ.CH, max_len=SQ.L, noise_scheduler=sch, d_model=60, num_layers=3, n_head=12,
                        num_training_steps=steps, lr_max=LR_MAX).cuda()
    Trainer(model, seed=0).fit(Z, batch_size=BATCH, max_epochs=EPOCHS_TF)
    model.eval()
    out["sets"]["transformer_100_epochs"] = score_samples(draw(model))
    print("transformer", out["sets"]["transformer_100_epochs"], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_metrics.json"))
    ap.add_argument("--only", choices=("timing", "quality"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dtw_bench.py measures on an MI355X; no device found")
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    if args.only != "quality":
        result["timing"] = timing(args.reps)
    if args.only != "timing":
        result["quality"] = quality()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
