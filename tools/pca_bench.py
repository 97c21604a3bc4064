"""The Frechet distance and the float64 eigensolver on one MI355X: what they cost and what they say.  Writes
profiles/frechet.json.

    python3 tools/pca_bench.py [--out profiles/frechet.json] [--only timing|quality]

Timing.  At the ECG evaluation size (10 000 samples against 87 554 series of 187 points): ``utils.pca.covariance`` of the
originals and of the samples, one ``eigh`` at D = 187 (with vectors, and values only), and a whole ``FrechetDistance`` call
with the originals' moments kept (every call after the first) and not kept (a fresh object per call), between device
events: a warm-up, then REPS repetitions of ITERS calls (mean / min / max of the repetitions).  ``eigh`` reads 8 bytes back
per sweep, so its time holds those host round trips.  The same whole call at 1024 x 4096 x 187 next to float64 numpy on the
host's threads (``np.cov``, ``np.linalg.eigh``), with the largest difference between the two.

Quality.  The sample sets of tools/sinkhorn_bench.py --only quality (4096-series four-family target, 1024 samples each): FD
and its two terms next to the halves-of-the-data baseline, the variance ratio along the data's main axes, and which term
carries a set's excess over the baseline."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmd_bench import clustered, timed  # noqa: E402

SIZES = {"ecg_eval": (10000, 87554, 187), "1024x4096": (1024, 4096, 187)}
COMPONENTS = 10


def host_frechet(X, Y):
    """float64 numpy: np.cov, the root and the inner spectrum through np.linalg.eigh."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    cx, cy = np.cov(X, rowvar=False), np.cov(Y, rowvar=False)
    w, v = np.linalg.eigh(cy)
    root = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = root @ cx @ root
    lam = np.linalg.eigvalsh((m + m.T) / 2.0)
    return float((mx - my) @ (mx - my) + np.trace(cx) + np.trace(cy) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def _carrier(excess_mean, excess_cov):
    """Which term holds the larger part of a set's excess over the baseline; "none" for a set at or under it."""
    if excess_mean + excess_cov <= 0.0:
        return "none"
    return "mean" if excess_mean > excess_cov else "covariance"


def timing(iters, reps):
    from fastfourierdiffusion_amd.sampling.metrics import FrechetDistance
    from fastfourierdiffusion_amd.utils import pca

    out = {"what": "ms per call between device events: mean / min / max of REPS repetitions of ITERS calls after a warm-up; "
                   "eigh and the whole calls hold one 8-byte read-back per Jacobi sweep", "components": COMPONENTS,
           "iters": iters, "reps": reps, "sizes": {}}
    for name, (m, n, D) in SIZES.items():
        X, Y = clustered(n, m, D, n)
        entry = {"samples": m, "originals": n, "D": D, "iters": iters}
        entry["covariance_of_the_originals"] = timed(lambda: pca.covariance(Y), iters, reps)
        entry["covariance_of_the_samples"] = timed(lambda: pca.covariance(X), iters, reps)
        for label, rows, count in (("covariance_of_the_originals", Y, n), ("covariance_of_the_samples", X, m)):
            t = entry[label]["ms_mean"] * 1e-3
            entry[label]["fp64_tflops"] = 2.0 * count * D * D / t / 1e12  # (the full square; half of it is formed)
            entry[label]["gb_per_s_read"] = 4.0 * count * D / t / 1e9
        _, cov = pca.covariance(Y)
        sweeps = pca.eigh(cov, info=True)[2].sweeps
        launches = 2 * (D + (D & 1) - 1) * sweeps
        entry["eigh_with_vectors"] = dict(timed(lambda: pca.eigh(cov), iters, reps), sweeps=sweeps, launches=launches)
        entry["eigh_values_only"] = dict(timed(lambda: pca.eigh(cov, vectors=False), iters, reps), sweeps=sweeps)
        entry["eigh_with_vectors"]["us_per_launch"] = 1e3 * entry["eigh_with_vectors"]["ms_mean"] / launches
        metric = FrechetDistance(Y, components=COMPONENTS)
        entry["values"] = metric(X)
        entry["frechet_distance_originals_kept"] = timed(lambda: metric(X), iters, reps)
        entry["frechet_distance_originals_not_kept"] = timed(lambda: FrechetDistance(Y, components=COMPONENTS)(X), iters, reps)
        if name == "1024x4096":
            Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
            host = {"threads": os.environ.get("OMP_NUM_THREADS", str(os.cpu_count()))}
            host_frechet(Xh, Yh)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = host_frechet(Xh, Yh)
                t.append(1e3 * (time.perf_counter() - t0))
            host["frechet_distance"] = {"ms_mean": float(np.mean(t)), "ms_min": min(t), "ms_max": max(t)}
            host["value"] = got
            host["difference_to_device"] = abs(got - entry["values"]["frechet_distance"])
            entry["host_float64_numpy"] = host
        out["sizes"][name] = entry
        print(name, json.dumps({k: (round(v["ms_mean"], 3) if isinstance(v, dict) and "ms_mean" in v else None)
                                for k, v in entry.items() if isinstance(v, dict)}), flush=True)
        del X, Y
    return out


def quality():
    import solver_quality as SQ
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import FrechetDistance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft
    from manifold_bench import BATCH, BUDGET, EPOCHS_TF, LR_MAX, N_SAMPLES, SEED

    X = SQ.dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    originals = X.reshape(X.shape[0], -1).contiguous()
    metric = FrechetDistance(originals, components=COMPONENTS)
    baseline = metric.baseline_metrics

    def score_samples(samples):
        rows = unstandardize_idft(samples.cuda(), mean, std).reshape(samples.shape[0], -1).contiguous()
        found = {k: float(v) for k, v in metric(rows).items()}
        excess_mean = found["frechet_mean_term"] - baseline["frechet_mean_term_self"]
        excess_cov = found["frechet_cov_term"] - baseline["frechet_cov_term_self"]
        found.update(ratio_to_baseline=found["frechet_distance"] / baseline["frechet_distance_self"],
                     excess_mean_term=excess_mean, excess_cov_term=excess_cov,
                     term_carrying_the_excess=_carrier(excess_mean, excess_cov))
        return found

    def draw(model):
        s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=SEED,
                             **SQ.SOLVERS["euler_maruyama"][0])
        return s.sample(num_samples=N_SAMPLES, num_diffusion_steps=BUDGET)

    out = {"what": f"FrechetDistance ({COMPONENTS} components) in the time domain of 1024 samples against the 4096-series "
                   "four-family target, next to the halves-of-the-data baseline (2048 against 2048); Euler-Maruyama, 200 score "
                   "evaluations, VP, Philox seed 1", "n_data": SQ.N_DATA, "n_samples": N_SAMPLES,
           "baseline": {k: float(v) for k, v in baseline.items()}, "sets": {}}
    g = torch.Generator().manual_seed(SEED)
    pick = torch.randint(0, SQ.N_DATA, (N_SAMPLES,), generator=g)
    out["sets"]["exact_draws_bandwidth_0.1"] = score_samples(Z.cpu()[pick] + SQ.BANDWIDTH * torch.randn(N_SAMPLES, SQ.L, SQ.CH,
                                                                                                   generator=g))
    out["sets"]["training_series_themselves"] = score_samples(Z.cpu()[pick])
    print("baseline", out["baseline"], flush=True)
    print("exact", out["sets"]["exact_draws_bandwidth_0.1"], flush=True)
    print("training series", out["sets"]["training_series_themselves"], flush=True)
    steps = EPOCHS_TF * (SQ.N_DATA // BATCH)
    sch = SQ.scheduler("vp")
    torch.manual_seed(0)
    model = ScoreModule(n_channels=SQ.CH, max_len=SQ.L, noise_scheduler=sch, d_model=60, num_layers=3, n_head=12,
                        num_training_steps=steps, lr_max=LR_MAX).cuda()
    t0 = time.perf_counter()
    Trainer(model, seed=0).fit(Z, batch_size=BATCH, max_epochs=EPOCHS_TF)
    out["training_seconds"] = time.perf_counter() - t0
    model.eval()
    out["sets"]["transformer_100_epochs"] = score_samples(draw(model))
    print("transformer", out["sets"]["transformer_100_epochs"], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet.json"))
    ap.add_argument("--only", choices=("timing", "quality"))
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pca_bench.py measures on an MI355X; no device found")
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    if args.only != "quality":
        result["timing"] = timing(args.iters, args.reps)
    if args.only != "timing":
        result["quality"] = quality()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
