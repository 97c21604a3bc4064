"""Nearest-neighbour sample metrics on one MI355X: what they cost and what they say.  Writes profiles/manifold_metrics.json.

    python3 tools/manifold_bench.py [--out profiles/manifold_metrics.json] [--only timing|quality]

Timing.  ffd_nn_search and ffd_nn_ball_count (through ``utils.neighbours``) and a whole ``ManifoldMetrics`` call, at the
ECG evaluation size (10 000 samples against 87 554 series of 187 points) and at 1024 x 4096 x 187, between device events:
a warm-up, then REPS repetitions of ITERS calls (mean / min / max of the repetitions).  The metric is timed with its
original set's self-search cached (every call after the first) and not cached (a fresh object per call).  The rate of
a ball count counts 2 D FLOP per (query, reference) pair over the whole call -- centring both sets included, so it is a
lower bound on the pair kernel's own rate -- against the 157.3 TFLOP/s fp32 matrix peak; a search's rate is the same
count over a call that also writes the distance block out and merges it.  The comparison line is a float64 numpy
restatement (centred Gram form through the host's BLAS, argpartition + sort for the k smallest) on the host's threads
at 1024 x 4096 x 187, which it can finish.

Quality.  The four-family target of tools/solver_quality.py (4096 series, L = 187), 1024 samples each of: exact draws of
the bandwidth-0.1 mixture; the ``MixtureScoreModule.from_data`` sampler over a sweep of bandwidths down to 0; the ECG
transformer trained by the recipe of tools/train_quality.py (VP, 100 epochs).  All samplers: Euler-Maruyama, 200 score
evaluations, Philox draws, seed 1.  Every key of ``ManifoldMetrics`` (k = 5) in the time domain next to the time-domain
sliced Wasserstein distance."""
import argparse
import json
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import solver_quality as SQ  # noqa: E402

FP32_PEAK = 157.3e12
SIZES = {"ecg_eval": (10000, 87554, 187), "1024x4096": (1024, 4096, 187)}
K = 5
N_SAMPLES, BUDGET, SEED = 1024, 200, 1
BANDWIDTHS = (0.1, 0.03, 0.01, 0.003, 0.0)
EPOCHS_TF, BATCH, LR_MAX = 100, 64, 1e-3


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


def with_rate(entry, nq, nr, D):
    flops = 2.0 * nq * nr * D
    entry["tflop"] = flops / 1e12
    entry["tflops"] = flops / (entry["ms_mean"] * 1e-3) / 1e12
    entry["share_of_fp32_peak"] = flops / (entry["ms_mean"] * 1e-3) / FP32_PEAK
    return entry


def host_knn(Q, R, k, exclude_self):
    """float64: centred Gram form through BLAS, the k smallest by argpartition, sorted."""
    Q, R = Q.astype(np.float64), R.astype(np.float64)
    mean = R.mean(axis=0)
    Q, R = Q - mean, R - mean
    d = np.maximum((Q * Q).sum(1)[:, None] + (R * R).sum(1)[None, :] - 2.0 * (Q @ R.T), 0.0)
    if exclude_self:
        np.fill_diagonal(d, np.inf)
    part = np.argpartition(d, k - 1, axis=1)[:, :k]
    vals = np.take_along_axis(d, part, axis=1)
    order = np.argsort(vals, axis=1, kind="stable")
    return np.take_along_axis(vals, order, axis=1), np.take_along_axis(part, order, axis=1)


def host_metrics(Y, X, k):
    """The eight numbers in float64 on the host (Gram form): the work a whole ManifoldMetrics call does."""
    self_y, _ = host_knn(Y, Y, k, True)
    self_x, _ = host_knn(X, X, k, True)
    Y64, X64 = Y.astype(np.float64), X.astype(np.float64)
    d = np.maximum((X64 * X64).sum(1)[:, None] + (Y64 * Y64).sum(1)[None, :] - 2.0 * (X64 @ Y64.T), 0.0)
    near = d.argmin(axis=1)
    dmin = d[np.arange(len(X)), near]
    cx = (d <= self_y[None, :, k - 1]).sum(axis=1)
    cy = (d.T <= self_x[None, :, k - 1]).sum(axis=1)
    return dict(precision=float((cx > 0).mean()), recall=float((cy > 0).mean()), density=float(cx.sum()) / (k * len(X)),
                coverage=float((d.min(axis=0) <= self_y[:, k - 1]).mean()), authenticity=float((dmin > self_y[near, 0]).mean()),
                nn_distance_mean=float(np.sqrt(dmin).mean()), nn_distance_min=float(np.sqrt(dmin.min())),
                copy_share=float((dmin == 0).mean()))


def timing(iters, reps):
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics
    from fastfourierdiffusion_amd.utils import neighbours as NB

    out = {"what": "ms per call between device events: mean / min / max of REPS repetitions of ITERS calls after a warm-up; "
                   "tflops = 2 D FLOP per pair over the whole call (centring, and for a search the distance block's round "
                   "trip and merge, included) against the 157.3 TFLOP/s fp32 matrix peak",
           "k": K, "iters": iters, "reps": reps, "work_budget_bytes": NB.WORK_BUDGET_BYTES, "sizes": {}}
    for name, (m, n, D) in SIZES.items():
        g = torch.Generator(device="cuda").manual_seed(n)
        centres = 3.0 * torch.randn(4, D, device="cuda", generator=g)
        Y = centres[torch.randint(0, 4, (n,), device="cuda", generator=g)] + torch.randn(n, D, device="cuda", generator=g)
        X = centres[torch.randint(0, 4, (m,), device="cuda", generator=g)] + torch.randn(m, D, device="cuda", generator=g)
        self_y, rad_y = NB.self_search(Y, K)
        _, rad_x = NB.self_search(X, K)
        it = iters if name != "ecg_eval" else max(1, iters // 4)
        entry = {"samples": m, "originals": n, "D": D, "iters": it}
        entry["search_samples_in_originals_k1"] = with_rate(timed(lambda: NB.nearest_neighbours(X, Y, 1), it, reps), m, n, D)
        entry["search_originals_in_samples_k1"] = with_rate(timed(lambda: NB.nearest_neighbours(Y, X, 1), it, reps), n, m, D)
        entry["self_search_samples"] = with_rate(timed(lambda: NB.self_search(X, K), it, reps), m, m, D)
        entry["self_search_originals"] = with_rate(timed(lambda: NB.self_search(Y, K), it, reps), n, n, D)
        entry["ball_count_samples_in_originals"] = with_rate(timed(lambda: NB.ball_counts(X, Y, rad_y), it, reps), m, n, D)
        entry["ball_count_originals_in_samples"] = with_rate(timed(lambda: NB.ball_counts(Y, X, rad_x), it, reps), n, m, D)
        metric = ManifoldMetrics(Y, k=K)
        values = metric(X)
        entry["manifold_metrics_cached"] = timed(lambda: metric(X), it, reps)
        entry["manifold_metrics_not_cached"] = timed(lambda: ManifoldMetrics(Y, k=K)(X), it, reps)
        entry["values"] = values
        if name == "1024x4096":
            Yh, Xh = Y.cpu().numpy(), X.cpu().numpy()
            host = {"threads": os.environ.get("OMP_NUM_THREADS", str(os.cpu_count()))}
            for label, fn in (("search_samples_in_originals_k1", lambda: host_knn(Xh, Yh, 1, False)),
                              ("self_search_originals", lambda: host_knn(Yh, Yh, K, True)),
                              ("manifold_metrics", lambda: host_metrics(Yh, Xh, K))):
                fn()
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    got = fn()
                    t.append(1e3 * (time.perf_counter() - t0))
                host[label] = {"ms_mean": float(np.mean(t)), "ms_min": min(t), "ms_max": max(t)}
            host["values"] = got
            entry["host_float64_numpy"] = host
        out["sizes"][name] = entry
        print(name, json.dumps({k: (round(v["ms_mean"], 3) if isinstance(v, dict) and "ms_mean" in v else None)
                                for k, v in entry.items() if isinstance(v, dict)}), flush=True)
        del Y, X
    return out


def quality():
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft

    X = SQ.dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    metrics = MetricCollection([partial(ManifoldMetrics, k=K),
                                partial(SlicedWasserstein, random_seed=42, num_directions=1000)], original_samples=X.cpu(),
                               include_baselines=False)

    def score_samples(samples):
        found = metrics(unstandardize_idft(samples.cuda(), mean, std).cpu())
        return {k: float(v) for k, v in found.items() if k.startswith("time_") and not k.endswith("_all")}

    def draw(model):
        s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=SEED,
                             **SQ.SOLVERS["euler_maruyama"][0])
        return s.sample(num_samples=N_SAMPLES, num_diffusion_steps=BUDGET)

    out = {"what": "ManifoldMetrics (k = 5) and the sliced Wasserstein distance, time domain, of 1024 samples against the "
                   "4096-series four-family target; Euler-Maruyama, 200 score evaluations, VP, Philox seed 1",
           "n_data": SQ.N_DATA, "n_samples": N_SAMPLES, "k": K, "sets": {}}
    g = torch.Generator().manual_seed(SEED)
    pick = torch.randint(0, SQ.N_DATA, (N_SAMPLES,), generator=g)
    out["sets"]["exact_draws_bandwidth_0.1"] = score_samples(Z.cpu()[pick] + SQ.BANDWIDTH * torch.randn(N_SAMPLES, SQ.L, SQ.CH,
                                                                                                   generator=g))
    out["sets"]["training_series_themselves"] = score_samples(Z.cpu()[pick])
    print("exact", out["sets"]["exact_draws_bandwidth_0.1"], flush=True)
    sch = SQ.scheduler("vp")
    for bw in BANDWIDTHS:
        model = MixtureScoreModule.from_data(Z.cpu(), sch, bandwidth=bw).cuda().eval()
        samples = draw(model)
        name = f"mixture_from_data_bandwidth_{bw:g}"
        if not bool(torch.isfinite(samples).all()):
            out["sets"][name] = {"unusable": "non-finite samples"}
        else:
            out["sets"][name] = score_samples(samples)
        print(name, out["sets"][name], flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifold_metrics.json"))
    ap.add_argument("--only", choices=("timing", "quality"))
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/manifold_bench.py measures on an MI355X; no device found")
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
