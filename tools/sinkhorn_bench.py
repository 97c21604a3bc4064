"""Entropic optimal transport on one MI355X: what it costs and what it says.  Writes profiles/sinkhorn.json.

    python3 tools/sinkhorn_bench.py [--out profiles/sinkhorn.json] [--only timing|quality]

Timing.  One ffd_sinkhorn_softmin pass (through ``utils.sinkhorn.softmin``) next to ffd_nn_ball_count and ffd_mmd_rowsums
(one gamma) on the same pair of sets in the same process -- the same tiles with cheaper epilogues, the two yardsticks --
at the ECG evaluation size (10 000 samples against 87 554 series of 187 points) and at 1024 x 4096 x 187, between device
events: a warm-up, then REPS repetitions of ITERS calls (mean / min / max of the repetitions).  The originals' self
potential (``self_potential`` over the metric's schedule), and a whole ``SinkhornDivergence`` call with the self potential
kept (every call after the first) and not kept (a fresh object per call).  The rate counts 2 D FLOP per pair over the
whole call against the 157.3 TFLOP/s fp32 matrix peak: the share of the matrix pipe the call keeps busy, not a kernel's.
The comparison line is a float64 numpy restatement of one softmin pass (centred Gram form through the host's BLAS, a
log-sum-exp) on the host's threads at the small size, with the largest difference to the device.

Quality.  The sample sets of tools/manifold_bench.py (4096-series four-family target, 1024 samples each): S next to the
halves-of-the-data baseline, ``sinkhorn_change``, and the precision (k = 5) among the tenth of the samples with the
largest transport price f - p against the precision of the rest; and the same with LONG_FINAL passes at the final eps
(the ``long_`` keys): whether the reading survives convergence."""
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

from mmd_bench import clustered, timed, with_rate  # noqa: E402

SIZES = {"ecg_eval": (10000, 87554, 187), "1024x4096": (1024, 4096, 187)}
BLUR = 0.05
LONG_FINAL = 60  # the quality sets once more with this many passes at the final eps: does the reading survive convergence?
K = 5


def host_softmin(A, B, h, eps):
    """float64: centred Gram form through BLAS, then the log-sum-exp."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    mean = B.mean(axis=0)
    A, B = A - mean, B - mean
    u = (h[None, :] - np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)) / eps
    m = u.max(axis=1)
    return -eps * (m + np.log(np.exp(u - m[:, None]).sum(axis=1) / B.shape[0]))


def timing(iters, reps):
    from fastfourierdiffusion_amd.sampling.metrics import SinkhornDivergence
    from fastfourierdiffusion_amd.utils import kernel_mmd as KM
    from fastfourierdiffusion_amd.utils import neighbours as NB
    from fastfourierdiffusion_amd.utils import sinkhorn as SK

    out = {"what": "ms per call between device events: mean / min / max of REPS repetitions of ITERS calls after a warm-up; "
                   "tflops = 2 D FLOP per pair over the whole call (centring and the merge included) against the 157.3 TFLOP/s "
                   "fp32 matrix peak", "blur": BLUR, "iters": iters, "reps": reps, "sizes": {}}
    for name, (m, n, D) in SIZES.items():
        X, Y = clustered(n, m, D, n)
        centre = KM.column_mean(Y)
        sigma2 = float(KM.bandwidth(Y).item())
        eps = BLUR * BLUR * sigma2
        schedule = SK.schedule(float(SK.diameter2(Y, centre).item()), eps)
        _, rad_y = NB.self_search(Y, K)
        it = iters if name != "ecg_eval" else max(1, iters // 4)
        entry = {"samples": m, "originals": n, "D": D, "iters": it, "eps": eps, "schedule_entries": len(schedule),
                 "schedule_first": schedule[0]}
        h = sigma2 * torch.randn(n, device="cuda", dtype=torch.float64)
        gamma = KM.ladder_gammas(sigma2, (1.0,))
        entry["ball_count_samples_in_originals"] = with_rate(timed(lambda: NB.ball_counts(X, Y, rad_y), it, reps), m, n, D)
        entry["mmd_rowsums_1_gamma"] = with_rate(timed(lambda: KM.row_sums(X, Y, centre, gamma), it, reps), m, n, D)
        for label, e in (("softmin_final_eps", eps), ("softmin_first_eps", schedule[0])):
            entry[label] = with_rate(timed(lambda: SK.softmin(X, Y, centre, h, e), it, reps), m, n, D)
        # again, in the other order: the spread between two timings of the same call in one process
        entry["mmd_rowsums_again"] = with_rate(timed(lambda: KM.row_sums(X, Y, centre, gamma), it, reps), m, n, D)
        for label in ("softmin_final_eps", "softmin_first_eps"):
            entry[label]["ratio_to_mmd_rowsums"] = entry[label]["ms_mean"] / entry["mmd_rowsums_1_gamma"]["ms_mean"]
            entry[label]["ratio_to_ball_count"] = entry[label]["ms_mean"] / entry["ball_count_samples_in_originals"]["ms_mean"]
        entry["mmd_rowsums_1_gamma"]["ratio_to_ball_count"] = (entry["mmd_rowsums_1_gamma"]["ms_mean"] /
                                                              entry["ball_count_samples_in_originals"]["ms_mean"])
        few = 1 if name == "ecg_eval" else max(1, it // 2)
        entry["self_potential_of_the_originals"] = timed(lambda: SK.self_potential(Y, centre, schedule), few, reps)
        metric = SinkhornDivergence(Y, blur=BLUR)
        entry["values"] = metric(X)
        entry["sinkhorn_divergence_q_kept"] = timed(lambda: metric(X), few, reps)
        entry["sinkhorn_divergence_q_not_kept"] = timed(lambda: SinkhornDivergence(Y, blur=BLUR)(X), few, reps)
        if name == "1024x4096":
            Xh, Yh, hh = X.cpu().numpy(), Y.cpu().numpy(), h.cpu().numpy()
            host = {"threads": os.environ.get("OMP_NUM_THREADS", str(os.cpu_count()))}
            host_softmin(Xh, Yh, hh, eps)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = host_softmin(Xh, Yh, hh, eps)
                t.append(1e3 * (time.perf_counter() - t0))
            host["softmin_final_eps"] = {"ms_mean": float(np.mean(t)), "ms_min": min(t), "ms_max": max(t)}
            dev = SK.softmin(X, Y, centre, h, eps).cpu().numpy()
            host["largest_difference_to_device"] = float(np.abs(dev - got).max())
            host["largest_value"] = float(np.abs(got).max())
            entry["host_float64_numpy"] = host
        out["sizes"][name] = entry
        print(name, json.dumps({k: (round(v["ms_mean"], 3) if isinstance(v, dict) and "ms_mean" in v else None)
                                for k, v in entry.items() if isinstance(v, dict)}), flush=True)
        del X, Y
    return out


def quality():
    import solver_quality as SQ
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import SinkhornDivergence
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils import neighbours as NB
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft
    from manifold_bench import BANDWIDTHS, BATCH, BUDGET, EPOCHS_TF, LR_MAX, N_SAMPLES, SEED

    X = SQ.dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    originals = X.reshape(X.shape[0], -1).contiguous()
    metric = SinkhornDivergence(originals, blur=BLUR)
    metric_long = SinkhornDivergence(originals, blur=BLUR, n_final=LONG_FINAL)
    baseline, baseline_long = metric.baseline_metrics, metric_long.baseline_metrics
    _, rad_y = NB.self_search(originals, K)

    def score_samples(samples):
        rows = unstandardize_idft(samples.cuda(), mean, std).reshape(samples.shape[0], -1).contiguous()
        found = metric(rows)
        price = metric.transport_price(rows)
        inside = (NB.ball_counts(rows, originals, rad_y) > 0).double()
        top = torch.argsort(price, descending=True)[: rows.shape[0] // 10]
        rest = torch.ones(rows.shape[0], dtype=torch.bool, device=rows.device)
        rest[top] = False
        found.update(sinkhorn_divergence_self=baseline["sinkhorn_divergence_self"],
                     sinkhorn_change_self=baseline["sinkhorn_change_self"], precision=float(inside.mean()),
                     precision_top_price_tenth=float(inside[top].mean()), precision_rest=float(inside[rest].mean()))
        long = metric_long(rows)
        top_long = torch.argsort(metric_long.transport_price(rows), descending=True)[: rows.shape[0] // 10]
        found.update(long_divergence=long["sinkhorn_divergence"], long_change=long["sinkhorn_change"],
                     long_divergence_self=baseline_long["sinkhorn_divergence_self"],
                     long_change_self=baseline_long["sinkhorn_change_self"],
                     long_precision_top_price_tenth=float(inside[top_long].mean()))
        return {k: float(v) for k, v in found.items()}

    def draw(model):
        s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=SEED,
                             **SQ.SOLVERS["euler_maruyama"][0])
        return s.sample(num_samples=N_SAMPLES, num_diffusion_steps=BUDGET)

    out = {"what": f"SinkhornDivergence (blur {BLUR}) in the time domain of 1024 samples against the 4096-series four-family "
                   "target, and the precision (k = 5) among the tenth of the samples with the largest transport price f - p "
                   "against the rest; long_*: the same with n_final = %d; Euler-Maruyama, 200 score evaluations, VP, Philox seed 1" % LONG_FINAL,
           "n_data": SQ.N_DATA, "n_samples": N_SAMPLES, "sets": {}}
    g = torch.Generator().manual_seed(SEED)
    pick = torch.randint(0, SQ.N_DATA, (N_SAMPLES,), generator=g)
    out["sets"]["exact_draws_bandwidth_0.1"] = score_samples(Z.cpu()[pick] + SQ.BANDWIDTH * torch.randn(N_SAMPLES, SQ.L, SQ.CH,
                                                                                                   generator=g))
    out["sets"]["training_series_themselves"] = score_samples(Z.cpu()[pick])
    print("exact", out["sets"]["exact_draws_bandwidth_0.1"], flush=True)
    print("training series", out["sets"]["training_series_themselves"], flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinkhorn.json"))
    ap.add_argument("--only", choices=("timing", "quality"))
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sinkhorn_bench.py measures on an MI355X; no device found")
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
