"""Kernel two-sample statistics on one MI355X: what they cost and what they say.  Writes profiles/kernel_mmd.json.

    python3 tools/mmd_bench.py [--out profiles/kernel_mmd.json] [--only timing|quality]

Timing.  ffd_mmd_rowsums (through ``utils.kernel_mmd.row_sums``) with one gamma and with the five-gamma ladder, and
ffd_nn_ball_count on the same pair of sets in the same process (the same tiles with a cheaper epilogue), at the ECG
evaluation size (10 000 samples against 87 554 series of 187 points) and at 1024 x 4096 x 187, between device events: a
warm-up, then REPS repetitions of ITERS calls (mean / min / max of the repetitions).  A whole ``KernelMMD`` call with the
originals' part cached (every call after the first) and not cached (a fresh object per call); a 1000-permutation test
at N = 8192 pooled rows.  The rate counts 2 D FLOP per pair over the whole call against the 157.3 TFLOP/s fp32 matrix
peak: the share of the matrix pipe the call keeps busy, not a kernel's.  The comparison line is a float64 numpy
restatement (centred Gram form through the host's BLAS, one exp per gamma) on the host's threads at the small size.

Quality.  The sample sets of tools/manifold_bench.py (4096-series four-family target, 1024 samples each): ``mmd2`` next
to ``mmd2_self``, ``p_value`` at 1000 permutations, and the precision (k = 5) among the tenth of the samples with the
largest witness value against the precision of the rest."""
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

FP32_PEAK = 157.3e12
SIZES = {"ecg_eval": (10000, 87554, 187), "1024x4096": (1024, 4096, 187)}
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
PERMUTATIONS, PERM_ROWS = 1000, 4096
K = 5


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
    entry["tflops"] = flops / (entry["ms_mean"] * 1e-3) / 1e12
    entry["share_of_fp32_peak"] = flops / (entry["ms_mean"] * 1e-3) / FP32_PEAK
    return entry


def host_rowsums(A, B, gammas):
    """float64: centred Gram form through BLAS, one exp per gamma."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    mean = B.mean(axis=0)
    A, B = A - mean, B - mean
    d = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)
    return np.stack([np.exp(-g * d).sum(axis=1) for g in gammas])


def clustered(n, m, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 3.0 * torch.randn(4, D, device="cuda", generator=g)
    Y = centres[torch.randint(0, 4, (n,), device="cuda", generator=g)] + torch.randn(n, D, device="cuda", generator=g)
    X = centres[torch.randint(0, 4, (m,), device="cuda", generator=g)] + torch.randn(m, D, device="cuda", generator=g)
    return X.contiguous(), Y.contiguous()


def timing(iters, reps):
    from fastfourierdiffusion_amd.sampling.metrics import KernelMMD
    from fastfourierdiffusion_amd.utils import kernel_mmd as KM
    from fastfourierdiffusion_amd.utils import neighbours as NB

    out = {"what": "ms per call between device events: mean / min / max of REPS repetitions of ITERS calls after a warm-up; "
                   "tflops = 2 D FLOP per pair over the whole call (centring and the fold included) against the 157.3 TFLOP/s "
                   "fp32 matrix peak", "scales": SCALES, "iters": iters, "reps": reps, "sizes": {}}
    for name, (m, n, D) in SIZES.items():
        X, Y = clustered(n, m, D, n)
        centre = KM.column_mean(Y)
        gammas = KM.ladder_gammas(float(KM.bandwidth(Y).item()), SCALES)
        _, rad_y = NB.self_search(Y, K)
        it = iters if name != "ecg_eval" else max(1, iters // 4)
        entry = {"samples": m, "originals": n, "D": D, "iters": it}
        entry["ball_count_samples_in_originals"] = with_rate(timed(lambda: NB.ball_counts(X, Y, rad_y), it, reps), m, n, D)
        entry["rowsums_1_gamma"] = with_rate(timed(lambda: KM.row_sums(X, Y, centre, gammas[2:3]), it, reps), m, n, D)
        entry["rowsums_5_gammas"] = with_rate(timed(lambda: KM.row_sums(X, Y, centre, gammas), it, reps), m, n, D)
        # again, in the other order: the spread between two timings of the same call in one process
        entry["ball_count_again"] = with_rate(timed(lambda: NB.ball_counts(X, Y, rad_y), it, reps), m, n, D)
        for key in ("rowsums_1_gamma", "rowsums_5_gammas"):
            entry[key]["ratio_to_ball_count"] = entry[key]["ms_mean"] / entry["ball_count_samples_in_originals"]["ms_mean"]
        metric = KernelMMD(Y)
        entry["values"] = metric(X)
        entry["kernel_mmd_cached"] = timed(lambda: metric(X), it, reps)
        entry["kernel_mmd_not_cached"] = timed(lambda: KernelMMD(Y)(X), max(1, it // 2), reps)
        if name == "1024x4096":
            Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
            host = {"threads": os.environ.get("OMP_NUM_THREADS", str(os.cpu_count()))}
            for label, gs in (("rowsums_1_gamma", gammas[2:3]), ("rowsums_5_gammas", gammas)):
                host_rowsums(Xh, Yh, gs)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    got = host_rowsums(Xh, Yh, gs)
                    t.append(1e3 * (time.perf_counter() - t0))
                host[label] = {"ms_mean": float(np.mean(t)), "ms_min": min(t), "ms_max": max(t)}
            dev = KM.row_sums(X, Y, centre, gammas).cpu().numpy()
            host["largest_row_mean_difference_to_device"] = float(np.abs(dev - got).max()) / n
            entry["host_float64_numpy"] = host
        out["sizes"][name] = entry
        print(name, json.dumps({k: (round(v["ms_mean"], 3) if isinstance(v, dict) and "ms_mean" in v else None)
                                for k, v in entry.items() if isinstance(v, dict)}), flush=True)
        del X, Y
    X, Y = clustered(PERM_ROWS, PERM_ROWS, 187, 7)
    centre = KM.column_mean(Y)
    gammas = KM.ladder_gammas(float(KM.bandwidth(Y).item()), SCALES)
    A = torch.from_numpy(KM.permutation_assignments(PERM_ROWS, PERM_ROWS, PERMUTATIONS, 0)).cuda()
    entry = timed(lambda: KM.permutation_test(X, Y, centre, gammas, A), max(1, iters // 4), reps)
    entry.update(pooled_rows=2 * PERM_ROWS, permutations=PERMUTATIONS, D=187,
                 fp64_matrix_tflops=2.0 * (2 * PERM_ROWS) ** 2 * (PERMUTATIONS + 1) / (entry["ms_mean"] * 1e-3) / 1e12,
                 p_value=KM.p_value(KM.permutation_test(X, Y, centre, gammas, A)))
    out["permutation_test_N8192_P1000"] = entry
    print("permutation test", json.dumps(entry), flush=True)
    return out


def quality():
    import solver_quality as SQ
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import KernelMMD
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
    metric = KernelMMD(originals, permutations=PERMUTATIONS, random_seed=SEED)
    baseline = metric.baseline_metrics
    _, rad_y = NB.self_search(originals, K)

    def score_samples(samples):
        rows = unstandardize_idft(samples.cuda(), mean, std).reshape(samples.shape[0], -1).contiguous()
        found = metric(rows)
        w = metric.witness(rows)
        inside = (NB.ball_counts(rows, originals, rad_y) > 0).double()
        top = torch.argsort(w, descending=True)[: rows.shape[0] // 10]
        rest = torch.ones(rows.shape[0], dtype=torch.bool, device=rows.device)
        rest[top] = False
        found.update(mmd2_self=baseline["mmd2_self"], p_value_self=baseline["p_value_self"],
                     precision=float(inside.mean()), precision_top_witness_tenth=float(inside[top].mean()),
                     precision_rest=float(inside[rest].mean()))
        return {k: float(v) for k, v in found.items()}

    def draw(model):
        s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=SEED,
                             **SQ.SOLVERS["euler_maruyama"][0])
        return s.sample(num_samples=N_SAMPLES, num_diffusion_steps=BUDGET)

    out = {"what": "KernelMMD (scales 1/4 ... 4, 1000 permutations) in the time domain of 1024 samples against the 4096-series "
                   "four-family target, and the precision (k = 5) among the tenth of the samples with the largest witness "
                   "value against the rest; Euler-Maruyama, 200 score evaluations, VP, Philox seed 1",
           "n_data": SQ.N_DATA, "n_samples": N_SAMPLES, "permutations": PERMUTATIONS, "sets": {}}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_mmd.json"))
    ap.add_argument("--only", choices=("timing", "quality"))
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mmd_bench.py measures on an MI355X; no device found")
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
