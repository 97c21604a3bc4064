"""Sample quality of the solvers of the fused loop against an exact score, and the cost of that score.

    python3 tools/solver_quality.py [out.json]            (default: profiles/solver_quality.json)
    python3 tools/solver_quality.py kernel [out.json]     (default: profiles/mixture_score.json)

Quality.  A seeded synthetic set of 4096 series (L = 187, C = 1), multimodal by construction (four families of sinusoid
sums with random phase and amplitude), goes through dft and standardization; ``MixtureScoreModule.from_data`` with a
bandwidth turns it into a Gaussian mixture whose diffused score is exact (ffd_mixture_score), so the samplers run
against the very distribution the data define.  For both schedulers and each of euler_maruyama, euler_maruyama + 1
corrector step, ode_euler, ode_heun, ode_ab2, dpmpp_2m, the budget of score evaluations is swept over
{10, 20, 50, 100, 200, 1000}; 4096 samples (Philox draws, three seeds) are scored against the dataset with the sliced and
marginal Wasserstein distances of MetricCollection (time domain and spectrum).  The FLOOR is the same distance for exact
draws of the mixture (pick a component, add sqrt(v) noise) over the same three seeds: a solver counts as converged when
it is inside the floor's spread.  Each row also reports dt g^2 G^2 / c at the last step the solver's grid takes (how far
an Euler-Maruyama step moves along the displacement there; 1 lands on the posterior mean -- with bandwidth 0 under VP it
is about 100 at 1000 steps and the last step throws the sample off the data, which is why the sweep uses a bandwidth).

Kernel.  Time per ffd_mixture_score call at B = 512, D = 187 with K = 4096 and K = 87 554 (the ECG training set's size),
between device events: 3 repetitions of ITERS calls after a warm-up, once with the means resident (one buffer, as in a
sampling loop, where they stay in the last-level cache) and once with x and the means rotated over enough copies to
exceed it.  The share of the fp32 peak counts 7 FLOP per (row, component, coordinate).
"""
import ctypes as C
import json
import math
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fastfourierdiffusion_amd import _native as N  # noqa: E402

L, CH, N_DATA, N_SAMPLES = 187, 1, 4096, 4096
BANDWIDTH = 0.1  # standard deviations of the standardized spectrum
BUDGETS = (10, 20, 50, 100, 200, 1000)
SEEDS = (1, 2, 3)
SNR = 0.16
FP32_PEAK = 157.3e12
# solver name -> (DiffusionSampler kwargs, score evaluations per step or interval, grid points for a budget)
SOLVERS = {
    "euler_maruyama": (dict(solver="euler_maruyama"), lambda b: b),
    "euler_maruyama_pc1": (dict(solver="euler_maruyama", corrector_steps=1, snr=SNR), lambda b: b // 2),
    "ode_euler": (dict(solver="ode_euler"), lambda b: b + 1),
    "ode_heun": (dict(solver="ode_heun"), lambda b: b // 2 + 1),
    "ode_ab2": (dict(solver="ode_ab2"), lambda b: b + 1),
    "dpmpp_2m": (dict(solver="dpmpp_2m"), lambda b: b + 1),
}


def dataset(seed=0):
    """(N_DATA, L, 1) time series: four families of sums of two or three sinusoids, random phase and amplitude."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / L
    fams = [((2.0, 5.0), 1.0), ((3.0, 7.0, 11.0), 0.8), ((1.0, 13.0), 1.2), ((4.0, 6.0, 9.0), 0.6)]
    fam = rng.integers(0, len(fams), N_DATA)
    X = np.zeros((N_DATA, L))
    for i in range(N_DATA):
        freqs, scale = fams[fam[i]]
        for f in freqs:
            X[i] += scale * rng.uniform(0.5, 1.5) * np.sin(2 * math.pi * (f * t + rng.uniform()))
        X[i] += 0.5 * (fam[i] - 1.5)  # the families also differ in level
    return torch.from_numpy(X[:, :, None].astype(np.float32))


def scheduler(sde):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=True)
    sch.set_noise_scaling(L)
    return sch


def last_step_gain(sch, sde, n_points, solver, var):
    """dt g(t)^2 G_l^2 / c_lc, largest over the coordinates, at the last point the solver evaluates the score at."""
    ts = torch.linspace(1.0, sch.eps, n_points)
    dt = float(ts[0] - ts[1])
    t = float(ts[-1] if solver.startswith("euler_maruyama") or solver == "ode_heun" else ts[-2])
    a, b = sch._sde_ab()
    if sde == "vp":
        la = -0.25 * t * t * (b - a) - 0.5 * t * a
        alpha2, sigma2, g2 = math.exp(2 * la), -math.expm1(2 * la), a + t * (b - a)
    else:
        alpha2, sigma2 = 1.0, (a * (b / a) ** t) ** 2
        g2 = (a * math.sqrt(2 * math.log(b / a)) * (b / a) ** t) ** 2
    G2 = sch.G.double().numpy() ** 2
    c = alpha2 * var.double().numpy() + sigma2 * G2[:, None]
    return float((dt * g2 * G2[:, None] / c).max())


def quality(out_path):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft

    X = dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    metrics = MetricCollection([partial(SlicedWasserstein, random_seed=42, num_directions=1000),
                                partial(MarginalWasserstein, random_seed=42)], original_samples=X.cpu(),
                               include_baselines=False)

    def score_samples(samples):
        found = metrics(unstandardize_idft(samples.cuda(), mean, std).cpu())
        return {k: v for k, v in found.items() if k.endswith("_mean") or k.endswith("_max")}

    def spread(rows):
        keys = rows[0].keys()
        return {k: {"mean": float(np.mean([r[k] for r in rows])), "min": float(min(r[k] for r in rows)),
                    "max": float(max(r[k] for r in rows))} for k in keys}

    floor_rows = []
    for seed in SEEDS:
        g = torch.Generator().manual_seed(seed)
        pick = torch.randint(0, N_DATA, (N_SAMPLES,), generator=g)
        floor_rows.append(score_samples(Z.cpu()[pick] + BANDWIDTH * torch.randn(N_SAMPLES, L, CH, generator=g)))
    result = {"what": "sliced / marginal Wasserstein distance of 4096 samples to the 4096-series dataset that defines the "
                      "mixture; mean / min / max over three seeds", "L": L, "C": CH, "n_data": N_DATA,
              "n_samples": N_SAMPLES, "bandwidth": BANDWIDTH, "budgets": list(BUDGETS), "seeds": list(SEEDS),
              "floor": spread(floor_rows), "sde": {}}
    for sde in ("vp", "ve"):
        sch = scheduler(sde)
        model = MixtureScoreModule.from_data(Z.cpu(), sch, bandwidth=BANDWIDTH).cuda().eval()
        var = model.mixture.variance.detach().cpu()
        table = {}
        for name, (kw, points) in SOLVERS.items():
            table[name] = {}
            for budget in BUDGETS:
                n = points(budget)
                rows = []
                for seed in SEEDS:
                    s = DiffusionSampler(score_model=model, sample_batch_size=N_SAMPLES, rng="philox", seed=seed, **kw)
                    rows.append(score_samples(s.sample(num_samples=N_SAMPLES, num_diffusion_steps=n)))
                table[name][str(budget)] = {"grid_points": n, "last_step_dt_g2_G2_over_c":
                                            last_step_gain(sch, sde, n, name, var), **spread(rows)}
                print(sde, name, budget, {k: round(v["mean"], 4) for k, v in table[name][str(budget)].items()
                                          if isinstance(v, dict)}, flush=True)
        result["sde"][sde] = table
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


def kernel(out_path):
    lib = N.lib()
    B, D, ITERS, REPS = 512, L * CH, 50, 3
    desc = N.SdeDesc(N.FFD_SDE_VP, 0, 0.1, 20.0)
    G = scheduler("vp").G.cuda()
    t = torch.tensor([0.5], device="cuda")
    result = {"what": "ms per ffd_mixture_score call (k_mixture_part + k_mixture_merge), device events around ITERS calls, "
                      "mean / min / max of 3 repetitions; share of the 157.3 TFLOP/s fp32 peak at 7 FLOP per (row, component, "
                      "coordinate)", "B": B, "D": D, "iters": ITERS, "cases": {}}
    stream = int(torch.cuda.current_stream().cuda_stream)
    for K in (4096, 87554):
        copies = max(2, math.ceil(300e6 / (K * D * 4)))  # enough means to exceed the 256 MB last-level cache
        g = torch.Generator(device="cuda").manual_seed(K)
        means = torch.randn(copies, K, D, device="cuda", generator=g)
        xs = means[0, torch.randint(0, K, (copies, B), device="cuda", generator=g)] * math.exp(-0.5 * 2.5) + \
            0.8 * torch.randn(copies, B, D, device="cuda", generator=g)
        logw = torch.full((K,), -math.log(K), device="cuda")
        var = torch.full((D,), 0.01, device="cuda")
        n = lib.ffd_mixture_work_floats(B, K, L, CH)
        work = torch.empty(n, device="cuda")
        out = torch.empty(B, D, device="cuda")

        def call(i):
            rc = lib.ffd_mixture_score(C.byref(desc), xs[i].data_ptr(), t.data_ptr(), 0, means[i].data_ptr(),
                                       logw.data_ptr(), var.data_ptr(), G.data_ptr(), out.data_ptr(), B, K, L, CH,
                                       work.data_ptr(), n, stream)
            assert rc == 0, rc

        case = {}
        for mode in ("resident", "rotated"):
            for i in range(10):
                call(i % copies if mode == "rotated" else 0)
            ms = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(ITERS):
                    call(i % copies if mode == "rotated" else 0)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / ITERS)
            flops = 7.0 * B * K * D
            case[mode] = {"ms_mean": float(np.mean(ms)), "ms_min": min(ms), "ms_max": max(ms),
                          "tflops": flops / (np.mean(ms) * 1e-3) / 1e12,
                          "share_of_fp32_peak": flops / (np.mean(ms) * 1e-3) / FP32_PEAK}
        case["means_copies_rotated"] = copies
        result["cases"][f"K{K}"] = case
        print(K, case, flush=True)
        del means, xs
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "kernel":
        kernel(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "mixture_score.json"))
    else:
        quality(args[0] if args else os.path.join(ROOT, "profiles", "solver_quality.json"))
