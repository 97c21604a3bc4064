"""Sample quality with a network trained on the device: `python tools/train_quality.py [out.json]`
(default profiles/train_quality.json).

The MLP score network (MLPScoreModule at its defaults: d_model 72, d_mlp 512, 3 blocks; 300 epochs) and the ECG
transformer (ScoreModule, d_model 60, 12 heads, 3 layers, dim_feedforward 2048; 100 epochs) are trained with
`training.Trainer.fit` on the standardized spectra of the 4096-series multimodal target of tools/solver_quality.py
(L = 187, C = 1), under VP and VE, without dropout.  4096 samples are then drawn with Euler-Maruyama and with `ode_ab2`
at 200 score evaluations (Philox draws, three seeds) and scored against the data set with the same metrics as
tools/solver_quality.py.  Next to them: the floor of exact draws and the closed-form mixture score's numbers for the
same solvers, read from profiles/solver_quality.json.
"""
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

EPOCHS, BATCH, LR_MAX, BUDGET = 300, 64, 1e-3, 200
EPOCHS_TF = 100  # the ECG transformer (d_model 60, 12 heads, 3 layers, dim_feedforward 2048)
SOLVERS = {"euler_maruyama": BUDGET, "ode_ab2": BUDGET + 1}  # grid points for 200 score evaluations


def main(out_path):
    from fastfourierdiffusion_amd.models.score_models import MLPScoreModule, ScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    X = SQ.dataset().cuda()
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    metrics = MetricCollection([partial(SlicedWasserstein, random_seed=42, num_directions=1000),
                                partial(MarginalWasserstein, random_seed=42)], original_samples=X.cpu(),
                               include_baselines=False)
    keys = ("time_sliced_wasserstein_mean", "time_marginal_wasserstein_mean", "freq_sliced_wasserstein_mean")

    def score_samples(samples):
        found = metrics(unstandardize_idft(samples.cuda(), mean, std).cpu())
        return {k: float(found[k]) for k in keys}

    def spread(rows):
        return {k: {"mean": float(np.mean([r[k] for r in rows])), "min": float(min(r[k] for r in rows)),
                    "max": float(max(r[k] for r in rows))} for k in keys}

    with open(os.path.join(ROOT, "profiles", "solver_quality.json")) as f:
        mix = json.load(f)
    steps = EPOCHS * (SQ.N_DATA // BATCH)
    result = {"what": "time-domain sliced Wasserstein distance (and two companions) of 4096 samples of a score network "
                      "TRAINED ON THE DEVICE to the 4096-series dataset; mean / min / max over three sampling seeds",
              "model": "MLPScoreModule d_model=72 d_mlp=512 num_layers=3, dropout 0 (the reference trains with 0.1)",
              "training": {"epochs": EPOCHS, "batch_size": BATCH, "steps": steps, "lr_max": LR_MAX, "seed": 0},
              "score_evaluations": BUDGET, "floor_exact_draws": {k: mix["floor"][k] for k in keys}, "sde": {}}
    result["transformer"] = {"model": "ScoreModule d_model=60 n_head=12 num_layers=3 dim_feedforward=2048, dropout 0",
                             "training": {"epochs": EPOCHS_TF, "batch_size": BATCH, "steps": EPOCHS_TF * (SQ.N_DATA // BATCH)}}
    for net in ("mlp", "transformer"):
        epochs = EPOCHS if net == "mlp" else EPOCHS_TF
        steps = epochs * (SQ.N_DATA // BATCH)
        for sde in ("vp", "ve"):
            sch = SQ.scheduler(sde)
            torch.manual_seed(0)
            if net == "mlp":
                model = MLPScoreModule(n_channels=SQ.CH, max_len=SQ.L, noise_scheduler=sch, num_training_steps=steps,
                                       lr_max=LR_MAX).cuda()
            else:
                model = ScoreModule(n_channels=SQ.CH, max_len=SQ.L, noise_scheduler=sch, d_model=60, num_layers=3, n_head=12,
                                    num_training_steps=steps, lr_max=LR_MAX).cuda()
            tr = Trainer(model, seed=0)
            v0 = float(evaluate_loss(model, Z, 512, seed=1)["loss"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = tr.fit(Z, batch_size=BATCH, max_epochs=epochs)["train_loss"]
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            v1 = float(evaluate_loss(model, Z, 512, seed=1)["loss"])
            entry = {"train_seconds": seconds, "ms_per_step": 1e3 * seconds / steps, "loss_fixed_draws_before": v0,
                     "loss_fixed_draws_after": v1, "train_loss_first_epoch": float(hist[:64].mean()),
                     "train_loss_last_epoch": float(hist[-64:].mean()), "solvers": {}}
            model.eval()
            for name, points in SOLVERS.items():
                rows = []
                for seed in SQ.SEEDS:
                    s = DiffusionSampler(score_model=model, sample_batch_size=SQ.N_SAMPLES, rng="philox", seed=seed,
                                         **SQ.SOLVERS[name][0])
                    rows.append(score_samples(s.sample(num_samples=SQ.N_SAMPLES, num_diffusion_steps=points)))
                entry["solvers"][name] = {"grid_points": points, "trained": spread(rows),
                                          "mixture_score": {k: mix["sde"][sde][name][str(BUDGET)][k] for k in keys}}
                print(net, sde, name, {k: round(v["mean"], 4) for k, v in entry["solvers"][name]["trained"].items()}, flush=True)
            result["sde" if net == "mlp" else "transformer"][sde] = entry
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_quality.json"))
