"""Sample quality of a class-conditional network trained on the device, per class and guidance scale:
`python tools/class_quality.py [out.json]` (default profiles/class_quality.json).

The four-family target of tools/solver_quality.py (4096 series, L = 187, C = 1; the family of a series is regenerated with
the same generator and is its label) goes through dft and standardization.  The ECG transformer with classes
(ClassConditionalScoreModule, d_model 60, 12 heads, 3 layers, dim_feedforward 2048, 4 classes) is trained as in
tools/train_quality.py (100 epochs, batch 64, lr_max 1e-3, VP, no dropout of activations) with p_uncond = 0.1.

Per class k and per g in {0, 1, 1.5, 2, 3}, 1024 samples labelled k are drawn with Euler-Maruyama at 200 steps (Philox
draws, one batch of 4 x 1024 with the four labels) and scored against THAT CLASS's series:

  * the time-domain sliced Wasserstein distance (1000 directions), next to the floor of exact draws (1024 of the class's
    own series with the bandwidth's noise, three seeds) and to the exact class-conditional score
    (``MixtureScoreModule.from_data`` on the class's subset, the same sampler);
  * the share of samples whose nearest training series (Euclidean, time domain, over all 4096) belongs to family k.

g = 0 ignores the label: its row is the unconditional model scored against each class, the reference point for what the
label buys.  A larger g is expected to raise the share and, past some scale, to cost diversity (a larger distance).
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

EPOCHS, BATCH, LR_MAX, STEPS, P_UNCOND, PER_CLASS = 100, 64, 1e-3, 200, 0.1, 1024
SCALES = (0.0, 1.0, 1.5, 2.0, 3.0)
N_FAM = 4
KEY = "time_sliced_wasserstein_mean"


def families(seed=0):
    """The family index of every series of SQ.dataset(seed): the generator's first draw."""
    return np.random.default_rng(seed).integers(0, N_FAM, SQ.N_DATA)


def main(out_path):
    from fastfourierdiffusion_amd.models.score_models import ClassConditionalScoreModule, MixtureScoreModule
    from fastfourierdiffusion_amd.sampling.metrics import MetricCollection, SlicedWasserstein
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.fourier import dft, unstandardize_idft
    from fastfourierdiffusion_amd.utils.losses import evaluate_loss

    X = SQ.dataset().cuda()
    fam = families()
    y = torch.from_numpy(fam)
    spec = dft(X)
    mean, std = spec.mean(0), spec.std(0).clamp_min(1e-6)
    Z = ((spec - mean) / std).contiguous()
    Xt = X.cpu()
    metrics = [MetricCollection([partial(SlicedWasserstein, random_seed=42, num_directions=1000)],
                                original_samples=Xt[fam == k], include_baselines=False) for k in range(N_FAM)]
    flat = X.reshape(SQ.N_DATA, -1)
    fam_dev = y.cuda()

    def to_time(samples):
        return unstandardize_idft(samples.cuda(), mean, std)

    def distance(k, time_samples):
        return float(metrics[k](time_samples.cpu())[KEY])

    def nearest_share(k, time_samples):
        d2 = torch.cdist(time_samples.reshape(len(time_samples), -1), flat)
        return float((fam_dev[d2.argmin(dim=1)] == k).float().mean())

    sch = SQ.scheduler("vp")
    steps = EPOCHS * (SQ.N_DATA // BATCH)
    torch.manual_seed(0)
    model = ClassConditionalScoreModule(n_channels=SQ.CH, max_len=SQ.L, noise_scheduler=sch, n_classes=N_FAM, d_model=60,
                                        num_layers=3, n_head=12, num_training_steps=steps, lr_max=LR_MAX).cuda()
    tr = Trainer(model, seed=0, p_uncond=P_UNCOND)
    v0 = float(evaluate_loss(model, Z, 512, seed=1, labels=y)["loss"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = tr.fit(Z, batch_size=BATCH, max_epochs=EPOCHS, labels=y)["train_loss"]
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    model.eval()
    result = {"what": "per class and guidance scale: time-domain sliced Wasserstein distance of 1024 labelled samples to that "
                      "class's series, and the share of samples whose nearest training series is of the requested family",
              "model": "ClassConditionalScoreModule d_model=60 n_head=12 num_layers=3 dim_feedforward=2048 n_classes=4, VP",
              "training": {"epochs": EPOCHS, "batch_size": BATCH, "steps": steps, "lr_max": LR_MAX, "p_uncond": P_UNCOND,
                           "seed": 0, "train_seconds": seconds, "ms_per_step": 1e3 * seconds / steps,
                           "loss_fixed_draws_before": v0,
                           "loss_fixed_draws_after": float(evaluate_loss(model, Z, 512, seed=1, labels=y)["loss"]),
                           "loss_fixed_draws_after_null_labels": float(evaluate_loss(model, Z, 512, seed=1)["loss"]),
                           "train_loss_first_epoch": float(hist[:64].mean()), "train_loss_last_epoch": float(hist[-64:].mean())},
              "sampler": {"solver": "euler_maruyama", "steps": STEPS, "rng": "philox", "seed": 1, "samples_per_class": PER_CLASS},
              "class_sizes": [int((fam == k).sum()) for k in range(N_FAM)], "classes": {}}
    # floors and the exact class-conditional score
    for k in range(N_FAM):
        Zk = Z.cpu()[fam == k]
        rows = []
        for seed in SQ.SEEDS:
            g = torch.Generator().manual_seed(seed)
            pick = torch.randint(0, len(Zk), (PER_CLASS,), generator=g)
            rows.append(distance(k, to_time(Zk[pick] + SQ.BANDWIDTH * torch.randn(PER_CLASS, SQ.L, SQ.CH, generator=g))))
        exact = MixtureScoreModule.from_data(Zk, SQ.scheduler("vp"), bandwidth=SQ.BANDWIDTH).cuda().eval()
        xs = to_time(DiffusionSampler(exact, PER_CLASS, rng="philox", seed=1).sample(PER_CLASS, STEPS))
        result["classes"][str(k)] = {"floor_exact_draws": {"mean": float(np.mean(rows)), "min": min(rows), "max": max(rows)},
                                     "exact_class_conditional_score": {KEY: distance(k, xs),
                                                                       "nearest_series_in_family": nearest_share(k, xs)},
                                     "trained": {}}
        print("class", k, result["classes"][str(k)], flush=True)
    labels = torch.arange(N_FAM).repeat_interleave(PER_CLASS)
    sampler = DiffusionSampler(model, N_FAM * PER_CLASS, rng="philox", seed=1)
    for gscale in SCALES:
        t0 = time.perf_counter()
        xs = to_time(sampler.sample(N_FAM * PER_CLASS, STEPS, labels=labels, guidance_scale=gscale))
        torch.cuda.synchronize()
        took = time.perf_counter() - t0
        for k in range(N_FAM):
            part = xs[k * PER_CLASS:(k + 1) * PER_CLASS]
            row = {KEY: distance(k, part), "nearest_series_in_family": nearest_share(k, part),
                   "sample_std_over_class_std": float(part.std(0).mean() / X[fam_dev == k].std(0).mean())}
            result["classes"][str(k)]["trained"][f"g={gscale}"] = row
            print("g", gscale, "class", k, row, flush=True)
        result["sampler"][f"seconds_g={gscale}"] = took
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "class_quality.json"))
