"""How far conditional sampling by replacement is from the true conditional, where the true conditional is known.

    python3 tools/imputation_quality.py [out.json]            (default: profiles/imputation_quality.json)
    python3 tools/imputation_quality.py --guided-only [out.json]   the guided rows alone, merged into the file's other rows

The synthetic set of tools/solver_quality.py (4096 series, L = 187, C = 1, four families of sinusoid sums) defines a
Gaussian mixture in the TIME domain: ``MixtureScoreModule.from_data`` with a bandwidth, no Fourier noise scaling, so the
diffused score is exact (ffd_mixture_score) and so is the conditional of the unobserved points given the observed ones:
with y the observed values, the posterior weight of component i is log r_i = log w_i - 1/2 sum_observed (y - mu_i)^2 / v,
and given the component the unobserved points are mu_i + sqrt(v) z.

Two sets of N_HELD truths: series of a second seed of the same generator (held out: they are NOT draws of the mixture,
whose components are narrow beside the distance between two series, so against them the exact conditional is no lower
bound -- it is the model's own overconfidence that is scored) and draws of the mixture itself (a training series plus
bandwidth noise: here the exact conditional is the true one and its score is the floor).  For a prefix mask (a forecast:
the first half observed) and a random 50 % mask (an imputation), M completions of every truth are drawn
  (a) by ``sample_conditional`` (replacement, domain="time") at several step counts, without and with one Langevin
      corrector step per reverse step, Philox draws, three seeds;
  (a') by ``sample_conditional(..., resample=r, jump=j)`` (resampling, "time travel") without corrector at EQUAL SCORE
      EVALUATIONS as rows of (a): 20 steps x r = 10 and 50 x 4 against the 200-evaluation rows, 200 x 5 against the
      1000-evaluation row, each with jump 1, 2 and 10;
  (a'') by ``sample_conditional(..., guidance=Guidance(scale, obs_var = bandwidth^2, rho = 1, replace))`` (reconstruction
      guidance through the score's closed-form Jacobian) without corrector: 50 / 200 / 1000 steps at scale 1, scale 0.5 and
      2 at 200 steps, each with and without the replacement behind the step, the same seeds; a guided step is one score
      evaluation and one vector-Jacobian product;
  (b) from the exact conditional, three seeds: the FLOOR, its spread the resolution of the comparison,
and scored against the truth with ``ensemble_scores``: the mean CRPS over the unobserved points and the energy score,
averaged over the truths, and the share of unobserved truths inside the 5 % .. 95 % band.  Replacement is known to be an
approximation when observed and unobserved parts are dependent (here they are: the families differ in level and
frequency); the table says by how much on this data."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from solver_quality import CH, L, dataset  # noqa: E402

BANDWIDTH = 0.1
N_HELD, M = 32, 256
STEPS = (20, 50, 200, 1000)
SEEDS = (1, 2, 3)
SNR = 0.16
RESAMPLED = ((20, 10), (50, 4), (200, 5))  # (steps, resample): 200, 200 and 1000 score evaluations
JUMPS = (1, 2, 10)
GUIDED = ((50, 1.0), (200, 1.0), (1000, 1.0), (200, 0.5), (200, 2.0))  # (steps, scale)


def masks():
    prefix = torch.zeros(L)
    prefix[: L // 2] = 1.0
    g = torch.Generator().manual_seed(7)
    rand = torch.zeros(L)
    rand[torch.randperm(L, generator=g)[: L // 2]] = 1.0
    return {"prefix_forecast": prefix, "random_half_imputation": rand}


def exact_conditional(train, held, mask, seed):
    """(N_HELD, M, L, C) draws of the mixture's conditional given the held-out series on the mask (uniform weights)."""
    g = torch.Generator().manual_seed(seed)
    mu = train.double().reshape(train.shape[0], -1)         # (K, D)
    y = held.double().reshape(held.shape[0], -1)            # (S, D)
    obs = mask.repeat_interleave(CH).bool()
    d2 = ((y[:, None, obs] - mu[None, :, obs]) ** 2).sum(-1)  # (S, K)
    logr = -0.5 * d2 / BANDWIDTH ** 2
    r = torch.softmax(logr, dim=1)
    pick = torch.multinomial(r, M, replacement=True, generator=g)  # (S, M)
    draws = mu[pick] + BANDWIDTH * torch.randn(held.shape[0], M, mu.shape[1], generator=g, dtype=torch.float64)
    draws[:, :, obs] = y[:, None, obs]
    return draws.float().reshape(held.shape[0], M, L, CH), r


def spread(rows):
    return {k: {"mean": float(np.mean([r[k] for r in rows])), "min": float(min(r[k] for r in rows)),
                "max": float(max(r[k] for r in rows))} for k in rows[0]}


def main(out_path, guided_only=False):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule
    from fastfourierdiffusion_amd.sampling import Guidance, ensemble_scores
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    train = dataset(0)
    g = torch.Generator().manual_seed(11)
    truths = {"held_out_series": dataset(1)[:N_HELD],
              "mixture_draws": train[torch.randint(0, train.shape[0], (N_HELD,), generator=g)] +
              BANDWIDTH * torch.randn(N_HELD, L, CH, generator=g)}
    sch = VPScheduler(fourier_noise_scaling=False)
    sch.set_noise_scaling(L)
    model = MixtureScoreModule.from_data(train, sch, bandwidth=BANDWIDTH, fourier_noise_scaling=False).cuda().eval()

    def score(ens, held, mask):
        out = ensemble_scores(ens, held, mask=mask, quantiles=(0.05, 0.5, 0.95))
        lo, hi = out["quantiles"][0], out["quantiles"][2]
        scored = (1.0 - mask)[None, :, None].expand_as(held).bool()
        inside = ((held.double() >= lo) & (held.double() <= hi))[scored].double().mean()
        return {"crps_mean": float(out["crps_mean"].mean()), "energy_score": float(out["energy_score"].mean()),
                "coverage_90": float(inside)}

    result = {"what": "mean over the truths of crps_mean (unobserved points) and energy_score of M completions "
                      "per series, and the share of unobserved truths inside the 5 % .. 95 % band; mean / min / max over "
                      "three seeds.  floor: draws of the exact conditional; replacement: sample_conditional, domain time",
              "L": L, "C": CH, "n_components": int(train.shape[0]), "bandwidth": BANDWIDTH, "sde": "vp", "n_held_out": N_HELD,
              "members": M, "steps": list(STEPS), "seeds": list(SEEDS), "snr": SNR,
              "resampled": "sample_conditional(resample=r, jump=j), no corrector: steps x r score evaluations",
              "resampled_steps_r": [list(v) for v in RESAMPLED], "jumps": list(JUMPS), "truths": {}}
    if guided_only:  # every other row stays what the file holds
        with open(out_path) as f:
            result = json.load(f)
    result["guided"] = ("sample_conditional(guidance=Guidance(scale, obs_var=bandwidth^2, rho=1, replace)), no corrector: "
                        "one score evaluation and one vector-Jacobian product per step")
    result["guided_steps_scale"] = [list(v) for v in GUIDED]
    for kind, name, mask in [(k, n, mk) for k in truths for n, mk in masks().items()]:
        held = truths[kind]
        observed = held[:, None].expand(N_HELD, M, L, CH).reshape(N_HELD * M, L, CH).contiguous()
        guided = {}
        for replace in (False, True):
            table = {}
            for steps, scale in GUIDED:
                rows = []
                for seed in SEEDS:
                    s = DiffusionSampler(score_model=model, sample_batch_size=N_HELD * M, rng="philox", seed=seed)
                    out = s.sample_conditional(observed, mask, N_HELD * M, steps, domain="time", final_replace=True,
                                               guidance=Guidance(scale, BANDWIDTH ** 2, 1.0, replace))
                    rows.append(score(out.reshape(N_HELD, M, L, CH), held, mask))
                table[f"steps_{steps}_scale_{scale:g}"] = {"score_evaluations": steps, "vjps": steps, **spread(rows)}
                print(kind, name, f"guided replace={replace} steps={steps} scale={scale:g}",
                      {k: round(v["mean"], 5) for k, v in table[f"steps_{steps}_scale_{scale:g}"].items() if isinstance(v, dict)},
                      flush=True)
            guided[f"replace_{int(replace)}"] = table
        if guided_only:
            result["truths"][kind][name]["guided"] = guided
            continue
        floor_rows, ess = [], None
        for seed in SEEDS:
            draws, r = exact_conditional(train, held, mask, seed)
            floor_rows.append(score(draws, held, mask))
            ess = float((1.0 / (r * r).sum(1)).mean())
        entry = {"observed_points": int(mask.sum()), "posterior_effective_components_mean": ess,
                 "floor": spread(floor_rows), "replacement": {}}
        print(kind, name, "floor", {k: round(v["mean"], 5) for k, v in entry["floor"].items()}, flush=True)
        for n_corr in (0, 1):
            table = {}
            for steps in STEPS:
                rows = []
                for seed in SEEDS:
                    s = DiffusionSampler(score_model=model, sample_batch_size=N_HELD * M, rng="philox", seed=seed,
                                         corrector_steps=n_corr, snr=SNR)
                    out = s.sample_conditional(observed, mask, N_HELD * M, steps, domain="time", final_replace=True)
                    rows.append(score(out.reshape(N_HELD, M, L, CH), held, mask))
                table[str(steps)] = {"score_evaluations": steps * (n_corr + 1), **spread(rows)}
                print(kind, name, f"corrector_steps={n_corr}", steps,
                      {k: round(v["mean"], 5) for k, v in table[str(steps)].items() if isinstance(v, dict)}, flush=True)
            entry["replacement"][f"corrector_steps_{n_corr}"] = table
        entry["resampled"] = {}
        for steps, r in RESAMPLED:
            table = {}
            for jump in JUMPS:
                rows = []
                for seed in SEEDS:
                    s = DiffusionSampler(score_model=model, sample_batch_size=N_HELD * M, rng="philox", seed=seed)
                    out = s.sample_conditional(observed, mask, N_HELD * M, steps, resample=r, jump=jump, domain="time",
                                               final_replace=True)
                    rows.append(score(out.reshape(N_HELD, M, L, CH), held, mask))
                table[f"jump_{jump}"] = {"score_evaluations": steps * r, **spread(rows)}
                print(kind, name, f"resampled steps={steps} r={r} jump={jump}",
                      {k: round(v["mean"], 5) for k, v in table[f"jump_{jump}"].items() if isinstance(v, dict)}, flush=True)
            entry["resampled"][f"steps_{steps}_r_{r}"] = table
        entry["guided"] = guided
        result["truths"].setdefault(kind, {})[name] = entry
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--guided-only"]
    main(argv[0] if argv else os.path.join(ROOT, "profiles", "imputation_quality.json"), "--guided-only" in sys.argv[1:])
