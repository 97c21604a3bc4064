"""Cost and accuracy of the log-likelihood through the probability-flow ODE (ffd_loglik_batch).

    python3 tools/loglik_bench.py [out.json] [--only cost,accuracy,fd_rel]      (default: profiles/loglik.json, all three)

``cost``: ECG (L 187, C 1, d 72, 10 layers) at B = 512 on a 21-point grid.  Milliseconds per Heun interval of the
likelihood at n_probes 1 and 4 -- every divergence evaluation is one forward at (1 + 2 n_probes) B rows -- next to an
``ode_heun`` SAMPLING interval (ffd_sample_batch_ode) measured in the same process, the runs alternating; one untimed
trajectory each warms the shapes.  ``operator_us_per_launch``: ffd_loglik_perturb, ffd_loglik_tail and ffd_prior_logp
alone on the loop's state shape, back-to-back launches between two events (launch spacing, not a kernel trace).

``accuracy``: on the mode mixture of tests/mixture_restatement.py (L 8) and on a ``from_data`` mixture of 64 synthetic
series at L = 187 (bandwidth 0.1), 16 points of the eps = 1e-3 marginal: max |delta - (log p_eps(x_eps) - log p_1(x_1))|
against the closed form ``log_pt`` at 25 .. 400 intervals, Euler and Heun, exact-trace probes (eps_j = sqrt(D) e_j); and
the rms deviation of Hutchinson's estimate (device Rademacher probes) from the exact-trace run at n_probes 1, 4, 16,
100 Heun intervals.

``fd_rel``: the finite-difference step swept over 1e-1 .. 1e-4, Heun, the same injected probes on both sides.
``rounding`` = device against the float64 restatement at the SAME fd_rel (what fp32 costs); ``truncation`` = that
float64 restatement against the exact divergence (mixture: the closed-form trace) or against the float64 restatement at
fd_rel = 1e-6 (networks: the float64 judges of tests/transformer_restatement.py / tests/lstm_restatement.py, random
weights, 8 intervals).  The default fd_rel is the one where neither dominates.
"""
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import loglik_restatement as LL  # noqa: E402
import lstm_restatement as LS  # noqa: E402
import mixture_restatement as M  # noqa: E402
import ode_restatement as R  # noqa: E402
import transformer_restatement as TR  # noqa: E402
from fastfourierdiffusion_amd import _native as N  # noqa: E402
from fastfourierdiffusion_amd.utils import synthetic  # noqa: E402
from oracle import ffd_oracle as O  # noqa: E402

EPS = 1e-3
HEUN, EULER = N.FFD_SOLVER_ODE_HEUN, N.FFD_SOLVER_ODE_EULER
NET_VE = dict(sigma_min=0.01, sigma_max=5.0)  # random weights: the standard sigma_max = 50 blows an 8-interval walk up


def dev_f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def scheduler(sde, L, kw=None):
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    sch = (VPScheduler if sde == "vp" else VEScheduler)(fourier_noise_scaling=True, eps=EPS, **(kw or M.sde_kwargs(sde)))
    sch.set_noise_scaling(L)
    return sch


def walk(model, x0, n, solver, k, fd_rel, probes=None, seed=0, dev=None):
    """(latent, delta) of ffd_loglik_batch over the n intervals of linspace(1, EPS, n + 1).  probes (2 | 1, k, B, L, C):
    ONE interval's injected set, reused for every interval (the entry is called interval by interval)."""
    ctx = model._ctx()
    stream = N.current_stream_ptr(dev)
    ts, _ = R.grid(n + 1, EPS)
    ts_c = (C.c_float * (n + 1))(*[float(t) for t in ts])
    x = dev_f32(x0, dev)
    delta = torch.zeros(x.shape[0], dtype=torch.float64, device=dev)
    if probes is None:
        N.check(ctx.lib.ffd_loglik_batch(ctx.handle, x.data_ptr(), delta.data_ptr(), x.shape[0], ts_c, n + 1, 0, n, solver, k,
                                         fd_rel, None, seed, 0, stream), ctx.handle, "ffd_loglik_batch")
    else:
        for j in range(n):
            N.check(ctx.lib.ffd_loglik_batch(ctx.handle, x.data_ptr(), delta.data_ptr(), x.shape[0], ts_c, n + 1, j, 1, solver,
                                             k, fd_rel, probes.data_ptr(), 0, 0, stream), ctx.handle, "ffd_loglik_batch")
    return x.cpu().numpy(), delta.cpu().numpy()


# ------------------------------------------------------------------ cost ----
def cost(dev):
    B, INTERVALS, REPS, TRAJ = 512, 20, 3, 2
    model, sch, _ = bench.build_model(dev, "ecg")
    ctx = model._ctx()
    lib, hdl = ctx.lib, ctx.handle
    stream = N.current_stream_ptr(dev)
    n = INTERVALS + 1
    sch.set_timesteps(n)
    ts_c = (C.c_float * n)(*sch.timesteps.tolist())
    L, Cn = model.max_len, model.n_channels
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    prior = DiffusionSampler(model, B, rng="philox", seed=42)
    delta = torch.zeros(B, dtype=torch.float64, device=dev)

    def trajectory(name, X):
        if name == "ode_heun_sampling":
            rc = lib.ffd_sample_batch_ode(hdl, X.data_ptr(), B, ts_c, n, float(sch.step_size), 0, INTERVALS, HEUN, 0, 0, stream)
        else:
            rc = lib.ffd_loglik_batch(hdl, X.data_ptr(), delta.data_ptr(), B, ts_c, n, 0, INTERVALS, HEUN, int(name[-1]), 1e-2,
                                      None, 42, 0, stream)
        N.check(rc, hdl, name)

    def timed(name):
        ms = []
        for _ in range(TRAJ):  # a fresh state per trajectory: a sampling run starts at the prior, a likelihood at data scale
            X = prior.sample_prior(B) if name == "ode_heun_sampling" else 0.5 * torch.randn((B, L, Cn), device=dev)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            trajectory(name, X)
            torch.cuda.synchronize(dev)
            ms.append((time.perf_counter() - t0) * 1e3 / INTERVALS)
        return sum(ms) / len(ms)

    names = ["ode_heun_sampling", "loglik_heun_k1", "loglik_heun_k4"]
    for s in names:
        timed(s)
    reps = {s: [] for s in names}
    for _ in range(REPS):
        for s in names:
            reps[s].append(timed(s))
    res = {"workload": "ecg", "batch": B, "intervals": INTERVALS, "repetitions": REPS, "trajectories_per_repetition": TRAJ,
           "runs": {}}
    for s in names:
        ms = sorted(reps[s])[len(reps[s]) // 2]
        k = 0 if s == "ode_heun_sampling" else int(s[-1])
        res["runs"][s] = {"ms_per_interval": round(ms, 4), "ms_per_interval_repetitions": [round(v, 4) for v in reps[s]],
                          "rows_per_evaluation": (1 + 2 * k) * B}
    base = res["runs"]["ode_heun_sampling"]["ms_per_interval"]
    for s in names[1:]:
        res["runs"][s]["cost_vs_sampling_interval"] = round(res["runs"][s]["ms_per_interval"] / base, 4)
    # where it goes: the forward's kernel classes and the likelihood's own launches, timed in situ over one trajectory
    for s in names[1:]:
        X = 0.5 * torch.randn((B, L, Cn), device=dev)
        N.check(lib.ffd_kernel_timing_begin(hdl, 0xFF, 20000), hdl, "timing_begin")
        trajectory(s, X)
        N.check(lib.ffd_kernel_timing_end(hdl), hdl, "timing_end")
        by = {}
        ms_, cnt = C.c_float(), C.c_int()
        for cls, key in ((N.K_FFN, "ffn"), (N.K_ATTN, "attention"), (N.K_OUTPROJ, "out_projection"), (N.K_EMBED, "embed"),
                         (N.K_UNEMBED, "unembed"), (N.K_SDE, "perturb_and_tail")):
            lib.ffd_kernel_timing_get(hdl, cls, C.byref(ms_), C.byref(cnt))
            if cnt.value:
                by[key] = {"launches": cnt.value, "ms_per_interval": round(ms_.value * cnt.value / INTERVALS, 4)}
        res["runs"][s]["kernel_ms_per_interval"] = by
    # the operators alone
    desc, G = sch._desc(), sch._G_on(dev)
    x = 0.5 * torch.randn((B, L, Cn), device=dev)
    xp, d1 = torch.empty_like(x), torch.empty_like(x)
    v1 = torch.zeros(B, dtype=torch.float64, device=dev)
    out = torch.zeros(B, dtype=torch.float64, device=dev)

    def launches(fn, count=200):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return round(e0.elapsed_time(e1) * 1e3 / count, 3)

    ops = {"note": "back-to-back launches between two events, device probes, state (512, 187, 1): launch spacing, not a trace"}
    for k in (1, 4):
        stack = torch.zeros((1 + 2 * k, B, L, Cn), device=dev)
        ops[f"ffd_loglik_perturb_k{k}"] = launches(lambda: N.check(lib.ffd_loglik_perturb(
            x.data_ptr(), G.data_ptr(), 1e-3, k, None, 42, 0, 0xF0000000, stack.data_ptr(), B, L, Cn, stream), None, "perturb"))
        ops[f"ffd_loglik_tail_predict_k{k}"] = launches(lambda: N.check(lib.ffd_loglik_tail(
            C.byref(desc), N.FFD_LOGLIK_PREDICT, x.data_ptr(), xp.data_ptr(), d1.data_ptr(), stack.data_ptr(), G.data_ptr(), 0.5,
            0.05, 1e-3, k, None, 42, 0, 0xF0000000, delta.data_ptr(), v1.data_ptr(), None, B, L, Cn, stream), None, "tail"))
    ops["ffd_prior_logp"] = launches(lambda: N.check(lib.ffd_prior_logp(C.byref(desc), x.data_ptr(), G.data_ptr(), out.data_ptr(),
                                                                        B, L, Cn, stream), None, "prior"))
    res["operator_us_per_launch"] = ops
    return res


# ------------------------------------------------------------------ accuracy ----
def mixtures():
    """name -> (means, log-weights, variance, points per run)"""
    L = 187
    rng = np.random.default_rng(8)
    tg = np.linspace(0.0, 1.0, L)[None, :, None]
    data = (np.sin(2 * np.pi * (tg * rng.uniform(1.0, 3.0, (64, 1, 1)) + rng.uniform(0, 1, (64, 1, 1))))
            + 0.05 * rng.standard_normal((64, L, 1))).astype(np.float32)
    return {"mode_L8": M.mode_mixture() + (256,),
            "from_data_L187": (data, np.full(64, -math.log(64.0), np.float32), np.full((L, 1), 0.01, np.float32), 64)}


def mixture_model(sde, mu, lw, var, dev):
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule

    sch = scheduler(sde, mu.shape[1])
    m = MixtureScoreModule(n_channels=mu.shape[2], max_len=mu.shape[1], noise_scheduler=sch, means=torch.from_numpy(mu),
                           log_weights=torch.from_numpy(lw), variance=torch.from_numpy(var))
    return m.to(dev).eval(), sch


def accuracy(dev):
    res = {"eps": EPS, "points": 16, "probes": "exact trace: eps_j = sqrt(D) e_j, n_probes = D"}
    for name, (mu, lw, var, n_hutch) in mixtures().items():
        L = mu.shape[1]
        G = M.fourier_G(L)
        for sde in ("vp", "ve"):
            kw = M.sde_kwargs(sde)
            model, _ = mixture_model(sde, mu, lw, var, dev)
            x0 = LL.eps_marginal_points(sde, kw, mu, lw, var, G, EPS, 16, 2)
            lp0 = M.log_pt(sde, kw, x0, EPS, mu, lw, var, G)
            pr = LL.exact_probes(16, L, 1)
            both = dev_f32(np.stack([pr, pr]), dev)
            row = {}
            for solver, code in (("ode_euler", EULER), ("ode_heun", HEUN)):
                row[solver] = {}
                for n in (25, 50, 100, 200, 400):
                    xT, d = walk(model, x0, n, code, L, 1e-2, both, dev=dev)
                    row[solver][str(n)] = float(np.abs(d - (lp0 - M.log_pt(sde, kw, xT, 1.0, mu, lw, var, G))).max())
            xh = LL.eps_marginal_points(sde, kw, mu, lw, var, G, EPS, n_hutch, 2)
            prh = LL.exact_probes(n_hutch, L, 1)
            _, exact = walk(model, xh, 100, HEUN, L, 1e-2, dev_f32(np.stack([prh, prh]), dev), dev=dev)
            hutch = {}
            for k in (1, 4, 16):
                _, d = walk(model, xh, 100, HEUN, k, 1e-2, None, seed=11, dev=dev)
                dv = d - exact
                hutch[str(k)] = {"rms_nats": round(float(np.sqrt((dv ** 2).mean())), 4),
                                 "mean_in_standard_errors": round(float(dv.mean() / (dv.std(ddof=1) / math.sqrt(n_hutch))), 2)}
            row["hutchinson_100_heun_intervals"] = {"points": n_hutch, "n_probes": hutch}
            res[f"{name}_{sde}"] = row
    return res


# ------------------------------------------------------------------ the fd_rel sweep ----
NETS = {"transformer_L20_C3_d16": dict(kind="transformer", d=16, H=4, NL=2, L=20, C=3, B=3),
        "lstm_L20_C3_d16": dict(kind="lstm", d=16, H=1, NL=2, L=20, C=3, B=3)}


def network(c, sde, dev):
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, ScoreModule

    kw = M.VP if sde == "vp" else NET_VE
    sch = scheduler(sde, c["L"], kw)
    common = dict(n_channels=c["C"], max_len=c["L"], noise_scheduler=sch, d_model=c["d"], num_layers=c["NL"])
    if c["kind"] == "lstm":
        m = LSTMScoreModule(fourier_noise_scaling=True, **common)
        sd = synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=146)
    else:
        m = ScoreModule(fourier_noise_scaling=True, n_head=c["H"], **common)
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=142)
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)

    def judge(x, t, k=0):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        tt = torch.full((xt.shape[0],), t, dtype=torch.float32)
        if c["kind"] == "lstm":
            return LS.lstm_score_forward64(xt, tt, sd, c["NL"])[0].numpy()
        return TR.score_forward64(xt, tt, sd, c["NL"], c["H"]).numpy()

    return m.to(dev).eval(), kw, judge


def fd_sweep(dev):
    rels = (1e-1, 1e-2, 1e-3, 1e-4)
    res = {"fd_rel": list(rels), "note": "max over the points, nats; rounding: device against the float64 restatement at the "
           "same fd_rel and probes; truncation: that restatement against the exact divergence (networks: against fd_rel = 1e-6)"}
    mu, lw, var = M.mode_mixture()
    L = mu.shape[1]
    G = M.fourier_G(L)
    for sde in ("vp", "ve"):
        kw = M.sde_kwargs(sde)
        model, _ = mixture_model(sde, mu, lw, var, dev)
        x0 = LL.eps_marginal_points(sde, kw, mu, lw, var, G, EPS, 16, 2)
        pr = LL.exact_probes(16, L, 1)
        both = dev_f32(np.stack([pr, pr]), dev)
        fn = M.score_fn(sde, kw, mu, lw, var, G)
        ts, _ = R.grid(101, EPS)
        _, exact = LL.integrate_exact("ode_heun", sde, kw, x0, fn, lambda x, t: LL.mixture_trace(sde, kw, x, t, mu, lw, var, G),
                                      ts, G)
        row = {"intervals": 100, "rounding": [], "truncation": []}
        for rel in rels:
            _, d = walk(model, x0, 100, HEUN, L, rel, both, dev=dev)
            _, d64 = LL.integrate("ode_heun", sde, kw, x0, fn, ts, G, n_probes=L, fd_rel=rel, probes=lambda e: pr)
            row["rounding"].append(float(np.abs(d - d64).max()))
            row["truncation"].append(float(np.abs(d64 - exact).max()))
        res[f"mixture_mode_L8_{sde}"] = row
    for name, c in NETS.items():
        for sde in ("vp", "ve"):
            model, kw, judge = network(c, sde, dev)
            B, L, Cn, n, k = c["B"], c["L"], c["C"], 8, 4
            rng = np.random.default_rng(len(name))
            x0 = rng.standard_normal((B, L, Cn)).astype(np.float32)
            pr = rng.choice([-1.0, 1.0], (2, k, B, L, Cn)).astype(np.float32)
            G = M.fourier_G(L)
            ts, _ = R.grid(n + 1, EPS)
            _, ref = LL.integrate("ode_heun", sde, kw, x0, judge, ts, G, n_probes=k, fd_rel=1e-6, probes=lambda e: pr[e % 2])
            row = {"intervals": n, "n_probes": k, "delta_scale": float(np.abs(ref).max()), "rounding": [], "truncation": []}
            for rel in rels:
                _, d = walk(model, x0, n, HEUN, k, rel, dev_f32(pr, dev), dev=dev)
                _, d64 = LL.integrate("ode_heun", sde, kw, x0, judge, ts, G, n_probes=k, fd_rel=rel, probes=lambda e: pr[e % 2])
                row["rounding"].append(float(np.abs(d - d64).max()))
                row["truncation"].append(float(np.abs(d64 - ref).max()))
            res[f"{name}_{sde}"] = row
    return res


def main() -> None:
    args = sys.argv[1:]
    only = ["cost", "accuracy", "fd_rel"]
    if "--only" in args:
        i = args.index("--only")
        only = args[i + 1].split(",")
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "loglik.json")
    assert torch.cuda.is_available(), "loglik_bench needs an MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    for key, fn in (("cost", cost), ("accuracy", accuracy), ("fd_rel", fd_sweep)):
        if key in only:
            t0 = time.perf_counter()
            res[key] = fn(dev)
            print(f"[loglik_bench] {key}: {time.perf_counter() - t0:.1f} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
