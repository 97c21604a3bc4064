"""Cost of one interval of each solver of the fused sampling loop.

    python3 tools/solver_bench.py [out.json] [--solvers euler_maruyama,ode_euler,ode_heun]
                                             (default: profiles/solver_steps.json, all three)
    python3 tools/solver_bench.py pc [out.json]
                                             (predictor-corrector: euler_maruyama, pc1, pc2, pc1_sample ->
                                             profiles/pc_steps.json)
    python3 tools/solver_bench.py cond [out.json] [--alongside extra.json]
                                             (conditional sampling: euler_maruyama, cond0, pc1, cond1 ->
                                             profiles/cond_steps.json)
    python3 tools/solver_bench.py resample [out.json] [--alongside extra.json]
                                             (resampled conditional sampling: cond0, res0_j2, res0_j10, cond1, res1_j2 ->
                                             profiles/resample_steps.json)
    python3 tools/solver_bench.py multistep [out.json] [--alongside extra.json]
                                             (linear multistep ODE solvers: euler_maruyama, ode_euler, ode_ab2, dpmpp_2m ->
                                             profiles/multistep_steps.json)

ECG (L 187, C 1, d 72, 10 layers) at B = 512 on a 21-point grid: 20 intervals for the ODE solvers
(ffd_sample_batch_ode), the grid's first 20 steps for Euler-Maruyama (ffd_sample_batch, Philox noise on the device).
One untimed trajectory per solver warms every shape; then 3 repetitions, the solvers alternating inside each so that a
drift of the clocks shows as spread instead of as a difference.  A repetition times TRAJ trajectories of 20 intervals
from a fresh prior draw between two device synchronisations and reports milliseconds per interval and per-sample score
evaluations per second (Heun evaluates the network twice per interval).  What the numbers do NOT say: how many
intervals a solver needs for a given sample quality -- that needs a trained checkpoint.

``pc``: ffd_sample_batch_pc on the same grid with 1 and 2 Langevin corrector steps per reverse step (batch norm; pc1_sample:
1 step, sample norm), Euler-Maruyama measured in the same run.  A corrector step is one more score evaluation plus
the corrector's three (batch norm: four) small launches, so pcN is expected near (1 + N) Euler-Maruyama steps.

``cond``: ffd_sample_batch_cond in the frequency domain (one observed series shared by the batch, a prefix mask, the
dataset's std) with 0 and 1 corrector steps, next to the same steps without conditioning: condN adds one
k_cond_project launch behind each of its N + 1 updates; ``cost_vs_unconditional`` is cond0 / euler_maruyama and
cond1 / pc1.

``multistep``: ode_ab2 and dpmpp_2m (one tail kernel, one score evaluation per interval, the previous interval's history
read and written beside x) next to ode_euler and Euler-Maruyama in the same run; ``cost_vs_ode_euler_interval`` is the
acceptance figure, expected near 1.00.

``resample``: ffd_sample_batch_resample with resample = 2 over the whole 21-point grid (U = 42 visits; jump 2: 11
transitions, jump 10: 3) next to ffd_sample_batch_cond's steps in the same process, the same observation.  A visit is a
conditional step, so ``cost_vs_conditional_step`` (ms per visit / ms per step of the twin) is expected near 1.00 plus a
transition's share.  ``operator_us_per_launch``: ffd_forward_transition and ffd_cond_project on the loop's own (512, 187,
1) state, 400 back-to-back launches each between two events (device draws) -- launch spacing, not a kernel trace.

``--alongside FILE``: the JSON object in FILE goes into the result as ``measured_alongside``, unchanged -- what was
measured next to this run and is not this tool's to measure (the other runs of an alternating series, the parent
commit's figures, a kernel trace): profiles/cond_steps.json carries its comparison that way.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from fastfourierdiffusion_amd import _native as N  # noqa: E402

B, INTERVALS, REPS, TRAJ = 512, 20, 3, 5
EVALS = {"euler_maruyama": 1, "ode_euler": 1, "ode_heun": 2, "pc1": 2, "pc2": 3, "pc1_sample": 2, "cond0": 1, "cond1": 2,
         "ode_ab2": 1, "dpmpp_2m": 1, "res0_j2": 1, "res0_j10": 1, "res1_j2": 2}
PC = {"pc1": (1, N.FFD_LANGEVIN_NORM_BATCH), "pc2": (2, N.FFD_LANGEVIN_NORM_BATCH),
      "pc1_sample": (1, N.FFD_LANGEVIN_NORM_SAMPLE)}
COND = {"cond0": (0, "euler_maruyama"), "cond1": (1, "pc1")}  # corrector steps, the unconditional twin
RES = {"res0_j2": (0, 2, 2, "cond0"), "res0_j10": (0, 10, 2, "cond0"), "res1_j2": (1, 2, 2, "cond1")}  # correctors, jump, r
SNR = 0.16


def main() -> None:
    args = sys.argv[1:]
    solvers = ["euler_maruyama", "ode_euler", "ode_heun"]
    default_out = "solver_steps.json"
    if args and args[0] == "pc":
        solvers, default_out = ["euler_maruyama", "pc1", "pc2", "pc1_sample"], "pc_steps.json"
        del args[0]
    elif args and args[0] == "cond":
        solvers, default_out = ["euler_maruyama", "cond0", "pc1", "cond1"], "cond_steps.json"
        del args[0]
    elif args and args[0] == "resample":
        solvers, default_out = ["cond0", "res0_j2", "res0_j10", "cond1", "res1_j2"], "resample_steps.json"
        del args[0]
    elif args and args[0] == "multistep":
        solvers, default_out = ["euler_maruyama", "ode_euler", "ode_ab2", "dpmpp_2m"], "multistep_steps.json"
        del args[0]
    alongside = None
    if "--alongside" in args:  # a JSON object measured next to this run, carried into the result unchanged
        i = args.index("--alongside")
        with open(args[i + 1]) as f:
            alongside = json.load(f)
        del args[i:i + 2]
    if "--solvers" in args:
        i = args.index("--solvers")
        solvers = args[i + 1].split(",")
        del args[i:i + 2]
    assert all(s in EVALS for s in solvers), solvers
    out_path = args[0] if args else os.path.join(ROOT, "profiles", default_out)
    assert torch.cuda.is_available(), "solver_bench needs an MI355X"
    dev = torch.device("cuda", 0)
    model, sch, _ = bench.build_model(dev, "ecg")
    ctx = model._ctx()
    lib, hdl = ctx.lib, ctx.handle
    stream = N.current_stream_ptr(dev)
    n = INTERVALS + 1
    sch.set_timesteps(n)
    ts_c = (C.c_float * n)(*sch.timesteps.tolist())
    h = float(sch.step_size)
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    prior = DiffusionSampler(model, B, rng="philox", seed=42)
    cond = None
    if any(sv in COND or sv in RES for sv in solvers):  # one observed series for the batch, a prefix mask, a std table
        L, Cn = model.max_len, model.n_channels
        g = torch.Generator().manual_seed(7)
        obs = torch.randn((1, L, Cn), generator=g).to(dev)
        mask = torch.zeros((1, L, Cn), device=dev)
        mask[:, :100] = 1.0  # "complete this beat from its first 100 samples"
        std = (0.5 + 1.5 * torch.rand((L, Cn), generator=g)).to(dev)
        cond = N.CondCfg(obs.data_ptr(), mask.data_ptr(), std.data_ptr(), 1, N.FFD_COND_FREQUENCY, 1, 0)

    def trajectory(solver, X):
        if solver == "euler_maruyama":
            rc = lib.ffd_sample_batch(hdl, X.data_ptr(), B, ts_c, n, h, 0, INTERVALS, 42, 0, None, 0, 0, stream)
        elif solver in COND:
            rc = lib.ffd_sample_batch_cond(hdl, X.data_ptr(), B, ts_c, n, h, 0, INTERVALS, COND[solver][0], SNR,
                                           N.FFD_LANGEVIN_NORM_BATCH, 42, 0, None, 0, 0, C.byref(cond), stream)
        elif solver in RES:  # the whole schedule over the n-point grid
            n_corr, jump, r, _ = RES[solver]
            rc = lib.ffd_sample_batch_resample(hdl, X.data_ptr(), B, ts_c, n, h, 0, r * n, jump, r, n_corr, SNR,
                                               N.FFD_LANGEVIN_NORM_BATCH, 42, 0, None, C.byref(cond), stream)
        elif solver in PC:
            rc = lib.ffd_sample_batch_pc(hdl, X.data_ptr(), B, ts_c, n, h, 0, INTERVALS, PC[solver][0], SNR, PC[solver][1], 42,
                                         0, None, 0, 0, stream)
        else:
            code = {"ode_euler": N.FFD_SOLVER_ODE_EULER, "ode_heun": N.FFD_SOLVER_ODE_HEUN,
                    "ode_ab2": N.FFD_SOLVER_ODE_AB2, "dpmpp_2m": N.FFD_SOLVER_DPMPP_2M}[solver]
            rc = lib.ffd_sample_batch_ode(hdl, X.data_ptr(), B, ts_c, n, h, 0, INTERVALS, code, 0, 0, stream)
        N.check(rc, hdl, solver)

    def timed(solver):
        X = prior.sample_prior(B)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(TRAJ):
            trajectory(solver, X)
        torch.cuda.synchronize(dev)
        assert torch.isfinite(X).all(), solver
        return (time.perf_counter() - t0) * 1e3 / (TRAJ * (RES[solver][2] * n if solver in RES else INTERVALS))

    for s in solvers:
        timed(s)  # warm-up
    reps = {s: [] for s in solvers}
    for _ in range(REPS):
        for s in solvers:
            reps[s].append(timed(s))
    res = {"device": torch.cuda.get_device_name(0), "workload": "ecg", "batch": B, "intervals": INTERVALS,
           "repetitions": REPS, "trajectories_per_repetition": TRAJ, "solvers": {}}
    for s in solvers:
        ms = sorted(reps[s])[len(reps[s]) // 2]
        res["solvers"][s] = {"ms_per_interval": round(ms, 4), "ms_per_interval_repetitions": [round(v, 4) for v in reps[s]],
                             "score_evaluations_per_interval": EVALS[s],
                             "sample_score_evaluations_per_s": round(EVALS[s] * B / (ms * 1e-3), 1)}
    if "euler_maruyama" in solvers:
        em = res["solvers"]["euler_maruyama"]["ms_per_interval"]
        for s in solvers:
            res["solvers"][s]["cost_vs_euler_maruyama_step"] = round(res["solvers"][s]["ms_per_interval"] / em, 4)
    if "ode_euler" in solvers:
        oe = res["solvers"]["ode_euler"]["ms_per_interval"]
        for s in ("ode_ab2", "dpmpp_2m"):
            if s in solvers:
                res["solvers"][s]["cost_vs_ode_euler_interval"] = round(res["solvers"][s]["ms_per_interval"] / oe, 4)
    for s, (_, twin) in COND.items():
        if s in solvers and twin in solvers:
            res["solvers"][s]["cost_vs_unconditional"] = round(res["solvers"][s]["ms_per_interval"] /
                                                               res["solvers"][twin]["ms_per_interval"], 4)
    for s, (n_corr, jump, r, twin) in RES.items():
        if s in solvers and twin in solvers:
            res["solvers"][s].update(visits=r * n, transitions=(r - 1) * -(-n // jump), jump=jump, resample=r,
                                     cost_vs_conditional_step=round(res["solvers"][s]["ms_per_interval"] /
                                                                    res["solvers"][twin]["ms_per_interval"], 4))
    if any(s in RES for s in solvers):  # the two operators alone, on the loop's state shape
        L, Cn = model.max_len, model.n_channels
        X = prior.sample_prior(B)
        desc, G = sch._desc(), sch._G_on(dev)

        def launches(fn, count=400):
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            return round(e0.elapsed_time(e1) * 1e3 / count, 3)

        res["operator_us_per_launch"] = {
            "note": "back-to-back launches between two events, device draws, (512, 187, 1): launch spacing, not a kernel trace",
            "ffd_forward_transition": launches(lambda: N.check(lib.ffd_forward_transition(
                C.byref(desc), X.data_ptr(), G.data_ptr(), 0.25, 0.5, None, 42, 0, 0xE0000000, B, L, Cn, stream), None, "transition")),
            "ffd_cond_project": launches(lambda: N.check(lib.ffd_cond_project(
                C.byref(desc), X.data_ptr(), obs.data_ptr(), mask.data_ptr(), std.data_ptr(), G.data_ptr(), 0.5, 0, None, 42, 0,
                0xC0000000, 1, N.FFD_COND_FREQUENCY, B, L, Cn, stream), None, "project"))}
    if alongside is not None:
        res["measured_alongside"] = alongside
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
