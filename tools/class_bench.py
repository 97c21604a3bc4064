"""Cost of class conditioning and classifier-free guidance in the fused sampling loop, and of a training step with classes.

    python3 tools/class_bench.py [out.json]            (default: profiles/class_steps.json)

Sampling.  The ECG transformer of bench.py (L 187, C 1, d 72, 10 layers) on a 21-point grid, the grid's first 20
Euler-Maruyama steps (ffd_sample_batch, Philox noise on the device), five classes, a random table and random labels.
One untimed trajectory per variant warms every shape; then 3 repetitions, the variants alternating inside each.  A
repetition times TRAJ trajectories between two device synchronisations; the figure is the median's milliseconds per step.

    plain_B256 / plain_B512 / plain_B1024   no class state
    g1_B512                                 the conditional score: one evaluation of B rows behind one table launch
    cfg_B512, cfg_B256                      g = 2: one evaluation at 2 B rows, the table + stack launch, the combine

``comparisons``: g1_B512 / plain_B512, cfg_B512 / plain_B1024, cfg_B256 / plain_B512, and plain_B512 against the parent
commit's Euler-Maruyama figure in profiles/solver_steps.json (measured by tools/solver_bench.py on another day: a ratio
inside a few 1e-3 of 1 is that file's own repetition spread).

``operator_us_per_launch``: the new launches alone on the loop's shapes, 400 back-to-back launches each between two
events -- launch spacing, not a kernel trace.  The stack copy of x shares the table's launch inside the loop and has no
entry of its own in the ABI: it is not measured separately.

Training.  The ECG transformer of tools/train_quality.py (d 60, 12 heads, 3 layers, dim_feedforward 2048) at B = 64 and
512: ``Trainer.step`` on Philox draws with and without classes (p_uncond 0.1), median of 3 repetitions of 30 steps.
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

INTERVALS, REPS, TRAJ, N_CLASSES = 20, 3, 5, 5
VARIANTS = {"plain_B256": (256, None), "plain_B512": (512, None), "plain_B1024": (1024, None), "g1_B512": (512, 1.0),
            "cfg_B512": (512, 2.0), "cfg_B256": (256, 2.0)}


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "class_steps.json")
    assert torch.cuda.is_available(), "class_bench needs an MI355X"
    dev = torch.device("cuda", 0)
    model, sch, _ = bench.build_model(dev, "ecg")
    ctx = model._ctx()
    lib, hdl = ctx.lib, ctx.handle
    stream = N.current_stream_ptr(dev)
    n = INTERVALS + 1
    sch.set_timesteps(n)
    ts_c = (C.c_float * n)(*sch.timesteps.tolist())
    h = float(sch.step_size)
    L, Cn, d = model.max_len, model.n_channels, model.d_model
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    gen = torch.Generator().manual_seed(7)
    table = (0.02 * torch.randn((N_CLASSES + 1, d), generator=gen)).to(dev)
    labels_host = torch.randint(0, N_CLASSES, (1024,), generator=gen, dtype=torch.int32)
    labels = labels_host.to(dev)
    priors = {B: DiffusionSampler(model, B, rng="philox", seed=42) for B in (256, 512, 1024)}

    def timed(name):
        B, g = VARIANTS[name]
        if g is None:
            N.check(lib.ffd_class_disable(hdl), hdl, "ffd_class_disable")
        else:
            cfg = N.ClassCfg(table.data_ptr(), labels.data_ptr(), labels_host.data_ptr(), N_CLASSES, B, g, 0)
            N.check(lib.ffd_class_enable(hdl, C.byref(cfg)), hdl, "ffd_class_enable")
        X = priors[B].sample_prior(B)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(TRAJ):
            N.check(lib.ffd_sample_batch(hdl, X.data_ptr(), B, ts_c, n, h, 0, INTERVALS, 42, 0, None, 0, 0, stream), hdl, name)
        torch.cuda.synchronize(dev)
        N.check(lib.ffd_class_disable(hdl), hdl, "ffd_class_disable")
        assert torch.isfinite(X).all(), name
        return (time.perf_counter() - t0) * 1e3 / (TRAJ * INTERVALS)

    for v in VARIANTS:
        timed(v)  # warm-up
    reps = {v: [] for v in VARIANTS}
    for _ in range(REPS):
        for v in VARIANTS:
            reps[v].append(timed(v))
    res = {"device": torch.cuda.get_device_name(0), "workload": "ecg", "intervals": INTERVALS, "repetitions": REPS,
           "trajectories_per_repetition": TRAJ, "n_classes": N_CLASSES, "guidance_scale_of_cfg": 2.0, "variants": {}}
    ms = {}
    for v, (B, g) in VARIANTS.items():
        ms[v] = sorted(reps[v])[len(reps[v]) // 2]
        res["variants"][v] = {"batch": B, "rows_per_evaluation": B if g in (None, 1.0) else 2 * B, "ms_per_step": round(ms[v], 4),
                              "ms_per_step_repetitions": [round(x, 4) for x in reps[v]]}
    with open(os.path.join(ROOT, "profiles", "solver_steps.json")) as f:
        parent = json.load(f)["solvers"]["euler_maruyama"]
    res["comparisons"] = {
        "g1_B512_over_plain_B512": round(ms["g1_B512"] / ms["plain_B512"], 4),
        "cfg_B512_over_plain_B1024": round(ms["cfg_B512"] / ms["plain_B1024"], 4),
        "cfg_B256_over_plain_B512": round(ms["cfg_B256"] / ms["plain_B512"], 4),
        "plain_B512_over_parent_solver_steps_json": round(ms["plain_B512"] / parent["ms_per_interval"], 4),
        "parent_ms_per_interval": parent["ms_per_interval"], "parent_repetitions": parent["ms_per_interval_repetitions"]}

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

    B = 512
    temb = torch.randn(d, device=dev)
    out = torch.empty(2 * B, d, device=dev)
    hid = torch.randn(2 * B * L * d, device=dev)
    sco = torch.randn(2 * B * L * Cn, device=dev)
    res["operator_us_per_launch"] = {
        "note": "back-to-back launches between two events at B = 512: launch spacing, not a kernel trace",
        "ffd_class_temb (B, d)": launches(lambda: lib.ffd_class_temb(temb.data_ptr(), 0, table.data_ptr(), N_CLASSES,
                                                                      labels.data_ptr(), B, d, 0, out.data_ptr(), stream)),
        "ffd_class_temb stacked (2 B, d)": launches(lambda: lib.ffd_class_temb(temb.data_ptr(), 0, table.data_ptr(), N_CLASSES,
                                                                                labels.data_ptr(), B, d, 1, out.data_ptr(), stream)),
        "ffd_cfg_combine hidden rows (B L d floats)": launches(lambda: lib.ffd_cfg_combine(
            hid.data_ptr(), hid.data_ptr() + 4 * B * L * d, 2.0, B * L * d, stream)),
        "ffd_cfg_combine score (B L C floats)": launches(lambda: lib.ffd_cfg_combine(
            sco.data_ptr(), sco.data_ptr() + 4 * B * L * Cn, 2.0, B * L * Cn, stream))}

    # ---- a training step with and without classes ----
    from fastfourierdiffusion_amd.models.score_models import ClassConditionalScoreModule, ScoreModule
    from fastfourierdiffusion_amd.training import Trainer

    res["training_step_ms"] = {"model": "d_model 60, 12 heads, 3 layers, dim_feedforward 2048 (L 187, C 1); p_uncond 0.1"}
    for Bt in (64, 512):
        row = {}
        X = torch.randn(Bt, L, Cn, device=dev)
        y = torch.randint(0, N_CLASSES, (Bt,), generator=gen)
        trainers = {}
        for name in ("plain", "classes"):
            torch.manual_seed(0)
            kw = dict(n_channels=Cn, max_len=L, noise_scheduler=sch, d_model=60, num_layers=3, n_head=12)
            m = (ScoreModule(**kw) if name == "plain" else ClassConditionalScoreModule(n_classes=N_CLASSES, **kw)).to(dev)
            trainers[name] = Trainer(m, seed=0)
        rp = {k: [] for k in trainers}
        for rep in range(REPS + 1):  # (the first repetition warms up)
            for name, tr in trainers.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(30):
                    tr.step(X, labels=y if name == "classes" else None, lr=1e-4)
                torch.cuda.synchronize(dev)
                if rep:
                    rp[name].append((time.perf_counter() - t0) * 1e3 / 30)
        for name in trainers:
            row[name] = round(sorted(rp[name])[len(rp[name]) // 2], 4)
            row[name + "_repetitions"] = [round(v, 4) for v in rp[name]]
        row["classes_over_plain"] = round(row["classes"] / row["plain"], 4)
        row["note"] = "Trainer.step with labels validates them on the host every call (one copy); fit hands them over once"
        res["training_step_ms"][f"B{Bt}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
