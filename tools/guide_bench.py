"""What a guided conditional step costs next to a replacement step, at the ECG shape (L = 187, C = 1), B = 512.

    python3 tools/guide_bench.py [out.json]                  (default: profiles/guided_steps.json)

One process, one MI355X.  For the ECG transformer (bench.py's model: d 72, 12 heads, 10 layers, F 2048; the guided loop
takes its forward and input VJP from a parameter-only ``ffd_train``) and for a mixture of 4096 components of the same
shape:
  * one ``ffd_sample_batch_guided`` step against one ``ffd_sample_batch_cond`` step (n_corrector = 0), frequency domain,
    a shared prefix observation, Philox draws, both with the projection;
  * the launches of a guided step on their own: the score (training forward / ``ffd_mixture_score``), ``ffd_guide_seed``,
    the VJP (``ffd_train_input_vjp`` / ``ffd_mixture_score_vjp``), ``ffd_guide_combine``.
Times are device-event times over REPS calls behind WARM warm-up calls, each ending in a synchronise; the median of
three repetitions.  The loops run steps [900, 900 + n) of the 1000-point grid (t = 0.1 ... 0.05) at scale 1e-3: the
transformer's weights are synthetic, not a score, and a guided run of them from t = 1 leaves fp32;
the time of a step does not depend on the values."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

B, L, CH, K = 512, 187, 1, 4096
GRID, FIRST, STEPS, WARM, REPS = 1000, 900, 50, 5, 3


def timed(fn, count):
    """ms per call of ``fn`` over ``count`` calls (device events), median of REPS repetitions behind WARM calls."""
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / count)
    return statistics.median(out)


def main(out_path):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    dev = torch.device("cuda")
    lib = N.lib()
    stream = N.current_stream_ptr(dev)
    tf, sch, _ = bench.build_model(dev, "ecg")
    rng = np.random.default_rng(0)
    msch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
    msch.set_noise_scaling(L)
    mix = MixtureScoreModule(n_channels=CH, max_len=L, noise_scheduler=msch,
                             means=torch.from_numpy(rng.standard_normal((K, L, CH)).astype(np.float32)),
                             variance=torch.full((L, CH), 0.01)).cuda().eval()
    sch.set_timesteps(GRID)
    ts = sch.timesteps.to(torch.float32)
    ts_c = (C.c_float * GRID)(*ts.tolist())
    h = float(sch.step_size)
    obs = torch.from_numpy(rng.standard_normal((1, L, CH)).astype(np.float32)).cuda()
    mask = torch.zeros(1, L, CH, device=dev)
    mask[:, : L // 2] = 1.0
    cond = N.CondCfg(obs.data_ptr(), mask.data_ptr(), None, 1, N.FFD_COND_FREQUENCY, 0, 0)
    guide = N.GuideCfg(1e-3, 1e-2, 1.0, 1, 0)
    desc = sch._desc()
    G = sch._G_on(dev)
    x0 = torch.from_numpy((0.3 * rng.standard_normal((B, L, CH))).astype(np.float32)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "L": L, "C": CH}, "grid": GRID, "first_step": FIRST,
           "steps_per_call": STEPS, "repetitions": REPS, "what": "ms per reverse step / per launch, device events, median",
           "models": {}}

    for name, model in (("ecg_transformer", tf), ("mixture_K4096", mix)):
        ctx = model._ctx()
        net = DiffusionSampler(model, B)
        handle = net._guide_net_handle()  # None for the mixture
        x = x0.clone()

        def guided():
            x.copy_(x0)
            N.check(lib.ffd_sample_batch_guided(ctx.handle, handle, x.data_ptr(), B, ts_c, GRID, h, FIRST, STEPS, 7, 0, None,
                                                C.byref(cond), C.byref(guide), None, stream), ctx.handle, "guided")

        def replaced():
            x.copy_(x0)
            N.check(lib.ffd_sample_batch_cond(ctx.handle, x.data_ptr(), B, ts_c, GRID, h, FIRST, STEPS, 0, 0.16, 0, 7, 0, None,
                                              0, 0, C.byref(cond), stream), ctx.handle, "cond")

        t_guided, t_cond = timed(guided, 1) / STEPS, timed(replaced, 1) / STEPS
        assert torch.isfinite(x).all()
        # the launches on their own
        score, u, v, jtv = (torch.empty_like(x0) for _ in range(4))
        times = torch.full((B,), float(ts[FIRST]), device=dev)
        t_dev = times[:1]
        if handle is not None:
            fwd = lambda: N.check(lib.ffd_train_forward(handle, x0.data_ptr(), times.data_ptr(), score.data_ptr(), B, stream),  # noqa: E731
                                  None, "ffd_train_forward")
            vjp = lambda: N.check(lib.ffd_train_input_vjp(handle, v.data_ptr(), jtv.data_ptr(), B, stream), None,  # noqa: E731
                                  "ffd_train_input_vjp")
            infer = lambda: N.check(lib.ffd_score_forward(ctx.handle, x0.data_ptr(), float(ts[FIRST]), score.data_ptr(), B,  # noqa: E731
                                                          stream), ctx.handle, "ffd_score_forward")
        else:
            m = model.mixture
            n1, n2 = lib.ffd_mixture_work_floats(B, K, L, CH), lib.ffd_mixture_vjp_work_floats(B, K, L, CH)
            work = torch.empty(max(n1, n2), device=dev)
            margs = (m.means.data_ptr(), m.log_weights.data_ptr(), m.variance.data_ptr(), G.data_ptr())
            fwd = lambda: N.check(lib.ffd_mixture_score(C.byref(desc), x0.data_ptr(), t_dev.data_ptr(), 0, *margs,  # noqa: E731
                                                        score.data_ptr(), B, K, L, CH, work.data_ptr(), n1, stream), None, "score")
            vjp = lambda: N.check(lib.ffd_mixture_score_vjp(C.byref(desc), x0.data_ptr(), t_dev.data_ptr(), 0, *margs,  # noqa: E731
                                                            v.data_ptr(), jtv.data_ptr(), B, K, L, CH, work.data_ptr(), n2,
                                                            stream), None, "vjp")
            infer = None
        seed = lambda: N.check(lib.ffd_guide_seed(C.byref(desc), x0.data_ptr(), score.data_ptr(), obs.data_ptr(),  # noqa: E731
                                                  mask.data_ptr(), None, G.data_ptr(), float(ts[FIRST]), 1,
                                                  N.FFD_COND_FREQUENCY, B, L, CH, u.data_ptr(), v.data_ptr(), None, None, stream),
                               None, "ffd_guide_seed")
        comb = lambda: N.check(lib.ffd_guide_combine(score.data_ptr(), u.data_ptr(), jtv.data_ptr(), 0.9, 1e-3,  # noqa: E731
                                                     score.data_ptr(), B * L * CH, stream), None, "ffd_guide_combine")
        fwd()
        seed()
        entry = {"guided_step_ms": t_guided, "replacement_step_ms": t_cond, "guided_over_replacement": t_guided / t_cond,
                 "launches_ms": {"score_forward_of_the_guided_step": timed(fwd, 20), "guide_seed": timed(seed, 50),
                                 "input_vjp": timed(vjp, 20), "guide_combine": timed(comb, 50)}}
        if infer is not None:
            entry["launches_ms"]["inference_forward_of_the_replacement_step"] = timed(infer, 20)
        res["models"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del net
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "guided_steps.json"))
