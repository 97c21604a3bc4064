"""What a training step costs: `python tools/train_bench.py [out.json]` (default profiles/train_step.json).

Networks: the ECG transformer (L = 187, C = 1, d_model 60, 12 heads, 3 layers, dim_feedforward 2048) and the default MLP
(MLPScoreModule, d_model 72, d_mlp 512, 3 blocks), each at B = 64 and B = 512.  Each figure is the median of REPS
repetitions of INNER back-to-back calls between two events after WARMUP calls, with the repetitions' min and max.

  step            Trainer.step: perturbation, training forward, loss + gradient, backward, norm, AdamW
  parts           the training forward alone, loss_and_grad, the norm, AdamW (each timed on its own)
  eval_batch      one ffd_sm_eval_batch (the inference forward + loss) at the same B, same process; the flop count says a
                  step is 3 x it
  torch_cpu       the same step by torch autograd of the oracle's forward + torch.optim.AdamW on 16 host threads
  kernel_classes  the transformer's step split by kernel class: every operator timed alone at the layer's shape, times its
                  launches per step (GEMMs: forward dense, dgrad, wgrad of the five products; attention forward / backward;
                  LayerNorm forward / backward), and what is left of the measured step (elementwise kernels, launch gaps)
  gemm            dgrad and wgrad at the ECG transformer's FFN shape (M = B x 187 rows, 2048 x 60), TFLOP/s against the
                  157.3 fp32 matrix peak
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fastfourierdiffusion_amd import _native as N  # noqa: E402

WARMUP, REPS, INNER = 20, 10, 50
FP32_PEAK = 157.3e12
L, CH = 187, 1


def timed(fn, inner=INNER, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


TF = dict(d=60, H=12, NL=3, F=2048)


def tf_kernel_classes(B, step_ms):
    """Every operator of a transformer layer alone at its shape, times its launches per step."""
    lib, stream = N.lib(), N.current_stream_ptr(torch.device("cuda"))
    M, d, H, F, NL = B * L, TF["d"], TF["H"], TF["F"], TF["NL"]
    hd = d // H
    r = lambda *sh: torch.randn(*sh, device="cuda")  # noqa: E731
    out = {}

    def gemm(n, k):  # forward dense + dgrad + wgrad of one (N, K) product at M rows
        dY, W, X = r(M, n), r(n, k), r(M, k)
        dX, dW, db = torch.empty(M, k, device="cuda"), torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
        nbytes = lib.ffd_dense_wgrad_work_bytes(M, n, k)
        work = torch.empty(max(nbytes, 8) // 8 + 1, device="cuda", dtype=torch.float64)
        dg = timed(lambda: lib.ffd_dense_dgrad(dY.data_ptr(), W.data_ptr(), None, None, dX.data_ptr(), M, n, k, stream), 10, 5, 3)
        wg = timed(lambda: lib.ffd_dense_wgrad(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), db.data_ptr(), M, n, k, work.data_ptr(),
                                               nbytes, stream), 10, 5, 3)
        return dg["median_ms"], wg["median_ms"]

    prods = {"in_proj (3d x d)": (3 * d, d), "out_proj (d x d)": (d, d), "linear1 (F x d)": (F, d), "linear2 (d x F)": (d, F)}
    dgrad_ms = wgrad_ms = 0.0
    for name, (n, k) in prods.items():
        a, b = gemm(n, k)
        out[f"dgrad {name}"], out[f"wgrad {name}"] = a, b
        dgrad_ms += a
        wgrad_ms += b
    qkv, o, lse, do, dqkv = r(M, 3 * d), torch.empty(M, d, device="cuda"), torch.empty(B, H, L, device="cuda"), r(M, d), torch.empty(M, 3 * d, device="cuda")
    out["attention forward"] = timed(lambda: lib.ffd_attention_lse_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, L, H, hd, stream), 10, 5, 3)["median_ms"]
    out["attention backward"] = timed(lambda: lib.ffd_attention_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), B, L, H, hd, stream), 10, 5, 3)["median_ms"]
    x, g, bt, y, xh, rs, dg_, db_ = r(M, d), r(d), r(d), torch.empty(M, d, device="cuda"), torch.empty(M, d, device="cuda"), torch.empty(M, device="cuda"), torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    out["layernorm forward"] = timed(lambda: lib.ffd_layernorm_stats_fwd(x.data_ptr(), g.data_ptr(), bt.data_ptr(), y.data_ptr(), xh.data_ptr(), rs.data_ptr(), M, d, 1e-5, stream), 10, 5, 3)["median_ms"]
    out["layernorm backward"] = timed(lambda: lib.ffd_layernorm_bwd(do.data_ptr(), xh.data_ptr(), rs.data_ptr(), g.data_ptr(), y.data_ptr(), dg_.data_ptr(), db_.data_ptr(), M, d, stream), 10, 5, 3)["median_ms"]
    per_step = {"dgrad (4 products x %d layers)" % NL: NL * dgrad_ms, "wgrad (4 products x %d layers)" % NL: NL * wgrad_ms,
                "attention forward": NL * out["attention forward"], "attention backward": NL * out["attention backward"],
                "layernorm forward (2 per layer)": 2 * NL * out["layernorm forward"],
                "layernorm backward (2 per layer)": 2 * NL * out["layernorm backward"]}
    per_step["everything else (forward dense, ends, loss, norm, AdamW, gaps)"] = step_ms - sum(per_step.values())
    return {"per_launch_ms": out, "per_step_ms": per_step}


def net_rows(B, kind="mlp"):
    from fastfourierdiffusion_amd.models.score_models import MLPScoreModule, ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler
    from fastfourierdiffusion_amd.training import Trainer
    from fastfourierdiffusion_amd.utils.losses import _eval_batch
    from oracle import ffd_oracle as O

    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(L)
    torch.manual_seed(0)
    if kind == "mlp":
        model = MLPScoreModule(n_channels=CH, max_len=L, noise_scheduler=sch).cuda()
        fwd = lambda x, t, sd: O.mlp_score_forward(x, t, sd, 3)  # noqa: E731
    else:
        model = ScoreModule(n_channels=CH, max_len=L, noise_scheduler=sch, d_model=TF["d"], num_layers=TF["NL"],
                            n_head=TF["H"]).cuda()
        fwd = lambda x, t, sd: O.score_forward(x, t, sd, TF["NL"], TF["H"])  # noqa: E731
    heavy = kind != "mlp"
    tr = Trainer(model)
    X = torch.randn(B, L, CH, device="cuda")
    t = torch.rand(B, device="cuda") * 0.9 + 0.05
    lib, stream = N.lib(), N.current_stream_ptr(X.device)
    score = torch.empty_like(X)
    per = torch.empty(B, device="cuda", dtype=torch.float64)
    kw = dict(inner=10, reps=5, warmup=5) if heavy else {}
    row = {"B": B, "step": timed(lambda: tr.step(X, timesteps=t), **kw)}
    sq = tr.grad_sqnorm()
    row["parts"] = {
        "training_forward": timed(lambda: lib.ffd_train_forward(tr.handle, X.data_ptr(), t.data_ptr(), score.data_ptr(), B, stream), **kw),
        "loss_and_grad": timed(lambda: tr.loss_and_grad(X, timesteps=t), **kw),
        "grad_sqnorm": timed(lambda: lib.ffd_train_grad_sqnorm(tr.handle, sq.data_ptr(), stream), **kw),
        "adamw": timed(lambda: tr.apply_update(sq, lr=0.0), **kw),
    }
    model.eval()
    row["eval_batch"] = timed(lambda: _eval_batch(model, X, t, None, 0, 0, False, True, per), **kw)
    if heavy:
        row["kernel_classes"] = tf_kernel_classes(B, row["step"]["median_ms"])
    row["step_over_eval_batch"] = row["step"]["median_ms"] / row["eval_batch"]["median_ms"]
    # the same step on the host: fp32 autograd of the oracle's forward, clip, AdamW
    torch.set_num_threads(16)
    sd = {k: v.detach().cpu().clone().requires_grad_(k != "time_encoder.W") for k, v in model.state_dict().items()}
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-2)
    Xc, tc, G = X.cpu(), t.cpu(), sch.G
    zc = torch.randn_like(Xc)

    def host_step():
        mc, sg = sch.marginal_coeffs(tc)
        std = sg[:, None] * G[None, :]
        xn = mc[:, None, None] * Xc + std[:, :, None] * zc
        r = fwd(xn, tc, sd) + zc / std[:, :, None]
        loss = ((1.0 / (1.0 / std ** 2).sum(1)) * (r ** 2).flatten(1).mean(1)).mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()

    n_in, n_rep = (1, 3) if heavy else (10, REPS)
    for _ in range(1 if heavy else 5):
        host_step()
    ts = []
    for _ in range(n_rep):
        t0 = time.perf_counter()
        for _ in range(n_in):
            host_step()
        ts.append((time.perf_counter() - t0) * 1000.0 / n_in)
    row["torch_cpu_16_threads"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    return row


def gemm_rows(B):
    lib, stream = N.lib(), N.current_stream_ptr(torch.device("cuda"))
    M, F, d = B * L, 2048, 60
    out = {"M": M}
    for name, n, k in (("linear1 (N = 2048, K = 60)", F, d), ("linear2 (N = 60, K = 2048)", d, F)):
        dY, W, X = (torch.randn(s, device="cuda") for s in ((M, n), (n, k), (M, k)))
        dX, dW, db = torch.empty(M, k, device="cuda"), torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
        nbytes = lib.ffd_dense_wgrad_work_bytes(M, n, k)
        work = torch.empty(max(nbytes, 8) // 8 + 1, device="cuda", dtype=torch.float64)
        flop = 2.0 * M * n * k
        for op, fn in (("dgrad", lambda: lib.ffd_dense_dgrad(dY.data_ptr(), W.data_ptr(), None, None, dX.data_ptr(), M, n, k, stream)),
                       ("wgrad", lambda: lib.ffd_dense_wgrad(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), db.data_ptr(), M, n, k,
                                                             work.data_ptr(), nbytes, stream))):
            assert fn() == 0
            r = timed(fn, inner=10, warmup=5)
            r["tflops"] = flop / (r["median_ms"] * 1e-3) / 1e12
            r["share_of_fp32_peak"] = r["tflops"] * 1e12 / FP32_PEAK
            if op == "wgrad":
                r["chunks"] = lib.ffd_dense_wgrad_chunks(M, n, k)
            out[f"{op} {name}"] = r
    return out


def main(out_path):
    result = {"what": "milliseconds per training step on one MI355X; median / min / max of %d repetitions of %d calls after "
                      "%d warm-up calls" % (REPS, INNER, WARMUP),
              "ecg_transformer": [net_rows(B, "transformer") for B in (64, 512)],
              "mlp_default": [net_rows(B) for B in (64, 512)],
              "gemm_at_the_ecg_ffn_shape": [gemm_rows(B) for B in (64, 512)]}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_step.json"))
