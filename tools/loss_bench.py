"""Cost of the score-matching validation loss next to the forward pass it wraps, and the HBM rate of its two kernels.

    python3 tools/loss_bench.py [out.json]        (default: profiles/loss_eval_ecg.json)

1. ECG (L 187, C 1, d 72, 10 layers) at B = 512: milliseconds per ffd_sm_eval_batch (Philox draws) beside milliseconds
   per ffd_score_forward_ts on the same batch; 3 warm-up and 20 timed iterations each, HIP events around the timed
   window.  The difference is the perturbation + loss launches.
2. ffd_sm_perturb and ffd_sm_loss alone at 8192 x 512 x 8 (134 MB per tensor) with NP buffer sets in rotation, so that
   no launch finds its operands in the 256 MiB Infinity Cache: achieved GB/s against the algorithmic bytes
   (perturb: read x0, write x_noisy = 8 B per element, + 4 B with injected z; loss: read the score = 4 B, + 4 B with z).
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from fastfourierdiffusion_amd import _native as N  # noqa: E402

WARM, ITERS = 3, 20


def timed(fn, warm=WARM, iters=ITERS):
    """Mean milliseconds per call of fn(i) over `iters` calls after `warm`, between two HIP events."""
    for i in range(warm):
        fn(i)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(warm + i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loss_eval_ecg.json")
    assert torch.cuda.is_available(), "loss_bench needs an MI355X"
    dev = torch.device("cuda", 0)
    lib = N.lib()
    s = N.current_stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(1)

    # 1. the evaluation loss next to the forward
    B = 512
    model, sch, _ = bench.build_model(dev, "ecg")
    ctx = model._ctx()
    L, Cn = model.max_len, model.n_channels
    x0 = torch.randn(B, L, Cn, device=dev, generator=g)
    t = torch.rand(B, device=dev, generator=g) * (1.0 - 1e-5) + 1e-5
    mc, sg = (v.contiguous() for v in sch.marginal_coeffs(t))
    score = torch.empty_like(x0)
    per = torch.empty(B, device=dev, dtype=torch.float64)

    def fwd(i):
        N.check(lib.ffd_score_forward_ts(ctx.handle, x0.data_ptr(), t.data_ptr(), score.data_ptr(), None, B, -1, s),
                ctx.handle, "ffd_score_forward_ts")

    def ev(i):
        N.check(lib.ffd_sm_eval_batch(ctx.handle, x0.data_ptr(), t.data_ptr(), mc.data_ptr(), sg.data_ptr(), None, 42, 0,
                                      0, 1, per.data_ptr(), B, s), ctx.handle, "ffd_sm_eval_batch")

    # alternate the two, twice, so that a drift of the clocks shows up as a spread instead of as a difference
    rounds = [(timed(fwd), timed(ev)) for _ in range(2)]
    fwd_ms, ev_ms = min(r[0] for r in rounds), min(r[1] for r in rounds)

    # 2. the two kernels alone, HBM-resident operands
    Bk, Lk, Ck = 8192, 512, 8
    n = Bk * Lk * Ck
    NP = 4
    Gh = (C.c_float * Lk)()
    lib.ffd_host_noise_scaling(Lk, 1, Gh)
    Gd = torch.tensor(list(Gh), device=dev)
    tk = torch.rand(Bk, device=dev, generator=g) * (1.0 - 1e-5) + 1e-5
    mck, sgk = (v.contiguous() for v in sch.marginal_coeffs(tk))
    xs = [torch.randn(Bk, Lk, Ck, device=dev, generator=g) for _ in range(NP)]
    ys = [torch.empty_like(xs[0]) for _ in range(NP)]
    zs = [torch.randn(Bk, Lk, Ck, device=dev, generator=g) for _ in range(NP)]
    perk = torch.empty(Bk, device=dev, dtype=torch.float64)

    def perturb(z):
        def run(i):
            k = i % NP
            rc = lib.ffd_sm_perturb(xs[k].data_ptr(), ys[k].data_ptr(), mck.data_ptr(), sgk.data_ptr(), Gd.data_ptr(),
                                    zs[k].data_ptr() if z else None, 42, 0, Bk, Lk, Ck, s)
            assert rc == 0
        return run

    def loss(z):
        def run(i):
            k = i % NP
            rc = lib.ffd_sm_loss(xs[k].data_ptr(), sgk.data_ptr(), Gd.data_ptr(), zs[k].data_ptr() if z else None, 42, 0,
                                 0, 1, perk.data_ptr(), Bk, Lk, Ck, s)
            assert rc == 0
        return run

    kernels = {}
    for name, fn, nbytes in (("k_sm_perturb_v4 (Philox)", perturb(False), 8 * n),
                             ("k_sm_perturb_v4 (injected z)", perturb(True), 12 * n),
                             ("k_sm_loss (Philox)", loss(False), 4 * n), ("k_sm_loss (injected z)", loss(True), 8 * n)):
        ms = timed(fn, warm=NP, iters=5 * NP)
        kernels[name] = {"ms": round(ms, 4), "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 1)}

    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "iters": ITERS,
           "ecg_B512": {"ffd_score_forward_ts_ms": round(fwd_ms, 4), "ffd_sm_eval_batch_ms": round(ev_ms, 4),
                        "added_ms": round(ev_ms - fwd_ms, 4), "added_share_of_forward": round((ev_ms - fwd_ms) / fwd_ms, 5),
                        "rounds_ms": [[round(a, 4), round(b, 4)] for a, b in rounds]},
           "kernels_8192x512x8": kernels, "buffer_sets_in_rotation": NP}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
