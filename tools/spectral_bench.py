"""Cost of the localization metrics, the frequency smoothing and the spectral profiles on the device, per stage.

    python3 tools/spectral_bench.py [out.json]               on an MI355X (default: profiles/spectral_profile.json)
    python3 tools/spectral_bench.py --reference [out.json]   where the reference sources are mounted: times the
                                                             reference's own fp32 CPU functions on 16 host threads on
                                                             the same inputs and merges them into the same file

Shapes: the ECG training set (87 554 x 187 x 1) and 8192 x 512 x 8.  Per shape: the stages of ffd_localization
(ffd_localization_bench: the entry point's own stage sequence with HIP events around the time-domain rows, dft +
density + frequency rows, the two product launches), the whole ffd_localization / ffd_spectral_profile call and, at an
odd length (ECG, and 8192 x 511 x 8 in place of 512), ffd_smooth_frequency.  Every figure is the mean of 200 timed
runs after 10 warm-up runs, each run between its own pair of HIP events, with the fastest and the slowest run beside
it.  The runs rotate through enough copies of the input to exceed the 256 MB last-level cache (plus the call's own
scratch, written in between), so a run reads its input from HBM, not from what the previous run left in the cache.
The product kernel's rate is its 2 * 2 B L^2 FLOPs per second against the 157.3 TFLOP/s fp32 MFMA peak; its operand
(the normalized rows, written by the stage before it) is as cache-resident as it is inside the real call.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = {"ecg_train_87554x187x1": (87554, 187, 1), "8192x512x8": (8192, 512, 8)}
WARM, ITERS = 10, 200
LLC_BYTES = 256 << 20
SIGMA = 2.0


def make_input(B, L, Cn, device, copies=1):
    g = torch.Generator(device=device).manual_seed(17)
    x = torch.randn(B, L, Cn, device=device, generator=g)
    return x if copies == 1 else x.unsqueeze(0).repeat(copies, 1, 1, 1).contiguous()


def n_copies(B, L, Cn):
    """Copies of the input whose total exceeds the last-level cache."""
    return LLC_BYTES // (4 * B * L * Cn) + 2


def stats(ms):
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed(fn, copies, warm=WARM, iters=ITERS):
    """fn(i) runs on input copy i; every timed run sits between its own pair of events."""
    for i in range(warm):
        fn(i % copies)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (start, stop) in enumerate(ev):
        start.record()
        fn((warm + i) % copies)
        stop.record()
    torch.cuda.synchronize()
    return stats([start.elapsed_time(stop) for start, stop in ev])


def run_device(out_path):
    from fastfourierdiffusion_amd import _native as N

    assert torch.cuda.is_available(), "spectral_bench needs an MI355X"
    dev = torch.device("cuda", 0)
    lib = N.lib()
    s = N.current_stream_ptr(dev)
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "iters": ITERS, "fp32_mfma_peak_tflops": PEAK_TFLOPS,
           "cache": "inputs rotated through copies that exceed the 256 MB last-level cache: read from HBM", "shapes": {}}
    for name, (B, L, Cn) in SHAPES.items():
        K = n_copies(B, L, Cn)
        x = make_input(B, L, Cn, dev, K)
        loc = torch.empty(2, B, device=dev)
        work = torch.empty((lib.ffd_localization_work_bytes(B, L, Cn) + 7) // 8, dtype=torch.float64, device=dev)
        ms = (C.c_float * 9)()
        N.check(lib.ffd_localization_bench(x.data_ptr(), K, loc[0].data_ptr(), loc[1].data_ptr(), work.data_ptr(),
                                           work.numel() * 8, B, L, Cn, WARM, ITERS, ms, s), None, "ffd_localization_bench")
        stage = [{"mean_ms": round(ms[3 * i], 4), "min_ms": round(ms[3 * i + 1], 4), "max_ms": round(ms[3 * i + 2], 4)}
                 for i in range(3)]
        flops = 2.0 * 2 * B * L * L
        tflops = flops / (stage[2]["mean_ms"] * 1e-3) / 1e12
        entry = {"input_copies": K, "time_rows": stage[0], "dft_density_freq_rows": stage[1], "product": stage[2],
                 "product_flops": flops, "product_tflops": round(tflops, 2),
                 "product_share_of_peak": round(tflops / PEAK_TFLOPS, 4)}
        entry["ffd_localization"] = timed(lambda i: N.check(lib.ffd_localization(
            x[i].data_ptr(), loc[0].data_ptr(), loc[1].data_ptr(), work.data_ptr(), work.numel() * 8, B, L, Cn, s)), K)
        del work
        nf = L // 2 + 1
        curves = torch.empty(2 * nf + 2 * L, device=dev)
        pw = torch.empty((lib.ffd_spectral_profile_work_bytes(B, L, Cn) + 7) // 8, dtype=torch.float64, device=dev)
        entry["ffd_spectral_profile"] = timed(lambda i: N.check(lib.ffd_spectral_profile(
            x[i].data_ptr(), curves.data_ptr(), curves[nf:].data_ptr(), curves[2 * nf:].data_ptr(),
            curves[2 * nf + L:].data_ptr(), pw.data_ptr(), pw.numel() * 8, B, L, Cn, s)), K)
        del pw
        Ls = L if L % 2 else L - 1
        xs = x[:, :, :Ls].contiguous()
        out = torch.empty_like(xs[0])
        sw = torch.empty((lib.ffd_smooth_frequency_work_bytes(B, Ls, Cn) + 7) // 8, dtype=torch.float64, device=dev)
        entry["ffd_smooth_frequency"] = timed(lambda i: N.check(lib.ffd_smooth_frequency(
            xs[i].data_ptr(), out.data_ptr(), sw.data_ptr(), sw.numel() * 8, B, Ls, Cn, SIGMA, s)), K)
        entry["smooth_length"] = Ls
        res["shapes"][name] = entry
        del sw, xs, out, x
    merge(out_path, res)


def run_reference(out_path):
    from oracle._ref_import import import_reference

    import_reference()
    from fdiff.utils.fourier import localization_metrics, smooth_frequency

    torch.set_num_threads(16)
    res = {"reference_cpu": {"threads": torch.get_num_threads(), "shapes": {}}}
    for name, (B, L, Cn) in SHAPES.items():
        x = make_input(B, L, Cn, torch.device("cpu"))
        entry = {}
        Ls = L if L % 2 else L - 1
        for key, fn in (("localization_metrics_ms", lambda: localization_metrics(x)),
                        ("smooth_frequency_ms", lambda: smooth_frequency(x[:, :Ls], SIGMA))):
            fn()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            entry[key] = round((time.perf_counter() - t0) / 3 * 1e3, 2)
        res["reference_cpu"]["shapes"][name] = entry
    merge(out_path, res)


def merge(out_path, res):
    old = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            old = json.load(f)
    old.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--reference"]
    path = args[0] if args else os.path.join(ROOT, "profiles", "spectral_profile.json")
    (run_reference if "--reference" in sys.argv[1:] else run_device)(path)
