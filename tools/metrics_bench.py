"""Time the sliced Wasserstein metric at the ECG evaluation size (n = 87 554 training rows, m = 10 000 samples,
D = 187, K = 1000 directions) on one MI355X and write profiles/metrics_ecg_eval.json:

  * SlicedWasserstein.__call__ with the original set already prepared, and the prepare step (HIP events, one warm-up,
    REPS repetitions, median and spread);
  * each kernel class alone (ffd_w2_bench_kernels: projection, segmented sort, quantile integral, column transpose)
    with its rate against the chip's peaks: projection TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak and its
    store rate, the sort in keys/s and HBM bytes moved per key, the integral in GB/s;
  * the comparison line: the float64 numpy closed form (the stand-in for the reference, whose POT path is not
    installable here) for the same 1000 directions on the host's cores.

tools/metrics_bench.py [--reps 10] [--n 87554] [--m 10000] [--dirs 1000] [--out profiles/metrics_ecg_eval.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from fastfourierdiffusion_amd import _native as N
from fastfourierdiffusion_amd.sampling.metrics import SlicedWasserstein

SORT_CHUNK = 8192  # csrc/ffd_metrics.hip


def w2_sorted(a, b):
    n, m = len(a), len(b)
    bp = np.unique(np.concatenate([np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n]))
    lo, hi = bp[:-1], bp[1:]
    return float(np.sqrt(np.sum((hi - lo) * (a[lo // m] - b[lo // n]) ** 2) / (n * m)))


def host_comparator(X, Y, seed, K):
    rng = np.random.default_rng(seed)
    out = np.empty(K)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    for k in range(K):  # the reference's loop: one direction at a time
        v = rng.normal(size=X.shape[1])
        u = v / np.linalg.norm(v)
        out[k] = w2_sorted(np.sort(X64 @ u), np.sort(Y64 @ u))
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=87554)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--features", type=int, default=187)
    ap.add_argument("--dirs", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "metrics_ecg_eval.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs an MI355X"
    n, m, D, K = a.n, a.m, a.features, a.dirs
    rs = np.random.RandomState(11)
    X = rs.randn(n, D).astype(np.float32)
    Y = (1.1 * rs.randn(m, D) + 0.05).astype(np.float32)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    dev = Xd.device

    metric = SlicedWasserstein(Xd, random_seed=42, num_directions=K, save_all_distances=True)

    def prepare():
        metric._prepared.clear()
        metric(Yd[:1])  # m = 1: the projection and sort of the other set and the integral are negligible beside n

    res = {"shape": {"n": n, "m": m, "D": D, "K": K}, "reps": a.reps}
    res["prepare_original_set"] = timed(prepare, a.reps)
    out = metric(Yd)
    res["call_with_prepared_set"] = timed(lambda: metric(Yd), a.reps)

    # kernel classes
    lib = N.lib()
    kk = min(K, D)  # the column transpose has D columns to take
    dirs = torch.from_numpy(np.stack(metric._wd(Xd, Yd, False).get_random_directions(K)).astype(np.float32)).to(dev)
    rows = torch.empty((K, n), device=dev, dtype=torch.float32)
    scratch = torch.empty((K, n), device=dev, dtype=torch.float32)
    other = torch.sort(Yd @ dirs.T, dim=0).values.T.contiguous()  # (K, m): bench input only, not a result
    dist = torch.empty(K, device=dev, dtype=torch.float64)
    ms_all = (C.c_float * 4)()
    N.check(lib.ffd_w2_bench_kernels(Xd.data_ptr(), n, D, dirs.data_ptr(), K, rows.data_ptr(), scratch.data_ptr(),
                                     other.data_ptr(), m, dist.data_ptr(), a.reps, ms_all, N.current_stream_ptr(dev)),
            None, "ffd_w2_bench_kernels")
    col_ms = ms_all[3]
    proj_ms, sort_ms, int_ms = ms_all[0], ms_all[1], ms_all[2]
    passes = 0
    r = SORT_CHUNK
    while r < n:
        passes, r = passes + 1, 2 * r
    res["kernels"] = {
        "k_w2_project": {"ms": round(proj_ms, 3), "tflops": round(2.0 * n * D * K / proj_ms / 1e9, 2),
                         "frac_of_157.3_tflops": round(2.0 * n * D * K / proj_ms / 1e9 / 157.3, 4),
                         "store_gb_s": round(4.0 * n * K / proj_ms / 1e6, 1)},
        "sort (k_w2_sort_chunk + k_w2_merge)": {"ms": round(sort_ms, 3), "gkeys_per_s": round(n * K / sort_ms / 1e6, 2),
                                                "merge_passes": passes, "hbm_bytes_per_key": 8 * (1 + passes),
                                                "hbm_gb_s": round(8.0 * (1 + passes) * n * K / sort_ms / 1e6, 1)},
        "k_w2_integral": {"ms": round(int_ms, 3), "gb_s": round(4.0 * (n + m) * K / int_ms / 1e6, 1)},
        "k_w2_columns": {"ms": round(col_ms, 3), "columns": kk, "gb_s": round(8.0 * n * kk / col_ms / 1e6, 1)},
        "note": "HIP events around each class, mean of reps launches; HBM peak 8 TB/s (6.3 achievable)",
    }

    t0 = time.perf_counter()
    ref = host_comparator(X, Y, 42, K)
    host_s = time.perf_counter() - t0
    got = np.array(out["sliced_wasserstein_all"])
    res["host_float64_comparator"] = {"seconds": round(host_s, 2), "threads": torch.get_num_threads(),
                                      "cpus_available": len(os.sched_getaffinity(0))}
    res["speedup_call_vs_host"] = round(host_s * 1e3 / res["call_with_prepared_set"]["median_ms"], 1)
    res["speedup_prepare_plus_call_vs_host"] = round(
        host_s * 1e3 / (res["call_with_prepared_set"]["median_ms"] + res["prepare_original_set"]["median_ms"]), 1)
    res["max_abs_difference_to_comparator"] = float(np.abs(got - ref).max())
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
