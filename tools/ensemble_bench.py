"""Time the ensemble scores (ffd_ens_pointwise, ffd_ens_energy) on one MI355X and write profiles/ensemble_scores.json.

Two sizes: S = 64 series of m = 1024 members (an evaluation batch) and S = 1 series of m = 8192 members, D = 187 (the ECG
length).  Each entry point is timed between device events: a warm-up, then REPS repetitions of ITERS calls (mean / min /
max of the repetitions).  ffd_ens_bench_energy times the energy score's stages apart; the pair kernel's rate counts
2 D FLOP per pair (i < j) against the 157.3 TFLOP/s fp32 matrix peak -- the tiles it computes carry more: the columns of a
64 x 256 tile that lie below the diagonal are computed and dropped.  The comparison line is the float64 numpy restatement
of the same scores (sorted CRPS, quantiles, ranks; Gram-form pair distances) on the host's threads.

tools/ensemble_bench.py [--iters 10] [--reps 3] [--out profiles/ensemble_scores.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fastfourierdiffusion_amd import _native as N  # noqa: E402

SIZES = ((64, 1024, 187), (1, 8192, 187))
LEVELS = (0.05, 0.5, 0.95)
FP32_PEAK = 157.3e12


def host_pointwise(X, y):
    X = X.astype(np.float64)
    m = X.shape[1]
    xs = np.sort(X, axis=1)
    i = np.arange(1, m + 1, dtype=np.float64)[None, :, None]
    crps = np.abs(X - y[:, None, :]).sum(axis=1) / m - ((2.0 * i - m - 1.0) * xs).sum(axis=1) / (m * m)
    quant = np.quantile(X, LEVELS, axis=1)
    return crps, crps.mean(axis=1), quant, (X < y[:, None, :]).sum(axis=1), (X == y[:, None, :]).sum(axis=1)


def host_energy(X, y):
    X = X.astype(np.float64)
    S, m, _ = X.shape
    out = np.empty(S)
    for s in range(S):
        V = X[s] - X[s].mean(axis=0)
        n = (V * V).sum(axis=1)
        d2 = np.maximum(n[:, None] + n[None, :] - 2.0 * (V @ V.T), 0.0)
        np.fill_diagonal(d2, 0.0)
        out[s] = np.sqrt(((X[s] - y[s]) ** 2).sum(axis=1)).sum() / m - np.sqrt(d2).sum() / (2.0 * m * m)
    return out


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return {"ms_mean": round(float(np.mean(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "ensemble_scores.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_bench needs an MI355X"
    torch.set_num_threads(16)
    lib = N.lib()
    stream = int(torch.cuda.current_stream().cuda_stream)
    res = {"what": "ms per call between device events: warm-up, then reps repetitions of iters calls (mean / min / max of the "
                   "repetitions); host: the float64 numpy restatement, seconds", "iters": a.iters, "reps": a.reps,
           "levels": list(LEVELS), "cases": {}}
    for S, m, D in SIZES:
        rs = np.random.RandomState(S + m)
        X = (rs.randn(S, 1, D) + rs.randn(S, m, D)).astype(np.float32)
        y = (X[:, 0, :] + rs.randn(S, D)).astype(np.float32)
        Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
        nq = len(LEVELS)
        nbytes = lib.ffd_ens_work_bytes(S, m, D, nq, 1 << 30)
        work = torch.empty((nbytes + 15) // 16 * 2, device="cuda", dtype=torch.float64)
        crps = torch.empty((S, D), device="cuda", dtype=torch.float64)
        mean = torch.empty(S, device="cuda", dtype=torch.float64)
        quant = torch.empty((nq, S, D), device="cuda", dtype=torch.float64)
        below = torch.empty((S, D), device="cuda", dtype=torch.int32)
        equal = torch.empty_like(below)
        es = torch.empty(S, device="cuda", dtype=torch.float64)
        lv = (C.c_double * nq)(*LEVELS)

        def pointwise():
            rc = lib.ffd_ens_pointwise(Xd.data_ptr(), yd.data_ptr(), None, 1, S, m, D, lv, nq, 0, crps.data_ptr(),
                                       mean.data_ptr(), quant.data_ptr(), below.data_ptr(), equal.data_ptr(),
                                       work.data_ptr(), nbytes, stream)
            assert rc == 0, rc

        def energy():
            rc = lib.ffd_ens_energy(Xd.data_ptr(), yd.data_ptr(), None, 1, S, m, D, 0, es.data_ptr(), work.data_ptr(),
                                    nbytes, stream)
            assert rc == 0, rc

        case = {"ffd_ens_pointwise": timed(pointwise, a.iters, a.reps), "ffd_ens_energy": timed(energy, a.iters, a.reps)}
        ms = (C.c_float * 2)()
        N.check(lib.ffd_ens_bench_energy(Xd.data_ptr(), yd.data_ptr(), None, 1, S, m, D, 0, es.data_ptr(), work.data_ptr(),
                                         nbytes, a.iters * a.reps, ms, stream), None, "ffd_ens_bench_energy")
        flops = 2.0 * D * S * m * (m - 1) / 2.0
        case["energy_stages"] = {"mean_centre_truth_ms": round(ms[0], 4), "k_ens_pairs_ms": round(ms[1], 4),
                                 "k_ens_pairs_tflops": round(flops / (ms[1] * 1e-3) / 1e12, 2),
                                 "k_ens_pairs_share_of_fp32_matrix_peak": round(flops / (ms[1] * 1e-3) / FP32_PEAK, 4)}
        t0 = time.perf_counter()
        h_crps, h_mean, h_quant, h_below, h_equal = host_pointwise(X, y)
        t1 = time.perf_counter()
        h_es = host_energy(X, y)
        t2 = time.perf_counter()
        case["host_float64"] = {"pointwise_s": round(t1 - t0, 3), "energy_s": round(t2 - t1, 3),
                                "threads": torch.get_num_threads(), "cpus_available": len(os.sched_getaffinity(0))}
        case["speedup_pointwise"] = round((t1 - t0) * 1e3 / case["ffd_ens_pointwise"]["ms_mean"], 1)
        case["speedup_energy"] = round((t2 - t1) * 1e3 / case["ffd_ens_energy"]["ms_mean"], 1)
        case["max_abs_difference_to_host"] = {
            "crps": float(np.abs(crps.cpu().numpy() - h_crps).max()), "quantiles": float(np.abs(quant.cpu().numpy() - h_quant).max()),
            "below_equal_mismatches": int((below.cpu().numpy() != h_below).sum() + (equal.cpu().numpy() != h_equal).sum()),
            "energy": float(np.abs(es.cpu().numpy() - h_es).max())}
        res["cases"][f"S{S}_m{m}_D{D}"] = case
        print(S, m, D, json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
