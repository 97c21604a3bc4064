"""Step 0 of "sample each batch as CU-partitioned halves running out of phase": measure before building.

  python tools/partition_probe.py [--steps 300] [--runs 3] [--out profiles/partition_probe.txt]

1. Enumerates the CU mask of hipExtStreamCreateWithCUMask on this chip: one stream per single mask bit, a kernel that
   records where it ran (XCC id, shader engine, CU), so bit -> (xcc, se, cu) is measured, not assumed.  (Only the XCD
   that owns the bit is confined by such a mask: an XCD without a mask bit runs its share of the grid on any CU.)
2. Builds two partition layouts from that table -- "spread": every part owns the same number of CUs of every XCD;
   "xcd": every part owns whole XCDs -- and checks each mask with a grid that fills it.  A layout whose parts turn out
   to overlap is reported and not timed.
3. Times the ECG line (B = 512, steps 10 .. 10 + steps of a 1000-step run) alternating between
     one     B = 512 on the default stream (what bench.py times), and again on an ordinary stream as a control,
     plain2  2 x B = 256 on two ordinary streams (the arrangement of tools/two_streams.py),
     P parts x B = 512 / P on P masked streams, one ffd_ctx each, for P = 2 and (as data only: more queues than the
             process gets by default) P = 4, both layouts, and part i starting i x offset us after part 0.
   The parts run with the kernel forms the planner would pick for their share of the chip (the unsliced row-owning FFN at
   12 waves, one tile per CU), forced through ffd_tune.  Every run starts behind a gate (a delay kernel on the default
   stream) so that the host is ahead of the device on every stream before the first kernel runs; times are HIP events
   from the gate to the last part's end.
The gate: the partitioned loop is worth building only if, for some configuration, every partitioned run is below every
one-stream run.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libpartition_probe.so")
WORDS = 8  # 256 mask bits


def load_probe():
    src = os.path.join(HERE, "partition_probe.hip")
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-fPIC", "-shared",
                               "--offload-arch=gfx950", "-o", SO, src])
    pp = C.CDLL(SO)
    vp, u64 = C.c_void_p, C.c_ulonglong
    for name, args in {"pp_stream_create": [C.POINTER(vp), C.POINTER(C.c_uint32), C.c_int], "pp_stream_destroy": [vp],
                       "pp_stream_sync": [vp], "pp_event_create": [C.POINTER(vp)], "pp_event_destroy": [vp],
                       "pp_event_record": [vp, vp], "pp_stream_wait": [vp, vp],
                       "pp_event_ms": [vp, vp, C.POINTER(C.c_float)], "pp_wall_clock_khz": [C.POINTER(C.c_int)],
                       "pp_where": [vp, C.c_int, C.c_int, u64, C.POINTER(C.c_uint)], "pp_delay": [vp, u64]}.items():
        getattr(pp, name).argtypes = args
        getattr(pp, name).restype = C.c_int
    pp.pp_smid_bits.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    pp.pp_smid_bits.restype = None
    return pp


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")


def mask_words(bits):
    w = (C.c_uint32 * WORDS)()
    for b in bits:
        w[b // 32] |= 1 << (b % 32)
    return w


def layouts_from_table(table, parts):
    """table: bit -> xcc.  {"spread": [bits of part 0, ...], "xcd": [...]}, or raises where the counts do not divide."""
    by_xcc = {}
    for bit in sorted(table):
        by_xcc.setdefault(table[bit], []).append(bit)
    xccs = sorted(by_xcc)
    if len(xccs) % parts or any(len(v) % parts for v in by_xcc.values()):
        raise ValueError(f"{len(xccs)} XCDs / their CU counts do not divide by {parts}")
    spread = [[] for _ in range(parts)]
    for x in xccs:
        n = len(by_xcc[x]) // parts
        for p in range(parts):
            spread[p] += by_xcc[x][p * n:(p + 1) * n]
    per = len(xccs) // parts
    xcd = [[b for x in xccs[p * per:(p + 1) * per] for b in by_xcc[x]] for p in range(parts)]
    return {"spread": spread, "xcd": xcd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=5, help="steps per enqueue before turning to the next stream")
    ap.add_argument("--offsets", default="0,100,260", help="start offsets between consecutive parts, us")
    ap.add_argument("--gate-us", type=int, default=6000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_probe.txt"))
    args = ap.parse_args()

    import torch
    import bench
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    assert torch.cuda.is_available(), "partition_probe.py needs the GPU"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lib = N.lib()
    pp = load_probe()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    khz = C.c_int(0)
    ok(pp.pp_wall_clock_khz(C.byref(khz)), "wall clock rate")
    ticks_per_us = khz.value / 1000.0
    se_bits, cu_bits = C.c_int(0), C.c_int(0)
    pp.pp_smid_bits(C.byref(se_bits), C.byref(cu_bits))

    def decode(smid):
        cu = smid & ((1 << cu_bits.value) - 1)
        se = (smid >> cu_bits.value) & ((1 << se_bits.value) - 1)
        return smid >> (cu_bits.value + se_bits.value), se, cu

    def stream_of(bits):
        s = C.c_void_p()
        ok(pp.pp_stream_create(C.byref(s), mask_words(bits) if bits is not None else None, WORDS if bits is not None else 0),
           "stream create")
        return s

    def where(stream, n_wgs, hold_us):
        buf = (C.c_uint * n_wgs)()
        ok(pp.pp_where(stream, n_wgs, 1024, int(hold_us * ticks_per_us), buf), "pp_where")
        return sorted(set(buf))

    props = torch.cuda.get_device_properties(dev)
    n_cu = props.multi_processor_count
    say(f"# partition probe: {props.name}, {n_cu} CUs, wall clock {khz.value} kHz, "
        f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}")

    # ---- 1. the mask enumeration ---------------------------------------------------------------------------------
    # Workgroups go round the XCDs whatever the mask says, and an XCD in which the mask enables no CU runs them on any
    # of its CUs.  So under a one-bit mask only one XCD is confined: the one whose workgroups all met on one CU.
    say("\n## CU mask enumeration: mask bit -> x<xcc>s<shader engine>c<cu>, the one XCD whose 8 of 64 workgroups shared a CU")
    table, where_bit, loose = {}, {}, 0
    for bit in range(min(n_cu, 32 * WORDS)):
        s = stream_of([bit])
        buf = (C.c_uint * 64)()
        ok(pp.pp_where(s, 64, 1024, int(20 * ticks_per_us), buf), "pp_where")
        ok(pp.pp_stream_destroy(s), "stream destroy")
        per_xcc = {}
        for x, se, cu in map(decode, buf):
            per_xcc.setdefault(x, set()).add((x, se, cu))
        single = [next(iter(v)) for v in per_xcc.values() if len(v) == 1]
        loose += sum(len(v) > 1 for v in per_xcc.values())
        if len(single) == 1:
            where_bit[bit], table[bit] = single[0], single[0][0]
    for w in range(0, n_cu, 32):
        say(f"bits {w:3d}..{w + 31:3d}: " + " ".join("x%ds%dc%d" % where_bit[b] if b in where_bit else "?" for b in range(w, w + 32)))
    n_xcc = len(set(table.values()))
    rule = bool(table) and all(x == b % n_xcc for b, x in table.items())
    say(f"{len(table)} bits resolved, {n_xcc} XCDs, {len(set(where_bit.values()))} distinct CUs; "
        f"xcc == bit % {n_xcc}: {'yes for every bit' if rule else 'NO'}; "
        f"XCDs without a mask bit that ran on more than one CU: {loose} of {(n_xcc - 1) * len(table)}")
    if len(table) != n_cu or len(set(where_bit.values())) != n_cu:
        # (the masks below then rest on the driver's round robin over the XCDs, and the grid check under each mask is
        #  the evidence for them)
        say("enumeration incomplete: the layouts below assume xcc == bit % 8")
        table, where_bit, n_xcc = {b: b % 8 for b in range(n_cu)}, {}, 8

    # ---- 2. layouts ----------------------------------------------------------------------------------------------
    say("\n## partition masks (hex words 0..7) and where a grid of 4096 workgroups ran under each")
    parts_cfg = {}
    for P in (2, 4):
        for name, parts in layouts_from_table(table, P).items():
            confined = True
            for i, bits in enumerate(parts):
                s = stream_of(bits)
                ids = where(s, 4096, 20)
                ok(pp.pp_stream_destroy(s), "stream destroy")
                hist = {}
                for x, _, _ in map(decode, ids):
                    hist[x] = hist.get(x, 0) + 1
                same = {decode(i_) for i_ in ids} == {where_bit.get(b) for b in bits}
                confined = confined and len(ids) == len(bits)
                say(f"P={P} {name:6s} part {i}: " + " ".join(f"{w:08x}" for w in mask_words(bits)) +
                    f" -> {len(ids)} CUs, per XCD {[hist.get(x, 0) for x in range(n_xcc)]}, "
                    f"{'the enumerated CUs' if same else 'NOT the enumerated CUs'}")
            if confined:
                parts_cfg[(P, name)] = parts
            else:
                say(f"P={P} {name}: the parts overlap (an XCD without a mask bit is not excluded): not a partition, not timed")

    # ---- 3. timing -----------------------------------------------------------------------------------------------
    K, B = args.steps, 512

    x0 = {}  # every chain's prior draw: each timed run starts from it again

    def setup(b):
        model, sch, _ = bench.build_model(dev, "ecg")
        sch.set_timesteps(1000)
        ts_c = (C.c_float * 1000)(*sch.timesteps.tolist())
        X = DiffusionSampler(model, b, rng="philox", seed=1).sample_prior(b)
        x0[X.data_ptr()] = (X, X.clone())
        return model, X, ts_c, float(sch.step_size)

    def tune(knobs):
        ok(lib.ffd_tune(b"reset", 0), "ffd_tune reset")
        for k, v in knobs.items():
            ok(lib.ffd_tune(k.encode(), v), f"ffd_tune {k}")

    PART_KNOBS = {"ffn_rows_nw": 12, "rows_slices": -1, "mid_path": 0}  # the forms of a part's share of the chip
    PART_KNOBS4 = dict(PART_KNOBS, ffn_rows=2)  # (B = 128 is below the size at which the planner takes k_ffn_rows)

    def form(model, b):
        fl, by = C.c_double(0), C.c_double(0)
        ctx = model._ctx()
        return " + ".join((ctx.lib.ffd_kernel_work(ctx.handle, k, b, 0, C.byref(fl), C.byref(by)) or b"?").decode() for k in (1, 0))

    full = setup(B)
    halves = {P: [setup(B // P) for _ in range(P)] for P in (2, 4)}
    gate, ends = C.c_void_p(), [C.c_void_p() for _ in range(5)]
    ok(pp.pp_event_create(C.byref(gate)), "event")
    for e in ends:
        ok(pp.pp_event_create(C.byref(e)), "event")

    def timed(chains, knobs, offset_us):
        """chains: [(setup tuple, stream, global sample offset)].  ms per step from the gate to the last chain's end."""
        tune(knobs)
        for (_, X, _, _), _, _ in chains:
            X.copy_(x0[X.data_ptr()][1])
        torch.cuda.synchronize()
        ok(pp.pp_delay(None, int(args.gate_us * ticks_per_us)), "gate")
        ok(pp.pp_event_record(gate, None), "gate record")
        for i, (_, s, _) in enumerate(chains):
            if s is not None:
                ok(pp.pp_stream_wait(s, gate), "wait gate")
                if i and offset_us:
                    ok(pp.pp_delay(s, int(i * offset_us * ticks_per_us)), "offset")
        for c in range(0, K, args.chunk):
            for (model, X, ts_c, dt), s, off in chains:
                bench.run_steps(model, X, ts_c, 1000, dt, 10 + c, min(args.chunk, K - c), False, s, off)
        for (_, s, _), e in zip(chains, ends):
            ok(pp.pp_event_record(e, s), "end record")
        torch.cuda.synchronize()
        ms = C.c_float(0)
        worst = 0.0
        for _, e in zip(chains, ends):
            ok(pp.pp_event_ms(gate, e, C.byref(ms)), "elapsed")
            worst = max(worst, ms.value)
        return worst / K

    offsets = [int(v) for v in args.offsets.split(",")]
    configs = [("one     B=512 default stream", [(full, None, 0)], {}, 0)]
    streams, plain = {}, []
    try:
        plain = [stream_of(None), stream_of(None)]
        configs.append(("one'    B=512 an ordinary stream (control)", [(full, plain[0], 0)], {}, 0))
        configs.append(("plain2  2 x 256, two ordinary streams", [(halves[2][i], plain[i], 256 * i) for i in range(2)], PART_KNOBS, 0))
        for (P, name), parts in parts_cfg.items():
            try:
                streams[(P, name)] = [stream_of(bits) for bits in parts]
            except RuntimeError as e:
                say(f"P={P} {name}: {e} -- not timed")
                continue
            for off in offsets if P == 2 else offsets[:1] + offsets[-1:]:
                # (P = 4: the layer period is shared by four, so the largest offset is halved)
                o = off if P == 2 else off // 2
                configs.append((f"P={P} {name:6s} offset {o:3d} us",
                                [(halves[P][i], streams[(P, name)][i], (B // P) * i) for i in range(P)],
                                PART_KNOBS if P == 2 else PART_KNOBS4, o))
        say(f"\n## kernel forms: one stream B=512: {form(full[0], B)}")
        tune(PART_KNOBS)
        say(f"## halves (ffd_tune {PART_KNOBS}): B=256: {form(halves[2][0][0], 256)}")
        tune(PART_KNOBS4)
        say(f"## quarters (ffd_tune {PART_KNOBS4}): B=128: {form(halves[4][0][0], 128)}")
        for _, chains, knobs, _ in configs:  # warm every context on its stream (workspaces, code objects)
            tune(knobs)
            for (model, X, ts_c, dt), s, off in chains:
                bench.run_steps(model, X, ts_c, 1000, dt, 0, 10, False, s, off)
            torch.cuda.synchronize()
        say(f"\n## ms per step, ECG, 512 samples in all, {K} steps per run, {args.runs} runs, configurations alternating")
        res = {c[0]: [] for c in configs}
        for _ in range(args.runs):
            for name, chains, knobs, off in configs:
                res[name].append(timed(chains, knobs, off))
        one = res[configs[0][0]] + res[configs[1][0]]  # both one-stream arrangements count for the gate
        for name, *_ in configs:
            v = res[name]
            verdict = "" if name in (configs[0][0], configs[1][0]) else ("  every run below every one-stream run" if max(v) < min(one) else
                                                         "  not below the one-stream runs")
            say(f"{name:42s} " + " ".join(f"{x:.4f}" for x in v) + f"   mean {sum(v) / len(v):.4f}{verdict}")
        passed = [n for n, *_ in configs if n.startswith("P=2") and max(res[n]) < min(one)]
        say(f"\nGATE (P = 2 only): {'PASSED by ' + '; '.join(passed) if passed else 'NOT passed: no partitioned configuration has every run below every one-stream run'}")
    finally:
        tune({})
        torch.cuda.synchronize()
        for ss in list(streams.values()) + [plain]:
            for s in ss:
                pp.pp_stream_destroy(s)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
