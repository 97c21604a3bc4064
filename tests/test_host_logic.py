"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol
include/ffd.h declares, host-only entry points agree with the golden vectors, the
fdiff-compatible Python surface keeps the reference's names / state_dict keys / error
behaviour, and the multi-GPU shard plan is exercised with world_size-2 gloo."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def test_library_exports_every_declared_symbol(lib):
    from fastfourierdiffusion_amd import _native

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    declared = set(re.findall(r"\b(ffd_[a-z0-9_]+)\s*\(", header))
    declared -= {"ffd_ctx"}
    assert declared, "no declarations parsed"
    assert declared == set(_native.SIGNATURES), declared ^ set(_native.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ffd_[a-z0-9_]+)", nm))
    assert declared <= exported, declared - exported
    assert b"gfx950" in lib.ffd_version()


def test_no_device_fails_loudly(lib):
    """Without a GPU (this container) context creation reports an error, never a CPU path."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fastfourierdiffusion_amd import _native as N

    desc = N.ModelDesc(0, 1, 187, 72, 12, 10, 2048, 0, 0.1, 20.0, 1, 1e-5)
    h = C.c_void_p()
    rc = lib.ffd_create(C.byref(h), C.byref(desc), 0)
    assert rc == -4 and h.value
    assert b"no HIP device" in lib.ffd_last_error(h) or b"failed" in lib.ffd_last_error(h)
    lib.ffd_destroy(h)
    # unsupported shapes are rejected before any device work
    for bad in (N.ModelDesc(0, 1, 187, 36, 12, 10, 2048, 0, 0.1, 20.0, 1, 1e-5),   # d_model w/o kernel
                N.ModelDesc(0, 1, 600, 72, 12, 10, 2048, 0, 0.1, 20.0, 1, 1e-5),   # L > 512
                N.ModelDesc(0, 1, 187, 72, 12, 10, 2000, 0, 0.1, 20.0, 1, 1e-5)):  # F % 64
        rc = lib.ffd_create(C.byref(h), C.byref(bad), 0)
        assert rc == -2, lib.ffd_last_error(h)
        lib.ffd_destroy(h)


def test_host_noise_scaling_matches_golden(lib, golden):
    g = golden["g2_tables"]
    for L in cases.TABLE_LENS:
        for f in (0, 1):
            out = (C.c_float * L)()
            assert lib.ffd_host_noise_scaling(L, f, out) == 0
            np.testing.assert_array_equal(np.array(out[:], dtype=np.float32), g[f"G_L{L}_f{f}"])


def test_host_timesteps_within_one_ulp_of_torch(lib, golden):
    """torch.linspace's last ulp depends on the host's vector width, so the library takes
    the grid from the caller; its own scalar linspace must agree to <= 1 ulp."""
    g = golden["g2_tables"]
    for n in cases.TABLE_STEPS:
        ts = (C.c_float * n)()
        dt = C.c_float()
        assert lib.ffd_host_timesteps(n, 1e-5, ts, C.byref(dt)) == 0
        a = np.array(ts[:], dtype=np.float32)
        ref = g[f"ts_N{n}"]
        assert np.all(np.abs(a - ref) <= np.spacing(np.maximum(np.abs(ref), 1e-5).astype(np.float32)))
        assert a[0] == 1.0 and a[-1] == np.float32(1e-5)
    assert lib.ffd_host_timesteps(1, 1e-5, ts, C.byref(dt)) == -1  # reference: timesteps[1] IndexError


@pytest.mark.parametrize("case", cases.GATE_CASES, ids=lambda c: f"K{c[0]}R{c[1]}L{c[2]}")
def test_host_gate_matches_golden(lib, golden, case):
    from fastfourierdiffusion_amd.utils.caching import E2CRFCache

    K, R, L, steps = case
    g = golden["g9_gate"]
    sizes = [lib.ffd_host_gate(s, L, K, R) for s in steps]
    np.testing.assert_array_equal(sizes, g[f"gate_K{K}_R{R}_L{L}_sizes"])
    cache = E2CRFCache(num_layers=1, max_len=L, device=torch.device("cpu"), K=K, R=R)
    for s, n in zip(steps, sizes):
        assert cache.determine_recompute_set(None, 0.1, s) == set(range(n))  # always a prefix


def test_fdiff_surface_and_state_dict_keys():
    import fastfourierdiffusion_amd as pkg

    pkg.install_as_fdiff(force=True)
    from fdiff.models.score_models import LSTMScoreModule, ScoreModule
    from fdiff.sampling.sampler import DiffusionSampler
    from fdiff.schedulers.sde import SDE, VEScheduler, VPScheduler
    from fdiff.utils.caching import E2CRFCache
    from fdiff.utils.dataclasses import DiffusableBatch
    from fdiff.utils.fourier import dft, idft  # noqa: F401
    from fastfourierdiffusion_amd.utils import synthetic

    sch = VPScheduler(beta_min=0.1, beta_max=20, fourier_noise_scaling=True)
    assert isinstance(sch, SDE) and sch.T == 1.0 and sch.eps == 1e-5
    sch.set_noise_scaling(187)
    sch.set_timesteps(1000)
    assert sch.G.shape == (187,) and sch.G_matrix.shape == (187, 187) and sch.timesteps.shape == (1000,)
    assert float(sch.step_size) == pytest.approx(0.0010010004, rel=1e-6)
    m = ScoreModule(n_channels=1, max_len=187, noise_scheduler=sch, d_model=72, num_layers=10, n_head=12)
    ref_keys = set(synthetic.transformer_state_dict(1, 187, 72, 10).keys())
    assert set(m.state_dict().keys()) == ref_keys
    assert sum(p.numel() for p in m.parameters()) == 3_202_413  # SURVEY: confirmed by import of the reference
    for a in ("max_len", "n_channels", "noise_scheduler", "num_training_steps", "d_model", "scale_noise", "cache",
              "use_cache", "cached_backbone", "device"):
        assert hasattr(m, a), a
    lm = LSTMScoreModule(n_channels=4, max_len=251, noise_scheduler=VPScheduler(), d_model=72, num_layers=10)
    assert set(lm.state_dict().keys()) == set(synthetic.lstm_state_dict(4, 251, 72, 10).keys())
    assert sum(p.numel() for p in lm.parameters()) == 426_424
    with pytest.raises(AttributeError):  # Q9: LSTM cannot enable caching
        lm.enable_caching()
    with pytest.raises(NotImplementedError):
        ScoreModule(n_channels=1, max_len=8, noise_scheduler=object())
    s = DiffusionSampler(score_model=m, sample_batch_size=50)
    for a in ("score_model", "noise_scheduler", "sample_batch_size", "n_channels", "max_len", "use_cache"):
        assert hasattr(s, a), a
    s2 = DiffusionSampler(score_model=m, sample_batch_size=1, use_cache=True, cache_kwargs={"K": 3, "R": 150})
    assert isinstance(m.cache, E2CRFCache) and m.cache.K == 3 and m.cache.R == 150 and m.use_cache
    first = m.cache
    DiffusionSampler(score_model=m, sample_batch_size=1, use_cache=True, cache_kwargs={})
    assert m.cache is not first and m._first_cache is first  # Q5
    assert set(m.cache.get_cache_stats()) == {"cache_hit_ratio", "cache_ratio", "recompute_count", "cache_hit_count",
                                              "current_step"}
    m.disable_caching()
    assert m.cache is None and not m.use_cache
    b = DiffusableBatch(X=torch.zeros(3, 5, 2), y=None, timesteps=torch.full((3,), 0.5))
    assert len(b) == 3 and b.device.type == "cpu"
    ve = VEScheduler(sigma_min=0.01, sigma_max=2)
    assert ve.sigma_max == 2 and ve.noise_scaling is False
    del s2


def test_same_seed_same_init_as_torch_reference_modules():
    """Equal torch seeds give the weights the reference would draw (same module
    construction order, score_models.py:55-66): checked against stock torch modules."""
    import math

    import torch.nn as nn

    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    torch.manual_seed(123)
    m = ScoreModule(n_channels=3, max_len=20, noise_scheduler=VPScheduler(), d_model=24, num_layers=2, n_head=4)
    torch.manual_seed(123)
    emb = nn.Embedding(20, 24, max_norm=math.sqrt(24))
    W = torch.randn(12) * 30.0
    dense = nn.Linear(24, 24)
    embedder = nn.Linear(3, 24)
    assert torch.equal(m.pos_encoder.embedding.weight, emb.weight)
    assert torch.equal(m.time_encoder.W, W)
    assert torch.equal(m.time_encoder.dense.weight, dense.weight)
    assert torch.equal(m.embedder.weight, embedder.weight)


def test_load_from_checkpoint_roundtrip(tmp_path):
    """cmd/sample.py:68-75 path: a Lightning-style checkpoint (hyper_parameters + state_dict, with the
    scheduler object pickled under the reference's module path) loads through the mirror.  No real
    checkpoint exists in this environment, so the file is synthesised here (parity unpinned)."""
    import fastfourierdiffusion_amd as pkg

    pkg.install_as_fdiff(force=True)
    from fdiff.models.score_models import LSTMScoreModule, ScoreModule
    from fdiff.schedulers.sde import VPScheduler

    sch = VPScheduler(beta_min=0.1, beta_max=20, fourier_noise_scaling=True)
    src = ScoreModule(n_channels=2, max_len=12, noise_scheduler=sch, d_model=24, num_layers=2, n_head=4)
    sd = dict(src.state_dict())
    sd["cached_backbone.0.linear1.weight"] = torch.zeros(3)  # left behind by enable_caching during training
    ckpt = {"state_dict": sd, "pytorch-lightning_version": "2.1.0", "epoch": 3,
            "hyper_parameters": dict(n_channels=2, max_len=12, noise_scheduler=sch, fourier_noise_scaling=True,
                                     d_model=24, num_layers=2, n_head=4, num_training_steps=1000, lr_max=1e-3,
                                     likelihood_weighting=False)}
    path = tmp_path / "epoch=3.ckpt"
    torch.save(ckpt, path)
    m = ScoreModule.load_from_checkpoint(checkpoint_path=str(path), weights_only=False)
    assert isinstance(m.noise_scheduler, VPScheduler) and m.noise_scheduler.beta_1 == 20 and m.max_len == 12
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    l_src = LSTMScoreModule(n_channels=2, max_len=12, noise_scheduler=sch, d_model=8, num_layers=2)
    torch.save({"state_dict": l_src.state_dict(),
                "hyper_parameters": dict(n_channels=2, max_len=12, noise_scheduler=sch, d_model=8, num_layers=2)},
               tmp_path / "l.ckpt")
    lm = LSTMScoreModule.load_from_checkpoint(tmp_path / "l.ckpt")
    assert torch.equal(lm.state_dict()["backbone.1.weight_hh_l0"], l_src.state_dict()["backbone.1.weight_hh_l0"])


def test_cpu_tensors_are_refused():
    from fastfourierdiffusion_amd._native import FFDError
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler
    from fastfourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fastfourierdiffusion_amd.utils.fourier import dft

    sch = VPScheduler()
    sch.set_noise_scaling(20)
    m = ScoreModule(n_channels=3, max_len=20, noise_scheduler=sch, d_model=24, num_layers=2, n_head=4)
    with pytest.raises(FFDError):
        m(DiffusableBatch(X=torch.zeros(2, 20, 3), timesteps=torch.ones(2)))
    with pytest.raises(AssertionError):
        m(DiffusableBatch(X=torch.zeros(2, 21, 3), timesteps=torch.ones(2)))
    if not torch.cuda.is_available():
        with pytest.raises(FFDError):
            dft(torch.zeros(2, 20, 3))
        with pytest.raises(FFDError):
            sch.step(torch.zeros(2, 20, 3), 0.5, torch.zeros(2, 20, 3))


_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
from fastfourierdiffusion_amd.sharding import shard_range, reduce_max_seconds, gather_seconds
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
off, cnt = shard_range(1001, 2, rank)
t = reduce_max_seconds(0.5 + rank, None)
per_rank = gather_seconds(0.5 + rank, None)
gathered = [None, None]
dist.all_gather_object(gathered, (off, cnt))
if rank == 0:
    print(json.dumps({{"ranges": gathered, "tmax": t, "per_rank": per_rank}}))
dist.destroy_process_group()
"""


def test_shard_plan_two_ranks_gloo(tmp_path):
    from fastfourierdiffusion_amd.sharding import shard_range

    # pure function: contiguous, disjoint, covering, balanced within 1
    for n, w in ((1001, 2), (65536, 8), (7, 8), (512, 1)):
        rs = [shard_range(n, w, r) for r in range(w)]
        assert rs[0][0] == 0 and sum(c for _, c in rs) == n
        assert all(rs[i][0] + rs[i][1] == rs[i + 1][0] for i in range(w - 1))
        assert max(c for _, c in rs) - min(c for _, c in rs) <= 1
    script = tmp_path / "w.py"
    port = 29000 + (os.getpid() % 2000)
    script.write_text(_WORKER.format(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    import json

    res = json.loads(outs[0].strip().splitlines()[-1])
    assert res["ranges"] == [[0, 501], [501, 500]] and res["tmax"] == 1.5 and res["per_rank"] == [0.5, 1.5]


def test_bench_self_launcher_rank_plan():
    """`python bench.py --gpus N` (the form the driver uses) must start N ranks by itself: the parent prints the
    plan with --launch-plan (no GPU, no torch import), one fresh child per GPU with RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set; a WORLD_SIZE that disagrees with --gpus is refused instead of silently timing one GPU."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--launch-plan", "--workload",
                        "syn512", "--batch", "8192", "--cache"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert plan["n_gpus"] == 8 and len(plan["ranks"]) == 8
    ports = {p["env"]["MASTER_PORT"] for p in plan["ranks"]}
    assert len(ports) == 1 and int(ports.pop()) > 0
    for i, p in enumerate(plan["ranks"]):
        e = p["env"]
        assert (p["rank"], e["RANK"], e["LOCAL_RANK"], e["WORLD_SIZE"], e["MASTER_ADDR"]) == (i, str(i), str(i), "8", "127.0.0.1")
        assert p["cmd"][1].endswith("bench.py") and "--launch-plan" not in p["cmd"]
        assert p["cmd"][2:] == ["--gpus", "8", "--workload", "syn512", "--batch", "8192", "--cache"]
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                         env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE=2" in bad.stderr


def test_bench_self_launcher_relays_rank0_and_fails_on_child_failure(tmp_path, monkeypatch):
    """The launcher itself, with stand-in children: rank 0's JSON line is relayed, a failing rank fails the run."""
    import importlib
    import io
    import contextlib

    bench = importlib.import_module("bench")
    child = tmp_path / "child.py"
    child.write_text("import os, sys, json\n"
                     "r = int(os.environ['RANK'])\n"
                     "if r == 0: print('noise'); print(json.dumps({'n_gpus': int(os.environ['WORLD_SIZE']), 'rank': r}))\n"
                     "sys.exit(3 if os.environ.get('FAIL_RANK') == str(r) else 0)\n")

    def fake_plan(n, argv, port):
        return [{"rank": r, "cmd": [sys.executable, str(child)],
                 "env": {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n)}} for r in range(n)]

    monkeypatch.setattr(bench, "launch_plan", fake_plan)
    args = bench.parse_args(["--gpus", "3"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert bench.self_launch(args, ["--gpus", "3"]) == 0
    import json

    assert json.loads(buf.getvalue().strip()) == {"n_gpus": 3, "rank": 0}
    monkeypatch.setenv("FAIL_RANK", "2")
    with contextlib.redirect_stdout(io.StringIO()):
        assert bench.self_launch(args, ["--gpus", "3"]) != 0


def test_bench_full_option_and_dump_outputs(tmp_path):
    """A plain bench run times the steps only (--full adds the side measurements, --ablation needs it); --dump-outputs
    writes the samples as float32, a fixed seeded subset of batch rows past the size budget, one file per rank."""
    import importlib

    bench = importlib.import_module("bench")
    assert not bench.parse_args([]).full and bench.parse_args(["--full", "--ablation"]).ablation
    with pytest.raises(SystemExit):
        bench.parse_args(["--ablation"])
    x = torch.arange(512 * 187, dtype=torch.float32).reshape(512, 187, 1)
    bench.dump_outputs(str(tmp_path / "a"), x, 0, 1)
    assert np.array_equal(np.load(tmp_path / "a" / "samples.npy"), x.numpy())
    big = torch.randn(8192, 512, 8)
    for r in range(2):
        bench.dump_outputs(str(tmp_path / "b"), big, r, 2)
    parts = [np.load(tmp_path / "b" / f"samples_rank{r}.npy") for r in range(2)]
    assert sum(p.nbytes for p in parts) <= bench.DUMP_BYTES and parts[0].dtype == np.float32
    assert np.array_equal(parts[0], parts[1]) and parts[0].shape[1:] == (512, 8)
    assert any(np.array_equal(parts[0][0], big[i].numpy()) for i in range(big.shape[0]))


def test_hydra_surface_targets_resolve_and_instantiate():
    """The north_star's "Hydra-config API surface": the reference pins it by composing and instantiating every
    cmd/conf/*.yaml (tests/test_hydra_configs.py:21-51).  hydra / omegaconf are not installed here, so the same
    check runs on tests/golden/hydra_targets.json -- the `_target_` strings, `_partial_` flags and kwargs extracted
    from cmd/conf/{sampler,score_model,score_model/noise_scheduler}/*.yaml by oracle/gen_hydra_targets.py -- through
    install_as_fdiff() and the package's own instantiate()."""
    import functools
    import json

    import fastfourierdiffusion_amd as pkg
    from fastfourierdiffusion_amd.utils.extraction import get_model_type, instantiate

    pkg.install_as_fdiff(force=True)
    tg = json.load(open(os.path.join(ROOT, "tests", "golden", "hydra_targets.json")))

    def resolved(name, fourier):
        e = tg[name]
        cfg = {"_target_": e["_target_"], "_partial_": e["_partial_"]}
        # OmegaConf reads `1e-5` as a float where PyYAML's YAML-1.1 resolver leaves a string
        cfg.update({k: (float(v) if isinstance(v, str) and re.fullmatch(r"[0-9.]+e-?[0-9]+", v) else v)
                    for k, v in e["kwargs"].items()})
        for k in e["interpolated"]:  # ${fourier_transform} / ${score_model.fourier_noise_scaling}
            cfg[k] = fourier
        return cfg

    assert tg["sample"]["use_cache"] is False and tg["sample"]["cache_kwargs"] == {}
    for fourier in (True, False):
        for model_cfg in ("score_model/default", "score_model/lstm", "score_model/mlp"):
            for sched in ("vpsde", "vesde"):
                cfg = resolved(model_cfg, fourier)
                cfg["noise_scheduler"] = resolved(f"score_model/noise_scheduler/{sched}", fourier)
                assert cfg["_target_"].startswith("fdiff.models.score_models.")
                model_partial = instantiate(cfg)
                assert isinstance(model_partial, functools.partial)
                model = model_partial(n_channels=2, max_len=24, num_training_steps=10)  # cmd/train.py:47-51
                assert type(model) is get_model_type({"score_model": cfg})
                assert model.d_model == 72 and model.num_layers == 10 and model.scale_noise is fourier
                sch = model.noise_scheduler
                assert type(sch).__name__ == ("VPScheduler" if sched == "vpsde" else "VEScheduler")
                assert sch.noise_scaling is fourier and sch.eps == 1e-5
                if sched == "vpsde":
                    assert (sch.beta_0, sch.beta_1) == (0.1, 20)  # sde.py:184-185
                else:
                    assert (sch.sigma_min, sch.sigma_max) == (0.01, 2)
                sampler_partial = instantiate(resolved("sampler/default", fourier))
                sampler = sampler_partial(score_model=model)  # cmd/sample.py:80-91
                assert type(sampler).__module__.endswith("sampling.sampler") and sampler.sample_batch_size == 50
                if model_cfg == "score_model/default":
                    cached = sampler_partial(score_model=model, use_cache=True, cache_kwargs={"K": 3})
                    assert cached.use_cache and model.cache.K == 3
                    model.disable_caching()


def test_extraction_helpers_on_a_synthetic_run_directory(tmp_path):
    """utils/extraction.py:20-121 as cmd/sample.py:52-75 uses it: best checkpoint by val_loss, model class from the
    training config, flatten / pretty-print.  No real lightning_logs exist here, so the tree is synthesised."""
    from fastfourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule
    from fastfourierdiffusion_amd.utils import extraction as ex

    ck = tmp_path / "lightning_logs" / "abc123" / "checkpoints"
    ck.mkdir(parents=True)
    for name in ("epoch=3-val_loss=0.52.ckpt", "epoch=17-val_loss=0.07.ckpt", "epoch=40-val_loss=0.30.ckpt",
                 "last.ckpt", "epoch=99-val_loss=0.01.txt"):
        (ck / name).write_bytes(b"")
    assert ex.get_best_checkpoint(ck).name == "epoch=17-val_loss=0.07.ckpt"
    with pytest.raises(UnboundLocalError):  # the reference returns an unbound local when nothing matches
        ex.get_best_checkpoint(tmp_path)
    for tgt, cls in (("ScoreModule", ScoreModule), ("MLPScoreModule", MLPScoreModule), ("LSTMScoreModule", LSTMScoreModule)):
        assert ex.get_model_type({"score_model": {"_target_": f"fdiff.models.score_models.{tgt}"}}) is cls
    with pytest.raises(NotImplementedError):
        ex.get_model_type({"score_model": {"_target_": "fdiff.models.score_models.Other"}})
    cfg = {"random_seed": 42, "fourier_transform": True,
           "score_model": {"_target_": "fdiff.models.score_models.ScoreModule", "_partial_": True, "d_model": 72,
                           "noise_scheduler": {"_target_": "fdiff.schedulers.sde.VPScheduler", "beta_min": 0.1}},
           "trainer": {"callbacks": [{"_target_": "pl.callbacks.ModelCheckpoint", "monitor": "val/loss"},
                                     {"_target_": "pl.callbacks.LearningRateMonitor"}], "max_epochs": 200}}
    flat = ex.flatten_config(cfg)
    assert flat == {"random_seed": 42, "fourier_transform": True, "score_model": "fdiff.models.score_models.ScoreModule",
                    "d_model": 72, "noise_scheduler": "fdiff.schedulers.sde.VPScheduler", "beta_min": 0.1,
                    "callbacks": ["pl.callbacks.ModelCheckpoint", "pl.callbacks.LearningRateMonitor"],
                    "monitor": "val/loss", "max_epochs": 200}
    text = ex.dict_to_str({"a": 1, "long_list": [1, 2, 3, 4, 5]})
    assert "[1, 2, 3, '...']" in text and text.count("\n") == 2

    class DM:
        dataset_parameters = {"n_channels": 1, "max_len": 187, "num_training_steps": 100}

    class TR:
        max_epochs, accumulate_grad_batches = 200, 4

    assert ex.get_training_params(DM(), TR())["num_training_steps"] == 5000


def test_isa_lint_finds_dropped_accumulator_copies_and_clobbered_fragments(tmp_path):
    """tools/check_mfma_operands.py on hand-made ISA: the two signatures of the hipcc 7.2 miscompile seen in
    k_oproj_ffn_split (a VGPR -> AGPR copy turned into a no-op; a prefetched weight fragment member overwritten
    while its siblings are still read) are reported, ordinary register reuse is not."""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_mfma_operands.py")
    bad = tmp_path / "bad.s"
    bad.write_text("""_Z3badv:
	global_load_dwordx4 v[24:27], v[14:15], off
                                        ; kill: def $agpr8 killed $vgpr44 killed $exec
	v_accvgpr_read_b32 v25, a8
	v_mfma_f32_16x16x4_f32 a[12:15], v24, v16, a[12:15]
	v_mfma_f32_16x16x4_f32 a[12:15], v25, v16, a[12:15]
	v_mfma_f32_16x16x4_f32 a[12:15], v26, v16, a[12:15]
	s_endpgm
""")
    ok = tmp_path / "ok.s"
    ok.write_text("""_Z2okv:
	global_load_dwordx4 v[24:27], v[14:15], off
	v_mfma_f32_16x16x4_f32 a[12:15], v24, v16, a[12:15]
	v_max_f32_e32 v24, 0, v30
	v_mfma_f32_16x16x4_f32 a[12:15], v25, v24, a[12:15]
	v_mfma_f32_16x16x4_f32 a[12:15], v26, v24, a[12:15]
	s_endpgm
""")
    r = subprocess.run([sys.executable, tool, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "dropped accumulator copy" in r.stdout and "v25 overwritten" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, tool, str(ok)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 suspicious" in r.stdout, r.stdout


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_isa_lint_clean_on_every_kernel_source():
    """make lint: the gfx950 ISA of every csrc/*.hip carries neither signature."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastfourierdiffusion_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "lint", "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # The hot kernels' register budgets, from the metadata of the same ISA files: the row-owning FFN keeps its 50-group
    # fragment stream unrolled (past LLVM's default full-unroll budget it stays a loop, indexes the fragment array at run
    # time and goes to ~1 KB of scratch: 6-10 ms launches) and the instances the ECG and config-5 benches launch
    # (12 and 8 waves, two-chunk slots) hold no scratch inside their slot loops: at most the 88 B of the multi-tile
    # fused form's tile boundaries; the LSTM wavefront at d_model 72 holds none.
    import re

    def kernels(path):
        txt = open(path).read()
        names = re.findall(r"^\s+\.name:\s+(\S+)", txt, re.M)
        priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", txt, re.M)
        assert len(names) == len(priv)
        return dict(zip(names, map(int, priv)))

    rows = {k: v for k, v in kernels(os.path.join(csrc, ".isa", "ffd_ffn_rows.s")).items() if "k_ffn_rows" in k}
    assert len(rows) >= 10
    for name, scratch in rows.items():
        assert scratch <= 128, (name, scratch)
        if "ELb1EEEv" in name:  # one tile per workgroup (the ECG B = 512 launch): nothing spilled at all
            assert scratch == 0, (name, scratch)
    wave = {k: v for k, v in kernels(os.path.join(csrc, ".isa", "ffd_lstm.s")).items() if "k_lstm_waveILi72E" in k}
    assert wave and all(v == 0 for v in wave.values()), wave



def test_tune_knobs_are_per_thread():
    """ffd_tune's knobs are thread_local (round 4): a value set on one thread is neither seen nor overwritten by another,
    a new thread starts from the defaults, and "reset" restores the calling thread's table only.  (No device needed.)"""
    import ctypes as C
    import threading

    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()

    def get(key):
        v = C.c_int(-12345)
        assert lib.ffd_tune_get(key, C.byref(v)) == 0, key
        return v.value

    assert lib.ffd_tune(b"reset", 0) == 0
    defaults = {k: get(k) for k in (b"ffn_rows_nw", b"rows_slices", b"lstm_wave_spin_ms", b"attn_hpw", b"ffn_rows")}
    assert defaults[b"lstm_wave_spin_ms"] == 2000 and defaults[b"ffn_rows"] == 1
    assert lib.ffd_tune(b"ffn_rows_nw", 8) == 0 and lib.ffd_tune(b"rows_slices", 4) == 0
    seen, go, done = {}, threading.Event(), threading.Event()

    def other():
        seen["start"] = {k: get(k) for k in defaults}           # a fresh thread: defaults, not the main thread's 8 / 4
        assert lib.ffd_tune(b"ffn_rows_nw", 12) == 0 and lib.ffd_tune(b"attn_hpw", 1) == 0
        go.set()
        done.wait(10)
        seen["end"] = {k: get(k) for k in defaults}             # untouched by the main thread's reset

    t = threading.Thread(target=other)
    t.start()
    assert go.wait(10)
    assert get(b"ffn_rows_nw") == 8 and get(b"rows_slices") == 4 and get(b"attn_hpw") == defaults[b"attn_hpw"]
    assert lib.ffd_tune(b"reset", 0) == 0
    assert {k: get(k) for k in defaults} == defaults
    done.set()
    t.join(10)
    assert seen["start"] == defaults
    assert seen["end"][b"ffn_rows_nw"] == 12 and seen["end"][b"attn_hpw"] == 1 and seen["end"][b"rows_slices"] == defaults[b"rows_slices"]
    assert lib.ffd_tune_get(b"no_such_knob", C.byref(C.c_int())) != 0
