"""CPU-side tests of class-conditional score models and classifier-free guidance (no GPU): the new C-ABI symbols are
exported and bound like include/ffd.h declares them, every argument error and refusal comes back before any device work,
the Python surface refuses what it cannot run, ``ClassConditionalScoreModule`` keeps ``ScoreModule``'s state-dict keys
and round-trips a checkpoint, labels are sliced per batch, and the judge of the device tests
(tests/class_restatement.py) is sound: the one-hot forward is the network with ``+ table[y]`` written out, its table
gradient is a finite difference's, and the restated label dropout has its rate and is keyed by the global row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import class_restatement as CL
import philox_restatement as PR
import train_restatement as TR
from conftest import rel_err
from fastfourierdiffusion_amd.utils import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ffd_class_enable", "ffd_class_disable", "ffd_class_temb", "ffd_cfg_combine", "ffd_class_drop",
               "ffd_class_table_grad", "ffd_train_classes", "ffd_train_labels")
INVALID, UNSUPPORTED, STATE = -1, -2, -3
P_ = 0x1000  # dummies, never dereferenced
A_, B_, T_, Y_, O_ = (P_ * k for k in range(1, 6))


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _header_decl(name):
    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"^(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared in include/ffd.h"
    return m.group(1), [" ".join(re.sub(r"/\*.*?\*/", "", p).split()) for p in m.group(2).split(",")]


def _ctype_of(param):
    if "*" in param or "[" in param:
        return "pointer"
    return {"double": C.c_double, "float": C.c_float, "int": C.c_int, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "size_t": C.c_size_t}[param.split()[-2]]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_exported_and_bound_like_the_header(lib, name):
    from fastfourierdiffusion_amd import _native

    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, re.M), f"{name} is not exported"
    res, args = _native.SIGNATURES[name]
    ret, params = _header_decl(name)
    assert res is C.c_int and ret == "int" and len(args) == len(params), (name, len(args), params)
    for a, p in zip(args, params):
        want = _ctype_of(p)
        if want == "pointer":
            assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
        else:
            assert a is want, (name, p, a)
    assert getattr(lib, name).argtypes == args


def test_class_cfg_layout_tag_and_documents():
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} ffd_class_cfg;", header)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl).strip()
        if decl:
            fields.append(decl.split()[-1].lstrip("*"))
    assert fields == [f[0] for f in N.ClassCfg._fields_] == ["table", "labels", "labels_host", "n_classes", "n_labels",
                                                             "guidance_scale", "reserved"]
    assert C.sizeof(N.ClassCfg) == 3 * 8 + 4 * 4
    assert [getattr(N.ClassCfg, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 36]
    # the dropout's stream tag: named next to SM_TAG_*, free between loglik's probes and the loss's reserved tags
    internal = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "ffd_internal.h")).read()
    assert re.search(r"SM_TAG_CLASS_DROP\s*=\s*0xFFFFFFFCu", internal)
    assert CL.TAG_CLASS_DROP == 0xFFFFFFFC and CL.TAG_CLASS_DROP not in PR.RESERVED and CL.TAG_CLASS_DROP > 0xFFFFFFF0
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS + ("ffd_class_cfg",):
        assert name in integration, f"{name} is missing from INTEGRATION.md"
    assert "ffd_class.hip" in open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the operators' argument errors: no device work ----
def test_operators_refuse_bad_arguments_without_a_device(lib):
    def temb(t=A_, stride=8, table=T_, nc=3, y=Y_, B=2, d=8, stack=0, out=O_):
        return lib.ffd_class_temb(t, stride, table, nc, y, B, d, stack, out, None)

    for bad in (dict(t=None), dict(table=None), dict(out=None), dict(B=0), dict(d=0), dict(nc=0), dict(stride=4),
                dict(stride=-8), dict(out=T_), dict(out=A_, stride=0), dict(out=A_, stack=1)):
        assert temb(**bad) == INVALID, bad

    def combine(c=A_, u=B_, g=2.5, n=16):
        return lib.ffd_cfg_combine(c, u, g, n, None)

    for bad in (dict(c=None), dict(u=None), dict(u=A_), dict(n=0), dict(g=float("nan")), dict(g=float("inf")),
                dict(c=A_ + 2), dict(u=B_ + 1)):
        assert combine(**bad) == INVALID, bad

    def drop(y=Y_, nc=3, idx=None, B=4, p=0.1, out=O_):
        return lib.ffd_class_drop(y, nc, idx, B, p, 7, 0, out, None)

    for bad in (dict(out=None), dict(B=0), dict(nc=0), dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(out=Y_)):
        assert drop(**bad) == INVALID, bad

    def grad(dt=A_, y=Y_, nc=3, B=4, d=8, out=O_):
        return lib.ffd_class_table_grad(dt, y, nc, B, d, out, None)

    for bad in (dict(dt=None), dict(y=None), dict(out=None), dict(nc=0), dict(B=0), dict(d=0)):
        assert grad(**bad) == INVALID, bad


# ------------------------------------------------------------------- the context state: refusals without a device ----
def _create(lib, kind=0, L=5, Cn=1, d=8, H=2, NL=2, F=64):
    from fastfourierdiffusion_amd import _native as N

    desc = N.ModelDesc(kind, Cn, L, d, H, NL, F, 0, 0.1, 20.0, 1, 1e-5)
    h = C.c_void_p()
    lib.ffd_create(C.byref(h), C.byref(desc), 0)  # (without a device: FFD_ERR_HIP, the context is returned all the same)
    assert h.value
    return h


def _cfg(labels=(0, 1, 2), n_classes=3, g=1.0, table=T_, dev=Y_, n=None):
    from fastfourierdiffusion_amd import _native as N

    host = (C.c_int32 * len(labels))(*labels) if labels is not None else None
    cfg = N.ClassCfg(table, dev if labels is not None else None, C.cast(host, C.c_void_p) if host is not None else None,
                     n_classes, len(labels) if n is None and labels is not None else (n or 0), g, 0)
    cfg._keep = host
    return cfg


def test_class_enable_refuses_bad_configurations(lib):
    from fastfourierdiffusion_amd import _native as N

    h = _create(lib)
    assert lib.ffd_class_enable(None, C.byref(_cfg())) == INVALID and lib.ffd_class_disable(None) == INVALID
    assert lib.ffd_class_enable(h, None) == INVALID
    for bad in (dict(table=None), dict(n_classes=0), dict(g=float("nan")), dict(g=float("inf")), dict(labels=(0, 4, 1)),
                dict(labels=(0, -2, 1)), dict(n=0)):
        assert lib.ffd_class_enable(h, C.byref(_cfg(**bad))) == INVALID, bad
    no_host = N.ClassCfg(T_, Y_, None, 3, 3, 1.0, 0)  # device labels without their host copy
    assert lib.ffd_class_enable(h, C.byref(no_host)) == INVALID
    assert b"labels_host" in lib.ffd_last_error(h)
    for ok in (dict(), dict(labels=(-1, 3, 0)), dict(labels=None), dict(g=0.0), dict(g=-1.5), dict(g=2.5)):
        assert lib.ffd_class_enable(h, C.byref(_cfg(**ok))) == 0, ok
    assert lib.ffd_class_disable(h) == 0
    lib.ffd_destroy(h)
    mix = _create(lib, kind=3, L=8, d=0, H=0, NL=0, F=3)
    assert lib.ffd_class_enable(mix, C.byref(_cfg())) == UNSUPPORTED
    lib.ffd_destroy(mix)


def _loops(lib, h, B, use_cache=0):
    """every sampling-loop entry at batch B on dummies -> {name: status}"""
    from fastfourierdiffusion_amd import _native as N

    ts = (C.c_float * 6)(*np.linspace(1.0, 1e-5, 6))
    grid = (h, A_, B, ts, 6, 0.2, 0, 1)
    cond = N.CondCfg(B_, T_, None, 1, 1, 1, 0)
    out = {"ffd_sample_batch": lib.ffd_sample_batch(*grid, 1, 0, None, use_cache, 0, None),
           "ffd_sample_batch_pc": lib.ffd_sample_batch_pc(*grid, 1, 0.16, 0, 1, 0, None, use_cache, 0, None),
           "ffd_sample_batch_cond": lib.ffd_sample_batch_cond(*grid, 0, 0.16, 0, 1, 0, None, use_cache, 0, C.byref(cond), None)}
    for solver in (1, 2, 4, 5):
        out[f"ffd_sample_batch_ode[{solver}]"] = lib.ffd_sample_batch_ode(*grid, solver, use_cache, 0, None)
    if not use_cache:
        out["ffd_sample_batch_resample"] = lib.ffd_sample_batch_resample(*grid, 2, 2, 0, 0.16, 0, 1, 0, None, C.byref(cond), None)
    return out


def test_context_refusals_come_before_any_device_work(lib):
    """On a context whose weights were never loaded every entry would answer FFD_ERR_STATE 'not finalised': the class
    checks come first, so their own status and message are what is seen -- with or without a device."""
    from fastfourierdiffusion_amd import _native as N

    h = _create(lib)
    assert lib.ffd_class_enable(h, C.byref(_cfg(labels=(0, 1, 2), g=2.5))) == 0
    for name, rc in _loops(lib, h, B=4).items():  # n_labels != B
        assert rc == INVALID and b"3 labels for a batch of 4" in lib.ffd_last_error(h), (name, rc, lib.ffd_last_error(h))
    assert lib.ffd_score_forward_ts(h, A_, B_, O_, None, 4, -1, None) == INVALID
    assert lib.ffd_sm_eval_batch(h, A_, B_, T_, T_, None, 0, 0, 0, 1, O_, 4, None) == INVALID
    for name, rc in _loops(lib, h, B=3, use_cache=1).items():  # the cache
        assert rc == STATE and b"class conditioning" in lib.ffd_last_error(h), (name, rc, lib.ffd_last_error(h))
    assert lib.ffd_score_forward_ts(h, A_, B_, O_, None, 3, 2, None) == STATE and b"class" in lib.ffd_last_error(h)
    # the entries without a class form
    assert lib.ffd_score_forward(h, A_, 0.5, O_, 3, None) == STATE and b"class" in lib.ffd_last_error(h)
    assert lib.ffd_score_forward_cached(h, A_, 0.5, O_, None, 3, 0, None) == STATE and b"class" in lib.ffd_last_error(h)
    ts = (C.c_float * 6)(*np.linspace(1.0, 1e-5, 6))
    assert lib.ffd_loglik_batch(h, A_, B_, 3, ts, 6, 0, 1, 1, 1, 1e-2, None, 0, 0, None) == STATE
    assert b"ffd_loglik_batch has no class-conditional form" in lib.ffd_last_error(h)
    cond, guide = N.CondCfg(B_, T_, None, 1, 1, 1, 0), N.GuideCfg(1.0, 1.0, 0.0, 0, 0)
    assert lib.ffd_sample_batch_guided(h, None, A_, 3, ts, 6, 0.2, 0, 1, 1, 0, None, C.byref(cond), C.byref(guide), None,
                                       None) == STATE
    assert b"ffd_sample_batch_guided has no class-conditional form" in lib.ffd_last_error(h)
    # with matching labels the class checks pass, and the unfinalised context is what the entries then report
    for name, rc in _loops(lib, h, B=3).items():
        assert rc == STATE and b"not finalised" in lib.ffd_last_error(h), (name, rc)
    # disabled: as before
    assert lib.ffd_class_disable(h) == 0
    assert lib.ffd_score_forward(h, A_, 0.5, O_, 3, None) == STATE and b"not finalised" in lib.ffd_last_error(h)
    lib.ffd_destroy(h)


def test_training_entries_refuse_bad_arguments(lib):
    from fastfourierdiffusion_amd import _native as N

    desc = N.ModelDesc(0, 1, 5, 8, 2, 2, 64, 0, 0.1, 20.0, 1, 1e-5)
    h = C.c_void_p()
    lib.ffd_train_create(C.byref(h), C.byref(desc), 0.0, 0)
    assert h.value
    assert lib.ffd_train_classes(None, 3) == INVALID and lib.ffd_train_labels(None, Y_, 3, 0.1) == INVALID
    assert lib.ffd_train_labels(h, Y_, 3, 0.1) == STATE  # no classes yet
    assert lib.ffd_train_classes(h, 0) == INVALID
    assert lib.ffd_train_bind(h, b"class_embedding.weight", A_, B_, T_, O_, 32) == INVALID  # unknown before the call
    assert lib.ffd_train_classes(h, 3) == 0
    assert lib.ffd_train_classes(h, 3) == INVALID  # twice
    for bad in (dict(n=0), dict(p=-0.1), dict(p=1.1), dict(p=float("nan"))):
        assert lib.ffd_train_labels(h, Y_, bad.get("n", 3), bad.get("p", 0.1)) == INVALID, bad
    assert lib.ffd_train_labels(h, Y_, 3, 0.0) == 0 and lib.ffd_train_labels(h, None, 0, 1.0) == 0
    assert lib.ffd_train_bind(h, b"class_embedding.weight", A_, B_, T_, O_, 31) == INVALID  # (3 + 1) x 8 elements
    assert lib.ffd_train_bind(h, b"class_embedding.weight", A_, B_, T_, O_, 32) == 0
    lib.ffd_train_destroy(h)
    # after a bind the tensor list is closed
    lib.ffd_train_create(C.byref(h), C.byref(desc), 0.0, 0)
    assert lib.ffd_train_bind(h, b"embedder.bias", A_, B_, T_, O_, 8) == 0
    assert lib.ffd_train_classes(h, 3) == STATE
    lib.ffd_train_destroy(h)
    # the workspace size does not know about classes: the effective labels live outside it
    assert lib.ffd_train_work_bytes(C.byref(desc), 3) > 0


# ----------------------------------------------------------------------------------------------- the Python surface ----
def _model(n_classes=3, **kw):
    from fastfourierdiffusion_amd.models.score_models import ClassConditionalScoreModule
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler

    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(5)
    torch.manual_seed(3)
    return ClassConditionalScoreModule(n_channels=1, max_len=5, noise_scheduler=sch, n_classes=n_classes, d_model=8,
                                       num_layers=2, n_head=2, **kw)


def test_module_keys_initialisation_and_native_weights():
    from fastfourierdiffusion_amd.models.score_models import ScoreModule

    m = _model()
    base = ScoreModule(n_channels=1, max_len=5, noise_scheduler=m.noise_scheduler, d_model=8, num_layers=2, n_head=2)
    assert set(m.state_dict()) == set(base.state_dict()) | {"class_embedding.weight"}
    assert tuple(m.class_embedding.weight.shape) == (4, 8)
    assert [n for n, _ in m._weight_items()] == [n for n, _ in base._weight_items()]  # the context never sees the table
    torch.manual_seed(0)
    big = _model(n_classes=200)
    assert abs(float(big.class_embedding.weight.std()) - 0.02) < 2e-3  # N(0, 0.02^2)
    with pytest.raises(AssertionError):
        _model(n_classes=0)


def test_labels_are_validated_and_sliced_per_batch():
    from fastfourierdiffusion_amd.models.score_models import class_labels
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    y = class_labels([0, 1, 2, -1, 3, 1, 0], 7, 3, "cpu")
    assert y.dtype == torch.int32 and y.tolist() == [0, 1, 2, -1, 3, 1, 0]
    assert class_labels(2, 4, 3, "cpu").tolist() == [2, 2, 2, 2] and class_labels(None, 4, 3, "cpu") is None
    for bad in ([0, 4], [0, -2], [0.0, 1.0], [True, False]):
        with pytest.raises(AssertionError):
            class_labels(bad, 2, 3, "cpu")
    with pytest.raises(AssertionError):
        class_labels([0, 1, 2], 4, 3, "cpu")
    # batches of 3 over 7 samples: the slices of the loop (the remainder is dropped by the sampler, as ever)
    assert [DiffusionSampler._label_slice(y, lo, 3).tolist() for lo in (0, 3)] == [[0, 1, 2], [-1, 3, 1]]
    assert DiffusionSampler._label_slice(None, 0, 3) is None


def test_python_refusals():
    from fastfourierdiffusion_amd.models.score_models import ScoreModule
    from fastfourierdiffusion_amd.sampling.guidance import Guidance
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler

    m = _model()
    s = DiffusionSampler(m, sample_batch_size=2)
    with pytest.raises(NotImplementedError):
        s.log_likelihood(torch.zeros(2, 5, 1), 4, labels=[0, 1])
    with pytest.raises(NotImplementedError):
        s.sample_conditional(torch.zeros(5, 1), torch.ones(5), 2, 4, labels=[0, 1], guidance=Guidance(scale=1.0))
    with pytest.raises(NotImplementedError):
        s.impute(torch.zeros(5, 1), torch.ones(5), 2, 4, labels=[0, 1], guidance=Guidance(scale=1.0))
    with pytest.raises(ValueError):
        s.sample(2, 4, labels=[0, 1], guidance_scale=float("nan"))
    with pytest.raises(AssertionError):
        s.sample(2, 4, labels=[0, 5])
    with pytest.raises(TypeError):
        s.sample_conditional(torch.zeros(5, 1), torch.ones(5), 2, 4, label=[0, 1])
    cached = DiffusionSampler(_model(), sample_batch_size=2, use_cache=True, cache_kwargs={})
    with pytest.raises(NotImplementedError):
        cached.sample(2, 4, labels=[0, 1])
    # a model without classes takes no labels
    plain = ScoreModule(n_channels=1, max_len=5, noise_scheduler=m.noise_scheduler, d_model=8, num_layers=2, n_head=2)
    with pytest.raises(AssertionError):
        DiffusionSampler(plain, sample_batch_size=2).sample(2, 4, labels=[0, 1])
    with pytest.raises(AssertionError):
        DiffusionSampler(plain, sample_batch_size=2).sample(2, 4, guidance_scale=2.0)


def test_checkpoint_round_trip(tmp_path):
    """What Trainer.save_checkpoint writes for the module (hyper_parameters from the subclass's signature + state_dict),
    read back by load_from_checkpoint."""
    from fastfourierdiffusion_amd.models.score_models import ClassConditionalScoreModule
    from fastfourierdiffusion_amd.training import Trainer

    m = _model(lr_max=2e-3)
    hp = Trainer.hyper_parameters(type("T", (), {"model": m})())
    assert hp["n_classes"] == 3 and hp["d_model"] == 8 and hp["fourier_noise_scaling"] is True
    path = tmp_path / "c.ckpt"
    torch.save({"state_dict": {k: v.clone() for k, v in m.state_dict().items()}, "hyper_parameters": hp}, path)
    back = ClassConditionalScoreModule.load_from_checkpoint(path)
    assert back.n_classes == 3 and back.lr_max == 2e-3
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


# ------------------------------------------------------------------------------------------------------ the judge ----
TF = dict(kind="transformer", L=5, C=1, d=8, H=2, NL=2, F=64, B=5)
MLP = dict(kind="mlp", L=4, C=2, d=8, H=1, NL=2, F=16, B=5)
LSTM = dict(kind="lstm", L=4, C=2, d=8, H=1, NL=2, B=5)


def _sd(c, seed=21):
    if c["kind"] == "transformer":
        sd = synthetic.transformer_state_dict(c["C"], c["L"], c["d"], c["NL"], dim_feedforward=c["F"], seed=seed)
    elif c["kind"] == "mlp":
        sd = synthetic.mlp_state_dict(c["C"], c["L"], c["d"], c["F"], c["NL"], seed=seed)
    else:
        sd = synthetic.lstm_state_dict(c["C"], c["L"], c["d"], c["NL"], seed=seed)
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


@pytest.mark.parametrize("c", [TF, MLP], ids=lambda c: c["kind"])
def test_one_hot_judge_is_the_network_with_the_row_added(c):
    rng = np.random.default_rng(5)
    sd, table = _sd(c), 0.3 * rng.standard_normal((4, c["d"])).astype(np.float32)
    x = rng.standard_normal((c["B"], c["L"], c["C"])).astype(np.float32)
    t = rng.uniform(0.05, 1.0, c["B"]).astype(np.float32)
    for variant in (0, 1):
        y = CL.labels_for(c["B"], variant)
        a = CL.forward_np(c["kind"], x, t, sd, table, y, c["NL"], c["H"])
        b = CL.forward_direct(c["kind"], x, t, sd, table, y, c["NL"], c["H"])
        assert rel_err(a, b) < 1e-13, (c["kind"], variant, rel_err(a, b))
    # None is every label null; a zero table is the plain network
    null = CL.forward_np(c["kind"], x, t, sd, table, None, c["NL"], c["H"])
    assert np.array_equal(null, CL.forward_np(c["kind"], x, t, sd, table, np.full(c["B"], 3), c["NL"], c["H"]))
    assert np.array_equal(null, CL.forward_np(c["kind"], x, t, sd, table, np.full(c["B"], -1), c["NL"], c["H"]))
    assert rel_err(a, null) > 1e-3  # the labels matter at this table


def test_one_hot_judge_for_the_lstm_adds_the_row_to_the_embedding():
    """The LSTM has no written-out twin here: a table whose rows all equal v is the network with v added to the time
    encoder's bias, whatever the labels."""
    c = LSTM
    rng = np.random.default_rng(6)
    sd = _sd(c)
    v = 0.3 * rng.standard_normal(c["d"]).astype(np.float32)
    table = np.tile(v, (4, 1))
    x = rng.standard_normal((c["B"], c["L"], c["C"])).astype(np.float32)
    t = rng.uniform(0.05, 1.0, c["B"]).astype(np.float32)
    a = CL.forward_np("lstm", x, t, sd, table, CL.labels_for(c["B"]), c["NL"])
    sd2 = dict(sd)
    sd2["time_encoder.dense.bias"] = sd["time_encoder.dense.bias"].double() + torch.from_numpy(v).double()
    b = CL.forward_np("lstm", x, t, sd2, np.zeros_like(table), None, c["NL"])
    assert rel_err(a, b) < 1e-13


@pytest.mark.parametrize("c", [TF, MLP], ids=lambda c: c["kind"])
def test_table_gradient_of_the_judge_against_finite_differences(c):
    rng = np.random.default_rng(8)
    sd, table = _sd(c), 0.3 * rng.standard_normal((4, c["d"])).astype(np.float32)
    B, L, Cn = c["B"], c["L"], c["C"]
    x0, z = (rng.standard_normal((B, L, Cn)).astype(np.float32) for _ in range(2))
    t = rng.uniform(0.05, 1.0, B).astype(np.float32)
    sch = TR.scheduler("vp", L)
    mc, sigma = (v.numpy() for v in sch.marginal_coeffs(torch.from_numpy(t)))
    G = sch.G.numpy()
    y = CL.labels_for(B)  # class 3 (null) appears as -1; every row of the table is read
    _, _, g = CL.gradients(c["kind"], sd, table, c["NL"], c["H"], x0, t, mc, sigma, G, z, y, False, torch.float64)

    def f(tab):
        s = TR.cast(TR.renormed(sd) if c["kind"] == "transformer" else sd, torch.float64)
        with torch.no_grad():
            return float(CL.loss(c["kind"], s, torch.from_numpy(tab), c["NL"], c["H"], x0, t, mc, sigma, G, z, y, False,
                                 torch.float64)[0])

    fd = np.zeros((4, c["d"]))
    base = table.astype(np.float64)
    h = 1e-6
    for i in range(4):
        for j in range(c["d"]):
            up, dn = base.copy(), base.copy()
            up[i, j] += h
            dn[i, j] -= h
            fd[i, j] = (f(up) - f(dn)) / (2 * h)
    assert rel_err(g[CL.TABLE], fd) < 1e-6, rel_err(g[CL.TABLE], fd)
    # and it is the restated operator applied to the time embedding's gradient: rows of absent classes are zero
    only0 = CL.gradients(c["kind"], sd, table, c["NL"], c["H"], x0, t, mc, sigma, G, z, np.zeros(B, np.int32), False,
                         torch.float64)[2][CL.TABLE]
    assert np.abs(only0[0]).max() > 0 and not only0[1:].any()


def test_restated_operators():
    rng = np.random.default_rng(9)
    temb, table = rng.standard_normal((3, 8)), rng.standard_normal((4, 8))
    y = np.array([2, -1, 3])
    out = CL.class_temb(temb, 8, table, y, 3, 1)
    assert out.shape == (6, 8)
    assert np.array_equal(out[0], temb[0] + table[2]) and np.array_equal(out[1], temb[1] + table[3])
    assert np.array_equal(out[3:], temb + table[3])
    shared = CL.class_temb(temb[0], 0, table, None, 3, 0)
    assert np.array_equal(shared, np.tile(temb[0] + table[3], (3, 1)))
    c, u = rng.standard_normal(7), rng.standard_normal(7)
    assert np.array_equal(CL.cfg_combine(c, u, 1.0), u + (c - u)) and np.array_equal(CL.cfg_combine(c, u, 0.0), u)
    assert np.allclose(CL.cfg_combine(c, u, 2.5), 2.5 * c - 1.5 * u, rtol=0, atol=1e-14)
    g = CL.table_grad(rng.standard_normal((5, 8)), np.array([0, 0, -1, 3, 2]), 3)
    assert g.shape == (4, 8) and not g[1].any()


def test_restated_drop_rate_and_row_keying():
    n, nc = 20000, 3
    labels = (np.arange(n) % nc).astype(np.int32)
    for p in (0.0, 0.1, 0.5, 1.0):
        out = CL.class_drop(labels, nc, None, n, p, 1234, 0)
        rate = float((out == nc).mean())
        assert abs(rate - p) <= 4 * np.sqrt(max(p * (1 - p), 1e-12) / n), (p, rate)  # 4 sigma of the binomial
        assert np.array_equal(out[out != nc], labels[out != nc])
    # the same global row gives the same draw in two batchings, with and without an index, across a Philox block
    whole = CL.class_drop(labels, nc, None, 64, 0.5, 99, 2)
    idx = np.array([5, 0, 63, 17, 5, 3])
    assert np.array_equal(CL.class_drop(labels, nc, idx, 6, 0.5, 99, 2), whole[idx])
    assert np.array_equal(CL.class_drop(labels[3:], nc, None, 20, 0.5, 99, 5), np.where(
        whole[3:23] == nc, nc, labels[3:23]))
    u = CL.drop_uniforms(np.arange(16), 99, 2)
    assert np.array_equal(u, PR.uniforms(99, CL.TAG_CLASS_DROP, 2, 16))  # consecutive rows: consecutive slots
    assert not np.array_equal(u, PR.uniforms(99, PR.TAG_TIMES, 2, 16))   # a stream of its own
    assert (CL.class_drop(None, nc, None, 8, 0.0, 1, 0) == nc).all()


@pytest.mark.parametrize("case", CL.GRAD_CASES, ids=lambda c: c["name"])
def test_gradient_cases_stay_clear_of_the_relu_kink(case):
    """What the device test asserts before it compares a gradient, checked here for every (sde, p_uncond) pair: the
    smallest |pre-activation| through the judge is above KINK_MARGIN x the fp32 forward's error; at p_uncond = 0.5 the
    batch holds kept and dropped labels; a one-channel case's bias gradient keeps CL.BIAS_CANCELLATION of its terms."""
    for sde in ("vp", "ve"):
        for p in CL.P_UNCOND:
            model, sd, table, (x0, t, mc, sigma, z), labels, eff = CL.grad_case_setup(case, sde, p)
            margin, e32 = CL.kink_report(case["kind"], sd, table, case["NL"], case["H"], x0, t, mc, sigma,
                                         model.noise_scheduler.G.numpy(), z, eff)
            assert margin > TR.KINK_MARGIN * e32, (case["name"], sde, p, margin, e32)
            dropped = (eff == CL.N_CLASSES) & (CL.effective(labels, CL.N_CLASSES) != CL.N_CLASSES)
            assert dropped.any() == (p > 0) and not dropped.all()
            if case["C"] == 1:  # the one-element bias gradient is not a cancellation
                ratio = CL.bias_cancellation(case["kind"], sd, table, case["NL"], case["H"], x0, t, mc, sigma,
                                             model.noise_scheduler.G.numpy(), z, eff)
                assert ratio >= CL.BIAS_CANCELLATION, (case["name"], sde, p, ratio)


def test_a_scheduler_from_a_checkpoint_brings_no_device_copies_along(tmp_path):
    """Trainer.save_checkpoint pickles the scheduler with the hyper-parameters and load_from_checkpoint reads the file with
    map_location="cpu": a per-device copy of G saved along would come back as a host tensor under the device's key, and the
    kernels would be handed a host pointer.  The copies are not pickled, and a cached copy on another device is replaced."""
    from fastfourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler

    for cls in (VPScheduler, VEScheduler):
        sch = cls(fourier_noise_scaling=True)
        sch.set_noise_scaling(8)
        sch._G_dev["cuda:0"] = torch.ones(8)  # (what a scheduler that served a device holds; here a stand-in)
        torch.save({"s": sch}, tmp_path / "s.pt")
        with torch.serialization.safe_globals([VPScheduler, VEScheduler]):
            back = torch.load(tmp_path / "s.pt", map_location="cpu", weights_only=True)["s"]
        assert back._G_dev == {} and torch.equal(back.G, sch.G) and back.noise_scaling
        assert "cuda:0" in sch._G_dev  # the live object keeps its cache
        assert sch._G_on(torch.device("cpu")).device.type == "cpu"
        sch._G_dev["meta"] = torch.ones(8)  # a stale entry under another device's key is not handed out
        assert sch._G_on(torch.device("meta")).device.type == "meta"
