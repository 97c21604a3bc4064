"""CPU-side tests of the entropic optimal-transport statistics (no GPU): the C surface and its argument checks, the host
schedule, the Python surface (``utils.sinkhorn``, ``SinkhornDivergence``: refusals, keys, the kept self potential, baseline
and composition on a fake native layer), and the numpy restatement (tests/sinkhorn_restatement.py) against statements it
shares no code with: a written-out double loop, S(Y, Y) = 0, S(Y, Y + v) = |v|^2, S >= 0, the exact assignment cost at
small epsilon, the energy-distance limit at large epsilon, and the centred Gram form against the difference form."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import kernel_mmd_restatement as KR
import sinkhorn_restatement as SR
from host_entry_checks import HostBuffers, checks_work, one_host_prologue, refuses_every_alias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_sinkhorn_softmin_work_bytes", "ffd_sinkhorn_softmin", "ffd_sinkhorn_work_bytes", "ffd_sinkhorn",
         "ffd_sinkhorn_diameter2_work_bytes", "ffd_sinkhorn_diameter2", "ffd_host_sinkhorn_schedule")
KEYS = ("sinkhorn_divergence", "sinkhorn_distance", "sinkhorn_ot", "sinkhorn_change", "sinkhorn_eps")


@pytest.fixture(scope="module")
def lib():
    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


# ------------------------------------------------------------------ the C surface ----
def _header_args(header, name):
    decl = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert decl, name
    params = [" ".join(p.split()) for p in decl.group(2).split(",")]
    return decl.group(1), [p.rsplit(" ", 1)[0].replace(" *", "*") for p in params]


def test_symbols_header_and_argtypes(lib):
    from fastfourierdiffusion_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype.get(a, C.c_void_p) for a in args] == list(want_args), (name, args)
        assert all(a in ctype or a.endswith("*") for a in args), (name, args)
    assert len(_header_args(header, "ffd_sinkhorn_softmin")[1]) == 13
    assert len(_header_args(header, "ffd_sinkhorn")[1]) == 17
    assert len(_header_args(header, "ffd_host_sinkhorn_schedule")[1]) == 6
    csrc = os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "ffd_sinkhorn.hip" in make and "ffd_sinkhorn.o" in make and ".isa/ffd_sinkhorn.s" in make
    # one statement of the pair tile: the new source includes the shared header and repeats none of it
    text = open(os.path.join(csrc, "ffd_sinkhorn.hip")).read()
    assert '#include "ffd_pairtile.h"' in text
    for piece in ("void nn_tile(", "float nn_d2(", "void k_nn_colpart(", "void k_nn_colmean(", "void k_nn_centre("):
        assert piece not in text, piece
    one_host_prologue(csrc)  # ... and none of the host prologue
    assert "atomic" not in text.replace("No atomics", "")
    run = re.search(r"constexpr int SK_RUN = (\d+);", text)
    assert run and int(run.group(1)) * 256 == SR.RUN_COLUMNS  # a constant of the source: what the tests' run edges assume


def test_work_bytes_monotone_and_zero_for_refused(lib):
    values = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097, 60000)
    for query in (lib.ffd_sinkhorn_softmin_work_bytes, lib.ffd_sinkhorn_work_bytes):
        for axis in range(3):
            prev = 0
            for v in values:
                shape = [65, 257, 17]
                shape[axis] = v
                b = query(*shape)
                assert b > 0 and b >= prev and b % 16 == 0, (axis, v, b, prev)
                prev = b
        assert query(1 << 24, 1 << 24, 1 << 16) > 0
        for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), ((1 << 24) + 1, 4, 4), (4, (1 << 24) + 1, 4),
                    (4, 4, (1 << 16) + 1)):
            assert query(*bad) == 0, bad
    # the loop holds both sets and every potential twice: more than one softmin of the same shape
    assert lib.ffd_sinkhorn_work_bytes(65, 257, 17) > lib.ffd_sinkhorn_softmin_work_bytes(65, 257, 17)
    for axis in range(2):
        prev = 0
        for v in values:
            shape = [1025, 17]
            shape[axis] = v
            b = lib.ffd_sinkhorn_diameter2_work_bytes(*shape)
            assert b > 0 and b >= prev, (axis, v)
            prev = b
    for bad in ((0, 4), (4, 0), ((1 << 24) + 1, 4), (4, (1 << 16) + 1)):
        assert lib.ffd_sinkhorn_diameter2_work_bytes(*bad) == 0, bad


BAD_EPS = (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-60, 1e60)


def test_argument_errors_before_device_work(lib):
    n, m, D = 6, 9, 5
    sneed, lneed = lib.ffd_sinkhorn_softmin_work_bytes(n, m, D), lib.ffd_sinkhorn_work_bytes(n, m, D)
    dneed = lib.ffd_sinkhorn_diameter2_work_bytes(m, D)
    b = HostBuffers(x=n * D * 4, y=m * D * 4, centre=D * 4, h=m * 8, old=n * 8, out=n * 8, work=max(sneed, lneed, dneed),
                     qin=m * 8, f=n * 8, g=m * 8, p=n * 8, q=m * 8, out3=24, diam=8)

    def soft(query=b.x, nq=n, ref=b.y, nr=m, D=D, centre=b.centre, h=b.h, eps=0.5, old=b.old, out=b.out, work=b.work,
             nbytes=sneed):
        return lib.ffd_sinkhorn_softmin(query, nq, ref, nr, D, centre, h, eps, old, out, work, nbytes, None)

    for kw in (dict(query=None), dict(ref=None), dict(centre=None), dict(h=None), dict(out=None), dict(work=None), dict(nq=0),
               dict(nr=0), dict(D=0), dict(nq=-1), dict(D=-3), dict(nbytes=0), dict(nbytes=sneed - 1), dict(work=b.work + 4),
               dict(work=b.x), dict(work=b.y), dict(work=b.centre), dict(work=b.h), dict(work=b.old), dict(out=b.x),
               dict(out=b.y), dict(out=b.centre), dict(out=b.h), dict(out=b.old), dict(out=b.work)):
        assert soft(**kw) == INVALID, kw
    for bad in BAD_EPS:
        assert soft(eps=bad) == INVALID and soft(eps=bad, old=None) == INVALID, bad
    # every written region on every other region, with and without `old`, two sets and one; the workspace misaligned, a
    # byte short, and exactly the need
    soft_in = dict(query=b.x, ref=b.y, centre=b.centre, h=b.h)
    assert refuses_every_alias(soft, dict(out=b.out, work=b.work), dict(soft_in, old=b.old)) == 12
    assert refuses_every_alias(partial(soft, old=None), dict(out=b.out, work=b.work), dict(soft_in, old=None)) == 10
    assert refuses_every_alias(partial(soft, query=b.y, nq=m, old=None, out=b.g), dict(out=b.g, work=b.work),
                               dict(ref=b.y, centre=b.centre, h=b.h)) == 8
    checks_work(soft, b.work, sneed)
    checks_work(partial(soft, old=None), b.work, sneed)
    big = (1 << 24) + 1
    assert soft(nq=big) == UNSUPPORTED and soft(nr=big) == UNSUPPORTED and soft(D=(1 << 16) + 1) == UNSUPPORTED

    good = (C.c_double * 4)(8.0, 2.0, 0.5, 0.5)

    def loop(x=b.x, n=n, y=b.y, m=m, D=D, centre=b.centre, sched=C.addressof(good), n_eps=4, qin=b.qin, f=b.f, g=b.g, p=b.p,
             q=b.q, out3=b.out3, work=b.work, nbytes=lneed):
        return lib.ffd_sinkhorn(x, n, y, m, D, centre, sched, n_eps, qin, f, g, p, q, out3, work, nbytes, None)

    for kw in (dict(x=None), dict(y=None), dict(centre=None), dict(sched=None), dict(f=None), dict(g=None), dict(p=None),
               dict(q=None), dict(out3=None), dict(work=None), dict(n=0), dict(m=0), dict(D=0), dict(n=-2), dict(n_eps=0),
               dict(n_eps=-1), dict(nbytes=0), dict(nbytes=lneed - 1), dict(work=b.work + 8), dict(work=b.x), dict(work=b.y),
               dict(work=b.centre), dict(work=b.qin), dict(work=b.f), dict(work=b.out3), dict(f=b.x), dict(g=b.y),
               dict(p=b.centre), dict(q=b.qin), dict(f=b.g), dict(p=b.f), dict(q=b.g), dict(out3=b.q), dict(out3=b.qin)):
        assert loop(**kw) == INVALID, kw
    for kw in (dict(x=None), dict(n_eps=0), dict(nbytes=lneed - 1), dict(f=b.g), dict(work=b.y)):  # ... and without q_in
        assert loop(qin=None, **kw) == INVALID, kw
    loop_out = dict(f=b.f, g=b.g, p=b.p, q=b.q, out3=b.out3, work=b.work)
    assert refuses_every_alias(loop, loop_out, dict(x=b.x, y=b.y, centre=b.centre, qin=b.qin)) == 6 * 9
    assert refuses_every_alias(partial(loop, qin=None), loop_out, dict(x=b.x, y=b.y, centre=b.centre, qin=None)) == 6 * 8
    checks_work(loop, b.work, lneed)
    checks_work(partial(loop, qin=None), b.work, lneed)
    for bad in BAD_EPS:
        for at in range(3):
            sched = (C.c_double * 3)(4.0, 1.0, 0.25)
            sched[at] = bad
            assert loop(sched=C.addressof(sched), n_eps=3) == INVALID, (bad, at)
    assert loop(n=big) == UNSUPPORTED and loop(m=big) == UNSUPPORTED and loop(D=(1 << 16) + 1) == UNSUPPORTED

    def diam(y=b.y, n=m, D=D, centre=b.centre, out=b.diam, work=b.work, nbytes=dneed):
        return lib.ffd_sinkhorn_diameter2(y, n, D, centre, out, work, nbytes, None)

    for kw in (dict(y=None), dict(centre=None), dict(out=None), dict(work=None), dict(n=0), dict(D=0), dict(nbytes=0),
               dict(nbytes=dneed - 1), dict(work=b.work + 8), dict(work=b.y), dict(work=b.centre), dict(out=b.y),
               dict(out=b.centre), dict(out=b.work)):
        assert diam(**kw) == INVALID, kw
    assert refuses_every_alias(diam, dict(out=b.diam, work=b.work), dict(y=b.y, centre=b.centre)) == 6
    checks_work(diam, b.work, dneed)
    assert diam(n=big) == UNSUPPORTED and diam(D=(1 << 16) + 1) == UNSUPPORTED
    assert b.untouched()


# ------------------------------------------------------------------ the host schedule ----
def _lib_schedule(lib, diam2, eps, scaling, n_final, capacity=None):
    count = lib.ffd_host_sinkhorn_schedule(diam2, eps, scaling, n_final, None, 0)
    if count < 0 or capacity == 0:
        return count
    out = (C.c_double * (count + 2))(*([-7.0] * (count + 2)))
    got = lib.ffd_host_sinkhorn_schedule(diam2, eps, scaling, n_final, C.addressof(out), count if capacity is None else capacity)
    return got, list(out)


def test_host_schedule_against_the_restatement(lib):
    for diam2, eps, scaling, n_final in ((37.5, 0.01, 0.5, 3), (1.0, 1.0, 0.5, 1), (1.0, 2.0, 0.9, 4), (1e4, 1e-3, 0.8, 2),
                                         (5.0, 0.3, 0.25, 7), (3.0, 3.0 * 0.25 ** 3, 0.5, 2)):
        want = SR.schedule(diam2, eps, scaling, n_final)
        got, out = _lib_schedule(lib, diam2, eps, scaling, n_final)
        assert got == len(want) and out[:got] == want and out[got:] == [-7.0, -7.0], (diam2, eps, scaling)
        assert out[got - 1] == eps and out[got - n_final:got] == [eps] * n_final
        assert out[0] == (diam2 if diam2 > eps else eps) and all(a > b for a, b in zip(out, out[1:got - n_final + 1]))
        # the capacity rule: too small a capacity returns the count and writes nothing
        for capacity in (0, 1, got - 1):
            if capacity < got:
                short, untouched = _lib_schedule(lib, diam2, eps, scaling, n_final, capacity) if capacity else (
                    lib.ffd_host_sinkhorn_schedule(diam2, eps, scaling, n_final, None, 0), [-7.0])
                assert short == got and set(untouched) == {-7.0}, capacity
    # an entry that lands exactly on the target is not kept twice over: the list is strictly decreasing down to eps
    assert SR.schedule(4.0, 1.0, 0.5, 1) == [4.0, 1.0]
    for bad in ((0.0, 1.0, 0.5, 3), (-1.0, 1.0, 0.5, 3), (float("nan"), 1.0, 0.5, 3), (float("inf"), 1.0, 0.5, 3),
                (1.0, 0.0, 0.5, 3), (1.0, -2.0, 0.5, 3), (1.0, float("nan"), 0.5, 3), (1.0, float("inf"), 0.5, 3),
                (1.0, 0.1, 0.0, 3), (1.0, 0.1, 1.0, 3), (1.0, 0.1, -0.5, 3), (1.0, 0.1, float("nan"), 3), (1.0, 0.1, 0.5, 0),
                (1.0, 0.1, 0.5, -1)):
        assert lib.ffd_host_sinkhorn_schedule(*bad, None, 0) == INVALID, bad
    buf = (C.c_double * 4)()
    assert lib.ffd_host_sinkhorn_schedule(4.0, 1.0, 0.5, 1, C.addressof(buf), -1) == INVALID
    assert lib.ffd_host_sinkhorn_schedule(4.0, 1.0, 0.5, 1, None, 4) == INVALID
    assert lib.ffd_host_sinkhorn_schedule(1.0, 1e-300, 0.9999999, 1, None, 0) == UNSUPPORTED


# ------------------------------------------------------------------ the Python surface ----
class _FakeLib:
    """Stands in for libffd: reads the arrays the binding passes (host memory here) and answers with the restatement.  The
    host schedule is the library's own (it needs no device)."""

    def __init__(self, real):
        self.calls = []
        self.ffd_host_sinkhorn_schedule = real.ffd_host_sinkhorn_schedule

    @staticmethod
    def _arr(ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).reshape(shape)

    def _bytes(self, *shape):
        return 64

    ffd_mmd_centre_work_bytes = ffd_mmd_bandwidth_work_bytes = ffd_mmd_rowsums_work_bytes = _bytes
    ffd_sinkhorn_softmin_work_bytes = ffd_sinkhorn_work_bytes = ffd_sinkhorn_diameter2_work_bytes = _bytes

    def ffd_mmd_centre(self, x, n, D, out, work, nbytes, stream):
        self.calls.append(("centre", n))
        self._arr(out, (D,), np.float32)[:] = KR.centre_of(self._arr(x, (n, D), np.float32))
        return 0

    def ffd_mmd_bandwidth(self, y, n, D, out, work, nbytes, stream):
        self.calls.append(("bandwidth", n))
        self._arr(out, (1,), np.float64)[0] = KR.sigma2(self._arr(y, (n, D), np.float32))
        return 0

    def ffd_mmd_rowsums(self, a, na, b, nb, D, centre, gammas, ng, excl, out, work, nbytes, stream):
        self.calls.append(("rowsums", na, nb))
        g = self._arr(gammas, (ng,), np.float64)
        self._arr(out, (ng, na), np.float64)[:] = KR.row_sums(self._arr(a, (na, D), np.float32),
                                                              self._arr(b, (nb, D), np.float32), g, bool(excl))
        return 0

    def ffd_mmd_scores(self, xx, xy, yy, n, m, ng, mmd2, wit, stream):
        u, bsd, w = KR.scores_from_rowsums(self._arr(xx, (ng, n), np.float64), self._arr(xy, (ng, n), np.float64),
                                           self._arr(yy, (ng, m), np.float64))
        self._arr(mmd2, (2, ng + 1), np.float64)[:] = [u, bsd]
        self._arr(wit, (n,), np.float64)[:] = w
        return 0

    def ffd_sinkhorn_diameter2(self, y, n, D, centre, out, work, nbytes, stream):
        self.calls.append(("diameter2", n))
        self._arr(out, (1,), np.float64)[0] = SR.diameter2(self._arr(y, (n, D), np.float32), self._arr(centre, (D,), np.float32))
        return 0

    def ffd_sinkhorn_softmin(self, query, nq, ref, nr, D, centre, h, eps, old, out, work, nbytes, stream):
        self.calls.append(("softmin", nq, nr, eps, old is not None, query == ref))
        self._arr(out, (nq,), np.float64)[:] = SR.softmin(
            self._arr(query, (nq, D), np.float32), self._arr(ref, (nr, D), np.float32), self._arr(h, (nr,), np.float64), eps,
            None if old is None else self._arr(old, (nq,), np.float64).copy())
        return 0

    def ffd_sinkhorn(self, x, n, y, m, D, centre, sched, n_eps, qin, f, g, p, q, out3, work, nbytes, stream):
        self.calls.append(("sinkhorn", n, m, n_eps, qin is not None))
        r = SR.sinkhorn(self._arr(x, (n, D), np.float32), self._arr(y, (m, D), np.float32),
                        list(self._arr(sched, (n_eps,), np.float64)), None if qin is None else self._arr(qin, (m,), np.float64))
        for ptr, key, rows in ((f, "f", n), (g, "g", m), (p, "p", n), (q, "q", m)):
            self._arr(ptr, (rows,), np.float64)[:] = r[key]
        self._arr(out3, (3,), np.float64)[:] = [r["S"], r["ot_xy"], r["change"]]
        return 0


def _host_rows(x, name="x", min_rows=1):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    assert t.dim() == 2 and t.shape[0] >= min_rows
    return t.to(torch.float32).contiguous()


@pytest.fixture
def fake(monkeypatch, lib):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import metrics
    from fastfourierdiffusion_amd.utils import kernel_mmd, sinkhorn

    f = _FakeLib(lib)
    monkeypatch.setattr(metrics, "_to_device", _host_rows)
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    for module in (kernel_mmd, sinkhorn):
        monkeypatch.setattr(module, "_rows", _host_rows)
        monkeypatch.setattr(module, "_centre", lambda c, D: c.reshape(-1))
        monkeypatch.setattr(module, "_f64", lambda x, name, shape: x.contiguous())
    return f


def _require_host(t, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise AssertionError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def test_python_refusals_before_any_native_call(monkeypatch, lib):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import SinkhornDivergence
    from fastfourierdiffusion_amd.utils import sinkhorn as SK

    # the schedule is host only and runs as it is; its refusals are Python's
    assert SK.schedule(37.5, 0.01, 0.5, 3) == SR.schedule(37.5, 0.01, 0.5, 3)
    assert SK.schedule(1.0, 2.0) == [2.0] * 3

    def no_native():
        raise AssertionError("a native call was reached")

    monkeypatch.setattr(N, "lib", no_native)
    for bad in (dict(diameter2=0.0, eps=1.0), dict(diameter2=float("nan"), eps=1.0), dict(diameter2=1.0, eps=0.0),
                dict(diameter2=1.0, eps=float("inf")), dict(diameter2=1.0, eps=0.1, scaling=1.0),
                dict(diameter2=1.0, eps=0.1, scaling=0.0), dict(diameter2=1.0, eps=0.1, n_final=0)):
        with pytest.raises(AssertionError):
            SK.schedule(**bad)
    X, Y = SR.make_sets(20, 30, 4, "gaussian", 1)
    tx, ty, c = torch.from_numpy(X), torch.from_numpy(Y), torch.zeros(4)
    h, old = torch.zeros(30, dtype=torch.float64), torch.zeros(20, dtype=torch.float64)
    # host tensors and arrays: a clear error, no upload and no fallback
    for call in (lambda: SK.softmin(tx, ty, c, h, 1.0), lambda: SK.sinkhorn_divergence(tx, ty, c, [1.0]),
                 lambda: SK.diameter2(ty, c), lambda: SK.self_potential(ty, c, [1.0])):
        with pytest.raises(N.FFDError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        SK.softmin(X, Y, c, h, 1.0)
    # dtype, shape, epsilons and potentials, on a layer that accepts host rows
    monkeypatch.setattr(N, "require_gpu_tensor", _require_host)
    with pytest.raises(N.FFDError):
        SK.softmin(tx, ty, c, h, 1.0)  # a host potential
    with pytest.raises(N.FFDError):
        SK.sinkhorn_divergence(tx, ty, c, [1.0], q=h)
    monkeypatch.setattr(SK, "_f64", KM_f64_on_host)
    with pytest.raises(AssertionError):
        SK.softmin(tx.double(), ty, c, h, 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx[0], ty, c, h, 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx[:, :3], ty, c, h, 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx, ty, c[:3], h, 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx, ty, c, h[:29], 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx, ty, c, h.float(), 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(tx, ty, c, h, 1.0, old=old[:19])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(AssertionError):
            SK.softmin(tx, ty, c, h, bad)
        with pytest.raises(AssertionError):
            SK.sinkhorn_divergence(tx, ty, c, [1.0, bad])
    with pytest.raises(AssertionError):
        SK.sinkhorn_divergence(tx, ty, c, [])
    with pytest.raises(AssertionError):
        SK.sinkhorn_divergence(tx, ty[:, :3], c, [1.0])
    with pytest.raises(AssertionError):
        SK.sinkhorn_divergence(tx, ty, c, [1.0], q=old)  # 20 entries for 30 originals
    with pytest.raises(AssertionError):
        SK.self_potential(ty, c, [])
    for kwargs in (dict(blur=0.0), dict(blur=-1.0), dict(blur=float("inf")), dict(scaling=0.0), dict(scaling=1.0),
                   dict(n_final=0)):
        with pytest.raises(AssertionError):
            SinkhornDivergence(Y, **kwargs)
    with pytest.raises(AssertionError):
        SinkhornDivergence(Y[:1])


def KM_f64_on_host(x, name, shape):
    assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and tuple(x.shape) == tuple(shape), name
    return x.contiguous()


def test_sinkhorn_divergence_keys_kept_potential_and_baseline(fake):
    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y = SR.make_sets(40, 56, 6, "clustered", 2)
    metric = M.SinkhornDivergence(Y, blur=0.3)
    assert metric.name == "sinkhorn" and isinstance(metric, M.Metric) and M.SinkhornDivergence.views == M.Metric.views
    got = metric(X)
    assert tuple(got) == KEYS and all(isinstance(v, float) for v in got.values())
    want, price = SR.pipeline(X, Y, blur=0.3)
    for key, value in want.items():
        assert got[key] == pytest.approx(value, rel=1e-9, abs=1e-12), key
    assert got["sinkhorn_distance"] == max(got["sinkhorn_divergence"], 0.0) ** 0.5
    kinds = [c[0] for c in fake.calls]
    n_sched = len(SR.schedule(SR.diameter2(Y, KR.centre_of(Y)), want["sinkhorn_eps"]))
    assert kinds.count("centre") == 1 and kinds.count("bandwidth") == 1 and kinds.count("diameter2") == 1
    assert kinds.count("softmin") == n_sched + 1 and fake.calls[-1] == ("sinkhorn", 40, 56, n_sched, True)
    assert all(c[1:3] == (56, 56) and c[5] for c in fake.calls if c[0] == "softmin")  # the originals against themselves
    fake.calls.clear()
    assert metric(X) == got
    assert [c[0] for c in fake.calls] == ["sinkhorn"]  # the originals' part is kept
    tp = metric.transport_price(X)
    assert tp.dtype == torch.float64 and tp.shape == (40,) and np.allclose(tp.numpy(), price, rtol=1e-9, atol=1e-12)
    base = metric.baseline_metrics
    assert tuple(base) == tuple(f"{key}_self" for key in KEYS)
    fake.calls.clear()
    assert metric.baseline_metrics == base and not fake.calls  # a function of the originals alone: kept
    half = Y.shape[0] // 2
    sched = SR.schedule(SR.diameter2(Y, KR.centre_of(Y)), want["sinkhorn_eps"])
    assert base["sinkhorn_divergence_self"] == pytest.approx(SR.sinkhorn(Y[half:], Y[:half], sched)["S"], rel=1e-9, abs=1e-12)
    assert base["sinkhorn_eps_self"] == got["sinkhorn_eps"]


def test_metric_collection_composes_the_metric_and_leaves_the_others(fake, monkeypatch):
    from fastfourierdiffusion_amd.sampling import KernelMMD, SinkhornDivergence
    from fastfourierdiffusion_amd.sampling import metrics as M

    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x)[:, ::-1].copy())  # any other view of the rows
    X, Y = SR.make_sets(24, 30, 5, "gaussian", 4)
    mmd_keys = ("mmd2", "mmd2_biased", "mmd2_s0.5", "mmd2_s2", "witness_max", "witness_share_positive")
    alone = M.MetricCollection([partial(KernelMMD, scales=(0.5, 2))], original_samples=Y)(X)
    coll = M.MetricCollection([partial(KernelMMD, scales=(0.5, 2)), partial(SinkhornDivergence, blur=0.5, n_final=2)],
                              original_samples=Y)
    found = coll(X)
    want = sorted(f"{p}_{key}{suffix}" for p in ("time", "freq") for key in mmd_keys + KEYS for suffix in ("", "_self"))
    assert list(found) == want
    assert {k: v for k, v in found.items() if "sinkhorn" not in k} == alone  # the other metric's keys and values: unchanged
    assert found["time_sinkhorn_divergence"] == pytest.approx(SR.pipeline(X, Y, blur=0.5, n_final=2)[0]["sinkhorn_divergence"],
                                                              rel=1e-9, abs=1e-12)
    assert M.Metric.views == ("time", "freq") and M.DTWMetrics.views == ("time",)


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("family", SR.FAMILIES)
def test_softmin_is_the_written_out_double_loop(family):
    X, Y = SR.make_sets(5, 13, 4, family, 31)
    rng = np.random.default_rng(32)
    cost = SR.dist2(X, Y)
    for h in (np.zeros(13), cost.mean() * rng.standard_normal(13)):
        for eps in (0.05 * cost.mean(), cost.mean(), 50.0 * cost.mean()):
            got, want = SR.softmin(X, Y, h, eps), SR.softmin_loops(X, Y, h, eps)
            assert np.abs(got - want).max() <= 1e-10 * (cost.max() + np.abs(h).max()), (eps,)
            old = rng.standard_normal(5)
            assert np.array_equal(SR.softmin(X, Y, h, eps, old), 0.5 * (old + got))
    # the two ends: the smallest shifted cost plus eps log(nr / ties), and the mean shifted cost
    h = cost.mean() * rng.standard_normal(13)
    assert np.abs(SR.softmin(X, Y, h, 1e-9) - ((cost - h).min(axis=1) + 1e-9 * np.log(13))).max() <= 1e-12 * cost.max()
    assert np.abs(SR.softmin(X, Y, h, 1e9 * cost.mean()) - (cost - h).mean(axis=1)).max() <= 1e-6 * cost.max()


def _converged(X, Y, eps, n_final=60):
    centre = np.concatenate([X, Y]).astype(np.float64).mean(axis=0)
    diam2 = max(SR.diameter2(X, centre), SR.diameter2(Y, centre))
    return SR.sinkhorn(X, Y, SR.schedule(diam2, eps, 0.5, n_final))


def test_equal_sets_give_exactly_zero_and_a_shift_gives_its_square():
    _, Y = SR.make_sets(1, 23, 5, "clustered", 33)
    eps = SR.sigma2(Y)  # (a blur of 1: at 0.05 sigma^2 the iteration needs thousands of passes to settle to 1e-9)
    r = _converged(Y, Y.copy(), eps)
    # Jacobi ordering: the x|y and x|x problems are one computation, pass for pass
    assert r["S"] == 0.0 and np.array_equal(r["f"], r["p"]) and np.array_equal(r["g"], r["q"])
    # |x - (y + v)|^2 = |x - y|^2 - 2 <x - y, v> + |v|^2, and the cross term integrates to the same value under every
    # coupling of the two marginals (0 here: equal means), so OT_eps moves by |v|^2 and the self terms not at all
    v = np.array([0.5, -1.0, 0.25, 2.0, -0.125])  # exact in fp32, and so are the sums with Y
    shifted = (Y.astype(np.float64) + v)
    r = _converged(Y, shifted, eps, n_final=300)
    v2 = float(v @ v)
    print(f"S(Y, Y + v) = {r['S']:.12f}, |v|^2 = {v2}, last change {r['change']:.2e}")
    assert r["change"] <= 1e-9 * v2 and abs(r["S"] - v2) <= 1e-8 * v2


@pytest.mark.parametrize("family", SR.FAMILIES)
def test_divergence_is_non_negative_on_random_pairs(family):
    for seed in range(6):
        X, Y = SR.make_sets(9 + seed, 14, 3, family, 40 + seed)
        for blur in (0.1, 1.0):
            r = _converged(X, Y, blur * blur * SR.sigma2(Y))
            assert r["S"] >= -1e-9 * SR.dist2(X, Y).max(), (seed, blur, r["S"])


@pytest.mark.parametrize("n", [2, 5, 7])
def test_small_epsilon_is_within_the_entropic_gap_of_the_exact_assignment(n):
    """W <= OT_eps(x, y) <= W + eps log n (the optimal permutation plan has KL(pi | a x b) = log n) and
    0 <= OT_eps(x, x) <= eps log n, so |S - W| <= eps log n for two uniform sets of n rows."""
    rng = np.random.default_rng(50 + n)
    X = rng.integers(-6, 7, (n, 3)).astype(np.float32)
    Y = rng.integers(-6, 7, (n, 3)).astype(np.float32)
    W = SR.assignment_cost(X, Y)
    eps = 0.02
    r = _converged(X, Y, eps, n_final=400)
    print(f"n = {n}: S {r['S']:.6f}, exact assignment {W:.6f}, gap allowed {eps * np.log(n):.4f}, change {r['change']:.1e}")
    assert r["change"] <= 1e-6 and abs(r["S"] - W) <= eps * np.log(n) + 1e-6
    assert SR.assignment_cost(X, X) == 0.0


def test_large_epsilon_is_half_the_energy_distance():
    X, Y = SR.make_sets(17, 29, 4, "gaussian", 60)
    X = X + np.float32(0.75)
    limit = SR.energy_limit(X, Y)
    mean_gap = np.asarray(X, np.float64).mean(axis=0) - np.asarray(Y, np.float64).mean(axis=0)
    assert limit == pytest.approx(float(mean_gap @ mean_gap), rel=1e-12)
    scale = SR.dist2(X, Y).mean()
    errs = []
    for factor in (1e2, 1e4):
        r = SR.sinkhorn(X, Y, [factor * scale] * 40)
        errs.append(abs(r["S"] - limit))
    print(f"S against the limit {limit:.6f}: off by {errs[0]:.2e} at eps = 1e2 C, {errs[1]:.2e} at 1e4 C")
    assert errs[0] <= 0.05 * limit and errs[1] <= 1e-3 * limit and errs[1] < errs[0]


@pytest.mark.parametrize("family", SR.FAMILIES)
def test_centred_gram_form_against_the_difference_form(family):
    """The fp32 twin's costs, centred on the originals' mean, against float64's difference form: within the floor of the
    largest cost; and its softmin within the same floor, which is what makes max(floor, 3 e_ref) a bar and not a wish."""
    X, Y = SR.make_sets(65, 257, 187, family, 70)
    centre = SR.centre_of(Y)
    cost, cost32 = SR.dist2(X, Y), SR.gram32_d2(X, Y, centre)
    err = float(np.abs(cost32 - cost).max())
    print(f"{family}: centred Gram d2 off by {err:.3e} of {cost.max():.1f}")
    assert err <= SR.FLOOR * cost.max()
    rng = np.random.default_rng(71)
    h = cost.mean() * rng.standard_normal(257)
    for eps in (1e-3 * cost.mean(), cost.mean()):
        e_ref = float(np.abs(SR.softmin_cost32(cost32, h, eps) - SR.softmin_cost(cost, h, eps)).max())
        assert e_ref <= SR.FLOOR * (cost.max() + np.abs(h).max()), (eps, e_ref)
    assert SR.bar(0.0, 8.0) == 8.0 * SR.FLOOR and SR.bar(1.0, 8.0) == 3.0
    # the loop on the twin follows the loop in float64
    sched = SR.schedule(SR.diameter2(Y, centre), 0.01 * SR.sigma2(Y))
    a, b = SR.sinkhorn(X, Y, sched), SR.sinkhorn32(X, Y, centre, sched)
    assert abs(a["S"] - b["S"]) <= SR.FLOOR * cost.max()
    assert np.array_equal(SR.self_potential(Y, sched), a["q"])
