"""CPU-side tests of the kernel two-sample statistics (no GPU): the C surface and its argument checks, the Python surface
(``utils.kernel_mmd``, ``KernelMMD``: refusals, keys, cache, composition on a fake native layer), the numpy restatement
(tests/kernel_mmd_restatement.py) against formulations it shares no code with, the reason the Gram form is centred, and
the condition on the permutation cases that keeps the GPU test's count band from hiding a failure."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import kernel_mmd_restatement as KR
from host_entry_checks import HostBuffers, checks_work, one_host_prologue, refuses_every_alias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_mmd_centre_work_bytes", "ffd_mmd_centre", "ffd_mmd_bandwidth_work_bytes", "ffd_mmd_bandwidth",
         "ffd_mmd_rowsums_work_bytes", "ffd_mmd_rowsums", "ffd_mmd_scores", "ffd_mmd_gram_work_bytes", "ffd_mmd_gram",
         "ffd_mmd_permute_work_bytes", "ffd_mmd_permute")


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
    from fastfourierdiffusion_amd.utils import kernel_mmd

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    limits = re.search(r"enum\s*\{\s*FFD_MMD_MAX_GAMMAS\s*=\s*(\d+),\s*FFD_MMD_MAX_POOLED\s*=\s*(\d+),\s*"
                       r"FFD_MMD_MAX_PERMUTATIONS\s*=\s*(\d+)\s*\}", header)
    assert limits and tuple(int(v) for v in limits.groups()) == \
        (kernel_mmd.MAX_GAMMAS, kernel_mmd.MAX_POOLED, kernel_mmd.MAX_PERMUTATIONS) == (8, 16384, 4096)
    ctype = {"int": C.c_int, "size_t": C.c_size_t}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype.get(a, C.c_void_p) for a in args] == list(want_args), (name, args)
        assert all(a in ctype or a.endswith("*") for a in args), (name, args)
    assert len(_header_args(header, "ffd_mmd_rowsums")[1]) == 13
    assert len(_header_args(header, "ffd_mmd_permute")[1]) == 9
    make = open(os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc", "Makefile")).read()
    assert "ffd_mmd.hip" in make and "ffd_pairtile.h" in make
    # one statement of the pair tile: the shared header has it, neither source repeats it
    csrc = os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc")
    shared = open(os.path.join(csrc, "ffd_pairtile.h")).read()
    for piece in ("void nn_tile(", "float nn_d2(", "void k_nn_colpart(", "void k_nn_colmean(", "void k_nn_centre("):
        assert piece in shared, piece
        for source in ("ffd_neighbours.hip", "ffd_mmd.hip"):
            text = open(os.path.join(csrc, source)).read()
            assert piece not in text and '#include "ffd_pairtile.h"' in text, (piece, source)
    one_host_prologue(csrc)  # ... and one statement of the host prologue


def test_work_bytes_monotone_and_zero_for_refused(lib):
    values = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097, 60000)
    base = [65, 257, 17, 5]
    for axis in range(4):
        prev = 0
        for v in values:
            if axis == 3 and v > 8:
                break
            shape = list(base)
            shape[axis] = v
            b = lib.ffd_mmd_rowsums_work_bytes(*shape)
            assert b > 0 and b >= prev and b % 16 == 0, (axis, v, b, prev)
            prev = b
    assert lib.ffd_mmd_rowsums_work_bytes(1 << 24, 1 << 24, 1 << 16, 8) > 0
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0), (4, 4, 4, 9), (-1, 4, 4, 1), ((1 << 24) + 1, 4, 4, 1),
                (4, (1 << 24) + 1, 4, 1), (4, 4, (1 << 16) + 1, 1)):
        assert lib.ffd_mmd_rowsums_work_bytes(*bad) == 0, bad
    for query, low in ((lib.ffd_mmd_centre_work_bytes, 1), (lib.ffd_mmd_bandwidth_work_bytes, 2)):
        for axis in range(2):
            prev = 0
            for v in values:
                shape = [1025, 17]
                shape[axis] = max(v, low) if axis == 0 else v
                b = query(*shape)
                assert b > 0 and b >= prev, (axis, v)
                prev = b
        for bad in ((low - 1, 4), (4, 0), ((1 << 24) + 1, 4), (4, (1 << 16) + 1)):
            assert query(*bad) == 0, bad
    prev_g = prev_p = 0
    for v in (2, 3, 62, 63, 64, 65, 1000, 8192):
        g, p = lib.ffd_mmd_gram_work_bytes(v, 2, 17), lib.ffd_mmd_permute_work_bytes(v, 2, 100)
        assert g > prev_g and p >= prev_p > -1
        prev_g, prev_p = g, p
    assert lib.ffd_mmd_gram_work_bytes(8192, 8192, 187) >= 16384 * 16384 * 4
    assert lib.ffd_mmd_permute_work_bytes(8192, 8192, 4096) > 0
    assert lib.ffd_mmd_permute_work_bytes(96, 160, 64) <= lib.ffd_mmd_permute_work_bytes(96, 160, 65)
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 0), (8192, 8193, 4), (4, 4, (1 << 16) + 1)):
        assert lib.ffd_mmd_gram_work_bytes(*bad) == 0, bad
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 0), (8192, 8193, 4), (4, 4, 4097)):
        assert lib.ffd_mmd_permute_work_bytes(*bad) == 0, bad


def test_argument_errors_before_device_work(lib):
    na, nb, D, ng, P = 6, 9, 5, 3, 7
    need = lib.ffd_mmd_rowsums_work_bytes(na, nb, D, ng)
    gneed, pneed = lib.ffd_mmd_gram_work_bytes(na, nb, D), lib.ffd_mmd_permute_work_bytes(na, nb, P)
    cneed, bneed = lib.ffd_mmd_centre_work_bytes(nb, D), lib.ffd_mmd_bandwidth_work_bytes(nb, D)
    b = HostBuffers(a=na * D * 4, b=nb * D * 4, centre=D * 4, out=ng * max(na, nb) * 8, work=max(need, pneed, cneed, bneed),
                     gwork=gneed, xx=ng * na * 8, xy=ng * na * 8, yy=ng * nb * 8, mmd2=(2 * ng + 2) * 8, wit=na * 8,
                     assign=P * (na + nb), t=P * 8, sig=8)
    gam = (C.c_double * 8)(0.5, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    gptr = C.addressof(gam)

    def rows(a=b.a, na=na, bb=b.b, nb=nb, D=D, centre=b.centre, g=gptr, ng=ng, excl=0, out=b.out, work=b.work, nbytes=need):
        return lib.ffd_mmd_rowsums(a, na, bb, nb, D, centre, g, ng, excl, out, work, nbytes, None)

    for kw in (dict(a=None), dict(bb=None), dict(centre=None), dict(g=None), dict(out=None), dict(work=None), dict(na=0),
               dict(nb=0), dict(D=0), dict(na=-1), dict(D=-3), dict(ng=0), dict(ng=9), dict(ng=-1), dict(excl=1),
               dict(a=b.b, excl=1), dict(nbytes=0), dict(nbytes=need - 1), dict(work=b.work + 4), dict(work=b.a),
               dict(work=b.b), dict(work=b.centre), dict(out=b.a), dict(out=b.b), dict(out=b.centre), dict(out=b.work)):
        assert rows(**kw) == INVALID, kw
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        bad_g = (C.c_double * 3)(0.5, bad, 1.0)
        assert rows(g=C.addressof(bad_g)) == INVALID, bad
    # every written region on every other region; the workspace misaligned, a byte short, and exactly the need
    assert refuses_every_alias(rows, dict(out=b.out, work=b.work), dict(a=b.a, bb=b.b, centre=b.centre)) == 8
    assert refuses_every_alias(partial(rows, a=b.b, na=nb), dict(out=b.out, work=b.work), dict(bb=b.b, centre=b.centre)) == 6
    checks_work(rows, b.work, need)
    big = (1 << 24) + 1
    assert rows(na=big) == UNSUPPORTED and rows(nb=big) == UNSUPPORTED and rows(D=(1 << 16) + 1) == UNSUPPORTED

    def centre(x=b.b, n=nb, D=D, out=b.centre, work=b.work, nbytes=cneed):
        return lib.ffd_mmd_centre(x, n, D, out, work, nbytes, None)

    def band(y=b.b, n=nb, D=D, out=b.sig, work=b.work, nbytes=bneed):
        return lib.ffd_mmd_bandwidth(y, n, D, out, work, nbytes, None)

    for kw in (dict(n=0), dict(D=0), dict(out=None), dict(work=None), dict(nbytes=0), dict(work=b.work + 8), dict(work=b.b)):
        assert centre(**kw) == INVALID and band(**kw) == INVALID, kw
    assert centre(x=None) == INVALID and band(y=None) == INVALID and band(n=1) == INVALID
    assert centre(out=b.b) == INVALID and band(out=b.b) == INVALID
    assert centre(nbytes=cneed - 1) == INVALID and band(nbytes=bneed - 1) == INVALID
    assert refuses_every_alias(centre, dict(out=b.centre, work=b.work), dict(x=b.b)) == 4
    assert refuses_every_alias(band, dict(out=b.sig, work=b.work), dict(y=b.b)) == 4
    checks_work(centre, b.work, cneed)
    checks_work(band, b.work, bneed)
    assert centre(n=big) == UNSUPPORTED and band(n=big) == UNSUPPORTED and band(D=(1 << 16) + 1) == UNSUPPORTED

    def scores(xx=b.xx, xy=b.xy, yy=b.yy, n=na, m=nb, ng=ng, mmd2=b.mmd2, wit=b.wit):
        return lib.ffd_mmd_scores(xx, xy, yy, n, m, ng, mmd2, wit, None)

    for kw in (dict(xx=None), dict(xy=None), dict(yy=None), dict(mmd2=None), dict(wit=None), dict(n=1), dict(m=1), dict(n=0),
               dict(ng=0), dict(ng=9), dict(mmd2=b.xx), dict(mmd2=b.yy), dict(wit=b.xy), dict(wit=b.mmd2)):
        assert scores(**kw) == INVALID, kw
    assert refuses_every_alias(scores, dict(mmd2=b.mmd2, wit=b.wit), dict(xx=b.xx, xy=b.xy, yy=b.yy)) == 8
    assert scores(n=big) == UNSUPPORTED

    def gram(x=b.a, n=na, y=b.b, m=nb, D=D, centre=b.centre, g=gptr, ng=ng, work=b.gwork, nbytes=gneed):
        return lib.ffd_mmd_gram(x, n, y, m, D, centre, g, ng, work, nbytes, None)

    for kw in (dict(x=None), dict(y=None), dict(centre=None), dict(g=None), dict(work=None), dict(n=1), dict(m=1), dict(D=0),
               dict(ng=0), dict(ng=9), dict(nbytes=gneed - 1), dict(work=b.gwork + 4), dict(work=b.a), dict(work=b.b)):
        assert gram(**kw) == INVALID, kw
    assert refuses_every_alias(gram, dict(work=b.gwork), dict(x=b.a, y=b.b, centre=b.centre)) == 3
    checks_work(gram, b.gwork, gneed)
    assert gram(n=16383) == UNSUPPORTED and gram(D=(1 << 16) + 1) == UNSUPPORTED

    def permute(k=b.gwork, n=na, m=nb, assign=b.assign, P=P, t=b.t, work=b.work, nbytes=pneed):
        return lib.ffd_mmd_permute(k, n, m, assign, P, t, work, nbytes, None)

    for kw in (dict(k=None), dict(assign=None), dict(t=None), dict(work=None), dict(n=1), dict(m=1), dict(P=0), dict(P=-1),
               dict(nbytes=pneed - 1), dict(work=b.work + 4), dict(k=b.gwork + 4), dict(work=b.gwork), dict(work=b.assign),
               dict(t=b.gwork), dict(t=b.assign), dict(t=b.work)):
        assert permute(**kw) == INVALID, kw
    assert refuses_every_alias(permute, dict(t=b.t, work=b.work), dict(k=b.gwork, assign=b.assign)) == 6
    assert permute(assign=b.gwork) == INVALID and permute(k=b.assign) == INVALID  # two read regions, refused all the same
    checks_work(permute, b.work, pneed)
    assert permute(P=4097) == UNSUPPORTED and permute(n=16383) == UNSUPPORTED
    assert b.untouched()


# ------------------------------------------------------------------ the Python surface ----
class _FakeLib:
    """Stands in for libffd: reads the arrays the binding passes (host memory here) and answers with the restatement."""

    def __init__(self):
        self.calls = []
        self.grams = {}

    @staticmethod
    def _arr(ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).reshape(shape)

    def ffd_mmd_centre_work_bytes(self, n, D):
        return 64

    ffd_mmd_bandwidth_work_bytes = ffd_mmd_centre_work_bytes

    def ffd_mmd_rowsums_work_bytes(self, na, nb, D, ng):
        return 64

    def ffd_mmd_gram_work_bytes(self, n, m, D):
        return 64

    ffd_mmd_permute_work_bytes = ffd_mmd_gram_work_bytes

    def ffd_mmd_centre(self, x, n, D, out, work, nbytes, stream):
        self.calls.append(("centre", n))
        self._arr(out, (D,), np.float32)[:] = KR.centre_of(self._arr(x, (n, D), np.float32))
        return 0

    def ffd_mmd_bandwidth(self, y, n, D, out, work, nbytes, stream):
        self.calls.append(("bandwidth", n))
        self._arr(out, (1,), np.float64)[0] = KR.sigma2(self._arr(y, (n, D), np.float32))
        return 0

    def ffd_mmd_rowsums(self, a, na, b, nb, D, centre, gammas, ng, excl, out, work, nbytes, stream):
        self.calls.append(("rowsums", na, nb, ng, excl, a == b))
        g = self._arr(gammas, (ng,), np.float64)
        self._arr(out, (ng, na), np.float64)[:] = KR.row_sums(self._arr(a, (na, D), np.float32),
                                                              self._arr(b, (nb, D), np.float32), g, bool(excl))
        return 0

    def ffd_mmd_scores(self, xx, xy, yy, n, m, ng, mmd2, wit, stream):
        self.calls.append(("scores", n, m, ng))
        u, bsd, w = KR.scores_from_rowsums(self._arr(xx, (ng, n), np.float64), self._arr(xy, (ng, n), np.float64),
                                           self._arr(yy, (ng, m), np.float64))
        self._arr(mmd2, (2, ng + 1), np.float64)[:] = [u, bsd]
        self._arr(wit, (n,), np.float64)[:] = w
        return 0

    def ffd_mmd_gram(self, x, n, y, m, D, centre, gammas, ng, work, nbytes, stream):
        self.calls.append(("gram", n, m, ng))
        self.grams[work] = KR.gram(self._arr(x, (n, D), np.float32), self._arr(y, (m, D), np.float32),
                                   self._arr(gammas, (ng,), np.float64))
        return 0

    def ffd_mmd_permute(self, gwork, n, m, assign, P, t, work, nbytes, stream):
        self.calls.append(("permute", n, m, P))
        self._arr(t, (P,), np.float64)[:] = KR.perm_stats(self.grams[gwork], self._arr(assign, (P, n + m), np.uint8), n, m)
        return 0


def _host_rows(x, name="x", min_rows=1):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    assert t.dim() == 2 and t.shape[0] >= min_rows
    return t.to(torch.float32).contiguous()


@pytest.fixture
def fake(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import metrics
    from fastfourierdiffusion_amd.utils import kernel_mmd

    f = _FakeLib()
    monkeypatch.setattr(metrics, "_to_device", _host_rows)
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    monkeypatch.setattr(kernel_mmd, "_rows", _host_rows)
    monkeypatch.setattr(kernel_mmd, "_centre", lambda c, D: c.reshape(-1))
    monkeypatch.setattr(kernel_mmd, "_f64", lambda x, name, shape: x.contiguous())
    return f


def test_python_refusals_before_any_native_call(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import KernelMMD
    from fastfourierdiffusion_amd.utils import kernel_mmd as KM

    def no_native():
        raise AssertionError("a native call was reached")

    monkeypatch.setattr(N, "lib", no_native)
    X, Y = KR.make_sets(20, 30, 4, "gaussian", 1)
    tx, ty, c = torch.from_numpy(X), torch.from_numpy(Y), torch.zeros(4)
    # host tensors and arrays: a clear error, no upload and no fallback
    for call in (lambda: KM.row_sums(tx, ty, c, [1.0]), lambda: KM.bandwidth(ty), lambda: KM.column_mean(ty),
                 lambda: KM.permutation_test(tx, ty, c, [1.0], KM.permutation_assignments(20, 30, 3, 0))):
        with pytest.raises(N.FFDError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        KM.row_sums(X, Y, c, [1.0])
    with pytest.raises(N.FFDError):
        KM.mmd_scores(torch.zeros(1, 5, dtype=torch.float64), torch.zeros(1, 5, dtype=torch.float64),
                      torch.zeros(1, 6, dtype=torch.float64))
    # dtype, shape, row counts and bandwidths, on a layer that accepts host rows
    monkeypatch.setattr(N, "require_gpu_tensor", lambda t, name="tensor": N_require_host(t, name))
    with pytest.raises(AssertionError):
        KM.row_sums(tx.double(), ty, c, [1.0])
    with pytest.raises(AssertionError):
        KM.row_sums(tx[0], ty, c, [1.0])
    with pytest.raises(AssertionError):
        KM.row_sums(tx[:, :3], ty, c, [1.0])
    with pytest.raises(AssertionError):
        KM.row_sums(tx, ty, c[:3], [1.0])
    with pytest.raises(AssertionError):
        KM.row_sums(tx, ty, c, [1.0], exclude_self=True)
    for bad in ([], [1.0] * 9, [-1.0], [float("nan")], [float("inf")]):
        with pytest.raises(AssertionError):
            KM.row_sums(tx, ty, c, bad)
    with pytest.raises(AssertionError):
        KM.bandwidth(ty[:1])
    with pytest.raises(AssertionError):
        KM.permutation_test(tx[:1], ty, c, [1.0], np.ones((2, 31), np.uint8))
    with pytest.raises(AssertionError):
        KM.permutation_test(tx, ty, c, [1.0], np.ones((2, 50), np.uint8))  # not n ones per row
    with pytest.raises(AssertionError):
        KM.permutation_test(tx, ty, c, [1.0], KM.permutation_assignments(20, 29, 3, 0))
    with pytest.raises(ValueError, match="4096"):
        KM.permutation_test(tx, ty, c, [1.0], np.tile(KM.permutation_assignments(20, 30, 0, 0), (4097, 1)))
    big = torch.zeros(16383, 1)
    with pytest.raises(ValueError, match="16384"):
        KM.permutation_test(big, big[:2], c[:1], [1.0], np.zeros((1, 16385), np.uint8))
    for shape in ((1, 1), (0, 5)):
        with pytest.raises(AssertionError):
            KM.mmd_scores(torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64),
                          torch.zeros(1, 6, dtype=torch.float64))
    with pytest.raises(AssertionError):
        KM.ladder_gammas(0.0)
    for kwargs in (dict(scales=()), dict(scales=(1.0,) * 9), dict(scales=(0.0, 1.0)), dict(permutations=-1),
                   dict(permutations=4096)):
        with pytest.raises(AssertionError):
            KernelMMD(Y, **kwargs)
    with pytest.raises(AssertionError):
        KernelMMD(Y[:1])
    metric = KernelMMD(np.zeros((16000, 2), np.float32), permutations=10)
    with pytest.raises(ValueError, match="16384"):
        metric._check_pooled(385, 16000)
    metric._check_pooled(384, 16000)
    KernelMMD(np.zeros((16000, 2), np.float32))._check_pooled(100000, 16000)  # no test, no limit


def N_require_host(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise AssertionError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def test_kernel_mmd_keys_cache_and_baseline(fake):
    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y = KR.make_sets(60, 90, 6, "clustered", 2)
    metric = M.KernelMMD(Y, permutations=40, random_seed=3)
    assert metric.name == "kernel_mmd" and isinstance(metric, M.Metric)
    got = metric(X)
    keys = ("mmd2", "mmd2_biased", "mmd2_s0.25", "mmd2_s0.5", "mmd2_s1", "mmd2_s2", "mmd2_s4", "witness_max",
            "witness_share_positive", "p_value")
    assert tuple(got) == keys and all(isinstance(v, float) for v in got.values())
    want, w = KR.pipeline(X, Y)
    for key, value in want.items():
        assert got[key] == pytest.approx(value, rel=1e-12, abs=1e-15), key
    T = KR.perm_stats(KR.gram(X, Y, KR.ladder(KR.sigma2(Y))), KR.assignments(60, 90, 40, 3), 60, 90)
    assert got["p_value"] == KR.p_value(T) and T[0] == pytest.approx(want["mmd2"], rel=1e-10)
    kinds = [c[0] for c in fake.calls]
    assert kinds.count("centre") == 1 and kinds.count("bandwidth") == 1 and kinds.count("rowsums") == 3
    assert ("rowsums", 90, 90, 5, 1, True) in fake.calls and ("rowsums", 60, 90, 5, 0, False) in fake.calls
    assert ("permute", 60, 90, 41) in fake.calls
    fake.calls.clear()
    assert metric(X) == got
    kinds = [c[0] for c in fake.calls]
    assert kinds.count("rowsums") == 2 and "centre" not in kinds and "bandwidth" not in kinds  # the originals' part is kept
    wit = metric.witness(X)
    assert wit.dtype == torch.float64 and np.allclose(wit.numpy(), w, rtol=1e-12, atol=1e-15)
    base = metric.baseline_metrics
    assert tuple(base) == tuple(f"{key}_self" for key in keys)
    fake.calls.clear()
    assert metric.baseline_metrics == base and not fake.calls  # a function of the originals alone: kept
    half = Y.shape[0] // 2
    g = KR.ladder(KR.sigma2(Y))
    u, _, _ = KR.scores_from_rowsums(KR.row_sums(Y[half:], Y[half:], g, True), KR.row_sums(Y[half:], Y[:half], g),
                                     KR.row_sums(Y[:half], Y[:half], g, True))
    assert base["mmd2_self"] == pytest.approx(u[-1], rel=1e-12, abs=1e-15)
    plain = M.KernelMMD(Y, scales=(1, 3))
    assert tuple(plain(X)) == ("mmd2", "mmd2_biased", "mmd2_s1", "mmd2_s3", "witness_max", "witness_share_positive")


def test_metric_collection_composes_the_metric(fake, monkeypatch):
    from fastfourierdiffusion_amd.sampling import KernelMMD
    from fastfourierdiffusion_amd.sampling import metrics as M

    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x)[:, ::-1].copy())  # any other view of the rows
    X, Y = KR.make_sets(40, 50, 5, "gaussian", 4)
    coll = M.MetricCollection([partial(KernelMMD, scales=(0.5, 2))], original_samples=Y)
    found = coll(X)
    keys = ("mmd2", "mmd2_biased", "mmd2_s0.5", "mmd2_s2", "witness_max", "witness_share_positive")
    want = sorted([f"{p}_{key}" for p in ("time", "freq") for key in keys] +
                  [f"{p}_{key}_self" for p in ("time", "freq") for key in keys])
    assert list(found) == want
    assert found["time_mmd2"] == pytest.approx(KR.pipeline(X, Y, (0.5, 2))[0]["mmd2"], rel=1e-12, abs=1e-15)


def test_assignments_of_the_library_are_the_restatement_s():
    from fastfourierdiffusion_amd.utils import kernel_mmd as KM

    for n, m, P, seed in ((5, 7, 20, 0), (96, 160, 30, KR.PERM_SEED)):
        A = KM.permutation_assignments(n, m, P, seed)
        assert A.dtype == np.uint8 and A.shape == (P + 1, n + m) and np.array_equal(A, KR.assignments(n, m, P, seed))
        assert (A.sum(axis=1) == n).all() and A[0, :n].all() and not A[0, n:].any()
        assert len({row.tobytes() for row in A}) > P // 2


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("family", KR.FAMILIES)
def test_unbiased_estimate_from_row_sums_is_the_textbook_double_sum(family):
    X, Y = KR.make_sets(37, 53, 7, family, 21)
    gammas = KR.ladder(KR.sigma2(Y))
    u, bsd, w = KR.scores_from_rowsums(KR.row_sums(X, X, gammas, True), KR.row_sums(X, Y, gammas), KR.row_sums(Y, Y, gammas, True))
    for g, gamma in enumerate(gammas):
        tu, tb = KR.mmd_textbook(X, Y, gamma)
        assert u[g] == pytest.approx(tu, rel=1e-11, abs=1e-14) and bsd[g] == pytest.approx(tb, rel=1e-11, abs=1e-14)
        assert bsd[g] >= 0.0
    assert u[-1] == pytest.approx(np.mean(u[:-1]), rel=1e-12) and bsd[-1] == pytest.approx(np.mean(bsd[:-1]), rel=1e-12)
    assert w.shape == (37,)
    # a python loop over the pairs, one gamma
    gamma, acc = gammas[2], 0.0
    for i in range(5):
        row = 0.0
        for j in range(53):
            row += float(np.exp(-gamma * sum((float(X[i, d]) - float(Y[j, d])) ** 2 for d in range(7))))
        acc = max(acc, abs(row - KR.row_sums(X, Y, [gamma])[0, i]))
    assert acc < 1e-12


def test_x_equal_y_gives_a_biased_estimate_of_exactly_zero():
    _, Y = KR.make_sets(2, 41, 5, "clustered", 22)
    gammas = KR.ladder(KR.sigma2(Y))
    rs = KR.row_sums(Y, Y, gammas, True)
    _, bsd, w = KR.scores_from_rowsums(rs, KR.row_sums(Y, Y, gammas), rs)
    # XY holds the diagonal the self terms leave out: (s + n) / n^2 + (s + n) / n^2 - 2 (s + n) / n^2
    assert np.abs(bsd).max() <= 1e-15
    rs1 = KR.row_sums(Y, Y, gammas[:1], True)
    xy1 = rs1 + 1.0
    n = Y.shape[0]
    assert ((rs1.sum() + n) / (n * n) + (rs1.sum() + n) / (n * n)) - 2.0 * xy1.sum() / (n * n) == pytest.approx(0.0, abs=1e-15)


def test_null_mean_of_the_unbiased_estimate_is_zero_within_its_standard_error():
    values = []
    for seed in range(60):
        rng = np.random.default_rng(900 + seed)
        X, Y = rng.standard_normal((40, 3)).astype(np.float32), rng.standard_normal((50, 3)).astype(np.float32)
        g = KR.ladder(6.0)  # the population's sigma^2 = 2 D: the same kernel for every seed
        values.append(KR.scores_from_rowsums(KR.row_sums(X, X, g, True), KR.row_sums(X, Y, g), KR.row_sums(Y, Y, g, True))[0][-1])
    values = np.array(values)
    stderr = values.std(ddof=1) / np.sqrt(len(values))
    print(f"null MMD^2_u over {len(values)} seeds: mean {values.mean():.3e}, standard error {stderr:.3e}")
    assert abs(values.mean()) <= 3.0 * stderr and (values < 0).any() and (values > 0).any()


@pytest.mark.parametrize("family", KR.FAMILIES)
def test_sigma2_is_the_mean_over_all_explicit_pairs(family):
    for n, D in ((2, 3), (33, 1), (70, 19)):
        _, Y = KR.make_sets(2, n, D, family, 23)
        assert KR.sigma2(Y) == pytest.approx(KR.sigma2_pairs(Y), rel=1e-12)
    assert KR.ladder(2.0, (0.25, 1, 4)) == [1.0, 0.25, 0.0625]


def test_permutation_statistic_properties():
    X, Y = KR.make_sets(30, 44, 6, "gaussian", 24)
    gammas = KR.ladder(KR.sigma2(Y))
    K = KR.gram(X, Y, gammas)
    A = KR.assignments(30, 44, 50, 5)
    T = KR.perm_stats(K, A, 30, 44)
    # assignment 0 is the unbiased estimate of the mean kernel
    u, _, _ = KR.scores_from_rowsums(KR.row_sums(X, X, gammas, True), KR.row_sums(X, Y, gammas), KR.row_sums(Y, Y, gammas, True))
    assert T[0] == pytest.approx(u[-1], rel=1e-11, abs=1e-15)
    # a constant added to every off-diagonal entry changes nothing
    shifted = K + 0.37
    shifted[np.arange(74), np.arange(74)] = 0.0
    assert np.abs(KR.perm_stats(shifted, A, 30, 44) - T).max() <= 1e-14
    centred = K - K.sum() / (74 * 73)
    centred[np.arange(74), np.arange(74)] = 0.0
    assert np.abs(KR.perm_stats(centred, A, 30, 44) - T).max() <= 1e-14
    # a loop over one assignment
    a = A[7].astype(bool)
    loop = (K[np.ix_(a, a)].sum() / (30 * 29) + K[np.ix_(~a, ~a)].sum() / (44 * 43) - 2 * K[np.ix_(a, ~a)].sum() / (30 * 44))
    assert T[7] == pytest.approx(loop, rel=1e-11, abs=1e-15)
    assert KR.p_value(np.array([1.0, 0.5, 2.0, 1.0])) == 3.0 / 4.0 and KR.count_ge([1.0, 0.5, 2.0, 1.0], 0.5) == 1


def test_centring_holds_the_bar_and_the_uncentred_gram_does_not():
    """One cluster 0.5 wide, 100 sqrt(D) from the origin: the fp32 Gram form of the rows as they are misses float64's row
    means by more than the bar; centred on the column mean it holds the floor.  (On the clustered family, 10 sqrt(D)
    away, the mean over a row's columns still hides the uncentred form's error: 7e-7 at D = 187.)"""
    rng = np.random.default_rng(25)
    Y = (100.0 + 0.5 * rng.standard_normal((300, 16))).astype(np.float32)
    X = (100.0 + 0.5 * rng.standard_normal((130, 16))).astype(np.float32)
    gammas = KR.ladder(KR.sigma2(Y))
    cen = KR.e_ref_rowmeans(X, Y, gammas, KR.centre_of(Y))
    unc = KR.e_ref_rowmeans(X, Y, gammas, None)
    print(f"row means, one cluster at 100, D = 16: centred {cen:.3e}, uncentred {unc:.3e}, floor {KR.FLOOR:.1e}")
    assert cen <= KR.FLOOR < unc and unc > 3.0 * cen


@pytest.mark.parametrize("case", range(len(KR.PERM_CASES)))
def test_the_count_band_of_every_permutation_case(case):
    """The GPU test accepts a count of T_p >= T_0 between float64's counts at T_0 +- bar.  That band may hold at most
    BAND_MAX permutations for the seeds chosen: a condition on the inputs.  The shifted case rejects at 1 / (P + 1)."""
    X, Y, P = KR.perm_case(case)
    n, m = X.shape[0], Y.shape[0]
    assert (n, m, X.shape[1], P) == KR.PERM_CASES[case][:4]
    gammas = KR.ladder(KR.sigma2(Y))
    A = KR.assignments(n, m, P, KR.PERM_SEED)
    T = KR.perm_stats(KR.gram(X, Y, gammas), A, n, m)
    e_ref = float(np.abs(KR.perm_stats(KR.gram_mean32(X, Y, gammas, KR.centre_of(Y)), A, n, m) - T).max())
    bar = KR.bar(e_ref)
    lo, hi = KR.count_ge(T, bar), KR.count_ge(T, -bar)
    print(f"case {case}: T_0 {T[0]:.4e}, e_ref {e_ref:.2e}, bar {bar:.1e}, counts {lo} .. {hi}, p {KR.p_value(T):.4f}")
    assert bar == KR.FLOOR and lo <= KR.count_ge(T) <= hi and hi - lo <= KR.BAND_MAX
    if KR.PERM_CASES[case][4] > 0:
        assert hi == 0 and KR.p_value(T) == 1.0 / (P + 1)
    else:
        assert KR.p_value(T) > 0.05


def test_the_ladder_by_squaring_would_hold_the_bar_too():
    """The emulation DESIGN.md section 3 quotes: on the clustered 130 x 513 x 187 case (seed 1) the row means of a doubling
    ladder taken from the widest kernel by four squarings against one exp per gamma, both against float64."""
    A, B = KR.make_sets(130, 513, 187, "clustered", 1)
    centre = KR.centre_of(B)
    gammas = KR.ladder(KR.sigma2(B), (4.0, 2.0, 1.0, 0.5, 0.25))  # ascending gamma: scale 4 is the widest kernel
    want = KR.row_sums(A, B, gammas)
    each = np.abs(KR.row_sums32(A, B, gammas, centre) - want).max(axis=1) / 513
    squared = np.abs(KR.row_sums32_squaring(A, B, gammas, centre) - want).max(axis=1) / 513
    print("row-mean error, scales 4 ... 1/4: one exp each", " ".join(f"{e:.2e}" for e in each),
          "| by squaring", " ".join(f"{e:.2e}" for e in squared))
    assert each.max() <= 1e-7 and squared.max() <= 2e-7 and squared[0] == each[0]


def test_limit_inputs_are_answered_from_their_distinct_values():
    """The GPU limit tests compute float64's answer from the 1021 distinct values and their counts: on a short hashed set
    that is the direct restatement, for row sums both ways round and for the permutation statistic."""
    rows = KR.hashed_rows(3000)
    assert rows.min() == 0.0 and rows.max() == 1020.0 and KR.hashed_counts(rows).sum() == 3000
    few = np.array(KR.LIMIT_FEW, np.float32)[:, None]
    gammas = KR.ladder(KR.sigma2(KR.DISTINCT), (1.0, 0.25))
    by_value = KR.row_sums(KR.DISTINCT, few, gammas)
    assert np.array_equal(by_value[:, rows[:, 0].astype(int)], KR.row_sums(rows, few, gammas))
    d = KR.dist2(few, KR.DISTINCT)
    counted = np.stack([(np.exp(-g * d) * KR.hashed_counts(rows)).sum(axis=1) for g in gammas])
    assert np.abs(counted - KR.row_sums(few, rows, gammas)).max() <= 1e-10
    X, Y = rows[:120], rows[120:320]
    A = KR.assignments(120, 200, 25, 2)
    direct = KR.perm_stats(KR.gram(X, Y, gammas), A, 120, 200)
    got = KR.perm_stats_of_values(KR.mean_kernel_of_values(gammas), rows[:320, 0], A, 120, 200)
    assert np.abs(got - direct).max() <= 1e-13
    centre = KR.centre_of(Y)
    direct32 = KR.perm_stats(KR.gram_mean32(X, Y, gammas, centre), A, 120, 200)
    got32 = KR.perm_stats_of_values(KR.mean_kernel_of_values(gammas, centre), rows[:320, 0], A, 120, 200)
    assert np.abs(got32 - direct32).max() <= 1e-13
