"""CPU-side tests of the float64 moment statistics (no GPU): the C surface and its argument checks, the Python surface
(``utils.pca``, ``FrechetDistance``: refusals, keys, the kept originals, baseline and composition on a fake native layer),
and the numpy restatement (tests/pca_restatement.py) against a judge it shares no code with (``np.cov``,
``np.linalg.eigh``) and against closed forms: the 2 x 2 eigenproblem, unit and diagonal covariances, FD(Y, Y), symmetry in
the arguments, and the exact scaling that relative thresholds give."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import kernel_mmd_restatement as KR
import pca_restatement as PR
from host_entry_checks import HostBuffers, checks_work, refuses_every_alias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("ffd_cov_work_bytes", "ffd_cov", "ffd_sym_eig_work_bytes", "ffd_sym_eig", "ffd_sym_root_work_bytes", "ffd_sym_root",
         "ffd_frechet_work_bytes", "ffd_frechet", "ffd_pca_variances_work_bytes", "ffd_pca_variances", "ffd_pca_transform")
ARG_COUNTS = {"ffd_cov": 8, "ffd_sym_eig": 9, "ffd_sym_root": 7, "ffd_frechet": 12, "ffd_pca_variances": 8,
              "ffd_pca_transform": 8}
BIG_N, BIG_D = (1 << 24) + 1, 1025


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
    from fastfourierdiffusion_amd.utils import pca

    header = open(os.path.join(ROOT, "include", "ffd.h")).read()
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}
    for name in NAMES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        res, args = _header_args(header, name)
        want_res, want_args = N.SIGNATURES[name]
        assert ctype[res] is want_res, name
        assert [ctype.get(a, C.c_void_p) for a in args] == list(want_args), (name, args)
        assert all(a in ctype or a.endswith("*") for a in args), (name, args)
        if name in ARG_COUNTS:
            assert len(args) == ARG_COUNTS[name], name
    limit = re.search(r"FFD_PCA_MAX_D = (\d+)", header)
    assert limit and int(limit.group(1)) == pca.MAX_D == 1024
    csrc = os.path.join(ROOT, "fastfourierdiffusion_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "ffd_pca.hip" in make and "ffd_pca.o" in make and ".isa/ffd_pca.s" in make
    text = open(os.path.join(csrc, "ffd_pca.hip")).read()
    assert "atomic" not in text.replace("No atomics", "")
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in text  # the products run on the fp64 matrix instruction
    slab = re.search(r"constexpr int PCA_SLAB = (\d+);", text)
    assert slab and int(slab.group(1)) == PR.SLAB  # a constant of the source: what the tests' slab edge assumes


def test_work_bytes_monotone_and_zero_for_refused(lib):
    rows = (2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097, 16385, 60000, 1 << 20, 1 << 24)
    dims = (1, 2, 3, 15, 16, 17, 63, 64, 65, 187, 255, 256, 257, 1023, 1024)
    prev = 0
    for n in rows:
        b = lib.ffd_cov_work_bytes(n, 17)
        assert b > 0 and b >= prev and b % 16 == 0, (n, b, prev)
        prev = b
    prev = 0
    for D in dims:
        b = lib.ffd_cov_work_bytes(1025, D)
        assert b > 0 and b >= prev and b % 16 == 0, (D, b, prev)
        prev = b
    for bad in ((1, 4), (0, 4), (-1, 4), (4, 0), (4, -2), (BIG_N, 4), (4, BIG_D)):
        assert lib.ffd_cov_work_bytes(*bad) == 0, bad
    for query in (lib.ffd_sym_eig_work_bytes, lib.ffd_sym_root_work_bytes, lib.ffd_frechet_work_bytes):
        prev = 0
        for D in dims:
            b = query(D)
            assert b > 0 and b >= prev and b % 16 == 0, (D, b, prev)
            prev = b
        for bad in (0, -1, BIG_D):
            assert query(bad) == 0, bad
    assert lib.ffd_frechet_work_bytes(187) > lib.ffd_sym_eig_work_bytes(187) > lib.ffd_sym_root_work_bytes(187)
    for axis in range(2):
        prev = 0
        for v in (1, 2, 3, 15, 16, 17, 64, 65, 187):
            shape = [187, 10]
            shape[axis] = v
            shape[0] = max(shape)  # k <= D
            b = lib.ffd_pca_variances_work_bytes(*shape)
            assert b > 0 and b >= prev and b % 16 == 0, (axis, v, b, prev)
            prev = b
    for bad in ((0, 1), (4, 0), (4, 5), (4, -1), (BIG_D, 4)):
        assert lib.ffd_pca_variances_work_bytes(*bad) == 0, bad


def test_argument_errors_before_device_work(lib):
    n, D, k = 7, 5, 3
    cneed, eneed, rneed = lib.ffd_cov_work_bytes(n, D), lib.ffd_sym_eig_work_bytes(D), lib.ffd_sym_root_work_bytes(D)
    fneed, vneed = lib.ffd_frechet_work_bytes(D), lib.ffd_pca_variances_work_bytes(D, k)
    vec, mat = D * 8, D * D * 8
    b = HostBuffers(x=n * D * 4, mean=vec, cov=mat, work=max(cneed, eneed, rneed, fneed, vneed), a=mat, w=vec, v=mat, info=24,
                     root=mat, mx=vec, cx=mat, my=vec, cy=mat, out5=40, out=k * 8, scores=n * k * 8)

    def cov(x=b.x, n=n, D=D, mean=b.mean, cov=b.cov, work=b.work, nbytes=cneed):
        return lib.ffd_cov(x, n, D, mean, cov, work, nbytes, None)

    for kw in (dict(x=None), dict(mean=None), dict(cov=None), dict(work=None), dict(n=1), dict(n=0), dict(n=-3), dict(D=0),
               dict(D=-1), dict(nbytes=0), dict(nbytes=cneed - 1), dict(work=b.work + 8), dict(work=b.x), dict(work=b.mean),
               dict(work=b.cov), dict(mean=b.x), dict(cov=b.x), dict(cov=b.mean), dict(mean=b.cov)):
        assert cov(**kw) == INVALID, kw
    # every written region on every other region, optional ones given and left out; the workspace misaligned, a byte
    # short, and exactly the need
    assert refuses_every_alias(cov, dict(mean=b.mean, cov=b.cov, work=b.work), dict(x=b.x)) == 9
    checks_work(cov, b.work, cneed)
    assert cov(n=BIG_N) == UNSUPPORTED and cov(D=BIG_D) == UNSUPPORTED

    def eig(a=b.a, D=D, max_sweeps=30, w=b.w, v=b.v, info=b.info, work=b.work, nbytes=eneed):
        return lib.ffd_sym_eig(a, D, max_sweeps, w, v, info, work, nbytes, None)

    for kw in (dict(a=None), dict(w=None), dict(info=None), dict(work=None), dict(D=0), dict(D=-2), dict(max_sweeps=-1),
               dict(nbytes=0), dict(nbytes=eneed - 1), dict(work=b.work + 8), dict(work=b.a), dict(work=b.w), dict(work=b.v),
               dict(w=b.a), dict(v=b.a), dict(v=b.w), dict(w=b.v)):
        assert eig(**kw) == INVALID, kw
    for kw in (dict(a=None), dict(w=None), dict(info=None), dict(work=None), dict(D=0), dict(max_sweeps=-1),
               dict(nbytes=eneed - 1), dict(work=b.work + 8), dict(work=b.a), dict(work=b.w), dict(w=b.a)):
        assert eig(v=None, **kw) == INVALID, kw  # ... and without vectors
    assert refuses_every_alias(eig, dict(w=b.w, v=b.v, work=b.work), dict(a=b.a)) == 9
    assert refuses_every_alias(partial(eig, v=None), dict(w=b.w, v=None, work=b.work), dict(a=b.a)) == 4
    checks_work(eig, b.work, eneed)
    checks_work(partial(eig, v=None), b.work, eneed)
    assert eig(D=BIG_D) == UNSUPPORTED and eig(D=BIG_D, v=None) == UNSUPPORTED

    def root(w=b.w, v=b.v, D=D, out=b.root, work=b.work, nbytes=rneed):
        return lib.ffd_sym_root(w, v, D, out, work, nbytes, None)

    for kw in (dict(w=None), dict(v=None), dict(out=None), dict(work=None), dict(D=0), dict(D=-1), dict(nbytes=0),
               dict(nbytes=rneed - 1), dict(work=b.work + 8), dict(work=b.w), dict(work=b.v), dict(work=b.root), dict(out=b.w),
               dict(out=b.v)):
        assert root(**kw) == INVALID, kw
    assert refuses_every_alias(root, dict(out=b.root, work=b.work), dict(w=b.w, v=b.v)) == 6
    checks_work(root, b.work, rneed)
    assert root(D=BIG_D) == UNSUPPORTED

    def fd(mx=b.mx, cx=b.cx, my=b.my, cy=b.cy, root=b.root, D=D, max_sweeps=30, out5=b.out5, info=b.info, work=b.work,
           nbytes=fneed):
        return lib.ffd_frechet(mx, cx, my, cy, root, D, max_sweeps, out5, info, work, nbytes, None)

    for kw in (dict(mx=None), dict(cx=None), dict(my=None), dict(cy=None), dict(out5=None), dict(info=None), dict(work=None),
               dict(D=0), dict(D=-1), dict(max_sweeps=-1), dict(nbytes=0), dict(nbytes=fneed - 1), dict(work=b.work + 8),
               dict(work=b.mx), dict(work=b.cx), dict(work=b.my), dict(work=b.cy), dict(work=b.out5), dict(out5=b.mx),
               dict(out5=b.cx), dict(out5=b.my), dict(out5=b.cy)):
        assert fd(**kw) == INVALID, kw
        assert fd(root=None, **kw) == INVALID, kw  # ... and without a supplied root
    assert fd(work=b.root) == INVALID and fd(out5=b.root) == INVALID
    fd_in = dict(mx=b.mx, cx=b.cx, my=b.my, cy=b.cy)
    assert refuses_every_alias(fd, dict(out5=b.out5, work=b.work), dict(fd_in, root=b.root)) == 12
    assert refuses_every_alias(partial(fd, root=None), dict(out5=b.out5, work=b.work), dict(fd_in, root=None)) == 10
    checks_work(fd, b.work, fneed)
    checks_work(partial(fd, root=None), b.work, fneed)
    assert fd(D=BIG_D) == UNSUPPORTED and fd(D=BIG_D, root=None) == UNSUPPORTED

    def pcv(cov=b.cov, v=b.v, D=D, k=k, out=b.out, work=b.work, nbytes=vneed):
        return lib.ffd_pca_variances(cov, v, D, k, out, work, nbytes, None)

    for kw in (dict(cov=None), dict(v=None), dict(out=None), dict(work=None), dict(D=0), dict(k=0), dict(k=-1), dict(k=D + 1),
               dict(nbytes=0), dict(nbytes=vneed - 1), dict(work=b.work + 8), dict(work=b.cov), dict(work=b.v), dict(work=b.out),
               dict(out=b.cov), dict(out=b.v)):
        assert pcv(**kw) == INVALID, kw
    assert refuses_every_alias(pcv, dict(out=b.out, work=b.work), dict(cov=b.cov, v=b.v)) == 6
    checks_work(pcv, b.work, vneed)
    assert pcv(D=BIG_D) == UNSUPPORTED

    def tr(x=b.x, n=n, D=D, mean=b.mean, v=b.v, k=k, scores=b.scores):
        return lib.ffd_pca_transform(x, n, D, mean, v, k, scores, None)

    for kw in (dict(x=None), dict(mean=None), dict(v=None), dict(scores=None), dict(n=0), dict(n=-1), dict(D=0), dict(k=0),
               dict(k=D + 1), dict(scores=b.x), dict(scores=b.mean), dict(scores=b.v)):
        assert tr(**kw) == INVALID, kw
    assert refuses_every_alias(tr, dict(scores=b.scores), dict(x=b.x, mean=b.mean, v=b.v)) == 3
    assert tr(n=BIG_N) == UNSUPPORTED and tr(D=BIG_D) == UNSUPPORTED
    assert b.untouched()


# ------------------------------------------------------------------ the Python surface ----
class _FakeLib:
    """Stands in for libffd: reads the arrays the binding passes (host memory here) and answers with the restatements."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).reshape(shape)

    def _bytes(self, *shape):
        return 64

    ffd_mmd_centre_work_bytes = ffd_mmd_bandwidth_work_bytes = ffd_mmd_rowsums_work_bytes = _bytes
    ffd_cov_work_bytes = ffd_sym_eig_work_bytes = ffd_sym_root_work_bytes = ffd_frechet_work_bytes = _bytes
    ffd_pca_variances_work_bytes = _bytes

    def ffd_mmd_centre(self, x, n, D, out, work, nbytes, stream):
        self._arr(out, (D,), np.float32)[:] = KR.centre_of(self._arr(x, (n, D), np.float32))
        return 0

    def ffd_mmd_bandwidth(self, y, n, D, out, work, nbytes, stream):
        self._arr(out, (1,), np.float64)[0] = KR.sigma2(self._arr(y, (n, D), np.float32))
        return 0

    def ffd_mmd_rowsums(self, a, na, b, nb, D, centre, gammas, ng, excl, out, work, nbytes, stream):
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

    def ffd_cov(self, x, n, D, mean, cov, work, nbytes, stream):
        self.calls.append(("cov", n, D))
        m, c = PR.covariance(self._arr(x, (n, D), np.float32))
        self._arr(mean, (D,), np.float64)[:] = m
        self._arr(cov, (D, D), np.float64)[:] = c
        return 0

    def ffd_sym_eig(self, a, D, max_sweeps, w, v, info, work, nbytes, stream):
        self.calls.append(("eig", D, max_sweeps, v is not None))
        lam, vec, sweeps, ratio, done = PR.jacobi_eigh(self._arr(a, (D, D), np.float64), v is not None, max_sweeps)
        self._arr(w, (D,), np.float64)[:] = lam
        if v is not None:
            self._arr(v, (D, D), np.float64)[:] = vec
        self._arr(info, (3,), np.float64)[:] = [sweeps, ratio, float(done)]
        return 0

    def ffd_sym_root(self, w, v, D, root, work, nbytes, stream):
        self.calls.append(("root", D))
        self._arr(root, (D, D), np.float64)[:] = PR.sym_root(self._arr(w, (D,), np.float64), self._arr(v, (D, D), np.float64))
        return 0

    def ffd_frechet(self, mx, cx, my, cy, root, D, max_sweeps, out5, info, work, nbytes, stream):
        self.calls.append(("frechet", D, root is not None))
        f = PR.frechet(self._arr(mx, (D,), np.float64), self._arr(cx, (D, D), np.float64), self._arr(my, (D,), np.float64),
                       self._arr(cy, (D, D), np.float64), None if root is None else self._arr(root, (D, D), np.float64))
        self._arr(out5, (5,), np.float64)[:] = [f["fd"], f["mean_term"], f["cov_term"], f["trace_x"], f["trace_y"]]
        self._arr(info, (3,), np.float64)[:] = [1.0, 0.0, 1.0]
        return 0

    def ffd_pca_variances(self, cov, v, D, k, out, work, nbytes, stream):
        self.calls.append(("variances", D, k))
        self._arr(out, (k,), np.float64)[:] = PR.pc_variances(self._arr(cov, (D, D), np.float64),
                                                              self._arr(v, (D, D), np.float64), k)
        return 0

    def ffd_pca_transform(self, x, n, D, mean, v, k, scores, stream):
        self.calls.append(("transform", n, D, k))
        self._arr(scores, (n, k), np.float64)[:] = PR.transform(self._arr(x, (n, D), np.float32),
                                                                self._arr(mean, (D,), np.float64),
                                                                self._arr(v, (D, D), np.float64), k)
        return 0


def _host_rows(x, name="x", min_rows=1):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    assert t.dim() == 2 and t.shape[0] >= min_rows
    return t.to(torch.float32).contiguous()


def _f64_on_host(x, name, shape):
    assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and tuple(x.shape) == tuple(shape), name
    return x.contiguous()


@pytest.fixture
def fake(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling import metrics
    from fastfourierdiffusion_amd.utils import kernel_mmd, pca

    f = _FakeLib()
    monkeypatch.setattr(metrics, "_to_device", _host_rows)
    monkeypatch.setattr(N, "lib", lambda: f)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: 0)
    for module in (kernel_mmd, pca):
        monkeypatch.setattr(module, "_rows", _host_rows)
        monkeypatch.setattr(module, "_f64", _f64_on_host)
    monkeypatch.setattr(kernel_mmd, "_centre", lambda c, D: c.reshape(-1))
    return f


def _require_host(t, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise AssertionError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def test_python_refusals_before_any_native_call(monkeypatch):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import FrechetDistance
    from fastfourierdiffusion_amd.utils import pca

    def no_native():
        raise AssertionError("a native call was reached")

    monkeypatch.setattr(N, "lib", no_native)
    X = PR.make_rows(20, 4, "offset", 1)
    tx = torch.from_numpy(X)
    mean, cov = (torch.from_numpy(a) for a in PR.covariance(X))
    w, v = (torch.from_numpy(a) for a in PR.jacobi_eigh(cov.numpy())[:2])
    # host tensors and arrays: a clear error, no upload and no fallback
    for call in (lambda: pca.covariance(tx), lambda: pca.transform(tx, mean, v, 2)):
        with pytest.raises(N.FFDError, match="no CPU fallback"):
            call()
    for call in (lambda: pca.eigh(cov), lambda: pca.sym_root(w, v), lambda: pca.frechet_distance(mean, cov, mean, cov),
                 lambda: pca.pc_variances(cov, v, 2)):
        with pytest.raises(N.FFDError):
            call()
    for call in (lambda: pca.covariance(X), lambda: pca.eigh(cov.numpy()), lambda: pca.sym_root(w, v.numpy())):
        with pytest.raises(TypeError):
            call()
    # dtype, shape and counts, on a layer that accepts host tensors
    monkeypatch.setattr(N, "require_gpu_tensor", _require_host)
    monkeypatch.setattr(pca, "_f64", _f64_on_host)
    for call in (lambda: pca.covariance(tx[:1]), lambda: pca.covariance(tx[0]), lambda: pca.covariance(tx.double()),
                 lambda: pca.covariance(torch.zeros(3, pca.MAX_D + 1)),
                 lambda: pca.eigh(cov[:3]), lambda: pca.eigh(cov.float()), lambda: pca.eigh(cov, max_sweeps=0),
                 lambda: pca.eigh(torch.zeros(pca.MAX_D + 1, pca.MAX_D + 1, dtype=torch.float64)),
                 lambda: pca.sym_root(w[:3], v), lambda: pca.sym_root(w.float(), v), lambda: pca.sym_root(w, v[:3]),
                 lambda: pca.frechet_distance(mean[:3], cov, mean, cov), lambda: pca.frechet_distance(mean, cov, mean, cov[:3, :3]),
                 lambda: pca.frechet_distance(mean, cov, mean.float(), cov),
                 lambda: pca.frechet_distance(mean, cov, mean, cov, root_y=cov[:3]),
                 lambda: pca.frechet_distance(mean, cov, mean, cov, max_sweeps=-2),
                 lambda: pca.pc_variances(cov, v, 0), lambda: pca.pc_variances(cov, v, 5), lambda: pca.pc_variances(cov, v[:3, :3], 2),
                 lambda: pca.transform(tx, mean, v, 0), lambda: pca.transform(tx, mean, v, 5),
                 lambda: pca.transform(tx, mean[:3], v, 2), lambda: pca.transform(tx[:, :3], mean, v, 2),
                 lambda: pca.transform(tx, mean, v.float(), 2)):
        with pytest.raises(AssertionError):
            call()
    for kwargs in (dict(components=0), dict(components=-1)):
        with pytest.raises(AssertionError):
            FrechetDistance(X, **kwargs)
    with pytest.raises(AssertionError):
        FrechetDistance(X[:1])
    with pytest.raises(AssertionError):
        FrechetDistance(np.zeros((4, pca.MAX_D + 1), np.float32))


def test_eigh_raises_when_the_cap_is_hit(fake):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.utils import pca

    a = torch.from_numpy(PR.make_matrix(16, "indefinite", 3))
    with pytest.raises(N.FFDError, match="did not converge in 1 sweeps"):
        pca.eigh(a, max_sweeps=1)
    w, v, info = pca.eigh(a, info=True)
    assert 1 < info.sweeps <= 20 and info.off <= PR.STOP and fake.calls[-1] == ("eig", 16, 30, True)
    assert torch.equal(pca.eigh(a, vectors=False), w) and fake.calls[-1] == ("eig", 16, 30, False)


def test_frechet_distance_keys_kept_originals_and_baseline(fake):
    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y = PR.make_rows(40, 6, "offset", 2), PR.make_rows(56, 6, "offset", 3)
    metric = M.FrechetDistance(Y, components=4)
    assert metric.name == "frechet" and isinstance(metric, M.Metric) and M.FrechetDistance.views == M.Metric.views
    got = metric(X)
    assert tuple(got) == PR.KEYS and all(isinstance(v, float) for v in got.values())
    want = PR.pipeline(X, Y, components=4)
    for key, value in want.items():
        assert got[key] == pytest.approx(value, rel=1e-12, abs=1e-15), key
    assert got["frechet_w2"] == max(got["frechet_distance"], 0.0) ** 0.5
    assert got["frechet_distance"] == got["frechet_mean_term"] + got["frechet_cov_term"]
    assert [c[0] for c in fake.calls] == ["cov", "eig", "root", "cov", "frechet", "variances"]
    assert fake.calls[0] == ("cov", 56, 6) and fake.calls[4] == ("frechet", 6, True) and fake.calls[5] == ("variances", 6, 4)
    fake.calls.clear()
    assert metric(X) == got
    assert [c[0] for c in fake.calls] == ["cov", "frechet", "variances"]  # the originals' part is kept
    # more components than features: all of them
    assert tuple(M.FrechetDistance(Y, components=10)(X)) == PR.KEYS and fake.calls[-1] == ("variances", 6, 6)
    scores = metric.transform(X, 3)
    mean_y, _, w, v, _ = PR.moments(Y)
    assert scores.dtype == torch.float64 and scores.shape == (40, 3)
    assert np.allclose(scores.numpy(), PR.transform(X, mean_y, v, 3), rtol=1e-12, atol=1e-14)
    spectrum = metric.explained_variance()
    assert spectrum.shape == (6,) and np.array_equal(spectrum.numpy(), w[::-1]) and (spectrum[:-1] >= spectrum[1:]).all()
    base = metric.baseline_metrics
    assert tuple(base) == tuple(f"{key}_self" for key in PR.KEYS) and not any(key.endswith("_dummy") for key in base)
    fake.calls.clear()
    assert metric.baseline_metrics == base and not fake.calls  # a function of the originals alone: kept
    for key, value in PR.baseline(Y, components=4).items():
        assert base[key] == pytest.approx(value, rel=1e-12, abs=1e-15), key


def test_metric_collection_composes_the_metric_and_leaves_the_others(fake, monkeypatch):
    from fastfourierdiffusion_amd.sampling import FrechetDistance, KernelMMD
    from fastfourierdiffusion_amd.sampling import metrics as M

    monkeypatch.setattr(M, "dft", lambda x: np.asarray(x)[:, ::-1].copy())  # any other view of the rows
    X, Y = PR.make_rows(24, 5, "offset", 4), PR.make_rows(30, 5, "offset", 5)
    mmd_keys = ("mmd2", "mmd2_biased", "mmd2_s0.5", "mmd2_s2", "witness_max", "witness_share_positive")
    alone = M.MetricCollection([partial(KernelMMD, scales=(0.5, 2))], original_samples=Y)(X)
    coll = M.MetricCollection([partial(KernelMMD, scales=(0.5, 2)), partial(FrechetDistance, components=3)], original_samples=Y)
    found = coll(X)
    want = sorted(f"{p}_{key}{suffix}" for p in ("time", "freq") for key in mmd_keys + PR.KEYS for suffix in ("", "_self"))
    assert list(found) == want
    ours = {f"{p}_{key}{suffix}" for p in ("time", "freq") for key in PR.KEYS for suffix in ("", "_self")}
    assert {k: v for k, v in found.items() if k not in ours} == alone  # the other metric's keys and values: unchanged
    assert found["time_frechet_distance"] == pytest.approx(PR.pipeline(X, Y, components=3)["frechet_distance"], rel=1e-12)
    assert found["freq_frechet_distance"] == pytest.approx(PR.pipeline(X[:, ::-1], Y[:, ::-1], 3)["frechet_distance"], rel=1e-9)
    assert M.Metric.views == ("time", "freq") and M.FrechetDistance.views == ("time", "freq")


# ------------------------------------------------------------------ the restatement against the judge ----
@pytest.mark.parametrize("D", PR.EIG_DIMS)
def test_restated_eigensolver_against_lapack(D):
    """Measured with exactly this algorithm: at most 18 sweeps (D = 256, rank deficient), eigenvalue error at most
    0.86 D 2^-52 |A|_F (D = 2) and 0.15 D 2^-52 |A|_F from D = 16 on, |V^T V - I| at most 2.5 D 2^-52."""
    for kind in PR.KINDS:
        case = PR.restated_case(D, kind)
        a, w, v = case["a"], case["w"], case["v"]
        assert np.array_equal(a, a.T)
        print(f"D = {D} {kind}: {case['sweeps']} sweeps, eigenvalues off by {case['e_val'] / (D * PR.EPS * case['fro']):.3f}, "
              f"residual {case['res'] / (D * PR.EPS * case['fro']):.3f} (D 2^-52 |A|_F), |V^T V - I| "
              f"{case['orth'] / (D * PR.EPS):.3f} (D 2^-52)")
        assert case["done"] and case["sweeps"] <= 20 and case["ratio"] <= PR.STOP
        assert case["e_val"] <= D * PR.EPS * case["fro"], kind
        assert case["res"] <= D * PR.EPS * case["fro"], kind
        assert case["orth"] <= 3 * D * PR.EPS, kind
        assert (np.diff(w) >= 0).all()
        if kind in ("identity", "diagonal"):
            assert case["sweeps"] == 0 and np.array_equal(w, np.sort(np.diag(a))) and case["e_val"] == 0.0
        if kind == "indefinite" and D > 1:
            assert w[0] < 0 < w[-1]
        if kind == "rank_deficient" and D >= 16:  # the eigenvalues LAPACK puts at zero are zero within the bar
            assert np.abs(w[: D - D // 2]).max() <= D * PR.EPS * case["fro"]
        if D <= 64:
            assert np.array_equal(PR.jacobi_eigh(a, vectors=False)[0], w)  # the values do not depend on the vectors


@pytest.mark.parametrize("family", PR.FAMILIES)
def test_restated_covariance_against_numpy(family):
    for n, D in ((2, 1), (3, 15), (65, 17), (PR.SLAB + 1, 187)):
        x = PR.make_rows(n, D, family, 11)
        mean, cov = PR.covariance(x)
        jm, jc = PR.judge_cov(x)
        scale = np.sqrt(np.outer(np.diag(jc), np.diag(jc)))
        assert np.array_equal(cov, cov.T)
        assert (np.abs(mean - jm) <= n * 2.0 ** -53 * np.abs(x.astype(np.float64)).mean(axis=0)).all()
        assert (np.abs(cov - jc) <= 2 * n * 2.0 ** -53 * scale).all()


def test_two_by_two_eigenproblem_in_closed_form():
    rng = np.random.default_rng(5)
    for _ in range(50):
        a, b, d = rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4, 3)
        w, v, sweeps, _, done = PR.jacobi_eigh(np.array([[a, b], [b, d]]))
        mid, rad = (a + d) / 2.0, np.hypot((a - d) / 2.0, b)
        assert done and sweeps <= 2
        assert np.abs(w - [mid - rad, mid + rad]).max() <= 4 * PR.EPS * (abs(mid) + rad)
        assert np.abs(v.T @ v - np.eye(2)).max() <= 4 * PR.EPS


def _full_rank_pair(D, seed):
    X, Y = PR.make_rows(3 * D + 1, D, "offset", seed), PR.make_rows(2 * D + 3, D, "offset", seed + 1)
    return PR.covariance(X) + PR.covariance(Y)


def test_frechet_closed_forms():
    rng = np.random.default_rng(6)
    for D in (1, 2, 7, 32):
        a, b = rng.standard_normal(D), rng.standard_normal(D)
        f = PR.frechet(a, np.eye(D), b, np.eye(D))
        assert f["cov_term"] == 0.0 and f["fd"] == f["mean_term"] == float((a - b) @ (a - b))  # N(a, I) against N(b, I)
        # diagonal covariances: sum (sqrt a_i - sqrt b_i)^2
        va, vb = rng.uniform(0.1, 4.0, D), rng.uniform(0.1, 4.0, D)
        f = PR.frechet(a, np.diag(va), a, np.diag(vb))
        want = float(((np.sqrt(va) - np.sqrt(vb)) ** 2).sum())
        assert f["mean_term"] == 0.0 and abs(f["fd"] - want) <= 4 * D * PR.EPS * float(va.sum() + vb.sum())


@pytest.mark.parametrize("D", [16, 187])
def test_frechet_against_the_judge_zero_and_symmetry(D):
    """The judge cannot tell answers closer than its own spread apart; D 2^-52 (tr S_x + tr S_y) is the rounding of the
    D square roots and the sums the value is made of."""
    mx, cx, my, cy = _full_rank_pair(D, 20 + D)
    scale = float(np.trace(cx) + np.trace(cy))
    spread = PR.judge_spread(mx, cx, my, cy)
    floor = D * PR.EPS * scale
    f_xy, f_yx = PR.frechet(mx, cx, my, cy), PR.frechet(my, cy, mx, cx)
    judge = PR.judge_fd(mx, cx, my, cy)
    print(f"D = {D}: FD {f_xy['fd']:.12f}, judge {judge:.12f}, off by {abs(f_xy['fd'] - judge) / scale:.2e} of the traces; "
          f"judge's spread {spread / scale:.2e}; FD(Y, Y) {PR.frechet(my, cy, my, cy)['fd'] / scale:.2e}")
    assert spread <= 8e-14 * scale
    assert abs(f_xy["fd"] - judge) <= max(10 * spread, floor)
    assert abs(f_xy["fd"] - f_yx["fd"]) <= max(10 * spread, floor)  # symmetric in its arguments
    assert f_xy["fd"] > 0 and f_xy["mean_term"] >= 0
    same = PR.frechet(my, cy, my, cy)
    assert same["mean_term"] == 0.0 and abs(same["fd"]) <= max(10 * abs(PR.judge_fd(my, cy, my, cy)), floor)


def test_rows_times_two_scale_everything_bit_for_bit():
    """All thresholds are relative: nothing in the chain knows the data's unit."""
    for family in PR.FAMILIES:
        X, Y = PR.make_rows(40, 12, family, 30), PR.make_rows(50, 12, family, 31)
        mx, cx = PR.covariance(X)
        my, cy = PR.covariance(Y)
        mx2, cx2 = PR.covariance(X * np.float32(2))
        my2, cy2 = PR.covariance(Y * np.float32(2))
        assert np.array_equal(mx2, 2 * mx) and np.array_equal(cx2, 4 * cx)
        w, v = PR.jacobi_eigh(cy)[:2]
        w4, v4 = PR.jacobi_eigh(cy2)[:2]
        assert np.array_equal(w4, 4 * w) and np.array_equal(v4, v)
        f, f4 = PR.frechet(mx, cx, my, cy), PR.frechet(mx2, cx2, my2, cy2)
        assert all(f4[key] == 4 * f[key] for key in f), family
