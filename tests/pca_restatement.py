"""A float64 numpy restatement of csrc/ffd_pca.hip (the same algorithm: deviation-form covariance, cyclic Jacobi in the
round-robin order with Rutishauser's rotation and relative thresholds only, the mirrored root, the Frechet distance through
the eigenvalues of the symmetrised S_y^1/2 S_x S_y^1/2) and, apart from it, a judge that shares no code with it: ``np.cov``,
``np.linalg.eigh`` and the Frechet distance through LAPACK.  Input families and matrix kinds for both test files."""
from functools import lru_cache

import numpy as np

EPS = 2.0 ** -52
STOP = 2.0 ** -53          # a sweep starts only while off(A) > STOP |A|_F
MAX_SWEEPS = 30
SLAB = 256                 # csrc/ffd_pca.hip PCA_SLAB: rows per covariance slab
FAMILIES = ("series", "offset", "anisotropic")
KINDS = ("series", "rank_deficient", "anisotropic", "indefinite", "identity", "diagonal")
EIG_DIMS = (1, 2, 3, 16, 17, 64, 187, 256)
KEYS = ("frechet_distance", "frechet_w2", "frechet_mean_term", "frechet_cov_term", "variance_ratio",
        "pc_variance_ratio_min", "pc_variance_ratio_max")


# ------------------------------------------------------------------ inputs ----
def make_rows(n, D, family, seed):
    """(n, D) fp32 rows.  series: random sinusoids of 1-5 cycles plus 0.05 noise (an ill-conditioned covariance); offset:
    mean 100, unit spread; anisotropic: Gaussian columns scaled 1 .. 1e-6."""
    rng = np.random.default_rng(seed)
    if family == "series":
        t = np.arange(D) / max(D, 1)
        cycles = rng.integers(1, 6, (n, 1))
        phase = rng.uniform(0, 2 * np.pi, (n, 1))
        amp = rng.uniform(0.5, 1.5, (n, 1))
        x = amp * np.sin(2 * np.pi * cycles * t[None, :] + phase) + 0.05 * rng.standard_normal((n, D))
    elif family == "offset":
        x = 100.0 + rng.standard_normal((n, D))
    elif family == "anisotropic":
        x = rng.standard_normal((n, D)) * np.logspace(0, -6, D)[None, :]
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_matrix(D, kind, seed):
    """A (D, D) float64 matrix, symmetric bit for bit."""
    rng = np.random.default_rng(seed)
    if kind == "series":
        a = np.cov(make_rows(4 * D + 2, D, "series", seed).astype(np.float64), rowvar=False).reshape(D, D)
    elif kind == "rank_deficient":
        a = np.cov(make_rows(max(D // 2, 2), D, "series", seed).astype(np.float64), rowvar=False).reshape(D, D)
    elif kind == "anisotropic":
        a = np.cov(make_rows(4 * D + 2, D, "anisotropic", seed).astype(np.float64), rowvar=False).reshape(D, D)
    elif kind == "indefinite":
        a = rng.standard_normal((D, D))
    elif kind == "identity":
        return np.eye(D)
    elif kind == "diagonal":
        return np.diag(rng.permutation(D).astype(np.float64) - D / 3.0)
    else:
        raise ValueError(kind)
    return mirror(0.5 * (a + a.T))


def mirror(a):
    """The upper triangle on both sides."""
    u = np.triu(a)
    return u + np.triu(a, 1).T


# ------------------------------------------------------------------ the restatement ----
def covariance(x):
    """(mean, unbiased covariance) in the deviation form, float64."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    dev = x - mean
    return mean, mirror(dev.T @ dev) / (n - 1)


@lru_cache(maxsize=None)
def round_pairs(D, rnd):
    """The pairs (p < q) of round ``rnd`` of the round-robin order over D indices, D rounded up to even; a pair with the
    padded index is left out."""
    npad = D + (D & 1)
    m = npad - 1
    k = np.arange(1, npad // 2)
    a = np.concatenate([[m], (rnd + k) % m])
    b = np.concatenate([[rnd], (rnd - k + m) % m])
    p, q = np.minimum(a, b), np.maximum(a, b)
    keep = q < D
    return p[keep], q[keep]


def off_ratio(a):
    """off(A) / |A|_F with the two sums of squares kept apart (0 for the zero matrix)."""
    off = a - np.diag(np.diag(a))
    off2 = float((off * off).sum())
    all2 = off2 + float((np.diag(a) ** 2).sum())
    return np.sqrt(off2 / all2) if all2 > 0 else 0.0


def jacobi_eigh(a, vectors=True, max_sweeps=MAX_SWEEPS):
    """(w ascending, v or None, sweeps, final off / |A|_F, converged)."""
    a = mirror(np.asarray(a, np.float64))
    D = a.shape[0]
    vt = np.eye(D) if vectors else None  # the vectors as rows
    rounds = D + (D & 1) - 1
    sweeps = 0
    while True:
        ratio = off_ratio(a)
        done = ratio <= STOP
        if done or sweeps == max_sweeps:
            break
        for rnd in range(rounds):
            p, q = round_pairs(D, rnd)
            if p.size == 0:
                continue
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                tau = (aqq - app) / (2.0 * apq)
                t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            t = np.where(apq != 0.0, t, 0.0)
            c = np.where(apq != 0.0, 1.0 / np.sqrt(1.0 + t * t), 1.0)
            s = t * c
            # B = A J, column p of it c a_p - s a_q and column q s a_p + c a_q: formed as the rows of its transpose (A is
            # symmetric bit for bit), then R = J^T B by rows; an index without a partner this round keeps its row
            sit_out = [rnd] if D & 1 else []
            cc, ss = c[:, None], s[:, None]
            ap, aq = a[p], a[q]
            bt = np.empty_like(a)
            bt[p], bt[q], bt[sit_out] = cc * ap - ss * aq, ss * ap + cc * aq, a[sit_out]
            b = np.ascontiguousarray(bt.T)
            bp, bq = b[p], b[q]
            r = np.empty_like(a)
            r[p], r[q], r[sit_out] = cc * bp - ss * bq, ss * bp + cc * bq, b[sit_out]
            r = mirror(r)
            r[p, p], r[q, q] = app - t * apq, aqq + t * apq
            r[p, q] = r[q, p] = 0.0
            a = r
            if vectors:
                vp, vq = vt[p], vt[q]
                vt[p], vt[q] = cc * vp - ss * vq, ss * vp + cc * vq
        sweeps += 1
    w = np.diag(a).copy()
    order = np.argsort(w, kind="stable")
    return w[order], (np.ascontiguousarray(vt[order].T) if vectors else None), sweeps, ratio, done


def sym_root(w, v):
    return mirror((v * np.sqrt(np.maximum(w, 0.0))[None, :]) @ v.T)


def frechet(mean_x, cov_x, mean_y, cov_y, root_y=None):
    """{FD, mean term, covariance term, tr S_x, tr S_y} as the library forms them."""
    if root_y is None:
        w, v = jacobi_eigh(cov_y)[:2]
        root_y = sym_root(w, v)
    m = root_y @ (cov_x @ root_y)
    lam = jacobi_eigh(0.5 * (m + m.T), vectors=False)[0]
    gap = np.asarray(mean_x) - np.asarray(mean_y)
    mean_term = float(gap @ gap)
    tx, ty = float(np.trace(cov_x)), float(np.trace(cov_y))
    cov_term = (tx + ty) - 2.0 * float(np.sqrt(np.maximum(lam, 0.0)).sum())
    return {"fd": mean_term + cov_term, "mean_term": mean_term, "cov_term": cov_term, "trace_x": tx, "trace_y": ty}


def pc_variances(cov, v, k):
    top = v[:, ::-1][:, :k]
    return np.einsum("di,de,ei->i", top, cov, top)


def transform(x, mean, v, k):
    return (np.asarray(x, np.float64) - mean) @ v[:, ::-1][:, :k]


def moments(y):
    mean, cov = covariance(y)
    w, v = jacobi_eigh(cov)[:2]
    return mean, cov, w, v, sym_root(w, v)


def metric_values(X, prepared, components=10):
    """What ``FrechetDistance`` reports for samples X against prepared originals."""
    mean_y, cov_y, w, v, root = prepared
    mean_x, cov_x = covariance(X)
    f = frechet(mean_x, cov_x, mean_y, cov_y, root)
    k = min(components, w.size)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios = pc_variances(cov_x, v, k) / w[::-1][:k]
    return dict(zip(KEYS, (f["fd"], max(f["fd"], 0.0) ** 0.5, f["mean_term"], f["cov_term"], f["trace_x"] / f["trace_y"],
                           float(ratios.min()), float(ratios.max()))))


def pipeline(X, Y, components=10):
    return metric_values(X, moments(Y), components)


def baseline(Y, components=10):
    half = Y.shape[0] // 2
    return {f"{key}_self": value for key, value in metric_values(Y[half:], moments(Y[:half]), components).items()}


# ------------------------------------------------------------------ the judge (LAPACK; shares nothing with the above) ----
def judge_cov(x):
    x = np.asarray(x, np.float64)
    return x.mean(axis=0), np.cov(x, rowvar=False).reshape(x.shape[1], x.shape[1])


def judge_fd(mean_x, cov_x, mean_y, cov_y):
    lam_y, vec_y = np.linalg.eigh(cov_y)
    half = (vec_y * np.sqrt(np.clip(lam_y, 0.0, None))) @ vec_y.T
    inner = half @ cov_x @ half
    lam = np.linalg.eigvalsh((inner + inner.T) / 2.0)
    d = np.asarray(mean_x) - np.asarray(mean_y)
    return float(d @ d) + float(np.trace(cov_x) + np.trace(cov_y) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def judge_spread(mean_x, cov_x, mean_y, cov_y):
    """How far the judge's two argument orders lie apart: it cannot tell answers closer than this apart."""
    return abs(judge_fd(mean_x, cov_x, mean_y, cov_y) - judge_fd(mean_y, cov_y, mean_x, cov_x))


# ------------------------------------------------------------------ what both test files measure once ----
def eig_errors(a, w, v):
    """(eigenvalue error against LAPACK, residual |A V - V diag(w)|_max, |V^T V - I|_max) of a decomposition of ``a``."""
    lam = np.linalg.eigvalsh(a)
    e_val = float(np.abs(np.asarray(w) - lam).max())
    if v is None:
        return e_val, None, None
    res = float(np.abs(a @ v - v * np.asarray(w)[None, :]).max())
    orth = float(np.abs(v.T @ v - np.eye(a.shape[0])).max())
    return e_val, res, orth


@lru_cache(maxsize=None)
def restated_case(D, kind):
    """The matrix of (D, kind), the restatement's decomposition of it and its errors: computed once per process."""
    a = make_matrix(D, kind, 1000 + 7 * D + KINDS.index(kind))
    w, v, sweeps, ratio, done = jacobi_eigh(a)
    e_val, res, orth = eig_errors(a, w, v)
    fro = float(np.sqrt((a * a).sum()))
    return {"a": a, "w": w, "v": v, "sweeps": sweeps, "ratio": ratio, "done": done, "e_val": e_val, "res": res, "orth": orth,
            "fro": fro}
