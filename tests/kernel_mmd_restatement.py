"""Float64 numpy restatement of the kernel two-sample statistics (ffd_mmd_rowsums, ffd_mmd_bandwidth, ffd_mmd_scores,
ffd_mmd_gram, ffd_mmd_permute and ``KernelMMD``): squared distances in difference form, one ``exp`` per gamma and pair.
It shares no code with the library and never calls it.  Also the inputs of the tests, the fp32 centred-Gram restatement
the bar is taken from (centred on a vector, or not), and the permutation cases with the band their counts are judged by.

Conventions: X (n, D) the samples, Y (m, D) the originals; k_gamma(a, b) = exp(-gamma |a - b|^2); row sums are
(n_gamma, rows); the mean kernel is the mean over the gammas."""
import numpy as np

FAMILIES = ("gaussian", "clustered")
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
FLOOR = 2e-6
# (n, m, D, P, mean shift): P random assignments behind the observed one
PERM_CASES = [(96, 160, 5, 1000, 0.0), (256, 256, 24, 500, 0.0), (256, 256, 24, 500, 0.25), (200, 328, 187, 500, 0.0)]
PERM_SEED = 11
BAND_MAX = 4


def make_sets(na, nb, D, family, seed):
    """(A, B) fp32: the recipes of the nearest-neighbour tests (a standard normal, or 4 clusters 0.5 wide about 10)."""
    rng = np.random.default_rng(seed)
    if family == "gaussian":
        B = rng.standard_normal((nb, D))
        A = rng.standard_normal((na, D))
    else:
        c = 3 * rng.standard_normal((4, D)) + 10
        B = c[rng.integers(0, 4, nb)] + 0.5 * rng.standard_normal((nb, D))
        A = c[rng.integers(0, 4, na)] + 0.5 * rng.standard_normal((na, D))
    return A.astype(np.float32), B.astype(np.float32)


def perm_case(i):
    """(X, Y, P) of a numbered permutation case: Gaussian rows, the samples moved by the shift in every coordinate."""
    n, m, D, P, shift = PERM_CASES[i]
    rng = np.random.default_rng(7300 + i)
    Y = rng.standard_normal((m, D))
    X = rng.standard_normal((n, D)) + shift
    return X.astype(np.float32), Y.astype(np.float32), P


def dist2(A, B):
    """(na, nb) float64 squared distances in difference form, the sum over the coordinates in order."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((A.shape[0], B.shape[0]))
    for d in range(A.shape[1]):
        t = A[:, d:d + 1] - B[None, :, d]
        out += t * t
    return out


def row_sums(A, B, gammas, exclude_self=False):
    """(n_gamma, na) float64: sum_j exp(-gamma |a_i - b_j|^2), without the pair i == j under ``exclude_self``."""
    d = dist2(A, B)
    out = np.empty((len(gammas), d.shape[0]))
    for g, gamma in enumerate(gammas):
        k = np.exp(-float(gamma) * d)
        if exclude_self:
            assert d.shape[0] == d.shape[1]
            k[np.arange(d.shape[0]), np.arange(d.shape[0])] = 0.0
        out[g] = k.sum(axis=1)
    return out


def sigma2(Y):
    """2 n / (n - 1) mean_j |y_j - ybar|^2: the mean squared distance between two distinct rows, in closed form."""
    Y = np.asarray(Y, np.float64)
    n = Y.shape[0]
    return 2.0 * (n / (n - 1.0)) * float(((Y - Y.mean(axis=0)) ** 2).sum(axis=1).mean())


def sigma2_pairs(Y):
    """The same number from every explicit pair i != j."""
    d = dist2(Y, Y)
    n = d.shape[0]
    return float(d.sum()) / (n * (n - 1.0))


def ladder(s2, scales=SCALES):
    """gamma_s = 1 / (2 sigma^2 s)."""
    return [1.0 / (2.0 * s2 * float(s)) for s in scales]


def scores_from_rowsums(xx, xy, yy):
    """(unbiased (n_gamma + 1), biased (n_gamma + 1), witness (n)) from XX, XY (n_gamma, n) and YY (n_gamma, m); the last
    column is the mean kernel's."""
    xx, xy, yy = (np.asarray(a, np.float64) for a in (xx, xy, yy))
    n, m = xx.shape[1], yy.shape[1]
    xx = np.concatenate([xx, xx.mean(axis=0, keepdims=True)])
    xy = np.concatenate([xy, xy.mean(axis=0, keepdims=True)])
    yy = np.concatenate([yy, yy.mean(axis=0, keepdims=True)])
    sxx, sxy, syy = xx.sum(axis=1), xy.sum(axis=1), yy.sum(axis=1)
    unbiased = sxx / (n * (n - 1.0)) + syy / (m * (m - 1.0)) - 2.0 * sxy / (n * m)
    biased = (sxx + n) / (n * n) + (syy + m) / (m * m) - 2.0 * sxy / (n * m)
    return unbiased, biased, xx[-1] / (n - 1.0) - xy[-1] / m


def mmd_textbook(X, Y, gamma):
    """(unbiased, biased) MMD^2 as the textbook double sums over explicit pairs."""
    kxx, kxy, kyy = (np.exp(-gamma * dist2(a, b)) for a, b in ((X, X), (X, Y), (Y, Y)))
    n, m = kxx.shape[0], kyy.shape[0]
    unbiased = ((kxx.sum() - np.trace(kxx)) / (n * (n - 1.0)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1.0))
                - 2.0 * kxy.mean())
    return float(unbiased), float(kxx.mean() + kyy.mean() - 2.0 * kxy.mean())


def pipeline(X, Y, scales=SCALES):
    """The float64 ``KernelMMD`` numbers of samples X against originals Y: bandwidth from Y, the ladder, the scores."""
    g = ladder(sigma2(Y), scales)
    unbiased, biased, w = scores_from_rowsums(row_sums(X, X, g, True), row_sums(X, Y, g), row_sums(Y, Y, g, True))
    out = {"mmd2": float(unbiased[-1]), "mmd2_biased": float(biased[-1])}
    for s, v in zip(scales, unbiased):
        out[f"mmd2_s{float(s):g}"] = float(v)
    out["witness_max"] = float(w.max())
    out["witness_share_positive"] = float((w > 0).mean())
    return out, w


# ---- the permutation test ----
def gram(X, Y, gammas):
    """The pooled (x first) mean-kernel matrix, float64, diagonal 0."""
    Z = np.concatenate([np.asarray(X, np.float64), np.asarray(Y, np.float64)])
    d = dist2(Z, Z)
    K = np.mean([np.exp(-float(g) * d) for g in gammas], axis=0)
    K[np.arange(len(Z)), np.arange(len(Z))] = 0.0
    return K


def assignments(n, m, P, seed):
    """(P + 1, n + m) uint8 with n ones per row: row 0 the observed assignment, row p >= 1 the first n entries of the
    p-th permutation drawn from ``numpy.random.Generator(PCG64([seed, n, m]))``."""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(n), int(m)]))
    A = np.zeros((P + 1, n + m), np.uint8)
    A[0, :n] = 1
    for p in range(1, P + 1):
        A[p, rng.permutation(n + m)[:n]] = 1
    return A


def perm_stats(K, A, n, m):
    """T_p = a^T K a / (n (n - 1)) + b^T K b / (m (m - 1)) - 2 a^T K b / (n m), float64, b = 1 - a."""
    a = np.asarray(A, np.float64)
    b = 1.0 - a
    Ka, Kb = a @ K, b @ K
    return ((Ka * a).sum(axis=1) / (n * (n - 1.0)) + (Kb * b).sum(axis=1) / (m * (m - 1.0))
            - 2.0 * (Ka * b).sum(axis=1) / (n * m))


def count_ge(T, shift=0.0):
    """#{p >= 1 : T_p >= T_0 + shift}."""
    T = np.asarray(T, np.float64)
    return int((T[1:] >= T[0] + shift).sum())


def p_value(T):
    return (1.0 + count_ge(T)) / len(T)


# ---- the fp32 centred-Gram restatement the bar is taken from ----
def gram32_d2(A, B, centre=None):
    """fp32 (n_i + n_j) - 2 z_i . z_j clamped at 0, rows centred on ``centre`` (None: as they are)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    if centre is not None:
        c = np.asarray(centre, np.float32)
        A, B = A - c, B - c
    na = (A * A).sum(axis=1, dtype=np.float32)
    nb = (B * B).sum(axis=1, dtype=np.float32)
    return np.maximum((na[:, None] + nb[None, :]) - np.float32(2) * (A @ B.T), np.float32(0)).astype(np.float32)


def row_sums32(A, B, gammas, centre, exclude_self=False):
    """The straightforward fp32 form: fp32 Gram distances, one fp32 ``exp`` per gamma, the sum in float64."""
    d = gram32_d2(A, B, centre)
    out = np.empty((len(gammas), d.shape[0]))
    for g, gamma in enumerate(gammas):
        k = np.exp(np.float32(-gamma) * d).astype(np.float32)
        if exclude_self:
            k[np.arange(d.shape[0]), np.arange(d.shape[0])] = 0.0
        out[g] = k.sum(axis=1, dtype=np.float64)
    return out


def centre_of(B):
    """The column mean in float64, rounded to fp32: what the device centres on."""
    return np.asarray(B, np.float64).mean(axis=0).astype(np.float32)


def e_ref_rowmeans(A, B, gammas, centre, exclude_self=False):
    """The largest error of the fp32 restatement's row means (row sums over the column count) against float64."""
    return float(np.abs(row_sums32(A, B, gammas, centre, exclude_self) - row_sums(A, B, gammas, exclude_self)).max()) / B.shape[0]


def bar(e_ref):
    """max(2e-6, 3 e_ref): the project's standing form."""
    return max(FLOOR, 3.0 * e_ref)


def gram_mean32(X, Y, gammas, centre):
    """The pooled mean-kernel matrix from the fp32 restatement, as float64, diagonal 0."""
    Z = np.concatenate([np.asarray(X, np.float32), np.asarray(Y, np.float32)])
    d = gram32_d2(Z, Z, centre)
    K = np.mean([np.exp(np.float32(-g) * d).astype(np.float32).astype(np.float64) for g in gammas], axis=0)
    K[np.arange(len(Z)), np.arange(len(Z))] = 0.0
    return K


# ---- the ladder by repeated squaring: the epilogue that was NOT built ----
def row_sums32_squaring(A, B, gammas, centre):
    """The fp32 form a doubling ladder would allow: ``gammas`` ascending, each twice the one before; one fp32 ``exp`` at
    the smallest gamma (the widest kernel), every narrower kernel the square of the one before.  Sums in float64."""
    assert all(abs(b / a - 2.0) < 1e-12 for a, b in zip(gammas, gammas[1:]))
    d = gram32_d2(A, B, centre)
    k = np.exp(np.float32(-gammas[0]) * d).astype(np.float32)
    out = np.empty((len(gammas), d.shape[0]))
    for g in range(len(gammas)):
        out[g] = k.sum(axis=1, dtype=np.float64)
        k = (k * k).astype(np.float32)
    return out


# ---- the accepted limits: integer-valued rows, D = 1, so that float64's answer needs the 1021 distinct values only ----
LIMIT_ROWS = 1 << 24
LIMIT_D = 1 << 16
LIMIT_FEW = (3.0, 200.0, 501.0, 760.0, 1013.0)
LIMIT_POOLED, LIMIT_ASSIGNMENTS = 16384, 4096
DISTINCT = np.arange(1021, dtype=np.float32)[:, None]


def hashed_rows(n):
    """(n, 1) fp32 rows (j * 2654435761 mod 2^32) mod 1021: integers below 1021, every value many times over."""
    j = np.arange(n, dtype=np.uint64)
    return (((j * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) % np.uint64(1021)).astype(np.float32)[:, None]


def hashed_counts(rows):
    """How often each of the 1021 values occurs, float64."""
    return np.bincount(np.asarray(rows)[:, 0].astype(np.int64), minlength=1021).astype(np.float64)


def mean_kernel_of_values(gammas, centre=None):
    """(1021, 1021) mean kernel between the distinct values: float64 in difference form (centre None), or the fp32
    centred-Gram restatement as float64."""
    if centre is None:
        d = dist2(DISTINCT, DISTINCT)
        return np.mean([np.exp(-float(g) * d) for g in gammas], axis=0)
    d = gram32_d2(DISTINCT, DISTINCT, centre)
    return np.mean([np.exp(np.float32(-g) * d).astype(np.float32).astype(np.float64) for g in gammas], axis=0)


def perm_stats_of_values(F, values, A, n, m):
    """T_p for pooled rows that take the integer ``values`` (N,), from the kernel F between the distinct values and each
    assignment's counts per value; the pairs i == i (F's diagonal, once per row) are left out as the device leaves them."""
    onehot = np.zeros((len(values), 1021), np.float32)
    onehot[np.arange(len(values)), np.asarray(values).astype(np.int64)] = 1.0
    ca = (np.asarray(A, np.float32) @ onehot).astype(np.float64)  # counts <= 2^14: exact in fp32
    cb = onehot.sum(axis=0, dtype=np.float64)[None, :] - ca
    diag = np.diag(F)
    u = ((ca @ F) * ca).sum(axis=1) - ca @ diag
    w = ((cb @ F) * cb).sum(axis=1) - cb @ diag
    v = ((ca @ F) * cb).sum(axis=1)
    return u / (n * (n - 1.0)) + w / (m * (m - 1.0)) - 2.0 * v / (n * m)
