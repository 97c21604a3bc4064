"""float64 numpy restatement of the ensemble scores (include/ffd.h ffd_ens_pointwise, ffd_ens_energy), written from
the definitions and sharing no code with the library.

X (S, m, D) ensemble, y (S, D) truth, w None or (1 | S, D) with entries 0 / 1 (0: an observed coordinate, excluded from
every score, per-point outputs 0).  With x_(1) <= ... <= x_(m) the sorted members of one point:

  crps   = (1/m) sum_i |x_i - y| - (1/Z) sum_i (2 i - m - 1) x_(i),   Z = m^2, or m (m - 1) with fair
  quant  = x_(floor(h)+1) + (h - floor(h)) (x_(floor(h)+2) - x_(floor(h)+1)),  h = (m - 1) p      (numpy's type 7)
  energy = (1/m) sum_i ||x_i - y||_w - (1/(2Z)) sum_ij ||x_i - x_j||_w

The quantile is interpolated in numpy's own rounding order (a + (b - a) g below g = 1/2, b - (b - a) (1 - g) from there
on -- the same real number), so that it equals np.quantile bit for bit.

``energy(..., dtype, form)`` evaluates the pair term as a Gram matrix in ``dtype``: d_ij^2 = n_i + n_j - 2 g_ij, clamped
at 0, diagonal 0, of the weighted rows either centred on the ensemble mean ("centred", the library's form) or as they are
("uncentred"); with dtype float32 every product, sum and square root of the score is fp32 arithmetic.  form=None is the
definition itself (differences), the float64 value every bound refers to."""
import numpy as np


def _weights(w, S, D):
    if w is None:
        return np.ones((S, D), dtype=bool)
    w = np.asarray(w)
    assert w.ndim == 2 and w.shape[1] == D and w.shape[0] in (1, S), w.shape
    return np.broadcast_to(w != 0, (S, D))


def z_norm(m, fair):
    if fair:
        assert m >= 2, "the fair estimator needs two members"
        return float(m) * float(m - 1)
    return float(m) * float(m)


def crps(X, y, w=None, fair=False):
    """(S, D) float64, 0 at the coordinates with weight 0."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    S, m, D = X.shape
    xs = np.sort(X, axis=1)
    i = np.arange(1, m + 1, dtype=np.float64)[None, :, None]
    out = np.abs(X - y[:, None, :]).sum(axis=1) / m - ((2.0 * i - m - 1.0) * xs).sum(axis=1) / z_norm(m, fair)
    return np.where(_weights(w, S, D), out, 0.0)


def crps_pairwise(X, y, w=None, fair=False):
    """The O(m^2) form: (1/m) sum_i |x_i - y| - (1/(2Z)) sum_ij |x_i - x_j|."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    S, m, D = X.shape
    pair = np.abs(X[:, :, None, :] - X[:, None, :, :]).sum(axis=(1, 2))
    out = np.abs(X - y[:, None, :]).sum(axis=1) / m - pair / (2.0 * z_norm(m, fair))
    return np.where(_weights(w, S, D), out, 0.0)


def crps_mean(X, y, w=None, fair=False):
    """(S,): the mean of crps over the coordinates with weight 1 (0 where there is none)."""
    S, _, D = np.shape(X)
    on = _weights(w, S, D)
    c = crps(X, y, w, fair)
    n = on.sum(axis=1)
    return np.where(n > 0, (c * on).sum(axis=1) / np.maximum(n, 1), 0.0)


def quantiles(X, levels, w=None):
    """(n_q, S, D) float64."""
    X = np.asarray(X, dtype=np.float64)
    S, m, D = X.shape
    xs = np.sort(X, axis=1)
    out = np.empty((len(levels), S, D))
    for q, p in enumerate(levels):
        assert 0.0 <= p <= 1.0
        h = (m - 1) * np.float64(p)
        lo = int(np.floor(h))
        g = h - np.floor(h)
        a, b = xs[:, min(lo, m - 1), :], xs[:, min(lo + 1, m - 1), :]
        diff = b - a
        out[q] = a + diff * g if g < 0.5 else b - diff * (1.0 - g)
        if g == 0.0:
            out[q] = a
    return np.where(_weights(w, S, D)[None], out, 0.0)


def ranks(X, y, w=None):
    """(below, equal): (S, D) int32 counts of members < y and == y."""
    X = np.asarray(X)
    y = np.asarray(y)
    S, m, D = X.shape
    on = _weights(w, S, D)
    below = (X < y[:, None, :]).sum(axis=1)
    equal = (X == y[:, None, :]).sum(axis=1)
    return np.where(on, below, 0).astype(np.int32), np.where(on, equal, 0).astype(np.int32)


def centred_rows(X, w=None):
    """float64 rows centred on the ensemble mean and weighted, and R (S,): the largest row norm of each series."""
    X = np.asarray(X, dtype=np.float64)
    S, m, D = X.shape
    Z = (X - X.mean(axis=1, keepdims=True)) * _weights(w, S, D)[:, None, :]
    return Z, np.sqrt((Z * Z).sum(axis=2)).max(axis=1)


def pair_term(X, w=None, dtype=np.float64, form=None):
    """(S,) sum_ij ||x_i - x_j||_w (both orders, the diagonal included as 0)."""
    S, m, D = np.shape(X)
    on = _weights(w, S, D)
    if form is None:
        X = np.asarray(X, dtype=np.float64)
        out = np.zeros(S)
        for s in range(S):
            V = X[s][:, on[s]]
            step = max(1, (1 << 22) // max(1, m * V.shape[1]))  # rows of differences held at once
            for i in range(0, m, step):
                out[s] += np.sqrt(((V[i:i + step, None, :] - V[None, :, :]) ** 2).sum(axis=2)).sum()
        return out
    assert form in ("centred", "uncentred"), form
    out = np.zeros(S, dtype=dtype)
    for s in range(S):
        V = np.asarray(X[s], dtype=dtype)
        if form == "centred":
            V = V - np.asarray(np.asarray(X[s], dtype=np.float64).mean(axis=0), dtype=dtype)[None, :]
        V = np.ascontiguousarray(V * on[s].astype(dtype)[None, :])
        n = (V * V).sum(axis=1, dtype=dtype)
        d2 = (n[:, None] + n[None, :]) - dtype(2.0) * (V @ V.T)
        d2 = np.maximum(d2, dtype(0.0))
        np.fill_diagonal(d2, dtype(0.0))
        out[s] = np.sqrt(d2).sum(dtype=dtype)
    return out


def truth_term(X, y, w=None, dtype=np.float64):
    """(S,) sum_i ||x_i - y||_w."""
    S, m, D = np.shape(X)
    on = _weights(w, S, D).astype(dtype)
    d = (np.asarray(X, dtype=dtype) - np.asarray(y, dtype=dtype)[:, None, :]) * on[:, None, :]
    return np.sqrt((d * d).sum(axis=2, dtype=dtype)).sum(axis=1, dtype=dtype)


def energy(X, y, w=None, fair=False, dtype=np.float64, form=None):
    """(S,) float64 energy score; (dtype, form) as in the module docstring."""
    m = np.shape(X)[1]
    t = truth_term(X, y, w, np.float64 if form is None else dtype)
    p = pair_term(X, w, dtype, form)
    if form is None:
        return t / m - p / (2.0 * z_norm(m, fair))
    return np.asarray(t / dtype(m) - p / dtype(2.0 * z_norm(m, fair)), dtype=np.float64)


def energy_bar(X, y, w=None, fair=False):
    """The bound of the energy score against float64, per series: max(2e-6 R, 3 e32) with R the largest centred weighted
    row norm and e32 the error of the fp32 centred evaluation of the same input.  Returns (bar, reference, e32)."""
    ref = energy(X, y, w, fair)
    e32 = np.abs(energy(X, y, w, fair, np.float32, "centred") - ref)
    _, R = centred_rows(X, w)
    return np.maximum(2e-6 * R, 3.0 * e32), ref, e32


# the tight ensemble far from the origin on which the uncentred Gram form of the pair term fails
TIGHT = dict(S=1, m=64, D=187, seed=7, spread=1e-2, offset=100.0)


def make_case(S, m, D, seed, spread=1.0, offset=0.0):
    """Seeded fp32 ensemble (S, m, D) and truth (S, D): member = offset + level_s,d + spread * N(0, 1)."""
    rng = np.random.default_rng(seed)
    level = rng.standard_normal((S, 1, D))
    X = (offset + level + spread * rng.standard_normal((S, m, D))).astype(np.float32)
    y = (offset + level[:, 0, :] + spread * rng.standard_normal((S, D))).astype(np.float32)
    return X, y
