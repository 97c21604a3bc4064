"""Float64 numpy restatement of the nearest-neighbour statistics (ffd_nn_search, ffd_nn_ball_count, ffd_nn_scores and
``ManifoldMetrics``): brute-force difference form, stable argsort by (value, index).  It shares no code with the
library.  Also the inputs of the tests, the scale and the bar they are judged by, and an fp32 Gram restatement (centred
on the reference mean, or not) that the bar is taken from.  For the sizes past one slab, chunk and column block
(tests/test_neighbours_sizes_gpu.py): ``SIZE_CASES``, the statistics on a subset of the query rows, radii with no
distance near them, and integer rows whose answers are exact."""
import numpy as np

# (nq, nr, D, k), numbered from 0: one row, the 64-row and 256-column tile edges on both sides, D below / at / above the
# 16-column padding, the ECG length, k up to 16
CASES = [(1, 5, 1, 1), (63, 65, 5, 3), (64, 64, 16, 5), (65, 257, 17, 5), (130, 300, 187, 5), (257, 129, 60, 8),
         (300, 300, 187, 3), (5, 1000, 8, 16)]
FAMILIES = ("gaussian", "clustered")
KEYS = ("precision", "recall", "density", "coverage", "authenticity", "nn_distance_mean", "nn_distance_min",
        "copy_share")


def make_case(case, family):
    """(Q, R, k) of a numbered case, fp32, the draws in the documented order."""
    return _draw(CASES[case], 4100 + case, family)


# (nq, nr, D, k), numbered from 0, the sizes the first set stops short of: a second 1024-row slab of the reference mean
# holding one row and 5 column tiles (a chunk of 8 under the default budget); the widest chunk (32 tiles) plus one
# column, k = 32 merged across the two; two column tiles per ball-count workgroup, the last chunk one tile of one column;
# several query blocks x several chunks under small budgets; D past one 256-column block of the mean; two flattened
# (L, C) layouts, one of odd D; the largest accepted D
SIZE_CASES = [(65, 1025, 17, 5), (130, 8193, 8, 32), (65, 16385, 8, 5), (300, 8193, 5, 3), (70, 130, 257, 5),
              (65, 257, 960, 5), (33, 65, 4745, 3), (3, 5, 65536, 2)]
SUBSAMPLE = 512  # rows of a reference set longer than 8193 that size_radius2 measures against


def _draw(shape, seed, family):
    nq, nr, D, k = shape
    rng = np.random.default_rng(seed)
    if family == "gaussian":
        R = rng.standard_normal((nr, D))
        Q = rng.standard_normal((nq, D))
    else:
        c = 3 * rng.standard_normal((4, D)) + 10
        R = c[rng.integers(0, 4, nr)] + 0.5 * rng.standard_normal((nr, D))
        Q = c[rng.integers(0, 4, nq)] + 0.5 * rng.standard_normal((nq, D))
    return Q.astype(np.float32), R.astype(np.float32), k


def make_size_case(i, family):
    """(Q, R, k) of a numbered size case: the recipes of ``make_case``, generator seed 5200 + i, the same draw order."""
    return _draw(SIZE_CASES[i], 5200 + i, family)


def dist2(Q, R):
    """(nq, nr) float64 squared distances in difference form, the sum over the coordinates in order."""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    out = np.zeros((Q.shape[0], R.shape[0]))
    for d in range(Q.shape[1]):
        t = Q[:, d:d + 1] - R[None, :, d]
        out += t * t
    return out


def knn(Q, R, k, exclude_self=False):
    """(sorted dist2 (nq, k), index (nq, k)): the k smallest by (value, then lower index)."""
    d = dist2(Q, R)
    if exclude_self:
        assert d.shape[0] == d.shape[1]
        d[np.arange(d.shape[0]), np.arange(d.shape[0])] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order.astype(np.int32)


def knn_rows(Q, R, k, rows, exclude_self=False):
    """``knn`` for the listed query rows only: (sorted dist2 (len(rows), k), index (len(rows), k)); under
    ``exclude_self`` the excluded column is the row's index in Q."""
    rows = np.asarray(rows, np.int64)
    d = dist2(np.asarray(Q)[rows], R)
    if exclude_self:
        d[np.arange(len(rows)), rows] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order.astype(np.int32)


def scale(Q, R):
    """The largest squared norm of any row of either set after subtracting the reference set's float64 column mean."""
    mean = np.asarray(R, np.float64).mean(axis=0)
    return max(float(((np.asarray(A, np.float64) - mean) ** 2).sum(axis=1).max()) for A in (Q, R))


def gram32(Q, R, centred=True):
    """The fp32 Gram form n_i + n_j - 2 z_i . z_j, clamped at 0; centred on the reference set's mean (computed in
    float64, rounded to fp32) or on nothing."""
    Q, R = np.asarray(Q, np.float32), np.asarray(R, np.float32)
    if centred:
        mean = R.astype(np.float64).mean(axis=0).astype(np.float32)
        Q, R = Q - mean, R - mean
    nq = (Q * Q).sum(axis=1, dtype=np.float32)
    nr = (R * R).sum(axis=1, dtype=np.float32)
    g = Q @ R.T
    return np.maximum((nq[:, None] + nr[None, :]) - np.float32(2) * g, np.float32(0)).astype(np.float32)


def e_ref(Q, R, centred=True):
    """The largest error of the fp32 Gram restatement against float64, relative to the scale."""
    return float(np.abs(gram32(Q, R, centred).astype(np.float64) - dist2(Q, R)).max()) / scale(Q, R)


def bar(Q, R):
    """max(2e-6, 3 e_ref): the project's standing form (2e-6 is the w2 projection's)."""
    return max(2e-6, 3.0 * e_ref(Q, R))


def self_radius2(R, k):
    """The reference set's own k-th self-neighbour squared distance per row (min(k, nr - 1)-th where needed), as fp32."""
    kk = min(k, R.shape[0] - 1)
    return knn(R, R, kk, exclude_self=True)[0][:, kk - 1].astype(np.float32)


def _pair_block(Q, R, exclude_self, rows):
    """d2 of the listed query rows (all of them for None) against R, the pair i == i at infinity under exclude_self."""
    rows = np.arange(np.asarray(Q).shape[0]) if rows is None else np.asarray(rows, np.int64)
    d = dist2(np.asarray(Q)[rows], R)
    if exclude_self:
        d[np.arange(len(rows)), rows] = np.inf
    return d


def ball_counts(Q, R, radius2, exclude_self=False, shift=0.0, rows=None):
    """count[i] = #{ j : d2(i, j) <= radius2[j] + shift } in float64, for the listed query rows (all for None)."""
    d = _pair_block(Q, R, exclude_self, rows)
    return (d <= np.asarray(radius2, np.float64)[None, :] + shift).sum(axis=1).astype(np.int32)


def size_radius2(R, k):
    """The ball radii of the size cases, fp32.  Up to 8193 rows: ``self_radius2`` (the values only, so a partition of
    256 rows at a time stands for the sort).  Beyond: the k-th distance to a fixed subsample of SUBSAMPLE rows (a row of
    the subsample leaves itself out), times (SUBSAMPLE / nr)^(2 / D), the ratio of the two densities' ball radii -- a
    float64 self-search of all rows would cost more than every other restatement of the suite together."""
    R = np.asarray(R)
    nr, D = R.shape
    kk = min(k, nr - 1)
    if nr <= 8193:
        out = np.empty(nr)
        for a in range(0, nr, 256):
            d = _pair_block(R, R, True, np.arange(a, min(a + 256, nr)))
            out[a:a + 256] = np.partition(d, kk - 1, axis=1)[:, kk - 1]
        return out.astype(np.float32)
    pick = np.arange(SUBSAMPLE) * (nr // SUBSAMPLE)
    d = dist2(R, R[pick])
    d[pick, np.arange(SUBSAMPLE)] = np.inf
    return (np.partition(d, kk - 1, axis=1)[:, kk - 1] * (SUBSAMPLE / nr) ** (2.0 / D)).astype(np.float32)


def gapped_radii(Q, R, radius2, bar, scale, exclude_self=False, rows=None):
    """(radii, how many moved): every radius2[j] moved up by fp32 steps of 4 bar scale until no d2(i, j), i over the
    listed rows of Q (all for None), lies within 2 bar scale of it.  With such radii float64's counts at -+ bar scale
    coincide for every listed row, so a ball count within that band is float64's own count."""
    d = _pair_block(Q, R, exclude_self, rows)
    rad = np.array(radius2, np.float32)
    half, step = 2.0 * bar * scale, np.float32(4.0 * bar * scale)
    assert step > 0 and (rad + step > rad).all()  # a step an fp32 radius of this size can take
    cols = np.arange(len(rad))
    moved = np.zeros(len(rad), bool)
    while len(cols):
        near = (np.abs(d[:, cols] - rad[cols].astype(np.float64)[None, :]) <= half).any(axis=0)
        cols = cols[near]
        rad[cols] += step
        moved[cols] = True
    return rad, int(moved.sum())


# ---- the accepted limits: integer-valued rows, D = 1, every squared distance an integer ----
LIMIT_ROWS = 1 << 24
LIMIT_REFERENCE = (3.0, 200.0, 501.0, 760.0, 1013.0)  # adjacent values sum to an odd number: no integer is equidistant
LIMIT_QUERIES = (0.0, 510.0, 1020.0)
LIMIT_OFFSET = float(1 << 23)  # fp32 still holds the integers offset by it; their squares it does not


def hashed_rows(n):
    """(n, 1) fp32 rows (j * 2654435761 mod 2^32) mod 1021: integers below 1021, every value many times over."""
    j = np.arange(n, dtype=np.uint64)
    return (((j * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) % np.uint64(1021)).astype(np.float32)[:, None]


def scores_from_arrays(self_y, xy_d2, xy_idx, yx_d2, count_x, count_y, k):
    """The eight numbers from the six arrays ffd_nn_scores reads, in float64."""
    self_y = np.asarray(self_y, np.float64)
    n, m = self_y.shape[0], len(xy_d2)
    xy_d2, yx_d2 = np.asarray(xy_d2, np.float64).reshape(m), np.asarray(yx_d2, np.float64).reshape(n)
    xy_idx = np.asarray(xy_idx).reshape(m)
    count_x, count_y = np.asarray(count_x).reshape(m), np.asarray(count_y).reshape(n)
    nn = np.sqrt(xy_d2)
    return dict(precision=float((count_x > 0).sum()) / m, recall=float((count_y > 0).sum()) / n,
                density=float(count_x.astype(np.float64).sum()) / (k * m),
                coverage=float((yx_d2 <= self_y[:, k - 1]).sum()) / n,
                authenticity=float((xy_d2 > self_y[xy_idx, 0]).sum()) / m,
                nn_distance_mean=float(nn.sum()) / m, nn_distance_min=float(nn.min()),
                copy_share=float((xy_d2 == 0.0).sum()) / m)


def scores(Y, X, k, shift=0.0):
    """The float64 pipeline: originals Y (n, D), samples X (m, D).  The ball radii are the fp32-rounded k-th
    self-neighbour distances, as the device takes them; ``shift`` is added to every radius of a ball count and to the
    coverage radius (the band of the tests)."""
    self_y, _ = knn(Y, Y, k, exclude_self=True)
    self_x, _ = knn(X, X, k, exclude_self=True)
    xy_d2, xy_idx = knn(X, Y, 1)
    yx_d2, _ = knn(Y, X, 1)
    count_x = ball_counts(X, Y, self_y[:, k - 1].astype(np.float32), shift=shift)
    count_y = ball_counts(Y, X, self_x[:, k - 1].astype(np.float32), shift=shift)
    shifted = self_y.copy()
    shifted[:, k - 1] += shift
    out = scores_from_arrays(shifted, xy_d2[:, 0], xy_idx[:, 0], yx_d2[:, 0], count_x, count_y, k)
    out["authenticity"] = float((xy_d2[:, 0] > self_y[xy_idx[:, 0], 0]).sum()) / X.shape[0]
    return out
