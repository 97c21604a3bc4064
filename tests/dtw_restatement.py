"""Numpy restatement of the banded dynamic time warping of include/ffd.h (ffd_dtw_*), in float64 and in fp32, and the
float64 pipeline behind ``DTWMetrics``.  Shared by tests/test_dtw_host.py and tests/test_dtw_gpu.py.

For series a, b of (L, C) and a half-width w (clipped to L - 1):
    c(i, j) = sum_ch (a[i,ch] - b[j,ch])^2, ch in order;  D(0, 0) = c(0, 0);
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)) over |i - j| <= w;  dtw2 = D(L-1, L-1).
The recurrence runs over anti-diagonals d = i + j, vectorised over the pairs and over the band offset o = i - j: the
cells of diagonal d depend on diagonal d - 1 at o - 1 and o + 1 and on diagonal d - 2 at o, so L = 4096 costs 8191 steps.
The fp32 form uses fp32 for the differences, their squares, the channel sum and every add, in the order above.

The bar of every comparison with float64: max(REL * the case's largest float64 value, 3 * the largest
|fp32 restatement - float64| of the case)."""
import numpy as np

REL = 2e-6
# (n originals, m samples, L, C, w): the Gaussian cases of the scores; case c draws X then Y from default_rng(10 + c)
SCORE_CASES = ((48, 40, 24, 1, 3), (33, 65, 17, 2, 4), (64, 64, 48, 2, 5))
SCORE_KEYS = ("dtw_nn_distance_mean", "dtw_coverage_distance_mean", "dtw_warp_gain", "dtw_1nn_accuracy_samples",
              "dtw_1nn_accuracy_originals", "dtw_1nn_accuracy")


def dtw2(A, B, w, dtype=np.float64):
    """dtw2 of the paired rows of A and B (n, L, C) at half-width w, every operation in ``dtype``: (n,) of ``dtype``."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    assert A.ndim == 3 and A.shape == B.shape
    n, L, C = A.shape
    w = min(int(w), L - 1)
    assert w >= 0
    inf = dtype(np.inf)
    offsets = np.arange(-w, w + 1)
    prev1 = np.full((n, 2 * w + 3), inf, dtype=dtype)  # diagonal d - 1, column o + w + 1, one +inf column at each end
    prev2 = prev1.copy()
    for d in range(2 * L - 1):
        o = offsets[(offsets + d) % 2 == 0]
        i, j = (d + o) // 2, (d - o) // 2
        ok = (i >= 0) & (i < L) & (j >= 0) & (j < L)
        o, i, j = o[ok], i[ok], j[ok]
        cost = np.zeros((n, o.size), dtype=dtype)
        for ch in range(C):
            diff = A[:, i, ch] - B[:, j, ch]
            cost = cost + diff * diff
        col = o + w + 1
        if d == 0:
            best = np.zeros((n, 1), dtype=dtype)
        else:
            best = np.minimum(np.minimum(prev1[:, col - 1], prev1[:, col + 1]), prev2[:, col])
        new = np.full_like(prev1, inf)
        new[:, col] = cost + best
        assert new.dtype == dtype
        prev2, prev1 = prev1, new
    return prev1[:, w + 1].copy()


def all_pairs(Q, R, w, dtype=np.float64, rows_at_once=64):
    """dtw2 of every row of Q (nq, L, C) with every row of R (nr, L, C): (nq, nr) of ``dtype``."""
    Q, R = np.asarray(Q), np.asarray(R)
    out = np.empty((Q.shape[0], R.shape[0]), dtype=dtype)
    for i0 in range(0, Q.shape[0], rows_at_once):
        q = Q[i0:i0 + rows_at_once]
        a = np.repeat(q, R.shape[0], axis=0)
        b = np.tile(R, (q.shape[0], 1, 1))
        out[i0:i0 + q.shape[0]] = dtw2(a, b, w, dtype).reshape(q.shape[0], R.shape[0])
    return out


def bar(f64, f32):
    """The bar of a case from its float64 values and the fp32 restatement's."""
    f64, f32 = np.asarray(f64, np.float64), np.asarray(f32, np.float64)
    return max(REL * float(np.abs(f64).max()), 3.0 * float(np.abs(f32 - f64).max()))


def gaussian(n, L, C, seed):
    return np.random.default_rng(seed).standard_normal((n, L, C)).astype(np.float32)


def pulses(n, L, C, seed, jitter=2):
    """One bump per series on a constant background, its position jittered by up to ``jitter`` samples, its height and
    the background drawn per series, and a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64)[None, :, None]
    pos = L / 2.0 + rng.integers(-jitter, jitter + 1, size=(n, 1, 1))
    width = max(1.0, L / 12.0)
    height = 1.0 + rng.random((n, 1, C))
    ground = 0.2 * rng.standard_normal((n, 1, C))
    x = ground + height * np.exp(-0.5 * ((t - pos) / width) ** 2) + 0.02 * rng.standard_normal((n, L, C))
    return x.astype(np.float32)


FAMILIES = {"gaussian": gaussian, "pulses": pulses}


def shifted_pulse(L, C, shift, start=2):
    """(a, b) of (1, L, C): the same three-sample pulse on a constant background, b's ``shift`` samples later."""
    assert start >= 1 and start + 3 + shift <= L - 1
    a = np.full((1, L, C), 0.5, np.float32)
    b = a.copy()
    shape = np.array([1.0, 3.0, 2.0], np.float32)[:, None] + np.arange(C, dtype=np.float32)[None, :]
    a[0, start:start + 3] = shape
    b[0, start + shift:start + shift + 3] = shape
    return a, b


def integer_rows(n, L, C, seed):
    """Rows of small integers: every cost and every sum is an integer below 2^24, exact in fp32."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, L, C)).astype(np.float32)


def score_case(case):
    """(X samples (m, L, C), Y originals (n, L, C), w) of SCORE_CASES[case]."""
    n, m, L, C, w = SCORE_CASES[case]
    rng = np.random.default_rng(10 + case)
    X = rng.standard_normal((m, L, C)).astype(np.float32)
    Y = rng.standard_normal((n, L, C)).astype(np.float32)
    return X, Y, w


def nearest(D, exclude_self=False):
    """Per row of the pair matrix D the smallest value, the diagonal left out on request."""
    D = np.array(D, copy=True)
    if exclude_self:
        D[np.arange(D.shape[0]), np.arange(D.shape[0])] = np.inf
    return D.min(axis=1)


def searches(X, Y, w, dtype=np.float64):
    """The five k = 1 searches of the metric: squared distances xx (m), xy (m), yx (n), yy (n) at w and e2 (m) at 0."""
    xy = all_pairs(X, Y, w, dtype)
    return {"xx": nearest(all_pairs(X, X, w, dtype), True), "xy": xy.min(axis=1), "yx": xy.T.min(axis=1),
            "yy": nearest(all_pairs(Y, Y, w, dtype), True), "e2": all_pairs(X, Y, 0, dtype).min(axis=1)}


def scores_from_searches(s):
    """The six numbers, and the two counts behind the accuracies."""
    xx, xy, yx, yy, e2 = (np.asarray(s[key], np.float64) for key in ("xx", "xy", "yx", "yy", "e2"))
    moved = e2 > 0
    gain = 1.0 - float(np.sqrt(xy[moved] / e2[moved]).mean()) if moved.any() else 0.0
    count_x, count_y = int((xx < xy).sum()), int((yy < yx).sum())
    acc_x, acc_y = count_x / xx.size, count_y / yy.size
    values = (float(np.sqrt(xy).mean()), float(np.sqrt(yx).mean()), gain, acc_x, acc_y, 0.5 * (acc_x + acc_y))
    return dict(zip(SCORE_KEYS, values)), (count_x, count_y)


def pipeline(X, Y, w):
    """float64 ``DTWMetrics``: the keys, the counts and the searches."""
    s = searches(X, Y, w)
    found, counts = scores_from_searches(s)
    return found, counts, s
