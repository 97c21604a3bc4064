"""Float64 numpy restatement of the entropic optimal-transport statistics (ffd_sinkhorn_softmin, ffd_sinkhorn,
ffd_sinkhorn_diameter2, ffd_host_sinkhorn_schedule and ``SinkhornDivergence``): squared distances in difference form, the
softmin as a log-sum-exp, the same Jacobi-ordered loop, schedule and extrapolation, and S.  It shares no code with the
library and never calls it.  Also the inputs of the tests, the fp32 centred-Gram twin the bar is taken from, the exact
assignment cost by brute force, and the large-epsilon limit.

Conventions: X (n, D) the samples, Y (m, D) the originals, uniform weights; C_ij = |x_i - y_j|^2;
softmin_eps(x | y, h)_i = -eps log((1 / m) sum_j exp((h_j - C_ij) / eps)); the potentials f, p live on X's rows and g, q on
Y's; S = mean (f - p) + mean (g - q)."""
import itertools

import numpy as np

FAMILIES = ("gaussian", "clustered")
FLOOR = 2e-6
RUN_COLUMNS = 1024  # ffd_sinkhorn.hip SK_RUN = 4 column tiles of 256


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


def dist2(A, B):
    """(na, nb) float64 squared distances in difference form, the sum over the coordinates in order."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((A.shape[0], B.shape[0]))
    for d in range(A.shape[1]):
        t = A[:, d:d + 1] - B[None, :, d]
        out += t * t
    return out


def centre_of(B):
    """The column mean in float64, rounded to fp32: what the device centres on."""
    return np.asarray(B, np.float64).mean(axis=0).astype(np.float32)


def sigma2(Y):
    """2 n / (n - 1) mean_j |y_j - ybar|^2: the mean squared distance between two distinct rows."""
    Y = np.asarray(Y, np.float64)
    n = Y.shape[0]
    return 2.0 * (n / (n - 1.0)) * float(((Y - Y.mean(axis=0)) ** 2).sum(axis=1).mean())


def diameter2(Y, centre):
    """4 max_j |y_j - centre|^2."""
    Z = np.asarray(Y, np.float64) - np.asarray(centre, np.float64)
    return 4.0 * float((Z * Z).sum(axis=1).max())


def schedule(diam2, eps, scaling=0.5, n_final=3):
    """diam2, diam2 scaling^2, ... while above eps, then n_final entries of eps."""
    out, e = [], float(diam2)
    while e > eps:
        out.append(e)
        e *= scaling * scaling
    return out + [float(eps)] * n_final


# ---- the softmin ----
def softmin_cost(C, h, eps, old=None):
    """The softmin from a cost matrix C (nq, nr), float64; the damped update with ``old``."""
    C, h = np.asarray(C, np.float64), np.asarray(h, np.float64)
    u = (h[None, :] - C) / float(eps)
    m = u.max(axis=1)
    out = -float(eps) * (m + np.log(np.exp(u - m[:, None]).sum(axis=1) / C.shape[1]))
    return out if old is None else 0.5 * (np.asarray(old, np.float64) + out)


def softmin(X, Y, h, eps, old=None):
    return softmin_cost(dist2(X, Y), h, eps, old)


def softmin_loops(X, Y, h, eps):
    """The definition written out: python loops over the pairs and coordinates, no maximum taken out."""
    out = []
    for x in np.asarray(X, np.float64):
        total = 0.0
        for y, hj in zip(np.asarray(Y, np.float64), h):
            total += float(np.exp((float(hj) - sum((float(a) - float(b)) ** 2 for a, b in zip(x, y))) / eps))
        out.append(-eps * float(np.log(total / len(Y))))
    return np.array(out)


# ---- the loop ----
def sinkhorn_costs(Cxy, Cxx, Cyy, eps_schedule, q=None, softmin_fn=softmin_cost):
    """The symmetric Jacobi-ordered loop from the three cost matrices: every pass updates all four potentials from the
    previous pass's values (the first pass undamped), then one undamped pass at the last eps.  ``q``: a supplied self
    potential of y.  A dict of S, ot_xy, change, f, g, p, q."""
    n, m = Cxy.shape
    Cyx = np.ascontiguousarray(Cxy.T)
    f, g, p = np.zeros(n), np.zeros(m), np.zeros(n)
    qq = np.zeros(m)
    change = 0.0
    for k, eps in enumerate(eps_schedule):
        damp = k > 0
        f1 = softmin_fn(Cxy, g, eps, f if damp else None)
        g1 = softmin_fn(Cyx, f, eps, g if damp else None)
        p1 = softmin_fn(Cxx, p, eps, p if damp else None)
        if q is None:
            qq = softmin_fn(Cyy, qq, eps, qq if damp else None)
        change = max(float(np.abs(f1 - f).max()), float(np.abs(g1 - g).max()))
        f, g, p = f1, g1, p1
    eps = eps_schedule[-1]
    fo, go, po = softmin_fn(Cxy, g, eps), softmin_fn(Cyx, f, eps), softmin_fn(Cxx, p, eps)
    qo = softmin_fn(Cyy, qq, eps) if q is None else np.asarray(q, np.float64).copy()
    return {"S": float((fo - po).mean() + (go - qo).mean()), "ot_xy": float(fo.mean() + go.mean()), "change": change,
            "f": fo, "g": go, "p": po, "q": qo}


def sinkhorn(X, Y, eps_schedule, q=None):
    return sinkhorn_costs(dist2(X, Y), dist2(X, X), dist2(Y, Y), eps_schedule, q)


def self_potential(Y, eps_schedule):
    """q alone: the y|y passes of the loop."""
    C = dist2(Y, Y)
    q = np.zeros(C.shape[0])
    for k, eps in enumerate(eps_schedule):
        q = softmin_cost(C, q, eps, q if k > 0 else None)
    return softmin_cost(C, q, eps_schedule[-1])


def pipeline(X, Y, blur=0.05, scaling=0.5, n_final=3):
    """The float64 ``SinkhornDivergence`` numbers of samples X against originals Y, and f - p per sample."""
    centre = centre_of(Y)
    eps = blur * blur * sigma2(Y)
    sched = schedule(diameter2(Y, centre), eps, scaling, n_final)
    r = sinkhorn(X, Y, sched)
    return {"sinkhorn_divergence": r["S"], "sinkhorn_distance": max(r["S"], 0.0) ** 0.5, "sinkhorn_ot": r["ot_xy"],
            "sinkhorn_change": r["change"], "sinkhorn_eps": eps}, r["f"] - r["p"]


# ---- the fp32 centred-Gram twin the bar is taken from ----
def gram32_d2(A, B, centre):
    """fp32 (n_i + n_j) - 2 z_i . z_j clamped at 0, rows centred on ``centre``."""
    c = np.asarray(centre, np.float32)
    A, B = np.asarray(A, np.float32) - c, np.asarray(B, np.float32) - c
    na = (A * A).sum(axis=1, dtype=np.float32)
    nb = (B * B).sum(axis=1, dtype=np.float32)
    return np.maximum((na[:, None] + nb[None, :]) - np.float32(2) * (A @ B.T), np.float32(0)).astype(np.float32)


def softmin_cost32(C32, h, eps, old=None):
    """The straightforward fp32 form from fp32 costs: h rounded to fp32, u = h - C and (u - max) log2(e) / eps in fp32, one
    fp32 ``exp2`` per pair, the sum, the logarithm and the damping in float64."""
    C32 = np.asarray(C32, np.float32)
    u = (np.asarray(h, np.float64).astype(np.float32)[None, :] - C32).astype(np.float32)
    m = u.max(axis=1)
    c = np.float32(1.4426950408889634 / float(eps))
    e = np.exp2(((u - m[:, None]).astype(np.float32) * c).astype(np.float32)).astype(np.float32)
    out = -m.astype(np.float64) - float(eps) * np.log(e.sum(axis=1, dtype=np.float64) / C32.shape[1])
    return out if old is None else 0.5 * (np.asarray(old, np.float64) + out)


def sinkhorn32(X, Y, centre, eps_schedule, q=None):
    """The loop on the fp32 twin."""
    return sinkhorn_costs(gram32_d2(X, Y, centre), gram32_d2(X, X, centre), gram32_d2(Y, Y, centre), eps_schedule, q,
                          softmin_fn=softmin_cost32)


def bar(e_ref, scale):
    """max(2e-6 scale, 3 e_ref): the project's standing form, on a quantity of the costs' magnitude."""
    return max(FLOOR * float(scale), 3.0 * float(e_ref))


# ---- what S is judged against where no restatement of the loop is needed ----
def assignment_cost(X, Y):
    """min over the permutations s of (1 / n) sum_i |x_i - y_s(i)|^2, by brute force: W_2^2 between two uniform sets of
    n = m <= 7 rows (Birkhoff: an optimal plan of equal uniform marginals is a permutation)."""
    C = dist2(X, Y)
    n = C.shape[0]
    assert C.shape == (n, n) and n <= 7
    rows = np.arange(n)
    return min(float(C[rows, list(s)].sum()) for s in itertools.permutations(range(n))) / n


def energy_limit(X, Y):
    """The limit of S as eps -> infinity: every entropic plan tends to the product coupling, so
    S -> mean C_xy - (mean C_xx + mean C_yy) / 2, which is half the energy distance 2 E C(x, y) - E C(x, x') - E C(y, y')
    of the kernel -C, and |mean x - mean y|^2 for the squared cost."""
    return float(dist2(X, Y).mean() - 0.5 * (dist2(X, X).mean() + dist2(Y, Y).mean()))
