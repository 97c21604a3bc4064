"""GPU tests of the kernel two-sample statistics (ffd_mmd.hip, ``utils.kernel_mmd``, ``KernelMMD``) against the float64
restatement (tests/kernel_mmd_restatement.py).

Bars: a quantity on the kernel's scale -- a row sum over its column count, an MMD^2, a witness value, a permutation
statistic -- within max(2e-6, 3 e_ref) of float64, e_ref the error of the fp32 centred-Gram restatement on the same
input; ``ffd_mmd_scores`` and ``ffd_mmd_bandwidth`` are fp64 throughout: 1e-12 relative.  Every test prints its measured
maximum before it asserts.  There is ONE epilogue path (an exponential per gamma and pair, a doubling ladder is not
special-cased), so n_gamma gammas at once must give the bits of n_gamma calls."""
import numpy as np
import pytest
import torch

import kernel_mmd_restatement as KR

pytestmark = pytest.mark.gpu

RUN_COLUMNS = 1024  # ffd_mmd.hip MMD_RUN = 4 column tiles of 256
LADDER = (0.25, 0.5, 1.0, 2.0, 4.0)
EIGHT = (0.1, 0.3, 0.7, 1.0, 1.9, 3.3, 6.1, 11.0)  # no ratio a power of two


@pytest.fixture(scope="module")
def KM():
    from fastfourierdiffusion_amd.utils import kernel_mmd

    return kernel_mmd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gamma_sets(Y):
    s2 = KR.sigma2(Y) if Y.shape[0] > 1 else 2.0 * Y.shape[1]
    return [KR.ladder(s2, (1.0,)), KR.ladder(s2, LADDER), KR.ladder(s2, EIGHT)]


def _check_rowsums(KM, A, B, label, exclude_self=False):
    """Device row sums of every gamma set against float64, over the column count; returns the largest error."""
    centre = KR.centre_of(B)
    a = _dev(A)
    b = a if exclude_self else _dev(B)
    worst = 0.0
    for gammas in _gamma_sets(B):
        got = KM.row_sums(a, b, _dev(centre), gammas, exclude_self=exclude_self).cpu().numpy()
        want = KR.row_sums(A, B, gammas, exclude_self)
        bar = KR.bar(KR.e_ref_rowmeans(A, B, gammas, centre, exclude_self))
        err = float(np.abs(got - want).max()) / B.shape[0]
        print(f"{label} n_gamma {len(gammas)}: row-mean error {err:.3e}, bar {bar:.1e}")
        assert got.shape == want.shape and err <= bar, (label, len(gammas), err, bar)
        worst = max(worst, err)
    return worst


# ------------------------------------------------------------------ row sums ----
@pytest.mark.parametrize("family", KR.FAMILIES)
@pytest.mark.parametrize("na,nb,D", [(1, 2, 3), (2, 2, 5), (130, 513, 7), (3, RUN_COLUMNS + 1, 4), (5, 2 * RUN_COLUMNS + 257, 2)])
def test_row_sums_small_and_run_edges(KM, family, na, nb, D):
    A, B = KR.make_sets(na, nb, D, family, 3000 + na + nb)
    _check_rowsums(KM, A, B, f"{family} {na}x{nb}x{D}")


@pytest.mark.parametrize("D", [1, 15, 16, 17, 187])
@pytest.mark.parametrize("na", [63, 64, 65])
def test_row_sums_at_the_tile_edges(KM, na, D):
    for nb in (255, 256, 257):
        for family in KR.FAMILIES:
            A, B = KR.make_sets(na, nb, D, family, 3100 + na + nb + D)
            _check_rowsums(KM, A, B, f"{family} {na}x{nb}x{D}")


@pytest.mark.parametrize("family", KR.FAMILIES)
@pytest.mark.parametrize("n,D", [(2, 3), (65, 16), (257, 187), (RUN_COLUMNS + 1, 5)])
def test_row_sums_exclude_self(KM, family, n, D):
    _, B = KR.make_sets(1, n, D, family, 3200 + n)
    _check_rowsums(KM, B, B, f"{family} self {n}x{D}", exclude_self=True)


def test_exact_and_degenerate_cases(KM):
    _, B = KR.make_sets(1, 300, 6, "gaussian", 3300)
    A, _ = KR.make_sets(70, 1, 6, "gaussian", 3301)
    a, b, c = _dev(A), _dev(B), _dev(KR.centre_of(B))
    # gamma = 0: a row sum is exactly the column count, with and without the diagonal
    assert (KM.row_sums(a, b, c, [0.0, 0.0]).cpu().numpy() == 300.0).all()
    assert (KM.row_sums(b, b, c, [0.0], exclude_self=True).cpu().numpy() == 299.0).all()
    # every off-diagonal value underflows: exactly 0 with exclude_self (the Gram form's d2(i, i) is not exactly 0, so the
    # diagonal is never formed)
    assert float(KR.dist2(B, B)[~np.eye(300, dtype=bool)].min()) > 1e-3
    assert (KM.row_sums(b, b, c, [1e9, 1e12], exclude_self=True).cpu().numpy() == 0.0).all()
    # the library overwrites every element of its outputs (the binding hands it fresh memory: call it directly)
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    out = torch.full((3, 70), float("nan"), device="cuda", dtype=torch.float64)
    g = np.array(KR.ladder(12.0, (0.5, 1, 2)))
    nbytes = lib.ffd_mmd_rowsums_work_bytes(70, 300, 6, 3)
    work = torch.full(((nbytes + 7) // 8,), float("nan"), device="cuda", dtype=torch.float64)
    N.check(lib.ffd_mmd_rowsums(a.data_ptr(), 70, b.data_ptr(), 300, 6, c.data_ptr(), g.ctypes.data, 3, 0, out.data_ptr(),
                                work.data_ptr(), nbytes, N.current_stream_ptr(a.device)), None, "ffd_mmd_rowsums")
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - KR.row_sums(A, B, g)).max() / 300 <= KR.FLOOR
    assert torch.equal(out, KM.row_sums(a, b, c, g))


@pytest.mark.parametrize("family", KR.FAMILIES)
def test_bit_identity(KM, family):
    A, B = KR.make_sets(200, 2 * RUN_COLUMNS + 300, 17, family, 3400)
    a, b, c = _dev(A), _dev(B), _dev(KR.centre_of(B))
    gammas = KR.ladder(KR.sigma2(B), LADDER)
    whole = KM.row_sums(a, b, c, gammas)
    assert torch.equal(whole, KM.row_sums(a, b, c, gammas))  # two runs
    for cut in (64, 77, 199):  # a query set cut in two, at and off a tile edge
        parts = torch.cat([KM.row_sums(a[:cut].contiguous(), b, c, gammas), KM.row_sums(a[cut:].contiguous(), b, c, gammas)], dim=1)
        assert torch.equal(whole, parts), cut
    more = torch.cat([a, _dev(KR.make_sets(150, 1, 17, family, 3401)[0])])  # a set with rows appended
    assert torch.equal(whole, KM.row_sums(more, b, c, gammas)[:, :200])
    shifted = torch.cat([more[200:], a])  # ... and put in front: other rows around it, another place in its tile
    assert torch.equal(whole, KM.row_sums(shifted, b, c, gammas)[:, 150:])
    # one epilogue path: the five-gamma call is five one-gamma calls, bit for bit; so is the eight-gamma one
    for gs in (gammas, KR.ladder(KR.sigma2(B), EIGHT)):
        ones = torch.cat([KM.row_sums(a, b, c, [g]) for g in gs])
        assert torch.equal(KM.row_sums(a, b, c, gs), ones)
    self_whole = KM.row_sums(b, b, c, gammas, exclude_self=True)
    assert torch.equal(self_whole, KM.row_sums(b, b, c, gammas, exclude_self=True))
    strided = _dev(np.ascontiguousarray(B.T)).T  # one non-contiguous tensor as both sets: copied once, still one buffer
    assert not strided.is_contiguous() and torch.equal(self_whole, KM.row_sums(strided, strided, c, gammas, exclude_self=True))


# ------------------------------------------------------------------ bandwidth, scores ----
@pytest.mark.parametrize("n", [2, 1023, 1024, 1025])
def test_bandwidth(KM, n):
    for family, D in (("gaussian", 5), ("clustered", 187)):
        _, Y = KR.make_sets(1, n, D, family, 3500 + n)
        got = float(KM.bandwidth(_dev(Y)).item())
        want = KR.sigma2(Y)
        print(f"sigma^2 {family} n = {n}: relative error {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-12 * want
        centre = KM.column_mean(_dev(Y)).cpu().numpy().astype(np.float64)
        mean = Y.astype(np.float64).mean(axis=0)  # the fp64 mean rounded once to fp32: half an ulp of the largest entry
        assert centre.shape == (D,) and np.abs(centre - mean).max() <= 2.0 ** -24 * max(1.0, float(np.abs(mean).max())) * 1.001


@pytest.mark.parametrize("n,m,ng", [(2, 2, 1), (257, 300, 5), (1000, 513, 8)])
def test_scores_on_the_device_s_own_row_sums(KM, n, m, ng):
    X, Y = KR.make_sets(n, m, 9, "clustered", 3600 + n)
    x, y, c = _dev(X), _dev(Y), _dev(KR.centre_of(Y))
    gammas = KR.ladder(KR.sigma2(Y), EIGHT[:ng])
    xx, xy, yy = KM.row_sums(x, x, c, gammas, True), KM.row_sums(x, y, c, gammas), KM.row_sums(y, y, c, gammas, True)
    mmd2, witness = KM.mmd_scores(xx, xy, yy)
    u, b, w = KR.scores_from_rowsums(xx.cpu().numpy(), xy.cpu().numpy(), yy.cpu().numpy())
    got = mmd2.cpu().numpy()
    # 1e-12 relative to the largest of the terms that cancel in each number (a difference near 0 has no scale of its own)
    hx, hy = xx.cpu().numpy(), yy.cpu().numpy()
    terms = np.maximum(hx.sum(axis=1) / (n * (n - 1.0)), np.maximum(hy.sum(axis=1) / (m * (m - 1.0)),
                                                                    2.0 * xy.cpu().numpy().sum(axis=1) / (n * m)))
    terms = np.append(terms, terms.mean())
    wterms = np.maximum(hx.mean(axis=0) / (n - 1.0), xy.cpu().numpy().mean(axis=0) / m)
    err = max(float((np.abs(got[0] - u) / terms).max()), float((np.abs(got[1] - b) / terms).max()),
              float((np.abs(witness.cpu().numpy() - w) / wterms).max()))
    print(f"scores {n} x {m}, {ng} gammas: largest error relative to the terms {err:.2e}")
    assert got.shape == (2, ng + 1) and err <= 1e-12
    # and against the float64 pipeline, on the kernel's scale
    fu, fb, fw = KR.scores_from_rowsums(KR.row_sums(X, X, gammas, True), KR.row_sums(X, Y, gammas), KR.row_sums(Y, Y, gammas, True))
    err = max(float(np.abs(got[0] - fu).max()), float(np.abs(got[1] - fb).max()), float(np.abs(witness.cpu().numpy() - fw).max()))
    print(f"  against float64 rows: {err:.2e}")
    assert err <= KR.FLOOR and (got[1] >= -KR.FLOOR).all()


# ------------------------------------------------------------------ the permutation test ----
@pytest.mark.parametrize("case", range(len(KR.PERM_CASES)))
def test_permutation_statistics(KM, case):
    X, Y, P = KR.perm_case(case)
    n, m = X.shape[0], Y.shape[0]
    gammas = KR.ladder(KR.sigma2(Y))
    A = KM.permutation_assignments(n, m, P, KR.PERM_SEED)
    assert np.array_equal(A, KR.assignments(n, m, P, KR.PERM_SEED))
    centre = KR.centre_of(Y)
    got = KM.permutation_test(_dev(X), _dev(Y), _dev(centre), gammas, A).cpu().numpy()
    want = KR.perm_stats(KR.gram(X, Y, gammas), A, n, m)
    bar = KR.bar(float(np.abs(KR.perm_stats(KR.gram_mean32(X, Y, gammas, centre), A, n, m) - want).max()))
    err = float(np.abs(got - want).max())
    count, lo, hi = KR.count_ge(got), KR.count_ge(want, bar), KR.count_ge(want, -bar)
    print(f"case {case}: largest |T_p - float64| {err:.3e}, bar {bar:.1e}; count {count} in [{lo}, {hi}], p {KM.p_value(got):.4f}")
    assert got.shape == (P + 1,) and err <= bar
    assert lo <= count <= hi and hi - lo <= KR.BAND_MAX
    if KR.PERM_CASES[case][4] > 0:
        assert KM.p_value(got) == 1.0 / (P + 1)
    # assignment 0 is the unbiased estimate the row sums give
    x, y, c = _dev(X), _dev(Y), _dev(centre)
    mmd2, _ = KM.mmd_scores(KM.row_sums(x, x, c, gammas, True), KM.row_sums(x, y, c, gammas), KM.row_sums(y, y, c, gammas, True))
    assert abs(float(mmd2[0, -1]) - got[0]) <= KR.FLOOR
    assert np.array_equal(got, KM.permutation_test(x, y, c, gammas, torch.from_numpy(A).cuda()).cpu().numpy())  # two runs


# ------------------------------------------------------------------ end to end ----
def test_kernel_mmd_metric_and_collection_against_float64():
    from functools import partial

    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y = KR.make_sets(300, 420, 24, "clustered", 3700)
    metric = M.KernelMMD(Y, permutations=200, random_seed=5)
    got = metric(X)
    want, w = KR.pipeline(X, Y)
    for key, value in want.items():
        print(f"{key}: device {got[key]:.6e}, float64 {value:.6e}")
        if key == "witness_share_positive":  # a count: between float64's shares of w > +bar and w > -bar
            assert float((w > KR.FLOOR).mean()) <= got[key] <= float((w > -KR.FLOOR).mean())
        else:
            assert abs(got[key] - value) <= KR.FLOOR, key
    T = KR.perm_stats(KR.gram(X, Y, KR.ladder(KR.sigma2(Y))), KR.assignments(300, 420, 200, 5), 300, 420)
    assert (1.0 + KR.count_ge(T, KR.FLOOR)) / 201 <= got["p_value"] <= (1.0 + KR.count_ge(T, -KR.FLOOR)) / 201
    assert metric(X) == got  # cached originals: the same bits
    base = metric.baseline_metrics
    half = Y.shape[0] // 2
    g = KR.ladder(KR.sigma2(Y))
    u, _, _ = KR.scores_from_rowsums(KR.row_sums(Y[half:], Y[half:], g, True), KR.row_sums(Y[half:], Y[:half], g),
                                     KR.row_sums(Y[:half], Y[:half], g, True))
    assert abs(base["mmd2_self"] - u[-1]) <= KR.FLOOR and 0.0 < base["p_value_self"] <= 1.0
    assert np.abs(metric.witness(X).cpu().numpy() - w).max() <= KR.FLOOR
    # composition: a MetricCollection holding it, on three-dimensional samples
    Y3 = np.random.default_rng(3701).standard_normal((120, 16, 2)).astype(np.float32)
    X3 = np.random.default_rng(3702).standard_normal((90, 16, 2)).astype(np.float32)
    coll = M.MetricCollection([partial(M.KernelMMD, scales=(0.5, 1, 2))], original_samples=torch.from_numpy(Y3))
    found = coll(torch.from_numpy(X3))
    ref, _ = KR.pipeline(X3.reshape(90, -1), Y3.reshape(120, -1), (0.5, 1, 2))
    assert "freq_mmd2" in found and "time_mmd2_self" in found and "time_mmd2_s0.5" in found
    for key, value in ref.items():
        if key != "witness_share_positive":
            assert abs(found[f"time_{key}"] - value) <= KR.FLOOR, key


def test_witness_ranks_a_planted_off_manifold_tenth_above_the_rest():
    from fastfourierdiffusion_amd.sampling.metrics import KernelMMD

    rng = np.random.default_rng(3800)
    Y = rng.standard_normal((600, 12)).astype(np.float32)
    X = rng.standard_normal((400, 12)).astype(np.float32)
    planted = np.arange(0, 400, 10)
    X[planted] = (3.0 + 0.3 * rng.standard_normal((40, 12))).astype(np.float32)  # a clump where the data has no mass
    w = KernelMMD(Y).witness(X).cpu().numpy()
    rest = np.setdiff1d(np.arange(400), planted)
    print(f"witness: planted min {w[planted].min():.4f}, rest max {w[rest].max():.4f}")
    assert w[planted].min() > w[rest].max()
    assert set(np.argsort(-w)[:40].tolist()) == set(planted.tolist())
    assert np.abs(w - KR.pipeline(X, Y)[1]).max() <= KR.FLOOR


# ------------------------------------------------------------------ refusals on the device ----
def test_refusals_on_the_device(KM):
    from fastfourierdiffusion_amd import _native as N

    X, Y = KR.make_sets(20, 30, 4, "gaussian", 3900)
    x, y, c = _dev(X), _dev(Y), _dev(KR.centre_of(Y))
    with pytest.raises(AssertionError):
        KM.row_sums(x, y, c, [1.0], exclude_self=True)
    with pytest.raises(AssertionError):
        KM.row_sums(x.double(), y, c, [1.0])
    with pytest.raises(N.FFDError):
        KM.row_sums(x.cpu(), y, c, [1.0])
    with pytest.raises(AssertionError):
        KM.bandwidth(y[:1])
    lib = N.lib()
    out = torch.full((1, 20), -7.0, device="cuda", dtype=torch.float64)
    g = np.array([1.0])
    nbytes = lib.ffd_mmd_rowsums_work_bytes(20, 30, 4, 1)
    work = torch.empty(nbytes // 8 + 2, device="cuda", dtype=torch.float64)
    stream = N.current_stream_ptr(x.device)

    def call(a=x, na=20, excl=0, w=work.data_ptr(), nb=nbytes, gam=g):
        return lib.ffd_mmd_rowsums(a.data_ptr(), na, y.data_ptr(), 30, 4, c.data_ptr(), gam.ctypes.data, len(gam), excl,
                                   out.data_ptr(), w, nb, stream)

    assert call(excl=1) == -1 and call(w=work.data_ptr() + 8) == -1 and call(nb=nbytes - 16) == -1
    assert call(gam=np.array([-1.0])) == -1 and call(na=(1 << 24) + 1) == -2
    assert lib.ffd_mmd_permute(work.data_ptr(), 8192, 8193, y.data_ptr(), 3, out.data_ptr(), work.data_ptr(), nbytes, stream) == -2
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert call() == 0 and (out != -7.0).all()
    with pytest.raises(ValueError, match="16384"):
        KM.permutation_test(torch.zeros(16383, 1, device="cuda"), torch.zeros(2, 1, device="cuda"), c[:1], [1.0],
                            np.zeros((1, 16385), np.uint8))


# ------------------------------------------------------------------ the accepted limits ----
# Rows of one integer below 1021 (D = 1), few rows on the other side: float64's answer needs the 1021 distinct values only.
def test_longest_query_set(KM):
    """na = 2^24 against 5 rows: 262 144 row blocks, the (gamma, row) index of the partial sums and the fold up to 2^25."""
    A, B = KR.hashed_rows(KR.LIMIT_ROWS), np.array(KR.LIMIT_FEW, np.float32)[:, None]
    centre = KR.centre_of(B)
    gammas = KR.ladder(KR.sigma2(KR.DISTINCT), (1.0, 0.25))
    got = KM.row_sums(_dev(A), _dev(B), _dev(centre), gammas).cpu().numpy()
    by_value = KR.row_sums(KR.DISTINCT, B, gammas)
    bar = KR.bar(float(np.abs(KR.row_sums32(KR.DISTINCT, B, gammas, centre) - by_value).max()) / 5)
    err = float(np.abs(got - by_value[:, A[:, 0].astype(np.int64)]).max()) / 5
    print(f"2^24 x 5: row-mean error {err:.3e}, bar {bar:.1e}")
    assert got.shape == (2, KR.LIMIT_ROWS) and err <= bar


def test_longest_reference_set(KM):
    """3 rows against nb = 2^24: 16 384 slabs of the mean, 16 384 column runs folded in order."""
    A, B = np.array([[0.0], [510.0], [1020.0]], np.float32), KR.hashed_rows(KR.LIMIT_ROWS)
    centre = KR.centre_of(B)
    gammas = KR.ladder(KR.sigma2(KR.DISTINCT), (1.0, 0.25))
    b = _dev(B)
    assert np.abs(KM.column_mean(b).cpu().numpy().astype(np.float64) - B.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -15
    got = KM.row_sums(_dev(A), b, _dev(centre), gammas).cpu().numpy()
    counts = KR.hashed_counts(B)
    want = np.stack([(np.exp(-g * KR.dist2(A, KR.DISTINCT)) * counts).sum(axis=1) for g in gammas])
    d32 = KR.gram32_d2(A, KR.DISTINCT, centre)
    ref32 = np.stack([(np.exp(np.float32(-g) * d32).astype(np.float32) * counts).sum(axis=1) for g in gammas])
    bar = KR.bar(float(np.abs(ref32 - want).max()) / KR.LIMIT_ROWS)
    err = float(np.abs(got - want).max()) / KR.LIMIT_ROWS
    print(f"3 x 2^24: row-mean error {err:.3e}, bar {bar:.1e}")
    assert got.shape == (2, 3) and err <= bar
    sigma2, want_s2 = float(KM.bandwidth(b).item()), KR.sigma2(B)  # the closed form at the row limit
    print(f"sigma^2 at n = 2^24: relative error {abs(sigma2 - want_s2) / want_s2:.2e}")
    assert abs(sigma2 - want_s2) <= 1e-12 * want_s2


@pytest.mark.parametrize("family", KR.FAMILIES)
def test_largest_feature_count(KM, family):
    """D = 2^16: 4096 steps of the tile's inner loop, a centred row of 256 KiB."""
    A, B = KR.make_sets(3, 5, KR.LIMIT_D, family, 4000)
    _check_rowsums(KM, A, B, f"{family} 3x5x65536")
    _check_rowsums(KM, B, B, f"{family} self 5x65536", exclude_self=True)
    got = float(KM.bandwidth(_dev(B)).item())
    assert abs(got - KR.sigma2(B)) <= 1e-12 * KR.sigma2(B)


def test_largest_permutation_test(KM):
    """N = 16 384 pooled rows (the 1 GiB matrix) and 4096 assignments: both limits of ffd_mmd_permute at once."""
    n = m = KR.LIMIT_POOLED // 2
    rows = KR.hashed_rows(KR.LIMIT_POOLED)
    X, Y = rows[:n], rows[n:]
    centre = KR.centre_of(Y)
    gammas = KR.ladder(KR.sigma2(Y))
    A = KM.permutation_assignments(n, m, KR.LIMIT_ASSIGNMENTS - 1, 3)
    got = KM.permutation_test(_dev(X), _dev(Y), _dev(centre), gammas, A).cpu().numpy()
    want = KR.perm_stats_of_values(KR.mean_kernel_of_values(gammas), rows[:, 0], A, n, m)
    ref32 = KR.perm_stats_of_values(KR.mean_kernel_of_values(gammas, centre), rows[:, 0], A, n, m)
    bar = KR.bar(float(np.abs(ref32 - want).max()))
    err = float(np.abs(got - want).max())
    print(f"N = 16384, P = 4096: largest |T_p - float64| {err:.3e}, bar {bar:.1e}, T_0 {got[0]:.3e}")
    assert got.shape == (KR.LIMIT_ASSIGNMENTS,) and err <= bar
