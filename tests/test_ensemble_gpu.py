"""GPU tests of the ensemble scores (ffd_ens_pointwise, ffd_ens_energy, ``ensemble_scores``) against the float64 numpy
restatement (tests/ens_restatement.py, which never calls the code under test).

Bars.  Per point the members are the same fp32 numbers on both sides and the device accumulates in fp64: ``below`` and
``equal`` are exact, ``quant`` is within 1e-12 relative, ``crps`` and ``crps_mean`` within 1e-12 max|x|.  The energy
score of a series is within max(2e-6 R, 3 e32): R the series' largest centred weighted row norm, e32 the error of the fp32
centred restatement on the same input (the project's standing form of bar; 2e-6 is the w2 projection's)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ens_restatement as E

pytestmark = pytest.mark.gpu

LEVELS = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
BIG_M = 8191  # from here on: S = 1, D = 3


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import os

    from fastfourierdiffusion_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        from fastfourierdiffusion_amd.build import build

        build()
    return _native.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _work(lib, S, m, D, nq, budget):
    nbytes = lib.ffd_ens_work_bytes(S, m, D, nq, budget)
    assert nbytes > 0
    return torch.empty((nbytes + 15) // 16 * 2, device="cuda", dtype=torch.float64), nbytes


def run_point(lib, X, y, w=None, levels=LEVELS, fair=False, budget=1 << 28):
    from fastfourierdiffusion_amd import _native as N

    S, m, D = X.shape
    nq = len(levels)
    Xd, yd, wd = _dev(X), _dev(y), _dev(w)
    crps = torch.full((S, D), float("nan"), device="cuda", dtype=torch.float64)
    mean = torch.full((S,), float("nan"), device="cuda", dtype=torch.float64)
    quant = torch.full((nq, S, D), float("nan"), device="cuda", dtype=torch.float64)
    below = torch.full((S, D), -1, device="cuda", dtype=torch.int32)
    equal = torch.full((S, D), -1, device="cuda", dtype=torch.int32)
    work, nbytes = _work(lib, S, m, D, nq, budget)
    lv = (C.c_double * nq)(*levels)
    rc = lib.ffd_ens_pointwise(Xd.data_ptr(), yd.data_ptr(), wd.data_ptr() if wd is not None else None,
                               1 if w is None else w.shape[0], S, m, D, lv, nq, int(fair), crps.data_ptr(), mean.data_ptr(),
                               quant.data_ptr(), below.data_ptr(), equal.data_ptr(), work.data_ptr(), nbytes,
                               N.current_stream_ptr(Xd.device))
    assert rc == 0, rc
    return dict(crps=crps.cpu().numpy(), crps_mean=mean.cpu().numpy(), quant=quant.cpu().numpy(),
                below=below.cpu().numpy(), equal=equal.cpu().numpy())


def run_energy(lib, X, y, w=None, fair=False, budget=1 << 28):
    from fastfourierdiffusion_amd import _native as N

    S, m, D = X.shape
    Xd, yd, wd = _dev(X), _dev(y), _dev(w)
    out = torch.full((S,), float("nan"), device="cuda", dtype=torch.float64)
    work, nbytes = _work(lib, S, m, D, 0, budget)
    rc = lib.ffd_ens_energy(Xd.data_ptr(), yd.data_ptr(), wd.data_ptr() if wd is not None else None,
                            1 if w is None else w.shape[0], S, m, D, int(fair), out.data_ptr(), work.data_ptr(), nbytes,
                            N.current_stream_ptr(Xd.device))
    assert rc == 0, rc
    return out.cpu().numpy()


def weights(mode, S, D, seed):
    rng = np.random.default_rng(seed)
    if mode == "ones":
        return None
    if mode == "single":  # all but one coordinate observed
        w = np.zeros((1, D), np.float32)
        w[0, rng.integers(D)] = 1
        return w
    w = (rng.uniform(size=(1 if mode == "shared" else S, D)) < 0.6).astype(np.float32)
    w[:, rng.integers(D)] = 1
    return w


def check_point(got, X, y, w, levels, fair):
    """-> (crps error / max|x|, largest relative quantile error); asserts the bars."""
    scale = float(np.abs(X).max())
    b, e = E.ranks(X, y, w)
    assert np.array_equal(got["below"], b) and np.array_equal(got["equal"], e)
    q = E.quantiles(X, levels, w)
    qerr = float((np.abs(got["quant"] - q) / np.maximum(np.abs(q), 1e-300)).max())
    c, cm = E.crps(X, y, w, fair), E.crps_mean(X, y, w, fair)
    cerr = max(float(np.abs(got["crps"] - c).max()), float(np.abs(got["crps_mean"] - cm).max())) / scale
    assert qerr <= 1e-12, qerr
    assert cerr <= 1e-12, cerr
    return cerr, qerr


def energy_refs(X, y, w):
    """fair -> (bar, float64 value) from one evaluation of the restatement's terms."""
    m = X.shape[1]
    t64, p64 = E.truth_term(X, y, w), E.pair_term(X, w)
    t32 = E.truth_term(X, y, w, np.float32)
    p32 = E.pair_term(X, w, np.float32, "centred")
    _, R = E.centred_rows(X, w)
    out = {}
    for fair in (False, True):
        if fair and m < 2:
            continue
        z2 = 2.0 * E.z_norm(m, fair)
        ref = t64 / m - p64 / z2
        e32 = np.abs(np.asarray(t32 / np.float32(m) - p32 / np.float32(z2), dtype=np.float64) - ref)
        out[fair] = (np.maximum(2e-6 * R, 3.0 * e32), ref, R)
    return out


def check_energy(lib, X, y, w, refs=None):
    """-> the largest error / R; asserts the bar for both estimators."""
    worst = 0.0
    for fair, (bar, ref, R) in (refs or energy_refs(X, y, w)).items():
        err = np.abs(run_energy(lib, X, y, w, fair) - ref)
        assert (err <= bar).all(), (fair, err, bar)
        worst = max(worst, float((err / np.maximum(R, 1e-300)).max()) if R.max() > 0 else 0.0)
    return worst


# ------------------------------------------------------------------ device against float64 ----
@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 257, 8191, 8192, 8193])
def test_scores_against_float64(lib, m):
    dims = (3,) if m >= BIG_M else (1, 3, 15, 16, 17, 64, 187, 260)
    worst = dict(crps=0.0, quant=0.0, energy=0.0)
    for D in dims:
        for S in ((1,) if m >= BIG_M else (1, 3)):
            X, y = E.make_case(S, m, D, seed=1000 * m + 10 * D + S)
            y[:, 0] = X[:, m // 2, 0]  # a truth equal to a member
            for k, mode in enumerate(("ones", "shared", "per-series", "single")):
                w = weights(mode, S, D, seed=m + D + k)
                for fair in ((False,) if m < 2 else (False, True)):
                    c, q = check_point(run_point(lib, X, y, w, LEVELS, fair), X, y, w, LEVELS, fair)
                    worst["crps"], worst["quant"] = max(worst["crps"], c), max(worst["quant"], q)
                if m >= BIG_M and mode in ("shared", "per-series"):
                    continue  # (the float64 pair term of 8192 members: twice per size is enough)
                worst["energy"] = max(worst["energy"], check_energy(lib, X, y, w))
    print(f"m = {m}: crps error / max|x| {worst['crps']:.2e}, quantile relative {worst['quant']:.2e}, "
          f"energy error / R {worst['energy']:.2e}")


# ------------------------------------------------------------------ further properties ----
def test_ties_and_ranks(lib):
    rng = np.random.default_rng(5)
    S, m, D = 2, 37, 6
    X = rng.integers(-2, 3, size=(S, m, D)).astype(np.float32)
    y = X[:, 5, :].copy()
    y[:, 1] = 0.5   # between two values
    y[:, 2] = -7.0  # below every member
    y[:, 3] = 9.0   # above every member
    got = run_point(lib, X, y)
    check_point(got, X, y, None, LEVELS, False)
    assert (got["equal"][:, 0] >= 1).all() and (got["equal"][:, 1] == 0).all()
    assert (got["below"][:, 2] == 0).all() and (got["below"][:, 3] == m).all() and (got["equal"][:, 3] == 0).all()
    assert ((got["below"] + got["equal"]) <= m).all()


def test_edge_levels_are_minimum_and_maximum(lib):
    for m in (1, 2, 65, 8193):
        X, y = E.make_case(2, m, 3, seed=m, offset=0.5)
        q = run_point(lib, X, y, levels=(0.0, 1.0))["quant"]
        assert np.array_equal(q[0], X.min(axis=1).astype(np.float64)), m
        assert np.array_equal(q[1], X.max(axis=1).astype(np.float64)), m


def test_energy_is_crps_for_one_coordinate(lib):
    for m, fair in ((2, False), (64, True), (257, False), (1500, True)):
        X, y = E.make_case(3, m, 1, seed=20 + m)
        bar, _, _ = E.energy_bar(X, y, None, fair)
        es = run_energy(lib, X, y, None, fair)
        cr = run_point(lib, X, y, None, LEVELS, fair)["crps"][:, 0]
        print(f"D = 1, m = {m}: |energy - crps| {np.abs(es - cr).max():.2e}, bar {bar.min():.2e}")
        assert (np.abs(es - cr) <= bar).all(), (m, es, cr, bar)


def test_one_member(lib):
    X, y = E.make_case(3, 1, 5, seed=31)
    w = np.float32([[1, 0, 1, 1, 0]])
    got = run_point(lib, X, y, w)
    want = np.abs(X[:, 0, :].astype(np.float64) - y) * w
    assert np.abs(got["crps"] - want).max() <= 1e-12 * np.abs(X).max()
    bar, _, _ = E.energy_bar(X, y, w)
    norm = np.sqrt((((X[:, 0, :].astype(np.float64) - y) ** 2) * w).sum(axis=1))
    assert (np.abs(run_energy(lib, X, y, w) - norm) <= bar).all()


def test_tight_ensemble_holds_the_energy_bar(lib):
    X, y = E.make_case(**E.TIGHT)
    bar, ref, _ = E.energy_bar(X, y)
    err = np.abs(run_energy(lib, X, y) - ref)
    print(f"tight ensemble (offset {E.TIGHT['offset']}, spread {E.TIGHT['spread']}): error {err[0]:.3e}, bar {bar[0]:.3e}")
    assert (err <= bar).all()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_zero_weight_coordinates_do_not_reach_any_output(lib):
    S, m, D = 3, 130, 21
    X, y = E.make_case(S, m, D, seed=41)
    for mode in ("shared", "per-series"):
        w = weights(mode, S, D, seed=7)
        off = np.broadcast_to(w == 0, (S, D))
        X2, y2 = X.copy(), y.copy()
        X2[np.broadcast_to(off[:, None, :], X.shape)] = 1e30
        y2[off] = -1e30
        a, b = run_point(lib, X, y, w), run_point(lib, X2, y2, w)
        assert _same(a, b)
        for k in ("crps", "below", "equal"):
            assert (a[k][off] == 0).all(), k
        assert (a["quant"][:, off] == 0).all()
        for fair in (False, True):
            assert np.array_equal(run_energy(lib, X, y, w, fair), run_energy(lib, X2, y2, w, fair))


def test_bit_identity(lib):
    S, m, D = 3, 300, 17
    X, y = E.make_case(S, m, D, seed=51)
    X[2], y[2] = X[0], y[0]  # the same series at positions 0 and 2
    w = weights("shared", S, D, seed=3)
    a = run_point(lib, X, y, w)
    ea = run_energy(lib, X, y, w)
    assert _same(a, run_point(lib, X, y, w)) and np.array_equal(ea, run_energy(lib, X, y, w))  # run to run
    one = run_point(lib, X[:1], y[:1], w)
    e1 = run_energy(lib, X[:1], y[:1], w)
    for pos in (0, 2):  # a series alone against the same series inside a batch
        assert np.array_equal(one["crps"][0], a["crps"][pos]) and np.array_equal(one["quant"][:, 0], a["quant"][:, pos])
        assert np.array_equal(one["below"][0], a["below"][pos]) and np.array_equal(one["equal"][0], a["equal"][pos])
        assert one["crps_mean"][0] == a["crps_mean"][pos] and e1[0] == ea[pos]
    # another block cut: one row (s, d) and one series at a time
    small = lib.ffd_ens_work_bytes(S, m, D, len(LEVELS), 0)
    assert small < lib.ffd_ens_work_bytes(S, m, D, len(LEVELS), 1 << 28)
    assert _same(a, run_point(lib, X, y, w, budget=0)) and np.array_equal(ea, run_energy(lib, X, y, w, budget=0))
    mid = 8 * S * D + 8 * m * 20  # about 20 rows at a time: blocks that cut through a series
    assert _same(a, run_point(lib, X, y, w, budget=mid))


def test_end_to_end_on_imputed_series(lib):
    """``ensemble_scores`` on the output of ``DiffusionSampler.impute`` (a small mixture: L = 16, C = 1, 8 components, 20
    steps, 64 completions of a series observed on a prefix) against the restatement, at the same bars."""
    from fastfourierdiffusion_amd.models.score_models import MixtureScoreModule
    from fastfourierdiffusion_amd.sampling import ensemble_scores
    from fastfourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fastfourierdiffusion_amd.schedulers.sde import VPScheduler
    from fastfourierdiffusion_amd.utils.fourier import dft

    L, Cn, K, m = 16, 1, 8, 64
    g = torch.Generator().manual_seed(0)
    data = torch.randn(K + 1, L, Cn, generator=g)
    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(L)
    model = MixtureScoreModule.from_data(dft(data[:K]).cpu(), sch, bandwidth=0.2).cuda().eval()
    series = data[K]
    mask = torch.zeros(L)
    mask[:6] = 1.0
    ens = DiffusionSampler(model, m, rng="philox", seed=4).impute(series, mask, m, 20, final_replace=True)
    assert tuple(ens.shape) == (m, L, Cn) and bool(torch.isfinite(ens).all())
    out = ensemble_scores(ens, series, mask=mask, quantiles=LEVELS)
    X = ens.numpy().reshape(1, m, L * Cn)
    y = series.numpy().reshape(1, L * Cn)
    w = (1.0 - mask.numpy())[None, :]
    got = dict(crps=out["crps"].numpy().reshape(1, -1), crps_mean=out["crps_mean"].numpy(),
               quant=out["quantiles"].numpy().reshape(len(LEVELS), 1, -1), below=out["below"].numpy().reshape(1, -1),
               equal=out["equal"].numpy().reshape(1, -1))
    check_point(got, X, y, w, LEVELS, False)
    bar, ref, _ = E.energy_bar(X, y, w)
    assert (np.abs(out["energy_score"].numpy() - ref) <= bar).all()
    # the observed points are excluded: their outputs are 0, the mean runs over the unobserved ones
    assert (out["crps"][0, :6] == 0).all() and (out["below"][0, :6] == 0).all() and (out["quantiles"][:, 0, :6] == 0).all()
    assert (out["crps"][0, 6:] > 0).all()
    assert float(out["crps_mean"][0]) == pytest.approx(float(out["crps"][0, 6:].mean()), rel=1e-13)
