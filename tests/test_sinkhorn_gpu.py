"""GPU tests of the entropic optimal-transport statistics (ffd_sinkhorn.hip, ``utils.sinkhorn``, ``SinkhornDivergence``)
against the float64 restatement (tests/sinkhorn_restatement.py).

Bar: a quantity on the costs' scale -- a softmin value, a potential, S, OT_eps -- within max(2e-6 scale, 3 e_ref) of
float64, e_ref the distance of the fp32 centred-Gram twin from float64 on the same input and scale the largest |C_ij| plus
the largest |h_j| of the case (the largest cost for the loop).  Every test prints its measured maximum before it asserts.

Measured on an MI355X (largest error over the bar's scale, over all cases of the test):
  softmin at the tile and run edges   2.97e-7 (floor 2e-6; 1.9e-7 at D <= 17)
  softmin past NN_K_CHUNK, D = 1030   1.67e-7
  the loop's potentials, S and OT     2.29e-7 of the largest cost (5.6e-8 at D = 3)
  S(Y, Y + v) against |v|^2           2.98e-7 absolute, 5.6e-8 of |v|^2
Every measured error is under the floor, so the 3 e_ref branch was never needed.  It exceeds the floor only at eps = 1e+3
mean costs, where the twin's one exp2 per pair rounds 1 - x to 2^-24 (e_ref 1.1e-6 ... 1.3e-6 of the scale at D >= 17);
the device keeps x from its series there.
"""
import numpy as np
import pytest
import torch

import sinkhorn_restatement as SR

pytestmark = pytest.mark.gpu

RUN = SR.RUN_COLUMNS
EPS_FACTORS = (1e-3, 3e-2, 1.0, 30.0, 1e3)  # times the mean cost of the case


@pytest.fixture(scope="module")
def SK():
    from fastfourierdiffusion_amd.utils import sinkhorn

    return sinkhorn


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_softmin(SK, A, B, label, seed):
    """Device softmin of every (h, eps) of the case against float64; returns the largest error over the bar's scale."""
    centre = SR.centre_of(B)
    a, b, c = _dev(A), _dev(B), _dev(centre)
    cost, cost32 = SR.dist2(A, B), SR.gram32_d2(A, B, centre)
    rng = np.random.default_rng(seed)
    mean_cost = float(cost.mean())
    worst = 0.0
    for h in (np.zeros(B.shape[0]), mean_cost * rng.standard_normal(B.shape[0])):
        scale = float(cost.max() + np.abs(h).max())
        hd = _dev(h)
        for factor in EPS_FACTORS:
            eps = factor * mean_cost
            want = SR.softmin_cost(cost, h, eps)
            bar = SR.bar(np.abs(SR.softmin_cost32(cost32, h, eps) - want).max(), scale)
            got = SK.softmin(a, b, c, hd, eps)
            err = float(np.abs(got.cpu().numpy() - want).max())
            worst = max(worst, err / scale)
            assert got.shape == (A.shape[0],) and err <= bar, (label, factor, err, bar)
        old = scale * rng.standard_normal(A.shape[0])
        damped = SK.softmin(a, b, c, hd, eps, old=_dev(old))
        assert torch.equal(damped, 0.5 * (_dev(old) + got)), label  # one more fp64 operation on the same softmin
    return worst


# ------------------------------------------------------------------ softmin against float64 ----
@pytest.mark.parametrize("D", [1, 15, 16, 17, 187])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 130])
def test_softmin_at_the_tile_and_run_edges(SK, nq, D):
    worst = 0.0
    for nr in (1, 255, 256, 257, RUN + 1, 2 * RUN + 1):
        for family in SR.FAMILIES:
            A, B = SR.make_sets(nq, nr, D, family, 5000 + nq + nr + D)
            worst = max(worst, _check_softmin(SK, A, B, f"{family} {nq}x{nr}x{D}", 5100 + nq + nr))
    print(f"softmin nq = {nq}, D = {D}: largest error {worst:.3e} of the scale, floor {SR.FLOOR:.1e}")


@pytest.mark.parametrize("family", SR.FAMILIES)
def test_softmin_past_the_chunk(SK, family):
    """D = 1030 pads to 1040 columns: the tile's sum over the coordinates is taken in two chunks through LDS."""
    A, B = SR.make_sets(3, 260, 1030, family, 5200)
    worst = _check_softmin(SK, A, B, f"{family} 3x260x1030", 5201)
    print(f"softmin {family} D = 1030: largest error {worst:.3e} of the scale")


# ------------------------------------------------------------------ softmin exact cases ----
def _integer_case(nq, nr, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-8, 9, (nq, D)).astype(np.float32)
    B = rng.integers(-8, 9, (nr, D)).astype(np.float32)
    h = rng.integers(-20, 21, nr).astype(np.float64)
    B[nr // 2], A[0] = B[0], B[0]  # row 0 lies on two columns that carry the largest h: a tie at its minimum
    h[nr // 2] = h[0] = 20.0
    return A, B, h


def test_softmin_exact_cases(SK):
    """Integer rows centred on 0: d2 and h - d2 are exact in fp32.  At a tiny eps every term but the minima underflows; at a
    huge one the value is the mean shifted cost (the next term, the variance over 2 eps, is below the floor)."""
    A, B, h = _integer_case(70, 300, 6, 5300)
    a, b, c, hd = _dev(A), _dev(B), _dev(np.zeros(6, np.float32)), _dev(h)
    shifted = SR.dist2(A, B) - h[None, :]
    scale = float(SR.dist2(A, B).max() + np.abs(h).max())
    low = shifted.min(axis=1)
    ties = (shifted == low[:, None]).sum(axis=1)
    assert ties.max() >= 2 and (np.sort(shifted, axis=1)[np.arange(70), ties] - low).min() >= 1.0
    eps = 1e-3  # the nearest other term is exp(-1000)
    got = SK.softmin(a, b, c, hd, eps).cpu().numpy()
    err = float(np.abs(got - (low + eps * np.log(300.0 / ties))).max())
    print(f"tiny eps: off the minimum form by {err:.3e}, floor {SR.FLOOR * scale:.1e}")
    assert err <= SR.FLOOR * scale
    eps = 1e6 * scale
    assert float(shifted.var(axis=1).max()) / (2.0 * eps) <= 0.05 * SR.FLOOR * scale
    got = SK.softmin(a, b, c, hd, eps).cpu().numpy()
    err = float(np.abs(got - shifted.mean(axis=1)).max())
    print(f"huge eps: off the mean form by {err:.3e}, floor {SR.FLOOR * scale:.1e}")
    assert err <= SR.FLOOR * scale
    # one reference row: the shifted cost itself, at any eps
    got = SK.softmin(a, b[:1].contiguous(), c, hd[:1].contiguous(), 3.0).cpu().numpy()
    assert np.array_equal(got, shifted[:, 0])
    # the library overwrites every element of its output (the binding hands it fresh memory: call it directly)
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    out = torch.full((70,), float("nan"), device="cuda", dtype=torch.float64)
    nbytes = lib.ffd_sinkhorn_softmin_work_bytes(70, 300, 6)
    work = torch.full(((nbytes + 7) // 8,), float("nan"), device="cuda", dtype=torch.float64)
    N.check(lib.ffd_sinkhorn_softmin(a.data_ptr(), 70, b.data_ptr(), 300, 6, c.data_ptr(), hd.data_ptr(), 5.0, None,
                                     out.data_ptr(), work.data_ptr(), nbytes, N.current_stream_ptr(a.device)), None,
            "ffd_sinkhorn_softmin")
    assert torch.isfinite(out).all() and torch.equal(out, SK.softmin(a, b, c, hd, 5.0))
    assert np.abs(out.cpu().numpy() - SR.softmin_cost(shifted + h[None, :], h, 5.0)).max() <= SR.FLOOR * scale


# ------------------------------------------------------------------ softmin bit-identity ----
@pytest.mark.parametrize("family", SR.FAMILIES)
def test_softmin_bit_identity(SK, family):
    A, B = SR.make_sets(200, 2 * RUN + 300, 17, family, 5400)
    a, b, c = _dev(A), _dev(B), _dev(SR.centre_of(B))
    cost = SR.dist2(A, B)
    h = _dev(float(cost.mean()) * np.random.default_rng(5401).standard_normal(B.shape[0]))
    for eps in (1e-2 * float(cost.mean()), float(cost.mean())):
        whole = SK.softmin(a, b, c, h, eps)
        assert torch.equal(whole, SK.softmin(a, b, c, h, eps))  # two runs
        for cut in (64, 77, 199):  # a query set cut in two, at and off a tile edge
            parts = torch.cat([SK.softmin(a[:cut].contiguous(), b, c, h, eps), SK.softmin(a[cut:].contiguous(), b, c, h, eps)])
            assert torch.equal(whole, parts), cut
        more = torch.cat([a, _dev(SR.make_sets(150, 1, 17, family, 5402)[0])])  # a set with rows appended
        assert torch.equal(whole, SK.softmin(more, b, c, h, eps)[:200])
        shifted = torch.cat([more[200:], a])  # ... and put in front: other rows around it, another place in its tile
        assert torch.equal(whole, SK.softmin(shifted, b, c, h, eps)[150:])
    # the self problem: one buffer as both sets, and a copy of it as the query set
    hb = _dev(np.zeros(B.shape[0]))
    assert torch.equal(SK.softmin(b, b, c, hb, 1.0), SK.softmin(b.clone(), b, c, hb, 1.0))


# ------------------------------------------------------------------ the loop ----
LOOP_SHAPES = [(2, 2), (64, 64), (65, 257), (130, 513)]


def _schedule_for(Y, blur):
    return SR.schedule(SR.diameter2(Y, SR.centre_of(Y)), blur * blur * SR.sigma2(Y))


@pytest.mark.parametrize("D", [3, 187])
@pytest.mark.parametrize("n,m", LOOP_SHAPES)
def test_loop_against_the_restatement(SK, n, m, D):
    worst = 0.0
    for blur in (0.3, 0.05):
        for family in SR.FAMILIES:
            X, Y = SR.make_sets(n, m, D, family, 5500 + n + m + D)
            centre, sched = SR.centre_of(Y), _schedule_for(Y, blur)
            want, twin = SR.sinkhorn(X, Y, sched), SR.sinkhorn32(X, Y, centre, sched)
            got = SK.sinkhorn_divergence(_dev(X), _dev(Y), _dev(centre), sched)
            scale = float(max(SR.dist2(X, Y).max(), SR.dist2(X, X).max(), SR.dist2(Y, Y).max()))
            have = {"f": got.f, "g": got.g, "p": got.p, "q": got.q}
            for key in ("f", "g", "p", "q"):
                err = float(np.abs(have[key].cpu().numpy() - want[key]).max())
                bar = SR.bar(np.abs(twin[key] - want[key]).max(), scale)
                worst = max(worst, err / scale)
                assert err <= bar, (family, blur, key, err, bar)
            for value, key in ((got.divergence, "S"), (got.ot_xy, "ot_xy"), (got.change, "change")):
                err = abs(value - want[key])
                bar = SR.bar(abs(twin[key] - want[key]), scale)
                worst = max(worst, err / scale)
                assert err <= bar, (family, blur, key, err, bar)
    print(f"loop {n} x {m} x {D}: largest error {worst:.3e} of the largest cost, floor {SR.FLOOR:.1e}")


@pytest.mark.parametrize("family", SR.FAMILIES)
def test_equal_sets_give_exactly_zero(SK, family):
    """The x|y and x|x passes do identical work on identical data, pass for pass: what the Jacobi ordering buys."""
    for m, D in ((2, 3), (65, 16), (257, 187), (RUN + 1, 5)):
        _, Y = SR.make_sets(1, m, D, family, 5600 + m)
        y = _dev(Y)
        got = SK.sinkhorn_divergence(y.clone(), y, _dev(SR.centre_of(Y)), _schedule_for(Y, 0.1))
        assert got.divergence == 0.0 and torch.equal(got.f, got.p) and torch.equal(got.g, got.q), (m, D, got.divergence)
        assert torch.equal(got.f, got.g)


def test_a_shift_gives_its_square(SK):
    """S(Y, Y + v) = |v|^2 on a converged schedule (the identity and the schedule of the host test)."""
    _, Y = SR.make_sets(1, 23, 5, "clustered", 33)
    v = np.array([0.5, -1.0, 0.25, 2.0, -0.125], np.float32)
    Z = Y + v
    centre = np.concatenate([Y, Z]).astype(np.float64).mean(axis=0)
    sched = SR.schedule(max(SR.diameter2(Y, centre), SR.diameter2(Z, centre)), SR.sigma2(Y), 0.5, 300)
    got = SK.sinkhorn_divergence(_dev(Y), _dev(Z), _dev(centre.astype(np.float32)), sched)
    v2 = float(v.astype(np.float64) @ v.astype(np.float64))
    scale = float(SR.dist2(Y, Z).max())
    print(f"S(Y, Y + v) = {got.divergence:.9f} against |v|^2 = {v2}: off by {abs(got.divergence - v2):.2e}, "
          f"change {got.change:.1e}, floor {SR.FLOOR * scale:.1e}")
    assert abs(got.divergence - v2) <= SR.FLOOR * scale and got.change <= SR.FLOOR * scale


@pytest.mark.parametrize("family", SR.FAMILIES)
def test_supplied_q_and_the_self_potential_bit_for_bit(SK, family):
    X, Y = SR.make_sets(130, 300, 17, family, 5700)
    x, y, c = _dev(X), _dev(Y), _dev(SR.centre_of(Y))
    sched = _schedule_for(Y, 0.2)
    first = SK.sinkhorn_divergence(x, y, c, sched)
    again = SK.sinkhorn_divergence(x, y, c, sched, q=first.q)
    for key in ("f", "g", "p", "q"):
        assert torch.equal(getattr(first, key), getattr(again, key)), key
    assert (first.divergence, first.ot_xy, first.change) == (again.divergence, again.ot_xy, again.change)
    # q is a function of y, the centre and the schedule alone: another x, and the softmin entry pass by pass
    other = SK.sinkhorn_divergence(_dev(SR.make_sets(40, 1, 17, family, 5701)[0]), y, c, sched)
    assert torch.equal(first.q, other.q) and torch.equal(first.q, SK.self_potential(y, c, sched))


def test_change_falls_along_a_lengthened_schedule(SK):
    X, Y = SR.make_sets(130, 257, 16, "gaussian", 5800)
    x, y, c = _dev(X), _dev(Y), _dev(SR.centre_of(Y))
    diam2, eps = SR.diameter2(Y, SR.centre_of(Y)), 0.25 * SR.sigma2(Y)
    changes = [SK.sinkhorn_divergence(x, y, c, SR.schedule(diam2, eps, 0.5, n_final)).change for n_final in (1, 4, 16, 64)]
    want = [SR.sinkhorn(X, Y, SR.schedule(diam2, eps, 0.5, n_final))["change"] for n_final in (1, 4, 16, 64)]
    print("change along n_final = 1, 4, 16, 64:", " ".join(f"{v:.2e}" for v in changes), "| float64",
          " ".join(f"{v:.2e}" for v in want))
    assert all(b < a for a, b in zip(changes, changes[1:])) and changes[-1] < 1e-3 * changes[0]


# ------------------------------------------------------------------ the metric end to end ----
def test_metric_and_collection_against_the_float64_pipeline(SK):
    from functools import partial

    from fastfourierdiffusion_amd.sampling import KernelMMD, SinkhornDivergence
    from fastfourierdiffusion_amd.sampling.metrics import MetricCollection
    from fastfourierdiffusion_amd.utils.fourier import dft

    rng = np.random.default_rng(5900)
    Y = rng.standard_normal((300, 12, 2)).astype(np.float32)
    X = (rng.standard_normal((130, 12, 2)) * 1.1 + 0.2).astype(np.float32)
    Yf, Xf = Y.reshape(300, -1), X.reshape(130, -1)
    metric = SinkhornDivergence(Yf, blur=0.2)
    got = metric(Xf)
    want, price = SR.pipeline(Xf, Yf, blur=0.2)
    scale = float(max(SR.dist2(Xf, Yf).max(), SR.dist2(Yf, Yf).max(), SR.dist2(Xf, Xf).max()))
    assert tuple(got) == tuple(want)
    centre = SR.centre_of(Yf)
    sched = SR.schedule(SR.diameter2(Yf, centre), want["sinkhorn_eps"])
    twin = SR.sinkhorn32(Xf, Yf, centre, sched)
    full = SR.sinkhorn(Xf, Yf, sched)
    bar = SR.bar(max(abs(twin["S"] - full["S"]), abs(twin["ot_xy"] - full["ot_xy"])), scale)
    for key in ("sinkhorn_divergence", "sinkhorn_ot", "sinkhorn_change"):
        print(f"{key}: device {got[key]:.9f}, float64 {want[key]:.9f}, bar {bar:.1e}")
        assert abs(got[key] - want[key]) <= bar, key
    assert got["sinkhorn_eps"] == pytest.approx(want["sinkhorn_eps"], rel=1e-12)
    assert got["sinkhorn_distance"] == max(got["sinkhorn_divergence"], 0.0) ** 0.5
    assert metric(Xf) == got  # the kept self potential: the same bits
    tp = metric.transport_price(Xf).cpu().numpy()
    assert np.abs(tp - price).max() <= SR.bar(np.abs((twin["f"] - twin["p"]) - price).max(), scale)
    base = metric.baseline_metrics
    half = SR.sinkhorn(Yf[150:], Yf[:150], sched)
    assert abs(base["sinkhorn_divergence_self"] - half["S"]) <= bar
    coll = MetricCollection([partial(KernelMMD, scales=(1.0,)), partial(SinkhornDivergence, blur=0.2)],
                            original_samples=torch.from_numpy(Y))
    found = coll(torch.from_numpy(X))
    assert found["time_sinkhorn_divergence"] == got["sinkhorn_divergence"]
    in_freq = SR.pipeline(dft(torch.from_numpy(X)).reshape(130, -1).cpu().numpy(),
                          dft(torch.from_numpy(Y)).reshape(300, -1).cpu().numpy(), blur=0.2)[0]
    assert abs(found["freq_sinkhorn_divergence"] - in_freq["sinkhorn_divergence"]) <= 4.0 * bar
    assert "time_mmd2" in found and "freq_sinkhorn_change_self" in found


def test_transport_price_ranks_a_planted_far_tenth_first():
    from fastfourierdiffusion_amd.sampling import SinkhornDivergence

    rng = np.random.default_rng(6000)
    Y = rng.standard_normal((400, 16)).astype(np.float32)
    X = rng.standard_normal((200, 16)).astype(np.float32)
    far = rng.choice(200, 20, replace=False)
    direction = rng.standard_normal(16)
    X[far] += (3.0 * direction / np.linalg.norm(direction) * np.sqrt(16)).astype(np.float32)  # 3 sigma sqrt(D) away
    price = SinkhornDivergence(Y, blur=0.3).transport_price(X).cpu().numpy()
    top = set(np.argsort(-price)[:20].tolist())
    print(f"planted rows among the 20 dearest: {len(top & set(far.tolist()))} of 20")
    assert top == set(far.tolist())


def test_refusals_on_the_device(SK):
    X, Y = SR.make_sets(20, 30, 4, "gaussian", 6100)
    x, y, c = _dev(X), _dev(Y), _dev(SR.centre_of(Y))
    h = torch.zeros(30, device="cuda", dtype=torch.float64)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(AssertionError):
            SK.softmin(x, y, c, h, bad)
    for bad in (1e-60, 1e60):  # positive and finite, but no fp32 exponent factor: the library's refusal
        with pytest.raises(AssertionError, match="ffd_sinkhorn_softmin"):
            SK.softmin(x, y, c, h, bad)
        with pytest.raises(AssertionError, match="ffd_sinkhorn"):
            SK.sinkhorn_divergence(x, y, c, [1.0, bad])
    with pytest.raises(AssertionError):
        SK.softmin(x, y, c, h[:29], 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(x, y, c, h.float(), 1.0)
    with pytest.raises(AssertionError):
        SK.softmin(x, y[:, :3], c, h, 1.0)
    with pytest.raises(AssertionError):
        SK.sinkhorn_divergence(x, y, c, [1.0], q=torch.zeros(20, device="cuda", dtype=torch.float64))
    with pytest.raises(Exception):
        SK.softmin(x.cpu(), y, c, h, 1.0)
    with pytest.raises(Exception):
        SK.softmin(x, y, c, h.cpu(), 1.0)
    # the library's own overlap refusal: the output inside the potential
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    nbytes = lib.ffd_sinkhorn_softmin_work_bytes(30, 30, 4)
    work = torch.empty((nbytes + 7) // 8, device="cuda", dtype=torch.float64)
    before = h.clone()
    assert lib.ffd_sinkhorn_softmin(y.data_ptr(), 30, y.data_ptr(), 30, 4, c.data_ptr(), h.data_ptr(), 1.0, None, h.data_ptr(),
                                    work.data_ptr(), nbytes, N.current_stream_ptr(y.device)) == -1
    torch.cuda.synchronize()
    assert torch.equal(h, before)
