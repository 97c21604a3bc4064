"""GPU tests of the dynamic-time-warping kernels (ffd_dtw.hip, ``utils.dtw``, ``DTWMetrics``) against the float64
restatement (tests/dtw_restatement.py).

Bar of every comparison with float64: max(2e-6 * the case's largest float64 value, 3 * the largest
|fp32 restatement - float64| of the case) (``DR.bar``).  Every test prints its measured share of the bar before it
asserts.  Measured on an MI355X: the device's values are the fp32 restatement's to the bit in every case of
``test_pairs_against_float64`` (the printed "off the fp32 restatement" is 0.0), so the device's share of the bar is 1/3
wherever the bar's second term decides (L = 187, 512, 4096) and less where the first does: at most 0.08 at L <= 3, 0.11 at
L = 17, 0.18 at L = 48, 0.23 around the time chunk (L = 63, 64, 65), 0.06 at C = 64."""
import numpy as np
import pytest
import torch

import dtw_restatement as DR

pytestmark = pytest.mark.gpu

TIME_CHUNK = 64  # ffd_dtw.hip DTW_TC
QUERY_TILE, QUERY_BLOCK = 4, 64  # DTW_QT, DTW_QBLOCK
COLUMN_CHUNK = 8192  # DTW_MAX_CBT * DTW_CBLOCK
WINDOWS = (0, 1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)  # every instance edge (0, 4, 8, 16, 32, 64) from both sides
ROWS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def DT():
    from fastfourierdiffusion_amd.utils import dtw

    return dtw


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _windows(L):
    """The listed windows that series of L accept, and one at or above L - 1 where the band still fits."""
    found = sorted({min(w, L - 1) for w in WINDOWS if min(w, L - 1) <= 64})
    return found + ([L + 5] if L - 1 <= 64 else [])


# ------------------------------------------------------------------ paired rows ----
@pytest.mark.parametrize("family", sorted(DR.FAMILIES))
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("L", [1, 2, 3, 17, 48, TIME_CHUNK - 1, TIME_CHUNK, TIME_CHUNK + 1, 187, 512])
def test_pairs_against_float64(DT, L, C, family):
    windows = _windows(L) if L < 512 else [0, 5, 17, 33, 64]
    worst = apart = 0.0
    for wi, w in enumerate(windows):
        rows = ROWS if L <= TIME_CHUNK + 1 else (ROWS[(wi + C) % 5], ROWS[(wi + C + 2) % 5])
        for n in rows:
            A, B = DR.FAMILIES[family](n, L, C, 1000 + L + n), DR.FAMILIES[family](n, L, C, 2000 + L + n)
            got = DT.dtw_pairs(A, B, w).cpu().numpy()
            f64, f32 = DR.dtw2(A, B, w), DR.dtw2(A, B, w, np.float32)
            bar = DR.bar(f64, f32)
            err = float(np.abs(got.astype(np.float64) - f64).max())
            assert got.shape == (n,) and got.dtype == np.float32 and err <= bar, (L, C, w, n, err, bar)
            worst, apart = max(worst, err / bar), max(apart, float(np.abs(got - f32).max() / f64.max()))
    print(f"{family} L {L} C {C}: largest share of the bar {worst:.3f}, off the fp32 restatement by {apart:.1e} of the scale")


def test_pairs_exact_cases(DT):
    for L, C in ((40, 1), (40, 2), (TIME_CHUNK + 9, 1), (150, 3)):
        A, B = DR.gaussian(70, L, C, 31), DR.gaussian(70, L, C, 32)
        ints_a, ints_b = DR.integer_rows(70, L, C, 33), DR.integer_rows(70, L, C, 34)
        prev = None
        for w in (0, 1, 3, 4, 5, 8, 9, 16, 17, 32, 33):
            assert (DT.dtw_pairs(A, A.copy(), w) == 0.0).all(), (L, C, w)  # a copy reads 0.0
            ab, ba = DT.dtw_pairs(A, B, w), DT.dtw_pairs(B, A, w)
            assert torch.equal(ab, ba), (L, C, w)  # symmetric to the bit
            assert prev is None or bool((ab <= prev).all()), (L, C, w)  # non-increasing in w
            prev = ab
            got = DT.dtw_pairs(ints_a, ints_b, w).cpu().numpy().astype(np.float64)
            assert np.array_equal(got, DR.dtw2(ints_a, ints_b, w)), (L, C, w)  # integer rows: float64's value exactly
            for s in sorted({0, min(1, w), w // 2, w}):
                a, b = DR.shifted_pulse(L, C, s)
                assert float(DT.dtw_pairs(a, b, w)[0]) == 0.0, (L, C, w, s)  # a shift inside the band costs nothing
            a, b = DR.shifted_pulse(L, C, w + 1)
            assert float(DT.dtw_pairs(a, b, w)[0]) > 0.0, (L, C, w)


# ------------------------------------------------------------------ search ----
def _check_search(DT, Q, R, w, k, exclude_self=False, label=""):
    """The nearest-neighbour contract against float64; returns (dist2, index) as numpy arrays."""
    q = _dev(Q)
    r = q if exclude_self else _dev(R)
    d2, idx = DT.dtw_neighbours(q, r, w, k=k, exclude_self=exclude_self)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    nq, nr = Q.shape[0], R.shape[0]
    assert d2.shape == idx.shape == (nq, k) and d2.dtype == np.float32 and idx.dtype == np.int32
    D64, D32 = DR.all_pairs(Q, R, w), DR.all_pairs(Q, R, w, np.float32)
    bar = DR.bar(D64, D32)
    if exclude_self:
        D64[np.arange(nq), np.arange(nq)] = np.inf
        assert (idx != np.arange(nq)[:, None]).all()
    assert (idx >= 0).all() and (idx < nr).all() and all(len(set(row)) == k for row in idx.tolist())
    of_index = float(np.abs(d2 - np.take_along_axis(D64, idx.astype(np.int64), axis=1)).max())
    of_rank = float(np.abs(d2 - np.sort(D64, axis=1)[:, :k]).max())
    print(f"{label} {nq}x{nr} k {k}: off the returned index's float64 by {of_index / bar:.3f} bar, off the r-th smallest by "
          f"{of_rank / bar:.3f} bar")
    assert of_index <= bar and of_rank <= bar, (label, of_index, of_rank, bar)
    assert (np.diff(d2, axis=1) >= 0).all()
    if k == 1:
        again = DT.dtw_pairs(Q, R[idx[:, 0]], w).cpu().numpy()
        assert np.array_equal(again, d2[:, 0])  # the search's value is the pair kernel's, to the bit
    return d2, idx


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 257])
def test_search_shapes(DT, nr):
    for nq, L, C, w in ((1, 9, 2, 2), (3, 17, 1, 4), (QUERY_TILE, 9, 2, 0), (5, 12, 3, 5), (QUERY_BLOCK - 1, 9, 1, 3),
                        (QUERY_BLOCK + 1, 6, 2, 30)):
        Q, R = DR.pulses(nq, L, C, 50 + nq), DR.pulses(nr, L, C, 60 + nr)
        for k in (1, 5, 32):
            if k <= nr:
                _check_search(DT, Q, R, w, k, label=f"L {L} C {C} w {w}")


def test_search_past_one_column_chunk(DT):
    Q, R = DR.gaussian(3, 5, 1, 70), DR.gaussian(COLUMN_CHUNK + 1, 5, 1, 71)
    R[COLUMN_CHUNK] = Q[1]  # the one row of the second chunk is a copy
    d2, idx = _check_search(DT, Q, R, 1, 5, label="chunk + 1")
    assert d2[1, 0] == 0.0 and idx[1, 0] == COLUMN_CHUNK
    _check_search(DT, Q, R, 1, 1, label="chunk + 1")


def test_search_exclude_self_ties_and_copies(DT):
    Y = DR.gaussian(131, 14, 2, 72)
    for k in (1, 5, 32):
        _check_search(DT, Y, Y, 3, k, exclude_self=True, label="self")
    # duplicated reference rows: integer rows, so float64's stable order is the required answer exactly
    Q, R = DR.integer_rows(37, 10, 1, 73), DR.integer_rows(300, 10, 1, 74)
    R[257], R[64], R[299] = R[3], R[63], R[3]
    for w in (0, 2):
        D64 = DR.all_pairs(Q, R, w)
        order = np.argsort(D64, axis=1, kind="stable")[:, :32]
        d2, idx = DT.dtw_neighbours(Q, R, w, k=32)
        assert np.array_equal(idx.cpu().numpy(), order)  # ties by the lower index
        assert np.array_equal(d2.cpu().numpy().astype(np.float64), np.take_along_axis(D64, order, axis=1))
    # planted copies read 0.0 at rank 0
    Q, R = DR.gaussian(20, 30, 2, 75), DR.gaussian(400, 30, 2, 76)
    where = np.random.default_rng(77).choice(400, size=20, replace=False)
    R[where] = Q
    d2, idx = _check_search(DT, Q, R, 4, 5, label="copies")
    assert (d2[:, 0] == 0.0).all() and np.array_equal(idx[:, 0], where) and (d2[:, 1] > 0.0).all()


def test_search_bit_identity(DT):
    Q, R = DR.gaussian(130, 12, 1, 78), DR.gaussian(700, 12, 1, 79)
    q, r = _dev(Q), _dev(R)
    for w, k in ((3, 5), (0, 1), (11, 32)):
        d2, idx = DT.dtw_neighbours(q, r, w, k=k)
        for budget in (None, 0, 1 << 18, 1 << 20):  # a second run, then one, four and sixteen units
            kwargs = {} if budget is None else {"budget_bytes": budget}
            d2_b, idx_b = DT.dtw_neighbours(q, r, w, k=k, **kwargs)
            assert torch.equal(d2_b, d2) and torch.equal(idx_b, idx), (w, k, budget)
        for cut in (1, 63, 66):  # the query set cut in two
            lo, hi = DT.dtw_neighbours(q[:cut].contiguous(), r, w, k=k), DT.dtw_neighbours(q[cut:].contiguous(), r, w, k=k)
            assert torch.equal(torch.cat([lo[0], hi[0]]), d2) and torch.equal(torch.cat([lo[1], hi[1]]), idx), (w, k, cut)
        # reference rows appended behind: a row's old winners keep their index, and rows no new row beats do not change
        more = _dev(np.concatenate([R, DR.gaussian(300, 12, 1, 80)]))
        d2_m, idx_m = DT.dtw_neighbours(q, more, w, k=k)
        same = (idx_m < 700).all(dim=1)  # (at k = 32 every list takes some new row: the prefix rule below covers those)
        assert torch.equal(d2_m[same], d2[same]) and torch.equal(idx_m[same], idx[same])
        new_i, new_d, old_i, old_d = idx_m.cpu().numpy(), d2_m.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()
        for i in range(130):  # the old rows a list keeps are a prefix of the old list, in its order, with their bits
            kept = new_i[i] < 700
            count = int(kept.sum())
            assert np.array_equal(new_i[i][kept], old_i[i][:count]) and np.array_equal(new_d[i][kept], old_d[i][:count]), (w, k, i)


def test_limits(DT):
    # the longest series at the widest band
    Q, R = DR.pulses(2, 4096, 1, 81, jitter=40), DR.pulses(3, 4096, 1, 82, jitter=40)
    _check_search(DT, Q, R, 64, 1, label="L 4096 w 64")
    _check_search(DT, Q, R, 64, 3, label="L 4096 w 64")
    # the most channels
    Q, R = DR.gaussian(5, 8, 64, 83), DR.gaussian(70, 8, 64, 84)
    for w in (0, 2, 7):
        _check_search(DT, Q, R, w, 5, label=f"C 64 w {w}")
    got = DT.dtw_pairs(Q, R[:5], 3).cpu().numpy()
    f64, f32 = DR.dtw2(Q, R[:5], 3), DR.dtw2(Q, R[:5], 3, np.float32)
    assert np.abs(got - f64).max() <= DR.bar(f64, f32)
    # past 65 535 row tiles: integer rows, answered exactly
    Q, R = DR.integer_rows(65537, 2, 1, 85), DR.integer_rows(1, 2, 1, 86)
    d2, idx = DT.dtw_neighbours(Q, R, 1)
    want = DR.dtw2(Q, np.repeat(R, 65537, axis=0), 1)
    assert np.array_equal(d2.cpu().numpy()[:, 0].astype(np.float64), want) and not idx.any()


def test_refusals_on_the_device_leave_the_outputs_untouched(DT):
    from fastfourierdiffusion_amd import _native as N

    lib = N.lib()
    nq, nr, L, C, k = 6, 9, 7, 2, 3
    q, r = _dev(DR.gaussian(nq, L, C, 87)), _dev(DR.gaussian(nr, L, C, 88))
    d2 = torch.full((nr, k), -7.0, device="cuda")
    idx = torch.full((nr, k), -7, device="cuda", dtype=torch.int32)
    need = lib.ffd_dtw_work_bytes(nq, nr, L, C, 2, k, 0)
    work = torch.zeros(need // 4 + 4, device="cuda")

    def search(q=q.data_ptr(), nq=nq, r=r.data_ptr(), nr=nr, L=L, C=C, w=2, k=k, excl=0, work=work.data_ptr(), nbytes=need):
        return lib.ffd_dtw_search(q, nq, r, nr, L, C, w, k, excl, d2.data_ptr(), idx.data_ptr(), work, nbytes, None)

    for kw in (dict(q=None), dict(nq=0), dict(w=-1), dict(k=0), dict(k=10), dict(k=33), dict(excl=1), dict(nbytes=need - 1),
               dict(work=work.data_ptr() + 4), dict(work=q.data_ptr()), dict(q=r.data_ptr(), nq=nr, excl=1, k=9)):
        assert search(**kw) == -1, kw
    for kw in (dict(L=4097, C=1), dict(C=65), dict(L=2048, C=33), dict(L=200, w=65), dict(nq=(1 << 24) + 1)):
        assert search(**kw) == -2, kw
    assert lib.ffd_dtw_pairs(q.data_ptr(), r.data_ptr(), nq, L, C, -1, d2.data_ptr(), None) == -1
    assert lib.ffd_dtw_pairs(q.data_ptr(), r.data_ptr(), nq, 200, 1, 65, d2.data_ptr(), None) == -2
    assert lib.ffd_dtw_pairs(q.data_ptr(), q.data_ptr(), nq, L, C, 1, q.data_ptr(), None) == -1
    out6 = torch.full((6,), -7.0, device="cuda", dtype=torch.float64)
    assert lib.ffd_dtw_scores(d2.data_ptr(), d2.data_ptr(), d2.data_ptr(), d2.data_ptr(), d2.data_ptr(), 1, 5, out6.data_ptr(),
                              None) == -1
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all()) and bool((idx == -7).all()) and bool((out6 == -7.0).all())
    with pytest.raises(NotImplementedError):
        DT.dtw_pairs(torch.zeros(2, 200, 1, device="cuda"), torch.zeros(2, 200, 1, device="cuda"), 0.5)


# ------------------------------------------------------------------ scores, DTWMetrics ----
@pytest.fixture(scope="module")
def score_refs():
    """float64's pipeline and the fp32 restatement's searches of the three Gaussian cases, computed once."""
    found = []
    for case in range(len(DR.SCORE_CASES)):
        X, Y, w = DR.score_case(case)
        found.append((X, Y, w, DR.pipeline(X, Y, w), DR.searches(X, Y, w, np.float32)))
    return found


def _numbers_within_the_bar(got, want, s64, s32, label):
    """The two distance means within the bar of the distances they average; the warp gain, a ratio of order one, within
    max(2e-6, 3 * the fp32 restatement's distance from float64) and inside [0, 1]."""
    root64 = np.concatenate([np.sqrt(s64[key]) for key in ("xy", "yx")])
    root32 = np.concatenate([np.sqrt(s32[key].astype(np.float64)) for key in ("xy", "yx")])
    bar = DR.bar(root64, root32)
    for key in DR.SCORE_KEYS[:2]:
        print(f"{label} {key}: {got[key]:.9g} against {want[key]:.9g}, {abs(got[key] - want[key]) / bar:.3f} bar")
        assert abs(got[key] - want[key]) <= bar, key
    gain32 = DR.scores_from_searches(s32)[0]["dtw_warp_gain"]
    gain_bar = max(DR.REL, 3.0 * abs(gain32 - want["dtw_warp_gain"]))
    print(f"{label} dtw_warp_gain: {got['dtw_warp_gain']:.9g} against {want['dtw_warp_gain']:.9g}, bar {gain_bar:.1e}")
    assert 0.0 <= got["dtw_warp_gain"] <= 1.0 and abs(got["dtw_warp_gain"] - want["dtw_warp_gain"]) <= gain_bar


@pytest.mark.parametrize("case", range(len(DR.SCORE_CASES)))
def test_scores_and_metric_against_the_float64_pipeline(DT, score_refs, case):
    from fastfourierdiffusion_amd import _native as N
    from fastfourierdiffusion_amd.sampling.metrics import DTWMetrics

    X, Y, w, (want, counts, s64), s32 = score_refs[case]
    n, m = Y.shape[0], X.shape[0]
    metric = DTWMetrics(Y, window=w)
    got = metric(X)
    assert tuple(got) == DR.SCORE_KEYS
    # the 1-NN counts are float64's (tests/test_dtw_host.py shows no row within reach of the bar)
    assert (round(got["dtw_1nn_accuracy_samples"] * m), round(got["dtw_1nn_accuracy_originals"] * n)) == counts
    for key in DR.SCORE_KEYS[3:]:
        assert got[key] == want[key], key
    _numbers_within_the_bar(got, want, s64, s32, f"case {case}")
    assert metric(X.reshape(m, -1)) == got and metric(_dev(X)) == got  # flat samples, device samples, the kept YY search
    assert DTWMetrics(Y, window=0)(X)["dtw_warp_gain"] == 0.0
    # the scoring kernel alone, on float64's searches rounded to fp32: the float64 formula of the same arrays
    arrays = {key: s64[key].astype(np.float32) for key in s64}
    dev = {key: _dev(value) for key, value in arrays.items()}
    out = torch.empty(6, device="cuda", dtype=torch.float64)
    N.check(N.lib().ffd_dtw_scores(dev["xx"].data_ptr(), dev["xy"].data_ptr(), dev["yx"].data_ptr(), dev["yy"].data_ptr(),
                                   dev["e2"].data_ptr(), n, m, out.data_ptr(), None), None, "ffd_dtw_scores")
    direct = DR.scores_from_searches(arrays)[0]
    for key, value in zip(DR.SCORE_KEYS, out.tolist()):
        assert value == pytest.approx(direct[key], rel=1e-12, abs=1e-15), key
    # the _self baseline: the two halves of the originals
    base = metric.baseline_metrics
    half = n // 2
    want_self, counts_self, s64_self = DR.pipeline(Y[half:], Y[:half], w)
    assert tuple(base) == tuple(f"{key}_self" for key in DR.SCORE_KEYS)
    assert base["dtw_1nn_accuracy_samples_self"] == counts_self[0] / (n - half)
    assert base["dtw_1nn_accuracy_originals_self"] == counts_self[1] / half
    _numbers_within_the_bar({key: base[f"{key}_self"] for key in DR.SCORE_KEYS}, want_self, s64_self,
                            DR.searches(Y[half:], Y[:half], w, np.float32), f"case {case} _self")


def test_metric_collection_on_the_device():
    from functools import partial

    from fastfourierdiffusion_amd.sampling import metrics as M

    X, Y, w = DR.score_case(1)
    tx, ty = torch.from_numpy(X), torch.from_numpy(Y)  # (the collection's transform takes tensors)
    sliced = partial(M.SlicedWasserstein, random_seed=3, num_directions=16)
    before = M.MetricCollection([sliced], original_samples=ty)(tx)
    after = M.MetricCollection([sliced, partial(M.DTWMetrics, window=w)], original_samples=ty)(tx)
    assert {key: after[key] for key in before} == before and [key for key in after if "dtw" not in key] == list(before)
    dtw_keys = sorted(key for key in after if "dtw" in key)
    assert dtw_keys == sorted([f"time_{key}" for key in DR.SCORE_KEYS] + [f"time_{key}_self" for key in DR.SCORE_KEYS])
    assert after["time_dtw_1nn_accuracy"] == DR.pipeline(X, Y, w)[0]["dtw_1nn_accuracy"]


def test_warp_gain_sees_a_phase_jitter():
    """Samples that are the originals' pulses with a fresh phase jitter inside the band: re-timing removes more of their
    nearest-original distance than of the same samples with the jitter taken out.  Both numbers come from the device."""
    from fastfourierdiffusion_amd.sampling.metrics import DTWMetrics

    n, m, L, w = 96, 80, 64, 4
    rng = np.random.default_rng(90)
    t = np.arange(L, dtype=np.float64)[None, :, None]

    def draw(count, shift):
        height, width = 1.0 + rng.random((count, 1, 1)), 2.0 + rng.random((count, 1, 1))
        noise = 0.02 * rng.standard_normal((count, L, 1))
        return lambda s: (height * np.exp(-0.5 * ((t - 30.0 - s * shift) / width) ** 2) + noise).astype(np.float32)

    Y = draw(n, 0.0)(0.0)
    samples = draw(m, rng.integers(-w, w + 1, size=(m, 1, 1)).astype(np.float64))
    jittered, aligned = samples(1.0), samples(0.0)
    metric = DTWMetrics(Y, window=w)
    gain_jittered, gain_aligned = metric(jittered)["dtw_warp_gain"], metric(aligned)["dtw_warp_gain"]
    print(f"dtw_warp_gain: jittered {gain_jittered:.4f}, the same samples aligned {gain_aligned:.4f}")
    assert 0.0 <= gain_aligned < gain_jittered <= 1.0
