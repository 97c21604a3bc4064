"""GPU tests of the nearest-neighbour kernels past one slab, one chunk and one column block (ffd_neighbours.hip): the
sizes at which ``k_nn_colpart`` / ``k_nn_colmean`` sum more than one 1024-row slab or fill a second 256-column block, the
search runs a chunk wider than the tiles that exist, the widest chunk and a partial one after it, several query blocks,
``k_nn_ball`` walks more than one column tile per workgroup, and the accepted limits themselves (2^24 rows, D = 2^16).

The contracts, the scale and the bar are those of tests/test_neighbours_gpu.py, whose helpers this file imports; the
inputs (``NR.SIZE_CASES``) and everything float64 says about them come from tests/neighbours_restatement.py.  Where the
whole float64 distance matrix would cost more than 2e8 multiply-adds the structural checks still cover every row and the
value checks 64 of them (``NR.knn_rows``): the tile edges and a random draw.  Ball counts run twice: at the radii as
they are, inside float64's band at radius^2 -+ bar scale, and at ``NR.gapped_radii`` of them, where that band is closed
for every row (asserted on the CPU in tests/test_neighbours_host.py) and the device's counts must EQUAL float64's."""
import functools
import time

import numpy as np
import pytest
import torch

import neighbours_restatement as NR
from test_neighbours_gpu import (DEFAULT_BUDGET, UNIT, _device_arrays, check_ball, check_search_structure,  # noqa: F401
                                 check_search_values, lib, run_ball, run_search)  # (lib: the module's fixture)

pytestmark = pytest.mark.gpu

SIZE_CASES = [(i, f) for f in NR.FAMILIES for i in range(len(NR.SIZE_CASES))]
FULL_CHECK = 2e8  # nq nr D up to which the value checks cover every row


def sample_rows(n, seed, must=None):
    """At most 64 sorted distinct rows of n: the listed ones that exist (by default the first and last row of the first
    two and of the last 64-row tile, and the two sides of column 8192), the rest drawn at random."""
    must = (0, 63, 64, 127, 8191, 8192, (n - 1) // 64 * 64, n - 1) if must is None else must
    must = sorted({r for r in must if 0 <= r < n})
    rest = np.setdiff1d(np.arange(n), must)
    rng = np.random.default_rng(seed)
    extra = rng.choice(rest, size=min(len(rest), 64 - len(must)), replace=False)
    return np.sort(np.concatenate([np.array(must, np.int64), extra.astype(np.int64)]))


def scale_and_bar(A, B, rows):
    """The scale of the whole pair (A, B) and the bar max(2e-6, 3 e_ref) with e_ref taken over the listed query rows."""
    scale = NR.scale(A, B)
    e_ref = float(np.abs(NR.gram32(A[rows], B).astype(np.float64) - NR.dist2(A[rows], B)).max()) / scale
    return scale, max(2e-6, 3.0 * e_ref)


@functools.lru_cache(maxsize=None)
def size_reference(i, family):
    """Everything float64 says about a size case, computed once; the arrays are read-only."""
    Q, R, k = NR.make_size_case(i, family)
    (nq, D), nr = Q.shape, R.shape[0]
    scale, bar = NR.scale(Q, R), NR.bar(Q, R)
    rows = None if float(nq) * nr * D <= FULL_CHECK else sample_rows(nq, 5200 + i)
    want = NR.knn(Q, R, k) if rows is None else NR.knn_rows(Q, R, k, rows)
    rad = NR.size_radius2(R, k)
    gapped, moved = NR.gapped_radii(Q, R, rad, bar, scale)
    out = dict(Q=Q, R=R, k=k, scale=scale, bar=bar, rows=rows, knn=want, rad=rad, gapped=gapped, moved=moved)
    for a in (Q, R, rad, gapped, *want):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the contracts at size ----
@pytest.mark.parametrize("i,family", SIZE_CASES)
def test_search_at_size(lib, i, family):
    ref = size_reference(i, family)
    Q, R, k = ref["Q"], ref["R"], ref["k"]
    got_d, got_i = run_search(lib, Q, R, k)
    check_search_structure(got_d, got_i, Q.shape[0], R.shape[0], k)
    check_search_values(got_d, got_i, Q, R, k, ref["knn"], ref["scale"], ref["bar"], rows=ref["rows"])


@pytest.mark.parametrize("i,family", SIZE_CASES)
def test_ball_count_at_size(lib, i, family):
    ref = size_reference(i, family)
    Q, R = ref["Q"], ref["R"]
    # 1. the radii as they are: inside the band, which is open for a few rows
    check_ball(run_ball(lib, Q, R, ref["rad"]), Q, R, ref["rad"], ref["scale"], ref["bar"])
    # 2. the gapped radii: the band is closed, so this is an equality test over every row
    got = run_ball(lib, Q, R, ref["gapped"])
    lo, hi = check_ball(got, Q, R, ref["gapped"], ref["scale"], ref["bar"])
    print(f"{ref['moved']} of {len(ref['rad'])} radii moved")
    assert np.array_equal(lo, hi) and np.array_equal(got, NR.ball_counts(Q, R, ref["gapped"]))
    assert 0 < got.mean() < R.shape[0]  # neither no ball nor every ball


@pytest.mark.parametrize("family", NR.FAMILIES)
@pytest.mark.parametrize("i", [1, 2])
def test_exclude_self_at_size(lib, i, family):
    """Q = R, the same buffer, with the pair i == j in the first column chunk, on its edge and in the last one."""
    ref = size_reference(i, family)
    R, k = ref["R"], ref["k"]
    nr = R.shape[0]
    rows = sample_rows(nr, 6200 + i, must=(0, 63, 64, 8191, 8192, nr - 1))  # and 58 random ones
    assert {0, 63, 64, 8191, 8192, nr - 1} <= set(rows.tolist()) and len(rows) == 64
    scale, bar = scale_and_bar(R, R, rows)
    got_d, got_i = run_search(lib, R, R, k, exclude_self=True, same=True)
    check_search_structure(got_d, got_i, nr, nr, k, exclude_self=True)
    check_search_values(got_d, got_i, R, R, k, NR.knn_rows(R, R, k, rows, exclude_self=True), scale, bar, rows=rows)
    gapped, moved = NR.gapped_radii(R, R, ref["rad"], bar, scale, exclude_self=True, rows=rows)
    got = run_ball(lib, R, R, gapped, exclude_self=True, same=True)
    lo, hi = check_ball(got, R, R, gapped, scale, bar, exclude_self=True, rows=rows)
    print(f"{moved} of {nr} radii moved")
    assert np.array_equal(lo, hi) and np.array_equal(got[rows], lo)
    wide = np.float32(1.5) * gapped
    check_ball(run_ball(lib, R, R, wide, exclude_self=True, same=True), R, R, wide, scale, bar, exclude_self=True, rows=rows)


@pytest.mark.parametrize("i", [1, 2])
def test_copies_of_the_columns_at_a_chunk_edge(lib, i):
    """Query rows overwritten with the reference rows at the last column of the widest chunk, the first of the next and
    the single column of the last chunk come out at that index and exactly 0.0; a ball of unbounded radius about the
    last column alone, every other radius 0, holds every query row once."""
    ref = size_reference(i, "gaussian")
    Q, R, k = ref["Q"].copy(), ref["R"], ref["k"]
    nr = R.shape[0]
    planted = {0: nr - 1, 63: 8191, 64: 8192, Q.shape[0] - 1: 0}
    for qi, ri in planted.items():
        Q[qi] = R[ri]
    got_d, got_i = run_search(lib, Q, R, k)
    for qi, ri in planted.items():
        assert got_d[qi, 0] == 0.0 and got_i[qi, 0] == ri, (qi, got_d[qi], got_i[qi])
    assert (got_d[:, 0] == 0.0).sum() == len(planted)
    rad = np.zeros(nr, np.float32)
    rad[nr - 1] = np.float32(1e30)
    count = run_ball(lib, Q, R, rad)
    others = np.setdiff1d(np.arange(Q.shape[0]), list(planted))
    assert (count[others] == 1).all() and count[0] == 1 and set(count[[63, 64, -1]].tolist()) <= {1, 2}


# ------------------------------------------------------------------ bit-identity across the plans ----
@pytest.mark.parametrize("i,family", [(3, "clustered"), (1, "gaussian")])
def test_bits_do_not_depend_on_the_plan(lib, i, family):
    """Budgets of 0, 16, 32 and 64 tiles: chunks of 1, 16, 32 and 32 column tiles (33 down to 2 chunks), query blocks
    of 1, 1, 1 and 2 row tiles (up to five, the last one ragged); the default takes everything at once."""
    ref = size_reference(i, family)
    Q, R, k = ref["Q"], ref["R"], ref["k"]
    nq, nr, D = Q.shape[0], R.shape[0], Q.shape[1]
    base = run_search(lib, Q, R, k)
    smallest = lib.ffd_nn_work_bytes(nq, nr, D, k, 0)
    for units, block in ((0, 1), (16, 16), (32, 32), (64, 64)):
        assert lib.ffd_nn_work_bytes(nq, nr, D, k, units * UNIT) == smallest + (block - 1) * UNIT  # cbt x qbt tiles
        again = run_search(lib, Q, R, k, budget=units * UNIT)
        assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1]), units
    h = nq // 2 + 1
    for budget in (DEFAULT_BUDGET, 16 * UNIT):
        parts = [run_search(lib, Q[:h], R, k, budget=budget), run_search(lib, Q[h:], R, k, budget=budget)]
        assert np.array_equal(base[0], np.concatenate([p[0] for p in parts]))
        assert np.array_equal(base[1], np.concatenate([p[1] for p in parts]))
    counts = run_ball(lib, Q, R, ref["rad"])
    assert np.array_equal(counts, run_ball(lib, Q, R, ref["rad"]))
    assert np.array_equal(counts, np.concatenate([run_ball(lib, Q[:h], R, ref["rad"]), run_ball(lib, Q[h:], R, ref["rad"])]))


# ------------------------------------------------------------------ the limits, exactly ----
def test_longest_query_set(lib):
    """nq = 2^24 integer rows against 5: every squared distance is an integer, the fp32 centred Gram form misses it by
    less than 0.5 (asserted on the CPU) and no query is equidistant from two reference rows, so the answers are exact."""
    t0 = time.perf_counter()
    Q, R = NR.hashed_rows(NR.LIMIT_ROWS), np.array(NR.LIMIT_REFERENCE, np.float32)[:, None]
    value = Q[:, 0].astype(np.int64)  # a row is one of 1021 values: numpy's answer per value, then per row
    d = (np.arange(1021.0)[:, None] - R[None, :, 0].astype(np.float64)) ** 2  # (1021, 5)
    got_d, got_i = run_search(lib, Q, R, 1)
    assert got_d.shape == (NR.LIMIT_ROWS, 1) and got_i.shape == (NR.LIMIT_ROWS, 1)
    assert np.array_equal(got_i[:, 0], d.argmin(axis=1)[value]) and np.array_equal(got_d[:, 0], d.min(axis=1)[value])
    for rad in ([2.5] * 5, [10000.5] * 5, [2.5, 10000.5, 100.5, 0.5, 250000.5]):
        rad = np.array(rad, np.float32)
        got = run_ball(lib, Q, R, rad)
        assert got.dtype == np.int32 and np.array_equal(got, (d <= rad.astype(np.float64)[None, :]).sum(axis=1)[value]), rad
    print(f"nq = 2^24: {time.perf_counter() - t0:.2f} s with the host side")


def test_longest_reference_set(lib):
    """nr = 2^24 integer rows (16 384 slabs, 2048 column chunks at the default budget, 1024 column tiles per ball-count
    workgroup), queries 0, 510 and 1020, k = 2: the two lowest indices holding the query's value, at exactly 0.0."""
    t0 = time.perf_counter()
    R, Q = NR.hashed_rows(NR.LIMIT_ROWS), np.array(NR.LIMIT_QUERIES, np.float32)[:, None]
    got_d, got_i = run_search(lib, Q, R, 2)
    want_i = np.array([np.flatnonzero(R[:, 0] == q)[:2] for q in Q[:, 0]], np.int32)
    assert want_i.shape == (3, 2)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, np.zeros((3, 2)))
    got = run_ball(lib, Q, R, np.full(NR.LIMIT_ROWS, 100.5, np.float32))
    want = [int(((R[:, 0].astype(np.float64) - float(q)) ** 2 <= 100.5).sum()) for q in Q[:, 0]]
    assert got.tolist() == want and min(want) > 100000
    print(f"nr = 2^24: {time.perf_counter() - t0:.2f} s with the host side")


def test_reference_mean_sums_every_slab(lib):
    """The Gram form is the same distance about any centre, so a reference mean that lost a slab only costs precision and
    the cases above cannot see it.  Integer rows 2^23 + v, v < 1021, can: about their mean (an integer in fp32) every
    term of the Gram form is exact, about a mean that lost the second slab's single row (8184 lower) the norms round to
    multiples of 8.  nr = 1025, so exact answers -- ties by the lower index included -- need both slabs."""
    offset = np.float32(NR.LIMIT_OFFSET)
    R, Q = NR.hashed_rows(1025) + offset, NR.hashed_rows(1025 + 70)[1025:] + offset
    want_d, want_i = NR.knn(Q, R, 5)
    got_d, got_i = run_search(lib, Q, R, 5)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)
    rad = ((np.arange(1025) % 7) ** 2 + 0.5).astype(np.float32)
    assert np.array_equal(run_ball(lib, Q, R, rad), NR.ball_counts(Q, R, rad))
    want_d, want_i = NR.knn(R, R, 5, exclude_self=True)
    got_d, got_i = run_search(lib, R, R, 5, exclude_self=True, same=True)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)


# ------------------------------------------------------------------ the Python path at size ----
def test_manifold_scores_at_size(lib):
    """Y (16 385, 8) originals, X (1100, 8) samples, k = 5: ``count_x`` runs two column tiles per workgroup, ``count_y``
    on 16 385 query rows."""
    from fastfourierdiffusion_amd.sampling.metrics import ManifoldMetrics
    from fastfourierdiffusion_amd.utils import neighbours

    rng = np.random.default_rng(5300)
    Y = rng.standard_normal((16385, 8)).astype(np.float32)
    X = rng.standard_normal((1100, 8)).astype(np.float32)
    k, n, m = 5, 16385, 1100
    got = neighbours.manifold_scores(Y, X, k)
    arrays = _device_arrays(Y, X, k)
    own = NR.scores_from_arrays(*arrays, k)
    assert tuple(got) == NR.KEYS
    for key in NR.KEYS:
        assert abs(got[key] - own[key]) <= 1e-12 * max(1.0, abs(own[key])), (key, got[key], own[key])
    print(got)
    assert 0.0 < got["precision"] < 1.0 and 0.0 < got["coverage"] < 1.0 and got["copy_share"] == 0.0
    self_y, xy_d2, xy_idx, yx_d2, count_x, count_y = arrays
    assert self_y.shape == (n, k) and xy_d2.shape == (m, 1) and yx_d2.shape == (n, 1)
    ry, rx = sample_rows(n, 5301), sample_rows(m, 5302)
    # the three searches: the structure over all rows, the values on 64 rows each (the indices come from a second,
    # bit-identical run: _device_arrays keeps only the one ffd_nn_scores reads)
    for d2, (A, B, kk, rows, excl) in ((self_y, (Y, Y, k, ry, True)), (xy_d2, (X, Y, 1, rx, False)), (yx_d2, (Y, X, 1, ry, False))):
        idx = _device_index(neighbours, A, B, kk, excl)
        check_search_structure(d2, idx, A.shape[0], B.shape[0], kk, exclude_self=excl)
        check_search_values(d2, idx, A, B, kk, NR.knn_rows(A, B, kk, rows, excl), *scale_and_bar(A, B, rows), rows=rows)
    assert np.array_equal(xy_idx, _device_index(neighbours, X, Y, 1, False))
    # the two ball counts at the device's own radii, on 64 rows each
    rad_y, rad_x = self_y[:, k - 1].astype(np.float32), _device_self(neighbours, X, k)[:, k - 1].astype(np.float32)
    check_ball(count_x, X, Y, rad_y, *scale_and_bar(X, Y, rx), rows=rx)
    check_ball(count_y, Y, X, rad_x, *scale_and_bar(Y, X, ry), rows=ry)
    # the cached original set gives the bits of a fresh object
    metric = ManifoldMetrics(Y, k=k)
    first = metric(X)
    assert metric._original_self is not None
    assert first == got and metric(X) == got and ManifoldMetrics(Y, k=k)(X) == got


def _device_index(neighbours, A, B, k, exclude_self):
    a = torch.from_numpy(A).cuda()
    b = a if exclude_self else torch.from_numpy(B).cuda()
    return neighbours.nearest_neighbours(a, b, k, exclude_self=exclude_self)[1].cpu().numpy()


def _device_self(neighbours, X, k):
    return neighbours.self_search(torch.from_numpy(X).cuda(), k)[0].cpu().numpy()
