"""CPU tests of tests/philox_restatement.py, the float64 restatement the device's noise generator is held to
(tests/test_philox_gpu.py): the Random123 known-answer vectors, the facts of the fp32 uniform, slicing at any alignment
and across the 2^32 / 2^34 element boundaries, the distribution of the restated draws, and the stream-tag plan of
include/ffd.h -- no two updates of one run share a stream inside the limits the loop entries enforce.
"""
import math

import numpy as np
import pytest
import torch

import philox_restatement as PR

# Random123's kat_vectors for philox4x32-10: counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


# ------------------------------------------------------------------ 1. known answers ----
@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_random123_known_answers(counter, key, want):
    assert tuple(int(w) for w in PR.philox4x32_10(counter, key)) == want


def test_known_answers_survive_vectorisation_and_blocks_differ():
    """the three vectors as ONE array call (the restatement is used on arrays), and every input word matters"""
    cs = np.array([k[0] for k in KAT], dtype=np.uint64).T
    # (the key is one pair per call: run the array call per key and pick that vector's lane)
    for i, (_, key, want) in enumerate(KAT):
        out = PR.philox4x32_10(tuple(cs), key)
        assert tuple(int(w[i]) for w in out) == want
    base = PR.philox4x32_10((1, 2, 3, 4), (5, 6))
    for j in range(4):
        c = [1, 2, 3, 4]
        c[j] += 1
        assert all(int(a) != int(b) for a, b in zip(PR.philox4x32_10(c, (5, 6)), base)), j
    for key in ((6, 6), (5, 7)):
        assert all(int(a) != int(b) for a, b in zip(PR.philox4x32_10((1, 2, 3, 4), key), base)), key
    assert [int(w) for w in PR.philox4x32_10((1, 2, 3, 4), (5, 6), rounds=9)] != [int(w) for w in base]


# ------------------------------------------------------------------ 2. the fp32 uniforms ----
def test_uniform_facts():
    half, plain = PR.uniform24_half, PR.uniform24
    assert half(0).dtype == np.float32 and plain(0).dtype == np.float32
    # endpoints: the smallest u is 2^-25 (words 0 .. 0xFF), so |z| <= sqrt(-2 ln 2^-25) = sqrt(50 ln 2) = 5.8871
    assert float(half(0)) == 2.0 ** -25 and float(half(0xFF)) == 2.0 ** -25 and float(half(0x100)) == 1.5 * 2.0 ** -24
    assert abs(PR.Z_MAX - 5.8871) < 5e-5 and math.isclose(math.sqrt(-2.0 * math.log(2.0 ** -25)), PR.Z_MAX, rel_tol=1e-15)
    # the top 256 words give u = 1.0 exactly ((2^24 - 1) + 0.5 rounds to 2^24 in fp32), the word below them does not
    top = np.arange(0xFFFFFF00, 0x100000000, dtype=np.uint64)
    assert top.size == 256 and np.all(half(top) == np.float32(1.0))
    assert float(half(0xFFFFFEFF)) == 1.0 - 2.0 ** -23  # (2^24 - 2) + 0.5 ties to the even 2^24 - 2
    # below 2^23 the half is kept, from 2^23 on the sum rounds to nearest-even: u is never 0 and never above 1
    assert float(half(0x7FFFFF00)) == (2 ** 23 - 1 + 0.5) * 2.0 ** -24
    assert float(half(0x80000000)) == 2.0 ** 23 * 2.0 ** -24 and float(half(0x80000100)) == (2 ** 23 + 2) * 2.0 ** -24
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    assert half(w).min() > 0.0 and half(w).max() <= 1.0
    # the time draws' uniform is exact, in [0, 1)
    assert float(plain(0)) == 0.0 and float(plain(0xFF)) == 0.0 and float(plain(0xFFFFFFFF)) == 1.0 - 2.0 ** -24
    assert np.array_equal(plain(w).astype(np.float64), (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)


def test_box_muller_edges():
    # u1 = 1: r = 0 and the pair is exactly 0 whatever the angle (a rate of 2^-24 per pair)
    for w2 in (0, 0x40000000, 0x9E3779B9, 0xFFFFFFFF):
        c, s = PR.box_muller(0xFFFFFF00, w2)
        assert float(c) == 0.0 and float(s) == 0.0
    # the smallest u1: r = Z_MAX, reached at the angle 2 pi u2 nearest 0 (u2 = 2^-25: cos = 1 - 1.8e-14)
    c, s = PR.box_muller(0, 0)
    assert abs(float(c) - PR.Z_MAX) < 1e-12 and 0.0 < float(s) < 2e-6
    w = np.random.default_rng(2).integers(0, 1 << 32, (2, 1 << 16), dtype=np.uint64)
    c, s = PR.box_muller(np.zeros_like(w[0]), w[1])
    assert np.abs(c).max() <= PR.Z_MAX and np.abs(s).max() <= PR.Z_MAX and np.allclose(c * c + s * s, PR.Z_MAX ** 2, rtol=1e-14)
    # u2 = 1/4, 1/2, 3/4 are off the lattice (k + 0.5) 2^-24, so no draw sits exactly on an axis below 2^23 ...
    c, s = PR.box_muller(0x12345678, 0x40000000)  # u2 = 1/4 + 2^-25
    assert float(c) < 0.0 < float(s) and abs(float(c)) < 1e-6
    # ... and from 2^23 on u2 is a multiple of 2^-23: u2 = 1/2 and 3/4 are hit
    c, s = PR.box_muller(0x12345678, 0x80000000)
    assert float(c) < 0.0 and abs(float(s)) < 1e-15
    # slot order: the draws of one block are cos, sin of (x, y), then cos, sin of (z, w)
    x, y, z, w4 = (int(v[0]) for v in PR._blocks(42, 7, 5, 1))
    got = PR.normals(42, 7, 20, 4)
    want = [*map(float, PR.box_muller(x, y)), *map(float, PR.box_muller(z, w4))]
    assert got.tolist() == want and len(set(want)) == 4


# ------------------------------------------------------------------ 3. slicing ----
@pytest.mark.parametrize("boundary", [0, 1 << 32, 1 << 34, 1 << 40, (1 << 62) - 64], ids=["0", "2^32", "2^34", "2^40", "2^62"])
def test_unaligned_calls_are_slices_of_the_aligned_call(boundary):
    """2^32 elements: the block index crosses 2^30; 2^34: counter word 0 wraps and counter word 1 becomes 1."""
    seed, tag = (1 << 40) + 17, 3
    lo = max(boundary - 24, 0)
    full = PR.normals(seed, tag, lo, 64)
    full_u = PR.uniforms(seed, tag, lo, 64)
    assert full.shape == (64,) and len(set(full.tolist())) == 64
    for g0 in range(lo, lo + 9):
        for n in (0, 1, 2, 3, 4, 5, 31):
            assert np.array_equal(PR.normals(seed, tag, g0, n), full[g0 - lo:g0 - lo + n]), (g0, n)
            assert np.array_equal(PR.uniforms(seed, tag, g0, n), full_u[g0 - lo:g0 - lo + n]), (g0, n)
    # element by element: slot g & 3 of block g >> 2, counter (lo32, hi32, tag, "FFDF"), key (lo32 seed, hi32 seed)
    for g in (lo, lo + 23, lo + 24, lo + 27):
        q = g >> 2
        words = [int(v) for v in PR.philox4x32_10((q & 0xFFFFFFFF, q >> 32, tag, 0x46464446), (seed & 0xFFFFFFFF, seed >> 32))]
        pair = PR.box_muller(*words[:2]) if g & 3 < 2 else PR.box_muller(*words[2:])
        assert float(pair[g & 1]) == float(full[g - lo])
        assert float(PR.uniform24(words[g & 3])) == float(full_u[g - lo])


def test_every_key_and_counter_word_selects_another_stream():
    base = PR.normals(42, 7, 0, 16)
    for other in (PR.normals(43, 7, 0, 16), PR.normals(42 + (1 << 32), 7, 0, 16), PR.normals(42, 8, 0, 16),
                  PR.normals(42, 7, 1 << 34, 16), PR.normals(42, 7, 16, 16)):
        assert np.abs(other - base).max() > 0.5 and not np.any(other == base)
    shape = (3, 5, 3)
    z = PR.sample_normals(9, 11, 4, shape)
    assert np.array_equal(z.ravel(), PR.normals(9, 11, 4 * 15, 45))
    assert np.array_equal(PR.sample_normals(9, 11, 5, (2, 5, 3)), z[1:])  # counting is by the global sample index


# ------------------------------------------------------------------ 4. distribution ----
SIGMAS = 4.5
KS_BAR = 1.95  # sqrt(N) D: p ~ 1e-3 under Kolmogorov's law
P4 = math.erfc(4.0 / math.sqrt(2.0))  # P(|z| > 4) = 6.334e-5
P5 = math.erfc(5.0 / math.sqrt(2.0))  # P(|z| > 5) = 5.733e-7 (the cut at 5.8871 takes 4e-9 of it)


def corr(a, b):
    """sample correlation times sqrt(N): ~ N(0, 1) for independent streams"""
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)) * math.sqrt(a.size))


def check_distribution(z, what):
    n = z.size
    m = float(z.mean())
    d = z - m
    var = float(np.dot(d, d) / n)
    kurt = float(np.mean(d ** 4) / var ** 2)
    zs = np.sort(z)
    cdf = (0.5 * torch.special.erfc(torch.from_numpy(zs) * (-1.0 / math.sqrt(2.0)))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = float(max(np.max(i / n - cdf), np.max(cdf - (i - 1.0) / n)))
    a = np.abs(z)
    n4, n5 = int(np.count_nonzero(a > 4.0)), int(np.count_nonzero(a > 5.0))
    fig = dict(mean=m * math.sqrt(n), var=(var - 1.0) * math.sqrt(n / 2.0), kurt=(kurt - 3.0) * math.sqrt(n / 24.0),
               ks=ks * math.sqrt(n), tail4=(n4 - n * P4) / math.sqrt(n * P4), tail5=(n5 - n * P5) / math.sqrt(n * P5),
               lag1=corr(z[:-1], z[1:]), lag4=corr(z[:-4], z[4:]), sq_lag1=corr(z[:-1] ** 2, z[1:] ** 2))
    print(f"{what}: N = {n}, kurtosis {kurt:.4f}, |z| > 4: {n4} ({n * P4:.1f} expected), |z| > 5: {n5} ({n * P5:.1f}), "
          f"max |z| {a.max():.4f}; in standard errors: " + ", ".join(f"{k} {v:+.2f}" for k, v in fig.items()))
    assert a.max() <= PR.Z_MAX
    for k, v in fig.items():
        if k == "ks":
            assert 0.0 < v < KS_BAR, (what, k, v)
        else:
            assert abs(v) <= SIGMAS, (what, k, v)
    return fig


def test_distribution_of_the_restated_draws():
    """2^22 blocks (16.7 M draws) of (seed 42, tag 7): moments, Kolmogorov-Smirnov distance, tail counts and the
    correlations between neighbouring tags and seeds, with a draw's neighbour (cos / sin of one pair), with the same slot
    of the next block, and between neighbouring squares -- each within 4.5 standard errors."""
    n = 4 << 22
    z = PR.normals(42, 7, 0, n)
    check_distribution(z, "(42, 7)")
    for what, other in (("tag 7 against tag 8", PR.normals(42, 8, 0, n)), ("seed 42 against 43", PR.normals(43, 7, 0, n))):
        c = corr(z, other)
        print(f"{what}: correlation {c:+.2f} standard errors")
        assert abs(c) <= SIGMAS, (what, c)
    # the four slots one by one: no slot is biased
    for slot in range(4):
        s = z[slot::4]
        assert abs(float(s.mean()) * math.sqrt(s.size)) <= SIGMAS, slot


@pytest.mark.parametrize("seed,tag", [(1234, 0xFFFFFFFF), ((1 << 40) + 17, 3)], ids=["prior_tag", "seed_2^40+17"])
def test_distribution_of_two_more_streams(seed, tag):
    """2^20 blocks each: the prior's reserved tag, and a seed whose high half is not zero"""
    check_distribution(PR.normals(seed, tag, 0, 4 << 20), f"({seed}, {tag:#x})")


def test_uniform_draws_are_uniform():
    u = PR.uniforms(42, PR.TAG_TIMES, 3, 1 << 20).astype(np.float64)
    n = u.size
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs((u.mean() - 0.5) * math.sqrt(12.0 * n)) <= SIGMAS
    us = np.sort(u)
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(np.max(i / n - us), np.max(us - (i - 1.0) / n)) * math.sqrt(n)
    assert ks < KS_BAR, ks


# ------------------------------------------------------------------ 5. the tag plan ----
def test_small_schedules_enumerated():
    """Every update of a run draws under its own tag, the families are the contiguous runs schedule_families states, and
    the per-update functions are the formulas of include/ffd.h."""
    assert PR.tag_predictor(5) == 5 and PR.tag_corrector(5, 1, 3) == 0x80000000 + 16
    assert PR.tag_projection(5, 3, 3) == 0xC0000000 + 23 and PR.tag_transition(2) == 0xE0000002
    assert (PR.TAG_PRIOR, PR.TAG_PERTURB, PR.TAG_TIMES) == (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD)
    for n_steps, n_corr, cond, jump, resample in [(6, 0, False, 1, 1), (6, 2, False, 1, 1), (7, 0, True, 1, 1), (7, 3, True, 1, 1),
                                                  (6, 1, True, 2, 2), (7, 2, True, 3, 3), (5, 0, True, 9, 2), (5, 1, True, 1, 4)]:
        sched = PR.schedule_tags(n_steps, n_corr, cond, jump, resample)
        tags = [t for _, t in sched]
        visits = n_steps * resample
        q = PR.n_transitions(n_steps, jump, resample)
        assert len(sched) == visits * (n_corr + 1) * (2 if cond else 1) + q
        assert len(set(tags)) == len(tags) and not set(tags) & set(PR.RESERVED)
        fam = PR.schedule_families(visits, n_corr, cond, q)
        assert not PR.families_collide(fam)
        want = set()
        for name, first, count in fam[:-1]:
            got = {t for (kind, *_), t in sched if kind == name}
            assert got == set(range(first, first + count)), name
            want |= got
        assert want == set(tags) and fam[-1] == ("reserved", 0xFFFFFFFD, 3)


# (entry, what the limit bounds, limit, families of a schedule of that size)
def _pc(p, split):      # p = n_steps * n_corrector, as n_steps = split, n_corrector = p / split
    return PR.schedule_families(split, p // split, False)


def _cond(p, split):    # p = n_steps * (n_corrector + 1)
    return PR.schedule_families(split, p // split - 1, True)


def _resample(p, split):  # p = visits * (n_corrector + 1); jump = 1: the most transitions a schedule of p visits can have
    visits = split
    return PR.schedule_families(visits, p // split - 1, True, max(visits - 1, 0))


LIMITS = [("pc", PR.LIMIT_PC, _pc), ("cond", PR.LIMIT_COND, _cond), ("resample", PR.LIMIT_RESAMPLE, _resample)]


def _splits(p):
    """(some of) the ways to write p as steps * per-step count with steps an int: 1, p, and the small prime powers in p"""
    out = {1, p} if p < 1 << 31 else {1}
    for f in (2, 3, 5, 7, 16, 256):
        if p % f == 0:
            out |= {f, p // f}
    return sorted(s for s in out if s < 1 << 31)


@pytest.mark.parametrize("entry,limit,families", LIMITS, ids=[e[0] for e in LIMITS])
def test_limits_keep_the_families_apart(entry, limit, families):
    """The largest schedule an entry accepts keeps every family inside its range, however the product is split between
    steps and correctors.  The limits are not loose either: the first size at which two families DO meet -- found from
    the plan, not from the library -- lies within 17 of the limit (the library rounds its bounds down to ...FFF0)."""
    for p in (limit, limit - 1, limit // 2):
        for split in _splits(p):
            assert not PR.families_collide(families(p, split)), (entry, hex(p), split)
    def collides(p):  # under some split: one step (the longest families), a few steps, one update per step
        return any(PR.families_collide(families(p, s)) for s in (1, 2, 3, p) if p % s == 0)

    first = next(p for p in range(limit + 1, limit + 64) if collides(p))
    print(f"{entry}: limit {limit:#x}, first colliding size {first:#x}")
    assert limit < first <= limit + 17
    for p in range(first, first + 8):  # and every size from there on collides
        assert collides(p), hex(p)


def test_what_a_collision_is():
    """families_collide on hand-made cases: a shared tag, a run into the reserved tags, a wrap past 2^32"""
    ok = [("predictor", 0, 10), ("corrector", 0x80000000, 0x40000000), ("projection", 0xC0000000, 5), ("reserved", 0xFFFFFFFD, 3)]
    assert not PR.families_collide(ok)
    assert PR.families_collide(ok[:1] + [("corrector", 0x80000000, 0x40000001)] + ok[2:])
    assert PR.families_collide([("transition", 0xE0000000, 0x1FFFFFFE), ("reserved", 0xFFFFFFFD, 3)])
    assert not PR.families_collide([("transition", 0xE0000000, 0x1FFFFFFD), ("reserved", 0xFFFFFFFD, 3)])
    assert PR.families_collide([("predictor", 0, 4), ("corrector", 0x80000000, 0x80000001)])  # wraps onto tag 0
    # the wrap in the per-update functions themselves
    assert PR.tag_corrector(0x7FFFFFFF, 1, 1) == 0 == PR.tag_predictor(0)
    assert PR.tag_projection(0, 0x3FFFFFFD, 0x3FFFFFFD) == PR.TAG_TIMES
    assert PR.tag_corrector(1, 0, 0x40000000) == PR.tag_projection(0, 0, 0x40000000)
    assert PR.tag_projection(0, 0x20000000, 0x20000000) == PR.tag_transition(0)
