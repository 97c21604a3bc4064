"""Float64 restatement of the on-device noise generator (numpy only): Philox4x32-10, the two fp32 uniforms, the
Box-Muller draws and the stream-tag plan of include/ffd.h.

Written from the Random123 definition of Philox4x32-10 (Salmon et al. 2011: per round, counter words (c0, c1, c2, c3) and
key (k0, k1) become (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) and the key is bumped by the Weyl
constants) and from the contract include/ffd.h states:

  * the draw of GLOBAL element g = (sample_offset + b) L C + i is slot g & 3 of Philox block g >> 2;
  * the block's counter is (lo32(g >> 2), hi32(g >> 2), tag, "FFDF"), its key (lo32(seed), hi32(seed));
  * slots 0, 1 are r cos(2 pi u2), r sin(2 pi u2) of the words (x, y), r = sqrt(-2 ln u1); slots 2, 3 those of (z, w);
  * u = ((w >> 8) + 0.5) 2^-24 EVALUATED IN FP32 (the sum rounds to nearest-even from 2^23 on); the time draws of the
    score-matching loss use u = (w >> 8) 2^-24 in [0, 1), which is exact.

Everything behind the fp32 uniform is float64: this is the exact Box-Muller value of the words, the yardstick the
device's hardware log2 / sqrt / sin / cos are measured against (tests/test_philox_gpu.py).
"""
import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (0xD2511F53, 0xCD9E8D57)  # multipliers of counter words 0 and 2
PHILOX_W = (0x9E3779B9, 0xBB67AE85)  # Weyl increments of the key (golden ratio, sqrt(3) - 1)
DOMAIN_WORD = 0x46464446             # "FFDF": counter word 3 of every block this library draws
Z_MAX = float(np.sqrt(50.0 * np.log(2.0)))  # 5.8871: the smallest u is 2^-25

TAG_PRIOR, TAG_PERTURB, TAG_TIMES = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
TAG_CORRECTOR0, TAG_PROJECTION0, TAG_TRANSITION0 = 0x80000000, 0xC0000000, 0xE0000000
RESERVED = (TAG_TIMES, TAG_PERTURB, TAG_PRIOR)
# the sizes the loop entries accept (include/ffd.h: a larger schedule is FFD_ERR_INVALID before any device work)
LIMIT_PC = 0x7FFFFFF0        # ffd_sample_batch_pc:        n_steps * n_corrector
LIMIT_COND = 0x3FFFFFF0      # ffd_sample_batch_cond:      n_steps * (n_corrector + 1)
LIMIT_RESAMPLE = 0x1FFFFFF0  # ffd_sample_batch_resample:  visits * (n_corrector + 1), visits = n_steps * resample


# ------------------------------------------------------------------ the generator ----
def philox4x32_10(counter4, key2, rounds=10):
    """Philox4x32 on arrays of counters: counter4 = (c0, c1, c2, c3), key2 = (k0, k1), each broadcastable, values below
    2^32.  Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [v & MASK32 for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter4])]
    k = [np.uint64(int(v) & 0xFFFFFFFF) for v in key2]
    m0, m1 = (np.uint64(v) for v in PHILOX_M)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [np.uint64((int(k[0]) + PHILOX_W[0]) & 0xFFFFFFFF), np.uint64((int(k[1]) + PHILOX_W[1]) & 0xFFFFFFFF)]
    return c


def uniform24_half(word):
    """The normal draws' uniform: ((w >> 8) + 0.5) 2^-24 in fp32, in [2^-25, 1] -- returned as float32."""
    top = (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)  # < 2^24: exact
    return (top + np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform24(word):
    """The time draws' uniform (ffd_sm_draw_times): (w >> 8) 2^-24, exact in fp32, in [0, 1) -- returned as float32."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def box_muller(w1, w2):
    """(r cos(2 pi u2), r sin(2 pi u2)) in float64, r = sqrt(-2 ln u1), from two words."""
    u1 = uniform24_half(w1).astype(np.float64)
    u2 = uniform24_half(w2).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def _blocks(seed, tag, first_block, n_blocks):
    """the four words of blocks first_block .. first_block + n_blocks - 1 under (seed, tag); Python ints throughout, so
    any 64-bit block index and seed"""
    seed, tag, first_block = int(seed), int(tag), int(first_block)
    assert 0 <= seed < 1 << 64 and 0 <= tag < 1 << 32 and 0 <= first_block and first_block + n_blocks <= 1 << 62
    q = np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64)
    return philox4x32_10((q & MASK32, q >> np.uint64(32), tag, DOMAIN_WORD), (seed & 0xFFFFFFFF, seed >> 32))


def _span(g0, n):
    g0, n = int(g0), int(n)
    assert g0 >= 0 and n >= 0
    first = g0 >> 2
    return first, (((g0 + n - 1) >> 2) - first + 1 if n else 0), g0 & 3


def normals(seed, tag, g0, n):
    """float64 N(0, 1) draws of global elements g0 .. g0 + n - 1 under (seed, tag)."""
    first, nb, skip = _span(g0, n)
    x, y, z, w = _blocks(seed, tag, first, nb)
    out = np.empty((nb, 4), np.float64)
    out[:, 0], out[:, 1] = box_muller(x, y)
    out[:, 2], out[:, 3] = box_muller(z, w)
    return out.reshape(-1)[skip:skip + int(n)]


def uniforms(seed, tag, g0, n):
    """float32 U[0, 1) draws (uniform24) of global elements g0 .. g0 + n - 1 under (seed, tag): one word each."""
    first, nb, skip = _span(g0, n)
    return uniform24(np.stack(_blocks(seed, tag, first, nb), axis=1).reshape(-1))[skip:skip + int(n)]


def sample_normals(seed, tag, sample_offset, shape):
    """the draws of a (B, L, C) call at `sample_offset`: element i of sample b is global element (sample_offset + b) L C + i"""
    B, L, Cn = shape
    return normals(seed, tag, int(sample_offset) * L * Cn, B * L * Cn).reshape(shape)


# ------------------------------------------------------------------ the tag plan ----
# Tags are 32-bit: the library forms them in uint32 arithmetic, so a schedule too large for its range WRAPS.
def tag_predictor(u):
    """the Euler-Maruyama predictor of reverse step (resampling: visit) u"""
    return int(u) & 0xFFFFFFFF


def tag_corrector(u, k, n_corrector):
    """Langevin corrector k of step / visit u"""
    return (TAG_CORRECTOR0 + int(u) * int(n_corrector) + int(k)) & 0xFFFFFFFF


def tag_projection(u, k, n_corrector):
    """the projection behind update k (k = n_corrector: the predictor's) of step / visit u"""
    return (TAG_PROJECTION0 + int(u) * (int(n_corrector) + 1) + int(k)) & 0xFFFFFFFF


def tag_transition(q):
    """forward transition q of a resampled run, in schedule order"""
    return (TAG_TRANSITION0 + int(q)) & 0xFFFFFFFF


def n_transitions(n_steps, jump, resample):
    return (resample - 1) * -(-n_steps // jump)


def schedule_families(visits, n_corrector, cond=False, transitions=0):
    """The tag families of a loop run of `visits` steps / visits as (name, first tag, count) WITHOUT wrapping: each
    family's tags are the contiguous run first .. first + count - 1 (u n + k walks 0 .. visits n - 1 once), so a
    schedule of any size can be judged without enumerating it.  The three reserved tags come last."""
    fam = [("predictor", 0, visits), ("corrector", TAG_CORRECTOR0, visits * n_corrector)]
    if cond:
        fam.append(("projection", TAG_PROJECTION0, visits * (n_corrector + 1)))
    if transitions:
        fam.append(("transition", TAG_TRANSITION0, transitions))
    return [f for f in fam if f[2] > 0] + [("reserved", TAG_TIMES, 3)]


def families_collide(families):
    """True if two families share a tag or one runs past 2^32 (and wraps onto the predictor's)."""
    spans = sorted((first, first + count) for _, first, count in families)
    return spans[-1][1] > 1 << 32 or any(a[1] > b[0] for a, b in zip(spans[:-1], spans[1:]))


def schedule_tags(n_steps, n_corrector, cond=False, jump=1, resample=1):
    """every (update, tag) of a whole run in execution order, by the per-update functions above (small schedules)"""
    out, q = [], 0
    for u in range(n_steps * resample):
        for k in range(n_corrector + 1):
            predictor = k == n_corrector
            out.append((("predictor", u) if predictor else ("corrector", u, k),
                        tag_predictor(u) if predictor else tag_corrector(u, k, n_corrector)))
            if cond:
                out.append((("projection", u, k), tag_projection(u, k, n_corrector)))
        if resample > 1 and visit_is_followed(n_steps, jump, resample, u):
            out.append((("transition", q), tag_transition(q)))
            q += 1
    return out


def visit_is_followed(n_steps, jump, resample, visit):
    """ffd.h's schedule: the grid is cut into blocks of `jump` steps, each run `resample` times; a forward transition
    follows the last step of every pass of a block but the last pass."""
    per = jump * resample
    n_blocks = -(-n_steps // jump)
    k = min(visit // per, n_blocks - 1)
    i0 = k * jump
    length = min(jump, n_steps - i0)
    w = visit - k * per
    return w % length == length - 1 and w // length < resample - 1
