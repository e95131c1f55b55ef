"""The device RNG's stream restated on the host (include/rgan.h rgan_rng_fill / rgan_rng_choice),
in numpy and Python ints: Philox-4x32-10 from its definition, the word-to-output maps of the
uniform and Box-Muller fills, Floyd's sampling with the Fisher-Yates pass, and a stateful mirror
of kernels.DeviceRNG that books the counter interval every call consumes.

Everything up to the last float conversion is integer arithmetic, so uniforms and indices are
reproduced exactly; normals are computed in float64 (the device's logf / sqrtf / sincospif round).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # Weyl key increments
MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1
SEED_MUL, SEED_ADD = 0x9E3779B97F4A7C15, 0x632BE59BD9B4E019  # kernels.DeviceRNG's seed mixing
CHOICE_MAX = 4096
EINVAL = 1001

# Counters of the raw kernel seed EDGE_SEED (what DeviceRNG(0) passes) at which one output word
# has its top 24 bits all 0 ("zero") or all 1 ("one"): (counter, word, extreme), every
# (word, extreme) pair once.  Regenerate with find_edge_counters(EDGE_SEED, 1 << 27).
EDGE_SEED = 0x632BE59BD9B4E019
EDGE_COUNTERS = (
    (3088197, 0, "zero"),
    (15811541, 1, "zero"),
    (30986463, 2, "zero"),
    (2605690, 3, "zero"),
    (9035141, 0, "one"),
    (6590583, 1, "one"),
    (19308597, 2, "one"),
    (35687297, 3, "one"),
)


def _split(x, nwords):
    """Python int(s) -> uint64 array (..., nwords) of 32-bit words, least significant first."""
    if isinstance(x, np.ndarray) and x.dtype != object:
        a = x.astype(np.uint64)
        assert a.shape[-1] == nwords, "a word array needs %d words in its last axis" % nwords
        return a
    flat = np.asarray(x, dtype=object)
    out = np.empty(flat.shape + (nwords,), dtype=np.uint64)
    for idx in np.ndindex(flat.shape):
        v = int(flat[idx])
        assert 0 <= v < 1 << (32 * nwords)
        for w in range(nwords):
            out[idx + (w,)] = (v >> (32 * w)) & MASK32
    return out


def philox4x32_10(counter128, key64):
    """Philox-4x32-10 (Salmon et al., SC'11).  ``counter128``: a Python int, a sequence of them,
    or an integer array (..., 4) of 32-bit words, least significant first; ``key64``: a Python
    int or two words.  Returns the output words as uint32 (..., 4)."""
    c = _split(counter128, 4)
    k = _split(key64, 2)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(k[..., 0]), int(k[..., 1])
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def stream_words(seed, base, count):
    """The project's stream: words of counters base .. base+count-1 (mod 2^64) under the raw
    kernel seed: counter words (ctr lo, ctr hi, 0, 0), key (seed lo, seed hi)."""
    with np.errstate(over="ignore"):
        ctr = np.uint64(base & MASK64) + np.arange(count, dtype=np.uint64)  # wraps mod 2^64
    c = np.zeros((count, 4), dtype=np.uint64)
    c[:, 0] = ctr & np.uint64(MASK32)
    c[:, 1] = ctr >> np.uint64(32)
    return philox4x32_10(c, seed & MASK64)


def quads(n):
    return -(-n // 4)


def fill_uniform(seed, base, n):
    """float32[n]: element 4q+i = (word_i(base+q) >> 8) * 2^-24, in [0, 1 - 2^-24]."""
    w = stream_words(seed, base, quads(n)).reshape(-1)[:n]
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)  # exact: 24 bits


def fill_normal(seed, base, n):
    """(float64[n] normals, float64[n] radius of each element's pair).  With U(w) =
    ((w >> 8) + 1) 2^-24 in (0, 1]: elements 4q, 4q+1 = r0 cos(2 pi U(w1)), r0 sin(2 pi U(w1)),
    r0 = sqrt(-2 ln U(w0)); elements 4q+2, 4q+3 the same from w2 (radius) and w3 (angle)."""
    w = stream_words(seed, base, quads(n))
    U = ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(U[:, 0::2]))  # (quads, 2): from w0, w2
    a = 2.0 * np.pi * U[:, 1::2]  # from w1, w3
    z = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(-1)[:n]  # (q, pair, cos|sin)
    return z, np.repeat(r.reshape(-1), 2)[:n]


def uniform_below(words, m):
    """Integer in [0, m) from one counter's words: (((w1 << 32) | w0) * m) >> 64."""
    return (((int(words[1]) << 32) | int(words[0])) * int(m)) >> 64


def choice(seed, base, N, n):
    """n distinct indices of [0, N) in the order the device returns them: Floyd's algorithm on
    counters base .. base+n-1, then a Fisher-Yates pass on base+n .. base+2n-1."""
    assert 0 < n <= N
    w = stream_words(seed, base, 2 * n)
    picks, taken = [], set()
    for s in range(n):
        j = N - n + s
        t = uniform_below(w[s], j + 1)
        p = j if t in taken else t
        taken.add(p)
        picks.append(p)
    for s in range(n - 1, 0, -1):
        k = uniform_below(w[n + s], s + 1)
        picks[s], picks[k] = picks[k], picks[s]
    return np.array(picks, dtype=np.int64)


def mix_seed(seed):
    """The raw kernel seed kernels.DeviceRNG(seed) passes."""
    return (int(seed) * SEED_MUL + SEED_ADD) & MASK64


class RefRNG:
    """kernels.DeviceRNG on the host: the same seed mixing, a Python-int counter every call
    advances by ceil(n / 4) (fills) or 2 n (choice), and ``intervals``, the [start, end) counter
    range of each call in order."""

    def __init__(self, seed):
        self.seed = mix_seed(seed)
        self.counter = 0
        self.intervals = []

    def _take(self, count):
        base = self.counter
        self.counter = (base + count) & MASK64
        self.intervals.append((base, base + count))
        return base

    def normal(self, shape):
        """(normals, radii), both float64 of ``shape``."""
        n = int(np.prod(shape))
        z, r = fill_normal(self.seed, self._take(quads(n)), n)
        return z.reshape(shape), r.reshape(shape)

    def uniform(self, shape):
        n = int(np.prod(shape))
        return fill_uniform(self.seed, self._take(quads(n)), n).reshape(shape)

    def choice(self, N, n):
        return choice(self.seed, self._take(2 * n), N, n)


def find_edge_counters(seed, limit, chunk=1 << 20):
    """{(word, "zero" | "one"): first counter below ``limit`` at which that word's top 24 bits
    are all 0 / all 1} under the raw kernel seed ``seed`` (the source of EDGE_COUNTERS)."""
    found = {}
    for start in range(0, limit, chunk):
        top = stream_words(seed, start, min(chunk, limit - start)) >> np.uint32(8)
        for name, value in (("zero", 0), ("one", 0xFFFFFF)):
            for q, word in zip(*np.nonzero(top == value)):
                found.setdefault((int(word), name), start + int(q))
        if len(found) == 8:
            break
    return found
