"""The host restatement of the device RNG (tests/rng_ref.py) is itself right: Philox-4x32-10
against the Random123 known answers, the integer scaling at its extremes, the sampling
algorithm's invariants, the counter bookkeeping, and the table of edge counters."""
import numpy as np
import pytest

from tests import rng_ref as R

# Random123 kat_vectors, philox4x32 10: (counter words, key words) -> output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _join(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(_join(ctr), _join(key))
    assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    # the same through a word array, vectorised with a second counter beside it
    both = R.philox4x32_10(np.array([ctr, KAT[0][0]], dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert tuple(int(x) for x in both[0]) == want
    assert tuple(int(x) for x in both[1]) == tuple(int(x) for x in R.philox4x32_10(0, _join(key)))


def test_stream_words_layout():
    """Counter words (ctr lo, ctr hi, 0, 0), key (seed lo, seed hi), counters wrapping mod 2^64."""
    seed, base = 0x0123456789ABCDEF, (1 << 64) - 2
    w = R.stream_words(seed, base, 4)
    for q in range(4):
        assert np.array_equal(w[q], R.philox4x32_10((base + q) & R.MASK64, seed))
    hi = R.stream_words(seed, (1 << 32) - 1, 2)  # the high counter word changes between the two
    assert np.array_equal(hi[1], R.philox4x32_10(np.array([0, 1, 0, 0], dtype=np.uint32), seed))


@pytest.mark.parametrize("m", [1, 2, 3, 2 ** 31 - 1])
def test_uniform_below_extremes(m):
    assert R.uniform_below((0, 0, 0xffffffff, 0xffffffff), m) == 0  # only words 0 and 1 count
    assert R.uniform_below((0xffffffff, 0xffffffff, 0, 0), m) == m - 1
    assert R.uniform_below((0, 0x80000000, 0, 0), m) == m // 2  # word 1 is the high half


def test_fill_maps():
    """Uniform element 4q+i comes from word i of counter base+q; the normal pairs take radius
    from words 0 / 2 and angle from words 1 / 3, cos first; tails are prefixes."""
    seed, base = R.mix_seed(3), 77
    w = R.stream_words(seed, base, 3)
    u = R.fill_uniform(seed, base, 11)
    assert u.dtype == np.float32 and u.shape == (11,)
    for e in range(11):
        assert float(u[e]) == (int(w[e // 4, e % 4]) >> 8) / 2.0 ** 24
    z, r = R.fill_normal(seed, base, 11)
    assert z.dtype == np.float64 and z.shape == r.shape == (11,)
    U = lambda x: ((int(x) >> 8) + 1) / 2.0 ** 24  # noqa: E731
    for e in range(11):
        q, i = divmod(e, 4)
        rad = np.sqrt(-2 * np.log(U(w[q, i & 2])))
        ang = 2 * np.pi * U(w[q, (i & 2) + 1])
        assert r[e] == rad and z[e] == pytest.approx(rad * (np.sin(ang) if i & 1 else np.cos(ang)), abs=1e-14)
    assert np.array_equal(R.fill_uniform(seed, base, 9), u[:9])
    assert np.array_equal(R.fill_normal(seed, base, 9)[0], z[:9])


@pytest.mark.parametrize("N,n", [(1, 1), (5, 5), (64, 64), (300, 300), (1000, 64), (5000, 300), (2 ** 31 - 1, 65)])
def test_choice_distinct_in_range(N, n):
    got = R.choice(R.mix_seed(1), 123, N, n)
    assert got.dtype == np.int64 and got.shape == (n,)
    if N == n:
        assert sorted(got.tolist()) == list(range(N))
    else:
        assert len(set(got.tolist())) == n and got.min() >= 0 and got.max() < N


def test_choice_is_floyd_then_fisher_yates():
    """Spelled out by hand at a size where collisions are certain (N = n = 6)."""
    seed, base, N = R.mix_seed(5), 9, 6
    w = R.stream_words(seed, base, 2 * N)
    picks = []
    for s in range(N):
        t = R.uniform_below(w[s], s + 1)  # j = N - n + s = s
        picks.append(s if t in picks else t)
    assert sorted(picks) == list(range(N))
    for s in range(N - 1, 0, -1):
        k = R.uniform_below(w[N + s], s + 1)
        picks[s], picks[k] = picks[k], picks[s]
    assert R.choice(seed, base, N, N).tolist() == picks


def test_refrng_intervals():
    """An interleaved sequence consumes pairwise disjoint, contiguous counter intervals of
    ceil(n / 4) (fills) and 2 n (choice), and each call equals the stateless draw at its base."""
    g = R.RefRNG(11)
    assert g.seed == (11 * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) % 2 ** 64
    assert R.RefRNG(0).seed == R.EDGE_SEED
    z0, _ = g.normal((3, 7))
    idx = g.choice(100, 9)
    u = g.uniform((5,))
    z1, r1 = g.normal((2, 1, 3))
    assert g.intervals == [(0, 6), (6, 24), (24, 26), (26, 28)] and g.counter == 28
    for (a0, a1), (b0, b1) in zip(g.intervals, g.intervals[1:]):
        assert a0 < a1 == b0 < b1
    assert z0.shape == (3, 7) and z1.shape == r1.shape == (2, 1, 3)
    assert np.array_equal(z0.reshape(-1), R.fill_normal(g.seed, 0, 21)[0])
    assert np.array_equal(idx, R.choice(g.seed, 6, 100, 9))
    assert np.array_equal(u, R.fill_uniform(g.seed, 24, 5))
    assert np.array_equal(z1.reshape(-1), R.fill_normal(g.seed, 26, 6)[0])


def test_edge_counters():
    """Every (word, extreme) pair is in the table, and each entry's word has its top 24 bits
    all 0 / all 1: the uniform there is exactly 0 / 1 - 2^-24 and the Box-Muller U 2^-24 / 1."""
    assert sorted((w, e) for _, w, e in R.EDGE_COUNTERS) == sorted((w, e) for w in range(4) for e in ("zero", "one"))
    for ctr, word, extreme in R.EDGE_COUNTERS:
        w = int(R.stream_words(R.EDGE_SEED, ctr, 1)[0, word])
        assert w >> 8 == (0 if extreme == "zero" else 0xFFFFFF), (ctr, word, extreme, hex(w))
        u = R.fill_uniform(R.EDGE_SEED, ctr, 4)
        assert float(u[word]) == (0.0 if extreme == "zero" else 1.0 - 2.0 ** -24) and float(u.max()) < 1.0
        z, r = R.fill_normal(R.EDGE_SEED, ctr, 4)
        assert np.isfinite(z).all()
        if word in (0, 2):
            assert r[word] == pytest.approx(np.sqrt(48 * np.log(2)) if extreme == "zero" else 0.0, rel=1e-15, abs=0)
