"""--rgan_rng device on the MI355X against a host replay of its stream (tests/rng_ref.py):
rng_fill, rng_choice_small and rng_choice (csrc/sampling.hip) reproduce the reference's
uniforms and indices bit for bit and its normals within a rounding budget, at the tail sizes,
the one-block / multi-block / grid-stride switches, the register / LDS switch of the choice
kernels, the two 24-bit extremes of every output word, across interleaved calls and graph
replays, and the device counter moves by exactly what each call consumed.

Every output is written through the raw entry points into a buffer with PAD extra elements
holding a sentinel (NaN / -1) that must survive.

Normal bound: |dev - ref| <= K_BUDGET 2^-24 max(r, 1), r the pair's radius.  The device computes
fl(sqrtf(fl(-2 logf(U))) * cos|sin pi(fl(2 U))), the reference the same in float64 from the same
U (exact in both).  No accuracy figures for the device library's logf / sqrtf / sincospif ship
with the toolchain, so each is allowed 4 ulp, and the two fp32 multiplies that can round (the
-2 x and the final r x trig; 2 U is exact) 0.5 ulp each: 4 + 4 + 4 + 0.5 + 0.5 = 13 ulp, each
relative to a factor of the output, so they add to first order.  One ulp of an fp32 value v is at
most 2^-23 |v| = 2 x 2^-24 |v| and |output| <= r, hence K_BUDGET = 26.  (The square root halves
the logarithm's share; the budget does not take credit for that.)  The errors guarded against
are of order 1: a swapped word, sin for cos, a stream shifted by one quad.
"""
import math

import numpy as np
import pytest
import torch

from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 8
K_BUDGET = 26.0
ULP24 = 2.0 ** -24

# 16384: the last one-block size, 16385 the first multi-block one; 2_097_152 + 5 is past
# 2048 blocks x 256 threads x 4, so the grid-stride loop runs twice
FILL_SIZES = [1, 2, 3, 4, 5, 1023, 16384, 16385, 2_097_152 + 5]
CHOICE_CASES = [(1, 1), (5, 5), (64, 64), (65, 65), (1000, 64), (1000, 65), (4096, 4096), (5000, 300),
                (2 ** 31 - 1, 1), (2 ** 31 - 1, 64), (2 ** 31 - 1, 65)]


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def L():
    from relativisticgan_amd import _lib
    return _lib


def _fill_cases():
    """(n, seed, base): seed 0 at a plain base, seed 7 placed so that the counter's high word
    changes inside the call (or, for one quad, in its advance)."""
    for n in FILL_SIZES:
        yield n, 0, 12345
        yield n, 7, (1 << 32) - (R.quads(n) + 1) // 2


class Raw:
    """kernels.DeviceRNG's three draws through the raw entry points into padded buffers."""

    def __init__(self, K, L, seed, base=0):
        self.L, self.rng = L, K.DeviceRNG(seed, DEV)
        self.rng.counter.fill_(base)
        self.bufs = []

    @property
    def counter(self):
        return int(self.rng.counter.item())

    def fill(self, n, kind, check=True):
        buf = torch.full((n + PAD,), math.nan, dtype=torch.float32, device=DEV)
        rc = self.L.lib().rgan_rng_fill(self.L.ptr(buf), n, kind, self.rng.seed, self.L.ptr(self.rng.counter),
                                        self.L.stream())
        return self._done(rc, buf, n, check)

    def normal(self, shape):
        return self.fill(math.prod(shape), 0).view(shape)

    def uniform(self, shape):
        return self.fill(math.prod(shape), 1).view(shape)

    def choice(self, N, n, check=True):
        buf = torch.full((max(n, 0) + PAD,), -1, dtype=torch.int64, device=DEV)
        rc = self.L.lib().rgan_rng_choice(self.L.ptr(buf), N, n, self.rng.seed, self.L.ptr(self.rng.counter),
                                          self.L.stream())
        return self._done(rc, buf, max(n, 0), check)

    def _done(self, rc, buf, n, check):
        self.bufs.append((buf, n))
        if not check:
            return rc, buf
        assert rc == 0
        return buf[:n]

    def assert_sentinels(self):
        for buf, n in self.bufs:
            tail = buf[n:]
            assert tail.numel() == PAD
            assert bool(torch.isnan(tail).all() if buf.is_floating_point() else (tail == -1).all()), (n, tail)


def _normal_err(dev, z, r):
    """max |dev - ref| / (2^-24 max(r, 1)) over the elements: passes at <= K_BUDGET."""
    d = dev.detach().cpu().double().numpy().reshape(-1)
    assert np.isfinite(d).all()
    return float((np.abs(d - z.reshape(-1)) / (ULP24 * np.maximum(r.reshape(-1), 1.0))).max())


@pytest.mark.parametrize("n,seed,base", list(_fill_cases()))
def test_uniform_bits(K, L, n, seed, base):
    g = Raw(K, L, seed, base)
    u = g.uniform((n,))
    assert g.counter == base + R.quads(n)
    want = R.fill_uniform(R.mix_seed(seed), base, n)
    assert torch.equal(u.cpu(), torch.from_numpy(want))
    assert float(u.max()) < 1.0 and float(u.min()) >= 0.0
    g.assert_sentinels()


@pytest.mark.parametrize("n,seed,base", list(_fill_cases()))
def test_normal_within_rounding(K, L, n, seed, base):
    g = Raw(K, L, seed, base)
    dev = g.normal((n,))
    assert g.counter == base + R.quads(n)
    z, r = R.fill_normal(R.mix_seed(seed), base, n)
    worst = _normal_err(dev, z, r)
    print(f"rng normal n={n} seed={seed} base={base}: worst |dev - ref| / (2^-24 max(r, 1)) = {worst:.3f}")
    assert worst <= K_BUDGET
    g.assert_sentinels()


@pytest.mark.parametrize("ctr,word,extreme", R.EDGE_COUNTERS)
def test_word_extremes(K, L, ctr, word, extreme):
    """The quad at a counter where one word's top 24 bits are all 0 / all 1."""
    g = Raw(K, L, 0, ctr)
    assert g.rng.seed == R.EDGE_SEED
    u = g.uniform((4,)).cpu()
    assert torch.equal(u, torch.from_numpy(R.fill_uniform(R.EDGE_SEED, ctr, 4)))
    assert float(u[word]) == (0.0 if extreme == "zero" else 1.0 - ULP24)
    assert float(u.max()) < 1.0  # never 1.0
    g.rng.counter.fill_(ctr)
    dev = g.normal((4,))
    z, r = R.fill_normal(R.EDGE_SEED, ctr, 4)
    d = dev.cpu().double().numpy()
    assert np.isfinite(d).all()
    worst = _normal_err(dev, z, r)
    print(f"rng edge ctr={ctr} word={word} {extreme}: worst = {worst:.3f}, normals {d.tolist()}")
    assert worst <= K_BUDGET
    pair = d[word & 2:(word & 2) + 2]
    if word in (0, 2) and extreme == "one":  # U = 1: log 0 -> radius 0
        assert pair[0] == 0.0 and pair[1] == 0.0
    if word in (0, 2) and extreme == "zero":  # U = 2^-24: the largest radius
        # every rounding above is relative to the radius or to cos / sin, so the pair's error
        # vector has norm <= K_BUDGET 2^-24 r (cos^2 + sin^2 = 1), and so has its length's error
        rmax = math.sqrt(48 * math.log(2))
        assert r[word] == pytest.approx(rmax, rel=1e-15)
        assert abs(math.hypot(pair[0], pair[1]) - rmax) <= K_BUDGET * ULP24 * rmax
    if word in (1, 3) and extreme == "one":  # sincospif(2): the sin output
        assert abs(d[word]) <= K_BUDGET * ULP24 * max(r[word], 1.0)
    g.assert_sentinels()


@pytest.mark.parametrize("N,n", CHOICE_CASES)
def test_choice_bits(K, L, N, n):
    """N = n makes collisions the common case; 64 / 65 straddle the register and LDS kernels;
    4096 fills the LDS arrays; N = 2^31 - 1 is the largest int."""
    for seed, base in ((0, 4321), (7, (1 << 32) - n)):
        g = Raw(K, L, seed, base)
        idx = g.choice(N, n)
        assert g.counter == base + 2 * n
        assert torch.equal(idx.cpu(), torch.from_numpy(R.choice(R.mix_seed(seed), base, N, n)))
        g.assert_sentinels()


def test_no_draw_where_none_is_due(K, L):
    g = Raw(K, L, 3, 99)
    for rc, buf in (g.fill(0, 0, check=False), g.fill(0, 1, check=False), g.choice(10, 0, check=False)):
        assert rc == 0
    for rc, buf in (g.choice(5, 6, check=False), g.choice(10000, 4097, check=False), g.choice(0, 0, check=False),
                    g.choice(-5, 0, check=False), g.choice(0, 1, check=False), g.fill(4, 2, check=False),
                    g.fill(4, -1, check=False)):
        assert rc == R.EINVAL == 1001
    torch.cuda.synchronize()
    assert g.counter == 99
    for buf, _ in g.bufs:  # nothing was written anywhere, not only past the end
        assert bool(torch.isnan(buf).all() if buf.is_floating_point() else (buf == -1).all())


def test_interleaved_calls(K, L):
    g, ref = Raw(K, L, 11), R.RefRNG(11)
    assert g.rng.seed == ref.seed
    calls = [("normal", (32, 128)), ("choice", (1000, 32)), ("uniform", (32, 1, 1, 1)), ("normal", (20000,)),
             ("choice", (5000, 300)), ("uniform", (5,))]
    for what, arg in calls:
        if what == "normal":
            dev, (z, r) = g.normal(arg), ref.normal(arg)
            assert tuple(dev.shape) == z.shape and _normal_err(dev, z, r) <= K_BUDGET
        elif what == "uniform":
            assert torch.equal(g.uniform(arg).cpu(), torch.from_numpy(ref.uniform(arg)))
        else:
            assert torch.equal(g.choice(*arg).cpu(), torch.from_numpy(ref.choice(*arg)))
        assert g.counter == ref.counter, (what, arg)
    assert ref.intervals == [(0, 1024), (1024, 1088), (1088, 1096), (1096, 6096), (6096, 6696), (6696, 6698)]
    g.assert_sentinels()


def test_graph_replay(K, L):
    """One captured normal / uniform / choice triple: replay k equals the reference's k-th
    repetition from the counter the first replay started at."""
    g = Raw(K, L, 5, 1000)

    def triple():
        return g.normal((16,)), g.uniform((7,)), g.choice(100, 8)

    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        triple()  # warm-up: moves the counter before the capture
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            z, u, idx = triple()
    torch.cuda.current_stream().wait_stream(s)
    start = g.counter
    ref = R.RefRNG(5)
    ref.counter = start
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        zr, rr = ref.normal((16,))
        assert _normal_err(z, zr, rr) <= K_BUDGET, k
        assert torch.equal(u.cpu(), torch.from_numpy(ref.uniform((7,)))), k
        assert torch.equal(idx.cpu(), torch.from_numpy(ref.choice(100, 8))), k
        assert g.counter == ref.counter == start + (k + 1) * (4 + 2 + 16)
    assert g.counter == start + 3 * (4 + 2 + 16)
    g.assert_sentinels()
