"""One plain float64 statement of train-mode BatchNorm2d + activation, first order: moments,
statistics, running statistics, the rank merge of SyncBN, the forward, the backward of one and of
two batch segments, the activation backward from the activation's output, the small ops beside
them, and the seeded inputs the first-order BatchNorm kernel tests run on.

Nothing here goes through relativisticgan_amd and nothing uses autograd: every function is the
formula itself on float64 CPU tensors.  Activations are NHWC on the device, so every tensor here is
its [P][C] matrix (P = B*H*W pixel rows, C channels) and every per-channel quantity a [C] vector.
tests/test_bn_ref_cpu.py pins these formulas to float64 F.batch_norm + torch.autograd.grad and
proves the condition every generator states (no element within KINK of a ReLU / LeakyReLU kink),
so the GPU tests compare every element and mask none.
"""
import math

import torch

ACTS = ("none", "relu", "lrelu", "tanh", "sigmoid", "selu")   # relativisticgan_amd._lib.ACT, in order
PIECEWISE = ("none", "relu", "lrelu")                         # act' is piecewise constant
EPS = 1e-5
ALPHA = 0.2
KINK = 1e-3               # no |z| below this in any generated input (z = gamma * xhat + beta)
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
U = 2.0 ** -24            # fp32 unit roundoff


# ------------------------------------------------------------------ activations
def act(z, name, alpha=ALPHA):
    if name == "none":
        return z
    if name == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if name == "lrelu":
        return torch.where(z > 0, z, alpha * z)
    if name == "tanh":
        return torch.tanh(z)
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-z))
    if name == "selu":
        return torch.where(z > 0, SELU_SCALE * z, SELU_SCALE * SELU_ALPHA * torch.expm1(z))
    raise ValueError(name)


def act_grad(z, name, alpha=ALPHA):
    """act'(z) from the activation's INPUT; at 0 torch's convention: ReLU'(0) = 0, LeakyReLU'(0) = alpha."""
    one = torch.ones_like(z)
    if name == "none":
        return one
    if name == "relu":
        return torch.where(z > 0, one, 0 * one)
    if name == "lrelu":
        return torch.where(z > 0, one, alpha * one)
    if name == "tanh":
        return 1.0 - torch.tanh(z) ** 2
    if name == "sigmoid":
        s = 1.0 / (1.0 + torch.exp(-z))
        return s * (1.0 - s)
    if name == "selu":
        return torch.where(z > 0, SELU_SCALE * one, SELU_SCALE * SELU_ALPHA * torch.exp(z))
    raise ValueError(name)


def act_grad_from_out(a, name, alpha=ALPHA):
    """act'(x) from the activation's OUTPUT a = act(x) (alpha > 0 keeps LeakyReLU's sign); an output
    of exactly 0 is the x <= 0 branch, as in torch's threshold / leaky_relu / elu backward."""
    one = torch.ones_like(a)
    if name == "none":
        return one
    if name == "relu":
        return torch.where(a > 0, one, 0 * one)
    if name == "lrelu":
        return torch.where(a > 0, one, alpha * one)
    if name == "tanh":
        return 1.0 - a * a
    if name == "sigmoid":
        return a * (1.0 - a)
    if name == "selu":
        return torch.where(a > 0, SELU_SCALE * one, a + SELU_SCALE * SELU_ALPHA)
    raise ValueError(name)


def act_lipschitz(name, alpha=ALPHA):
    """sup |act'|."""
    return {"none": 1.0, "relu": 1.0, "lrelu": max(1.0, abs(alpha)), "tanh": 1.0, "sigmoid": 0.25,
            "selu": SELU_SCALE * SELU_ALPHA}[name]


def act_curvature(name):
    """sup |act''| away from the kinks (0 for the piecewise-linear activations)."""
    return {"none": 0.0, "relu": 0.0, "lrelu": 0.0, "tanh": 4.0 / (3.0 * math.sqrt(3.0)),
            "sigmoid": 1.0 / (6.0 * math.sqrt(3.0)), "selu": SELU_SCALE * SELU_ALPHA}[name]


def act_backward(da, a, name, alpha=ALPHA, add=None):
    """dx = da * act'(x) (+ add), act' from the activation output a."""
    dx = da.double() * act_grad_from_out(a.double(), name, alpha)
    return dx if add is None else dx + add.double()


# ------------------------------------------------------------------ moments, statistics
def moments(y):
    """(n, mean[C], M2[C]) of y[P][C]: M2 = sum (y - mean)^2."""
    y = y.double()
    mean = y.mean(0)
    return y.shape[0], mean, ((y - mean) ** 2).sum(0)


def stats_of(n, mean, M2, eps=EPS):
    """(mean, 1 / sqrt(var + eps)) with the biased variance M2 / n."""
    return mean, 1.0 / torch.sqrt(M2 / n + eps)


def stats(y, eps=EPS):
    return stats_of(*moments(y), eps)


def merge(shards):
    """Pooled (n, mean, M2) of shards [(n_k, mean_k, M2_k)]; a shard of count 0 adds nothing
    (its mean and M2 are ignored, whatever they hold)."""
    live = [(n, m.double(), s.double()) for n, m, s in shards if n > 0]
    N = sum(n for n, _, _ in live)
    mean = sum(n * m for n, m, _ in live) / N
    M2 = sum(s + n * (m - mean) ** 2 for n, m, s in live)
    return N, mean, M2


def running_update(rm, rv, nbt, n, mean, M2, momentum, dtype=torch.float32):
    """The running-statistics update as the kernels state it, in fp32: r = (1 - m) * r + m * x with
    x = (float)mean and the unbiased (float)(M2 / (n - 1)), the biased value when n == 1;
    num_batches_tracked + 1.  A buffer that is None stays None; mean / M2 float64.  ``dtype``
    float64 is the same formula without the roundings (test_bn_ref_cpu.py holds it to
    torch.nn.BatchNorm2d)."""
    m = torch.tensor(momentum, dtype=dtype)
    unb = (M2 / (n - 1) if n > 1 else M2 / n).to(dtype)
    rm2 = None if rm is None else (1 - m) * rm.to(dtype) + m * mean.to(dtype)
    rv2 = None if rv is None else (1 - m) * rv.to(dtype) + m * unb
    return rm2, rv2, (None if nbt is None else nbt + 1)


# ------------------------------------------------------------------ forward
def _vec(v, like, fill):
    return torch.full_like(like, fill) if v is None else v.double()


def pre_act(y, mean, invstd, gamma=None, beta=None):
    """z = gamma * xhat + beta, xhat = (y - mean) * invstd; gamma / beta absent = 1 / 0."""
    mean, invstd = mean.double(), invstd.double()
    return _vec(gamma, mean, 1.0) * ((y.double() - mean) * invstd) + _vec(beta, mean, 0.0)


def forward(y, mean, invstd, gamma=None, beta=None, name="none", alpha=ALPHA):
    return act(pre_act(y, mean, invstd, gamma, beta), name, alpha)


def affine_error_bound(y, mean, invstd, gamma=None, beta=None):
    """The a-priori fp32 error of z evaluated as y * al + be, al = gamma * invstd, be = beta -
    mean * al (the kernels' fused form): 4 u (|y al| + |mean al| + |beta|) per element.  It is
    the price of |mean| >> std, where y al and mean al cancel."""
    mean = mean.double()
    al = _vec(gamma, mean, 1.0) * invstd.double()
    return 4 * U * ((y.double() * al).abs() + (mean * al).abs() + _vec(beta, mean, 0.0).abs())


def conditioning(mean, invstd):
    """|mean| / sqrt(var + eps) per channel: how many standard deviations the channel lies from 0."""
    return mean.double().abs() * invstd.double()


# ------------------------------------------------------------------ backward
def backward(da, y, mean, invstd, gamma=None, beta=None, name="none", alpha=ALPHA, P_global=None, add=None,
             sums=None):
    """One batch segment.  g = da * act'(z); sums = (sum g, sum g (y - mean)) [2][C] over THESE rows
    unless given (the all-reduced sums of a data-parallel run);
    dy = gamma * invstd * (g - sum_g / Pg - (y - mean) * invstd^2 * sum_gx / Pg) + add, Pg = P_global
    (>= P, default P); dgamma = invstd * sum_gx and dbeta = sum_g of THESE rows' sums.
    -> dict(g, sums, dy, dgamma, dbeta)."""
    da, y, mean, invstd = da.double(), y.double(), mean.double(), invstd.double()
    g = da * act_grad(pre_act(y, mean, invstd, gamma, beta), name, alpha)
    local = torch.stack([g.sum(0), (g * (y - mean)).sum(0)])
    s = local if sums is None else sums.double().view(2, -1)
    Pg = y.shape[0] if P_global is None else P_global
    dy = _vec(gamma, mean, 1.0) * invstd * (g - s[0] / Pg - (y - mean) * invstd ** 2 * s[1] / Pg)
    if add is not None:
        dy = dy + add.double()
    return dict(g=g, sums=local, dy=dy, dgamma=invstd * local[1], dbeta=local[0])


def backward_segments(da, y, seg_stats, gamma=None, beta=None, name="none", alpha=ALPHA):
    """nseg = len(seg_stats) equal row ranges of y, each with its own (mean, invstd): dy row range
    by row range, the affine gradients summed over the segments.  -> dict(dy, dgamma, dbeta, sums)."""
    nseg = len(seg_stats)
    Ps = y.shape[0] // nseg
    parts = [backward(da[k * Ps:(k + 1) * Ps], y[k * Ps:(k + 1) * Ps], seg_stats[k][0], seg_stats[k][1], gamma, beta,
                      name, alpha) for k in range(nseg)]
    return dict(dy=torch.cat([p["dy"] for p in parts]), dgamma=sum(p["dgamma"] for p in parts),
                dbeta=sum(p["dbeta"] for p in parts), sums=torch.stack([p["sums"] for p in parts]))


# ------------------------------------------------------------------ small ops
def channel_sum(t):
    return t.double().sum(0)


def scale(t, s):
    return t.double() * float(s)


def segment_sums(y, seg_rows=64):
    """The [S][2][C] double segment sums a conv epilogue hands to the segment kernels
    (include/rgan.h, rgan_conv_fwd_bn): segment s = rows [s * seg_rows, (s + 1) * seg_rows) of
    y[P][C], entry 0 = sum y, entry 1 = sum y^2.  P must be a multiple of seg_rows."""
    P, C = y.shape
    assert P % seg_rows == 0
    y3 = y.double().view(P // seg_rows, seg_rows, C)
    return torch.stack([y3.sum(1), (y3 * y3).sum(1)], 1).contiguous()


# ------------------------------------------------------------------ inputs
# Input regimes; one tensor mixes them by channel (kind of channel c = kinds[c % len(kinds)]).
#   a   randn * 3 + 1.5
#   b0  a constant channel, 0               b1  a constant channel, 2.5
#   c   mean 1e3, std 1
#   d0  std 1e-4 around 0 (var << eps)      d1  std 1e-4 around 0.7
#   e   as a, with row 0 (the shift of the kernels' shifted sums) set 50 standard deviations out
#   f   randn * 1e4
# WELL: |mean| is at most a few sqrt(var + eps); OFFSET: |mean| >> sqrt(var + eps), where the fused
# affine form y * al + be cancels (affine_error_bound).
WELL = ("a", "b0", "d0", "e", "f")
OFFSET = ("b1", "c", "d1")
COND_MAX = 8.0   # a channel with conditioning() above this is held to the a-priori bound as well


def channel(kind, P, g):
    r = torch.randn(P, generator=g)
    if kind == "a":
        return r * 3 + 1.5
    if kind == "b0":
        return torch.zeros(P)
    if kind == "b1":
        return torch.full((P,), 2.5)
    if kind == "c":
        return r + 1e3
    if kind == "d0":
        return r * 1e-4
    if kind == "d1":
        return r * 1e-4 + 0.7
    if kind == "e":
        v = r * 3 + 1.5
        v[0] = 1.5 + 150.0 * (1 if r[0] >= 0 else -1)
        return v
    if kind == "f":
        return r * 1e4
    raise ValueError(kind)


def mixes(C, only=None):
    """[(label, kinds per channel)]: every regime of WELL and of OFFSET in some channel, in as few
    tensors as C allows (regimes cycle over the channels; a narrow tensor is rotated).  ``only``:
    the regimes to keep."""
    out = []
    for label, kinds in (("well", WELL), ("offset", OFFSET)):
        if only is not None:
            kinds = tuple(k for k in kinds if k in only)
        for rot in range(0, len(kinds), max(1, min(C, len(kinds)))):
            out.append((f"{label}{rot}", [kinds[(c + rot) % len(kinds)] for c in range(C)]))
    return out


def affine(C, g):
    """gamma in +-[0.5, 1.5], |beta| in [0.05, 1.05]: a constant channel's z = beta stays off the kink."""
    sg = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    gamma = (torch.rand(C, generator=g) + 0.5) * sg
    sb = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta = (torch.rand(C, generator=g) + 0.05) * sb
    return gamma, beta


def off_kink(y, gamma=None, beta=None, eps=EPS, nseg=1):
    """y[P][C] (fp32) with every |z| >= max(KINK, twice affine_error_bound), z = gamma * xhat +
    beta in float64 with the batch statistics of each of y's nseg equal row ranges: elements
    nearer move 0.05 sqrt(var + eps) in y, away from zero (|gamma| >= 0.5 moves z by >= 0.025), at
    most twenty rounds (assert_off_kink states the result, and bwd_inputs asserts it): fp32 rounding
    of z cannot flip a branch of ReLU' / LeakyReLU' then.  (tests/test_kernels_gpu.py
    _bn_off_kink with the step in units of the channel's spread.)  A constant channel is never
    moved: its z is beta, and |beta| >= 0.05."""
    Ps = y.shape[0] // nseg
    out = []
    for k in range(nseg):
        y64 = y[k * Ps:(k + 1) * Ps].double()
        gm = _vec(gamma, y64[0], 1.0)
        for _ in range(20):
            mean, inv = stats(y64, eps)
            z = pre_act(y64, mean, inv, gamma, beta)
            # twice the margins asserted: a move shifts the statistics, and with them every other z, a little
            near = z.abs() < torch.clamp(2 * affine_error_bound(y64, mean, inv, gamma, beta), min=2 * KINK)
            near &= (y64 != y64[0]).any(0)   # not a constant channel
            if not bool(near.any()):
                break
            away = torch.where(z < 0, -1.0, 1.0) * torch.sign(gm)
            y64 = torch.where(near, y64 + 0.05 / inv * away, y64).float().double()
        out.append(y64.float())
    return torch.cat(out)


def min_margin(y, gamma=None, beta=None, eps=EPS, nseg=1):
    """min over elements of |z| - affine_error_bound: positive = fp32 z has float64 z's sign."""
    Ps = y.shape[0] // nseg
    m = math.inf
    for k in range(nseg):
        ys = y[k * Ps:(k + 1) * Ps]
        mean, inv = stats(ys, eps)
        z = pre_act(ys, mean, inv, gamma, beta)
        m = min(m, (z.abs() - affine_error_bound(ys, mean, inv, gamma, beta)).min().item())
    return m


def assert_off_kink(y, gamma=None, beta=None, eps=EPS, nseg=1):
    """Every |z| >= KINK in float64 with the batch statistics of each of y's nseg row ranges, and
    above the a-priori fp32 error of the kernels' fused affine form (min_margin > 0): no fp32
    evaluation of z takes the other branch of ReLU' / LeakyReLU' (or SELU')."""
    Ps = y.shape[0] // nseg
    for k in range(nseg):
        ys = y[k * Ps:(k + 1) * Ps]
        zmin = pre_act(ys, *stats(ys, eps), gamma, beta).abs().min().item()
        assert zmin >= KINK, (tuple(y.shape), nseg, k, zmin)
    m = min_margin(y, gamma, beta, eps, nseg)
    assert m > 0, (tuple(y.shape), nseg, m)


def inputs(P, C, kinds, seed, affine_on=True, nseg=1):
    """Seeded fp32 CPU inputs: y[P][C] off the kinks (for the statistics of each of nseg row
    ranges), gamma / beta (None with affine_on False), an upstream gradient da = randn + 0.5 +
    0.5 xhat (a constant part and a part along xhat: neither backward sum is a chance
    cancellation at large P) and an addend."""
    g = torch.Generator().manual_seed(seed)
    y = torch.stack([channel(kinds[c], P, g) for c in range(C)], 1)
    gamma, beta = affine(C, g) if affine_on else (None, None)
    y = off_kink(y, gamma, beta, nseg=nseg)
    Ps = P // nseg
    xhat = torch.cat([(y[k * Ps:(k + 1) * Ps].double() - m) * i for k in range(nseg)
                      for m, i in [stats(y[k * Ps:(k + 1) * Ps])]])
    da = (torch.randn(P, C, generator=g).double() + 0.5 + 0.5 * xhat).float()
    add = torch.randn(P, C, generator=g)
    return dict(y=y, gamma=gamma, beta=beta, da=da, add=add)


# Kinds for segments of a single row (n = 1: every channel is constant, z = beta, and the fused form's
# error is 4 u |y| * gamma / sqrt(eps), which must stay under |beta| >= 0.05: |y| of a few units)
TINY = ("a", "b0", "d0", "b1")

# (P, C, nseg) of every backward case of tests/test_bn_first_order_gpu.py (the launch rule each
# one reaches is stated there); test_bn_ref_cpu.py proves their inputs off the kinks
BWD_CASES = [
    (2048, 16, 1), (2049, 16, 1), (100, 16, 1), (100, 20, 1), (64, 128, 1), (64, 48, 1), (64, 144, 1),
    (100, 6, 1), (300, 70, 1),
    (2, 16, 2), (254, 16, 2), (256, 16, 2), (258, 16, 2), (2048, 16, 2), (2050, 16, 2), (4096, 16, 2), (4098, 16, 2),
    (258, 128, 2), (600, 20, 2),
]
SUMS_APPLY_CASES = [(4, 1024), (147, 1024), (4, 1008), (147, 1008)]
TWO_SHARD_CASES = [(200, 32, 1), (90, 6, 1)]


def bwd_mixes(P, C, nseg):
    return mixes(C, TINY) if P // nseg == 1 else mixes(C)


def bwd_inputs(P, C, nseg, mix, affine_on=True):
    """THE inputs of backward case (P, C, nseg), mix number ``mix`` of bwd_mixes (one seed per case
    and mix, used by the GPU module and by test_bn_ref_cpu.py alike), asserted off the kinks.
    -> (label, kinds, inputs dict).  Without gamma / beta z = xhat, and a constant channel's z
    would be 0: its regimes are replaced by ``a``."""
    label, kinds = bwd_mixes(P, C, nseg)[mix]
    if not affine_on:
        kinds = [k if k not in ("b0", "b1") else "a" for k in kinds]
    seed = 100003 * P + 1009 * C + 101 * nseg + 7 * mix + (0 if affine_on else 3)
    d = inputs(P, C, kinds, seed, affine_on=affine_on, nseg=nseg)
    assert_off_kink(d["y"], d["gamma"], d["beta"], nseg=nseg)
    return label, kinds, d


def all_bwd_cases():
    """(P, C, nseg) of every input bwd_inputs serves."""
    return BWD_CASES + [(P, C, 1) for P, C in SUMS_APPLY_CASES] + TWO_SHARD_CASES
