"""One float64 statement of the eight --loss_D heads and of the WGAN-GP penalty, and the seeded
inputs the head / penalty kernel tests run on.

The references are the oracle's own expressions (oracle/reference_cpu.py head_real, head_fake,
head_relativistic_D, head_G and the penalty of gradient_penalty, which the goldens pin to the
reference) on float64 CPU tensors with torch autograd.  Every generator returns float32 CPU
tensors and states a condition on them; tests/test_heads_ref_cpu.py proves each condition, so
the GPU tests compare every element and mask none.
"""
import torch

from oracle.reference_cpu import head_fake, head_G, head_real, head_relativistic_D

# (kind, side): side 0 = D on real (heads 1-4) or D (heads 5-8), 1 = D on fake (1-4), 2 = G
CASES = [(k, s) for k in (1, 2, 3, 4) for s in (0, 1, 2)] + [(k, s) for k in (5, 6, 7, 8) for s in (0, 2)]
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 65536)
BATCHES = (1, 5, 32, 64)            # the [B, 1, 1, 1] D outputs of the losses.py tests
# shards of a global batch, as the ranks of a data-parallel run hold them (any n <= n_global)
DIST_SPLITS = ((1025, 1025), (125,) * 8, (1, 333, 666), (65536, 65536))
ALL_SIZES = tuple(sorted(set(SIZES + BATCHES + tuple(sum(s) for s in DIST_SPLITS))))
HINGE = (4, 8)
KINK_NEAR, KINK_AWAY = 1e-3, 1e-2   # no element within NEAR of a hinge kink; offenders moved to AWAY
KINK_N, KINK_STEP = 64, 2.0 ** -9   # the ``kink`` inputs: 64 multiples of 2^-9, |v| <= 8

WIDE_PLANTS = (1e4, -1e4, 89.0, -89.0, 88.0, -88.0, 104.0, -104.0)
BCE_PLANTS = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-30)


def regimes(kind):
    """The input regimes that apply to a head."""
    return ("typical", "bce_edge") if kind == 1 else ("typical", "offset", "wide")


def needs(kind, side):
    """(reads r, reads f) of rgan_loss_head(kind, side)."""
    return (kind > 4 or side == 0), (kind > 4 or side != 0)


def ref_head(kind, side, r64, f64):
    """(loss, dr, df) of the oracle's head in float64; an unused input is None and so is its
    gradient."""
    r = r64.detach().clone().requires_grad_(True) if r64 is not None else None
    f = f64.detach().clone().requires_grad_(True) if f64 is not None else None
    ones = torch.ones_like(r if r is not None else f)
    zeros = torch.zeros_like(ones)
    if kind <= 4:
        if side == 0:
            loss = head_real(kind, r, ones)
        elif side == 1:
            loss = head_fake(kind, f, zeros)
        else:
            loss = head_G(kind, f, None, ones, zeros)
    elif side == 0:
        loss = head_relativistic_D(kind, r, f, ones, zeros)
    elif side == 2:
        loss = head_G(kind, f, r, ones, zeros)
    else:
        raise ValueError(f"heads 5-8 have no side {side}")
    loss.backward()
    return loss.detach(), (r.grad if r is not None else None), (f.grad if f is not None else None)


def ref_gp(g64, lam, n_global):
    """(loss, per-sample norms, d loss / d g) of the oracle's penalty expression on a float64
    gradient image [B, C, H, W] (its .mean() over the local batch written as .sum() / n_global)."""
    g = g64.detach().clone().requires_grad_(True)
    norms = g.norm(2, 1).norm(2, 1).norm(2, 1)
    loss = lam * ((norms - 1) ** 2).sum() / n_global
    loss.backward()
    return loss.detach(), norms.detach(), g.grad


def gp_closed_form(g64, lam, n_global):
    """include/rgan.h: loss = lam * sum_b (n_b - 1)^2 / n_global and
    dg_b = lam * 2 (n_b - 1) / n_global * g_b / n_b, zero where n_b = 0."""
    flat = g64.reshape(g64.shape[0], -1)
    nb = flat.pow(2).sum(1).sqrt()
    coef = torch.where(nb > 0, lam * 2 * (nb - 1) / n_global / nb.clamp_min(1e-300), torch.zeros_like(nb))
    return lam * ((nb - 1) ** 2).sum() / n_global, nb, (coef[:, None] * flat).reshape(g64.shape)


# ---------------------------------------------------------------- hinge kinks
def kink_margins(kind, r64, f64):
    """Float64 distance of every element from every hinge kink it can meet, over all sides of
    the head: (margins of r, margins of f), each [2, n] (kind 8) or [1, n] (kind 4)."""
    if kind == 4:  # side 0: relu(1 - r); side 1: relu(1 + f); side 2 has no kink
        return (1 - r64).abs()[None], (1 + f64).abs()[None]
    dr, df = r64 - f64.mean(), f64 - r64.mean()
    return torch.stack([(1 - dr).abs(), (1 + dr).abs()]), torch.stack([(1 + df).abs(), (1 - df).abs()])


def _push_off_kinks(kind, r, f):
    """Move every float32 element whose float64 margin is below KINK_NEAR to KINK_AWAY from that
    kink, on the side it is on; repeat (the relativistic means move with it) until none is."""
    for _ in range(100):
        r64, f64 = r.double(), f.double()
        mr, mf = kink_margins(kind, r64, f64)
        if min(mr.min().item(), mf.min().item()) >= KINK_NEAR:
            return r, f
        cr, cf = (0.0, 0.0) if kind == 4 else (f64.mean().item(), r64.mean().item())
        for t64, t, margins, centre, kinks in ((r64, r, mr, cr, (1.0, -1.0)), (f64, f, mf, cf, (-1.0, 1.0))):
            for row, k in zip(margins, kinks):
                near = row < KINK_NEAR
                side = (t64 - centre >= k).double() * 2 - 1
                t[near] = (centre + k + side * KINK_AWAY)[near].float()
    raise AssertionError("hinge inputs did not settle off the kinks")


def _plant(t, values, at):
    """Write values[i] to t[at + i] for as many as fit (all of them when n >= len(values))."""
    k = min(len(values), t.numel() - at) if at < t.numel() else 0
    t[at:at + k] = torch.tensor(values[:k], dtype=t.dtype)
    return k


def planted(values, n, which):
    """The planted values that gen() puts into r (which = 0) or f (which = 1) at size n: all of
    them from n = len(values) on, the first n below (f takes them in reverse order, at the end of
    the tensor, so that r - f of the RSGAN head meets the extremes too)."""
    vals = tuple(values) if which == 0 else tuple(reversed(values))
    return vals[:min(n, len(vals))]


def gen(regime, kind, n, seed=0):
    """Float32 CPU inputs (r, f) of n elements each.

    typical   N(0, 2^2), f shifted by -0.5; head 1: U(0.01, 0.99).
    offset    r ~ N(50, 1), f ~ N(49.5, 1) (heads 2-8): the relativistic means carry the rounding.
    wide      N(0, 30^2) with WIDE_PLANTS written into r (front) and f (back, reversed): the fp32
              expf overflow edge (+-88, +-89), past it (+-104) and +-1e4 (heads 2-8).
    bce_edge  U[0, 1) with BCE_PLANTS written the same way (head 1): exactly 0 and 1, where the
              -100 clamp and the 1e-12 denominator apply, and their fp32 neighbours.
    kink      n = KINK_N multiples of KINK_STEP with |v| <= 8, elements on each kink and
              KINK_STEP to either side of it (heads 4 and 8): see kink_inputs().
    For the hinge heads 4 and 8, typical / offset / wide hold no element within KINK_NEAR of a kink.
    """
    if regime == "kink":
        assert n == KINK_N
        return kink_inputs(kind)
    assert regime in regimes(kind), (regime, kind)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * kind + 101 * n + len(regime))
    if regime == "typical" and kind == 1:
        r = torch.rand(n, generator=g) * 0.98 + 0.01
        f = torch.rand(n, generator=g) * 0.98 + 0.01
    elif regime == "typical":
        r = torch.randn(n, generator=g) * 2
        f = torch.randn(n, generator=g) * 2 - 0.5
    elif regime == "offset":
        r = torch.randn(n, generator=g) + 50.0
        f = torch.randn(n, generator=g) + 49.5
    elif regime == "wide":
        r = torch.randn(n, generator=g) * 30
        f = torch.randn(n, generator=g) * 30
        _plant(r, planted(WIDE_PLANTS, n, 0), 0)
        pf = planted(WIDE_PLANTS, n, 1)
        _plant(f, pf, n - len(pf))
    else:
        r = torch.rand(n, generator=g)
        f = torch.rand(n, generator=g)
        _plant(r, planted(BCE_PLANTS, n, 0), 0)
        pf = planted(BCE_PLANTS, n, 1)
        _plant(f, pf, n - len(pf))
    if kind in HINGE:
        r, f = _push_off_kinks(kind, r, f)
    return r, f


def kink_points(kind):
    """(kinks of r, kinks of f) of the ``kink`` inputs: the values at which a hinge of some side
    of the head switches.  Head 8's inputs have mean r = 0.25 and mean f = -0.5 exactly."""
    if kind == 4:
        return (1.0,), (-1.0,)
    mr, mf = 0.25, -0.5
    return (mf + 1, mf - 1), (mr - 1, mr + 1)


def kink_inputs(kind):
    """Dyadic inputs on and around every kink.  Every value is a multiple of 2^-9 with |v| <= 8,
    so every sum, mean, difference and quotient by n = 64 the heads form is exact in float32: a
    kernel can differ from float64 only by a wrong branch or a wrong formula."""
    assert kind in HINGE
    g = torch.Generator().manual_seed(4242 + kind)
    d = KINK_STEP
    out = []
    for kinks, mean in zip(kink_points(kind), (0.25, -0.5)):
        t = torch.randint(-2048, 2049, (KINK_N,), generator=g).double() * d  # |v| <= 4
        plants = [k + s * d for k in kinks for s in (0, -1, 1)]
        t[:len(plants)] = torch.tensor(plants, dtype=torch.float64)
        if kind == 8:  # the last eight elements bring the mean to its target exactly
            rest = mean * KINK_N - t[:-8].sum().item()
            t[-8:-1] = round(rest / 8 / d) * d
            t[-1] = rest - t[-8:-1].sum().item()
        out.append(t)
    r, f = out
    assert max(r.abs().max().item(), f.abs().max().item()) <= 8
    assert torch.equal(r, (r / d).round() * d) and torch.equal(f, (f / d).round() * d)
    return r.float(), f.float()


# ---------------------------------------------------------------- penalty inputs
GP_SHAPES = ((1, 1), (3, 7), (8, 768), (5, 1025), (4, 12288), (2, 196608))
GP_ROWS = ("zero", "basis", "unit", "big", "small", "random")
# (n_global / batch, gscale, start): the rotation differs per combination so that a batch of two
# meets every kind of sample over the four
GP_COMBOS = ((1, 1.0, 0), (4, 1.0, 2), (1, -2.5, 4), (4, -2.5, 1))


def gp_rows(batch, start):
    """The kind of each sample of gp_inputs(batch, per, start): GP_ROWS in rotation from start."""
    return [GP_ROWS[(start + b) % len(GP_ROWS)] for b in range(batch)]


def gp_inputs(batch, per, start, seed=0):
    """A float32 CPU gradient image [batch, per] whose sample b is, by gp_rows(batch, start):
    zero    all zeros (norm 0: the kernel's own branch; loss term 1, gradient 0);
    basis   one element 1.0 and zeros (norm exactly 1: gradient exactly 0);
    unit    a random direction scaled to norm 1 within fp32 rounding (norm - 1 cancels);
    big     a random direction of norm 1e3;   small   of norm 1e-3;   random   N(0, 1)."""
    gen_ = torch.Generator().manual_seed(77 * seed + 13 * batch + per + 1000 * start)
    g = torch.randn(batch, per, generator=gen_, dtype=torch.float64)
    for b, kind in enumerate(gp_rows(batch, start)):
        if kind == "zero":
            g[b] = 0
        elif kind == "basis":
            g[b] = 0
            g[b, (7 * b + per // 2) % per] = 1.0
        elif kind != "random":
            g[b] *= {"unit": 1.0, "big": 1e3, "small": 1e-3}[kind] / g[b].norm()
    return g.float()
