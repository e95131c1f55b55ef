"""WGAN-GP double backward through train-mode BatchNorm2d + activation, kernel by kernel:
rgan_bn_dd_sums, rgan_bn_dd_apply, rgan_act_dd, and the SyncBN form of both backward passes
(global sums for the normalisation, a rank's local sums for its affine gradients), each
against torch fp64 autograd on the CPU.

Reference (independent of the kernels' algebra): z = batch_norm(y), out = act(z),
dy = d out / d y (create_graph, upstream dh), Pen = sum(a * dy); the kernels' outputs are
dPen/d(dh) (adj_dh), dPen/dy with dh held fixed (ydir: the direct term, including mean's and
invstd's dependence on y), dPen/dgamma and dPen/dbeta.  The stage sums are compared with
their fp64 definitions (act', act'' from autograd).  ``stats`` is the fp64 batch mean and
1/sqrt(var + eps) of y cast to fp32: the kernels take it as an input and the formula only
holds for the true batch statistics.

Kink premise: before any kernel runs, every element has |z| >= 1e-3 (elements nearer are
moved 0.05 in y, away from zero, at most three rounds, then it is asserted), so fp32
rounding of z (~1e-5) cannot put an element on the other branch of ReLU', LeakyReLU',
SELU' or SELU''.  No element is masked out of any comparison.

Shapes (B, C, H, W) pick one branch of bn_geo each at the smallest size: vector path one
chunk; scalar path (C % 4 != 0); scalar path with two channel groups and dead lanes, ragged
P = 315; several pixel chunks; tpr = 1 with a ragged second chunk; an odd number (129) of
channel groups; tpr = 64.  P >= 27 everywhere (two pixels per channel is ill-conditioned).

Tolerance: rel L2 < 2e-5 per tensor, the project's bound for fp32 BatchNorm backward against
fp64 (test_batchnorm_train, test_gp_gpu.py); an fp32 restatement of the algebra on the CPU
stays within 2e-7 of this reference, so the bound has ~100x margin.
Largest values observed on an MI355X (over all cases of this module):
  first backward   dy 5.3e-08, dgamma 9.7e-08, dbeta 6.1e-08
  stage 1 sums     sum a 0 (exact), sum a*xhat 1.1e-07, sum a*e 1.1e-07
  stage 2 sums     sum t 4.3e-07, sum t*xhat 2.5e-07
  bn_dd_apply      adj_dh 1.0e-07, ydir 1.7e-07, dgamma2 2.4e-07 (increment 2.5e-07),
                   dbeta2 4.3e-07 (increment 4.9e-07)
  act_dd           adj_dh 5.3e-08, ydir 9.9e-08
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

EPS = 1e-5
TOL = 2e-5
KINK = 1e-3
ALPHA = 0.2
ACTS = ("none", "relu", "lrelu", "tanh", "sigmoid", "selu")
HAS2 = ("tanh", "sigmoid", "selu")
ACT64 = {
    "none": lambda t: t * 1.0,
    "relu": F.relu,
    "lrelu": lambda t: F.leaky_relu(t, ALPHA),
    "tanh": torch.tanh,
    "sigmoid": torch.sigmoid,
    "selu": F.selu,
}
SHAPES = [(6, 8, 4, 4), (3, 5, 3, 3), (5, 6, 9, 7), (8, 64, 8, 8), (4, 12, 20, 20), (3, 516, 3, 3), (4, 1024, 4, 4)]


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    return kernels


def _rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(what, got, want, tag):
    r = _rel(got, want)
    print(f"[bn_dd] {tag} {what} rel {r:.3e}")
    assert r < TOL, (tag, what, r)


def _dev(t):
    """fp64 CPU [B, C, H, W] -> fp32 NHWC on the device."""
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


def _cvec(t):
    return t.float().to(DEV)


def _bc(v):
    return v[None, :, None, None]


def _stats64(y64):
    mean = y64.mean((0, 2, 3))
    inv = 1.0 / torch.sqrt(y64.var((0, 2, 3), unbiased=False) + EPS)
    return mean, inv


def _off_kink(y64, pre):
    """The kink premise: pre(y) -> (z, sign of dz/dy); elements with |z| < KINK move 0.05 in y,
    away from zero (fp32-representable y throughout).  Asserts min |z| >= KINK."""
    for _ in range(3):
        z, slope = pre(y64)
        near = z.abs() < KINK
        if not bool(near.any()):
            break
        away = torch.where(z < 0, -1.0, 1.0) * slope
        y64 = torch.where(near, y64 + 0.05 * away, y64).float().double()
    z, _ = pre(y64)
    assert z.abs().min().item() >= KINK
    return y64


def _act_d12(z, act):
    """act'(z), act''(z) in fp64 from autograd."""
    zz = z.detach().clone().requires_grad_(True)
    (d1,) = torch.autograd.grad(ACT64[act](zz).sum(), zz, create_graph=True)
    d2 = None
    if d1.requires_grad:
        (d2,) = torch.autograd.grad(d1.sum(), zz, allow_unused=True)
    return d1.detach(), (torch.zeros_like(z) if d2 is None else d2.detach())


@functools.lru_cache(maxsize=None)
def _bn_case(shape, act, affine=True):
    """Inputs (fp32-representable, fp64 on the CPU) and the fp64 reference of one case; computed
    once and shared (read-only) by the tests that use it."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * C + B * H * W + ACTS.index(act))
    rnd = lambda *s: torch.randn(*s, generator=gen).double()  # noqa: E731
    y64, dh64, a64 = rnd(*shape) * 1.5 + 0.5, rnd(*shape), rnd(*shape)
    if affine:
        g64 = (0.5 + torch.rand(C, generator=gen).double()) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
        b64 = 0.3 * rnd(C)
        g64, b64 = g64.float().double(), b64.float().double()
    else:
        g64, b64 = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)

    def pre(y):
        mean, inv = _stats64(y)
        return _bc(g64) * (y - _bc(mean)) * _bc(inv) + _bc(b64), _bc(torch.sign(g64)).expand_as(y)

    y64 = _off_kink(y64.float().double(), pre)
    mean, inv = _stats64(y64)
    # the reference: plain autograd
    y, dh = y64.clone().requires_grad_(True), dh64.clone().requires_grad_(True)
    g, b = g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    z = F.batch_norm(y, None, None, g, b, training=True, momentum=0.0, eps=EPS)
    out = ACT64[act](z)
    dgamma, dbeta = torch.autograd.grad(out, [g, b], dh.detach(), retain_graph=True)
    (dy,) = torch.autograd.grad(out, y, dh, create_graph=True)
    pen = (a64 * dy).sum()
    adj_dh, ydir, dgamma2, dbeta2 = torch.autograd.grad(pen, [dh, y, g, b], allow_unused=True)
    # the stage sums from their definitions
    xh = (y64 - _bc(mean)) * _bc(inv)
    d1, d2 = _act_d12(z.detach(), act)
    e = dh64 * d1
    red = lambda t: t.sum((0, 2, 3))  # noqa: E731
    s1 = torch.stack([red(a64), red(a64 * xh), red(a64 * e)])
    P = B * H * W
    pe = _bc(g64 * inv) * (a64 - _bc(s1[0] / P) - xh * _bc(s1[1] / P))
    t = pe * dh64 * d2
    s2 = torch.stack([red(t), red(t * xh)])
    zero = torch.zeros(C, dtype=torch.float64)
    return dict(P=P, C=C, y=y64, dh=dh64, a=a64, gamma=g64, beta=b64, stats=torch.cat([mean, inv]),
                dy=dy.detach(), dgamma=dgamma, dbeta=dbeta, adj_dh=adj_dh, ydir=ydir,
                dgamma2=zero if dgamma2 is None else dgamma2, dbeta2=zero if dbeta2 is None else dbeta2,
                s1=s1, s2=s2)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bn_dd_matches_fp64_autograd(K, shape, act):
    """bn_dd_sums (both stages) and bn_dd_apply (adj_dh, ydir, dgamma2 / dbeta2 written and
    accumulated, need_adj off) and the first backward's dy against the fp64 reference."""
    r = _bn_case(shape, act)
    tag = f"{shape} {act}"
    P, C, two = r["P"], r["C"], act in HAS2
    y, dh, a = _dev(r["y"]), _dev(r["dh"]), _dev(r["a"])
    gamma, beta, stats = _cvec(r["gamma"]), _cvec(r["beta"]), _cvec(r["stats"])
    fs, _ = K.bn_backward_sums(dh, y, stats, gamma, beta, act, ALPHA)
    dy, _, _ = K.bn_backward_apply(dh, y, stats, gamma, beta, act, ALPHA, fs, P, out=_nan_like(y))
    _check("dy", dy, r["dy"], tag)
    s1 = K.bn_dd_sums(a, y, dh, stats, gamma, beta, act, ALPHA, 1)
    for k, name in enumerate(("sum_a", "sum_a_xhat", "sum_a_e")):
        _check(name, s1.view(3, C)[k], r["s1"][k], tag)
    s2 = None
    if two:
        s2 = K.bn_dd_sums(a, y, dh, stats, gamma, beta, act, ALPHA, 2, s1, P)
        for k, name in enumerate(("sum_t", "sum_t_xhat")):
            _check(name, s2.view(2, C)[k], r["s2"][k], tag)
    dg2, db2 = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    adj, ydir = K.bn_dd_apply(a, y, dh, stats, gamma, beta, act, ALPHA, fs, s1, s2, P, adj_dh=_nan_like(y),
                              ydir=_nan_like(y), dgamma2=dg2, dbeta2=db2)
    _check("adj_dh", adj, r["adj_dh"], tag)
    _check("ydir", ydir, r["ydir"], tag)
    _check("dgamma2", dg2, r["dgamma2"], tag)
    if two:
        _check("dbeta2", db2, r["dbeta2"], tag)
    else:  # no stage 2: the kernel writes 0, the reference gradient is zero (or None)
        assert torch.count_nonzero(r["dbeta2"]) == 0 and torch.count_nonzero(db2) == 0, tag
    # accumulated onto a random base: the increment
    g0, b0 = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    dga, dba = g0.clone(), b0.clone()
    adj_a, ydir_a = K.bn_dd_apply(a, y, dh, stats, gamma, beta, act, ALPHA, fs, s1, s2, P, dgamma2=dga, dbeta2=dba,
                                  accumulate_affine=True)
    assert torch.equal(adj_a, adj) and torch.equal(ydir_a, ydir), tag
    _check("dgamma2 increment", dga.double() - g0.double(), r["dgamma2"], tag)
    if two:
        _check("dbeta2 increment", dba.double() - b0.double(), r["dbeta2"], tag)
    else:
        assert torch.equal(dba, b0), tag
    # need_adj off: no adj_dh, the same ydir
    none, ydir_b = K.bn_dd_apply(a, y, dh, stats, gamma, beta, act, ALPHA, fs, s1, s2, P, ydir=_nan_like(y),
                                 need_adj=False)
    assert none is None and torch.equal(ydir_b, ydir), tag


@pytest.mark.parametrize("act", ACTS)
def test_bn_dd_without_affine(K, act):
    """gamma = beta = None: the reference with unit weight and zero bias."""
    shape = (5, 6, 9, 7)
    r = _bn_case(shape, act, affine=False)
    tag = f"{shape} {act} no affine"
    P, two = r["P"], act in HAS2
    y, dh, a, stats = _dev(r["y"]), _dev(r["dh"]), _dev(r["a"]), _cvec(r["stats"])
    fs, _ = K.bn_backward_sums(dh, y, stats, None, None, act, ALPHA)
    dy, dg, db = K.bn_backward_apply(dh, y, stats, None, None, act, ALPHA, fs, P, out=_nan_like(y))
    assert dg is None and db is None
    _check("dy", dy, r["dy"], tag)
    s1 = K.bn_dd_sums(a, y, dh, stats, None, None, act, ALPHA, 1)
    s2 = K.bn_dd_sums(a, y, dh, stats, None, None, act, ALPHA, 2, s1, P) if two else None
    adj, ydir = K.bn_dd_apply(a, y, dh, stats, None, None, act, ALPHA, fs, s1, s2, P, adj_dh=_nan_like(y),
                              ydir=_nan_like(y))
    _check("adj_dh", adj, r["adj_dh"], tag)
    _check("ydir", ydir, r["ydir"], tag)


@pytest.mark.parametrize("act", ["lrelu", "tanh"])
@pytest.mark.parametrize("shape", [(8, 64, 8, 8), (6, 6, 5, 5)])
def test_syncbn_form_two_halves(K, shape, act):
    """The SyncBN form on one GPU: the batch's two halves as two ranks.  Whole-batch stats, each
    half's local sums added on the device (the all-reduce), every half applied with the
    global sums and P_global = P while its affine gradients come from its own sums and
    accumulate into one shared pair.  Both the first backward (bn_backward_apply_ex +
    bn_affine_grads, as the GP engine runs it under SyncBN) and the double backward must
    match the whole-batch fp64 reference."""
    r = _bn_case(shape, act)
    tag = f"{shape} {act} two halves"
    P, C, two = r["P"], r["C"], act in HAS2
    B = shape[0]
    y, dh, a = _dev(r["y"]), _dev(r["dh"]), _dev(r["a"])
    gamma, beta, stats = _cvec(r["gamma"]), _cvec(r["beta"]), _cvec(r["stats"])
    halves = [slice(0, B // 2), slice(B // 2, B)]
    fs_l = [K.bn_backward_sums(dh[h], y[h], stats, gamma, beta, act, ALPHA)[0] for h in halves]
    fs = fs_l[0] + fs_l[1]
    # first backward
    dy = _nan_like(y)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    for h, loc in zip(halves, fs_l):
        K.bn_backward_apply_ex(dh[h], y[h], stats, gamma, beta, act, ALPHA, fs, P, out=dy[h], dgamma=None,
                               dbeta=None)
        K.bn_affine_grads(loc, stats, C, dg, db, accumulate=True)
    _check("dy", dy, r["dy"], tag)
    _check("dgamma", dg, r["dgamma"], tag)
    _check("dbeta", db, r["dbeta"], tag)
    # double backward
    s1_l = [K.bn_dd_sums(a[h], y[h], dh[h], stats, gamma, beta, act, ALPHA, 1) for h in halves]
    s1 = s1_l[0] + s1_l[1]
    for k, name in enumerate(("sum_a", "sum_a_xhat", "sum_a_e")):
        _check(name, s1.view(3, C)[k], r["s1"][k], tag)
    s2_l, s2 = [None, None], None
    if two:
        s2_l = [K.bn_dd_sums(a[h], y[h], dh[h], stats, gamma, beta, act, ALPHA, 2, s1, P) for h in halves]
        s2 = s2_l[0] + s2_l[1]
        for k, name in enumerate(("sum_t", "sum_t_xhat")):
            _check(name, s2.view(2, C)[k], r["s2"][k], tag)
    adj, ydir = _nan_like(y), _nan_like(y)
    dg2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    for h, l1, l2 in zip(halves, s1_l, s2_l):
        K.bn_dd_apply(a[h], y[h], dh[h], stats, gamma, beta, act, ALPHA, fs, s1, s2, P, s1_local=l1, s2_local=l2,
                      adj_dh=adj[h], ydir=ydir[h], dgamma2=dg2, dbeta2=db2, accumulate_affine=True)
    _check("adj_dh", adj, r["adj_dh"], tag)
    _check("ydir", ydir, r["ydir"], tag)
    _check("dgamma2", dg2, r["dgamma2"], tag)
    if two:
        _check("dbeta2", db2, r["dbeta2"], tag)
    else:
        assert torch.count_nonzero(db2) == 0, tag


# rgan_act_dd launches min(ceil(n / 256), 8192) blocks of 256 threads: one sweep of the grid
# covers 8192 * 256 elements, so the last size makes the grid-stride loop run three times
ACT_DD_SHAPES = [(1,), (3, 5, 7, 3), (2 * 8192 * 256 + 333,)]


def _act_case(shape, act):
    gen = torch.Generator().manual_seed(77 + len(shape) + ACTS.index(act))
    rnd = lambda: torch.randn(*shape, generator=gen).double()  # noqa: E731
    y64, dh64, a64 = rnd(), rnd(), rnd()
    y64 = _off_kink(y64, lambda y: (y, torch.ones_like(y)))
    y, dh = y64.clone().requires_grad_(True), dh64.clone().requires_grad_(True)
    out = ACT64[act](y)
    (dy,) = torch.autograd.grad(out, y, dh, create_graph=True)
    adj_dh, ydir = torch.autograd.grad((a64 * dy).sum(), [dh, y], allow_unused=True)
    return dict(a=a64, dh=dh64, out=out.detach(), adj_dh=adj_dh, ydir=torch.zeros_like(y64) if ydir is None else ydir)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", ACT_DD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act_dd_matches_fp64_autograd(K, shape, act):
    """rgan_act_dd (layers without BatchNorm): adj_dh = a act'(y), ydir = a dh act''(y) from
    the activation output, against fp64 autograd of out = act(y); every flag combination."""
    r = _act_case(shape, act)
    tag = f"act_dd {shape} {act}"
    a, dh, o = (r[k].float().to(DEV) for k in ("a", "dh", "out"))
    for need_adj, need_ydir in ((True, True), (True, False), (False, True)):
        adj, ydir = K.act_dd(a, o, dh, act, ALPHA, need_adj=need_adj, need_ydir=need_ydir,
                             adj_dh=_nan_like(a) if need_adj else None, ydir=_nan_like(a) if need_ydir else None)
        assert (adj is not None) == need_adj and (ydir is not None) == need_ydir, tag
        if need_adj:
            _check("adj_dh", adj, r["adj_dh"], tag)
        if need_ydir and act in HAS2:
            _check("ydir", ydir, r["ydir"], tag)
        elif need_ydir:  # act'' = 0
            assert torch.count_nonzero(r["ydir"]) == 0 and torch.count_nonzero(ydir) == 0, tag
