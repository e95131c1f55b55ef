"""--rgan_r1 / --rgan_r2 on the MI355X: the zero-centred penalty kernels (csrc/gp_zc.hip) against
float64, the rgan::gp_zc_penalty operators, graph capture, the generalised GP engine against the
autograd composite and against float64 autograd on the oracle's D, one training iteration against
an exact float64 step built here from the oracle's nets and heads, the lazy schedule, the
flags-off launch sequence, data parallelism and the training CLI.

Kernel bound: 1e-5 relative, the bound tests/test_kernels_gpu.py holds the one-centred penalty
kernels to.  A squared norm is a sum of non-negative products: each thread accumulates its share
of a block's chunk in fp32 (at most 8 fused steps at the shapes below: a chunk is 2048 floats over
256 threads), and every sum after that is in double, so the expected relative error is below
10 * 2^-24 = 6e-7.  The gradient is two fp32 products per element (2 * 2^-24 = 1.2e-7).
"""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from tests.test_diffaug_gpu import _Counter
from tests.test_ema_gpu import TINY_CLI, _cut
from tests.test_gp_gpu import CASES
from tests.test_ops_gpu import OPCHECK
from tests.test_parity_gpu import TOL_BUF, TOL_GRAD, TOL_OUT, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgan_gp_zc_workspace", "rgan_gp_zc_penalty", "rgan_gp_zc_penalty_backward")

# ---------------------------------------------------------------- 1. kernels against float64
BATCHES = (1, 6, 65)
PERS = (1, 3, 4, 4095, 768, 12288, 49152)
GAMMA = 2.5  # exact in fp32


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _values(batch, per):
    gen = torch.Generator(device=DEV).manual_seed(1000 * batch + per)
    return torch.randn(batch, per, device=DEV, generator=gen)


def _want(g, n_global, gscale):
    g64 = g.double()
    sq = (g64 * g64).sum(1)
    return GAMMA / 2 * sq.sum() / n_global, sq, (1.0 if gscale is None else gscale) * GAMMA / n_global * g64


@pytest.mark.parametrize("per", PERS)
def test_kernels_match_float64(per):
    from relativisticgan_amd import kernels as K
    worst = {"loss": 0.0, "sq": 0.0, "dg": 0.0}
    for batch in BATCHES:
        vals = _values(batch, per)
        for misaligned in (False, True):
            gbuf, g, lead = _cut(vals, misaligned)
            for n_global in (batch, 2 * batch):
                loss, sq, gc = K.gp_zc_penalty(g, GAMMA, n_global)
                assert gc.data_ptr() == g.data_ptr()
                loss2, sq2, _ = K.gp_zc_penalty(g, GAMMA, n_global)  # fixed summation order
                assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(sq), _bits(sq2))
                for gscale in (None, 0.25):
                    w_loss, w_sq, w_dg = _want(vals, n_global, gscale)
                    gs = None if gscale is None else torch.tensor(gscale, device=DEV)
                    obuf, out, _ = _cut(torch.zeros_like(vals), misaligned)
                    dg = K.gp_zc_penalty_backward(g, GAMMA, n_global, gs, out=out)
                    assert dg.data_ptr() == out.data_ptr()
                    assert torch.isnan(obuf[:lead]).all() and torch.isnan(obuf[lead + vals.numel():]).all()
                    fresh = K.gp_zc_penalty_backward(g, GAMMA, n_global, gs)
                    assert torch.equal(_bits(fresh), _bits(dg))
                    # in place over a copy of g: the same bits, the guards untouched
                    ibuf, gi, _ = _cut(vals, misaligned)
                    assert K.gp_zc_penalty_backward(gi, GAMMA, n_global, gs, out=gi).data_ptr() == gi.data_ptr()
                    assert torch.equal(_bits(gi), _bits(dg)), (batch, per, misaligned)
                    assert torch.isnan(ibuf[:lead]).all() and torch.isnan(ibuf[lead + vals.numel():]).all()
                    e_dg = _rel(dg, w_dg)
                    worst["dg"] = max(worst["dg"], e_dg)
                    assert e_dg <= 1e-5, (batch, per, misaligned, n_global, gscale, e_dg)
                e_loss = abs(loss.item() - w_loss.item()) / abs(w_loss.item())
                e_sq = ((sq.double() - w_sq).abs() / w_sq).max().item()
                worst["loss"], worst["sq"] = max(worst["loss"], e_loss), max(worst["sq"], e_sq)
                assert e_loss <= 1e-5 and e_sq <= 1e-5, (batch, per, misaligned, n_global, e_loss, e_sq)
            # the forward only read g: values and guards are as they were
            assert torch.equal(_bits(g), _bits(vals))
            assert torch.isnan(gbuf[:lead]).all() and torch.isnan(gbuf[lead + vals.numel():]).all()
    print(f"gp_zc per={per}: worst rel err loss {worst['loss']:.2e} sq {worst['sq']:.2e} dg {worst['dg']:.2e}")


@pytest.mark.parametrize("per", (3, 768, 12288))
def test_all_zero_gradient(per):
    from relativisticgan_amd import kernels as K
    g = torch.zeros(6, per, device=DEV)
    loss, sq, _ = K.gp_zc_penalty(g, GAMMA, 6)
    dg = K.gp_zc_penalty_backward(g, GAMMA, 6, torch.tensor(0.25, device=DEV))
    assert loss.item() == 0.0 and (sq == 0).all() and (dg == 0).all()


def test_argument_checks():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd._lib import RganError
    g = _values(6, 768)
    with pytest.raises(RganError):
        K.gp_zc_penalty(g, GAMMA, 5)  # n_global < batch
    with pytest.raises(RganError):
        K.gp_zc_penalty_backward(g.t(), GAMMA, 6, None)
    with pytest.raises(RganError):
        K.gp_zc_penalty_backward(g, GAMMA, 6, None, out=torch.empty(6, 767, device=DEV))
    with pytest.raises(RganError):
        K.gp_zc_penalty(g.cpu(), GAMMA, 6)


# ---------------------------------------------------------------- 2. operators
def test_opcheck_and_autograd():
    from relativisticgan_amd import ops  # noqa: F401  (registers rgan::)
    g = _values(6, 768).view(6, 3, 16, 16).clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.rgan.gp_zc_penalty.default, (g, GAMMA, 12), test_utils=OPCHECK)
    gl = torch.tensor(0.25, device=DEV)
    torch.library.opcheck(torch.ops.rgan.gp_zc_penalty_backward.default, (g.detach(), GAMMA, 12, gl),
                          test_utils=("test_schema", "test_faketensor"))
    loss, sq = torch.ops.rgan.gp_zc_penalty(g, GAMMA, 12)
    w_loss, w_sq, w_dg = _want(g.detach().reshape(6, -1), 12, None)
    assert _rel(loss, w_loss) <= 1e-5 and _rel(sq, w_sq) <= 1e-5
    dg, = torch.autograd.grad(loss, g, create_graph=True)
    assert dg.shape == g.shape and _rel(dg, w_dg) <= 1e-5
    with pytest.raises(NotImplementedError):  # the backward of the backward is the engine's
        torch.autograd.grad(dg.sum(), g)


# ---------------------------------------------------------------- 3. capture
def test_captured_calls_follow_g_and_gscale():
    from relativisticgan_amd import kernels as K
    g = _values(6, 12288).clone()
    gs = torch.tensor(0.25, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.gp_zc_penalty_backward(K.gp_zc_penalty(g, GAMMA, 12)[2], GAMMA, 12, gs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss, sq, _ = K.gp_zc_penalty(g, GAMMA, 12)
        dg = K.gp_zc_penalty_backward(g, GAMMA, 12, gs)
    new = _values(6, 12288) * 3 + 1
    side.wait_stream(torch.cuda.current_stream())  # new is computed on the current stream
    with torch.cuda.stream(side):
        g.copy_(new)
        gs.fill_(-0.5)
        graph.replay()
    torch.cuda.synchronize()
    w_loss, w_sq, w_dg = _want(new, 12, -0.5)
    assert _rel(loss, w_loss) <= 1e-5 and _rel(sq, w_sq) <= 1e-5 and _rel(dg, w_dg) <= 1e-5


# ---------------------------------------------------------------- 4. engine against composite / float64
# gamma = 1, the value the trainer cases below use.  The penalty and its gradients are linear in
# gamma, so the relative bounds do not depend on it; the absolute escape for exactly-zero gradients
# (tests/test_gp_gpu.py's 1e-7) does: the two sides' roundoff there scales with gamma (at gamma = 10
# the arch-1 first conv bias, which feeds BatchNorm, differed by 5.1e-7 between them)
ZC_GAMMA = 1.0
ORACLE_CASES = ("arch0_tanh", "arch0_nobn", "arch0_bn_lrelu")


def _run_pen(D, point, fn, grads0):
    for q, g in zip(D.parameters(), grads0):
        q.grad = g.clone()
    pen = fn(D, point, ZC_GAMMA)
    pen.backward()
    torch.cuda.synchronize()
    return pen.detach().clone(), [q.grad.detach().clone() for q in D.parameters()], \
        {k: v.detach().clone() for k, v in D.state_dict().items()}


def _oracle_penalty(case, state0, point):
    """loss and D's gradients by float64 autograd on the oracle's D (same weights, train mode)."""
    from oracle import reference_cpu as O
    kw = {k: (v == "True" if isinstance(v, str) else v) for k, v in CASES[case].items()}
    D = O.build_D(O.make_param(cuda=False, batch_size=6, seed=1, **kw)).double()
    D.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()
                       for k, v in state0.items()})
    p = point.detach().cpu().double().requires_grad_(True)
    g, = torch.autograd.grad(D(p).sum(), p, create_graph=True)
    pen = ZC_GAMMA / 2 * (g * g).flatten(1).sum(1).mean()
    pen.backward()
    return pen.detach(), {n: q.grad.detach().clone() for n, q in D.named_parameters()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_native_penalty_matches_composite(case):
    from relativisticgan_amd import losses
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_D, weights_init
    torch.manual_seed(7)
    torch.set_num_threads(4)
    p = make_param(batch_size=6, seed=1, **CASES[case])
    D = DCGAN_D(p)
    D.apply(weights_init)
    D = D.to(DEV)
    S = p.image_size
    x = torch.rand(6, 3, S, S, device=DEV) * 2 - 1
    x0 = x.clone()
    grads0 = [torch.randn_like(q) * 1e-2 for q in D.parameters()]
    state0 = {k: v.clone() for k, v in D.state_dict().items()}
    pen_n, g_n, st_n = _run_pen(D, x, losses.zero_centered_penalty, grads0)
    D.load_state_dict(state0)
    pen_c, g_c, st_c = _run_pen(D, x, losses.zero_centered_penalty_composite, grads0)
    assert torch.equal(x, x0) and x.grad is None  # the point is read only; nothing flows to it
    assert abs(pen_n.item() - pen_c.item()) <= 2e-5 * abs(pen_c.item())
    names = [n for n, _ in D.named_parameters()]
    for n, a, b, g0 in zip(names, g_n, g_c, grads0):
        # the penalty's own contribution (the accumulated base cancels exactly); a conv bias
        # feeding BatchNorm has an exact gradient of 0: both are roundoff
        assert _rel(a - g0, b - g0) < 2e-5 or (a - b).abs().max() < 1e-7, (case, n, _rel(a - g0, b - g0))
    for k in st_c:  # BN running stats and spectral u/v move exactly as in one D(point) call
        if st_c[k].is_floating_point():
            assert _rel(st_n[k], st_c[k]) < 1e-6, (case, k)
        else:
            assert torch.equal(st_n[k], st_c[k]), (case, k)
    assert any(not torch.equal(st_n[k], state0[k]) for k in st_n) == any(
        "running" in k or "weight_u" in k for k in st_n)
    if case in ORACLE_CASES:
        # against float64 the engine starts from zero gradients: on top of the random ones the
        # penalty's own part is only known to an ulp of the base (6e-10 here), which is no
        # smaller than the whole gradient of the BatchNorm-free D at its initial weights
        w_pen, w_grads = _oracle_penalty(case, state0, x)
        D.load_state_dict(state0)
        pen_z, g_z, _ = _run_pen(D, x, losses.zero_centered_penalty, [torch.zeros_like(q) for q in D.parameters()])
        r = _rel(pen_z, w_pen)
        print(f"{case} penalty vs float64: rel {r:.2e}")
        assert r <= TOL_OUT, (case, r)
        assert names == list(w_grads)
        bad = []
        for n, a in zip(names, g_z):
            r = _rel(a, w_grads[n])
            print(f"{case} grad {n} vs float64: rel L2 {r:.2e}")
            if not r <= TOL_GRAD:
                bad.append((n, r))
        assert not bad, bad


# ---------------------------------------------------------------- 5. one iteration against an exact step
STEP = dict(image_size=32, batch_size=6, G_h_size=8, D_h_size=8, z_size=16, Tanh_GD=True, seed=1)
POLICY = "color,translation,cutout"
STEP_CASES = {
    "rsgan_r1_r2_batched": dict(loss_D=5, rgan_r1=2.0, rgan_r2=0.5),
    "ralsgan_r1_unbatched": dict(loss_D=7, rgan_r1=2.0, rgan_batch_D=False),
    "wgangp_r1": dict(loss_D=3, rgan_r1=2.0),
    "ralsgan_r1_diffaug": dict(loss_D=7, rgan_r1=2.0, rgan_diffaug=POLICY),
}


def _trainer(kw):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    cfg = dict(STEP, print_every=10 ** 9)
    cfg.update(kw)
    return Trainer(make_param(**cfg), synthetic_images(64, 32, device=DEV))


def _step_feed(kind):
    gen = torch.Generator().manual_seed(17)
    B = STEP["batch_size"]
    return {"x_D": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, "z_D": torch.randn(B, 16, 1, 1, generator=gen),
            "aug_D": torch.rand(2 * B, 8, generator=gen), "u": torch.rand(B, 1, 1, 1, generator=gen),
            "z_G": torch.randn(B, 16, 1, 1, generator=gen), "x_G": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1,
            "aug_G": torch.rand((2 if kind > 4 else 1) * B, 8, generator=gen)}


def _zc64(D, point, gamma):
    """gamma / 2 * mean_b ||d sum(D(point)) / d point_b||^2 by torch autograd, one more call of D."""
    p = point.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad(D(p).sum(), p, create_graph=True)
    return gamma / 2 * (g * g).flatten(1).sum(1).mean()


def _exact_step(kw, init_G, init_D, feed):
    """The iteration in float64 on the host: the oracle's nets and heads, the restated transform,
    torch autograd for the penalties, torch's Adam for the D step in between."""
    from oracle import reference_cpu as O
    from relativisticgan_amd.augment import parse_policy
    from tests import diffaug_ref as ref
    mask = parse_policy(kw.get("rgan_diffaug", ""))
    p = O.make_param(cuda=False, **STEP, **{k: v for k, v in kw.items() if not k.startswith("rgan_")})
    G, D = O.build_G(p).double(), O.build_D(p).double()
    G.load_state_dict({k: v.double() for k, v in init_G.items()})
    D.load_state_dict({k: v.double() for k, v in init_D.items()})
    f = {k: v.double() for k, v in feed.items()}
    kind, B = p.loss_D, p.batch_size
    ones, zeros = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)

    def T(x, u):
        return ref.forward(x, u, mask) if mask else x

    out = {}
    x_t = T(f["x_D"], feed["aug_D"][:B])
    fake_t = T(G(f["z_D"]).detach(), feed["aug_D"][B:])
    y_pred = D(x_t)
    if kind <= 4:
        err_real = O.head_real(kind, y_pred, ones)
        err_real.backward()
        err_fake = O.head_fake(kind, D(fake_t), zeros)
        err_fake.backward()
        out["errD"] = (err_real + err_fake).detach()
    else:
        errD = O.head_relativistic_D(kind, y_pred, D(fake_t), ones, zeros)
        errD.backward()
        out["errD"] = errD.detach()
    if kind == 3 or p.grad_penalty:
        gp = O.gradient_penalty(D, x_t, fake_t, f["u"], p.penalty, ones)
        gp.backward()
        out["gp"] = gp.detach()
    for key, point in (("r1", x_t), ("r2", fake_t)):  # on the batches D saw, R1 then R2
        gamma = kw.get("rgan_" + key, 0.0)
        if gamma:
            pen = _zc64(D, point, gamma)
            pen.backward()
            out[key] = pen.detach()
    out["gradD"] = {n: q.grad.detach().clone() for n, q in D.named_parameters()}
    out["bufD"] = {k: v.detach().clone() for k, v in D.named_buffers()}
    torch.optim.Adam(D.parameters(), lr=p.lr_D, betas=(p.beta1, p.beta2), weight_decay=p.weight_decay).step()
    # both sides start the G step from this D rounded to fp32 (tests/test_diffaug_gpu.py)
    out["postD"] = {k: v.detach().float() for k, v in D.state_dict().items()}
    D.load_state_dict({k: v.double() for k, v in out["postD"].items()})
    for q in D.parameters():
        q.requires_grad = False
    y_pred_fake = D(T(G(f["z_G"]), feed["aug_G"][:B]))
    y_real = D(T(f["x_G"], feed["aug_G"][B:])) if kind > 4 else None
    errG = O.head_G(kind, y_pred_fake, y_real, ones, zeros)
    errG.backward()
    out["errG"] = errG.detach()
    out["gradG"] = {n: q.grad.detach().clone() for n, q in G.named_parameters()}
    return out


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_iteration_matches_exact_step(name):
    kw = STEP_CASES[name]
    torch.set_num_threads(4)
    t = _trainer(kw)
    assert t.batch_D == (name != "ralsgan_r1_unbatched") and bool(t.aug) == ("rgan_diffaug" in kw)
    init_G = {k: v.detach().cpu().clone() for k, v in t.G.state_dict().items()}
    init_D = {k: v.detach().cpu().clone() for k, v in t.D.state_dict().items()}
    feed = _step_feed(kw["loss_D"])
    want = _exact_step(kw, init_G, init_D, feed)
    got = {}

    def hook(tag, r):
        if tag == "D":
            got["D"] = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)}
            got["gradD"] = {n: q.grad.detach().clone() for n, q in t.D.named_parameters()}
            got["bufD"] = {k: v.detach().clone() for k, v in t.D.named_buffers()}
        elif tag == "D.post":
            t.D.load_state_dict(want["postD"])
        elif tag == "G":
            got["G"] = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)}
            got["gradG"] = {n: q.grad.detach().clone() for n, q in t.G.named_parameters()}

    t.iteration(1, feed={k: v.to(DEV) for k, v in feed.items()}, hooks=hook)
    t.flush()
    torch.cuda.synchronize()
    report = []

    def check(label, a, b, tol):
        r = _rel(a, b)
        print(f"{name} {label}: rel L2 {r:.2e} (tol {tol:.0e})")
        if not r <= tol:
            report.append(f"{label}: {r:.2e} > {tol:.0e}")

    check("errD", got["D"]["errD"], want["errD"], TOL_OUT)
    check("errG", got["G"]["errG"], want["errG"], TOL_OUT)
    for key in ("gp", "r1", "r2"):
        assert (key in want) == (key in got["D"]), key
        if key in want:
            check(key, got["D"][key], want[key], TOL_OUT)
    assert ("r1" in want) and (("r2" in want) == (name == "rsgan_r1_r2_batched"))
    assert ("gp" in want) == (name == "wgangp_r1")
    for side in ("gradD", "gradG"):
        assert list(got[side]) == list(want[side])
        for n in want[side]:
            check(f"{side}.{n}", got[side][n], want[side][n], TOL_GRAD)
    assert list(got["bufD"]) == list(want["bufD"])
    for k, v in want["bufD"].items():
        if v.is_floating_point():
            check(f"bufD.{k}", got["bufD"][k], v, TOL_BUF)
        else:  # num_batches_tracked: one per call of D, the penalties' included
            assert int(got["bufD"][k]) == int(v), k
    assert not report, report


# ---------------------------------------------------------------- 6. lazy schedule
def _counted(t, run):
    from relativisticgan_amd import _lib as L
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        run(proxy)
        t.flush()
        torch.cuda.synchronize()
    finally:
        L._LIB = real
    return proxy.calls


def test_lazy_schedule():
    t = _trainer(dict(loss_D=7, rgan_r1=1.0, rgan_reg_every=4, Diters=2))
    per_iter = []

    def run(proxy):
        for i in range(5):
            proxy.calls.clear()
            t.iteration(i)
            per_iter.append(dict(proxy.calls))

    _counted(t, run)
    for i, calls in enumerate(per_iter):
        n = 2 if i % 4 == 0 else 0  # Diters each in iterations 0 and 4
        assert calls.get("rgan_gp_zc_penalty", 0) == n and calls.get("rgan_gp_zc_penalty_backward", 0) == n, (i, calls)
    assert "r1" in t.last["D"]  # iteration 4's record
    # iteration 0 of K = 4 weighs the penalty 4x: the same state and feed with K = 1
    feed = {k: v.to(DEV) for k, v in _step_feed(7).items()}
    r1 = {}
    for K in (1, 4):
        u = _trainer(dict(loss_D=7, rgan_r1=1.0, rgan_reg_every=K))
        u.iteration(0, feed=feed, hooks=lambda tag, r, K=K: r1.setdefault(K, r["r1"].clone()) if tag == "D" else None)
        u.flush()
    torch.cuda.synchronize()
    assert _rel(r1[4], 4 * r1[1]) <= TOL_OUT, (r1[4].item(), r1[1].item())
    assert r1[1].item() > 0


# ---------------------------------------------------------------- 7. flags off
OFF_CASES = {"ralsgan_batched": dict(loss_D=7), "wgangp_penalty": dict(loss_D=3),
             "sgan_unbatched": dict(loss_D=1, rgan_batch_D=False)}


@pytest.mark.parametrize("name", sorted(OFF_CASES))
def test_flags_off_make_no_new_call(name):
    t = _trainer(OFF_CASES[name])
    assert (t.r1, t.r2, t.reg_every) == (0.0, 0.0, 1)
    calls = _counted(t, lambda proxy: t.iteration(1))
    assert calls.get("rgan_conv_fwd", 0) + calls.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    assert not [n for n in NEW if n in calls], calls
    wgan = name == "wgangp_penalty"
    assert (calls.get("rgan_gp_penalty", 0), calls.get("rgan_gp_penalty_backward", 0),
            calls.get("rgan_gp_interp", 0)) == ((1, 1, 1) if wgan else (0, 0, 0))
    assert "r1" not in t.last["D"] and "r2" not in t.last["D"]
    # on: the one-centred penalty keeps its own kernels, the zero-centred one adds its pair
    u = _trainer(dict(OFF_CASES[name], rgan_r1=1.0, rgan_r2=1.0))
    on = _counted(u, lambda proxy: u.iteration(1))
    assert (on.get("rgan_gp_zc_penalty", 0), on.get("rgan_gp_zc_penalty_backward", 0)) == (2, 2)
    assert (on.get("rgan_gp_penalty", 0), on.get("rgan_gp_interp", 0)) == ((1, 1) if wgan else (0, 0))


# ---------------------------------------------------------------- 8. data parallel
def test_dp2_syncbn_matches_single_process():
    from tests.test_dp_gpu import _compare, _run, _spawn
    over = dict(rgan_r1=1.0, rgan_r2=1.0)
    single = _run("ralsgan", 1, 0, overrides=over)
    dpres = _spawn("ralsgan", overrides=over)
    _compare("ralsgan", dpres, single)


def test_dp2_per_shard_bn_runs():
    """Per-shard statistics are not the global-batch maths: finite, and shaped like the
    single-process step (the reducer armed exactly once per D step, or finish() would raise)."""
    from tests.test_dp_gpu import _run, _spawn
    over = dict(rgan_r1=1.0, rgan_r2=1.0)
    single = _run("ralsgan", 1, 0, n_iter=1, overrides=over)
    dpres = _spawn("ralsgan", sync_bn=False, n_iter=1, overrides=over)
    assert len(dpres) == len(single) == 1
    a, b = dpres[0], single[0]
    assert a["errD"].shape == b["errD"].shape and torch.isfinite(a["errD"]).all()
    assert list(a["gradD"]) == list(b["gradD"])
    for n in b["gradD"]:
        assert a["gradD"][n].shape == b["gradD"][n].shape and torch.isfinite(a["gradD"][n]).all(), n


# ---------------------------------------------------------------- 9. CLI
def test_train_cli_runs_checkpoints_and_resumes_on_schedule():
    from relativisticgan_amd.train import main
    root = tempfile.mkdtemp()
    out, extra = os.path.join(root, "out"), os.path.join(root, "extra")
    common = ["--loss_D", "7", *TINY_CLI, "--batch_size", "8", "--D_h_size", "8", "--seed", "1", "--gen_every", "3",
              "--gen_extra_images", "0", "--output_folder", out, "--extra_folder", extra, "--rgan_synthetic", "64",
              "--rgan_r1", "1", "--rgan_reg_every", "2"]
    r = subprocess.run([sys.executable, "-m", "relativisticgan_amd.train", *common, "--n_iter", "3"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Models saved" in r.stdout
    path = os.path.join(extra, "models", "state_01.pth")
    ck = torch.load(path, weights_only=True)
    assert ck["i"] == 3
    # resumed at iteration 3, the run does iterations 3 and 4: the rule names 4 only
    seen = {}
    calls = _counted(_Flush(), lambda proxy: seen.setdefault("t", main([*common, "--n_iter", "5", "--load", path])))
    assert calls.get("rgan_gp_zc_penalty", 0) == 1 and calls.get("rgan_gp_zc_penalty_backward", 0) == 1, calls
    assert "r1" in seen["t"].last["D"]


class _Flush:
    def flush(self):
        pass
