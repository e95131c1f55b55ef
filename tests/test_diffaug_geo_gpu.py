"""The geometric groups of --rgan_diffaug (xflip, rot90, warp) on the MI355X: the HIP resampler and
its adjoint (csrc/augment_geo.hip) against the float64 restatement (tests/diffaug_geo_ref.py),
their exactness and determinism, the adjoint identity, gating, the rgan::diffaug_geo operators,
graph capture, and one D + G training iteration with all six groups on and --rgan_aug_p 0.5
against an exact float64 step built here from the oracle's nets and heads.

Kernel bound: |err| <= 1e-5 max(1, |ref|), tests/test_diffaug_gpu.py's.  Inputs are in [-1, 1), so
every value is O(1).  The sampling coordinates are computed in double, so the four tap weights
are correctly rounded floats; a gathered value is then 4 products and 3 sums in fp32 (the adjoint
up to 16), and the colour map about ten more operations and one mean: about 3e-6 of rounding.
"""
import functools

import pytest
import torch

from tests import diffaug_geo_ref as ref
from tests.test_diffaug_gpu import STEP, STEP_CASES, _Counter
from tests.test_parity_gpu import TOL_GRAD, TOL_OUT, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, H, W): small images; a width that is no multiple of 4 (scalar stores); more than 4
# channels (two gathers instead of registers); a non-square image (run with the rot90 bit
# cleared); the multi-block reduction
SHAPES = [(5, 3, 8, 8), (3, 1, 16, 16), (4, 3, 32, 32), (3, 3, 10, 10), (2, 5, 12, 12), (2, 2, 9, 20),
          (2, 3, 256, 256)]
V_KINDS = ("rand", "lo", "hi", "id")
POLICIES = (8, 16, 32, 24, 26, 33, 56, 57, 62, 63)
ONE_BELOW = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
ALL_SIX = "color,translation,cutout,xflip,rot90,warp"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _policies(shape):
    """POLICIES, the rot90 bit cleared on a non-square image (duplicates and 0 dropped)."""
    if shape[2] == shape[3]:
        return POLICIES
    return tuple(dict.fromkeys(p & ~16 for p in POLICIES if p & ~16))


def _v(B, kind, gen):
    if kind == "lo":  # no flip, k = 0, smallest s, theta = -pi
        return torch.zeros(B, 8, device=DEV)
    if kind == "hi":  # flip, k = 3, largest s
        return torch.full((B, 8), ONE_BELOW, device=DEV)
    if kind == "id":  # s = 1, theta = 0
        return torch.tensor([[0, 0, .5, .5, 0, 0, 0, 0]], dtype=torch.float32, device=DEV).repeat(B, 1)
    return torch.rand(B, 8, device=DEV, generator=gen)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.rand(shape, device=DEV, generator=gen) * 2 - 1
    dy = torch.rand(shape, device=DEV, generator=gen) * 2 - 1
    u = torch.rand(shape[0], 8, device=DEV, generator=gen)
    return x, dy, u, {k: _v(shape[0], k, gen) for k in V_KINDS}


def _call(t, u, v, policy, **kw):
    from relativisticgan_amd import kernels as K
    return K.diffaug(t, u, policy, geo=v if policy >= 8 else None, **kw)


@functools.lru_cache(maxsize=None)
def _run(shape, policy, kind):
    """(y, dx) of the HIP kernels for one case (shared, never modified)."""
    x, dy, u, vs = _inputs(shape)
    return _call(x, u, vs[kind], policy), _call(dy, u, vs[kind], policy, adjoint=True)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_and_adjoint_match_fp64_restatement(shape):
    x, dy, u, vs = _inputs(shape)
    worst = 0.0
    for policy in _policies(shape):
        for kind in V_KINDS:
            y, dx = _run(shape, policy, kind)
            for name, got, want in (("forward", y, ref.forward(x.double(), u, vs[kind], policy)),
                                    ("adjoint", dx, ref.adjoint(dy.double(), u, vs[kind], policy))):
                excess = ((got.double() - want).abs() / want.abs().clamp_min(1.0)).max().item()
                worst = max(worst, excess)
                assert excess <= 1e-5, (shape, policy, kind, name, excess)
    print(f"diffaug_geo {shape}: worst |err| / max(1, |ref|) = {worst:.2e}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_integer_paths_are_exact(shape):
    """Without the colour and warp bits every output is a copied input or 0 (bitwise the fp32
    restatement); the identity row under the warp bit is bitwise the call without that bit; what
    translation and cutout do not keep is +0.0 under every policy."""
    x, dy, u, vs = _inputs(shape)
    for policy in _policies(shape):
        for kind in V_KINDS:
            y, dx = _run(shape, policy, kind)
            if not policy & 33:
                assert torch.equal(_bits(y), _bits(ref.forward(x, u, vs[kind], policy))), (policy, kind)
                assert torch.equal(_bits(dx), _bits(ref.adjoint(dy, u, vs[kind], policy))), (policy, kind)
            keep = ref.keep_mask(u, shape, policy)
            assert (_bits(y)[~keep] == 0).all(), (policy, kind)  # +0.0, bit for bit
        if policy & 32:
            y, dx = _run(shape, policy, "id")
            assert torch.equal(_bits(y), _bits(_call(x, u, vs["id"], policy & ~32))), policy
            assert torch.equal(_bits(dx), _bits(_call(dy, u, vs["id"], policy & ~32, adjoint=True))), policy


def test_two_calls_give_the_same_bits():
    shape = (2, 3, 256, 256)
    x, dy, u, vs = _inputs(shape)
    y, dx = _run(shape, 63, "rand")
    assert torch.equal(_bits(_call(x, u, vs["rand"], 63)), _bits(y))
    assert torch.equal(_bits(_call(dy, u, vs["rand"], 63, adjoint=True)), _bits(dx))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_adjoint_identity_on_gpu_outputs(shape):
    """<T_lin x, w> = <x, T^t w> with both sides from the kernels and the dot products in
    float64; T_lin x = T(x) - T(0).  w = T_lin x + noise, so the products do not cancel and the
    relative difference is measured against a number of the operands' own size."""
    x, noise, u, vs = _inputs(shape)
    for policy in _policies(shape):
        for kind in V_KINDS:
            v = vs[kind]
            lin = _call(x, u, v, policy).double() - _call(torch.zeros_like(x), u, v, policy).double()
            w = (lin + 0.5 * noise.double()).float()
            lhs = (lin * w.double()).sum().item()
            rhs = (x.double() * _call(w, u, v, policy, adjoint=True).double()).sum().item()
            assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (shape, policy, kind, lhs, rhs)


def _p(value):
    return torch.tensor([value], dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("shape", [(5, 3, 8, 8), (4, 3, 32, 32), (3, 3, 10, 10), (2, 3, 256, 256)], ids=_ids)
def test_gated_calls(shape):
    """p = 0: a bit copy; p = 1: the ungated bits; in between, sample b equals bit for bit an
    ungated call on that sample with the groups its gates open."""
    x, dy, u, vs = _inputs(shape)
    v = vs["rand"]
    B = shape[0]
    gate = torch.rand(B, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    for policy in (24, 33, 63):
        for t, adjoint in ((x, False), (dy, True)):
            assert torch.equal(_bits(_call(t, u, v, policy, adjoint=adjoint, gate=gate, p=_p(0.0))), _bits(t))
            assert torch.equal(_bits(_call(t, u, v, policy, adjoint=adjoint, gate=gate, p=_p(1.0))),
                               _bits(_run(shape, policy, "rand")[int(adjoint)]))
            for p in (0.3, 0.6):
                got = _call(t, u, v, policy, adjoint=adjoint, gate=gate, p=_p(p))
                masks = ref.open_masks(policy, gate, v, p)
                for b in range(B):
                    one = _call(t[b:b + 1], u[b:b + 1], v[b:b + 1], masks[b], adjoint=adjoint)
                    assert torch.equal(_bits(got[b:b + 1]), _bits(one)), (policy, adjoint, p, b, masks[b])
    assert len({m for p in (0.3, 0.6) for m in ref.open_masks(63, gate, v, p)}) > 1  # the gates do differ


def test_policy_below_8_is_rgan_diffaug():
    """rgan_diffaug_geo with no geometric bit, called directly: rgan_diffaug's / rgan_diffaug_p's bits."""
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import kernels as K
    shape = (4, 3, 32, 32)
    x, dy, u, vs = _inputs(shape)
    gate = torch.rand(4, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    p = _p(0.5)
    lib = L.lib()
    ws = torch.empty(int(lib.rgan_diffaug_geo_workspace(*shape)), device=DEV)
    for policy in range(8):
        for t, adjoint in ((x, 0), (dy, 1)):
            for g, q in ((None, None), (gate, p)):
                out = torch.empty_like(t)
                for v in (vs["rand"], None):  # v is not read
                    L.check(lib.rgan_diffaug_geo(L.ptr(t), L.ptr(u), L.ptr(v), L.ptr(g), L.ptr(q), *shape, policy,
                                                 adjoint, L.ptr(ws), L.ptr(out), L.stream()), "rgan_diffaug_geo")
                    want = K.diffaug(t, u, policy, adjoint=bool(adjoint), gate=g, p=q)
                    assert torch.equal(_bits(out), _bits(want)), (policy, adjoint, g is not None)


def test_out_buffer_and_argument_checks():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd._lib import RganError
    shape = (4, 3, 32, 32)
    x, _, u, vs = _inputs(shape)
    v = vs["rand"]
    pair = torch.full((8, 3, 32, 32), 7.0, device=DEV)
    K.diffaug(x, u, 63, out=pair[4:], geo=v)
    assert torch.equal(pair[4:], _run(shape, 63, "rand")[0]) and (pair[:4] == 7).all()
    # a source that is not 16-byte aligned takes the scalar kernels: same values
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)
    assert shifted.data_ptr() % 16 != 0
    y = K.diffaug(shifted, u, 63, geo=v)
    assert ((y - pair[4:]).abs() <= 1e-5).all()
    for bad in (dict(policy=64), dict(policy=63, geo=None), dict(policy=63, geo=v[:2]),
                dict(policy=63, geo=v.double()), dict(policy=63, geo=v.cpu()), dict(policy=63, out=x),
                dict(policy=63, gate=torch.rand(4, 4, device=DEV))):
        kw = dict(dict(geo=v), **bad)
        with pytest.raises(RganError):
            K.diffaug(x, u, kw.pop("policy"), **kw)
    with pytest.raises(RganError):
        K.diffaug(x.cpu(), u.cpu(), 63, geo=v.cpu())
    xr, _, ur, vr = _inputs((2, 2, 9, 20))
    for policy in (16, 24, 63):  # quarter turns need a square image
        with pytest.raises(RganError):
            K.diffaug(xr, ur, policy, geo=vr["rand"])


def test_opcheck_and_autograd_is_the_adjoint():
    from relativisticgan_amd import augment
    from relativisticgan_amd import ops  # noqa: F401  (registers rgan::)
    shape = (4, 3, 32, 32)
    x, dy, u, vs = _inputs(shape)
    v = vs["rand"]
    gate, p = torch.rand(4, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)), _p(0.5)
    xg = x.clone().requires_grad_(True)
    checks = ("test_schema", "test_autograd_registration", "test_faketensor")
    for extra in ((), (gate, p)):
        torch.library.opcheck(torch.ops.rgan.diffaug_geo.default, (xg, u, v, 63, *extra), test_utils=checks)
        torch.library.opcheck(torch.ops.rgan.diffaug_geo_backward.default, (dy, u, v, 63, *extra),
                              test_utils=("test_schema", "test_faketensor"))
        kw = dict(gate=extra[0], p=extra[1]) if extra else {}
        y = torch.ops.rgan.diffaug_geo(xg, u, v, 63, *extra)
        assert torch.equal(y, _call(x, u, v, 63, **kw))
        dyg = dy.clone().requires_grad_(True)
        gx, = torch.autograd.grad(y, xg, dyg, create_graph=True)
        assert torch.equal(gx, _call(dy, u, v, 63, adjoint=True, **kw))
        with pytest.raises(NotImplementedError):  # the backward of the backward is not registered
            torch.autograd.grad(gx.sum(), dyg)
        # the training step's node: the same gradient, with the output written into a buffer
        buf = torch.empty_like(x)
        y2 = augment.apply(xg, u, 63, out=buf, geo=v, **kw)
        assert y2.data_ptr() == buf.data_ptr() and torch.equal(y2, y)
        gx2, = torch.autograd.grad(y2, xg, dy)
        assert torch.equal(gx2, gx)


def test_captured_call_reads_the_new_uniforms():
    shape = (4, 3, 32, 32)
    x, _, u, vs = _inputs(shape)
    v = vs["rand"].clone()
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(x, u, v, 63, out=out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _call(x, u, v, 63, out=out)
    new_v = torch.rand(4, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(99))
    with torch.cuda.stream(side):
        v.copy_(new_v)
        out.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(_call(x, u, new_v, 63)))
    assert not torch.equal(out, _run(shape, 63, "rand")[0])


# ------------------------------------------------------------------ the training step
AUG_P = 0.5
B = STEP["batch_size"]


def _trainer(kw, policy, **more):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    p = make_param(print_every=10 ** 9, rgan_diffaug=policy, **STEP, **kw, **more)
    return Trainer(p, synthetic_images(64, 32, device=DEV))


def _step_feed(kind):
    gen = torch.Generator().manual_seed(23)
    n = (2 if kind > 4 else 1) * B
    return {"x_D": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, "z_D": torch.randn(B, 16, 1, 1, generator=gen),
            "aug_D": torch.rand(2 * B, 8, generator=gen), "gate_D": torch.rand(2 * B, 4, generator=gen),
            "geo_D": torch.rand(2 * B, 8, generator=gen), "u": torch.rand(B, 1, 1, 1, generator=gen),
            "z_G": torch.randn(B, 16, 1, 1, generator=gen), "x_G": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1,
            "aug_G": torch.rand(n, 8, generator=gen), "gate_G": torch.rand(n, 4, generator=gen),
            "geo_G": torch.rand(n, 8, generator=gen)}


def _ref_gated(x, feed, side, rows):
    """The restated transform of x under rows ``rows`` of the side's draws, every sample with the
    groups its gates open at AUG_P."""
    u, gate, v = (feed[k + side][rows] for k in ("aug_", "gate_", "geo_"))
    masks = ref.open_masks(63, gate, v, AUG_P)
    return torch.cat([ref.forward(x[b:b + 1], u[b:b + 1], v[b:b + 1], masks[b]) for b in range(x.shape[0])])


def _exact_step(kw, init_G, init_D, feed):
    """The iteration in float64 on the host, as tests/test_diffaug_gpu.py builds it: the oracle's
    nets and heads, the restated transform, torch autograd for the penalty, torch's Adam for the D
    step in between."""
    from oracle import reference_cpu as O
    p = O.make_param(cuda=False, **STEP, **{k: v for k, v in kw.items() if not k.startswith("rgan_")})
    G, D = O.build_G(p).double(), O.build_D(p).double()
    G.load_state_dict({k: v.double() for k, v in init_G.items()})
    D.load_state_dict({k: v.double() for k, v in init_D.items()})
    f = {k: v.double() for k, v in feed.items()}
    kind = p.loss_D
    ones, zeros = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    lo, hi = slice(0, B), slice(B, None)
    out = {}
    x_t = _ref_gated(f["x_D"], feed, "D", lo)
    fake_t = _ref_gated(G(f["z_D"]).detach(), feed, "D", hi)
    out["x_aug"] = x_t
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
    if kind == 3 or p.grad_penalty:  # the penalty interpolates what D saw
        gp = O.gradient_penalty(D, x_t, fake_t, f["u"], p.penalty, ones)
        gp.backward()
        out["gp"] = gp.detach()
    out["gradD"] = {n: q.grad.detach().clone() for n, q in D.named_parameters()}
    torch.optim.Adam(D.parameters(), lr=p.lr_D, betas=(p.beta1, p.beta2), weight_decay=p.weight_decay).step()
    # both sides start the G step from this D rounded to fp32 (as tests/test_diffaug_gpu.py notes)
    out["postD"] = {k: v.detach().float() for k, v in D.state_dict().items()}
    D.load_state_dict({k: v.double() for k, v in out["postD"].items()})
    for q in D.parameters():
        q.requires_grad = False
    y_pred_fake = D(_ref_gated(G(f["z_G"]), feed, "G", lo))
    y_real = D(_ref_gated(f["x_G"], feed, "G", hi)) if kind > 4 else None
    errG = O.head_G(kind, y_pred_fake, y_real, ones, zeros)
    errG.backward()
    out["errG"] = errG.detach()
    out["gradG"] = {n: q.grad.detach().clone() for n, q in G.named_parameters()}
    return out


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_iteration_with_all_six_groups_matches_exact_step(name):
    kw = STEP_CASES[name]
    torch.set_num_threads(4)
    t = _trainer(kw, ALL_SIX, rgan_aug_p=AUG_P)
    assert t.aug == 63 and t.ada is not None and t.batch_D == (name != "sgan_unbatched")
    init_G = {k: v.detach().cpu().clone() for k, v in t.G.state_dict().items()}
    init_D = {k: v.detach().cpu().clone() for k, v in t.D.state_dict().items()}
    feed = _step_feed(kw["loss_D"])
    want = _exact_step(kw, init_G, init_D, feed)
    got = {}

    def hook(tag, r):
        if tag == "D":
            got["D"] = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)}
            got["gradD"] = {n: q.grad.detach().clone() for n, q in t.D.named_parameters()}
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
    assert ("gp" in want) == (name == "wgangp_penalty")
    if "gp" in want:
        check("gp", got["D"]["gp"], want["gp"], TOL_OUT)
    for side in ("gradD", "gradG"):
        assert list(got[side]) == list(want[side])
        for n in want[side]:
            check(f"{side}.{n}", got[side][n], want[side][n], TOL_GRAD)
    assert not report, report
    # the record keeps the untransformed batch and the draws; what D saw is the transform of it
    assert torch.equal(got["D"]["x"].cpu(), feed["x_D"]) and torch.equal(got["D"]["geo"].cpu(), feed["geo_D"])
    assert torch.equal(got["G"]["geo"].cpu(), feed["geo_G"])
    assert _rel(got["D"]["x_aug"], want["x_aug"]) <= 1e-5


def _count_calls(policy, kw, **more):
    from relativisticgan_amd import _lib as L
    t = _trainer(kw, policy, **more)
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        t.iteration(1)
        t.flush()
        torch.cuda.synchronize()
    finally:
        L._LIB = real
    return proxy.calls


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_call_counts(name):
    kw = STEP_CASES[name]
    off = _count_calls("", kw)
    old = _count_calls("color,translation,cutout", kw)
    geo = _count_calls(ALL_SIX, kw)
    assert off.get("rgan_conv_fwd", 0) + off.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    # the three older groups alone: no call of the new entry points, and the calls they always made
    # (the D step's forward, one over the pair on the batched path; the G step's fake and, for heads
    # 5-8, real batch; one adjoint into G)
    assert not [k for k in old if k.startswith("rgan_diffaug_geo")], old
    want = (1 if name != "sgan_unbatched" else 2) + (2 if kw["loss_D"] > 4 else 1) + 1
    assert old.get("rgan_diffaug", 0) == want and old.get("rgan_diffaug_workspace", 0) == want, old
    # a geometric policy: the same number of calls, all of them to the new entry point
    assert geo.get("rgan_diffaug_geo", 0) == want and geo.get("rgan_diffaug_geo_workspace", 0) == want, geo
    assert "rgan_diffaug" not in geo and "rgan_diffaug_p" not in geo and "rgan_diffaug_workspace" not in geo, geo
    for calls in (old, geo):
        rest = {k: v for k, v in calls.items() if not k.startswith("rgan_diffaug")}
        assert rest == off, {k: (off.get(k), rest.get(k)) for k in set(off) | set(rest) if off.get(k) != rest.get(k)}


def test_geo_draw_comes_last():
    """Two trainers with the same seed and the device generator, one with ``color`` and one with
    ``color,xflip``: the same x, z and u in iteration 1 (the geometric rows are drawn after them)."""
    recs = []
    for policy in ("color", "color,xflip"):
        t = _trainer(STEP_CASES["ralsgan_batched"], policy, rgan_rng="device")

        def hook(tag, r, keep=("x", "z", "aug", "geo")):
            if tag == "D":
                recs.append({k: r[k].detach().clone() for k in keep if k in r})

        t.iteration(1, hooks=hook)
        t.flush()
        torch.cuda.synchronize()
    a, b = recs
    assert "geo" not in a and b["geo"].shape == (2 * B, 8)
    for k in ("x", "z", "aug"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
