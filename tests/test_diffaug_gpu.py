"""--rgan_diffaug on the MI355X: the HIP transform and its adjoint (csrc/augment.hip) against
the float64 restatement (tests/diffaug_ref.py), their exactness and determinism, the adjoint
identity, the rgan::diffaug operator, graph capture, and one D + G training iteration with
augmentation on against an exact float64 step built here from the oracle's nets and heads.

Kernel bound: |err| <= 1e-5 max(1, |ref|).  Inputs are in [-1, 1) (the images' range), so every
value is O(1); a result is about ten fp32 operations and one mean, i.e. about 2e-6 of rounding,
and the bound is about five times that.
"""
import functools

import pytest
import torch

from tests import diffaug_ref as ref
from tests.test_parity_gpu import TOL_GRAD, TOL_OUT, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, H, W).  The first five are the sizes D sees plus small odd ones; (2, 3, 256, 256) is the
# multi-block reduction.  The last three take the kernel's other paths: a width that is no
# multiple of 4 (scalar loads and stores), more than 4 channels (two reads instead of
# registers), and a non-square image with an odd height.
SHAPES = [(5, 3, 8, 8), (3, 1, 16, 16), (4, 3, 32, 32), (2, 3, 64, 64), (2, 3, 256, 256),
          (3, 3, 10, 10), (2, 5, 12, 12), (2, 2, 9, 20)]
U_KINDS = ("rand", "lo", "hi")
ONE_BELOW = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _u(B, kind, gen):
    if kind == "lo":
        return torch.zeros(B, 8, device=DEV)
    if kind == "hi":
        return torch.full((B, 8), ONE_BELOW, device=DEV)
    return torch.rand(B, 8, device=DEV, generator=gen)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.rand(shape, device=DEV, generator=gen) * 2 - 1
    dy = torch.rand(shape, device=DEV, generator=gen) * 2 - 1
    return x, dy, {k: _u(shape[0], k, gen) for k in U_KINDS}


@functools.lru_cache(maxsize=None)
def _run(shape, policy, kind):
    """(y, dx) of the HIP kernels for one case (shared, never modified)."""
    from relativisticgan_amd import kernels as K
    x, dy, us = _inputs(shape)
    return K.diffaug(x, us[kind], policy), K.diffaug(dy, us[kind], policy, adjoint=True)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_and_adjoint_match_fp64_restatement(shape):
    x, dy, us = _inputs(shape)
    worst = 0.0
    for policy in range(8):
        for kind in U_KINDS:
            y, dx = _run(shape, policy, kind)
            for name, got, want in (("forward", y, ref.forward(x.double(), us[kind], policy)),
                                    ("adjoint", dx, ref.adjoint(dy.double(), us[kind], policy))):
                excess = ((got.double() - want).abs() / want.abs().clamp_min(1.0)).max().item()
                worst = max(worst, excess)
                assert excess <= 1e-5, (shape, policy, kind, name, excess)
    print(f"diffaug {shape}: worst |err| / max(1, |ref|) = {worst:.2e}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_moves_are_exact(shape):
    """Policy 0 is a bitwise copy; without the colour bit every output is a copied input or 0
    (bitwise the fp32 restatement); what is cut out or shifted in is exactly 0 under every policy."""
    x, dy, us = _inputs(shape)
    for kind in U_KINDS:
        y0, dx0 = _run(shape, 0, kind)
        assert torch.equal(_bits(y0), _bits(x)) and torch.equal(_bits(dx0), _bits(dy))
        for policy in (2, 4, 6):
            y, dx = _run(shape, policy, kind)
            assert torch.equal(_bits(y), _bits(ref.forward(x, us[kind], policy))), (policy, kind)
            assert torch.equal(_bits(dx), _bits(ref.adjoint(dy, us[kind], policy))), (policy, kind)
        for policy in range(8):
            keep = ref.keep_mask(us[kind], shape, policy)
            y = _run(shape, policy, kind)[0]
            assert (_bits(y)[~keep] == 0).all(), (policy, kind)  # +0.0, bit for bit
            if policy & 6 and kind != "rand":
                assert not keep.all()  # the extreme parameters do mask something


@pytest.mark.parametrize("shape", [(2, 3, 256, 256), (4, 3, 32, 32), (3, 3, 10, 10)], ids=_ids)
def test_two_calls_give_the_same_bits(shape):
    from relativisticgan_amd import kernels as K
    x, dy, us = _inputs(shape)
    for policy in (1, 7):
        y, dx = _run(shape, policy, "rand")
        assert torch.equal(_bits(K.diffaug(x, us["rand"], policy)), _bits(y))
        assert torch.equal(_bits(K.diffaug(dy, us["rand"], policy, adjoint=True)), _bits(dx))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_adjoint_identity_on_gpu_outputs(shape):
    """<T_lin x, w> = <x, T^t w> with both sides from the kernels and the dot products in
    float64; T_lin x = T(x) - T(0).  w = T_lin x + noise, so the products do not cancel and the
    relative difference is measured against a number of the operands' own size."""
    from relativisticgan_amd import kernels as K
    x, noise, us = _inputs(shape)
    for policy in range(1, 8):
        for kind in U_KINDS:
            u = us[kind]
            lin = K.diffaug(x, u, policy).double() - K.diffaug(torch.zeros_like(x), u, policy).double()
            w = (lin + 0.5 * noise.double()).float()
            lhs = (lin * w.double()).sum().item()
            rhs = (x.double() * K.diffaug(w, u, policy, adjoint=True).double()).sum().item()
            assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (shape, policy, kind, lhs, rhs)


def test_out_buffer_and_argument_checks():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd._lib import RganError
    x, _, us = _inputs((4, 3, 32, 32))
    u = us["rand"]
    pair = torch.full((8, 3, 32, 32), 7.0, device=DEV)
    K.diffaug(x, u, 7, out=pair[4:])
    assert torch.equal(pair[4:], _run((4, 3, 32, 32), 7, "rand")[0]) and (pair[:4] == 7).all()
    # a source that is not 16-byte aligned takes the scalar kernels: same values
    shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)
    assert shifted.data_ptr() % 16 != 0
    y = K.diffaug(shifted, u, 7)
    assert ((y - pair[4:]).abs() <= 1e-5).all() and torch.equal(y == 0, pair[4:] == 0)
    with pytest.raises(RganError):
        K.diffaug(x, u, 8)
    with pytest.raises(RganError):
        K.diffaug(x, u, 7, out=x)
    with pytest.raises(RganError):
        K.diffaug(x, u[:2], 7)
    with pytest.raises(RganError):
        K.diffaug(x.cpu(), u.cpu(), 7)


def test_opcheck_and_autograd_is_the_adjoint():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd import ops  # noqa: F401  (registers rgan::)
    x, dy, us = _inputs((4, 3, 32, 32))
    u = us["rand"]
    xg = x.clone().requires_grad_(True)
    checks = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.rgan.diffaug.default, (xg, u, 7), test_utils=checks)
    torch.library.opcheck(torch.ops.rgan.diffaug_backward.default, (dy, u, 7),
                          test_utils=("test_schema", "test_faketensor"))
    y = torch.ops.rgan.diffaug(xg, u, 7)
    assert torch.equal(y, _run((4, 3, 32, 32), 7, "rand")[0])
    dyg = dy.clone().requires_grad_(True)
    gx, = torch.autograd.grad(y, xg, dyg, create_graph=True)
    assert torch.equal(gx, K.diffaug(dy, u, 7, adjoint=True))
    with pytest.raises(NotImplementedError):  # the backward of the backward is not registered
        torch.autograd.grad(gx.sum(), dyg)
    # the training step's node: the same gradient, with the output written into a buffer
    from relativisticgan_amd import augment
    buf = torch.empty_like(x)
    y2 = augment.apply(xg, u, 7, out=buf)
    assert y2.data_ptr() == buf.data_ptr() and torch.equal(y2, y)
    gx2, = torch.autograd.grad(y2, xg, dy)
    assert torch.equal(gx2, gx)


def test_captured_call_reads_the_new_uniforms():
    from relativisticgan_amd import kernels as K
    x, _, us = _inputs((4, 3, 32, 32))
    u = us["rand"].clone()
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.diffaug(x, u, 7, out=out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        K.diffaug(x, u, 7, out=out)
    gen = torch.Generator(device=DEV).manual_seed(99)
    new_u = torch.rand(4, 8, device=DEV, generator=gen)
    with torch.cuda.stream(side):
        u.copy_(new_u)
        out.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(K.diffaug(x, new_u, 7)))
    assert not torch.equal(out, _run((4, 3, 32, 32), 7, "rand")[0])


# ------------------------------------------------------------------ the training step
STEP = dict(image_size=32, batch_size=6, G_h_size=8, D_h_size=8, z_size=16, Tanh_GD=True, seed=1)
STEP_CASES = {
    "ralsgan_batched": dict(loss_D=7),
    "wgangp_penalty": dict(loss_D=3),
    "sgan_unbatched": dict(loss_D=1, rgan_batch_D=False),
}
POLICY = "color,translation,cutout"


def _trainer(kw, policy):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    p = make_param(print_every=10 ** 9, rgan_diffaug=policy, **STEP, **kw)
    return Trainer(p, synthetic_images(64, 32, device=DEV))


def _step_feed(kind):
    gen = torch.Generator().manual_seed(17)
    B = STEP["batch_size"]
    f = {"x_D": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, "z_D": torch.randn(B, 16, 1, 1, generator=gen),
         "aug_D": torch.rand(2 * B, 8, generator=gen), "u": torch.rand(B, 1, 1, 1, generator=gen),
         "z_G": torch.randn(B, 16, 1, 1, generator=gen), "x_G": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1,
         "aug_G": torch.rand((2 if kind > 4 else 1) * B, 8, generator=gen)}
    return f


def _exact_step(kw, init_G, init_D, feed):
    """The iteration in float64 on the host: the oracle's nets and heads, the restated transform,
    torch autograd for the penalty, torch's Adam for the D step in between."""
    from oracle import reference_cpu as O
    from relativisticgan_amd.augment import parse_policy
    mask = parse_policy(POLICY)
    p = O.make_param(cuda=False, **STEP, **{k: v for k, v in kw.items() if not k.startswith("rgan_")})
    G, D = O.build_G(p).double(), O.build_D(p).double()
    G.load_state_dict({k: v.double() for k, v in init_G.items()})
    D.load_state_dict({k: v.double() for k, v in init_D.items()})
    f = {k: v.double() for k, v in feed.items()}
    kind, B = p.loss_D, p.batch_size
    ones, zeros = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    out = {}
    # D step: x and the detached G(z) transformed with the two row groups of aug_D
    x_t = ref.forward(f["x_D"], feed["aug_D"][:B], mask)
    fake_t = ref.forward(G(f["z_D"]).detach(), feed["aug_D"][B:], mask)
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
    # both sides start the G step from this D rounded to fp32 (Adam's first step is a sign step:
    # an fp32 D step differs from it by +-lr wherever a gradient is near 0, as test_parity_gpu notes)
    out["postD"] = {k: v.detach().float() for k, v in D.state_dict().items()}
    D.load_state_dict({k: v.double() for k, v in out["postD"].items()})
    for q in D.parameters():
        q.requires_grad = False
    # G step: T(G(z)) with autograd; heads 5-8 also see a transformed fresh real batch
    y_pred_fake = D(ref.forward(G(f["z_G"]), feed["aug_G"][:B], mask))
    y_real = D(ref.forward(f["x_G"], feed["aug_G"][B:], mask)) if kind > 4 else None
    errG = O.head_G(kind, y_pred_fake, y_real, ones, zeros)
    errG.backward()
    out["errG"] = errG.detach()
    out["gradG"] = {n: q.grad.detach().clone() for n, q in G.named_parameters()}
    return out


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_iteration_with_augmentation_matches_exact_step(name):
    kw = STEP_CASES[name]
    torch.set_num_threads(4)
    t = _trainer(kw, POLICY)
    assert t.aug == 7 and t.batch_D == (name != "sgan_unbatched")
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
    # the record keeps the untransformed batch; what D saw is the transform of it
    B = STEP["batch_size"]
    assert torch.equal(got["D"]["x"].cpu(), feed["x_D"])
    assert _rel(got["D"]["x_aug"], ref.forward(feed["x_D"].double(), feed["aug_D"][:B], 7)) <= 1e-5


class _Counter:
    """The C-ABI library behind a proxy that counts calls per entry point (the approach of
    tools/abi_trace.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rgan_"):
            return fn

        def wrapped(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return wrapped


def _count_calls(policy, kw):
    from relativisticgan_amd import _lib as L
    t = _trainer(kw, policy)
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
def test_flag_off_makes_no_diffaug_call(name):
    kw = STEP_CASES[name]
    off, on = _count_calls("", kw), _count_calls(POLICY, kw)
    assert off.get("rgan_conv_fwd", 0) + off.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    assert "rgan_diffaug" not in off and "rgan_diffaug_workspace" not in off, off
    # on: forward calls of the D step (one over the pair on the batched path, else two) and of
    # the G step (fake, and the real batch for heads 5-8), plus one adjoint call into G
    batched_D = name != "sgan_unbatched"
    want = (1 if batched_D else 2) + (2 if kw["loss_D"] > 4 else 1) + 1
    assert on.get("rgan_diffaug", 0) == want, on
    rest = {k: v for k, v in on.items() if not k.startswith("rgan_diffaug")}
    assert rest == off, {k: (off.get(k), rest.get(k)) for k in set(off) | set(rest) if off.get(k) != rest.get(k)}
