"""--rgan_diffaug without a GPU: the restated transform's adjoint is its autograd derivative and
satisfies the adjoint identity in float64 (so the GPU tests can trust it), the policy parsing,
and the C-ABI's argument checks (rejected on the host, before any launch)."""
import ctypes

import pytest
import torch

from tests import diffaug_ref as ref

SHAPES = [(5, 3, 8, 8), (3, 1, 16, 16), (2, 3, 10, 12), (2, 5, 9, 7)]


def _u(B, kind, gen):
    if kind == "lo":
        return torch.zeros(B, 8)
    if kind == "hi":
        return torch.full((B, 8), float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))))
    return torch.rand(B, 8, generator=gen)


@pytest.mark.parametrize("policy", range(8))
def test_reference_adjoint_is_autograd_and_transpose(policy):
    gen = torch.Generator().manual_seed(policy)
    for shape in SHAPES:
        for kind in ("rand", "lo", "hi"):
            u = _u(shape[0], kind, gen)
            x = (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
            dy = torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1
            y = ref.forward(x, u, policy)
            gx, = torch.autograd.grad(y, x, dy)
            adj = ref.adjoint(dy, u, policy)
            assert (gx - adj).abs().max().item() <= 1e-12 * max(1.0, adj.abs().max().item()), (shape, kind)
            lhs = (ref.forward(x.detach(), u, policy, affine=False) * dy).sum().item()
            rhs = (x.detach() * adj).sum().item()
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (shape, kind, lhs, rhs)
            # what is not kept is exactly zero, and policy 0 is the identity
            keep = ref.keep_mask(u, shape, policy)
            assert (y.detach()[~keep] == 0).all()
            if policy == 0:
                assert torch.equal(y.detach(), x.detach()) and keep.all()


def test_reference_parameter_extremes():
    """u = 0 and u = nextafter(1, 0) give the extreme shifts -R / +R and box offsets 0 / H - K mod 2."""
    lo, hi = _u(1, "lo", None), _u(1, "hi", None)
    for H, W in ((8, 8), (32, 32), (10, 12), (9, 7), (256, 256)):
        Rh, Rw, Kh, Kw = int(H / 8 + .5), int(W / 8 + .5), int(H / 2 + .5), int(W / 2 + .5)
        a, b = ref.params(lo, H, W, 7), ref.params(hi, H, W, 7)
        assert (a["tx"].item(), a["ty"].item(), b["tx"].item(), b["ty"].item()) == (-Rh, -Rw, Rh, Rw)
        assert (a["r0"].item(), a["c0"].item()) == (-(Kh // 2), -(Kw // 2))
        assert (b["r0"].item(), b["c0"].item()) == (H - Kh % 2 - Kh // 2, W - Kw % 2 - Kw // 2)
        assert b["r1"].item() - b["r0"].item() == Kh - 1 and b["c1"].item() - b["c0"].item() == Kw - 1


def test_policy_parsing():
    from relativisticgan_amd import augment
    assert augment.parse_policy("") == 0 and augment.parse_policy(None) == 0
    assert augment.parse_policy("color") == 1 and augment.parse_policy("translation") == 2
    assert augment.parse_policy("cutout") == 4
    assert augment.parse_policy("color,translation,cutout") == 7
    assert augment.parse_policy("cutout, color") == 5 and augment.parse_policy("translation,cutout") == 6
    with pytest.raises(ValueError, match="unknown augmentation 'flip'"):
        augment.parse_policy("color,flip")


def test_flag_default_off_and_pac_error(capsys):
    from relativisticgan_amd import augment
    from relativisticgan_amd.config import make_param, parse
    assert make_param().rgan_diffaug == "" and parse([]).rgan_diffaug == ""
    assert parse(["--rgan_diffaug", "color,cutout"]).rgan_diffaug == "color,cutout"
    assert augment.validate("", pac=2) == 0  # off: PacGAN is unaffected
    with pytest.raises(ValueError, match="rgan_pac"):
        augment.validate("color", pac=2)
    with pytest.raises(SystemExit):
        parse(["--rgan_diffaug", "translation", "--rgan_pac", "2"])
    assert "--rgan_diffaug with --rgan_pac 2 is not supported" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse(["--rgan_diffaug", "zoom"])
    assert "unknown augmentation 'zoom'" in capsys.readouterr().err


def test_library_rejects_malformed_diffaug_calls():
    """Each malformed call returns RGAN_EINVAL (1001) from the host-side check: nothing is
    launched and no pointer is read (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    x, u, ws, y = (ctypes.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000))
    good = dict(x=x, u=u, batch=2, channels=3, h=8, w=8, policy=7, adjoint=0, ws=ws, y=y)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rgan_diffaug(a["x"], a["u"], a["batch"], a["channels"], a["h"], a["w"], a["policy"], a["adjoint"],
                                a["ws"], a["y"], None)

    for name in ("x", "u", "ws", "y"):
        assert call(**{name: None}) == 1001, name
    for name in ("batch", "channels", "h", "w"):
        for bad in (0, -1):
            assert call(**{name: bad}) == 1001, (name, bad)
    for bad in (-1, 8, 64):
        assert call(policy=bad) == 1001, bad
    for adjoint in (0, 1):
        assert call(y=x, adjoint=adjoint) == 1001  # y must not alias x


def test_workspace_size():
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    for B, C, H, W in ((1, 1, 1, 1), (5, 3, 8, 8), (64, 3, 64, 64), (64, 3, 256, 256), (2, 5, 9, 7)):
        n = lib.rgan_diffaug_workspace(B, C, H, W)
        assert 0 < n <= B * C * H * W, (B, C, H, W, n)
    # the multi-block reduction of the large workload: more than one partial per sample
    assert lib.rgan_diffaug_workspace(2, 3, 256, 256) > 2
    for bad in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, -1, 8), (2, 3, 8, 0)):
        assert lib.rgan_diffaug_workspace(*bad) == 0
