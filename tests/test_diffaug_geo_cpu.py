"""The geometric groups of --rgan_diffaug (xflip, rot90, warp) without a GPU: the names and the
flag, the draw, the restatement (tests/diffaug_geo_ref.py) against torch's own grid_sample and
rot90 and its adjoint identity in float64 (so the GPU tests can trust it), and the host-side
argument checks of rgan_diffaug_geo, from Python and under ASan + UBSan in a stand-alone program."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import diffaug_geo_ref as ref

ONE_BELOW = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))


def test_names_parse_to_bits():
    from relativisticgan_amd import augment
    assert augment.parse_policy("xflip") == 8 and augment.parse_policy("rot90") == 16
    assert augment.parse_policy("warp") == 32
    assert augment.parse_policy("xflip,rot90,warp") == 56
    assert augment.parse_policy("color,translation,cutout,xflip,rot90,warp") == 63
    assert augment.parse_policy("warp, color") == 33
    assert augment.BITS == {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16, "warp": 32}


def test_cli_accepts_the_names_and_pac_is_refused(capsys):
    from relativisticgan_amd import augment
    from relativisticgan_amd.config import make_param, parse
    assert parse(["--rgan_diffaug", "xflip,rot90,warp"]).rgan_diffaug == "xflip,rot90,warp"
    assert parse(["--rgan_diffaug", "color,warp", "--rgan_aug_p", "0.5"]).rgan_aug_p == 0.5
    assert make_param(rgan_diffaug="color,xflip").rgan_diffaug == "color,xflip"
    assert augment.validate("xflip,rot90,warp") == 56
    for name in ("xflip", "rot90", "warp"):
        with pytest.raises(ValueError, match="rgan_pac"):
            augment.validate(name, pac=2)
    with pytest.raises(SystemExit):
        parse(["--rgan_diffaug", "warp", "--rgan_pac", "2"])
    assert "--rgan_diffaug with --rgan_pac 2 is not supported" in capsys.readouterr().err


def test_draw_geo_shape_and_stream():
    from relativisticgan_amd import augment
    torch.manual_seed(3)
    v = augment.draw_geo(12, host=True)
    assert v.shape == (12, 8) and v.dtype == torch.float32 and (v >= 0).all() and (v < 1).all()
    # drawn last: the draws before it are those of a policy without a geometric group
    torch.manual_seed(5)
    a = (augment.draw(12, True), augment.draw_gates(12, True))
    torch.manual_seed(5)
    b = (augment.draw(12, True), augment.draw_gates(12, True), augment.draw_geo(12, True))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_parameters_of_the_extreme_rows():
    lo, hi, mid = torch.zeros(1, 8), torch.full((1, 8), ONE_BELOW), torch.tensor([[0, 0, .5, .5, 0, 0, 0, 0]])
    a, b, c = ref.params(lo, 56), ref.params(hi, 56), ref.params(mid, 56)
    assert (bool(a["flip"]), int(a["k"]), bool(b["flip"]), int(b["k"])) == (False, 0, True, 3)
    assert float(a["s"]) == 2 ** -0.25 and float(a["theta"]) == -math.pi
    assert abs(float(b["s"]) - 2 ** 0.25) < 1e-7 and 0 < math.pi - float(b["theta"]) < 1e-6
    assert float(c["s"]) == 1.0 and float(c["theta"]) == 0.0
    off = ref.params(hi, 7)
    assert (bool(off["flip"]), int(off["k"]), float(off["s"]), float(off["theta"])) == (False, 0, 1.0, 0.0)


@pytest.mark.parametrize("shape", [(3, 9, 20), (2, 12, 7), (1, 16, 16)], ids=str)
def test_warp_is_grid_sample(shape):
    """The four-tap gather against F.grid_sample(bilinear, zeros, align_corners=True) on the same
    float64 coordinates, non-square inputs included."""
    gen = torch.Generator().manual_seed(sum(shape))
    C, H, W = shape
    z = torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1
    for s, theta in ((1.0, 0.0), (2 ** -0.25, -math.pi), (2 ** 0.25, 3.0), (1.1, 0.7), (0.9, -2.2), (1.0, math.pi / 2)):
        r, c = ref.warp_coords(H, W, s, theta)
        grid = torch.stack([2 * c / (W - 1) - 1, 2 * r / (H - 1) - 1], dim=-1)[None]
        want = F.grid_sample(z[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
        got = ref.warp(z, s, theta)
        assert (got - want).abs().max().item() <= 1e-12, (shape, s, theta)
    assert torch.equal(ref.warp(z, 1.0, 0.0), z)


def test_warp_by_a_quarter_turn_is_rot90():
    gen = torch.Generator().manual_seed(4)
    for N in (8, 9):
        z = torch.rand((3, N, N), generator=gen, dtype=torch.float64) * 2 - 1
        assert (ref.warp(z, 1.0, math.pi / 2) - torch.rot90(z, 1, (1, 2))).abs().max().item() <= 1e-12
        assert (ref.warp(z, 1.0, -math.pi / 2) - torch.rot90(z, 3, (1, 2))).abs().max().item() <= 1e-12


def _v(B, kind, gen):
    if kind == "lo":
        return torch.zeros(B, 8)
    if kind == "hi":
        return torch.full((B, 8), ONE_BELOW)
    if kind == "id":
        return torch.tensor([[0, 0, .5, .5, 0, 0, 0, 0]], dtype=torch.float32).repeat(B, 1)
    return torch.rand(B, 8, generator=gen)


@pytest.mark.parametrize("policy", [8, 16, 32, 24, 26, 33, 56, 57, 62, 63])
def test_reference_adjoint_is_the_transpose(policy):
    """<T_lin x, w> = <x, T^t w> in float64, and the composition's fixed points: the identity row
    under the warp bit is the call without it, and what is not kept is exactly zero."""
    gen = torch.Generator().manual_seed(policy)
    shapes = [(3, 3, 8, 8), (2, 1, 9, 9)] + ([] if policy & 16 else [(2, 2, 9, 12)])
    for shape in shapes:
        for kind in ("rand", "lo", "hi", "id"):
            u, v = torch.rand(shape[0], 8, generator=gen), _v(shape[0], kind, gen)
            x = torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1
            w = torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1
            lhs = (ref.forward(x, u, v, policy, affine=False) * w).sum().item()
            rhs = (x * ref.adjoint(w, u, v, policy)).sum().item()
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (shape, kind, lhs, rhs)
            y = ref.forward(x, u, v, policy)
            assert (y[~ref.keep_mask(u, shape, policy)] == 0).all()
            if kind == "id":
                assert (y - ref.forward(x, u, v, policy & ~32)).abs().max().item() <= 1e-15
    # without a geometric bit the restatement is tests/diffaug_ref.py's
    from tests import diffaug_ref as base
    x = torch.rand((2, 3, 8, 8), generator=gen, dtype=torch.float64)
    u, v = torch.rand(2, 8, generator=gen), torch.rand(2, 8, generator=gen)
    assert torch.equal(ref.forward(x, u, v, policy & 7), base.forward(x, u, policy & 7))


def test_library_exports_the_symbols_and_ops():
    from relativisticgan_amd import _lib, ops
    from relativisticgan_amd.build import SOURCES
    lib = _lib.lib()
    for name in ("rgan_diffaug_geo", "rgan_diffaug_geo_workspace"):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    for name in ("diffaug_geo", "diffaug_geo_backward"):
        assert name in ops.OPS and hasattr(torch.ops.rgan, name), name
    assert "augment_geo.hip" in SOURCES
    assert lib.rgan_diffaug_geo_workspace(2, 3, 256, 256) == lib.rgan_diffaug_workspace(2, 3, 256, 256)


def test_library_rejects_malformed_calls():
    """RGAN_EINVAL (1001) from the host-side checks: nothing is launched and no pointer is read
    (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    x, u, v, g, p, ws, y = (ctypes.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000))
    good = dict(x=x, u=u, v=v, gate=g, p=p, batch=2, channels=3, h=8, w=8, policy=63, adjoint=0, ws=ws, y=y)

    def call(**kw):
        k = dict(good, **kw)
        return lib.rgan_diffaug_geo(k["x"], k["u"], k["v"], k["gate"], k["p"], k["batch"], k["channels"], k["h"],
                                    k["w"], k["policy"], k["adjoint"], k["ws"], k["y"], None)

    for name in ("x", "u", "v", "gate", "p", "ws", "y"):  # (gate or p alone null: exactly one of the two)
        assert call(**{name: None}) == 1001, name
    for name in ("x", "u", "v", "ws", "y"):
        assert call(gate=None, p=None, **{name: None}) == 1001, name
    for name in ("batch", "channels", "h", "w"):
        for bad in (0, -1):
            assert call(**{name: bad}) == 1001, (name, bad)
    for bad in (-1, 64, 128):
        assert call(policy=bad) == 1001, bad
    for policy in (16, 24, 63):
        assert call(policy=policy, h=9, w=20) == 1001 and call(policy=policy, h=9, w=20, gate=None, p=None) == 1001
    assert call(y=x) == 1001 and call(batch=65536) == 1001
    # without a geometric bit the checks are rgan_diffaug's / rgan_diffaug_p's
    assert call(policy=7, x=None) == 1001 and call(policy=7, gate=None, p=None, y=x) == 1001


def test_host_argument_checks_under_asan_ubsan():
    """tests/asan/geo_args.cpp against the host halves of csrc/augment.hip and csrc/augment_geo.hip
    built with -fsanitize=address,undefined (the device halves are compiled normally and never
    launched): a stand-alone program, objects cached next to tests/test_host_asan.py's."""
    import os
    import subprocess
    from tests import test_host_asan as H
    if not (os.path.exists(H.HIPCC) and os.path.exists(H.CLANG)):
        pytest.skip("needs the ROCm toolchain")
    harness = os.path.join(H.ROOT, "tests", "asan", "geo_args.cpp")
    headers = [os.path.join(H.CSRC, f) for f in os.listdir(H.CSRC) if f.endswith(".h")] + [os.path.join(H.INC, "rgan.h")]
    os.makedirs(H.BUILD, exist_ok=True)
    objs = []
    for src in ("augment.hip", "augment_geo.hip"):
        path = os.path.join(H.CSRC, src)
        obj = os.path.join(H.BUILD, f"{src[:-4]}-{H._digest([path] + headers)}.o")  # test_host_asan's names
        objs.append(obj)
        if not os.path.exists(obj):
            subprocess.run([H.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I" + H.INC, *H.SAN,
                            "-Wno-unused-result", "-c", path, "-o", obj + ".tmp"], check=True, capture_output=True)
            os.replace(obj + ".tmp", obj)
    hobj = os.path.join(H.BUILD, f"geo_args-{H._digest([harness] + headers)}.o")
    if not os.path.exists(hobj):
        subprocess.run([H.CLANG, "-O1", "-g", "-std=c++17", "-I" + H.INC, "-fsanitize=address", "-fsanitize=undefined",
                        "-fno-sanitize-recover=undefined", "-c", harness, "-o", hobj + ".tmp"], check=True,
                       capture_output=True)
        os.replace(hobj + ".tmp", hobj)
    exe = os.path.join(H.BUILD, "geo_args")
    subprocess.run([H.HIPCC, "--offload-arch=gfx950", *H.SAN, "-o", exe, hobj, *objs], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "geo_args ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
