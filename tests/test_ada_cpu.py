"""--rgan_aug_p / --rgan_ada_target without a GPU: flag validation, the exported symbols and their
host-side argument checks (refused before any launch), and the host restatement (tests/ada_ref.py)
against sequences worked out by hand, so the GPU tests can trust it."""
import ctypes
import math

import numpy as np
import pytest

from tests import ada_ref as ref

NAMES = ("rgan_diffaug_p", "rgan_ada_update", "rgan_ada_adjust")


# ---------------------------------------------------------------- flags
def test_flag_defaults_are_off():
    from relativisticgan_amd.config import make_param, parse, validate_ada
    for ns in (make_param(), parse([])):
        assert (ns.rgan_aug_p, ns.rgan_ada_target, ns.rgan_ada_interval, ns.rgan_ada_kimg) == (None, 0.0, 4, 500.0)
    # unset: not gated, every transform on every image -- with and without --rgan_diffaug
    assert validate_ada("") == (False, 1.0)
    assert validate_ada("color,cutout") == (False, 1.0)
    assert validate_ada("color", aug_p=0.25) == (True, 0.25)
    assert validate_ada("color", aug_p=0.0) == (True, 0.0) and validate_ada("color", aug_p=1.0) == (True, 1.0)
    assert validate_ada("color", target=0.6) == (True, 0.0)  # adaptation starts at 0 ...
    assert validate_ada("color", aug_p=0.5, target=0.6, interval=2, kimg=0.048) == (True, 0.5)  # ... or at P
    ns = parse(["--rgan_diffaug", "color", "--rgan_aug_p", "0.5", "--rgan_ada_target", "0.6",
                "--rgan_ada_interval", "2", "--rgan_ada_kimg", "0.048"])
    assert (ns.rgan_aug_p, ns.rgan_ada_target, ns.rgan_ada_interval, ns.rgan_ada_kimg) == (0.5, 0.6, 2, 0.048)


@pytest.mark.parametrize("kw, match", [
    (dict(policy="", aug_p=0.5), "rgan_diffaug"),
    (dict(policy="", target=0.6), "rgan_diffaug"),
    (dict(policy="", interval=2), "rgan_diffaug"),
    (dict(policy="", kimg=100.0), "rgan_diffaug"),
    (dict(policy="color", aug_p=-0.01), "rgan_aug_p"),
    (dict(policy="color", aug_p=1.01), "rgan_aug_p"),
    (dict(policy="color", aug_p=float("nan")), "rgan_aug_p"),
    (dict(policy="color", target=1.0), "rgan_ada_target"),
    (dict(policy="color", target=-0.2), "rgan_ada_target"),
    (dict(policy="color", target=0.6, interval=0), "rgan_ada_interval"),
    (dict(policy="color", target=0.6, kimg=0.0), "rgan_ada_kimg"),
    (dict(policy="color", target=0.6, kimg=-1.0), "rgan_ada_kimg"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_flag_validation(kw, match):
    from relativisticgan_amd.config import validate_ada
    with pytest.raises(ValueError, match=match):
        validate_ada(**kw)


def test_cli_reports_the_rule(capsys):
    from relativisticgan_amd.config import parse
    for argv, text in ((["--rgan_aug_p", "0.5"], "--rgan_diffaug"),
                       (["--rgan_diffaug", "color", "--rgan_aug_p", "2"], "--rgan_aug_p must lie in [0, 1]"),
                       (["--rgan_diffaug", "color", "--rgan_ada_target", "1.5"], "--rgan_ada_target must lie in (0, 1)"),
                       (["--rgan_diffaug", "color", "--rgan_ada_interval", "0"], "--rgan_ada_interval must be >= 1"),
                       (["--rgan_diffaug", "color", "--rgan_ada_kimg", "0"], "--rgan_ada_kimg must be > 0")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert text in capsys.readouterr().err, argv


def test_trainer_shares_the_validation():
    """The trainer checks a hand-built parameter set with the same function, before it builds anything
    on a device."""
    import inspect
    from relativisticgan_amd import train
    assert "validate_ada(" in inspect.getsource(train.Trainer.__init__)


# ---------------------------------------------------------------- the library
def test_library_exports_the_symbols_and_ops():
    import torch
    from relativisticgan_amd import _lib, ops
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    for name in ("diffaug_p", "diffaug_p_backward", "ada_update_"):
        assert name in ops.OPS and hasattr(torch.ops.rgan, name), name
    from relativisticgan_amd.build import SOURCES
    assert "ada.hip" in SOURCES


def test_library_rejects_malformed_calls():
    """RGAN_EINVAL (1001) from the host-side checks: nothing is launched and no pointer is read
    (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    a, b, h, s = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))
    assert lib.rgan_ada_update(None, b, 8, h, s, 1, None) == 1001
    assert lib.rgan_ada_update(a, None, 8, h, s, 1, None) == 1001
    assert lib.rgan_ada_update(a, b, 8, None, s, 1, None) == 1001
    assert lib.rgan_ada_update(a, b, 8, h, None, 1, None) == 1001
    for n in (0, -1, -2 ** 31):
        assert lib.rgan_ada_update(a, b, n, h, s, 0, None) == 1001, n
    assert lib.rgan_ada_adjust(None, s, None) == 1001
    assert lib.rgan_ada_adjust(h, None, None) == 1001

    x, u, g, p, ws, y = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))
    good = dict(x=x, u=u, gate=g, p=p, batch=2, channels=3, h=8, w=8, policy=7, adjoint=0, ws=ws, y=y)

    def call(**kw):
        k = dict(good, **kw)
        return lib.rgan_diffaug_p(k["x"], k["u"], k["gate"], k["p"], k["batch"], k["channels"], k["h"], k["w"],
                                  k["policy"], k["adjoint"], k["ws"], k["y"], None)

    for name in ("x", "u", "gate", "p", "ws", "y"):
        assert call(**{name: None}) == 1001, name
    for name in ("batch", "channels", "h", "w"):
        for bad in (0, -1):
            assert call(**{name: bad}) == 1001, (name, bad)
    for bad in (-1, 8, 64):
        assert call(policy=bad) == 1001, bad
    assert call(y=x) == 1001 and call(batch=65536) == 1001


def test_host_argument_checks_under_asan_ubsan():
    """tests/asan/ada_args.cpp against the host halves of csrc/augment.hip and csrc/ada.hip built
    with -fsanitize=address,undefined (the device halves are compiled normally and never launched):
    a stand-alone program, objects cached next to tests/test_host_asan.py's."""
    import os
    import subprocess
    from tests import test_host_asan as H
    if not (os.path.exists(H.HIPCC) and os.path.exists(H.CLANG)):
        pytest.skip("needs the ROCm toolchain")
    harness = os.path.join(H.ROOT, "tests", "asan", "ada_args.cpp")
    headers = [os.path.join(H.CSRC, f) for f in os.listdir(H.CSRC) if f.endswith(".h")] + [os.path.join(H.INC, "rgan.h")]
    os.makedirs(H.BUILD, exist_ok=True)
    objs = []
    for src in ("augment.hip", "ada.hip"):
        path = os.path.join(H.CSRC, src)
        obj = os.path.join(H.BUILD, f"{src[:-4]}-{H._digest([path] + headers)}.o")  # test_host_asan's names
        objs.append(obj)
        if not os.path.exists(obj):
            subprocess.run([H.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I" + H.INC, *H.SAN,
                            "-Wno-unused-result", "-c", path, "-o", obj + ".tmp"], check=True, capture_output=True)
            os.replace(obj + ".tmp", obj)
    hobj = os.path.join(H.BUILD, f"ada_args-{H._digest([harness] + headers)}.o")
    if not os.path.exists(hobj):
        subprocess.run([H.CLANG, "-O1", "-g", "-std=c++17", "-I" + H.INC, "-fsanitize=address", "-fsanitize=undefined",
                        "-fno-sanitize-recover=undefined", "-c", harness, "-o", hobj + ".tmp"], check=True,
                       capture_output=True)
        os.replace(hobj + ".tmp", hobj)
    exe = os.path.join(H.BUILD, "ada_args")
    subprocess.run([H.HIPCC, "--offload-arch=gfx950", *H.SAN, "-o", exe, hobj, *objs], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ada_args ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------- the restatement, by hand
def test_rank_counts_by_hand():
    inf, nan = math.inf, math.nan
    #        >    <    tie  tie(inf)  >      <      nan   nan   nan
    real = [2.0, 1.0, 3.0, inf, inf, -inf, nan, 1.0, nan]
    fake = [1.0, 2.0, 3.0, inf, 1.0, 1.0, 1.0, nan, nan]
    assert ref.rank_counts(real, fake) == (0, 9)
    assert ref.rank_counts(real[:1] + real[4:5], fake[:1] + fake[4:5]) == (2, 2)
    assert ref.rank_counts([0.0], [-0.0]) == (0, 1)  # +0 == -0: a tie
    assert ref.rank_counts(np.float32([1, 1, 1, 0]), np.float32([0, 0, 0, 1])) == (2, 4)


def test_controller_by_hand():
    # interval 2, 16 images per unit of p: two calls of 2 pairs move p by 4 / 16 = 1/4
    c = ref.Controller(p=0.5, target=0.5, interval=2, images_per_unit_p=16.0)
    up, down = ([1.0, 1.0], [0.0, 0.0]), ([0.0, 0.0], [1.0, 1.0])
    c.update(*up)
    assert (c.p, c.S, c.N, c.calls) == (0.5, 2, 2, 1)  # not due: p untouched, sums kept
    c.update(*up)
    assert (c.p, c.S, c.N, c.calls) == (0.75, 0, 0, 2)  # r = 1 > 1/2
    c.update(*up), c.update(*up)
    assert c.p == 1.0
    c.update(*up), c.update(*up)
    assert (c.p, c.calls) == (1.0, 6)  # clamped at 1
    for _ in range(4):
        c.update(*down), c.update(*down)
    assert (c.p, c.calls) == (0.0, 14)
    c.update(*down), c.update(*down)
    assert (c.p, c.S, c.N) == (0.0, 0, 0)  # clamped at 0
    # r == target exactly (3 right, 1 wrong of 4: r = 1/2): p stays, the sums are cleared all the same
    c.p = 0.375
    c.update([1.0, 1.0], [0.0, 0.0]), c.update([1.0, 0.0], [0.0, 1.0])
    assert (c.p, c.S, c.N, c.calls) == (0.375, 0, 0, 18)
    # N == 0 at a due call: nothing moves
    c.adjust(), c.adjust()
    assert (c.p, c.S, c.N, c.calls) == (0.375, 0, 0, 20)
    c.S, c.N = 0, 0
    c.adjust()
    c.accumulate(*down)
    assert c.p == 0.375
    c.adjust()  # call 22: due, N = 2, r = -1
    assert (c.p, c.calls) == (0.25, 22)
    assert c.state == [0.25, 0.0, 0.0, 22.0]


def test_sub_policy_by_hand():
    half, below = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0))
    gate = [[0.0, 0.9, 0.9, 0.0], [half, below, 0.9, 0.0], [below, half, below, 0.9], [0.1, 0.2, 0.3, 0.9]]
    assert ref.sub_policy(7, gate, 0.5) == [1, 2, 5, 7]  # 0.5 itself is closed, the float below it open
    assert ref.sub_policy(6, gate, 0.5) == [0, 2, 4, 6]
    assert ref.sub_policy(7, gate, 0.0) == [0, 0, 0, 0] and ref.sub_policy(7, gate, 1.0) == [7, 7, 7, 7]
    assert ref.sub_policy(7, gate, float("nan")) == [0, 0, 0, 0]
