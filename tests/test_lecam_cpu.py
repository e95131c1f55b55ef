"""--rgan_lecam without a GPU: flag validation, the exported symbols and their host-side argument
checks (refused before any launch), and the host restatement (tests/lecam_ref.py) against torch
float64 autograd of the restated loss and against sequences worked out by hand, so the GPU tests
can trust it."""
import ctypes

import numpy as np
import pytest

from tests import lecam_ref as ref

NAMES = ("rgan_lecam", "rgan_lecam_finish")


# ---------------------------------------------------------------- flags
def test_flag_defaults_are_off():
    from relativisticgan_amd.config import make_param, parse, validate_lecam
    for ns in (make_param(), parse([])):
        assert (ns.rgan_lecam, ns.rgan_lecam_beta, ns.rgan_lecam_start) == (0.0, 0.99, 1)
    assert validate_lecam(0.0) is False and validate_lecam(0.0, 0.99, 1) is False
    assert validate_lecam(0.3) is True and validate_lecam(0.3, 0.0, 7) is True
    ns = parse(["--rgan_lecam", "0.3", "--rgan_lecam_beta", "0.9", "--rgan_lecam_start", "5"])
    assert (ns.rgan_lecam, ns.rgan_lecam_beta, ns.rgan_lecam_start) == (0.3, 0.9, 5)
    # allowed with every head, packing, the penalties and the augmentation flags
    for more in (["--loss_D", "1"], ["--loss_D", "3"], ["--rgan_pac", "2"], ["--rgan_r1", "1"],
                 ["--rgan_diffaug", "color", "--rgan_ada_target", "0.6"]):
        assert parse(["--rgan_lecam", "0.3", *more]).rgan_lecam == 0.3


@pytest.mark.parametrize("args, match", [
    ((-0.1,), "rgan_lecam must"),
    ((float("nan"),), "rgan_lecam must"),
    ((0.3, 1.0), "rgan_lecam_beta"),
    ((0.3, -0.01), "rgan_lecam_beta"),
    ((0.3, float("nan")), "rgan_lecam_beta"),
    ((0.3, 0.99, 0), "rgan_lecam_start"),
    ((0.3, 0.99, -3), "rgan_lecam_start"),
    ((0.3, 0.99, 1.5), "rgan_lecam_start"),
    ((0.0, 0.9), "need --rgan_lecam"),
    ((0.0, 0.99, 2), "need --rgan_lecam"),
], ids=str)
def test_flag_validation(args, match):
    from relativisticgan_amd.config import validate_lecam
    with pytest.raises(ValueError, match=match):
        validate_lecam(*args)


def test_cli_reports_the_rule(capsys):
    from relativisticgan_amd.config import parse
    for argv, text in ((["--rgan_lecam", "-1"], "--rgan_lecam must be >= 0"),
                       (["--rgan_lecam", "0.3", "--rgan_lecam_beta", "1"], "--rgan_lecam_beta must lie in [0, 1)"),
                       (["--rgan_lecam", "0.3", "--rgan_lecam_start", "0"], "--rgan_lecam_start must be an integer >= 1"),
                       (["--rgan_lecam_beta", "0.9"], "need --rgan_lecam"),
                       (["--rgan_lecam_start", "3"], "need --rgan_lecam")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert text in capsys.readouterr().err, argv


def test_trainer_shares_the_validation():
    import inspect
    from relativisticgan_amd import train
    assert "validate_lecam(" in inspect.getsource(train.Trainer.__init__)


# ---------------------------------------------------------------- the library
def test_library_exports_the_symbols_and_ops():
    import torch
    from relativisticgan_amd import _lib, ops
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    for name in ("lecam_", "lecam_finish_"):
        assert name in ops.OPS and hasattr(torch.ops.rgan, name), name
        assert "rgan::" + name in ops.__doc__
    from relativisticgan_amd.build import SOURCES
    assert "lecam.hip" in SOURCES
    from relativisticgan_amd import lecam, losses
    assert all(hasattr(lecam.LeCam, m) for m in ("restart", "read", "state_dict", "load_state_dict"))
    assert callable(losses.lecam) and callable(losses.lecam_cat)


def test_library_rejects_malformed_calls():
    """RGAN_EINVAL (1001) from the host-side checks: nothing is launched and no pointer is read
    (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    yr, yf, dr, df, h, s, o = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000))
    good = dict(yr=yr, yf=yf, n=8, ng=8, h=h, s=s, dr=dr, df=df, o=o, mode=0)

    def call(**kw):
        k = dict(good, **kw)
        return lib.rgan_lecam(k["yr"], k["yf"], k["n"], k["ng"], k["h"], k["s"], k["dr"], k["df"], k["o"], k["mode"],
                              None)

    for n in (0, -1, -2 ** 31):
        assert call(n=n) == 1001 and call(n=n, ng=n) == 1001, n
    for n, ng in ((8, 7), (8, 0), (8, -8), (2 ** 31 - 1, 8)):
        assert call(n=n, ng=ng) == 1001, (n, ng)
    assert call(yr=None, yf=None) == 1001 and call(yr=None, yf=None, dr=None, df=None) == 1001  # both sides null
    assert call(yr=None) == 1001  # dr given for the absent real side
    assert call(yf=None) == 1001  # df given for the absent fake side
    assert call(yr=None, dr=None, n=0) == 1001 and call(yf=None, df=None, ng=7) == 1001
    assert call(h=None) == 1001 and call(s=None) == 1001 and call(o=None) == 1001
    for mode in (-1, 2, 7):
        assert call(mode=mode) == 1001, mode

    def finish(sums=o, ng=8, sides=3, hyper=h, state=s, loss=o):
        return lib.rgan_lecam_finish(sums, ng, sides, hyper, state, loss, None)

    assert finish(sums=None) == 1001 and finish(hyper=None) == 1001 and finish(state=None) == 1001
    assert finish(loss=None) == 1001
    for ng in (0, -1, -2 ** 31):
        assert finish(ng=ng) == 1001, ng
    for sides in (0, 4, -1):
        assert finish(sides=sides) == 1001, sides


def test_host_argument_checks_under_asan_ubsan():
    """tests/asan/lecam_args.cpp against the host half of csrc/lecam.hip built with
    -fsanitize=address,undefined (the device half is compiled normally and never launched): a
    stand-alone program, objects cached next to tests/test_host_asan.py's."""
    import os
    import subprocess
    from tests import test_host_asan as H
    if not (os.path.exists(H.HIPCC) and os.path.exists(H.CLANG)):
        pytest.skip("needs the ROCm toolchain")
    harness = os.path.join(H.ROOT, "tests", "asan", "lecam_args.cpp")
    headers = [os.path.join(H.CSRC, f) for f in os.listdir(H.CSRC) if f.endswith(".h")] + [os.path.join(H.INC, "rgan.h")]
    os.makedirs(H.BUILD, exist_ok=True)
    path = os.path.join(H.CSRC, "lecam.hip")
    obj = os.path.join(H.BUILD, f"lecam-{H._digest([path] + headers)}.o")  # test_host_asan's names
    if not os.path.exists(obj):
        subprocess.run([H.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I" + H.INC, *H.SAN,
                        "-Wno-unused-result", "-c", path, "-o", obj + ".tmp"], check=True, capture_output=True)
        os.replace(obj + ".tmp", obj)
    hobj = os.path.join(H.BUILD, f"lecam_args-{H._digest([harness] + headers)}.o")
    if not os.path.exists(hobj):
        subprocess.run([H.CLANG, "-O1", "-g", "-std=c++17", "-I" + H.INC, "-fsanitize=address", "-fsanitize=undefined",
                        "-fno-sanitize-recover=undefined", "-c", harness, "-o", hobj + ".tmp"], check=True,
                       capture_output=True)
        os.replace(hobj + ".tmp", hobj)
    exe = os.path.join(H.BUILD, "lecam_args")
    subprocess.run([H.HIPCC, "--offload-arch=gfx950", *H.SAN, "-o", exe, hobj, obj], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lecam_args ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------- the restatement
def _restated_loss(y_real, y_fake, a_real, a_fake, w, n_global):
    """§7.2 in torch float64, anchors detached."""
    import torch
    a_real, a_fake = a_real.detach(), a_fake.detach()
    L = 0.0
    if y_real is not None:
        L = L + ((y_real - a_fake) ** 2).sum() / n_global
    if y_fake is not None:
        L = L + ((y_fake - a_real) ** 2).sum() / n_global
    return w * L if torch.is_tensor(L) else torch.zeros((), dtype=torch.float64)


@pytest.mark.parametrize("n", [1, 5, 64, 257])
@pytest.mark.parametrize("shape", ["both", "real", "fake"])
def test_restated_gradients_are_autograd_of_the_restated_loss(n, shape):
    import torch
    gen = torch.Generator().manual_seed(100 * n + len(shape))
    for calls, n_global in ((0, n), (2, n), (3, n), (9, 2 * n)):
        yr = torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_(True) if shape != "fake" else None
        yf = (torch.randn(n, generator=gen, dtype=torch.float64) - 1).requires_grad_(True) if shape != "real" else None
        # the anchors require grad, so a gradient leaking into them would show
        a_real = torch.tensor(0.25, dtype=torch.float64, requires_grad=True)
        a_fake = torch.tensor(-0.5, dtype=torch.float64, requires_grad=True)
        c = ref.LeCam(0.3, 0.9, 3, a_real=0.25, a_fake=-0.5, calls=calls)
        w = 0.3 if calls >= 3 else 0.0
        assert c.weight() == w
        want_L = _restated_loss(yr, yf, a_real, a_fake, w, n_global)
        ins = [t for t in (yr, yf) if t is not None]
        want = torch.autograd.grad(want_L, ins + [a_real, a_fake], allow_unused=True)
        assert want[-1] is None and want[-2] is None  # detached
        np_r = None if yr is None else yr.detach().numpy()
        np_f = None if yf is None else yf.detach().numpy()
        L, gr, gf = c.step(np_r, np_f, n_global)
        assert abs(L - want_L.item()) <= 1e-12 * max(abs(want_L.item()), 1e-300)
        got = [g for g in (gr, gf) if g is not None]
        assert len(got) == len(ins)
        for g, wg in zip(got, want[:len(ins)]):
            assert np.abs(g - wg.numpy()).max() <= 1e-12 * max(np.abs(wg.numpy()).max(), 1e-300)
            if w == 0:
                assert (g == 0).all()
        assert (gr is None) == (yr is None) and (gf is None) == (yf is None)


def test_update_rule_by_hand():
    # beta = 1/2, dyadic values: every step is exact
    c = ref.LeCam(2.0, 0.5, 2)
    L, gr, gf = c.step([1.0, 3.0], [-1.0, -3.0])
    assert (L, c.state) == (0.0, [2.0, -2.0, 1.0, 0.0])  # calls == 0: the means, no weight
    assert (gr == 0).all() and (gf == 0).all()
    L, gr, gf = c.step([4.0, 4.0], [0.0, 0.0])  # calls 1 < start 2: still no weight, the anchors move
    assert (L, c.state) == (0.0, [3.0, -1.0, 2.0, 0.0]) and (gr == 0).all()
    L, gr, gf = c.step([1.0, 3.0], [1.0, 5.0])
    # (1+1)^2 + (3+1)^2 = 20, (1-3)^2 + (5-3)^2 = 8: L = 2 (20/2 + 8/2) = 28
    assert L == 28.0 and gr.tolist() == [4.0, 8.0] and gf.tolist() == [-4.0, 4.0]
    assert c.state == [2.5, 1.0, 3.0, 0.0]
    # n_global = 2 n: every mean, the term and the gradients halve
    d = ref.LeCam(2.0, 0.5, 2, a_real=3.0, a_fake=-1.0, calls=2)
    L, gr, gf = d.step([1.0, 3.0], [1.0, 5.0], n_global=4)
    assert L == 14.0 and gr.tolist() == [2.0, 4.0] and gf.tolist() == [-2.0, 2.0]
    assert d.state == [0.5 * 3.0 + 0.5 * 1.0, 0.5 * -1.0 + 0.5 * 1.5, 3.0, 0.0]


def test_single_side_calls_by_hand():
    """A real-only call moves a_real only and does not count; the fake-only call that follows
    reads the same count, moves a_fake and counts the step."""
    c = ref.LeCam(2.0, 0.5, 1, a_real=3.0, a_fake=-1.0, calls=2)
    L, gr, gf = c.step([1.0, 3.0], None)
    assert L == 20.0 and gr.tolist() == [4.0, 8.0] and gf is None and c.state == [2.5, -1.0, 2.0, 0.0]
    L, gr, gf = c.step(None, [0.5, 4.5])
    # the fake side reads a_real as the real-only call left it: (0.5-2.5)^2 + (4.5-2.5)^2 = 8
    assert L == 8.0 and gr is None and gf.tolist() == [-4.0, 4.0] and c.state == [2.5, 0.75, 3.0, 0.0]
    first = ref.LeCam(2.0, 0.5, 1)
    assert first.step([1.0, 3.0], None)[0] == 0.0 and first.state == [2.0, 0.0, 0.0, 0.0]
    assert first.step(None, [5.0, 7.0])[0] == 0.0 and first.state == [2.0, 6.0, 1.0, 0.0]  # still the first step


def test_shard_sums_add_up():
    rng = np.random.default_rng(3)
    yr, yf = rng.standard_normal(10), rng.standard_normal(10) - 1
    whole = ref.LeCam(0.3, 0.9, 1, a_real=0.25, a_fake=-0.5, calls=4)
    L, gr, gf = whole.step(yr, yf)
    parts = ref.LeCam(0.3, 0.9, 1, a_real=0.25, a_fake=-0.5, calls=4)
    sums = sum(ref.shard_sums(yr[lo:hi], yf[lo:hi], 0.25, -0.5) for lo, hi in ((0, 3), (3, 10)))
    g0, g1 = parts.grads(yr[:3], yf[:3], 10), parts.grads(yr[3:], yf[3:], 10)
    L2 = parts.finish(sums, 10, True, True)
    assert abs(L - L2) <= 1e-15 * abs(L) and np.allclose(parts.state, whole.state, rtol=1e-15, atol=0)
    assert (np.concatenate([g0[0], g1[0]]) == gr).all() and (np.concatenate([g0[1], g1[1]]) == gf).all()
