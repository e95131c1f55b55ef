"""The nearest-training-image check without a GPU: the numpy restatement (tests/nn_ref.py) against
brute force, the two scenarios the numbers are meant to tell apart, the flags, the exported symbols
and ops, and every host-side refusal of the rgan_nn_ entry points (also under ASan + UBSan)."""
import ctypes
import os

import numpy as np
import pytest

from tests import nn_ref as ref

NAMES = ("rgan_nn_row_bytes", "rgan_nn_pack_u8", "rgan_nn_topk_splits", "rgan_nn_topk_ws_bytes", "rgan_nn_topk",
         "rgan_nn_covered")
OPS = ("nn_pack_u8", "nn_topk", "nn_covered")
NO_SELF = -2 ** 63


# ---------------------------------------------------------------- the reference itself
def test_int32_bound():
    assert 255 ** 2 * 12288 == 799027200 < 2 ** 31
    assert 2 * 128 ** 2 * 12288 + 2 * 128 ** 2 * 12288 < 2 ** 31  # na + nb - 2 a.b at its extremes
    assert ref.MAX_ROW_BYTES == 12288 == ref.row_bytes(3, 64) and ref.row_bytes(3, 8) == 192 and ref.row_bytes(1, 8) == 64


def test_distances_against_brute_force_float64():
    rng = np.random.default_rng(0)
    A = rng.integers(0, 256, size=(9, 3, 16, 16), dtype=np.uint8)
    B = rng.integers(0, 256, size=(14, 3, 16, 16), dtype=np.uint8)
    a, na = ref.pack(A, 16)
    b, nb = ref.pack(B, 16)
    assert a.dtype == np.int8 and a.shape == (9, 768)
    brute = ((A.reshape(9, 1, -1).astype(np.float64) - B.reshape(1, 14, -1).astype(np.float64)) ** 2).sum(axis=2)
    d = ref.dist2(a, b)
    assert d.dtype == np.int64 and np.array_equal(d.astype(np.float64), brute)  # the shift by 128 cancels
    assert np.array_equal(na, ((A.astype(np.int64) - 128) ** 2).reshape(9, -1).sum(axis=1))
    dist, idx = ref.topk(a, b, 4)
    order = np.argsort(brute, axis=1, kind="stable")[:, :4]
    assert np.array_equal(idx, order) and np.array_equal(dist, np.take_along_axis(d, order, axis=1))
    radius = rng.integers(int(d.min()), int(d.max()), size=14)
    assert np.array_equal(ref.covered(a, b, radius), (brute <= radius[None, :]).any(axis=1))


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_box_mean_is_the_rounded_mean(f):
    rng = np.random.default_rng(f)
    s = 8
    x = rng.integers(0, 256, size=(5, 3, s * f, s * f), dtype=np.uint8)
    if f > 1:  # a box whose mean is exactly .5 (half ones, half zeros): rounds up to 1
        half = np.zeros(f * f, dtype=np.uint8)
        half[: f * f // 2] = 1
        x[1, 0, :f, :f] = half.reshape(f, f)
    desc, norm = ref.pack(x, s)
    mean = x.reshape(5, 3, s, f, s, f).astype(np.float64).mean(axis=(3, 5))
    want = np.floor(mean + 0.5).astype(np.int64) - 128
    assert np.array_equal(desc[:, :3 * s * s].astype(np.int64), want.reshape(5, -1))
    assert desc.shape[1] == 3 * s * s  # s * s = 64 divides every legal D: the rows have no pad bytes
    if f > 1:
        assert desc[1, 0] == 1 - 128
    else:
        assert np.array_equal(desc[:, :192].astype(np.int64) + 128, x.reshape(5, -1))
    d1, _ = ref.pack(x[:, :1], s)  # C = 1: 64 bytes; C = 3: 192 of 192; (1, 8) has no pad either
    assert d1.shape == (5, 64)


def test_pad_is_zero_after_the_shift():
    x = np.zeros((2, 3, 8, 8), dtype=np.uint8)
    desc, norm = ref.pack(x, 8)
    assert desc.shape == (2, 192) and (desc == -128).all() and (norm == 192 * 128 ** 2).all()
    # every legal side has s * s = a multiple of 64, so pack itself never pads; a caller's own padded rows
    # must carry zeros (not -128): zeros add nothing to a norm or a distance
    a = np.concatenate([desc, np.zeros((2, 64), dtype=np.int8)], axis=1)
    assert np.array_equal(ref.dist2(a, a), ref.dist2(desc, desc))


def test_tie_rule_and_fill():
    b = np.zeros((6, 64), dtype=np.int8)
    b[2, 0] = b[4, 0] = 3
    a = np.zeros((2, 64), dtype=np.int8)
    a[1, 0] = 3
    dist, idx = ref.topk(a, b, 8)
    assert idx[0].tolist() == [0, 1, 3, 5, 2, 4, -1, -1] and dist[0].tolist() == [0, 0, 0, 0, 9, 9] + [ref.INT32_MAX] * 2
    assert idx[1].tolist() == [2, 4, 0, 1, 3, 5, -1, -1]
    dist, idx = ref.topk(b[1:3], b, 2, self_offset=1)  # queries are rows 1.. of b: leave-one-out
    assert idx.tolist() == [[0, 3], [4, 0]] and dist.tolist() == [[0, 0], [0, 9]]
    assert ref.covered(b[1:3], b, np.zeros(6, dtype=np.int64), self_offset=1).tolist() == [1, 1]
    only = np.full(6, -1)
    only[2] = 0  # only row 2 has a radius that anything can meet: itself (excluded) and row 4
    assert ref.covered(b[2:3], b, only, self_offset=2).tolist() == [0]
    assert ref.covered(b[2:3], b, only).tolist() == [1]
    assert ref.median([3.0, 1.0, 2.0]) == 2.0 and ref.median([4.0, 1.0, 2.0, 3.0]) == 2.5


def _synthetic_bytes():
    from relativisticgan_amd.train import synthetic_images
    return ref.to_u8(synthetic_images(64, 32, device="cpu").numpy())


def test_scenario_memorised():
    """Fakes that are the reals plus noise in {-1, 0, 1}: a tiny ratio, every fake's nearest real is
    its source, precision = recall = 1."""
    real = _synthetic_bytes()
    rng = np.random.default_rng(1)
    fake = np.clip(real.astype(np.int64) + rng.integers(-1, 2, size=real.shape), 0, 255).astype(np.uint8)
    out, cross = ref.report(real, fake, 16, 3)
    print(out)
    assert list(out) == ["fake_nn", "real_nn", "ratio", "precision", "recall"]
    assert out["ratio"] < 0.05
    assert np.array_equal(cross[1][:, 0], np.arange(64))
    assert out["precision"] == 1.0 and out["recall"] == 1.0


def test_scenario_independent():
    """Fakes that are independent noise of the same law: as far from the reals as the reals are from
    each other."""
    real = _synthetic_bytes()
    fake = np.random.default_rng(2).integers(0, 256, size=real.shape, dtype=np.uint8)
    out, _ = ref.report(real, fake, 16, 3)
    print(out)
    assert 0.9 <= out["ratio"] <= 1.1


def test_grid_layout():
    rng = np.random.default_rng(3)
    real = rng.integers(1, 256, size=(5, 3, 8, 8), dtype=np.uint8)
    fake = rng.integers(1, 256, size=(9, 3, 8, 8), dtype=np.uint8)
    idx = np.array([[4, 0], [1, -1]] + [[2, 3]] * 7)
    g = ref.grid(real, fake, idx, 2)
    assert g.shape == (10 * 8 + 2, 10 * 3 + 2, 3) and g.dtype == np.uint8
    assert np.array_equal(g[2:10, 2:10], fake[0].transpose(1, 2, 0))
    assert np.array_equal(g[2:10, 12:20], real[4].transpose(1, 2, 0))
    assert np.array_equal(g[12:20, 12:20], real[1].transpose(1, 2, 0)) and not g[12:20, 22:30].any()
    assert np.array_equal(g[72:80, 22:30], real[3].transpose(1, 2, 0))  # row 7, the last; fake 8 is not shown
    assert not g[:2].any() and not g[:, :2].any() and not g[10:12].any() and not g[-2:].any() and not g[:, -2:].any()


# ---------------------------------------------------------------- flags
def test_flag_defaults_and_refusals(capsys, monkeypatch):
    from relativisticgan_amd.config import make_param, parse, validate_nn
    for ns in (make_param(), parse([])):
        assert (ns.rgan_nn_every, ns.rgan_nn, ns.rgan_nn_images, ns.rgan_nn_side, ns.rgan_nn_k) == (0, False, 8192, 64, 3)
    ns = parse(["--rgan_nn_every", "500", "--rgan_nn_images", "1000", "--rgan_nn_side", "16", "--rgan_nn_k", "5",
                "--rgan_nn", "True"])
    assert (ns.rgan_nn_every, ns.rgan_nn, ns.rgan_nn_images, ns.rgan_nn_side, ns.rgan_nn_k) == (500, True, 1000, 16, 5)
    assert parse(["--rgan_nn_every", "5", "--image_size", "32"]).rgan_nn_side == 64  # the working side is min(64, 32)
    assert parse(["--rgan_nn_every", "5", "--image_size", "256"]).rgan_nn_every == 5
    for argv, text in ((["--rgan_nn_every", "-1"], "--rgan_nn_every must be >= 0"),
                       (["--rgan_nn_images", "3"], "--rgan_nn_images must be >= --rgan_nn_k + 1 = 4"),
                       (["--rgan_nn_k", "0"], "--rgan_nn_k must lie in 1..8"),
                       (["--rgan_nn_k", "9"], "--rgan_nn_k must lie in 1..8"),
                       (["--rgan_nn_side", "24"], "--rgan_nn_side must be one of 8, 16, 32, 64"),
                       (["--rgan_nn_every", "5", "--image_size", "48"], "needs an --image_size it divides"),
                       (["--rgan_nn", "True", "--image_size", "96"], "needs an --image_size it divides"),
                       (["--rgan_nn_every", "5", "--rgan_nn_side", "8", "--image_size", "512"], "by at most 32")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert text in capsys.readouterr().err, argv
    assert validate_nn() is False and validate_nn(5) is True and validate_nn(0, True) is True
    assert validate_nn(5, False, 8192, 64, 3, 32) is True
    monkeypatch.setenv("WORLD_SIZE", "2")
    for argv in (["--rgan_nn_every", "5"], ["--rgan_nn", "True"]):
        with pytest.raises(SystemExit):
            parse(argv)
        assert "single-process" in capsys.readouterr().err
    assert parse([]).rgan_nn_every == 0  # off: data parallel runs are untouched


def test_nn_off_builds_no_check():
    from relativisticgan_amd import train
    from relativisticgan_amd.config import parse
    assert train.make_nn(parse([]), None) is None
    assert train.make_nn(parse(["--rgan_nn_every", "0", "--rgan_nn_images", "64", "--rgan_nn", "True"]), None) is None


def test_private_seed_and_line():
    from relativisticgan_amd import neighbours as nb, swd
    import torch
    assert nb.private_seed(None) == nb.private_seed(nb.DEFAULT_SEED) and nb.private_seed(1) != nb.private_seed(2)
    assert nb.SEED_TAG != swd.SEED_TAG and nb.private_seed(1) != swd.private_seed(1)
    assert nb.DEFAULTS == dict(n_images=8192, side=64, k=3)
    res = dict(fake_nn=31.2045, real_nn=33.0512, ratio=0.9441, precision=0.712, recall=0.388)
    assert nb.format_line(res, 64, 3) == ("NN s64 k3  fake->real: 31.2045  real->real: 33.0512  ratio: 0.9441  "
                                          "precision: 0.7120  recall: 0.3880")
    assert nb.format_line(dict(res, ratio=float("inf")), 8, 1).startswith("NN s8 k1  ") and "ratio: inf" in \
        nb.format_line(dict(res, ratio=float("inf")), 8, 1)
    for vals in ([3.0, 1.0, 2.0], [4.0, 1.0, 2.0, 3.0], [0.1, 0.7], [5.0]):
        assert nb.median(vals) == ref.median(vals)
    d2 = [0, 1, 767, 768, 799027200, 123456789]
    for D in (64, 192, 768, 1024, 12288):
        assert nb.rms(d2, D) == np.sqrt(np.array(d2, dtype=np.float64) / D).tolist()


# ---------------------------------------------------------------- the library
def test_library_exports_the_symbols_and_ops():
    import torch
    from relativisticgan_amd import _lib, ops
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    for name in OPS:
        assert name in ops.OPS and hasattr(torch.ops.rgan, name), name
        assert "rgan::" + name in ops.__doc__
    from relativisticgan_amd.build import SOURCES
    assert "nn.hip" in SOURCES
    from relativisticgan_amd import kernels, neighbours
    assert all(hasattr(neighbours.NearestNeighbours, m) for m in ("query", "report", "grid", "generate", "evaluate"))
    assert all(hasattr(kernels, m) for m in ("nn_row_bytes", "nn_pack_u8", "nn_topk", "nn_covered"))
    assert lib.rgan_abi_version() == 4
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "rgan.h")).read()
    assert "#define RGAN_NN_NO_SELF (-0x7fffffffffffffffLL - 1)" in hdr and kernels.NN_NO_SELF == NO_SELF


def test_sizes():
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    for C in range(0, 6):
        for s in (0, 4, 8, 16, 24, 32, 64, 128):
            legal = 1 <= C <= 4 and s in ref.SIDES and ref.row_bytes(C, s) <= 12288
            assert lib.rgan_nn_row_bytes(C, s) == (ref.row_bytes(C, s) if legal else 0), (C, s)
    assert lib.rgan_nn_row_bytes(4, 64) == 0 and lib.rgan_nn_row_bytes(3, 64) == 12288
    assert lib.rgan_nn_topk_splits(1, 1) == 1 and lib.rgan_nn_topk_splits(0, 5) == 0
    assert lib.rgan_nn_topk_splits(8192, 8192) == 8 and lib.rgan_nn_topk_splits(100, 300) == 3
    assert lib.rgan_nn_topk_ws_bytes(10, 300, 3, 7) == 10 * 7 * 3 * 8
    assert lib.rgan_nn_topk_ws_bytes(10, 300, 3, 0) == 10 * lib.rgan_nn_topk_splits(10, 300) * 3 * 8
    for bad in ((0, 5, 3, 1), (5, 0, 3, 1), (5, 5, 0, 1), (5, 5, 9, 1), (5, 5, 3, -1), (5, 5, 3, 4097),
                (2 ** 28, 5, 8, 1), (2 ** 20, 5, 8, 256)):
        assert lib.rgan_nn_topk_ws_bytes(*bad) == 0, bad


def test_library_rejects_malformed_calls():
    """RGAN_EINVAL (1001) from the host-side checks: nothing is launched and no pointer is read
    (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    a, na, b, nb, d, i, w, r = (ctypes.c_void_p(v) for v in range(0x1000, 0x9000, 0x1000))
    odd = ctypes.c_void_p(0x1008)
    big = 2 ** 62
    strides = ctypes.cast((ctypes.c_longlong * 4)(3072, 1024, 32, 1), ctypes.c_void_p)
    neg = ctypes.cast((ctypes.c_longlong * 4)(3072, 1024, -32, 1), ctypes.c_void_p)
    E = 1001
    # pack
    for args in ((None, 2, 3, 32, strides, 16, d, i), (a, 2, 3, 32, None, 16, d, i), (a, 2, 3, 32, strides, 16, None, i),
                 (a, 2, 3, 32, strides, 16, d, None), (a, 0, 3, 32, strides, 16, d, i), (a, 2, 0, 32, strides, 16, d, i),
                 (a, 2, 5, 32, strides, 16, d, i), (a, 2, 3, 32, strides, 12, d, i), (a, 2, 3, 32, strides, 0, d, i),
                 (a, 2, 3, 48, strides, 32, d, i), (a, 2, 3, 512, strides, 8, d, i), (a, 2, 4, 64, strides, 64, d, i),
                 (a, 2, 3, 16, strides, 32, d, i), (a, 2, 3, 0, strides, 16, d, i), (a, 2, 3, 32, neg, 16, d, i)):
        assert lib.rgan_nn_pack_u8(*args, None) == E, args
    # topk: (a, na, Q, b, nb, R, row_bytes, k, self_offset, nsplit, dist, idx, ws, ws_bytes)
    good = [a, na, 5, b, nb, 7, 64, 3, NO_SELF, 1, d, i, w, big]
    for pos, val in ((0, None), (1, None), (3, None), (4, None), (10, None), (11, None), (12, None),
                     (2, 0), (2, -1), (5, 0), (6, 0), (6, 32), (6, 96), (6, 12288 + 64), (6, -64), (7, 0), (7, 9),
                     (9, -1), (9, 4097), (13, 5 * 3 * 8 - 1), (0, odd), (3, odd), (12, ctypes.c_void_p(0x7004)),
                     (2, 2 ** 28 + 1)):
        args = list(good)
        args[pos] = val
        if pos == 2 and val > 5:
            args[7] = 8  # Q k past int
        assert lib.rgan_nn_topk(*args, None) == E, (pos, val)
    args = list(good)
    args[2], args[9] = 2 ** 20, 4096  # Q nsplit k past int
    assert lib.rgan_nn_topk(*args, None) == E
    # covered: (a, na, Q, b, nb, radius, R, row_bytes, self_offset, flag)
    good = [a, na, 5, b, nb, r, 7, 64, 0, d]
    for pos, val in ((0, None), (1, None), (3, None), (4, None), (5, None), (9, None), (2, 0), (6, 0), (7, 0),
                     (7, 100), (7, 12288 + 64), (0, odd), (3, odd)):
        args = list(good)
        args[pos] = val
        assert lib.rgan_nn_covered(*args, None) == E, (pos, val)


def test_wrappers_refuse_cpu_tensors():
    import torch
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd._lib import RganError
    x = torch.zeros((2, 3, 16, 16), dtype=torch.uint8)
    a, n = torch.zeros((2, 64), dtype=torch.int8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RganError, match="no CPU fallback"):
        K.nn_pack_u8(x, 8)
    with pytest.raises(RganError, match="no CPU fallback"):
        K.nn_topk(a, n, a, n, 1)
    with pytest.raises(RganError, match="no CPU fallback"):
        K.nn_covered(a, n, a, n, n)
    with pytest.raises(RganError, match="no descriptor"):
        K.nn_row_bytes(4, 64)
    assert K.nn_row_bytes(3, 8) == 192


def test_host_argument_checks_under_asan_ubsan():
    """tests/asan/nn_args.cpp against the host half of csrc/nn.hip built with
    -fsanitize=address,undefined (the device half is compiled normally and never launched): a
    stand-alone program, objects cached next to tests/test_host_asan.py's."""
    import subprocess
    from tests import test_host_asan as H
    if not (os.path.exists(H.HIPCC) and os.path.exists(H.CLANG)):
        pytest.skip("needs the ROCm toolchain")
    harness = os.path.join(H.ROOT, "tests", "asan", "nn_args.cpp")
    headers = [os.path.join(H.CSRC, f) for f in os.listdir(H.CSRC) if f.endswith(".h")] + [os.path.join(H.INC, "rgan.h")]
    os.makedirs(H.BUILD, exist_ok=True)
    path = os.path.join(H.CSRC, "nn.hip")
    obj = os.path.join(H.BUILD, f"nn-{H._digest([path] + headers)}.o")  # test_host_asan's names
    if not os.path.exists(obj):
        subprocess.run([H.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I" + H.INC, *H.SAN,
                        "-Wno-unused-result", "-c", path, "-o", obj + ".tmp"], check=True, capture_output=True)
        os.replace(obj + ".tmp", obj)
    hobj = os.path.join(H.BUILD, f"nn_args-{H._digest([harness] + headers)}.o")
    if not os.path.exists(hobj):
        subprocess.run([H.CLANG, "-O1", "-g", "-std=c++17", "-I" + H.INC, "-fsanitize=address", "-fsanitize=undefined",
                        "-fno-sanitize-recover=undefined", "-c", harness, "-o", hobj + ".tmp"], check=True,
                       capture_output=True)
        os.replace(hobj + ".tmp", hobj)
    exe = os.path.join(H.BUILD, "nn_args")
    subprocess.run([H.HIPCC, "--offload-arch=gfx950", *H.SAN, "-o", exe, hobj, obj], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "nn_args ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
