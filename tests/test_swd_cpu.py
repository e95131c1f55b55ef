"""The sliced Wasserstein metric without a GPU: the float64 restatement (tests/swd_ref.py) pinned
against scipy and against its own properties, the error model the GPU tests rely on checked with
an fp32 emulation, the new flags, the exported symbols and ops, and the host-side argument checks
of csrc/swd.hip and csrc/sort.hip (refused before any launch, also under ASan + UBSan)."""
import ctypes
import os

import numpy as np
import pytest

from tests import swd_ref as ref

NAMES = ("rgan_sort_segments", "rgan_sort_segments_ws_bytes", "rgan_sort_segments_tile", "rgan_swd_load_u8",
         "rgan_swd_pyr_down", "rgan_swd_laplace", "rgan_swd_positions", "rgan_swd_descriptors",
         "rgan_swd_stats_ws_bytes", "rgan_swd_normalize", "rgan_swd_unit_columns", "rgan_swd_project",
         "rgan_swd_l1_ws_bytes", "rgan_swd_l1")
OPS = ("sort_segments", "swd_load_u8", "swd_pyr_down", "swd_laplace", "swd_positions", "swd_descriptors_",
       "swd_normalize_", "swd_unit_columns_", "swd_project", "swd_l1")


def _images(seed, N=4, C=3, S=32):
    return np.random.default_rng(seed).integers(0, 256, size=(N, C, S, S), dtype=np.uint8)


def _draws(seed, N, S, P, K, D, R):
    rng = np.random.default_rng(seed)
    pos = {s: rng.integers(3, s - 3, size=(N, P, 2)).astype(np.int32) for s in ref.sides(S)}
    dirs = [ref.unit_columns(rng.standard_normal((K, D))) for _ in range(R)]
    return pos, dirs


# ---------------------------------------------------------------- the restatement is pinned
def test_down_is_scipy_mirror_convolution():
    ndi = pytest.importorskip("scipy.ndimage")
    x = _images(1, N=2, C=3, S=32).astype(np.float64)
    k2 = np.outer(ref.W5, ref.W5)
    for n in range(2):
        for c in range(3):
            want = ndi.convolve(x[n, c], k2, mode="mirror")[::2, ::2]
            assert np.abs(ref.down(x[n, c]) - want).max() == 0.0
    # the mirror rule spelled out: -1 -> 1, -2 -> 2, H -> H - 2, H + 1 -> H - 3
    H = 8
    ramp = np.arange(H, dtype=np.float64)[None, :] * np.ones((H, 1))
    p = np.pad(ramp, 2, mode="reflect")
    assert p[2, :2].tolist() == [2.0, 1.0] and p[2, -2:].tolist() == [H - 2.0, H - 3.0]


def test_up_by_hand_and_laplacian_of_a_constant():
    # one coarse pixel in the middle: up is 4 x the outer product of the filter around (2y, 2x)
    x = np.zeros((8, 8))
    x[3, 4] = 1.0
    u = ref.up(x)
    want = np.zeros((16, 16))
    want[4:9, 6:11] = 4.0 * np.outer(ref.W5, ref.W5)
    assert np.array_equal(u, want)
    # a constant image: every filter is an average, so each Laplacian level but the last is exactly 0
    lap = ref.laplacian(np.full((1, 1, 64, 64), 77.0))
    assert [s for s in lap] == [64, 32, 16]
    assert (lap[64] == 0).all() and (lap[32] == 0).all() and (lap[16] == 77.0).all()


def test_first_two_down_levels_are_fp32_exact():
    g = ref.gaussian(_images(2, N=2, C=3, S=64).astype(np.float64))
    g.append(ref.down(g[-1]))  # 64 -> 32 -> 16 -> 8
    assert ref.representable(g[1]).all() and ref.representable(g[2]).all()
    assert not ref.representable(g[3]).all()
    # and an fp32 chain reproduces them with difference 0.0
    g32 = ref.gaussian(_images(2, N=2, C=3, S=64).astype(np.float64), ref.to32)
    assert np.abs(g32[1] - g[1]).max() == 0.0 and np.abs(g32[2] - g[2]).max() == 0.0
    assert ref.representable(np.array([0.1, 0.5, 2.0 ** -30, 1.0 + 2.0 ** -24])).tolist() == [False, True, True, False]


# ---------------------------------------------------------------- properties
def test_distance_properties():
    N, C, S, P, D, R = 4, 3, 32, 6, 5, 2
    A, B = _images(3, N, C, S), _images(4, N, C, S)
    pos, dirs = _draws(5, N, S, P, 49 * C, D, R)
    aa = ref.swd(A, A, pos, dirs)
    assert all(v == 0.0 for v in aa.values())
    ab, ba = ref.swd(A, B, pos, dirs), ref.swd(B, A, pos, dirs)
    assert ab == ba and all(v > 0 for v in ab.values())
    assert list(ab) == [32, 16, "avg"] and ab["avg"] == (ab[32] + ab[16]) / 2


def test_sorting_is_1_lipschitz_in_the_max_norm():
    rng = np.random.default_rng(6)
    for n in (1, 2, 17, 1000):
        a = rng.standard_normal(n)
        for scale in (1e-9, 1e-3, 1.0, 100.0):
            b = a + scale * rng.uniform(-1, 1, n)
            assert np.abs(np.sort(a) - np.sort(b)).max() <= np.abs(a - b).max()


def test_normalise_and_unit_columns():
    rng = np.random.default_rng(7)
    d = rng.uniform(0, 255, (40, 147))
    d[:, 49:98] = 12.5  # a constant channel becomes zeros
    n = ref.normalize(d, 3).reshape(40, 3, 49)
    assert (n[:, 1] == 0).all()
    for c in (0, 2):
        assert abs(n[:, c].mean()) < 1e-12 and abs(n[:, c].std() - 1) < 1e-12
    u = ref.unit_columns(rng.standard_normal((49, 7)))
    assert np.abs((u * u).sum(axis=0) - 1).max() < 1e-14


def test_positions_cover_the_interior_exactly():
    for side in (16, 32, 256):
        u = np.array([0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24])
        p = ref.positions(u, side)
        assert p[0] == 3 and p[-1] == side - 4 and p[2] == 3 + (side - 6) // 2
        allu = np.arange(0, 2 ** 24, 4099) * 2.0 ** -24
        q = ref.positions(allu, side)
        assert q.min() == 3 and q.max() == side - 4 and set(np.unique(q)) == set(range(3, side - 3))


def test_total_order_keys_round_trip():
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan, -np.nan], dtype=np.float32)
    k = ref.total_order_keys(x)
    assert np.array_equal(ref.keys_to_floats(k).view(np.uint32), x.view(np.uint32))
    finite = x[:7]
    assert (np.diff(ref.total_order_keys(finite).astype(np.int64)) > 0).all()  # -0 < +0 included


# ---------------------------------------------------------------- the error model
@pytest.mark.parametrize("S", [32, 64, 128])
def test_fp32_pyramid_is_inside_the_stage_bound(S):
    x = _images(8, N=2, C=3, S=S).astype(np.float64)
    exact, single = ref.laplacian(x), ref.laplacian(x, ref.to32)
    bounds = ref.level_bounds(S)
    assert list(bounds) == ref.sides(S)
    for s in exact:
        err = np.abs(single[s] - exact[s]).max()
        print(f"S={S} level {s}: fp32 error {err:.3e}, bound {bounds[s]:.3e}")
        assert err <= bounds[s]


def test_fp32_metric_is_inside_the_projection_bound():
    """The end-to-end bound of tests/test_swd_gpu.py on an fp32 emulation: descriptors rounded to
    fp32, projections accumulated in fp32 in ascending k."""
    N, C, S, P, D, R = 4, 3, 32, 6, 5, 2
    A, B = _images(9, N, C, S), _images(10, N, C, S)
    pos, dirs = _draws(11, N, S, P, 49 * C, D, R)
    want = ref.swd(A, B, pos, dirs)
    dirs32 = [d.astype(np.float32) for d in dirs]
    da, db = ref.descriptors(A, pos, ref.to32), ref.descriptors(B, pos, ref.to32)
    for s in ref.sides(S):
        vals, bound = [], 0.0
        for d32 in dirs32:
            projs = []
            for desc in (da[s], db[s]):
                d32_desc = desc.astype(np.float32)
                acc = np.zeros((desc.shape[0], D), dtype=np.float32)
                for k in range(desc.shape[1]):
                    acc = (acc.astype(np.float64) + d32_desc[:, k:k + 1].astype(np.float64) * d32[k][None, :]
                           ).astype(np.float32)  # one rounding per k, as a fused multiply-add
                projs.append(acc.T.astype(np.float64))
            vals.append(ref.sliced(*projs))
            bound = max(bound, sum(ref.metric_bound(desc, d32, ref.level_bounds(S)[s], sd[s])
                                   for desc, sd in ((da[s], ref.min_std(A, pos)), (db[s], ref.min_std(B, pos)))))
        got = 1000.0 * float(np.mean(vals))
        print(f"level {s}: |fp32 - fp64| = {abs(got - want[s]):.3e}, bound {1000 * bound:.3e}")
        assert abs(got - want[s]) <= 1000.0 * bound


# ---------------------------------------------------------------- flags
def test_flag_defaults_and_refusals(capsys, monkeypatch):
    from relativisticgan_amd.config import make_param, parse
    for ns in (make_param(), parse([])):
        assert (ns.rgan_swd_every, ns.rgan_swd_images) == (0, 8192)
    ns = parse(["--rgan_swd_every", "500", "--rgan_swd_images", "1000"])
    assert (ns.rgan_swd_every, ns.rgan_swd_images) == (500, 1000)
    assert parse(["--rgan_swd_every", "5", "--rgan_pac", "2"]).rgan_swd_every == 5
    for argv, text in ((["--rgan_swd_every", "-1"], "--rgan_swd_every must be >= 0"),
                       (["--rgan_swd_images", "0"], "--rgan_swd_images must be >= 1"),
                       (["--rgan_swd_every", "5", "--image_size", "48"], "power of two")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert text in capsys.readouterr().err, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse(["--rgan_swd_every", "5"])
    assert "single-process" in capsys.readouterr().err
    assert parse([]).rgan_swd_every == 0  # off: data parallel runs are untouched


def test_swd_off_builds_no_metric():
    from relativisticgan_amd import train
    from relativisticgan_amd.config import parse
    assert train.make_swd(parse([]), None) is None
    assert train.make_swd(parse(["--rgan_swd_every", "0", "--rgan_swd_images", "64"]), None) is None


def test_private_seed_and_level_names():
    from relativisticgan_amd import swd
    from relativisticgan_amd.kernels import DeviceRNG
    assert swd.level_sides(32) == [32, 16] and swd.level_sides(256) == [256, 128, 64, 32, 16]
    for bad in (16, 48, 0):
        with pytest.raises(ValueError):
            swd.level_sides(bad)
    assert swd.private_seed(None) == swd.private_seed(swd.DEFAULT_SEED)
    assert swd.private_seed(1) != swd.private_seed(2)
    assert swd.DEFAULTS == dict(n_images=8192, patches=128, repeats=4, dirs=128)
    line = swd.format_line({32: 1.5, 16: 2.25, "avg": 1.875})
    assert line == "SWD x1e3  32: 1.5000  16: 2.2500  avg: 1.8750"


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
    assert "swd.hip" in SOURCES and "sort.hip" in SOURCES
    from relativisticgan_amd import swd
    assert all(hasattr(swd.SlicedWasserstein, m) for m in ("distance", "generate", "evaluate"))
    assert lib.rgan_sort_segments_tile() == 2048 and lib.rgan_abi_version() == 4


def test_library_rejects_malformed_calls():
    """RGAN_EINVAL (1001) from the host-side checks: nothing is launched and no pointer is read
    (they are dummies), so no GPU is needed."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    a, b, c, d = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))
    big = 2 ** 62
    strides = ctypes.cast((ctypes.c_longlong * 4)(3072, 1024, 32, 1), ctypes.c_void_p)
    assert lib.rgan_sort_segments(None, b, c, 2, 8, d, big, None) == 1001
    assert lib.rgan_sort_segments(a, b, c, 0, 8, d, big, None) == 1001
    assert lib.rgan_sort_segments(a, b, c, 2, 0, d, big, None) == 1001
    assert lib.rgan_sort_segments(a, b, c, 2 ** 16, 2 ** 15, d, big, None) == 1001
    assert lib.rgan_sort_segments(a, b, b, 2, 8, d, big, None) == 1001
    assert lib.rgan_sort_segments(a, b, c, 2, 8, d, 16, None) == 1001
    assert lib.rgan_sort_segments_ws_bytes(2 ** 16, 2 ** 15) == 0
    assert lib.rgan_sort_segments_ws_bytes(3, 2049) == 3 * 2 * 1024
    assert lib.rgan_swd_load_u8(a, 2, 3, 0, strides, b, None) == 1001
    assert lib.rgan_swd_load_u8(a, 2, 5, 32, strides, b, None) == 1001
    for S in (0, 16, 48, -32):
        assert lib.rgan_swd_pyr_down(a, 2, 3, S, b, None) == 1001, S
        assert lib.rgan_swd_laplace(a, b, 2, 3, S, c, None) == 1001, S
    assert lib.rgan_swd_pyr_down(a, 2, 3, 32, a, None) == 1001
    assert lib.rgan_swd_positions(a, 4, 6, b, None) == 1001
    assert lib.rgan_swd_descriptors(a, 2, 3, 6, 4, b, c, d, None) == 1001
    assert lib.rgan_swd_descriptors(a, 2, 3, 32, 0, b, c, d, None) == 1001
    assert lib.rgan_swd_normalize(a, 0, 3, b, 2, c, None) == 1001
    assert lib.rgan_swd_unit_columns(a, 49, 513, None) == 1001
    assert lib.rgan_swd_project(a, b, 8, 197, 8, c, None) == 1001
    assert lib.rgan_swd_project(a, b, 2 ** 23, 49, 256, c, None) == 1001
    assert lib.rgan_swd_l1(a, b, 0, c, d, big, None) == 1001
    assert lib.rgan_swd_l1(a, b, 2 ** 31, c, d, big, None) == 1001
    assert lib.rgan_swd_l1_ws_bytes(2 ** 31) == 0 and lib.rgan_swd_l1_ws_bytes(257) == 16


def test_host_argument_checks_under_asan_ubsan():
    """tests/asan/swd_args.cpp against the host halves of csrc/swd.hip and csrc/sort.hip built with
    -fsanitize=address,undefined (the device halves are compiled normally and never launched): a
    stand-alone program, objects cached next to tests/test_host_asan.py's."""
    import subprocess
    from tests import test_host_asan as H
    if not (os.path.exists(H.HIPCC) and os.path.exists(H.CLANG)):
        pytest.skip("needs the ROCm toolchain")
    harness = os.path.join(H.ROOT, "tests", "asan", "swd_args.cpp")
    headers = [os.path.join(H.CSRC, f) for f in os.listdir(H.CSRC) if f.endswith(".h")] + [os.path.join(H.INC, "rgan.h")]
    os.makedirs(H.BUILD, exist_ok=True)
    objs = []
    for stem in ("swd", "sort"):
        path = os.path.join(H.CSRC, stem + ".hip")
        obj = os.path.join(H.BUILD, f"{stem}-{H._digest([path] + headers)}.o")  # test_host_asan's names
        if not os.path.exists(obj):
            subprocess.run([H.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I" + H.INC, *H.SAN,
                            "-Wno-unused-result", "-c", path, "-o", obj + ".tmp"], check=True, capture_output=True)
            os.replace(obj + ".tmp", obj)
        objs.append(obj)
    hobj = os.path.join(H.BUILD, f"swd_args-{H._digest([harness] + headers)}.o")
    if not os.path.exists(hobj):
        subprocess.run([H.CLANG, "-O1", "-g", "-std=c++17", "-I" + H.INC, "-fsanitize=address", "-fsanitize=undefined",
                        "-fno-sanitize-recover=undefined", "-c", harness, "-o", hobj + ".tmp"], check=True,
                       capture_output=True)
        os.replace(hobj + ".tmp", hobj)
    exe = os.path.join(H.BUILD, "swd_args")
    subprocess.run([H.HIPCC, "--offload-arch=gfx950", *H.SAN, "-o", exe, hobj, *objs], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "swd_args ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
