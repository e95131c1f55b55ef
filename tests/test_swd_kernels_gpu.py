"""The kernels of csrc/swd.hip on the MI355X, each against the float64 restatement
tests/swd_ref.py under the bounds derived there (and checked on the CPU by tests/test_swd_cpu.py):
the pyramid exactly wherever the float64 value is an fp32 number and within the stage bound
elsewhere, the gather bit for bit, the statistics within the double sums' bound, the normalised
values and the unit columns within 2 ulp, the projection within the fixed-order fp32 bound, the L1
sum to 2^-40."""
import numpy as np
import pytest
import torch

from tests import swd_ref as ref

pytestmark = pytest.mark.gpu
RECORD = {}


def _K():
    from relativisticgan_amd import kernels as K
    return K


def _ulp32(x64):
    return np.spacing(np.abs(np.asarray(x64, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------- pyramid
def _pyramid_inputs(N, C, S):
    rng = np.random.default_rng(100 * S + 10 * C + N)
    rand = rng.integers(0, 256, size=(N, C, S, S), dtype=np.uint8)
    spots = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, S // 2), (S - 1, S // 2 - 1), (S // 2, 0),
             (S // 2 - 1, S - 1), (1, 1), (S - 2, S - 2)]  # corners, edge midpoints of both parities, next to a corner
    hot = np.zeros((len(spots), C, S, S), dtype=np.uint8)
    for i, (y, x) in enumerate(spots):
        hot[i, :, y, x] = 255 - i
    const = np.full((1, C, S, S), 77, dtype=np.uint8)
    return {"random": rand, "one_hot": hot, "constant": const}


def _device_levels(u8, layout):
    """{side: Laplacian level} and the Gaussian levels, through the kernels."""
    K = _K()
    t = torch.from_numpy(u8).cuda()
    if layout == "hwc":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # HWC bytes viewed as [N][C][S][S]
        assert not t.is_contiguous() or u8.shape[1] == 1
    g = [K.swd_load_u8(t)]
    while g[-1].shape[-1] > 16:
        g.append(K.swd_pyr_down(g[-1]))
    gauss = [x.cpu().numpy() for x in g]
    apart = [K.swd_laplace(g[k], g[k + 1]).cpu().numpy() for k in range(len(g) - 1)]
    lap = {}
    for k in range(len(g)):
        lev = K.swd_laplace(g[k], g[k + 1], out=g[k]) if k + 1 < len(g) else g[k]  # in place
        lap[int(lev.shape[-1])] = lev.cpu().numpy()
    for k, a in enumerate(apart):
        assert np.array_equal(a.view(np.uint32), lap[a.shape[-1]].view(np.uint32)), "in-place laplace differs"
    return lap, gauss


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("N,C,S", [(2, 3, 32), (1, 1, 64), (3, 3, 64)])
def test_pyramid_against_float64(N, C, S, layout):
    bounds = ref.level_bounds(S)
    worst = 0.0
    for name, u8 in _pyramid_inputs(N, C, S).items():
        lap, gauss = _device_levels(u8, layout)
        want_g = ref.gaussian(u8.astype(np.float64))
        assert np.array_equal(gauss[0], u8.astype(np.float32))
        for k in range(1, len(want_g)):
            assert ref.representable(want_g[k]).all()  # the first two down levels of u8 images
            assert np.array_equal(gauss[k].astype(np.float64), want_g[k]), (name, "G", k)
        want = ref.laplacian(u8.astype(np.float64))
        assert list(lap) == list(want) == ref.sides(S)
        for s in want:
            got = lap[s].astype(np.float64)
            exact = ref.representable(want[s])
            assert np.array_equal(got[exact], want[s][exact]), (name, s, "an fp32-representable value is off")
            err = np.abs(got - want[s]).max()
            assert err <= bounds[s], (name, s, err, bounds[s])
            if bounds[s] > 0:
                worst = max(worst, err / bounds[s])
        if name == "constant":
            for s in ref.sides(S)[:-1]:
                assert (lap[s] == 0).all()
            assert (lap[16] == 77).all()
    RECORD[("pyramid", N, C, S, layout)] = worst
    print(f"pyramid {N}x{C}x{S} {layout}: worst error / bound = {worst:.3e}")


def test_positions_kernel():
    K = _K()
    j = np.array([0, 1, 2 ** 23, 2 ** 24 - 1, 12345678, 2 ** 24 - 2, 5, 2 ** 22 + 1], dtype=np.float64)
    u = (j * 2.0 ** -24).astype(np.float32)
    for side in (16, 32, 64, 256):
        got = K.swd_positions(torch.from_numpy(u).cuda(), side).cpu().numpy()
        assert np.array_equal(got, ref.positions(u, side)), side
        assert got.min() == 3 and got.max() == side - 4
    # values outside [0, 1) are clamped into the interior
    odd = torch.tensor([-1.0, 1.0, 2.5, float("nan")], device="cuda")
    got = K.swd_positions(odd, 32).cpu().numpy()
    assert ((got >= 3) & (got <= 28)).all() and got[0] == 3 and got[1] == 28


# ---------------------------------------------------------------- descriptors, normalise
def _forced_positions(N, P, side, rng):
    ext = [(3, 3), (3, side - 4), (side - 4, 3), (side - 4, side - 4)]
    pos = rng.integers(3, side - 3, size=(N, P, 2)).astype(np.int32)
    for n in range(N):
        for p in range(P):
            i = n * P + p
            if i < 2 * len(ext) or p < min(P, len(ext)) and n == 0:
                pos[n, p] = ext[i % len(ext)]
    return pos


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P", [1, 5, 16])
@pytest.mark.parametrize("side", [16, 32])
def test_descriptors_and_normalise(side, P, C):
    K = _K()
    N = 6
    rng = np.random.default_rng(side + 7 * P + C)
    level = (rng.standard_normal((N, C, side, side)) * 40).astype(np.float32)
    if C == 3:
        level[:, 1] = 12.5  # a constant channel
    pos = _forced_positions(N, P, side, rng)
    assert {tuple(v) for v in pos.reshape(-1, 2)} >= {(3, 3), (3, side - 4), (side - 4, 3), (side - 4, side - 4)}
    M, Kd = N * P, 49 * C
    runs = []
    for _ in range(2):
        desc = torch.full((M, Kd), float("nan"), device="cuda")
        part = torch.zeros((N, C, 2), dtype=torch.float64, device="cuda")
        K.swd_descriptors(torch.from_numpy(level).cuda(), torch.from_numpy(pos).cuda(), desc, part)
        raw = desc.cpu().numpy().copy()
        stats = K.swd_normalize(desc, part)
        runs.append((raw, part.cpu().numpy(), stats.cpu().numpy(), desc.cpu().numpy()))
    raw, part, stats, norm = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "two calls differ"
    want_raw = ref.gather(level, pos)
    assert np.array_equal(raw.view(np.uint32), want_raw.view(np.uint32))
    r64 = want_raw.astype(np.float64).reshape(N, P, C, 49)
    # the per-image sums: a double sum of n terms is within (n - 1) 2^-53 sum |x| of the exact one
    n_img = P * 49
    for c in range(C):
        s, q = r64[:, :, c].sum(axis=(1, 2)), (r64[:, :, c] ** 2).sum(axis=(1, 2))
        assert (np.abs(part[:, c, 0] - s) <= n_img * 2.0 ** -53 * np.abs(r64[:, :, c]).sum(axis=(1, 2))).all()
        assert (np.abs(part[:, c, 1] - q) <= (n_img + 1) * 2.0 ** -53 * q).all()
    mean, std = ref.channel_stats(want_raw, C)
    count = M * 49
    for c in range(C):
        x = r64[:, :, c]
        eps = (count + 2) * 2.0 ** -53
        assert abs(stats[c, 0] - mean[c]) <= eps * np.abs(x).mean() + 2.0 ** -52 * abs(mean[c])
        ms = (x ** 2).mean()
        if std[c] == 0:
            assert stats[c, 1] == 0.0
        else:  # var = E x^2 - mean^2, each within eps of its size; std = sqrt(var)
            dvar = 4 * eps * ms
            assert abs(stats[c, 1] - std[c]) <= dvar / std[c] + 2.0 ** -52 * std[c]
    want = ref.normalize(want_raw, C)
    if C == 3:
        assert (norm.reshape(M, C, 49)[:, 1] == 0).all()
    assert (np.abs(norm.astype(np.float64) - want.astype(np.float32)) <= 2 * _ulp32(want)).all()


def test_descriptor_positions_outside_the_image_are_clamped():
    K = _K()
    side, C = 16, 1
    level = torch.arange(side * side, dtype=torch.float32, device="cuda").view(1, C, side, side).contiguous()
    pos = torch.tensor([[[-5, 100], [0, 0]]], dtype=torch.int32, device="cuda")
    desc = torch.empty((2, 49), device="cuda")
    part = torch.empty((1, 1, 2), dtype=torch.float64, device="cuda")
    K.swd_descriptors(level, pos, desc, part)
    want = ref.gather(level.cpu().numpy(), np.array([[[3, side - 4], [3, 3]]], dtype=np.int32))
    assert np.array_equal(desc.cpu().numpy(), want)


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("M,Kd,D", [(1, 49, 1), (37, 49, 8), (130, 147, 128), (257, 147, 130)])
def test_unit_columns_and_projection(M, Kd, D):
    K = _K()
    rng = np.random.default_rng(M + Kd + D)
    raw = rng.standard_normal((Kd, D)).astype(np.float32)
    dirs = K.swd_unit_columns(torch.from_numpy(raw.copy()).cuda())
    d32 = dirs.cpu().numpy()
    want_u = ref.unit_columns(raw)
    assert (np.abs(d32.astype(np.float64) - want_u.astype(np.float32)) <= 2 * _ulp32(want_u)).all()
    assert np.abs((d32.astype(np.float64) ** 2).sum(axis=0) - 1).max() < 1e-5
    desc = rng.standard_normal((M, Kd)).astype(np.float32)
    guard = torch.full((D * M + 64,), 123.0, device="cuda")
    out = guard[32:32 + D * M].view(D, M)
    got = K.swd_project(torch.from_numpy(desc).cuda(), dirs, out=out).cpu().numpy().astype(np.float64)
    g = guard.cpu().numpy()
    assert (g[:32] == 123.0).all() and (g[32 + D * M:] == 123.0).all()
    want, bound = ref.project(desc, d32), ref.project_bound(desc, d32)
    ratio = np.abs(got - want) / bound
    assert (ratio <= 1).all(), ratio.max()
    again = K.swd_project(torch.from_numpy(desc).cuda(), dirs).cpu().numpy()
    assert np.array_equal(again.astype(np.float64), got)
    RECORD[("project", M, Kd, D)] = float(ratio.max())
    print(f"project {M}x{Kd}x{D}: worst error / bound = {ratio.max():.3e}")


def test_zero_column_stays_zero():
    K = _K()
    raw = torch.ones((49, 3), device="cuda")
    raw[:, 1] = 0
    d = K.swd_unit_columns(raw).cpu().numpy()
    assert (d[:, 1] == 0).all() and np.allclose(d[:, 0], 1 / 7.0, rtol=1e-7)


# ---------------------------------------------------------------- L1
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001, 300001])
def test_l1_against_float64(n):
    K = _K()
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    K.swd_l1(ta, tb, out=out[1:2])
    got = out.cpu().numpy()
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).sum()
    assert got[0] == 0 and got[2] == 0
    assert abs(got[1] - want) <= 2.0 ** -40 * want
    assert K.swd_l1(tb, ta).item() == got[1] and K.swd_l1(ta, ta).item() == 0.0
