"""The rgan_nn_ kernels (csrc/nn.hip) on the MI355X against the numpy int64 restatement
(tests/nn_ref.py).  Everything is integer, so every comparison is ==."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nn_ref as ref

pytestmark = pytest.mark.gpu

INT32_MAX = ref.INT32_MAX


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def _norms(x):
    return (np.asarray(x, dtype=np.int64) ** 2).sum(axis=1)


def _topk(a, b, k, self_offset=None, nsplit=0):
    """K.nn_topk of int8 numpy rows, back as int64 numpy."""
    from relativisticgan_amd import kernels as K
    dist, idx = K.nn_topk(_dev(a, np.int8), _dev(_norms(a), np.int32), _dev(b, np.int8), _dev(_norms(b), np.int32), k,
                          self_offset=self_offset, nsplit=nsplit)
    assert dist.dtype == idx.dtype == torch.int32 and tuple(dist.shape) == tuple(idx.shape) == (a.shape[0], k)
    return dist.cpu().numpy().astype(np.int64), idx.cpu().numpy().astype(np.int64)


def _covered(a, b, radius, self_offset=None):
    from relativisticgan_amd import kernels as K
    flag = K.nn_covered(_dev(a, np.int8), _dev(_norms(a), np.int32), _dev(b, np.int8), _dev(_norms(b), np.int32),
                        _dev(radius, np.int32), self_offset=self_offset)
    assert flag.dtype == torch.int32 and tuple(flag.shape) == (a.shape[0],)
    return flag.cpu().numpy().astype(np.int64)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"dist {what}"
    assert np.array_equal(got[1], want[1]), f"idx {what}"


def _rows(rng, n, D):
    return rng.integers(-128, 128, size=(n, D)).astype(np.int8)


# ---------------------------------------------------------------- 1. lane map and orientation
def test_lane_map_and_orientation():
    """R = 8 = k: the whole 33 x 8 matrix comes back.  a and b follow different laws, so swapped rows
    and columns, or a k order that differs between the operands, give other numbers."""
    j = np.arange(64)
    a = ((7 * np.arange(33)[:, None] + 3 * j[None, :]) % 251 - 125).astype(np.int8)
    b = ((5 * np.arange(8)[:, None] + 11 * j[None, :]) % 241 - 120).astype(np.int8)
    want = ref.topk(a, b, 8)
    assert (want[1] >= 0).all() and len({tuple(r) for r in want[0]}) > 1
    _same(_topk(a, b, 8), want)
    # the same matrix in its own order: sort each row's (idx, dist) by idx
    got = _topk(a, b, 8)
    order = np.argsort(got[1], axis=1)
    assert np.array_equal(np.take_along_axis(got[0], order, axis=1), ref.dist2(a, b))


# ---------------------------------------------------------------- 2. shapes
QS, RS = (1, 33, 128, 129, 257), (1, 5, 127, 128, 129, 300)
_POOL = {}


def _pool(C, s):
    """257 query and 300 reference descriptors of random byte images, and their distance matrix, once."""
    if (C, s) not in _POOL:
        rng = np.random.default_rng(100 * C + s)
        a, _ = ref.pack(rng.integers(0, 256, size=(max(QS), C, s, s), dtype=np.uint8), s)
        b, _ = ref.pack(rng.integers(0, 256, size=(max(RS), C, s, s), dtype=np.uint8), s)
        _POOL[(C, s)] = a, b, ref.dist2(a, b)
    return _POOL[(C, s)]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("C,s", [(1, 8), (3, 8), (3, 16)])
def test_shapes_around_tile_and_mask_edges(C, s, k):
    a, b, d = _pool(C, s)
    assert a.shape[1] == ref.row_bytes(C, s)
    for Q in QS:
        for R in RS:
            _same(_topk(a[:Q], b[:R], k), ref.topk_d(d[:Q, :R], k), f"Q {Q} R {R}")


def test_long_k():
    from relativisticgan_amd import kernels as K
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=(260, 3, 64, 64), dtype=np.uint8)
    desc, norm = K.nn_pack_u8(torch.from_numpy(img).cuda(), 64)
    want_desc, want_norm = ref.pack(img, 64)
    assert tuple(desc.shape) == (260, 12288) and np.array_equal(desc.cpu().numpy(), want_desc)
    assert np.array_equal(norm.cpu().numpy(), want_norm)
    dist, idx = K.nn_topk(desc[:130], norm[:130], desc[130:], norm[130:], 3)
    _same((dist.cpu().numpy(), idx.cpu().numpy()), ref.topk(want_desc[:130], want_desc[130:], 3))


# ---------------------------------------------------------------- 3. extremes
def test_extremes():
    from relativisticgan_amd import kernels as K
    img = torch.zeros((5, 3, 64, 64), dtype=torch.uint8, device="cuda")
    img[2:] = 255
    desc, norm = K.nn_pack_u8(img, 64)
    assert (desc[:2] == -128).all() and (desc[2:] == 127).all()
    dist, idx = K.nn_topk(desc[:2], norm[:2], desc[2:], norm[2:], 3)
    assert (dist == 799027200).all() and idx.cpu().tolist() == [[0, 1, 2]] * 2
    dist, idx = K.nn_topk(desc[2:], norm[2:], desc[:2], norm[:2], 3)
    assert dist.cpu().tolist() == [[799027200, 799027200, INT32_MAX]] * 3 and idx.cpu().tolist() == [[0, 1, -1]] * 3
    # all-equal rows: every distance is 0, the smallest indices win
    rng = np.random.default_rng(8)
    same = np.repeat(_rows(rng, 1, 192), 200, axis=0)
    for k in (1, 3, 8):
        dist, idx = _topk(same[:70], same, k)
        assert not dist.any() and np.array_equal(idx, np.tile(np.arange(k), (70, 1)))
    # a reference twice, at 3 and 250: 3 first
    b = _rows(rng, 300, 192)
    b[250] = b[3]
    dist, idx = _topk(b[3:4], b, 3)
    assert idx[0, :2].tolist() == [3, 250] and dist[0, :2].tolist() == [0, 0] and dist[0, 2] > 0
    _same((dist, idx), ref.topk(b[3:4], b, 3))
    # fewer references than k
    got = _topk(b[:40], b[:5], 8)
    _same(got, ref.topk(b[:40], b[:5], 8))
    assert (got[0][:, 5:] == INT32_MAX).all() and (got[1][:, 5:] == -1).all() and (got[1][:, :5] >= 0).all()


# ---------------------------------------------------------------- 4. splits
def test_splits_give_identical_results():
    from relativisticgan_amd import _lib
    rng = np.random.default_rng(9)
    b = _rows(rng, 300, 192)
    a = _rows(rng, 140, 192)
    a[0] = b[10]
    b[200] = b[10]  # a tie at distance 0 between parts (10 and 200 lie in different parts from 2 parts on)
    a[1] = b[299]
    for k in (3, 8):
        want = ref.topk(a, b, k)
        assert want[1][0, :2].tolist() == [10, 200]
        # 50 parts hold 6 references each and 300 one each, fewer than k; 301 leaves a part empty
        for nsplit in (1, 2, 3, 7, 0, 50, 300, 301):
            _same(_topk(a, b, k, nsplit=nsplit), want, f"k {k} nsplit {nsplit}")
    assert _lib.lib().rgan_nn_topk_splits(140, 300) == 3  # what 0 stands for here


# ---------------------------------------------------------------- 5. leave-one-out
@pytest.mark.parametrize("lo", [0, 37])
def test_leave_one_out(lo):
    rng = np.random.default_rng(10 + lo)
    b = _rows(rng, 180, 192)
    hi = lo + 131
    q = np.arange(hi - lo)
    got = _topk(b[lo:hi], b, 3, self_offset=lo)
    assert not (got[1] == (q + lo)[:, None]).any()
    _same(got, ref.topk(b[lo:hi], b, 3, self_offset=lo))
    none = _topk(b[lo:hi], b, 3)
    assert np.array_equal(none[1][:, 0], q + lo) and not none[0][:, 0].any()
    _same(none, ref.topk(b[lo:hi], b, 3))
    # an offset that matches no pair excludes nothing
    _same(_topk(b[lo:hi], b, 3, self_offset=-1000), ref.topk(b[lo:hi], b, 3))
    _same(_topk(b[lo:hi], b, 3, self_offset=2 ** 40), ref.topk(b[lo:hi], b, 3))


# ---------------------------------------------------------------- 6. covered
def test_covered():
    rng = np.random.default_rng(12)
    a, b = _rows(rng, 150, 192), _rows(rng, 290, 192)
    d = ref.dist2(a, b)
    for qs, rs in ((0, 0), (77, 131), (149, 289), (130, 5)):
        radius = np.full(290, -1, dtype=np.int64)
        radius[rs] = d[qs, rs]  # equality counts
        got = _covered(a, b, radius)
        assert got[qs] == 1 and np.array_equal(got, ref.covered_d(d, radius))
        radius[rs] -= 1
        got = _covered(a, b, radius)
        assert got[qs] == 0 and np.array_equal(got, ref.covered_d(d, radius))
        radius[rs] += 1
        got = _covered(a, b, radius, self_offset=rs - qs)  # the pair itself is excluded
        assert got[qs] == 0 and np.array_equal(got, ref.covered_d(d, radius, rs - qs))
    lo, hi = int(np.percentile(d, 0.1)), int(np.percentile(d, 2))
    for seed in range(3):
        radius = np.random.default_rng(seed).integers(d.min() - 10, lo if seed else hi, size=290)
        want = ref.covered_d(d, radius)
        assert np.array_equal(_covered(a, b, radius), want)
        if seed == 0:
            assert 0 < want.sum() < 150  # both answers occur
    # leave-one-out against itself: a row is always within radius 0 of itself, which must not count
    zero = np.zeros(290, dtype=np.int64)
    assert _covered(b[20:160], b, zero).all() and not _covered(b[20:160], b, zero, self_offset=20).any()


# ---------------------------------------------------------------- 7. pack
@pytest.mark.parametrize("f", [1, 2, 4, 8])
@pytest.mark.parametrize("C,s", [(1, 8), (3, 8), (3, 16)])
def test_pack(C, s, f):
    from relativisticgan_amd import kernels as K
    S, N = s * f, 5
    rng = np.random.default_rng(1000 * C + 10 * s + f)
    img = rng.integers(0, 256, size=(N, C, S, S), dtype=np.uint8)
    img[1] = rng.integers(0, 2, size=(C, S, S))  # box sums that land exactly on .5 (and .25, .75)
    img[2] = 255
    img[3] = 0
    want_desc, want_norm = ref.pack(img, s)
    if f > 1:
        box = img[1].astype(np.int64).reshape(C, s, f, s, f).sum(axis=(2, 4))
        assert (2 * box == f * f).any()  # the .5 case occurs
    chw = torch.from_numpy(img).cuda()
    hwc = chw.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    parent = torch.zeros(img.size + 1, dtype=torch.uint8, device="cuda")
    parent[1:] = chw.reshape(-1)
    views = {"chw": chw, "hwc": hwc, "offset": parent[1:].view(N, C, S, S)}
    assert (C == 1 or not hwc.is_contiguous()) and views["offset"].data_ptr() % 2 == 1
    for name, view in views.items():
        desc, norm = K.nn_pack_u8(view, s)
        assert desc.dtype == torch.int8 and norm.dtype == torch.int32 and tuple(desc.shape) == (N, ref.row_bytes(C, s))
        assert np.array_equal(desc.cpu().numpy(), want_desc), name
        assert np.array_equal(norm.cpu().numpy().astype(np.int64), want_norm), name
    assert (want_desc[2] == 127).all() and (want_desc[3] == -128).all()
    if f == 1:
        assert np.array_equal(want_desc.astype(np.int64) + 128, img.reshape(N, -1))


# ---------------------------------------------------------------- 8. guard bands
def test_outputs_inside_guard_banded_parents():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd import _lib as L
    rng = np.random.default_rng(13)
    Q, R, k, G = 131, 203, 3, 64
    img = rng.integers(0, 256, size=(Q + R, 3, 16, 16), dtype=np.uint8)
    want_desc, want_norm = ref.pack(img, 8)
    row = want_desc.shape[1]

    def parent(n, dtype, fill):
        return torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")

    pdesc, pnorm = parent((Q + R) * row, torch.int8, 0x5A), parent(Q + R, torch.int32, 0x5A5A5A5A)
    desc, norm = pdesc[G:-G].view(Q + R, row), pnorm[G:-G]
    x = torch.from_numpy(img).cuda()
    strides = (ctypes.c_longlong * 4)(*x.stride())
    L.check(L.lib().rgan_nn_pack_u8(L.ptr(x), Q + R, 3, 16, ctypes.cast(strides, ctypes.c_void_p), 8, L.ptr(desc),
                                    L.ptr(norm), L.stream()), "rgan_nn_pack_u8")
    assert np.array_equal(desc.cpu().numpy(), want_desc) and np.array_equal(norm.cpu().numpy(), want_norm)
    pdist, pidx = parent(Q * k, torch.int32, 0x5A5A5A5A), parent(Q * k, torch.int32, 0x5A5A5A5A)
    out = pdist[G:-G].view(Q, k), pidx[G:-G].view(Q, k)
    K.nn_topk(desc[:Q], norm[:Q], desc[Q:], norm[Q:], k, out=out)
    want = ref.topk(want_desc[:Q], want_desc[Q:], k)
    _same((out[0].cpu().numpy(), out[1].cpu().numpy()), want)
    pflag = parent(Q, torch.int32, 0x5A5A5A5A)
    radius = np.sort(ref.dist2(want_desc[:Q], want_desc[Q:]).reshape(-1))[Q // 2] * np.ones(R, dtype=np.int64)
    K.nn_covered(desc[:Q], norm[:Q], desc[Q:], norm[Q:], _dev(radius, np.int32), out=pflag[G:-G])
    want_flag = ref.covered(want_desc[:Q], want_desc[Q:], radius)
    assert 0 < want_flag.sum() < Q and np.array_equal(pflag[G:-G].cpu().numpy(), want_flag)
    for p, fill in ((pdesc, 0x5A), (pnorm, 0x5A5A5A5A), (pdist, 0x5A5A5A5A), (pidx, 0x5A5A5A5A), (pflag, 0x5A5A5A5A)):
        assert (p[:G] == fill).all() and (p[-G:] == fill).all()
