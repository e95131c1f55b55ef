"""rgan_sort_segments on the MI355X: bit-for-bit against numpy's sort of the total-order uint32
keys (tests/swd_ref.py total_order_keys), over every length at which the code takes another path
around its tile T = rgan_sort_segments_tile() (below a wave, a wave, a short last tile, several
tiles), one and several segments, key sets that stress single passes, guard bands around every
buffer at offsets that are 4-byte but not 16-byte aligned, determinism and graph replay."""
import numpy as np
import pytest
import torch

from tests import swd_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN pattern: any stray write or read-through shows
BAND = 37


def _tile():
    from relativisticgan_amd import kernels as K
    return K.sort_segments_tile()


def _keys(kind, nseg, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x = rng.standard_normal((nseg, n)).astype(np.float32)
    elif kind == "equal":
        x = np.full((nseg, n), 1.25, dtype=np.float32)
    elif kind == "two":
        x = rng.choice(np.array([-3.5, 7.0], dtype=np.float32), size=(nseg, n))
    elif kind == "sorted":
        x = np.sort(rng.standard_normal((nseg, n)).astype(np.float32), axis=1)
    elif kind == "reversed":
        x = np.sort(rng.standard_normal((nseg, n)).astype(np.float32), axis=1)[:, ::-1].copy()
    elif kind == "low_byte":  # differ in the lowest byte only: the first pass does all the work
        x = (np.uint32(0x3F800000) | rng.integers(0, 256, size=(nseg, n)).astype(np.uint32)).view(np.float32)
    elif kind == "high_byte":  # differ in the highest byte only: the last pass does
        x = ((rng.integers(0, 256, size=(nseg, n)).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)
    elif kind == "special":
        pool = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                         0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                         0x7FFFFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32)
        x = rng.choice(pool, size=(nseg, n)).view(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def _want(x):
    return ref.keys_to_floats(np.sort(ref.total_order_keys(x), axis=1))


def _banded(nseg, n, device, fill=None):
    """A [nseg][n] float32 view at element offset BAND of a sentinel-filled parent (4-byte aligned,
    not 16-byte aligned)."""
    parent = torch.full((nseg * n + 2 * BAND,), SENTINEL, dtype=torch.int32, device=device)
    view = parent[BAND:BAND + nseg * n].view(torch.float32).view(nseg, n)
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
    if fill is not None:
        view.copy_(torch.from_numpy(fill).to(device))
    return parent, view


def _bands_intact(parent, total):
    p = parent.cpu().numpy()
    return (p[:BAND] == SENTINEL).all() and (p[BAND + total:] == SENTINEL).all()


def _run(x):
    from relativisticgan_amd import kernels as K
    nseg, n = x.shape
    pin, vin = _banded(nseg, n, "cuda", x)
    pout, vout = _banded(nseg, n, "cuda")
    ptmp, vtmp = _banded(nseg, n, "cuda")
    K.sort_segments(vin, out=vout, tmp=vtmp)
    torch.cuda.synchronize()
    got = vout.cpu().numpy()
    assert np.array_equal(vin.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was modified"
    for name, parent in (("in", pin), ("out", pout), ("tmp", ptmp)):
        assert _bands_intact(parent, nseg * n), f"guard band of {name} touched"
    return got


def _lengths():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


KINDS = ["normal", "equal", "two", "sorted", "reversed", "low_byte", "high_byte", "special"]


def test_tile_is_what_the_tests_assume():
    T = _tile()
    assert T >= 256 and T % 64 == 0


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_sort_matches_numpy_bit_for_bit(kind, nseg):
    for n in _lengths():
        x = _keys(kind, nseg, n, seed=1000 * nseg + n)
        got = _run(x)
        assert np.array_equal(got.view(np.uint32), _want(x).view(np.uint32)), (kind, nseg, n)


def test_many_segments_and_blocks():
    T = _tile()
    x = _keys("normal", 130, 2 * T + 1, seed=7)
    x[5] = _keys("special", 1, 2 * T + 1, seed=8)[0]
    x[64] = 0.5
    got = _run(x)
    assert np.array_equal(got.view(np.uint32), _want(x).view(np.uint32))


def test_in_place_and_deterministic():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd import ops  # noqa: F401  (registers the rgan:: operators)
    T = _tile()
    x = _keys("two", 3, 3 * T + 5, seed=9)
    x[1] = _keys("normal", 1, 3 * T + 5, seed=10)[0]
    a, b = _run(x), _run(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    t = torch.from_numpy(x).cuda()
    K.sort_segments(t, out=t)  # out may be the input
    assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert np.array_equal(torch.ops.rgan.sort_segments(torch.from_numpy(x).cuda()).cpu().numpy().view(np.uint32),
                          a.view(np.uint32))


def test_wrapper_refuses_bad_buffers():
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd._lib import RganError
    x = torch.zeros((2, 8), device="cuda")
    with pytest.raises(RganError):
        K.sort_segments(x, tmp=x)
    with pytest.raises(RganError):
        K.sort_segments(x.double())
    with pytest.raises(RganError):
        K.sort_segments(torch.zeros(8, device="cuda"))
    with pytest.raises(RganError):
        K.sort_segments(torch.zeros((2, 0), device="cuda"))


def test_graph_replay_sorts_new_keys():
    from relativisticgan_amd import _lib as L
    T = _tile()
    nseg, n = 3, T + 65
    x0, x1 = _keys("normal", nseg, n, seed=11), _keys("special", nseg, n, seed=12)
    src = torch.from_numpy(x0).cuda()
    out, tmp = torch.empty_like(src), torch.empty_like(src)
    nbytes = L.lib().rgan_sort_segments_ws_bytes(nseg, n)
    ws = L.workspace(nbytes, src.device)

    def call():
        L.check(L.lib().rgan_sort_segments(L.ptr(src), L.ptr(out), L.ptr(tmp), nseg, n, L.ptr(ws), nbytes, L.stream()),
                "rgan_sort_segments")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _want(x0).view(np.uint32))
    src.copy_(torch.from_numpy(x1).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _want(x1).view(np.uint32))
