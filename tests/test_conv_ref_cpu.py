"""tests/conv_ref.py checked without a GPU: the float64 reference against a naive loop nest, the bound's
two-sided sanity (torch's own fp32 conv inside it, one zeroed tap or pixel outside it) for every case the GPU
edge tests run, the view kinds' strides and alignment, assert_untouched, and the planner's accept / refuse
table through rgan_conv_workspace (the library loads without a GPU, as in tests/test_conv_plan_cpu.py)."""
import ctypes

import pytest
import torch

from tests import conv_ref as R
from tests.conv_ref import Case


def _naive(c, x, w):
    """conv2d / conv_transpose2d as a loop nest over (b, co, oh, ow, ci, kh, kw), float64."""
    Ho, Wo = c.out_hw
    x, w = x.double(), w.double()
    y = torch.zeros(c.yshape, dtype=torch.float64)
    for b in range(c.B):
        for co in range(c.cout):
            for ci in range(c.cin):
                for kh in range(c.k):
                    for kw in range(c.k):
                        for ih in range(c.H):
                            for iw in range(c.W):
                                if c.tr:
                                    oh, ow = ih * c.s - c.p + kh, iw * c.s - c.p + kw
                                    wv = w[ci, co, kh, kw]
                                else:
                                    oh, rh = divmod(ih + c.p - kh, c.s)
                                    ow, rw = divmod(iw + c.p - kw, c.s)
                                    if rh or rw:
                                        continue
                                    wv = w[co, ci, kh, kw]
                                if 0 <= oh < Ho and 0 <= ow < Wo:
                                    y[b, co, oh, ow] += x[b, ci, ih, iw] * wv
    return y


TINY = [Case(2, 2, 3, 4, 4, 3, 2, 1, False), Case(2, 3, 2, 3, 3, 4, 2, 1, True), Case(1, 2, 2, 3, 5, 3, 1, 2, False)]


@pytest.mark.parametrize("c", TINY, ids=lambda c: c.name)
def test_ref_against_loop_nest(c):
    """ref() == the loop nest: the forward with wscale, bias and lrelu; the two gradients as the adjoints of the
    loop nest (<dy, conv(x, w)> is linear in x and in w), element by element."""
    o = R.operands(c, seed=7)
    x, w, dy, bias = o["x"], o["w"], o["dy"], o["bias"]
    lin = _naive(c, x, w)
    val, bnd = R.ref("fwd", c, x, w)
    assert torch.allclose(val, lin, rtol=0, atol=1e-12)
    A = _naive(c, x.abs(), w.abs())
    assert torch.allclose(bnd, 1.01 * (c.K("fwd") + 8) * 2.0 ** -24 * A, rtol=1e-12, atol=0)
    val, bnd = R.ref("fwd", c, x, w, bias=bias, wscale=-0.75, act="lrelu", alpha=0.2)
    v = -0.75 * lin + bias.double().view(1, -1, 1, 1)
    assert torch.allclose(val, torch.where(v >= 0, v, 0.2 * v), rtol=0, atol=1e-12)
    assert torch.allclose(bnd, 1.01 * (c.K("fwd") + 8) * 2.0 ** -24 * (0.75 * A + bias.double().abs().view(1, -1, 1, 1)),
                          rtol=1e-12, atol=0)
    dx, _ = R.ref("dgrad", c, w=w, dy=dy)
    for idx in [(0, 0, 0, 0), (c.B - 1, c.cin - 1, c.H - 1, c.W - 1), (0, 1, 1, 2)]:
        e = torch.zeros(c.xshape)
        e[idx] = 1.0
        assert abs(dx[idx].item() - (_naive(c, e, w) * dy.double()).sum().item()) < 1e-12
    base = o["dw_base"]
    dw, bw = R.ref("wgrad", c, x=x, dy=dy, base=base)
    for idx in [(0, 0, 0, 0), tuple(n - 1 for n in c.wshape), (1, 1, 2, 1)]:
        e = torch.zeros(c.wshape)
        e[idx] = 1.0
        assert abs(dw[idx].item() - base[idx].item() - (_naive(c, x, e) * dy.double()).sum().item()) < 1e-12
        Aw = (_naive(c, x.abs(), e) * dy.double().abs()).sum().item() + abs(base[idx].item())
        assert abs(bw[idx].item() - 1.01 * (c.K("wgrad") + 8) * 2.0 ** -24 * Aw) < 1e-18
    db, bb = R.ref("dbias", c, dy=dy, base=o["db_base"], bias_row0=3)
    rows = dy.double().permute(0, 2, 3, 1).reshape(-1, c.cout)[3:]
    assert torch.allclose(db, rows.sum(0) + o["db_base"].double(), rtol=0, atol=1e-12)
    assert torch.allclose(bb, 1.01 * (c.K("wgrad") + 8) * 2.0 ** -24 * (rows.abs().sum(0) + o["db_base"].double().abs()))


def test_signed_unit():
    t = R.signed_unit((4096,), torch.Generator().manual_seed(1))
    assert t.dtype == torch.float32 and t.abs().min() >= 0.5 and t.abs().max() <= 1.0
    assert 0.4 < (t > 0).float().mean() < 0.6


def test_case_tables_keep_k_small():
    """Every op a family serves, and every accepted op of the geometry table, sums at most 1024 products."""
    for name, (c, ops, _) in R.FAMILIES.items():
        assert all(c.K(op) <= 1024 for op in ops), name
    for fam, c in R.SIZE1:
        assert all(c.K(op) <= 1024 for op in R.FAMILIES[fam][1]), c
        assert 1 in (c.H, c.W)
    for c, _ in R.GEOMETRIES:
        assert all(c.K(op) <= 1024 for op in R.OPS), c
        assert c.B == 2 and max(c.H, c.W) <= 16


def _mutants(c, o, op):
    """(x, w, dy) with one product of ``op`` dropped: one tap of w zeroed (fwd, dgrad) or one pixel of x that
    the output reads (wgrad)."""
    x, w, dy = o["x"].clone(), o["w"].clone(), o["dy"]
    if op == "wgrad":
        # a pixel every geometry of the tables reads: the centre for a ConvT (p > k - 1 crops its corners away),
        # the corner for a Conv (a stride > k or a k1 s2 kernel skips other pixels, never (0, 0))
        ih, iw = (c.H // 2, c.W // 2) if c.tr else (0, 0)
        x[c.B - 1, c.cin - 1, ih, iw] = 0.0
    else:
        w[-1, -1, c.k // 2, c.k // 2] = 0.0
    return x, w, dy


@pytest.mark.parametrize("c", R.all_cases(), ids=lambda c: c.name)
def test_bound_sanity(c):
    """The inputs keep a correct fp32 result inside the bound and a wrong one outside: torch's fp32 CPU conv
    and its autograd gradients pass; with one tap of w (one pixel of x for the weight gradient) zeroed, at
    least one element fails."""
    o = R.operands(c)
    for op in R.OPS:
        if c.K(op) > 1024:
            continue
        val, bnd = R.ref(op, c, o["x"], o["w"], o["dy"])
        got = R.linear(op, c, o["x"], o["w"], o["dy"], dtype=torch.float32)
        assert R.ratio(got, val, bnd) < 1.0, op
        x, w, dy = _mutants(c, o, op)
        bad = R.linear(op, c, x, w, dy, dtype=torch.float32)
        assert R.ratio(bad, val, bnd) > 1.0, op
    db, bb = R.ref("dbias", c, dy=o["dy"])
    assert R.ratio(o["dy"].sum((0, 2, 3)), db, bb) < 1.0
    dy = o["dy"].clone()
    dy[0, :, 0, 0] = 0.0
    assert R.ratio(dy.sum((0, 2, 3)), db, bb) > 1.0


@pytest.mark.parametrize("kind", R.IMAGE_KINDS)
def test_view_kinds(kind):
    """Each kind has the promised strides, offset and alignment, and its elements are distinct."""
    B, C, H, W = shape = (2, 8, 3, 5)
    t, parent = R.view(shape, kind)
    assert tuple(t.shape) == shape and parent.dim() == 1 and parent.storage_offset() == 0
    assert (parent.view(torch.int32) == R.FILL_BITS).all() and torch.isnan(parent).all()
    off = t.storage_offset()
    nhwc = (H * W * C, 1, W * C, C)
    want = {"nhwc": (nhwc, 0), "nchw": ((C * H * W, H * W, W, 1), 0), "off1": (nhwc, 1),
            "batch_slice": (nhwc, H * W * C),
            "chan_slice": ((H * W * (C + 8), 1, W * (C + 8), C + 8), 4),
            "crop": (((H + 2) * (W + 3) * C, 1, (W + 3) * C, C), ((W + 3) + 1) * C)}[kind]
    assert (t.stride(), off) == want
    assert parent.data_ptr() % 16 == 0
    assert (t.data_ptr() % 16 == 0) == (kind != "off1") and t.data_ptr() % 4 == 0
    assert {"batch_slice": (B + 2) * H * W * C, "chan_slice": B * H * W * (C + 8),
            "crop": B * (H + 2) * (W + 3) * C}.get(kind, parent.numel()) == parent.numel()
    # distinct elements, all inside the parent
    t.copy_(torch.arange(t.numel(), dtype=torch.float32).view(B, H, W, C).permute(0, 3, 1, 2))
    inside = parent[~torch.isnan(parent)]
    assert inside.numel() == t.numel() and inside.unique().numel() == t.numel()
    assert parent.numel() > t.numel() or kind in ("nhwc", "nchw")
    R.assert_untouched(parent, t)


@pytest.mark.parametrize("kind", R.FLAT_KINDS)
def test_flat_kinds(kind):
    t, parent = R.flat((3, 2, 4, 4), kind)
    assert t.is_contiguous() and tuple(t.shape) == (3, 2, 4, 4)
    assert t.storage_offset() == (1 if kind == "off1" else 0)
    assert (t.data_ptr() % 16 == 0) == (kind == "plain")
    t.fill_(1.0)
    R.assert_untouched(parent, t)
    assert parent.numel() == t.numel() + (2 if kind == "off1" else 0)


@pytest.mark.parametrize("kind", [k for k in R.IMAGE_KINDS if k not in ("nhwc", "nchw")])
def test_assert_untouched_fires(kind):
    """A one-element write outside the view is caught -- in front of it, behind it and (for the strided kinds)
    in a gap inside its extent -- whether it writes a number or a NaN of another bit pattern."""
    shape = (2, 4, 3, 5)
    t, parent = R.view(shape, kind)
    t.fill_(0.0)
    R.assert_untouched(parent, t)
    inside = torch.zeros(parent.numel(), dtype=torch.bool)
    inside.as_strided(shape, t.stride(), t.storage_offset()).fill_(True)
    outside = (~inside).nonzero().flatten().tolist()
    assert outside
    for i in {outside[0], outside[-1], outside[len(outside) // 2]}:
        p2 = parent.clone()
        t2 = p2.as_strided(shape, t.stride(), t.storage_offset())
        p2[i] = 0.0
        with pytest.raises(AssertionError, match="outside the view"):
            R.assert_untouched(p2, t2)
        p2[i] = float("nan")  # another NaN: a different bit pattern
        with pytest.raises(AssertionError, match="outside the view"):
            R.assert_untouched(p2, t2)


def _desc(c, nchw=False):
    from relativisticgan_amd import _lib
    d = _lib.RganConv()
    Ho, Wo = c.out_hw
    d.batch, d.cin, d.hin, d.win, d.cout, d.hout, d.wout = c.B, c.cin, c.H, c.W, c.cout, Ho, Wo
    d.kh = d.kw = c.k
    d.stride, d.pad, d.transposed = c.s, c.p, int(c.tr)
    xs, ys = R.strides_of(c.xshape, nchw and not c.tr), R.strides_of(c.yshape, nchw and c.tr)
    for i in range(4):
        d.xs[i], d.ys[i] = xs[i], ys[i]
    return d


@pytest.mark.parametrize("c,accept", R.GEOMETRIES, ids=lambda v: v.name if isinstance(v, Case) else "")
def test_planner_accept_refuse_table(c, accept):
    """rgan_conv_workspace(d, which, 0) > 0 exactly where the table says, NHWC and with the image side NCHW."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    for nchw in (False, True):
        d = _desc(c, nchw)
        got = tuple(lib.rgan_conv_workspace(ctypes.byref(d), which, 0) > 0 for which in (0, 1, 2))
        assert got == accept, (c, nchw, got)


def test_family_shapes_are_accepted():
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    for name, (c, ops, layout) in R.FAMILIES.items():
        for cc in [c, c.swapped()] + [s for f, s in R.SIZE1 if f == name]:
            d = _desc(cc, layout == "nchw")
            for op in ops:
                assert lib.rgan_conv_workspace(ctypes.byref(d), R.OPS.index(op), 0) > 0, (name, cc, op)
