"""Float64 reference, a-priori error bound, strided views and the case tables of the conv edge tests.

CPU only (no GPU import): tests/test_conv_ref_cpu.py checks this module without a GPU, and
tests/test_conv_edges_gpu.py runs the HIP conv entry points against it.

Inputs.  ``signed_unit`` draws magnitudes uniform in [0.5, 1] with a random sign, so one dropped,
doubled or misplaced product moves an output element by at least 0.25.

Bound.  Per output element, ``|got - ref| <= 1.01 (K + 8) 2^-24 A``: the standard a-priori bound of
a sum of K fp32 products in any order, A the same operation on the absolute values (plus |bias| and
the |base| of an accumulation), K the most products that feed one element (forward and ConvT data
gradient: taps x cin; Conv data gradient: taps x cout; weight and bias gradient: batch x pixels);
the + 8 covers the wscale multiply, the bias add, the activation multiply and the accumulate add.
With K <= 1024 the bound is at most about 0.063 A-units, a quarter of the smallest wrong product.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24

_Case = namedtuple("Case", "B cin cout H W k s p tr")


class Case(_Case):
    """One conv layer on one input: batch, channels, input map, kernel, stride, pad, transposed."""
    __slots__ = ()

    @property
    def out_hw(self):
        if self.tr:
            return (self.H - 1) * self.s - 2 * self.p + self.k, (self.W - 1) * self.s - 2 * self.p + self.k
        return (self.H + 2 * self.p - self.k) // self.s + 1, (self.W + 2 * self.p - self.k) // self.s + 1

    @property
    def xshape(self):
        return (self.B, self.cin, self.H, self.W)

    @property
    def yshape(self):
        return (self.B, self.cout) + self.out_hw

    @property
    def wshape(self):
        return (self.cin, self.cout, self.k, self.k) if self.tr else (self.cout, self.cin, self.k, self.k)

    def K(self, op):
        """The most products that feed one output element of ``op``."""
        taps = self.k * self.k
        if op == "fwd":
            return taps * self.cin
        if op == "dgrad":
            return taps * (self.cin if self.tr else self.cout)
        return self.B * (self.H * self.W if self.tr else self.out_hw[0] * self.out_hw[1])

    def swapped(self):
        return self._replace(H=self.W, W=self.H)

    @property
    def name(self):
        Ho, Wo = self.out_hw
        return (f"b{self.B}_{'convt' if self.tr else 'conv'}_{self.cin}x{self.H}x{self.W}_to_{self.cout}x{Ho}x{Wo}"
                f"_k{self.k}s{self.s}p{self.p}")


def signed_unit(shape, gen):
    """float32 values with magnitude uniform in [0.5, 1] and a random sign."""
    mag = 0.5 + 0.5 * torch.rand(shape, generator=gen, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64).double() * 2 - 1
    return (mag * sign).float()


def operands(c, seed=0):
    """x, w, dy, bias, dbias base, dw base of a case, from one seeded generator."""
    gen = torch.Generator().manual_seed(1000 + seed)
    return {"x": signed_unit(c.xshape, gen), "w": signed_unit(c.wshape, gen), "dy": signed_unit(c.yshape, gen),
            "bias": signed_unit((c.cout,), gen), "db_base": signed_unit((c.cout,), gen),
            "dw_base": signed_unit(c.wshape, gen)}


def _conv(c, x, w):
    return (F.conv_transpose2d if c.tr else F.conv2d)(x, w, stride=c.s, padding=c.p)


def linear(op, c, x=None, w=None, dy=None, dtype=torch.float64):
    """The bare conv (fwd), its data gradient (dgrad) or weight gradient (wgrad, by autograd) in ``dtype``."""
    cast = lambda t: None if t is None else t.detach().to(dtype).contiguous()  # noqa: E731
    x, w, dy = cast(x), cast(w), cast(dy)
    if op == "fwd":
        return _conv(c, x, w)
    if op == "dgrad":
        x0 = torch.zeros(c.xshape, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(_conv(c, x0, w), x0, dy)[0]
    if op == "wgrad":
        w0 = torch.zeros(c.wshape, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(_conv(c, x, w0), w0, dy)[0]
    raise ValueError(op)


def bound_of(K, A):
    return 1.01 * (K + 8) * U * A


def ref(op, c, x=None, w=None, dy=None, bias=None, wscale=None, act="none", alpha=0.0, base=None, bias_row0=0):
    """(float64 reference, per-element bound) of one entry point.

    op "fwd": act(conv(x, w) wscale + bias); "dgrad": dx = wscale x the data gradient of dy; "wgrad": dw
    (+ base when accumulating); "dbias": dy summed per channel over the pixel rows (b, h, w) from
    ``bias_row0`` on (+ base).  ``act``: "none" or "lrelu" (|act(v)| <= |v|, so the bound stays)."""
    if act not in ("none", "lrelu"):
        raise ValueError(act)
    d = lambda t: None if t is None else t.detach().double()  # noqa: E731
    if op == "dbias":
        rows = d(dy).permute(0, 2, 3, 1).reshape(-1, c.cout)[bias_row0:]
        val, A = rows.sum(0), rows.abs().sum(0)
    else:
        s = 1.0 if wscale is None else float(wscale)
        val = s * linear(op, c, x, w, dy)
        absd = lambda t: None if t is None else t.abs()  # noqa: E731
        A = abs(s) * linear(op, c, absd(x), absd(w), absd(dy))
        if bias is not None:
            if op != "fwd":
                raise ValueError("bias belongs to the forward")
            val = val + d(bias).view(1, -1, 1, 1)
            A = A + d(bias).abs().view(1, -1, 1, 1)
        if act == "lrelu":
            val = torch.where(val >= 0, val, alpha * val)
    if base is not None:
        val, A = val + d(base), A + d(base).abs()
    return val, bound_of(c.K("wgrad" if op == "dbias" else op), A)


def ratio(got, want, bound):
    """max over elements of |got - want| / bound (0 / 0 counts as 0, a NaN or x / 0 as inf)."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return r.max().item() if r.numel() else 0.0


# ----------------------------------------------------------------------------------------- views
FILL_BITS = 0x7FC0BEEF  # a quiet NaN with a payload: no kernel produces it, and it poisons whatever reads it
IMAGE_KINDS = ("nhwc", "nchw", "off1", "batch_slice", "chan_slice", "crop")
FLAT_KINDS = ("plain", "off1")


def _parent(n, device, fill):
    return torch.full((n,), fill, dtype=torch.int32, device=device).view(torch.float32)


def view(shape, kind, device="cpu", fill=FILL_BITS):
    """(tensor of ``shape`` = (B, C, H, W), its flat parent buffer pre-filled with the bit pattern ``fill``).

    nhwc / nchw: dense.  off1: NHWC data one float into its parent (4-byte aligned only).
    batch_slice: samples 1 .. B of a B + 2 parent.  chan_slice: channels [4, 4 + C) of a C + 8 NHWC
    parent (channel stride 1, pixel stride C + 8).  crop: the H x W window at (1, 1) of an
    (H + 2) x (W + 3) NHWC parent."""
    B, C, H, W = shape
    if kind == "nhwc":
        n, off, st = B * H * W * C, 0, (H * W * C, 1, W * C, C)
    elif kind == "nchw":
        n, off, st = B * C * H * W, 0, (C * H * W, H * W, W, 1)
    elif kind == "off1":
        n, off, st = B * H * W * C + 2, 1, (H * W * C, 1, W * C, C)
    elif kind == "batch_slice":
        n, off, st = (B + 2) * H * W * C, H * W * C, (H * W * C, 1, W * C, C)
    elif kind == "chan_slice":
        P = C + 8
        n, off, st = B * H * W * P, 4, (H * W * P, 1, W * P, P)
    elif kind == "crop":
        HP, WP = H + 2, W + 3
        n, off, st = B * HP * WP * C, (WP + 1) * C, (HP * WP * C, 1, WP * C, C)
    else:
        raise ValueError(kind)
    parent = _parent(n, device, fill)
    return parent.as_strided(shape, st, off), parent


def flat(shape, kind, device="cpu", fill=FILL_BITS):
    """(contiguous tensor of ``shape``, its flat parent): plain, or off1 = carved from the parent at offset 1
    (a weight gradient behind a 1-element bias in a flat gradient bucket)."""
    n = 1
    for s in shape:
        n *= s
    if kind == "plain":
        parent, off = _parent(n, device, fill), 0
    elif kind == "off1":
        parent, off = _parent(n + 2, device, fill), 1
    else:
        raise ValueError(kind)
    return parent[off:off + n].view(shape), parent


def assert_untouched(parent, tensor, fill=FILL_BITS):
    """Every parent element outside ``tensor`` (a view of it) still holds the bit pattern ``fill``."""
    bits = parent.detach().clone().view(torch.int32)
    off = tensor.storage_offset() - parent.storage_offset()
    bits.as_strided(tuple(tensor.shape), tensor.stride(), off).fill_(fill)
    bad = (bits != fill).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} elements outside the view were written, first at {bad[:8].tolist()}"


# ----------------------------------------------------------------------------------- case tables
# Kernel families at the smallest non-square (H < W) shape that reaches them; the H > W form is
# Case.swapped().  name: (Case, ops the family serves, image-side layout of the dense form).  The plan each
# reaches (csrc/conv_plan.hip) is stated beside it; K <= 1024 for every listed op.
FAMILIES = {
    # MODE_CONV, vector A loader but not FAST (cin % 32 != 0); dgrad: CONVT2 GEMM; wgrad: generic
    "gemm_scalar": (Case(2, 8, 16, 8, 12, 4, 2, 1, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # MODE_CONV FAST on 64 x 64 tiles; dgrad: FAST CONVT2; wgrad: FAST unsplit (K = 64 rows) with tap staging
    "gemm_fast": (Case(2, 32, 64, 8, 16, 4, 2, 1, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # MODE_CONVT2 forward (4 phases); dgrad: the direct conv (MODE_CONV); wgrad: ConvT generic
    "convt2": (Case(2, 16, 8, 4, 6, 4, 2, 1, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # ... with FAST loaders; wgrad: FAST over a 32-channel dy
    "convt2_fast": (Case(2, 64, 32, 4, 8, 4, 2, 1, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # 1x1 -> 4x4 expansion, N = (oh, ow, co): pack_weights; dgrad: k4 s1 p0 conv over 4x4
    "expand": (Case(3, 16, 32, 1, 1, 4, 1, 0, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # ... FAST on a 1x1 image, pack_t2d (K % 32 == 0, N % 128 == 0)
    "expand_fast": (Case(2, 64, 32, 1, 1, 4, 1, 0, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # k3 s1 p1 GEMM (pack_tiled, not the 16-tap brick); dgrad: flipped pack
    "k3s1p1": (Case(2, 12, 20, 8, 12, 3, 1, 1, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # the wide dense 1x1 layer (M <= 64, N >= 4096, K <= 512): 64 x 64 tiles; its wgrad (K <= 64 rows, M >= 4096)
    # (its data gradient sums 4096 products: outside K <= 1024, and the networks never take it)
    "dense_wide": (Case(2, 32, 4096, 1, 2, 1, 1, 0, False), ("fwd", "wgrad"), "nhwc"),
    # convt2_narrow_mfma, one tile, one channel chunk; dgrad: conv_narrow_in_mfma over the image; wgrad: generic
    "narrow_t": (Case(2, 16, 3, 4, 6, 4, 2, 1, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # ... the channel-split form (4 chunks of 16 channels + the slab reduce)
    "narrow_t_split": (Case(2, 64, 3, 4, 6, 4, 2, 1, True), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # conv_narrow_in_mfma (cout = 8: neither % 128 nor % 32); dgrad: convt2_narrow_mfma; wgrad: generic, N = 48
    "narrow_in": (Case(2, 3, 8, 8, 12, 4, 2, 1, False), ("fwd", "dgrad", "wgrad"), "nchw"),
    # conv_img_in: wout = 32 (swapped: 16); wgrad: generic over K = 1024 rows (its dgrad sums 2048 products)
    "img_in": (Case(2, 3, 128, 32, 64, 4, 2, 1, False), ("fwd", "wgrad"), "nchw"),
    # dense1 fwd / dgrad / wgrad: Conv(C, 1, k, 1, 0) over exactly a k x k map (square by construction)
    "dense1": (Case(2, 16, 1, 4, 4, 4, 1, 0, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # conv3_narrow_out; wgrad: wgrad3_narrow; dgrad: generic GEMM with the flipped pack
    "narrow3_out": (Case(2, 16, 3, 8, 12, 3, 1, 1, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
    # the mirror: k3 s1 p1 Conv 3 -> 8, whose dgrad runs conv3_narrow_out on the flipped kernel
    "narrow3_in": (Case(2, 3, 8, 8, 12, 3, 1, 1, False), ("fwd", "dgrad", "wgrad"), "nchw"),
    # FAST wgrad, split K (K = 256 rows in 2 splits): the RED_TAPS reduce
    "wgrad_split": (Case(2, 32, 64, 16, 32, 4, 2, 1, False), ("wgrad",), "nhwc"),
    # generic wgrad (cin = 24: no whole taps per tile)
    "wgrad_generic": (Case(2, 24, 16, 8, 12, 4, 2, 1, False), ("fwd", "dgrad", "wgrad"), "nhwc"),
}

# One dimension of size 1 where the geometry allows: (family it belongs to, Case)
SIZE1 = [
    ("convt2", Case(2, 16, 8, 1, 5, 4, 2, 1, True)), ("convt2", Case(2, 16, 8, 2, 1, 4, 2, 1, True)),
    ("narrow_t", Case(2, 16, 3, 1, 5, 4, 2, 1, True)), ("narrow_t", Case(2, 16, 3, 2, 1, 4, 2, 1, True)),
    ("convt2_fast", Case(2, 64, 32, 1, 5, 4, 2, 1, True)),
    ("k3s1p1", Case(2, 12, 20, 1, 7, 3, 1, 1, False)), ("narrow3_out", Case(2, 16, 3, 1, 7, 3, 1, 1, False)),
    ("narrow3_in", Case(2, 3, 8, 7, 1, 3, 1, 1, False)),
]

# The planner's accept / refuse table (rgan_conv_workspace(d, which, 0) > 0), batch 2, NHWC:
# (Case, (fwd, dgrad, wgrad) accepted).  A deliberate planner change edits it in review.
Y, N = True, False
GEOMETRIES = [
    (Case(2, 8, 16, 6, 10, 4, 2, 1, False), (Y, Y, Y)),
    (Case(2, 16, 8, 6, 10, 4, 2, 1, True), (Y, Y, Y)),
    (Case(2, 16, 8, 5, 7, 4, 2, 1, True), (Y, Y, Y)),       # k4 s2 p1 ConvT on odd maps
    (Case(2, 16, 8, 1, 5, 4, 2, 1, True), (Y, Y, Y)),
    (Case(2, 16, 8, 2, 1, 4, 2, 1, True), (Y, Y, Y)),
    (Case(2, 16, 8, 1, 1, 4, 2, 1, True), (Y, Y, Y)),
    (Case(2, 8, 16, 5, 7, 4, 2, 1, False), (Y, N, Y)),      # not an exact halving: no CONVT2 data gradient
    (Case(2, 8, 16, 2, 2, 4, 2, 1, False), (Y, Y, Y)),      # 2x2 -> 1x1
    (Case(2, 8, 16, 7, 9, 3, 2, 1, False), (Y, N, Y)),
    (Case(2, 8, 16, 6, 8, 2, 2, 0, False), (Y, N, Y)),
    (Case(2, 8, 16, 7, 9, 1, 2, 0, False), (Y, N, Y)),
    (Case(2, 8, 16, 7, 9, 3, 3, 1, False), (Y, N, Y)),
    (Case(2, 8, 16, 8, 8, 4, 4, 0, False), (Y, N, Y)),
    (Case(2, 8, 16, 6, 6, 6, 2, 2, False), (Y, N, Y)),
    (Case(2, 16, 8, 7, 9, 3, 2, 1, True), (N, Y, Y)),
    (Case(2, 16, 8, 6, 8, 2, 2, 0, True), (N, Y, Y)),
    (Case(2, 8, 16, 7, 9, 5, 1, 2, False), (Y, Y, Y)),
    (Case(2, 16, 8, 7, 9, 5, 1, 2, True), (Y, Y, Y)),       # stride-1 ConvT over a map: the flipped pack
    (Case(2, 8, 16, 7, 9, 3, 1, 2, False), (Y, Y, Y)),      # p > k - 1: negative pad in the flipped data gradient
    (Case(2, 16, 8, 7, 9, 3, 1, 2, True), (Y, Y, Y)),
    (Case(2, 16, 8, 7, 9, 3, 1, 0, True), (Y, Y, Y)),
    (Case(2, 16, 8, 7, 9, 3, 1, 3, True), (Y, Y, Y)),       # p > k - 1: negative effective pad in the forward
    (Case(2, 16, 8, 4, 4, 4, 1, 0, True), (Y, Y, Y)),
    (Case(2, 8, 3, 7, 9, 3, 1, 3, False), (Y, Y, Y)),       # conv3_narrow_out with pad 3
    (Case(2, 3, 8, 7, 9, 3, 1, 3, False), (Y, Y, Y)),       # ... its data gradient with pad 2 - 3 = -1
    (Case(2, 16, 1, 4, 6, 4, 1, 0, False), (Y, Y, Y)),      # 16 -> 1 but not the dense1 shape
    (Case(2, 16, 3, 4, 6, 4, 2, 1, True), (Y, Y, Y)),
    (Case(2, 3, 16, 8, 12, 4, 2, 1, False), (Y, Y, Y)),
]
OPS = ("fwd", "dgrad", "wgrad")


def strides_of(shape, nchw):
    B, C, H, W = shape
    return (C * H * W, H * W, W, 1) if nchw else (H * W * C, 1, W * C, C)


def all_cases():
    """Every Case of the tables above (the bound-sanity check of tests/test_conv_ref_cpu.py runs over it)."""
    out = []
    for c, _, _ in FAMILIES.values():
        out += [c, c.swapped()] if c.H != c.W else [c]
    out += [c for _, c in SIZE1] + [c for c, _ in GEOMETRIES]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq
