"""The conv entry points off the square, dense, aligned path: every kernel family of the planner
(csrc/conv_plan.hip) on non-square maps, on strided and 4-byte-aligned views, at the geometries the planner
accepts beyond the networks' three, with weight and bias gradients written into unaligned slices of a flat
buffer, and the fused BatchNorm / post-op statistics off the square.

Every result is compared element by element with the float64 reference of tests/conv_ref.py under its derived
bound ``|got - ref| <= 1.01 (K + 8) 2^-24 A`` (no global norm, no tuned tolerance), through the Python wrappers
with the bf16x6 emulation off; every output lives in a parent buffer pre-filled with a NaN bit pattern that must
survive outside the view.  The shapes (tests/conv_ref.py FAMILIES, SIZE1, GEOMETRIES) are the smallest that
reach each plan: batch 2 or 3, K <= 1024.  tests/test_conv_ref_cpu.py proves on the CPU that these inputs keep
a correct fp32 result inside the bound and a single dropped product outside it.

With RGAN_CONV_EDGES_RECORD=<file> the module writes one line per section and family: the case count, the
worst error / bound ratio, the seconds spent and the refused views (profiles/conv_edges_mi355x.txt).
"""
import os
import time

import pytest
import torch

from tests import conv_ref as R
from tests.conv_ref import Case

pytestmark = pytest.mark.gpu

DEV = "cuda"
WSCALE, ALPHA = 0.75, 0.2


def _gemm(args):
    """gemm_kernel<MODE (0 CONV, 1 CONVT2, 2 WGRAD), BM, BN, WM, WN, vector A, vector B, FAST>"""
    return f"void rgan::gemm_kernel<{args}>(rgan::GemmArgs)"


# The one kernel the launch profiler reports for the dense, aligned form of (family, op), in both orientations
# (the packs, reduces and the tap transpose are not profiled launches).  Not asserted for the odd views: the
# run-time fallback is the point there.
KERNELS = {
    ("gemm_scalar", "fwd"): _gemm("0, 256, 32, 4, 1, true, true, false"),
    ("gemm_scalar", "dgrad"): _gemm("1, 256, 32, 4, 1, true, true, false"),
    ("gemm_scalar", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
    ("gemm_fast", "fwd"): _gemm("0, 64, 64, 2, 2, true, true, true"),
    ("gemm_fast", "dgrad"): _gemm("1, 256, 32, 4, 1, true, true, true"),
    ("gemm_fast", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, true"),
    ("convt2", "fwd"): _gemm("1, 256, 32, 4, 1, true, true, false"),
    ("convt2", "dgrad"): _gemm("0, 256, 32, 4, 1, true, true, false"),
    ("convt2", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
    ("convt2_fast", "fwd"): _gemm("1, 256, 32, 4, 1, true, true, true"),
    ("convt2_fast", "dgrad"): _gemm("0, 64, 64, 2, 2, true, true, true"),
    ("convt2_fast", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, true"),
    ("expand", "fwd"): _gemm("0, 128, 128, 2, 2, true, true, false"),
    ("expand", "dgrad"): _gemm("0, 256, 32, 4, 1, true, true, true"),
    ("expand", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
    ("expand_fast", "fwd"): _gemm("0, 128, 128, 2, 2, true, true, true"),
    ("expand_fast", "dgrad"): _gemm("0, 64, 64, 2, 2, true, true, true"),
    ("expand_fast", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
    ("k3s1p1", "fwd"): _gemm("0, 256, 32, 4, 1, true, true, false"),
    ("k3s1p1", "dgrad"): _gemm("0, 256, 32, 4, 1, true, true, false"),
    ("k3s1p1", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
    ("dense_wide", "fwd"): _gemm("0, 64, 64, 2, 2, true, true, true"),
    ("dense_wide", "wgrad"): _gemm("2, 64, 64, 2, 2, true, true, false"),
    ("narrow_t", "fwd"): "void rgan::convt2_narrow_mfma<NC>(rgan::NarrowArgs)",
    ("narrow_t", "dgrad"): "void rgan::conv_narrow_in_mfma<CI>(rgan::NarrowArgs)",
    ("narrow_t", "wgrad"): _gemm("2, 128, 64, 2, 2, true, false, false"),
    ("narrow_t_split", "fwd"): "void rgan::convt2_narrow_mfma<NC>(rgan::NarrowArgs)",
    ("narrow_t_split", "dgrad"): "void rgan::conv_narrow_in_mfma<CI>(rgan::NarrowArgs)",
    ("narrow_t_split", "wgrad"): _gemm("2, 128, 64, 2, 2, true, false, false"),
    ("narrow_in", "fwd"): "void rgan::conv_narrow_in_mfma<CI>(rgan::NarrowArgs)",
    ("narrow_in", "dgrad"): "void rgan::convt2_narrow_mfma<NC>(rgan::NarrowArgs)",
    ("narrow_in", "wgrad"): _gemm("2, 128, 64, 2, 2, true, false, false"),
    ("img_in", "fwd"): "void rgan::conv_img_in<CI, WT, ACT>(rgan::NarrowArgs)",
    ("img_in", "wgrad"): _gemm("2, 128, 64, 2, 2, true, false, false"),
    ("dense1", "fwd"): "void rgan::dense1_fwd<VEC>(rgan::DenseArgs)",
    ("dense1", "dgrad"): "void rgan::dense1_dgrad<VEC>(rgan::DenseArgs, rgan::FastDiv)",
    ("dense1", "wgrad"): "rgan::dense1_wgrad(rgan::DenseArgs)",
    ("narrow3_out", "fwd"): "void rgan::conv3_narrow_out<NC>(rgan::NarrowArgs, int)",
    ("narrow3_out", "dgrad"): _gemm("0, 256, 32, 4, 1, false, true, false"),
    ("narrow3_out", "wgrad"): "void rgan::wgrad3_narrow<NC>(rgan::NarrowArgs, int, int)",
    ("narrow3_in", "fwd"): _gemm("0, 256, 32, 4, 1, false, true, false"),
    ("narrow3_in", "dgrad"): "void rgan::conv3_narrow_out<NC>(rgan::NarrowArgs, int)",
    ("narrow3_in", "wgrad"): _gemm("2, 64, 64, 2, 2, true, false, false"),
    ("wgrad_split", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, true"),
    ("wgrad_generic", "fwd"): _gemm("0, 256, 32, 4, 1, true, true, false"),
    ("wgrad_generic", "dgrad"): _gemm("1, 256, 32, 4, 1, true, true, false"),
    ("wgrad_generic", "wgrad"): _gemm("2, 128, 128, 2, 2, true, true, false"),
}

# Views that are refused (RganError before any launch, nothing written), as (family, op, operand, kind).  Every
# other vector / FAST path falls back to a scalar one.  These three are narrow plans whose input must be 16-byte
# aligned: rgan_conv_workspace plans without pointers and sizes the workspace for the narrow kernel, the entry
# point then plans the GEMM fallback for the 4-byte-aligned input, which needs a weight pack the workspace has no
# room for.  (convt2_narrow_mfma's one-chunk form runs: its own pack happens to be large enough.)
REFUSED = {
    ("narrow_t_split", "fwd", "x", "off1"),
    ("narrow3_out", "fwd", "x", "off1"),
    ("narrow3_in", "dgrad", "dy", "off1"),
}

# The 1x1 -> 4x4 expansion takes no bias (include/rgan.h rgan_conv_fwd): its "full" forward is wscale + lrelu.
NO_BIAS = ("expand", "expand_fast")

_RECORD = {}


def _note(section, family, r=0.0, refused=None, seconds=0.0):
    e = _RECORD.setdefault((section, family), [0, 0.0, [], 0.0])
    e[0] += 1
    e[1] = max(e[1], r)
    e[3] += seconds
    if refused:
        e[2].append(refused)


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    prev = kernels.set_gemm_emulation(False)
    yield kernels
    kernels.set_gemm_emulation(prev)
    path = os.environ.get("RGAN_CONV_EDGES_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("section family cases worst_err_over_bound seconds refused\n")
            for (section, family), (n, worst, refused, sec) in sorted(_RECORD.items()):
                f.write(f"{section} {family} {n} {worst:.4f} {sec:.3f} {','.join(refused) or '-'}\n")
            for key, names in sorted(_SEEN.items()):
                f.write(f"kernels {key[0]} {key[1]} {names}\n")


_SEEN = {}
_OPS, _REFS = {}, {}


def _operands(c):
    if c not in _OPS:
        _OPS[c] = R.operands(c)
    return _OPS[c]


def _ref(c, op, variant="full", row0=0):
    """The shared float64 references: fwd "full" = bias + wscale + lrelu, "scaled" = without the bias, "plain" =
    the bare conv; dgrad with
    wscale; wgrad / dbias written ("plain") or accumulated on the random base ("acc")."""
    key = (c, op, variant, row0)
    if key not in _REFS:
        o = _operands(c)
        if op == "fwd":
            kw = dict(wscale=WSCALE, act="lrelu", alpha=ALPHA) if variant != "plain" else {}
            if variant == "full":
                kw["bias"] = o["bias"]
            _REFS[key] = R.ref("fwd", c, o["x"], o["w"], **kw)
        elif op == "dgrad":
            _REFS[key] = R.ref("dgrad", c, w=o["w"], dy=o["dy"], wscale=WSCALE)
        elif op == "wgrad":
            _REFS[key] = R.ref("wgrad", c, x=o["x"], dy=o["dy"], base=o["dw_base"] if variant == "acc" else None)
        else:
            _REFS[key] = R.ref("dbias", c, dy=o["dy"], base=o["db_base"] if variant == "acc" else None,
                               bias_row0=row0)
    return _REFS[key]


def _sync():
    """Wait for the kernels; a device fault ends the whole session (nothing more runs on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, stopping the session: {e}", returncode=3)


def _img(data, kind):
    t, parent = R.view(tuple(data.shape), kind, DEV)
    t.copy_(data.to(DEV))
    return t, parent


def _flat(data, kind):
    t, parent = R.flat(tuple(data.shape), kind, DEV)
    t.copy_(data.to(DEV))
    return t, parent


def _geom(K, c):
    return K.ConvGeom(c.k, c.s, c.p, c.tr)


def _run(K, c, op, xk="nhwc", yk="nhwc", wk="plain", bk="plain", variant="full"):
    """One call with x / y-side / w / bias in the given view kinds.  Returns (got, reference, bound, refused).
    Checks that the inputs are unchanged and every parent is untouched outside its view, also after a refusal."""
    o = _operands(c)
    g = _geom(K, c)
    ins = []   # (tensor, parent, data)
    scale = torch.tensor([WSCALE], device=DEV)

    def put(name, kind, image=True):
        t, parent = (_img if image else _flat)(o[name], kind)
        ins.append((t, parent, o[name]))
        return t

    refused = False
    try:
        if op == "fwd":
            x, w = put("x", xk), put("w", wk, False)
            out, outp = R.view(c.yshape, yk, DEV)
            if variant == "full":
                K.conv_fwd(x, w, g, bias=put("bias", bk, False), act="lrelu", alpha=ALPHA, wscale=scale, out=out)
            elif variant == "scaled":
                K.conv_fwd(x, w, g, act="lrelu", alpha=ALPHA, wscale=scale, out=out)
            else:
                K.conv_fwd(x, w, g, out=out)
        elif op == "dgrad":
            dy, w = put("dy", yk), put("w", wk, False)
            out, outp = R.view(c.xshape, xk, DEV)
            K.conv_dgrad(dy, w, g, c.xshape, wscale=scale, out=out)
        else:
            x, dy = put("x", xk), put("dy", yk)
            out, outp = R.flat(c.wshape, wk, DEV)
            K.conv_wgrad(x, dy, g, c.wshape, into=out)
    except K.L.RganError:
        refused = True
    _sync()
    for t, parent, data in ins:
        assert torch.equal(t.cpu(), data), "an input was modified"
        R.assert_untouched(parent, t)
    if refused:
        assert (outp.view(torch.int32) == R.FILL_BITS).all(), "a refused op wrote to its output"
        return None, None, None, True
    R.assert_untouched(outp, out)
    val, bnd = _ref(c, op, variant)
    return out, val, bnd, False


def _profiled(K, fn):
    K.profile_begin(64)
    try:
        out = fn()
    finally:
        prof = K.profile_end()
    return out, [k["name"] for k in prof["kernels"]]


FAMILY_OPS = [(f, op) for f, (_, ops, _) in R.FAMILIES.items() for op in ops]


def _full(family):
    return "scaled" if family in NO_BIAS else "full"


def _dense_kinds(family, op):
    """The dense form: the family's image-side layout on the image-side tensor, NHWC elsewhere."""
    c, _, layout = R.FAMILIES[family]
    return (layout, "nhwc") if not c.tr else ("nhwc", layout)


# --------------------------------------------------------------------------- b. dense form, non-square maps
@pytest.mark.parametrize("family,op", FAMILY_OPS)
def test_dense_nonsquare(K, family, op):
    """Section b: every family at H < W and at H > W (and with one dimension of size 1 where the geometry
    allows), dense and aligned, against float64 element by element; the launch profiler names the family's
    kernel.  The forward runs both bare and with wscale, bias and lrelu."""
    c0, _, _ = R.FAMILIES[family]
    xk, yk = _dense_kinds(family, op)
    cases = [c0] + ([c0.swapped()] if c0.H != c0.W else []) + [s for f, s in R.SIZE1 if f == family]
    bad = []
    for c in cases:
        for variant in (("plain", _full(family)) if op == "fwd" else ("full",)):
            t0 = time.perf_counter()
            (got, val, bnd, refused), names = _profiled(K, lambda: _run(K, c, op, xk, yk, variant=variant))
            assert not refused, (c, op)
            r = R.ratio(got, val, bnd)
            _note("b_nonsquare", family, r, seconds=time.perf_counter() - t0)
            print(f"{family} {op} {c.name} {variant}: err/bound {r:.4f} kernels {names}")
            if r > 1.0:
                bad.append((c.name, variant, r))
            if c in (c0, c0.swapped()) and variant != "plain":
                _SEEN.setdefault((family, op), set()).add(tuple(names))
                assert names == [KERNELS[family, op]], (c.name, names)
    assert not bad, bad


# ------------------------------------------------------------------------------ a. views, one factor at a time
def _view_cases(op, what, xk0, yk0, bias=True):
    """(operand, kinds of x, y side, w, bias) for one section-a test."""
    out = []
    if what == "in":
        if op in ("fwd", "wgrad"):
            out += [("x", k, yk0, "plain", "plain") for k in R.IMAGE_KINDS]
        if op in ("dgrad", "wgrad"):
            out += [("dy", xk0, k, "plain", "plain") for k in R.IMAGE_KINDS]
    elif what == "out":
        if op == "fwd":
            out += [("y", xk0, k, "plain", "plain") for k in R.IMAGE_KINDS]
        elif op == "dgrad":
            out += [("dx", k, yk0, "plain", "plain") for k in R.IMAGE_KINDS]
        else:
            out += [("dw", xk0, yk0, k, "plain") for k in R.FLAT_KINDS]
    else:
        if op != "wgrad":
            out.append(("w", xk0, yk0, "off1", "plain"))
        if op == "fwd" and bias:
            out.append(("bias", xk0, yk0, "plain", "off1"))
    return out


@pytest.mark.parametrize("what", ["in", "out", "wb"])
@pytest.mark.parametrize("family,op", FAMILY_OPS)
def test_views(K, family, op, what):
    """Section a: one operand at a time in every view kind (the others dense): the input operand(s), then the
    output with its parent pre-filled and checked untouched, then w and bias one float into their parents.  A
    view the planner refuses must raise RganError, write nothing and be listed in REFUSED."""
    c, _, _ = R.FAMILIES[family]
    xk0, yk0 = _dense_kinds(family, op)
    bad = []
    for operand, xk, yk, wk, bk in _view_cases(op, what, xk0, yk0, family not in NO_BIAS):
        kind = {"x": xk, "dx": xk, "dy": yk, "y": yk, "w": wk, "dw": wk, "bias": bk}[operand]
        t0 = time.perf_counter()
        got, val, bnd, refused = _run(K, c, op, xk, yk, wk, bk, variant=_full(family) if op == "fwd" else "full")
        key = (family, op, operand, kind)
        if refused or key in REFUSED:
            _note("a_views", family, 0.0, refused=f"{op}:{operand}:{kind}", seconds=time.perf_counter() - t0)
            assert refused and key in REFUSED, (key, "refused" if refused else "ran, but is listed as refused")
            continue
        r = R.ratio(got, val, bnd)
        _note("a_views", family, r, seconds=time.perf_counter() - t0)
        print(f"{family} {op} {operand}={kind}: err/bound {r:.4f}")
        if r > 1.0:
            bad.append((operand, kind, r))
    assert not bad, bad


@pytest.mark.parametrize("family", NO_BIAS)
@pytest.mark.parametrize("fused_bn", [False, True], ids=["fwd", "fwd_bn"])
def test_expansion_bias_refused(K, family, fused_bn):
    """The 1x1 -> 4x4 expansion's GEMM has N = (oh, ow, co) columns and its epilogues read bias[n]: with a bias it
    is refused before any launch (it used to read past the bias: err / bound 1.8e4 and NaNs at these shapes,
    profiles/conv_edges_mi355x.txt)."""
    c = R.FAMILIES[family][0]
    o = _operands(c)
    x, w, bias = o["x"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV)
    out, outp = R.view(c.yshape, "nhwc", DEV)
    with pytest.raises(K.L.RganError):
        if fused_bn:
            K.conv_fwd_bn(x, w, _geom(K, c), bias=bias)
        else:
            K.conv_fwd(x, w, _geom(K, c), bias=bias, out=out)
    _sync()
    assert (outp.view(torch.int32) == R.FILL_BITS).all()
    _note("a_views", family, 0.0, refused="fwd_bn:bias" if fused_bn else "fwd:bias")


# ----------------------------------------------------------------------------------- c. the geometry table
@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("c,accept", R.GEOMETRIES, ids=lambda v: v.name if isinstance(v, Case) else "")
def test_geometries(K, c, accept, nchw):
    """Section c: every accepted op of the planner's table against float64, NHWC and with the image side NCHW;
    every refused op raises RganError and writes nothing."""
    kind = "nchw" if nchw else "nhwc"
    xk, yk = ("nhwc", kind) if c.tr else (kind, "nhwc")
    bad = []
    for op, ok in zip(R.OPS, accept):
        t0 = time.perf_counter()
        got, val, bnd, refused = _run(K, c, op, xk, yk)
        assert refused == (not ok), (c.name, op, "refused" if refused else "accepted")
        r = 0.0 if refused else R.ratio(got, val, bnd)
        _note("c_geometry", f"{'convt' if c.tr else 'conv'}_k{c.k}s{c.s}p{c.p}", r,
              refused=f"{c.name}:{op}" if refused else None, seconds=time.perf_counter() - t0)
        print(f"{c.name} {kind} {op}: " + ("refused" if refused else f"err/bound {r:.4f}"))
        if r > 1.0:
            bad.append((op, r))
    assert not bad, bad


# ------------------------------------------------------- d. weight and bias gradients into unaligned storage
ONE_PIXEL = Case(2, 8, 16, 2, 2, 4, 2, 1, False)   # hout * wout == 1 through the generic GEMM (dense1 is the other)
WGRAD_CASES = [(f, R.FAMILIES[f][0]) for f, (_, ops, _) in R.FAMILIES.items() if "wgrad" in ops] + \
              [("one_pixel", ONE_PIXEL)]


@pytest.mark.parametrize("family,c", WGRAD_CASES, ids=[f for f, _ in WGRAD_CASES])
def test_wgrad_unaligned(K, family, c):
    """Section d: the data-parallel gradient bucket made explicit -- dw and dbias as 4-byte-aligned slices of
    flat buffers: written (``into=``; with NCHW dy and a bias, which the wrapper converts) and accumulated on a
    random base (``out=`` / ``out_bias=``) with bias_row0 in {0, 32, 5} where the pixel rows allow; the parents
    are untouched outside the slices."""
    o = _operands(c)
    g = _geom(K, c)
    lay = R.FAMILIES[family][2] if family in R.FAMILIES else "nhwc"
    x, _ = _img(o["x"], lay if not c.tr else "nhwc")
    rows = c.yshape[0] * c.yshape[2] * c.yshape[3]
    bad = []

    def check(what, got, parent, val, bnd, t0):
        R.assert_untouched(parent, got)
        r = R.ratio(got, val, bnd)
        _note("d_wgrad_unaligned", family, r, seconds=time.perf_counter() - t0)
        print(f"{family} {what}: err/bound {r:.4f}")
        if r > 1.0:
            bad.append((what, r))

    for dyk in ("nhwc", "nchw"):
        t0 = time.perf_counter()
        dy, _ = _img(o["dy"], dyk)
        dw, dwp = R.flat(c.wshape, "off1", DEV)
        _, db = K.conv_wgrad(x, dy, g, c.wshape, with_bias=True, into=dw)
        _sync()
        check(f"into dy={dyk}", dw, dwp, *_ref(c, "wgrad", "plain"), t0)
        check(f"dbias dy={dyk}", db, db, *_ref(c, "dbias", "plain"), t0)
    dy, _ = _img(o["dy"], "nhwc")
    for row0 in (0, 32, 5):
        if row0 >= rows:
            continue
        t0 = time.perf_counter()
        dw, dwp = _flat(o["dw_base"], "off1")
        db, dbp = _flat(o["db_base"], "off1")
        K.conv_wgrad(x, dy, g, c.wshape, with_bias=True, out=dw, out_bias=db, bias_row0=row0)
        _sync()
        check(f"accumulate row0={row0}", dw, dwp, *_ref(c, "wgrad", "acc"), t0)
        check(f"dbias accumulate row0={row0}", db, dbp, *_ref(c, "dbias", "acc", row0), t0)
    # accumulated without a bias, into an aligned and an unaligned slice
    for kind in R.FLAT_KINDS:
        t0 = time.perf_counter()
        dw, dwp = _flat(o["dw_base"], kind)
        K.conv_wgrad(x, dy, g, c.wshape, out=dw)
        _sync()
        check(f"accumulate {kind} no bias", dw, dwp, *_ref(c, "wgrad", "acc"), t0)
    assert not bad, bad


# ------------------------------------------------------------------------ e. fused statistics off the square
# the smallest shapes for which rgan_conv_bn_segments / rgan_conv_post_segments answer > 0 (two samples of 4 x 16
# pixels: M = 128 rows, 64 per batch segment): (Case, segs of conv_fwd_bn, phases of its forward / data gradient)
STATS_CONV = Case(2, 32, 64, 8, 32, 4, 2, 1, False)    # fwd: CONV, S = 2; dgrad: CONVT2, 4 phases, S = 8
STATS_CONVT = Case(2, 64, 32, 4, 16, 4, 2, 1, True)    # fwd: CONVT2, 4 phases, S = 8 (one batch segment only);
#                                                        dgrad: CONV, S = 2


def _sum_bound(c, op, A):
    """The bound of a sum of elements whose own bounds are built on A: K + 64 for the 64-row add chain."""
    return R.bound_of(c.K(op) + 64, A)


def _rows(t):
    """[B, C, H, W] -> pixel rows [B * H * W, C] in (b, h, w) order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("xkind", ["nhwc", "batch_slice"])
@pytest.mark.parametrize("c,segs", [(STATS_CONV, 1), (STATS_CONV, 2), (STATS_CONVT, 1)],
                         ids=["conv_segs1", "conv_segs2", "convt_segs1"])
def test_fwd_bn_segments(K, c, segs, xkind):
    """Section e: conv_fwd_bn on a non-square map (and on a batch_slice input): the sums are fused, y is inside
    the bound, and the segment sums (sum y, sum y^2) match float64 sums of the float64 reference -- per batch
    segment (for the 4-phase ConvT: the phase-major segments add up to torch's per-channel totals) and, for a
    one-phase GEMM, per 64-row segment."""
    t0 = time.perf_counter()
    o = _operands(c)
    x, xp = _img(o["x"], xkind)
    w, bias = o["w"].to(DEV), o["bias"].to(DEV)
    d = K._desc(c.xshape, x.stride(), c.yshape, R.strides_of(c.yshape, False), _geom(K, c))
    import ctypes
    assert K.L.lib().rgan_conv_bn_segments(ctypes.byref(d), segs) > 0
    y, part, S = K.conv_fwd_bn(x, w, _geom(K, c), bias=bias, segs=segs)
    _sync()
    assert part is not None and S > 0 and tuple(part.shape) == (S, 2, c.cout)
    R.assert_untouched(xp, x)
    val, bnd = R.ref("fwd", c, o["x"], o["w"], bias=o["bias"])
    r = R.ratio(y, val, bnd)
    # per-element bounds of y^2: 2 |y| b + b^2
    A = bnd / R.bound_of(c.K("fwd"), 1.0)
    b1 = _sum_bound(c, "fwd", A)
    b2 = 2 * val.abs() * b1 + b1 * b1
    part = part.cpu()
    Bs = c.B // segs
    for k in range(segs):
        sl = slice(k * Bs, (k + 1) * Bs)
        got = part[k * S // segs:(k + 1) * S // segs].sum(0)
        r = max(r, R.ratio(got[0], _rows(val[sl]).sum(0), _rows(b1[sl]).sum(0)),
                R.ratio(got[1], (_rows(val[sl]) ** 2).sum(0), _rows(b2[sl]).sum(0)))
    if not c.tr:  # one phase: segment s = rows [64 s, 64 s + 64)
        rv, rb1, rb2 = (_rows(t).view(S, 64, c.cout) for t in (val, b1, b2))
        r = max(r, R.ratio(part[:, 0], rv.sum(1), rb1.sum(1)), R.ratio(part[:, 1], (rv ** 2).sum(1), rb2.sum(1)))
    _note("e_fused_stats", f"fwd_bn_{'convt' if c.tr else 'conv'}", r, seconds=time.perf_counter() - t0)
    print(f"fwd_bn {c.name} segs {segs} x={xkind}: err/bound {r:.4f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("dykind", ["nhwc", "batch_slice"])
@pytest.mark.parametrize("mode,nseg", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("c", [STATS_CONV, STATS_CONVT], ids=["conv_dgrad_convt2", "convt_dgrad_conv"])
def test_dgrad_post_segments(K, c, mode, nseg, dykind):
    """Section e: the producer post-op in the data-gradient GEMM on a non-square map (and a batch_slice dy):
    mode 1 out = v act'(a); mode 2 out = g = v act'(BN(y)) and the BatchNorm backward sums (sum g,
    sum g (y - mean)) per segment -- fused, inside the bound, and the segments of each batch segment (phase-major
    for the 4-phase CONVT2 data gradient of a Conv) add up to float64 per-channel totals of the reference."""
    import ctypes
    t0 = time.perf_counter()
    o = _operands(c)
    gen = torch.Generator().manual_seed(77)
    dy, dyp = _img(o["dy"], dykind)
    w = o["w"].to(DEV)
    g = _geom(K, c)
    v, bnd = R.ref("dgrad", c, w=o["w"], dy=o["dy"])
    a = R.signed_unit(c.xshape, gen)            # mode 1: the activation output; mode 2: the BatchNorm input y
    a_dev, _ = _img(a, "nhwc")
    if mode == 1:
        post = K.Post(1, "lrelu", ALPHA, a_dev)
        actp = torch.where(a.double() >= 0, 1.0, ALPHA).double()
    else:
        d = K._desc(c.xshape, R.strides_of(c.xshape, False), c.yshape, dy.stride(), g)
        assert K.L.lib().rgan_conv_post_segments(ctypes.byref(d), 1, 2, nseg, None) > 0
        # |gamma invstd (y - mean) + beta| >= 0.5 * 1 * 0.375 - 0.0625: the sign of the activation's argument is
        # never in doubt
        mean = 0.125 * R.signed_unit((nseg, c.cin), gen)
        invstd = 1.0 + 0.5 * torch.rand((nseg, c.cin), generator=gen)
        gamma, beta = R.signed_unit((c.cin,), gen), 0.0625 * R.signed_unit((c.cin,), gen)
        stats = torch.cat([mean, invstd], 1).to(DEV)
        post = K.Post(2, "lrelu", ALPHA, a_dev, stats=stats, gamma=gamma.to(DEV), beta=beta.to(DEV), nseg=nseg)
        seg = torch.arange(c.B) * nseg // c.B                       # sample -> batch segment
        mean_e = mean.double()[seg].view(c.B, c.cin, 1, 1)
        al = (gamma.double() * invstd.double())[seg].view(c.B, c.cin, 1, 1)
        arg = al * (a.double() - mean_e) + beta.double().view(1, -1, 1, 1)
        assert arg.abs().min() > 0.1
        actp = torch.where(arg >= 0, 1.0, ALPHA).double()
    out, outp = R.view(c.xshape, "nhwc", DEV)
    K.conv_dgrad(dy, w, g, c.xshape, out=out, post=post)
    _sync()
    assert post.fused
    R.assert_untouched(dyp, dy)
    gref = v * actp
    r = R.ratio(out, gref, bnd * actp)
    if mode == 2:
        S, ph = post.S, post.phases
        assert ph == (1 if c.tr else 4) and S % (ph * nseg) == 0 and tuple(post.part.shape) == (S, 2, c.cin)
        part = post.part.cpu().view(ph, nseg, S // ph // nseg, 2, c.cin).sum((0, 2))   # [nseg][2][C]
        A = bnd / R.bound_of(c.K("dgrad"), 1.0) * actp
        b1 = _sum_bound(c, "dgrad", A)
        dev = (a.double() - mean_e)
        Bs = c.B // nseg
        for k in range(nseg):
            sl = slice(k * Bs, (k + 1) * Bs)
            r = max(r, R.ratio(part[k, 0], _rows(gref[sl]).sum(0), _rows(b1[sl]).sum(0)),
                    R.ratio(part[k, 1], _rows((gref * dev)[sl]).sum(0), _rows((b1 * dev.abs())[sl]).sum(0)))
    _note("e_fused_stats", f"post{mode}_{'convt' if c.tr else 'conv'}_dgrad", r, seconds=time.perf_counter() - t0)
    print(f"post mode {mode} nseg {nseg} {c.name} dy={dykind}: err/bound {r:.4f}")
    assert r <= 1.0, r
