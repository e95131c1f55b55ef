"""Tensor-level wrappers over the C-ABI (no autograd here; see autograd.py).

Every function takes CUDA (HIP) tensors, allocates outputs with torch's caching
allocator and launches on the current stream.  Internal activations are NHWC
(torch channels_last strides on a [B, C, H, W] tensor); NCHW tensors are accepted
wherever the reference hands them over (images into D, out of G).
"""
import ctypes
import weakref
from dataclasses import dataclass

import torch

from . import _lib as L


@dataclass(frozen=True)
class ConvGeom:
    """One conv layer as the reference declares it (k, stride, pad, transposed)."""
    k: int
    stride: int
    pad: int
    transposed: bool
    upsample: int = 1  # 2: nearest Upsample(x2) in front of the conv (--NN_conv, GLI:351-356)

    def out_hw(self, h, w):
        h, w = h * self.upsample, w * self.upsample
        if self.transposed:
            return ((h - 1) * self.stride - 2 * self.pad + self.k, (w - 1) * self.stride - 2 * self.pad + self.k)
        return ((h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1)

    def in_hw(self, ho, wo):
        if self.transposed:
            h, w = (ho + 2 * self.pad - self.k) // self.stride + 1, (wo + 2 * self.pad - self.k) // self.stride + 1
        else:
            h, w = (ho - 1) * self.stride - 2 * self.pad + self.k, (wo - 1) * self.stride - 2 * self.pad + self.k
        return h // self.upsample, w // self.upsample


# Upsample(x2)+Conv2d(k3,s1,p1) runs as this transposed conv on the folded weight
# (csrc/upsample.hip; include/rgan.h rgan_nn_fold_weight).
NN_T = ConvGeom(4, 2, 1, True)


# activations with a nonzero second derivative (the WGAN-GP double backward needs act'')
ACT_HAS_GRAD2 = {"none": False, "relu": False, "lrelu": False, "tanh": True, "sigmoid": True, "selu": True}


def _nn_check(geom):
    if geom.upsample != 2 or geom.transposed or (geom.k, geom.stride, geom.pad) != (3, 1, 1):
        raise L.RganError(f"unsupported upsampling conv {geom}: only Upsample(x2)+Conv2d(k3,s1,p1) (--NN_conv)")


def empty_nhwc(B, C, H, W, device):
    return torch.empty_strided((B, C, H, W), (H * W * C, 1, W * C, C), dtype=torch.float32, device=device)


def is_nhwc(t):
    B, C, H, W = t.shape
    return t.stride() == (H * W * C, 1, W * C, C) or (H == 1 and W == 1 and t.stride()[1] == 1)


def as_nhwc(t):
    return t if is_nhwc(t) else t.contiguous(memory_format=torch.channels_last)


def affine_grad_bufs(y, gamma, beta, need_gamma, need_beta):
    """(dgamma, dbeta) buffers of BatchNorm over y's channels; None where not asked for."""
    C = y.shape[1]
    dgamma = torch.empty(C, dtype=torch.float32, device=y.device) if need_gamma and gamma is not None else None
    dbeta = torch.empty(C, dtype=torch.float32, device=y.device) if need_beta and beta is not None else None
    return dgamma, dbeta


def _desc(x_shape, x_stride, y_shape, y_stride, geom):
    d = L.RganConv()
    B, cin, hin, win = x_shape
    _, cout, hout, wout = y_shape
    d.batch, d.cin, d.hin, d.win = B, cin, hin, win
    d.cout, d.hout, d.wout = cout, hout, wout
    d.kh = d.kw = geom.k
    d.stride, d.pad, d.transposed = geom.stride, geom.pad, int(geom.transposed)
    for i in range(4):
        d.xs[i] = x_stride[i]
        d.ys[i] = y_stride[i]
    return d


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise L.RganError(f"expected float32 tensors, got {t.dtype}")


class _Entry:
    """One cached layout of a weight: ``ref`` the weight's base tensor (held weakly: a storage
    address can be reused by a later tensor with the same version count), ``ver`` / ``ptr`` the
    version and address of the weight ``buf`` was made from, and for a pack what makes it again:
    the descriptor ``d``, the layout ``which`` and ``geo``, the packed view's (shape, stride,
    offset) on its base, None for the base itself."""

    __slots__ = ("ref", "ver", "ptr", "buf", "d", "which", "geo")

    def __init__(self, ref, ver, ptr, buf, d=None, which=None, geo=None):
        self.ref, self.ver, self.ptr, self.buf, self.d, self.which, self.geo = ref, ver, ptr, buf, d, which, geo

    def matches(self, w):
        return self.ver == w._version and self.ptr == w.data_ptr()

    def current(self, base, w):
        """``buf`` holds the present values of ``w``, a view of (or) ``base``."""
        return self.ref() is base and self.matches(w)

    def mark(self, w):
        """``buf`` was rewritten from ``w``'s present values."""
        self.ver, self.ptr = w._version, w.data_ptr()


class _WeightCache:
    """{key: _Entry}; an entry goes when its weight's base is collected."""

    def __init__(self):
        self.entries = {}

    def _put(self, key, base, w, buf, d=None, which=None, geo=None):
        self.entries[key] = _Entry(weakref.ref(base, self._drop(key)), w._version, w.data_ptr(), buf, d, which, geo)

    def _drop(self, key):
        def cb(_ref):
            ent = self.entries.get(key)
            if ent is not None and ent.ref is _ref:
                del self.entries[key]
        return cb

    def clear(self):
        self.entries.clear()


class _PackCache(_WeightCache):
    """GEMM-ready weight layouts, cached per (weight tensor, layout, version).

    Weights change only at optimizer steps (fused Adam bumps the autograd version
    counter), while every net runs 2-4 times per iteration, so most conv launches reuse
    a packed copy.  Entries are keyed by the weight's base tensor object and
    one buffer per (weight, layout) is refilled in place when the version moves."""

    def get(self, w, which, geom, d):
        base = w._base if w._base is not None else w
        key = (id(base), which, geom, d.cin, d.cout, d.hin, d.win, d.hout, d.wout)
        ent = self.entries.get(key)
        if ent is not None and ent.current(base, w):
            return ent.buf
        lib = L.lib()
        n = lib.rgan_conv_pack_floats(ctypes.byref(d), which)
        if n == 0:
            return None  # the op reads the torch layout directly (or is unsupported: workspace says)
        reuse = ent is not None and ent.ref() is base and ent.buf.numel() == n
        buf = ent.buf if reuse else torch.empty(n, dtype=torch.float32, device=w.device)
        L.check(lib.rgan_conv_pack(ctypes.byref(d), which, L.ptr(w), L.ptr(buf), L.stream()), "rgan_conv_pack")
        # (the descriptor, layout and w's view geometry on its base let refresh() and the
        # optimizer's layout writer find the weight again: a view such as arch 1's dense layers
        # viewed as convolutions is a new tensor object at every call, so a weak reference to it
        # would die with the call and its layout would be repacked at every use)
        geo = None if w is base else (tuple(w.shape), tuple(w.stride()), w.storage_offset())
        self._put(key, base, w, buf, d, which, geo)
        return buf

    @staticmethod
    def _weight(ent):
        """The packed weight of an entry (its base parameter, or the view of it that was packed),
        or None when the entry is stale: the base is gone, or its storage no longer covers the
        saved view (e.g. ``p.data = smaller``) -- such an entry is never a valid layout source."""
        base = ent.ref()
        if base is None or ent.geo is None:
            return base
        shape, stride, offset = ent.geo
        extent = offset + 1 + sum((n - 1) * st for n, st in zip(shape, stride))  # elements, all n >= 1
        if any(n == 0 for n in shape) or base.untyped_storage().nbytes() < extent * base.element_size():
            return None
        return base.as_strided(shape, stride, offset)

    def _snapshot(self):
        """list(entries.items()).  Building the list allocates, an allocation can start a garbage
        collection, and a collected weight's weak-reference callback (_drop) deletes its entry:
        the dict then changes size under the iteration.  Taken again when that happens."""
        while True:
            try:
                return list(self.entries.items())
            except RuntimeError:
                continue

    def _live(self, params):
        """[(param index, key, entry, packed weight)] of the entries whose base is one of
        ``params``.  On the way, every entry whose weight view can no longer be rebuilt (see
        _weight) is dropped."""
        idx = {id(p): i for i, p in enumerate(params)}
        out = []
        for key, ent in self._snapshot():
            base, w = ent.ref(), self._weight(ent)
            if base is not None and w is None:
                if self.entries.get(key) is ent:
                    del self.entries[key]
            elif base is not None and id(base) in idx:
                out.append((idx[id(base)], key, ent, w))
        return out

    def refresh(self, params):
        """Repack, in one batched launch, every cached layout of ``params`` whose weight
        moved (called right after an optimizer step): the next convolutions find them
        current instead of packing one launch at a time."""
        todo = [(ent, w) for _, _, ent, w in self._live(params) if not ent.matches(w)]
        if not todo:
            return
        n = len(todo)
        descs = (ctypes.POINTER(L.RganConv) * n)(*[ctypes.pointer(e.d) for e, _ in todo])
        which = (ctypes.c_int * n)(*[e.which for e, _ in todo])
        ws = (ctypes.c_void_p * n)(*[w.data_ptr() for _, w in todo])
        outs = (ctypes.c_void_p * n)(*[e.buf.data_ptr() for e, _ in todo])
        L.check(L.lib().rgan_conv_pack_batch(n, ctypes.cast(descs, ctypes.c_void_p), ctypes.cast(which, ctypes.c_void_p),
                                             ctypes.cast(ws, ctypes.c_void_p), ctypes.cast(outs, ctypes.c_void_p),
                                             L.stream()), "rgan_conv_pack_batch")
        for ent, w in todo:
            ent.mark(w)

    def layouts_of(self, params):
        """[(param index, key, entry)] of every cached layout of ``params`` (for
        rgan_adam_packed, which rewrites them with the new values)."""
        return [(i, key, ent) for i, key, ent, w in self._live(params)
                if w.data_ptr() == params[i].data_ptr() and w.numel() == params[i].numel()]

    def mark_current(self, layouts):
        """The listed layouts were rewritten from their weights' current values."""
        for _, key, ent in layouts:
            w = self._weight(ent)
            if w is not None and self.entries.get(key) is ent:
                ent.mark(w)


PACKS = _PackCache()


class _FoldCache(_WeightCache):
    """Folded --NN_conv weights (Wt = A W A^T), one per (weight, version): like the packs,
    refolded only after an optimizer step.  A new Wt tensor is made per version so the
    pack cache (keyed by the Wt object) never sees a stale layout.  ``fn`` is the fold
    (nn_fold here; the image-layer patch weights use their own instance)."""

    def __init__(self, fn=None):
        super().__init__()
        self.fn = fn

    def get(self, w, *args):
        base = w._base if w._base is not None else w
        key = (id(base),) + args
        ent = self.entries.get(key)
        if ent is not None and ent.current(base, w):
            return ent.buf
        wt = (self.fn or nn_fold)(w, *args)
        self._put(key, base, w, wt)
        return wt


FOLDS = _FoldCache()


# ------------------------------------------------------------------ image layers as 1x1 GEMMs
G1X1 = ConvGeom(1, 1, 0, False)


def patchable(geom, cin_img):
    """k4 s2 p1 layer whose image side has <= 4 channels (D's first conv, G's last convT)."""
    return (geom.k, geom.stride, geom.pad, geom.upsample) == (4, 2, 1, 1) and cin_img <= 4


def patches_k4s2(img):
    """Patch matrix of an image [B][C][H][W] (any strides, C <= 4) on the half-size grid,
    as an NHWC [B, 64, H/2, W/2] tensor (rgan_patches_k4s2)."""
    L.require_cuda(img)
    _f32(img)
    B, C, H, W = img.shape
    X = empty_nhwc(B, 64, H // 2, W // 2, img.device)
    st = (L.c_ll * 4)(*img.stride())
    L.check(L.lib().rgan_patches_k4s2(L.ptr(img), B, C, H, W, st, L.ptr(X), L.stream()), "rgan_patches_k4s2")
    return X


def patch_weight(w, transposed):
    """Image-layer weight -> the 1x1 GEMM weight [O][64][1][1], W1[o][4t+c] = W[o][c][t]:
    Conv2d [co][ci][4][4] (o = co, c = ci) or ConvTranspose2d [ci][co][4][4] (o = ci, c = co)."""
    wc = w.contiguous()
    O, C = wc.shape[0], wc.shape[1]
    w1 = torch.empty((O, 64, 1, 1), dtype=torch.float32, device=w.device)
    L.check(L.lib().rgan_patch_weight(L.ptr(wc), O, C, C * 16, 16, L.ptr(w1), L.stream()), "rgan_patch_weight")
    return w1


PATCHW = _FoldCache(patch_weight)


def unpatch_grad(g1, O, C, row_stride, col_stride, out=None, into=None):
    """1x1-GEMM weight gradient -> torch layout [O][C][4][4] (dw[o][c][t] = g1[o*rs + (4t+c)*cs]);
    ``out`` given: added into it (gradient accumulation); ``into``: written into it."""
    acc = out is not None
    if into is not None and (acc or tuple(into.shape) != (O, C, 4, 4) or not into.is_contiguous()):
        raise L.RganError("unpatch_grad: `into` must be a contiguous [O][C][4][4] tensor (no accumulation)")
    dw = out if acc else (into if into is not None else torch.empty((O, C, 4, 4), dtype=torch.float32,
                                                                    device=g1.device))
    L.check(L.lib().rgan_unpatch_grad(L.ptr(g1), O, C, row_stride, col_stride, L.ptr(dw), int(acc), L.stream()),
            "rgan_unpatch_grad")
    return dw


def nn_fold(w):
    """Conv2d weight [cout][cin][3][3] -> ConvTranspose2d weight [cin][cout][4][4]."""
    L.require_cuda(w)
    _f32(w)
    cout, cin = w.shape[0], w.shape[1]
    if tuple(w.shape[2:]) != (3, 3):
        raise L.RganError(f"nn_fold expects a 3x3 kernel, got {tuple(w.shape)}")
    wt = torch.empty((cin, cout, 4, 4), dtype=torch.float32, device=w.device)
    L.check(L.lib().rgan_nn_fold_weight(L.ptr(w.contiguous()), cout, cin, L.ptr(wt), L.stream()),
            "rgan_nn_fold_weight")
    return wt


def nn_unfold_grad(dwt, w_shape):
    """Adjoint of nn_fold: dWt [cin][cout][4][4] -> dW [cout][cin][3][3]."""
    cout, cin = w_shape[0], w_shape[1]
    dw = torch.empty(w_shape, dtype=torch.float32, device=dwt.device)
    L.check(L.lib().rgan_nn_unfold_grad(L.ptr(dwt.contiguous()), cout, cin, L.ptr(dw), L.stream()),
            "rgan_nn_unfold_grad")
    return dw


_UNSUPPORTED = ("unsupported conv {} for input {}", "unsupported conv dgrad {} for {}",
                "unsupported conv wgrad {} for {}")  # per op 0 / 1 / 2 (rgan_conv_workspace's `which`)


def _conv_prologue(d, which, w, geom, cache, x_shape, device):
    """(cached pack of ``w`` or None, workspace) of op ``which`` on the descriptor ``d``; an op
    the library has no kernel for answers 0 bytes and raises."""
    packed = PACKS.get(w, which, geom, d) if cache else None
    nbytes = L.lib().rgan_conv_workspace(ctypes.byref(d), which, int(packed is not None))
    if nbytes == 0:
        raise L.RganError(_UNSUPPORTED[which].format(geom, tuple(x_shape)))
    return packed, L.workspace(nbytes, device)


def conv_fwd(x, w, geom, bias=None, act="none", alpha=0.0, wscale=None, out=None, nchw_out=False, cache=False,
             post=None):
    """y = act(conv(x, w)*wscale + bias); x [B,Cin,H,W] any strides; w torch layout.

    ``cache=True`` (module parameters only) reuses a packed weight while its version is
    unchanged.  ``post`` (no bias / act): a Post for the producer of ... (see conv_dgrad) --
    used when this conv computes a gradient (G's image-layer data gradient as a 1x1 GEMM)."""
    L.require_cuda(x, w, bias, wscale)
    _f32(x, w, bias)
    if geom.upsample != 1:
        _nn_check(geom)
        wt = FOLDS.get(w) if cache else nn_fold(w)
        return conv_fwd(x, wt, NN_T, bias=bias, act=act, alpha=alpha, wscale=wscale, out=out, nchw_out=nchw_out,
                        cache=cache, post=post)
    B, cin, H, W = x.shape
    cout = w.shape[1] if geom.transposed else w.shape[0]
    Ho, Wo = geom.out_hw(H, W)
    if out is None:
        out = (torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device) if nchw_out
               else empty_nhwc(B, cout, Ho, Wo, x.device))
    d = _desc(x.shape, x.stride(), out.shape, out.stride(), geom)
    packed, ws = _conv_prologue(d, 0, w, geom, cache, x.shape, x.device)
    if post is not None:
        post.fused = False
        if bias is None and act == "none" and _conv_post(0, d, x, w, packed, wscale, out, ws, post) is not False:
            return out
    L.check(L.lib().rgan_conv_fwd(ctypes.byref(d), L.ptr(x), L.ptr(w), L.ptr(packed), L.ptr(wscale), L.ptr(bias),
                                  L.ptr(out), L.ACT[act], float(alpha), L.ptr(ws), ws.numel(), L.stream()),
            "rgan_conv_fwd")
    return out


def conv_fwd_bn(x, w, geom, bias=None, wscale=None, cache=False, segs=1):
    """y = conv(x, w)*wscale + bias (NHWC) for a layer followed by train-mode BatchNorm.

    Returns (y, part, S): when the GEMM's vector epilogue or its split-K reduce covered the
    layer, ``part`` is
    its per-64-row segment sums (sum y, sum y^2) double[S][2][C] (merge with bn_segment_stats; batch
    segment k = segments [k*S/segs, (k+1)*S/segs)); otherwise (y, None, 0)."""
    if geom.upsample != 1:
        return conv_fwd(x, w, geom, bias=bias, wscale=wscale, cache=cache), None, 0
    L.require_cuda(x, w, bias, wscale)
    _f32(x, w, bias)
    B, cin, H, W = x.shape
    cout = w.shape[1] if geom.transposed else w.shape[0]
    Ho, Wo = geom.out_hw(H, W)
    out = empty_nhwc(B, cout, Ho, Wo, x.device)
    d = _desc(x.shape, x.stride(), out.shape, out.stride(), geom)
    lib = L.lib()
    S = lib.rgan_conv_bn_segments(ctypes.byref(d), int(segs))
    if S <= 0:
        return conv_fwd(x, w, geom, bias=bias, wscale=wscale, out=out, cache=cache), None, 0
    packed, ws = _conv_prologue(d, 0, w, geom, cache, x.shape, x.device)
    part = torch.empty((S, 2, cout), dtype=torch.float64, device=x.device)
    fused = L.c_int(0)
    L.check(lib.rgan_conv_fwd_bn(ctypes.byref(d), L.ptr(x), L.ptr(w), L.ptr(packed), L.ptr(wscale), L.ptr(bias),
                                 L.ptr(out), L.ptr(ws), ws.numel(), L.ptr(part), S, int(segs), ctypes.byref(fused),
                                 L.stream()), "rgan_conv_fwd_bn")
    return (out, part, S) if fused.value else (out, None, 0)


def bn_segment_stats(part, s0, s1, C, eps, momentum, running_mean=None, running_var=None,
                     num_batches_tracked=None, out=None):
    """Segment moments [s0, s1) of conv_fwd_bn -> (mean, invstd) float[2C] + running stats."""
    stats = torch.empty(2 * C, dtype=torch.float32, device=part.device) if out is None else out
    L.check(L.lib().rgan_bn_segment_stats(L.ptr(part), int(s0), int(s1), C, 64, float(eps), float(momentum),
                                          L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked),
                                          L.ptr(stats), None, L.stream()), "rgan_bn_segment_stats")
    return stats


def bn_segment_moments(part, s0, s1, C):
    """Segment moments [s0, s1) -> this rank's (count, mean, M2) double[3C] (SyncBN stage 1)."""
    mom = torch.empty(3 * C, dtype=torch.float64, device=part.device)
    L.check(L.lib().rgan_bn_segment_stats(L.ptr(part), int(s0), int(s1), C, 64, 0.0, 0.0, None, None, None, None,
                                          L.ptr(mom), L.stream()), "rgan_bn_segment_stats")
    return mom


class Post:
    """Producer post-op of rgan_conv_post (include/rgan.h RganPost): the backward pass of the
    layer that produced this GEMM's output operand, applied in the GEMM's epilogue / split-K
    reduce.  mode 1: out *= act'(x) (x = its activation output); mode 2: out = g = out *
    act'(BN(x)) and the BatchNorm backward sums per 64-row segment (x = its BN input y; finish
    with bn_backward_parts).  After the call ``fused`` says whether the GEMM applied it
    (else the output is the plain gradient) and, for mode 2, ``part`` / ``S`` / ``phases``
    hold the sums."""

    __slots__ = ("mode", "act", "alpha", "x", "stats", "gamma", "beta", "nseg", "fused", "part", "S", "phases")

    def __init__(self, mode, act, alpha, x, stats=None, gamma=None, beta=None, nseg=1):
        self.mode, self.act, self.alpha, self.x = mode, act, float(alpha), x
        self.stats, self.gamma, self.beta, self.nseg = stats, gamma, beta, nseg
        self.fused, self.part, self.S, self.phases = False, None, 0, 1


def _conv_post(which, d, inp, w, packed, wscale, out, ws, post):
    """rgan_conv_post for ``post`` (see Post); returns False when the GEMM cannot apply it."""
    if (tuple(post.x.shape) != tuple(out.shape) or post.x.stride() != out.stride()
            or post.x.data_ptr() % 16 or out.data_ptr() % 16):
        return False
    lib = L.lib()
    part, S = None, 0
    if post.mode == 2:
        ph = L.c_int(1)
        S = lib.rgan_conv_post_segments(ctypes.byref(d), which, 2, int(post.nseg), ctypes.byref(ph))
        post.phases = ph.value
        if S <= 0:
            return False
        part = torch.empty((S, 2, out.shape[1]), dtype=torch.float64, device=out.device)
    rp = L.RganPost(int(post.mode), L.ACT[post.act], float(post.alpha), int(post.nseg), post.x.data_ptr(),
                    L.ptr(post.stats), L.ptr(post.gamma), L.ptr(post.beta), L.ptr(part), int(S))
    fused = L.c_int(0)
    L.check(lib.rgan_conv_post(ctypes.byref(d), which, L.ptr(inp), L.ptr(w), L.ptr(packed), L.ptr(wscale),
                               L.ptr(out), L.ptr(ws), ws.numel(), ctypes.byref(rp), ctypes.byref(fused), L.stream()),
            "rgan_conv_post")
    if not fused.value:
        return None  # the plain result was written
    post.fused, post.part, post.S = True, part, S
    return True


def conv_dgrad(dy, w, geom, x_shape, wscale=None, out=None, like=None, cache=False, post=None):
    """dx of the conv (input grad), NHWC unless `like` (a tensor whose strides to copy) is given.
    ``post``: a Post for the layer that produced x (applied when the GEMM can: post.fused)."""
    L.require_cuda(dy, w, wscale)
    _f32(dy, w)
    if geom.upsample != 1:
        _nn_check(geom)
        wt = FOLDS.get(w) if cache else nn_fold(w)
        return conv_dgrad(dy, wt, NN_T, x_shape, wscale=wscale, out=out, like=like, cache=cache, post=post)
    B, cin, H, W = x_shape
    if out is None:
        if like is not None and not is_nhwc(like):
            out = torch.empty(x_shape, dtype=torch.float32, device=dy.device)
        else:
            out = empty_nhwc(B, cin, H, W, dy.device)
    d = _desc(out.shape, out.stride(), dy.shape, dy.stride(), geom)
    packed, ws = _conv_prologue(d, 1, w, geom, cache, x_shape, dy.device)
    if post is not None:
        post.fused = False
        if _conv_post(1, d, dy, w, packed, wscale, out, ws, post) is not False:
            return out
    L.check(L.lib().rgan_conv_dgrad(ctypes.byref(d), L.ptr(dy), L.ptr(w), L.ptr(packed), L.ptr(wscale), L.ptr(out),
                                    L.ptr(ws), ws.numel(), L.stream()), "rgan_conv_dgrad")
    return out


def g1_ok(x, w, geom):
    """G's first layer on its 1x1 input can run as rgan_g1_fwd_bn / rgan_g1_wgrad."""
    return (geom.transposed and geom.k == 4 and geom.stride == 1 and geom.pad == 0 and geom.upsample == 1
            and x.dim() == 4 and tuple(x.shape[2:]) == (1, 1) and x.shape[0] in (32, 64) and x.shape[1] in (64, 128)
            and w.shape[1] % 16 == 0 and w.is_contiguous() and x.is_contiguous() and x.data_ptr() % 16 == 0)


def g1_fwd_bn(x, w, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, act, alpha,
              out=None):
    """(y, a, stats) of G's first layer + BatchNorm + act in one launch (rgan_g1_fwd_bn)."""
    L.require_cuda(x, w)
    B, cin = x.shape[0], x.shape[1]
    cout = w.shape[1]
    y = empty_nhwc(B, cout, 4, 4, x.device)
    a = empty_nhwc(B, cout, 4, 4, x.device) if out is None else out
    if not is_nhwc(a):
        raise L.RganError("g1_fwd_bn: out must be NHWC")
    stats = torch.empty(2 * cout, dtype=torch.float32, device=x.device)
    L.check(L.lib().rgan_g1_fwd_bn(L.ptr(x), B, cin, L.ptr(w), cout, L.ptr(gamma), L.ptr(beta), float(eps),
                                   float(momentum), L.ptr(running_mean), L.ptr(running_var),
                                   L.ptr(num_batches_tracked), L.ACT[act], float(alpha), L.ptr(y), L.ptr(a),
                                   L.ptr(stats), L.stream()), "rgan_g1_fwd_bn")
    return y, a, stats


def g1_wgrad(x, dy, w_shape, out=None, into=None):
    """dW of G's first layer (rgan_g1_wgrad); ``out``: add into it, ``into``: write into it."""
    L.require_cuda(x, dy)
    dy = as_nhwc(dy)
    dw = out if out is not None else (into if into is not None else
                                      torch.empty(w_shape, dtype=torch.float32, device=x.device))
    L.check(L.lib().rgan_g1_wgrad(L.ptr(x), x.shape[0], x.shape[1], L.ptr(dy), w_shape[1], L.ptr(dw),
                                  int(out is not None), L.stream()), "rgan_g1_wgrad")
    return dw


def conv_wgrad(x, dy, geom, w_shape, with_bias=False, out=None, out_bias=None, into=None, bias_row0=0):
    """(dw in torch layout, dbias or None).  ``out`` / ``out_bias`` given: the gradients are
    ADDED into them in the GEMM epilogue (autograd accumulation without an add pass);
    ``into``: dw is WRITTEN into that tensor (e.g. its slice of a data-parallel gradient
    bucket, dp.grad_view) instead of a new one.  ``bias_row0``: dbias sums dy's pixel rows
    (b, h, w) from that one on (rgan_conv_wgrad_rows: the GP engine's [adjoint; forward] pairs)."""
    L.require_cuda(x, dy)
    _f32(x, dy)
    if into is not None:
        if out is not None or geom.upsample != 1:
            raise L.RganError("conv_wgrad: `into` excludes accumulation and NN_conv")
        if tuple(into.shape) != tuple(w_shape) or not into.is_contiguous():
            raise L.RganError("conv_wgrad: `into` must be a contiguous tensor of the weight's shape")
    if geom.upsample != 1:
        _nn_check(geom)
        if out is not None:
            raise L.RganError("accumulating NN_conv weight gradients is not supported")
        cout, cin = w_shape[0], w_shape[1]
        dwt, db = conv_wgrad(x, dy, NN_T, (cin, cout, 4, 4), with_bias=with_bias, bias_row0=bias_row0)
        return nn_unfold_grad(dwt, tuple(w_shape)), db
    acc = out is not None
    if acc and (tuple(out.shape) != tuple(w_shape) or not out.is_contiguous()):
        raise L.RganError("conv_wgrad: out must be a contiguous tensor of the weight's shape")
    dw = out if acc else (into if into is not None else torch.empty(w_shape, dtype=torch.float32, device=x.device))
    db = None
    if with_bias:
        if acc != (out_bias is not None):
            raise L.RganError("conv_wgrad: accumulate weight and bias gradients together")
        db = out_bias if acc else torch.empty(dy.shape[1], dtype=torch.float32, device=x.device)
        dy = as_nhwc(dy)
    d = _desc(x.shape, x.stride(), dy.shape, dy.stride(), geom)
    _, ws = _conv_prologue(d, 2, None, geom, False, x.shape, x.device)
    L.check(L.lib().rgan_conv_wgrad_rows(ctypes.byref(d), L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), int(bias_row0),
                                         int(acc), L.ptr(ws), ws.numel(), L.stream()), "rgan_conv_wgrad_rows")
    return dw, db


# ------------------------------------------------------------------ BatchNorm
def _pc(t):
    """[P][C] view parameters of an NHWC tensor."""
    B, C, H, W = t.shape
    if not is_nhwc(t):
        raise L.RganError("BatchNorm kernels expect NHWC (channels_last) activations")
    return B * H * W, C, C, 1


def bn_stats(y, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None, out=None):
    """Batch (mean, invstd) as float[2C]; updates running buffers when given."""
    P, C, sp, sc = _pc(y)
    lib = L.lib()
    stats = torch.empty(2 * C, dtype=torch.float32, device=y.device) if out is None else out
    part = L.workspace(lib.rgan_bn_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_stats(L.ptr(y), P, C, sp, sc, float(eps), float(momentum), L.ptr(running_mean),
                              L.ptr(running_var), L.ptr(num_batches_tracked), L.ptr(stats), L.ptr(part),
                              L.stream()), "rgan_bn_stats")
    return stats


def bn_moments(y):
    """This rank's per-channel (count, mean, M2) as double[3C] (SyncBN stage 1)."""
    P, C, sp, sc = _pc(y)
    lib = L.lib()
    mom = torch.empty(3 * C, dtype=torch.float64, device=y.device)
    part = L.workspace(lib.rgan_bn_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_moments(L.ptr(y), P, C, sp, sc, L.ptr(mom), L.ptr(part), L.stream()), "rgan_bn_moments")
    return mom


def bn_finalize(moments, nranks, C, eps, momentum, running_mean=None, running_var=None,
                num_batches_tracked=None, out=None):
    """Merge [nranks][3][C] moments in rank order -> stats float[2C] (SyncBN stage 2)."""
    stats = torch.empty(2 * C, dtype=torch.float32, device=moments.device) if out is None else out
    L.check(L.lib().rgan_bn_finalize(L.ptr(moments), int(nranks), C, float(eps), float(momentum),
                                     L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked),
                                     L.ptr(stats), L.stream()), "rgan_bn_finalize")
    return stats


def bn_backward_sums(da, y, stats, gamma, beta, act="none", alpha=0.0):
    da = as_nhwc(da)
    P, C, sp, sc = _pc(y)
    _, _, dsp, dsc = _pc(da)
    sums = torch.empty(2 * C, dtype=torch.float64, device=y.device)
    lib = L.lib()
    part = L.workspace(lib.rgan_bn_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_backward_sums(L.ptr(da), dsp, dsc, L.ptr(y), P, C, sp, sc, L.ptr(stats), L.ptr(gamma),
                                      L.ptr(beta), L.ACT[act], float(alpha), L.ptr(sums), L.ptr(part),
                                      L.stream()), "rgan_bn_backward_sums")
    return sums, da


def bn_backward_apply(da, y, stats, gamma, beta, act, alpha, sums, P_global, need_affine=True, out=None):
    P, C, sp, sc = _pc(y)
    _, _, dsp, dsc = _pc(da)
    dy = torch.empty_like(y) if out is None else out
    if dy.stride() != y.stride():
        raise L.RganError("bn_backward_apply: out must have y's strides")
    dgamma, dbeta = affine_grad_bufs(y, gamma, beta, need_affine, need_affine)
    L.check(L.lib().rgan_bn_backward_apply(L.ptr(da), dsp, dsc, L.ptr(y), P, C, sp, sc, L.ptr(stats),
                                           L.ptr(gamma), L.ptr(beta), L.ACT[act], float(alpha), L.ptr(sums),
                                           int(P_global), L.ptr(dy), sp, sc, L.ptr(dgamma), L.ptr(dbeta),
                                           L.stream()), "rgan_bn_backward_apply")
    return dy, dgamma, dbeta


def bn_backward_sums_apply(da, y, stats, gamma, beta, act, alpha, add=None, out=None, dgamma=None, dbeta=None,
                           accumulate_affine=False):
    """(sums double[2C], dy) of act(BN(y))'s backward in one call (rgan_bn_backward_sums_apply:
    one launch for <= 2048 rows, C % 16 == 0 and C >= 1024): sums as bn_backward_sums returns
    them, dy = BN-backward(da * act') + add; dgamma / dbeta (given buffers) written or, with
    accumulate_affine, added into.  Dense NHWC da / y / out / add; add may be out itself."""
    da = as_nhwc(da)
    P, C, _, _ = _pc(y)
    dy = torch.empty_like(y) if out is None else out
    if not is_nhwc(dy) or (add is not None and not is_nhwc(add)):
        raise L.RganError("bn_backward_sums_apply: out / add must be NHWC")
    sums = torch.empty(2 * C, dtype=torch.float64, device=y.device)
    lib = L.lib()
    part = L.workspace(lib.rgan_bn_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_backward_sums_apply(L.ptr(da), L.ptr(y), P, C, L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                            L.ACT[act], float(alpha), L.ptr(add), L.ptr(dy), L.ptr(dgamma),
                                            L.ptr(dbeta), int(bool(accumulate_affine)), L.ptr(sums), L.ptr(part),
                                            L.stream()), "rgan_bn_backward_sums_apply")
    return sums, dy


def bn_affine_grads(sums, stats, C, dgamma=None, dbeta=None, accumulate=False):
    """dgamma / dbeta (given buffers) from BatchNorm backward sums [2][C] (rgan_bn_affine_grads):
    written, or added into with ``accumulate``."""
    L.check(L.lib().rgan_bn_affine_grads(L.ptr(sums), L.ptr(stats), int(C), L.ptr(dgamma), L.ptr(dbeta),
                                         int(bool(accumulate)), L.stream()), "rgan_bn_affine_grads")


def bn_segment_stats_n(part, S, nseg, C, eps, momentum, running_mean, running_var, num_batches_tracked, out):
    """bn_segment_stats of the nseg equal batch segments of [0, S) in one launch: out[nseg][2C],
    running statistics updated in segment order."""
    L.check(L.lib().rgan_bn_segment_stats_n(L.ptr(part), 0, int(S), int(nseg), C, 64, float(eps), float(momentum),
                                            L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked),
                                            L.ptr(out), L.stream()), "rgan_bn_segment_stats_n")
    return out


def bn_segment_apply(part, S, y, eps, momentum, running_mean, running_var, num_batches_tracked, gamma, beta, act,
                     alpha, stats, out):
    """bn_segment_stats_n + bn_apply_segments in one call (rgan_bn_segment_apply): nseg =
    stats.shape[0] equal batch segments of y (dense NHWC, 16-byte aligned) and of conv_fwd_bn's
    S segment sums; one launch for small layers."""
    P, C, _, _ = _pc(y)
    L.check(L.lib().rgan_bn_segment_apply(L.ptr(part), int(S), int(stats.shape[0]), 64, L.ptr(y), P, C, float(eps),
                                          float(momentum), L.ptr(running_mean), L.ptr(running_var),
                                          L.ptr(num_batches_tracked), L.ptr(gamma), L.ptr(beta), L.ACT[act],
                                          float(alpha), L.ptr(stats), L.ptr(out), L.stream()),
            "rgan_bn_segment_apply")
    return out


def bn_apply_segments(y, stats, gamma, beta, act, alpha, out):
    """bn_apply of y's nseg = stats.shape[0] equal batch segments, each with its stats row,
    in one launch (dense NHWC y and out)."""
    P, C, _, _ = _pc(y)
    L.check(L.lib().rgan_bn_apply_segments(L.ptr(y), P, C, stats.shape[0], L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                           L.ACT[act], float(alpha), L.ptr(out), L.stream()),
            "rgan_bn_apply_segments")
    return out


def bn_backward_segments(da, y, stats, gamma, beta, act, alpha, need_gamma, need_beta, out):
    """bn_backward of y's nseg = stats.shape[0] equal batch segments in one set of launches
    (dense NHWC da, y, out); dgamma / dbeta summed over the segments."""
    P, C, _, _ = _pc(y)
    nseg = stats.shape[0]
    dgamma, dbeta = affine_grad_bufs(y, gamma, beta, need_gamma, need_beta)
    lib = L.lib()
    ws = L.workspace(nseg * lib.rgan_bn_partial_bytes(P // nseg, C), y.device)
    L.check(lib.rgan_bn_backward_segments(L.ptr(da), L.ptr(y), P, C, nseg, L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                          L.ACT[act], float(alpha), L.ptr(out), L.ptr(dgamma), L.ptr(dbeta),
                                          L.ptr(ws), L.stream()), "rgan_bn_backward_segments")
    return out, dgamma, dbeta


def bn_backward_parts(g, y, stats, gamma, beta, post, need_gamma, need_beta, out=None):
    """dy (and dgamma / dbeta summed over the batch segments) from g = da * act' and the
    segment sums a GEMM's post-op wrote (Post mode 2, post.fused): merge + apply."""
    P, C, _, _ = _pc(y)
    nseg = post.nseg
    if stats.dim() == 1:
        stats = stats.view(1, -1)
    dy = torch.empty_like(y) if out is None else out
    dgamma, dbeta = affine_grad_bufs(y, gamma, beta, need_gamma, need_beta)
    sums = torch.empty((nseg, 2, C), dtype=torch.float64, device=y.device)
    L.check(L.lib().rgan_bn_backward_parts(L.ptr(g), L.ptr(y), P, C, nseg, L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                           L.ptr(post.part), int(post.S), int(post.phases), L.ptr(dy),
                                           L.ptr(dgamma), L.ptr(dbeta), L.ptr(sums), L.stream()),
            "rgan_bn_backward_parts")
    return dy, dgamma, dbeta


def bn_apply(y, stats, gamma, beta, act="none", alpha=0.0, out=None):
    P, C, sp, sc = _pc(y)
    if out is None:
        out = torch.empty_like(y)
    Pa, Ca, asp, asc = _pc(out)
    L.check(L.lib().rgan_bn_apply(L.ptr(y), P, C, sp, sc, L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ACT[act],
                                  float(alpha), L.ptr(out), asp, asc, L.stream()), "rgan_bn_apply")
    return out


def bn_backward(da, y, stats, gamma, beta, act="none", alpha=0.0, need_affine=True, out=None):
    da = as_nhwc(da)
    P, C, sp, sc = _pc(y)
    _, _, dsp, dsc = _pc(da)
    dy = torch.empty_like(y) if out is None else out
    if dy.stride() != y.stride():
        raise L.RganError("bn_backward: out must have y's strides")
    dgamma, dbeta = affine_grad_bufs(y, gamma, beta, need_affine, need_affine)
    lib = L.lib()
    part = L.workspace(lib.rgan_bn_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_backward(L.ptr(da), dsp, dsc, L.ptr(y), P, C, sp, sc, L.ptr(stats), L.ptr(gamma),
                                 L.ptr(beta), L.ACT[act], float(alpha), L.ptr(dy), sp, sc, L.ptr(dgamma),
                                 L.ptr(dbeta), L.ptr(part), L.stream()), "rgan_bn_backward")
    return dy, dgamma, dbeta


def bn_backward_apply_ex(da, y, stats, gamma, beta, act, alpha, sums, P_global, add=None, out=None,
                         dgamma=None, dbeta=None, accumulate_affine=False):
    """dy = BN-backward(da * act') + add; dgamma/dbeta (given buffers) written or, with
    accumulate_affine, added into."""
    da = as_nhwc(da)
    P, C, sp, sc = _pc(y)
    _, _, dsp, dsc = _pc(da)
    dy = torch.empty_like(y) if out is None else out
    if dy.stride() != y.stride() or (add is not None and add.stride() != y.stride()):
        raise L.RganError("bn_backward_apply_ex: out / add must have y's strides")
    L.check(L.lib().rgan_bn_backward_apply_ex(L.ptr(da), dsp, dsc, L.ptr(y), P, C, sp, sc, L.ptr(stats),
                                              L.ptr(gamma), L.ptr(beta), L.ACT[act], float(alpha), L.ptr(sums),
                                              int(P_global), L.ptr(add), L.ptr(dy), sp, sc, L.ptr(dgamma),
                                              L.ptr(dbeta), int(bool(accumulate_affine)), L.stream()),
            "rgan_bn_backward_apply_ex")
    return dy


def bn_dd_sums(a, y, dh, stats, gamma, beta, act, alpha, stage, stage1=None, P_global=0):
    """WGAN-GP double backward through BN+act: stage 1 -> double[3C], stage 2 -> double[2C]."""
    P, C, sp, sc = _pc(y)
    for t in (a, dh):
        if t.stride() != y.stride():
            raise L.RganError("bn_dd_sums: a, dh must have y's strides")
    lib = L.lib()
    out = torch.empty((3 if stage == 1 else 2) * C, dtype=torch.float64, device=y.device)
    part = L.workspace(lib.rgan_bn_dd_partial_bytes(P, C), y.device)
    L.check(lib.rgan_bn_dd_sums(L.ptr(a), L.ptr(y), L.ptr(dh), P, C, sp, sc, L.ptr(stats), L.ptr(gamma),
                                L.ptr(beta), L.ACT[act], float(alpha), int(stage), L.ptr(stage1), int(P_global),
                                L.ptr(out), L.ptr(part), L.stream()), "rgan_bn_dd_sums")
    return out


def bn_dd_apply(a, y, dh, stats, gamma, beta, act, alpha, first_sums, s1, s2, P_global, s1_local=None,
                s2_local=None, adj_dh=None, ydir=None, need_adj=True, dgamma2=None, dbeta2=None,
                accumulate_affine=False):
    """-> (adj_dh or None, ydir); dgamma2 / dbeta2 buffers written (or added into)."""
    P, C, sp, sc = _pc(y)
    if adj_dh is None and need_adj:
        adj_dh = torch.empty_like(y)
    if ydir is None:
        ydir = torch.empty_like(y)
    for t in (a, dh, ydir) + ((adj_dh,) if adj_dh is not None else ()):
        if t.stride() != y.stride():
            raise L.RganError("bn_dd_apply: tensors must share y's strides")
    L.check(L.lib().rgan_bn_dd_apply(L.ptr(a), L.ptr(y), L.ptr(dh), P, C, sp, sc, L.ptr(stats), L.ptr(gamma),
                                     L.ptr(beta), L.ACT[act], float(alpha), L.ptr(first_sums), L.ptr(s1),
                                     L.ptr(s2), L.ptr(s1_local), L.ptr(s2_local), int(P_global),
                                     L.ptr(adj_dh if need_adj else None), L.ptr(ydir), L.ptr(dgamma2),
                                     L.ptr(dbeta2), int(bool(accumulate_affine)), L.stream()), "rgan_bn_dd_apply")
    return (adj_dh if need_adj else None), ydir


def act_dd(a, act_out, dh, act, alpha, need_adj=True, need_ydir=False, adj_dh=None, ydir=None):
    """No-BN layer: (adj_dh = a act'(y) or None, ydir = a dh act''(y) or None)."""
    for t in (a, dh, adj_dh, ydir):
        if t is not None and t.stride() != act_out.stride():
            raise L.RganError("act_dd: a, act_out, dh and the outputs must share strides")
    if need_adj and adj_dh is None:
        adj_dh = torch.empty_like(act_out)
    if need_ydir and ydir is None:
        ydir = torch.empty_like(act_out)
    if not need_ydir:
        ydir = None
    L.check(L.lib().rgan_act_dd(L.ptr(a), L.ptr(act_out), L.ptr(dh), act_out.numel(), L.ACT[act], float(alpha),
                                L.ptr(adj_dh if need_adj else None), L.ptr(ydir), L.stream()), "rgan_act_dd")
    return (adj_dh if need_adj else None), ydir


def act_backward_ex(da, a, act, alpha=0.0, add=None, out=None):
    """dx = da * act'(a) + add."""
    if da.stride() != a.stride() or (add is not None and add.stride() != a.stride()):
        raise L.RganError("act_backward_ex: da, a, add must share strides")
    dx = torch.empty_like(a) if out is None else out
    L.check(L.lib().rgan_act_backward_ex(L.ptr(da), L.ptr(a), L.ptr(add), a.numel(), L.ACT[act], float(alpha),
                                         L.ptr(dx), L.stream()), "rgan_act_backward_ex")
    return dx


def act_backward(da, a, act, alpha=0.0):
    """dx = da * act'(x) from the activation output a (same strides required)."""
    if da.stride() != a.stride():
        da = da.contiguous(memory_format=torch.channels_last) if is_nhwc(a) else da.contiguous()
    dx = torch.empty_like(a)
    L.check(L.lib().rgan_act_backward(L.ptr(da), L.ptr(a), a.numel(), L.ACT[act], float(alpha), L.ptr(dx),
                                      L.stream()), "rgan_act_backward")
    return dx


def channel_sum(t, out, accumulate=False):
    """out[c] (+)= sum over (b, h, w) of t[:, c] (bias gradients), NHWC or [B, C, 1, 1]."""
    B, C, H, W = t.shape
    if is_nhwc(t):
        sp, sc = (t.stride()[0] if H * W == 1 else C), 1
    else:
        raise L.RganError("channel_sum expects NHWC (channels_last) input")
    part = L.workspace(L.lib().rgan_bn_partial_bytes(B * H * W, C), t.device)
    L.check(L.lib().rgan_channel_sum(L.ptr(t), B * H * W, C, sp, sc, L.ptr(out), int(bool(accumulate)),
                                     L.ptr(part), L.stream()), "rgan_channel_sum")
    return out


# ------------------------------------------------------------------ loss heads / GP
HEAD_MAX_N = 65536  # one workgroup strides over the batch (include/rgan.h)


def _head_check(what, n, exact=(), gsum=None, gsum_min=0):
    """The head kernels take raw pointers and one count ``n``: every tensor handed to them must
    be float32 and contiguous, each (name, tensor, count) of ``exact`` must hold exactly
    ``count`` elements and ``gsum`` at least ``gsum_min``.  Pure Python, before any pointer is
    taken; a None tensor is an argument not given."""
    if not 1 <= n <= HEAD_MAX_N:
        raise L.RganError(f"{what}: n = {n} is outside 1 .. {HEAD_MAX_N}")
    for name, t, count in tuple(exact) + (("gsum", gsum, None),):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise L.RganError(f"{what}: {name} must be float32 (got {t.dtype})")
        if not t.is_contiguous():
            raise L.RganError(f"{what}: {name} must be contiguous")
        if count is not None and t.numel() != count:
            raise L.RganError(f"{what}: {name} has {t.numel()} elements, expected {count}")
    if gsum is not None and gsum.numel() < gsum_min:
        raise L.RganError(f"{what}: gsum has {gsum.numel()} elements, expected at least {gsum_min}")


def loss_head(kind, side, r, f, need_dr=True, need_df=True, dr=None, df=None):
    t = r if r is not None else f
    n = t.numel()
    _head_check("loss_head", n, (("r", r, n), ("f", f, n), ("dr", dr, n), ("df", df, n)))
    loss = torch.empty((), dtype=torch.float32, device=t.device)
    if dr is None:
        dr = torch.empty_like(r) if (r is not None and need_dr) else None
    if df is None:
        df = torch.empty_like(f) if (f is not None and need_df) else None
    L.check(L.lib().rgan_loss_head(int(kind), int(side), L.ptr(r), L.ptr(f), n, L.ptr(loss), L.ptr(dr),
                                   L.ptr(df), L.stream()), "rgan_loss_head")
    return loss, dr, df


def loss_head_pair(kind, r, f, need_dr=True, need_df=True, dr=None, df=None):
    """Heads 1-4 D side: (loss3 = [real, fake, sum], dr, df) in one launch."""
    n = r.numel()
    _head_check("loss_head_pair", n, (("r", r, n), ("f", f, n), ("dr", dr, n), ("df", df, n)))
    loss3 = torch.empty(3, dtype=torch.float32, device=r.device)
    if dr is None and need_dr:
        dr = torch.empty_like(r)
    if df is None and need_df:
        df = torch.empty_like(f)
    L.check(L.lib().rgan_loss_head_pair(int(kind), L.ptr(r), L.ptr(f), n, L.ptr(loss3), L.ptr(dr),
                                        L.ptr(df), L.stream()), "rgan_loss_head_pair")
    return loss3, dr, df


def loss_head_joint(kind, y, out=None):
    """Heads 5-8, G side, on the joint [D(G(z)); D(x)] output: (loss, dy) with dy's second
    half zero (rgan_loss_head_joint).  ``out`` receives dy (2n float32, contiguous)."""
    if y.numel() % 2:
        raise L.RganError(f"loss_head_joint: y has {y.numel()} elements, expected an even count [f; r]")
    n = y.numel() // 2
    _head_check("loss_head_joint", n, (("y", y, 2 * n), ("out", out, 2 * n)))
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    dy = torch.empty_like(y) if out is None else out
    L.check(L.lib().rgan_loss_head_joint(int(kind), L.ptr(y), n, L.ptr(loss), L.ptr(dy), L.stream()),
            "rgan_loss_head_joint")
    return loss, dy


def loss_head_dist(kind, side, phase, r, f, n_global, gsum=None, need_dr=True, need_df=True):
    t = r if r is not None else f
    n = t.numel()
    # phase 1 reads the global (sum r, sum f); phase 2 the global loss sum (heads 1-5) or all six
    _head_check("loss_head_dist", n, (("r", r, n), ("f", f, n)), gsum=gsum,
                gsum_min=1 if kind <= 5 else 2 if phase == 1 else 6)
    sums = torch.zeros(4, dtype=torch.float32, device=t.device)
    loss = torch.empty((), dtype=torch.float32, device=t.device)
    dr = torch.empty_like(r) if (phase == 2 and r is not None and need_dr) else None
    df = torch.empty_like(f) if (phase == 2 and f is not None and need_df) else None
    L.check(L.lib().rgan_loss_head_dist(int(kind), int(side), int(phase), L.ptr(r), L.ptr(f), n, int(n_global),
                                        L.ptr(gsum), L.ptr(sums), L.ptr(loss), L.ptr(dr), L.ptr(df), L.stream()),
            "rgan_loss_head_dist")
    return sums, loss, dr, df


def scale(t, s, out=None):
    if out is None:
        out = torch.empty_like(t)
    L.check(L.lib().rgan_scale(L.ptr(t), L.ptr(s), t.numel(), L.ptr(out), L.stream()), "rgan_scale")
    return out


def gp_interp(x, xf, u, out=None):
    B = x.shape[0]
    x = x.contiguous()
    xf = xf.contiguous()
    if out is None:
        out = torch.empty_like(x)
    elif not out.is_contiguous() or out.shape != x.shape:
        raise L.RganError("gp_interp: out must be contiguous and shaped like x")
    L.check(L.lib().rgan_gp_interp(L.ptr(x), L.ptr(xf), L.ptr(u.contiguous()), B, x[0].numel(), L.ptr(out),
                                   L.stream()), "rgan_gp_interp")
    return out


def gp_penalty(g, lam, n_global):
    g = g.contiguous()
    B = g.shape[0]
    norms = torch.empty(B, dtype=torch.float32, device=g.device)
    loss = torch.empty((), dtype=torch.float32, device=g.device)
    L.check(L.lib().rgan_gp_penalty(L.ptr(g), B, g[0].numel(), float(lam), int(n_global), L.ptr(norms),
                                    L.ptr(loss), L.stream()), "rgan_gp_penalty")
    return loss, norms, g


def gp_penalty_backward(g, norms, lam, n_global, gscale, out=None):
    """dGP/dg = gscale * lam * 2 (n_b - 1) / n_global * g / n_b per sample b.  ``out`` may be
    ``g`` itself (in place: each element is read before it is written)."""
    B = g.shape[0]
    if not g.is_contiguous():
        raise L.RganError("gp_penalty_backward: g must be contiguous")
    dg = torch.empty_like(g) if out is None else out
    if not dg.is_contiguous() or dg.shape != g.shape:
        raise L.RganError("gp_penalty_backward: out must be contiguous and shaped like g")
    L.check(L.lib().rgan_gp_penalty_backward(L.ptr(g), L.ptr(norms), B, g[0].numel(), float(lam), int(n_global),
                                             L.ptr(gscale), L.ptr(dg), L.stream()), "rgan_gp_penalty_backward")
    return dg


def gp_zc_penalty(g, gamma, n_global):
    """Zero-centred penalty head (R1 / R2): (gamma / 2 * sum_b ||g_b||^2 / n_global, the
    per-sample squared norms, g as the kernel read it)."""
    L.require_cuda(g)
    g = g.contiguous()
    B = g.shape[0]
    per = g[0].numel()
    sq = torch.empty(B, dtype=torch.float32, device=g.device)
    loss = torch.empty((), dtype=torch.float32, device=g.device)
    ws = L.workspace(L.lib().rgan_gp_zc_workspace(B, per), g.device)
    L.check(L.lib().rgan_gp_zc_penalty(L.ptr(g), B, per, float(gamma), int(n_global), L.ptr(sq), L.ptr(loss),
                                       L.ptr(ws), L.stream()), "rgan_gp_zc_penalty")
    return loss, sq, g


def gp_zc_penalty_backward(g, gamma, n_global, gscale, out=None):
    """dZC/dg = gscale * gamma / n_global * g (gscale a device scalar, or None for 1).  ``out``
    may be ``g`` itself (in place: each element is read before it is written)."""
    L.require_cuda(g, gscale, out)
    B = g.shape[0]
    if not g.is_contiguous():
        raise L.RganError("gp_zc_penalty_backward: g must be contiguous")
    dg = torch.empty_like(g) if out is None else out
    if not dg.is_contiguous() or dg.shape != g.shape:
        raise L.RganError("gp_zc_penalty_backward: out must be contiguous and shaped like g")
    L.check(L.lib().rgan_gp_zc_penalty_backward(L.ptr(g), B, g[0].numel(), float(gamma), int(n_global),
                                                L.ptr(gscale), L.ptr(dg), L.stream()),
            "rgan_gp_zc_penalty_backward")
    return dg


# ------------------------------------------------------------------ spectral norm
def sn_view(w, transposed):
    """(rows, cols, rs, hs, lo) of torch's reshape_weight_to_matrix (dim 0 conv, dim 1 convT)."""
    if w.dim() == 2:
        w = w.view(w.shape[0], w.shape[1], 1, 1)
    a, b, kh, kw = w.shape
    kk = kh * kw
    if transposed:  # [cin][cout][kh][kw] -> rows = cout
        return b, a * kk, kk, b * kk, kk
    return a, b * kk, b * kk, kk, kk


def spectral_power(w, u, v, transposed, eps=1e-12, do_iter=True):
    rows, cols, rs, hs, lo = sn_view(w, transposed)
    lib = L.lib()
    inv_sigma = torch.empty(1, dtype=torch.float32, device=w.device)
    ws = L.workspace(lib.rgan_spectral_ws_bytes(rows, cols), w.device)
    L.check(lib.rgan_spectral_power(L.ptr(w), rows, cols, rs, hs, lo, float(eps), L.ptr(u), L.ptr(v),
                                     L.ptr(inv_sigma), int(bool(do_iter)), L.ptr(ws), L.stream()),
            "rgan_spectral_power")
    return inv_sigma


def spectral_power_batch(layers, eps=1e-12):
    """One power iteration for every (w, u, v, transposed) of a net call, in four launches
    (rgan_spectral_power_batch): u, v updated in place; returns [(u_copy, v_copy, inv_sigma)]
    per layer (the copies autograd saves, as torch spectral_norm's clones)."""
    n = len(layers)
    if n == 0:
        return []
    if n > 16:
        raise L.RganError("spectral_power_batch: at most 16 layers per call")
    dev = layers[0][0].device
    arr = (L.RganSnLayer * n)()
    outs = []
    for i, (w, u, v, tr) in enumerate(layers):
        rows, cols, rs, hs, lo = sn_view(w, tr)
        uc, vc = torch.empty_like(u), torch.empty_like(v)
        inv = torch.empty(1, dtype=torch.float32, device=dev)
        arr[i] = L.RganSnLayer(w.data_ptr(), rows, cols, lo, rs, hs, u.data_ptr(), v.data_ptr(), uc.data_ptr(),
                               vc.data_ptr(), inv.data_ptr())
        outs.append((uc, vc, inv))
    lib = L.lib()
    ws = L.workspace(lib.rgan_spectral_batch_ws_bytes(n, ctypes.cast(arr, ctypes.c_void_p)), dev)
    L.check(lib.rgan_spectral_power_batch(n, ctypes.cast(arr, ctypes.c_void_p), float(eps), L.ptr(ws), L.stream()),
            "rgan_spectral_power_batch")
    return outs


def spectral_backward(w, dw_eff, u, v, inv_sigma, transposed, out=None):
    """dW_orig of W_eff = W / sigma(W) (u, v constant); ``out`` given: added into it."""
    rows, cols, rs, hs, lo = sn_view(w, transposed)
    acc = out is not None
    dw = out if acc else torch.empty_like(w)
    ws = L.workspace(4096, w.device)
    L.check(L.lib().rgan_spectral_backward(L.ptr(w), L.ptr(dw_eff), rows, cols, rs, hs, lo, L.ptr(u), L.ptr(v),
                                           L.ptr(inv_sigma), L.ptr(dw), int(acc), L.ptr(ws), L.stream()),
            "rgan_spectral_backward")
    return dw


# ------------------------------------------------------------------ device sampling
class DeviceRNG:
    """Counter-based device draws for --rgan_rng device (rgan_rng_fill / rgan_rng_choice):
    the counter is a device int64 the kernels advance, so graph replays draw fresh values."""

    def __init__(self, seed, device):
        self.seed = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & ((1 << 64) - 1)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)

    def normal(self, shape):
        out = torch.empty(shape, dtype=torch.float32, device=self.counter.device)
        L.check(L.lib().rgan_rng_fill(L.ptr(out), out.numel(), 0, self.seed, L.ptr(self.counter), L.stream()),
                "rgan_rng_fill")
        return out

    def uniform(self, shape):
        out = torch.empty(shape, dtype=torch.float32, device=self.counter.device)
        L.check(L.lib().rgan_rng_fill(L.ptr(out), out.numel(), 1, self.seed, L.ptr(self.counter), L.stream()),
                "rgan_rng_fill")
        return out

    def choice(self, N, n):
        """n distinct indices of [0, N) (numpy.random.choice(N, n, replace=False))."""
        out = torch.empty(n, dtype=torch.int64, device=self.counter.device)
        L.check(L.lib().rgan_rng_choice(L.ptr(out), int(N), int(n), self.seed, L.ptr(self.counter), L.stream()),
                "rgan_rng_choice")
        return out


# ------------------------------------------------------------------ Adam / data
def _arrays(params, *others):
    """void*[n] of ``params``' and each other tensor list's addresses, then long long[n] of
    ``params``' element counts: each array as the void* the C ABI takes."""
    n = max(len(params), 1)
    arrs = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (params,) + others]
    arrs.append((ctypes.c_longlong * n)(*[p.numel() for p in params]))
    return [ctypes.cast(a, ctypes.c_void_p) for a in arrs]


def adam(params, grads, exp_avgs, exp_avg_sqs, hyper, step):
    P, G, M, V, N = _arrays(params, grads, exp_avgs, exp_avg_sqs)
    L.check(L.lib().rgan_adam(len(params), P, G, M, V, N, L.ptr(hyper), L.ptr(step), L.stream()), "rgan_adam")


def adam_packed(params, grads, exp_avgs, exp_avg_sqs, hyper, step, layouts):
    """``adam`` that also writes the cached GEMM layouts ``layouts`` ([(param index, key,
    pack-cache entry)], _PackCache.layouts_of) from the updated values (rgan_adam_packed).
    ``step``: the count, a view whose next float is the group's arrival ticket (optim.Adam)."""
    if step.untyped_storage().nbytes() < 4 * (step.storage_offset() + 2):
        raise L.RganError("adam_packed: step must be followed by its arrival-ticket word (float[2] storage)")
    P, G, M, V, N = _arrays(params, grads, exp_avgs, exp_avg_sqs)
    k = len(layouts)
    packs = (L.RganAdamPack * max(k, 1))()
    for i, (j, _key, ent) in enumerate(layouts):
        packs[i] = L.RganAdamPack(j, ent.which, ctypes.pointer(ent.d), ent.buf.data_ptr())
    L.check(L.lib().rgan_adam_packed(len(params), P, G, M, V, N, L.ptr(hyper), L.ptr(step), k,
                                     ctypes.cast(packs, ctypes.c_void_p), L.stream()), "rgan_adam_packed")


def lr_decay(hyper, gamma):
    L.check(L.lib().rgan_lr_decay(L.ptr(hyper), float(gamma), L.stream()), "rgan_lr_decay")


def gather_images(images, idx, out=None):
    """images[idx] as float32; a uint8 dataset (decoded images, relativisticgan_amd.data) is
    converted on the fly with ToTensor + Normalize(0.5, 0.5) (GLI:160-166)."""
    B = idx.numel()
    per = images[0].numel()
    if out is None:
        out = torch.empty((B,) + tuple(images.shape[1:]), dtype=torch.float32, device=images.device)
    if images.dtype == torch.uint8:
        L.check(L.lib().rgan_gather_images_u8(L.ptr(images), L.ptr(idx), B, per, L.ptr(out), L.stream()),
                "rgan_gather_images_u8")
        return out
    L.check(L.lib().rgan_gather_images(L.ptr(images), L.ptr(idx), B, per, L.ptr(out), L.stream()),
            "rgan_gather_images")
    return out


# ------------------------------------------------------------------ differentiable augmentation
def diffaug(x, u, policy, adjoint=False, out=None, gate=None, p=None, geo=None):
    """The per-sample colour / translation / cutout transform of include/rgan.h rgan_diffaug
    (``policy``: bit 1 colour, 2 translation, 4 cutout; ``u``: [B][8] uniforms), or with
    ``adjoint`` its transpose applied to a gradient.  ``out``: a contiguous buffer other than
    ``x`` (e.g. half of a batched D input).  With ``gate`` ([B][4] uniforms) and ``p`` (a device
    double) each group of a sample is applied iff its gate is below p (rgan_diffaug_p).
    ``policy`` >= 8 (bit 8 x-flip, 16 quarter turns, 32 warp) needs ``geo``, the [B][8] uniforms
    of those groups, and runs rgan_diffaug_geo; below 8 ``geo`` is not read."""
    L.require_cuda(x, u, out)
    policy = int(policy)
    if policy >= 8:
        if policy > 63:
            raise L.RganError(f"diffaug: policy must lie in [0, 63], got {policy}")
        if geo is None:
            raise L.RganError("diffaug: policy >= 8 (xflip / rot90 / warp) needs geo, their [B][8] uniforms")
        if not (torch.is_tensor(geo) and geo.is_cuda and geo.device == x.device):
            raise L.RganError("diffaug: geo must be a tensor on x's device")
        if geo.dtype != torch.float32 or geo.dim() != 2 or geo.shape[1] != 8 or not geo.is_contiguous():
            raise L.RganError(f"diffaug: geo must be a contiguous float32 [B][8] tensor, got {geo.dtype} "
                              f"{tuple(geo.shape)}")
    if x.dim() != 4 or x.dtype != torch.float32 or u.dtype != torch.float32:
        raise L.RganError("diffaug: x must be a float32 [B][C][H][W] tensor and u float32")
    B, C, H, W = x.shape
    if tuple(u.shape) != (B, 8):
        raise L.RganError(f"diffaug: u must be [{B}][8] (one row of uniforms per sample), got {tuple(u.shape)}")
    if policy >= 8 and geo.shape[0] != B:
        raise L.RganError(f"diffaug: geo must be [{B}][8] (one row of uniforms per sample), got {tuple(geo.shape)}")
    if policy & 16 and H != W:
        raise L.RganError(f"diffaug: rot90 (policy bit 16) needs a square image, got {H} x {W}")
    if (gate is None) != (p is None):
        raise L.RganError("diffaug: gate and p come together (both or neither)")
    if gate is not None:
        if not (torch.is_tensor(gate) and torch.is_tensor(p)) or not (gate.is_cuda and p.is_cuda):
            raise L.RganError("diffaug: gate and p must be device tensors (p is read by the kernel at run time)")
        if gate.dtype != torch.float32 or tuple(gate.shape) != (B, 4) or not gate.is_contiguous():
            raise L.RganError(f"diffaug: gate must be a contiguous float32 [{B}][4] tensor, got {gate.dtype} "
                              f"{tuple(gate.shape)}")
        if p.dtype != torch.float64 or p.numel() != 1 or gate.device != x.device or p.device != x.device:
            raise L.RganError("diffaug: p must be one float64 on x's device")
    x = x.contiguous()
    u = u.contiguous()
    if out is None:
        out = torch.empty_like(x)
    elif not out.is_contiguous() or out.shape != x.shape or out.dtype != torch.float32:
        raise L.RganError("diffaug: out must be contiguous float32 and shaped like x")
    lib = L.lib()
    if policy >= 8:
        ws = torch.empty(max(int(lib.rgan_diffaug_geo_workspace(B, C, H, W)), 1), dtype=torch.float32,
                         device=x.device)
        L.check(lib.rgan_diffaug_geo(L.ptr(x), L.ptr(u), L.ptr(geo), L.ptr(gate), L.ptr(p), B, C, H, W, policy,
                                     int(bool(adjoint)), L.ptr(ws), L.ptr(out), L.stream()), "rgan_diffaug_geo")
        return out
    ws = torch.empty(max(int(lib.rgan_diffaug_workspace(B, C, H, W)), 1), dtype=torch.float32, device=x.device)
    if gate is not None:
        L.check(lib.rgan_diffaug_p(L.ptr(x), L.ptr(u), L.ptr(gate), L.ptr(p), B, C, H, W, int(policy),
                                   int(bool(adjoint)), L.ptr(ws), L.ptr(out), L.stream()), "rgan_diffaug_p")
        return out
    L.check(lib.rgan_diffaug(L.ptr(x), L.ptr(u), B, C, H, W, int(policy), int(bool(adjoint)), L.ptr(ws), L.ptr(out),
                             L.stream()), "rgan_diffaug")
    return out


# ------------------------------------------------------------------ adaptive augmentation probability
def _ada_arrays(hyper, state):
    L.require_cuda(hyper, state)
    for name, t in (("hyper", hyper), ("state", state)):
        if t.dtype != torch.float64 or t.numel() != 4 or not t.is_contiguous():
            raise L.RganError(f"ada: {name} must be a contiguous float64[4] device tensor")
    if hyper.device != state.device:
        raise L.RganError("ada: hyper and state must share a device")


def ada_update(y_real, y_fake, hyper, state, adjust=True):
    """The rank statistic of one D step added into ``state`` = {p, S, N, calls} (include/rgan.h
    rgan_ada_update): S += #(y_real > y_fake) - #(y_real < y_fake) row by row, N += rows; with
    ``adjust`` the controller step of ``ada_adjust`` in the same launch."""
    _ada_arrays(hyper, state)
    L.require_cuda(y_real, y_fake)
    _f32(y_real, y_fake)
    n = y_real.numel()
    if n <= 0 or y_fake.numel() != n or y_real.device != state.device or y_fake.device != state.device:
        raise L.RganError(f"ada_update: y_real and y_fake must hold the same number (> 0) of outputs on the "
                          f"state's device, got {n} and {y_fake.numel()}")
    y_real, y_fake = y_real.contiguous(), y_fake.contiguous()
    L.check(L.lib().rgan_ada_update(L.ptr(y_real), L.ptr(y_fake), n, L.ptr(hyper), L.ptr(state), int(bool(adjust)),
                                    L.stream()), "rgan_ada_update")


def ada_adjust(hyper, state):
    """calls += 1 and, at every interval-th call with N > 0, the move of p (rgan_ada_adjust)."""
    _ada_arrays(hyper, state)
    L.check(L.lib().rgan_ada_adjust(L.ptr(hyper), L.ptr(state), L.stream()), "rgan_ada_adjust")


# ------------------------------------------------------------------ LeCam regularisation of D
def _lecam_arrays(what, hyper, state, *more):
    L.require_cuda(hyper, state, *more)
    for name, t in (("hyper", hyper), ("state", state)) + tuple((f"double[4] #{k}", t) for k, t in enumerate(more)):
        if t.dtype != torch.float64 or t.numel() != 4 or not t.is_contiguous():
            raise L.RganError(f"{what}: {name} must be a contiguous float64[4] device tensor")
        if t.device != state.device:
            raise L.RganError(f"{what}: {name} must be on the state's device")


def lecam(y_real, y_fake, hyper, state, n_global=None, partial=False, need_dr=True, need_df=True, dr=None, df=None,
          out=None):
    """The LeCam term of one D step (include/rgan.h rgan_lecam) on D's outputs ``y_real`` /
    ``y_fake`` (either may be None): returns ``(out, dr, df)``.  Fused (default): ``out[0]`` is the
    term and ``state`` = {a_real, a_fake, calls, 0} has moved.  ``partial``: ``state`` is left
    alone and ``out`` holds this rank's four sums for ``lecam_finish``.  The gradients are scaled
    with ``n_global`` rows (default: this call's).  ``dr`` / ``df``: buffers to write them into
    (e.g. the halves of one [2B] buffer); ``need_*`` False: that gradient is not formed."""
    _lecam_arrays("lecam", hyper, state, *(() if out is None else (out,)))
    if y_real is None and y_fake is None:
        raise L.RganError("lecam: y_real or y_fake (or both) must be given")
    t = y_real if y_real is not None else y_fake
    n = t.numel()
    n_global = n if n_global is None else int(n_global)
    if not 1 <= n <= n_global < 2 ** 31:
        raise L.RganError(f"lecam: n = {n} rows of n_global = {n_global} (need 1 <= n <= n_global < 2^31)")
    for name, y, d in (("real", y_real, dr), ("fake", y_fake, df)):
        if y is None and d is not None:
            raise L.RganError(f"lecam: a gradient buffer for the absent {name} side")
        for what, v in (("y_" + name, y), ("dy_" + name, d)):
            if v is None:
                continue
            L.require_cuda(v)
            if v.dtype != torch.float32 or not v.is_contiguous() or v.device != state.device:
                raise L.RganError(f"lecam: {what} must be a contiguous float32 tensor on the state's device")
            if v.numel() != n:
                raise L.RganError(f"lecam: {what} has {v.numel()} elements, expected {n}")
    if dr is None and y_real is not None and need_dr:
        dr = torch.empty_like(y_real)
    if df is None and y_fake is not None and need_df:
        df = torch.empty_like(y_fake)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=state.device)
    L.check(L.lib().rgan_lecam(L.ptr(y_real), L.ptr(y_fake), n, n_global, L.ptr(hyper), L.ptr(state), L.ptr(dr),
                               L.ptr(df), L.ptr(out), int(bool(partial)), L.stream()), "rgan_lecam")
    return out, dr, df


def lecam_finish(sums, n_global, sides, hyper, state, loss=None):
    """The all-reduced sums of ``lecam(partial=True)`` turned into the term (returned, a
    float64[4] whose first element it is) and the move of the anchors (rgan_lecam_finish).
    ``sides``: 1 the real side was given, 2 the fake side, 3 both."""
    loss = sums if loss is None else loss
    _lecam_arrays("lecam_finish", hyper, state, sums, loss)
    if not 1 <= int(n_global) < 2 ** 31 or int(sides) not in (1, 2, 3):
        raise L.RganError(f"lecam_finish: n_global = {n_global}, sides = {sides} (need n_global >= 1, sides in 1..3)")
    L.check(L.lib().rgan_lecam_finish(L.ptr(sums), int(n_global), int(sides), L.ptr(hyper), L.ptr(state), L.ptr(loss),
                                      L.stream()), "rgan_lecam_finish")
    return loss


# ------------------------------------------------------------------ moving average of G
def ema_update(avgs, params, hyper, count):
    """One moving-average step of include/rgan.h rgan_ema_update over the tensor pairs:
    ``count += 1``, then ``avg = lerp(avg, p, 1 - beta_t)`` with beta_t from ``hyper`` (device
    double[2] {beta, warmup}) and the new count (device float[1]).  An ``avg`` walks its ``p``
    with one flat index, so it must share p's shape and strides (dense, any permutation)."""
    if len(avgs) != len(params):
        raise L.RganError(f"ema_update: {len(avgs)} averages for {len(params)} parameters")
    L.require_cuda(hyper, count, *avgs, *params)
    _f32(count, *avgs, *params)
    if hyper.dtype != torch.float64 or hyper.numel() < 2 or count.numel() < 1:
        raise L.RganError("ema_update: hyper must be float64[2] {beta, warmup} and count float32[1]")
    for a, p in zip(avgs, params):
        if a.shape != p.shape or a.stride() != p.stride():
            raise L.RganError(f"ema_update: average {tuple(a.shape)} / {a.stride()} does not match its parameter "
                              f"{tuple(p.shape)} / {p.stride()}")
        if p.numel() and 1 + sum((s - 1) * st for s, st in zip(p.shape, p.stride())) != p.numel():
            raise L.RganError("ema_update: tensors must be dense (the kernel walks numel floats of storage)")
    P, A, N = _arrays(params, avgs)
    L.check(L.lib().rgan_ema_update(len(params), A, P, N, L.ptr(hyper), L.ptr(count), L.stream()), "rgan_ema_update")


# ------------------------------------------------------------------ GEMM arithmetic
def set_gemm_emulation(on):
    """Run the FAST 128x128 forward / data-gradient conv GEMMs as fp32 emulated on the bf16 MFMA
    (bf16x6, see include/rgan.h) instead of the fp32 MFMA; returns the previous setting."""
    prev = L.lib().rgan_set_gemm_emulation(1 if on else 0)
    if prev < 0:
        raise L.RganError("rgan_set_gemm_emulation failed")
    return bool(prev)


# ------------------------------------------------------------------ live launch timing
def profile_begin(capacity=100000):
    L.check(L.lib().rgan_profile_begin(int(capacity)), "rgan_profile_begin")


def profile_end():
    """{'ms', 'flops', 'launches', 'kernels': [{name, ms, flops, launches}]} of the GEMM launches."""
    lib = L.lib()
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    L.check(lib.rgan_profile_end(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n)), "rgan_profile_end")
    kern = []
    for i in range(256):
        name = ctypes.create_string_buffer(200)
        kms, kfl, kn = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        if lib.rgan_profile_kernel(i, name, 200, ctypes.byref(kms), ctypes.byref(kfl), ctypes.byref(kn)) != 0:
            break  # past the last kernel id
        if kn.value:
            kern.append({"name": name.value.decode(), "ms": kms.value, "flops": kfl.value, "launches": kn.value,
                         "tflops": kfl.value / kms.value / 1e9 if kms.value > 0 else 0.0})
    return {"ms": ms.value, "flops": fl.value, "launches": n.value, "kernels": kern}


# ------------------------------------------------------------------ segmented sort
def _f32c(what, *ts):
    for t in ts:
        L.require_cuda(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.RganError(f"{what}: needs contiguous float32 device tensors")


def sort_segments_tile():
    """Keys per block of rgan_sort_segments (a segment takes ceil(len / tile) blocks)."""
    return int(L.lib().rgan_sort_segments_tile())


def sort_segments(x, out=None, tmp=None):
    """Each row of ``x`` [nseg][len] sorted ascending in the total order of its bit patterns
    (include/rgan.h rgan_sort_segments) into ``out`` (may be ``x``); ``tmp``: scratch of x's size."""
    if x.dim() != 2 or x.numel() == 0 or x.numel() >= 2 ** 31:
        raise L.RganError(f"sort_segments: needs [nseg][len] with 1 <= nseg len < 2^31, got {tuple(x.shape)}")
    out = torch.empty_like(x) if out is None else out
    tmp = torch.empty_like(x) if tmp is None else tmp
    _f32c("sort_segments", x, out, tmp)
    if out.numel() != x.numel() or tmp.numel() != x.numel() or tmp.data_ptr() in (x.data_ptr(), out.data_ptr()):
        raise L.RganError("sort_segments: out and tmp must have x's size, and tmp must be neither of them")
    nseg, n = x.shape
    nbytes = L.lib().rgan_sort_segments_ws_bytes(nseg, n)
    ws = L.workspace(nbytes, x.device)
    L.check(L.lib().rgan_sort_segments(L.ptr(x), L.ptr(out), L.ptr(tmp), nseg, n, L.ptr(ws), nbytes, L.stream()),
            "rgan_sort_segments")
    return out


# ------------------------------------------------------------------ sliced Wasserstein distance
def _swd_images(what, x):
    _f32c(what, x)
    if x.dim() != 4 or x.shape[2] != x.shape[3] or not 1 <= x.shape[1] <= 4 or x.numel() == 0:
        raise L.RganError(f"{what}: needs planar [N][C][S][S] images with C <= 4, got {tuple(x.shape)}")
    return tuple(int(v) for v in x.shape[:3])


def swd_load_u8(x, out=None):
    """uint8 images viewed as [N][C][S][S] through any strides (a CHW dataset, or the permuted view
    of HWC bytes) as planar float32 (rgan_swd_load_u8)."""
    L.require_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[2] != x.shape[3] or x.numel() == 0 or min(x.stride()) < 0:
        raise L.RganError(f"swd_load_u8: needs a uint8 [N][C][S][S] view, got {x.dtype} {tuple(x.shape)}")
    N, C, S, _ = x.shape
    out = torch.empty((N, C, S, S), dtype=torch.float32, device=x.device) if out is None else out
    _f32c("swd_load_u8", out)
    if out.numel() != x.numel():
        raise L.RganError("swd_load_u8: out has another size")
    strides = (ctypes.c_longlong * 4)(*x.stride())
    L.check(L.lib().rgan_swd_load_u8(L.ptr(x), N, C, S, ctypes.cast(strides, ctypes.c_void_p), L.ptr(out),
                                     L.stream()), "rgan_swd_load_u8")
    return out


def swd_pyr_down(x):
    """The next Gaussian-pyramid level of planar images (rgan_swd_pyr_down): half the side."""
    N, C, S = _swd_images("swd_pyr_down", x)
    out = torch.empty((N, C, S // 2, S // 2), dtype=torch.float32, device=x.device)
    L.check(L.lib().rgan_swd_pyr_down(L.ptr(x), N, C, S, L.ptr(out), L.stream()), "rgan_swd_pyr_down")
    return out


def swd_laplace(fine, coarse, out=None):
    """fine - up(coarse) (rgan_swd_laplace); ``out`` may be ``fine``."""
    N, C, S = _swd_images("swd_laplace", fine)
    out = torch.empty_like(fine) if out is None else out
    _f32c("swd_laplace", coarse, out)
    if tuple(coarse.shape) != (N, C, S // 2, S // 2) or out.shape != fine.shape:
        raise L.RganError(f"swd_laplace: coarse {tuple(coarse.shape)} / out do not go with fine {tuple(fine.shape)}")
    L.check(L.lib().rgan_swd_laplace(L.ptr(fine), L.ptr(coarse), N, C, S, L.ptr(out), L.stream()), "rgan_swd_laplace")
    return out


def swd_positions(u, side):
    """Patch centres 3 + floor(u (side - 6)) as int32, u uniform draws in [0, 1) (rgan_swd_positions)."""
    _f32c("swd_positions", u)
    pos = torch.empty(u.shape, dtype=torch.int32, device=u.device)
    L.check(L.lib().rgan_swd_positions(L.ptr(u), u.numel(), int(side), L.ptr(pos), L.stream()), "rgan_swd_positions")
    return pos


def swd_descriptors(img, pos, desc, part):
    """The 7x7xC patches of ``img`` [N][C][S][S] around ``pos`` [N][P][2] (int32 y, x) into the rows
    ``desc`` [N P][49 C], and the images' double {sum, sum of squares} per channel into ``part``
    [N][C][2] (rgan_swd_descriptors); desc and part may be slices of larger buffers."""
    N, C, S = _swd_images("swd_descriptors", img)
    L.require_cuda(pos, desc, part)
    if pos.dtype != torch.int32 or not pos.is_contiguous() or pos.dim() != 3 or pos.shape[0] != N or pos.shape[2] != 2:
        raise L.RganError(f"swd_descriptors: pos must be contiguous int32 [N][P][2], got {tuple(pos.shape)}")
    P = int(pos.shape[1])
    _f32c("swd_descriptors", desc)
    if tuple(desc.shape) != (N * P, 49 * C):
        raise L.RganError(f"swd_descriptors: desc must be [{N * P}][{49 * C}], got {tuple(desc.shape)}")
    if part.dtype != torch.float64 or not part.is_contiguous() or tuple(part.shape) != (N, C, 2):
        raise L.RganError(f"swd_descriptors: part must be contiguous float64 [{N}][{C}][2]")
    L.check(L.lib().rgan_swd_descriptors(L.ptr(img), N, C, S, P, L.ptr(pos), L.ptr(desc), L.ptr(part), L.stream()),
            "rgan_swd_descriptors")


def swd_normalize(desc, part):
    """``desc`` [M][49 C] normalised per channel in place with the statistics of ``part``
    [nparts][C][2]; returns them, float64 [C][2] {mean, std}, on the device (rgan_swd_normalize)."""
    _f32c("swd_normalize", desc)
    L.require_cuda(part)
    if part.dtype != torch.float64 or not part.is_contiguous() or part.dim() != 3 or part.shape[2] != 2:
        raise L.RganError("swd_normalize: part must be contiguous float64 [nparts][C][2]")
    nparts, C = int(part.shape[0]), int(part.shape[1])
    if desc.dim() != 2 or desc.shape[1] != 49 * C or desc.numel() == 0 or nparts == 0:
        raise L.RganError(f"swd_normalize: desc {tuple(desc.shape)} does not go with {C} channels")
    stats = torch.empty((C, 2), dtype=torch.float64, device=desc.device)
    L.check(L.lib().rgan_swd_normalize(L.ptr(desc), int(desc.shape[0]), C, L.ptr(part), nparts, L.ptr(stats),
                                       L.stream()), "rgan_swd_normalize")
    return stats


def swd_unit_columns(dirs):
    """``dirs`` [K][D] scaled in place to unit columns (rgan_swd_unit_columns)."""
    _f32c("swd_unit_columns", dirs)
    if dirs.dim() != 2 or dirs.numel() == 0:
        raise L.RganError("swd_unit_columns: dirs must be [K][D]")
    L.check(L.lib().rgan_swd_unit_columns(L.ptr(dirs), int(dirs.shape[0]), int(dirs.shape[1]), L.stream()),
            "rgan_swd_unit_columns")
    return dirs


def swd_project(desc, dirs, out=None):
    """proj [D][M] = (desc [M][K] dirs [K][D]) transposed, fp32 in ascending k (rgan_swd_project)."""
    _f32c("swd_project", desc, dirs)
    if desc.dim() != 2 or dirs.dim() != 2 or desc.shape[1] != dirs.shape[0] or desc.numel() == 0 or dirs.numel() == 0:
        raise L.RganError(f"swd_project: desc {tuple(desc.shape)} and dirs {tuple(dirs.shape)} do not go together")
    M, K, D = int(desc.shape[0]), int(desc.shape[1]), int(dirs.shape[1])
    out = torch.empty((D, M), dtype=torch.float32, device=desc.device) if out is None else out
    _f32c("swd_project", out)
    if out.numel() != D * M:
        raise L.RganError("swd_project: out has another size")
    L.check(L.lib().rgan_swd_project(L.ptr(desc), L.ptr(dirs), M, K, D, L.ptr(out), L.stream()), "rgan_swd_project")
    return out


def swd_l1(a, b, out=None):
    """sum |a - b| into ``out`` (a float64 device scalar or one-element view; rgan_swd_l1)."""
    _f32c("swd_l1", a, b)
    n = a.numel()
    if n == 0 or n != b.numel() or n >= 2 ** 31:
        raise L.RganError("swd_l1: a and b must hold the same 1 <= n < 2^31 elements")
    out = torch.empty(1, dtype=torch.float64, device=a.device) if out is None else out
    if out.dtype != torch.float64 or out.numel() != 1 or not out.is_cuda:
        raise L.RganError("swd_l1: out must be one float64 on the device")
    nbytes = L.lib().rgan_swd_l1_ws_bytes(n)
    ws = L.workspace(nbytes, a.device)
    L.check(L.lib().rgan_swd_l1(L.ptr(a), L.ptr(b), n, L.ptr(out), L.ptr(ws), nbytes, L.stream()), "rgan_swd_l1")
    return out


# ------------------------------------------------------------------ nearest training images
NN_NO_SELF = -2 ** 63  # RGAN_NN_NO_SELF: no reference is excluded


def nn_row_bytes(C, s):
    """Bytes of a descriptor row of ``C`` channels at working side ``s`` (rgan_nn_row_bytes): C s s
    rounded up to a multiple of 64; refuses C outside 1..4, s not in {8, 16, 32, 64} and > 12288."""
    n = int(L.lib().rgan_nn_row_bytes(int(C), int(s)))
    if n == 0:
        raise L.RganError(f"nn_row_bytes: no descriptor for {C} channels at side {s} (1 <= C <= 4, side in "
                          "{8, 16, 32, 64}, at most 12288 bytes)")
    return n


def nn_pack_u8(x, s):
    """uint8 images viewed as [N][C][S][S] through any strides -> ``(desc, norm)``: int8
    [N][row_bytes] box-mean descriptors at side ``s`` and their int32 squared norms (rgan_nn_pack_u8)."""
    L.require_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[2] != x.shape[3] or x.numel() == 0 or min(x.stride()) < 0:
        raise L.RganError(f"nn_pack_u8: needs a uint8 [N][C][S][S] view, got {x.dtype} {tuple(x.shape)}")
    N, C, S, _ = (int(v) for v in x.shape)
    s = int(s)
    row_bytes = nn_row_bytes(C, s)
    if S % s or S // s > 32:
        raise L.RganError(f"nn_pack_u8: side {s} must divide the image side {S}, by at most 32")
    desc = torch.empty((N, row_bytes), dtype=torch.int8, device=x.device)
    norm = torch.empty(N, dtype=torch.int32, device=x.device)
    strides = (ctypes.c_longlong * 4)(*x.stride())
    L.check(L.lib().rgan_nn_pack_u8(L.ptr(x), N, C, S, ctypes.cast(strides, ctypes.c_void_p), s, L.ptr(desc),
                                    L.ptr(norm), L.stream()), "rgan_nn_pack_u8")
    return desc, norm


def _nn_operands(what, a, na, b, nb):
    L.require_cuda(a, na, b, nb)
    for d, n in ((a, na), (b, nb)):
        if (d.dtype != torch.int8 or d.dim() != 2 or not d.is_contiguous() or d.numel() == 0
                or n.dtype != torch.int32 or not n.is_contiguous() or tuple(n.shape) != (d.shape[0],)):
            raise L.RganError(f"{what}: needs contiguous int8 [rows][row_bytes] descriptors with int32 [rows] norms")
    if a.shape[1] != b.shape[1]:
        raise L.RganError(f"{what}: row sizes {a.shape[1]} and {b.shape[1]} differ")
    return int(a.shape[0]), int(b.shape[0]), int(a.shape[1])


def nn_topk(a, na, b, nb, k, self_offset=None, nsplit=0, out=None):
    """``(dist, idx)``, int32 [Q][k]: for each row of ``a`` the ``k`` nearest rows of ``b`` by exact
    squared distance, ties to the smaller index; row ``q + self_offset`` of b is left out
    (``None``: none is).  ``nsplit``: parts of b, 0 = automatic; the result does not depend on it.
    ``out``: a (dist, idx) pair of contiguous int32 [Q][k] views to write (rgan_nn_topk)."""
    Q, R, row_bytes = _nn_operands("nn_topk", a, na, b, nb)
    k, nsplit = int(k), int(nsplit)
    if out is None:
        dist = torch.empty((Q, k), dtype=torch.int32, device=a.device)
        idx = torch.empty((Q, k), dtype=torch.int32, device=a.device)
    else:
        dist, idx = out
        L.require_cuda(dist, idx)
        for t in (dist, idx):
            if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (Q, k):
                raise L.RganError(f"nn_topk: out must be two contiguous int32 [{Q}][{k}] tensors")
    nbytes = L.lib().rgan_nn_topk_ws_bytes(Q, R, k, nsplit)
    ws = L.workspace(nbytes, a.device)
    self_offset = NN_NO_SELF if self_offset is None else int(self_offset)
    L.check(L.lib().rgan_nn_topk(L.ptr(a), L.ptr(na), Q, L.ptr(b), L.ptr(nb), R, row_bytes, k, self_offset, nsplit,
                                 L.ptr(dist), L.ptr(idx), L.ptr(ws), nbytes, L.stream()), "rgan_nn_topk")
    return dist, idx


def nn_covered(a, na, b, nb, radius, self_offset=None, out=None):
    """int32 [Q]: 1 where a row of ``a`` lies within ``radius[r]`` (int32 [R], squared, equality
    counts) of some row r of ``b`` other than ``q + self_offset``, else 0 (rgan_nn_covered)."""
    Q, R, row_bytes = _nn_operands("nn_covered", a, na, b, nb)
    L.require_cuda(radius)
    if radius.dtype != torch.int32 or not radius.is_contiguous() or tuple(radius.shape) != (R,):
        raise L.RganError(f"nn_covered: radius must be contiguous int32 [{R}]")
    flag = torch.empty(Q, dtype=torch.int32, device=a.device) if out is None else out
    L.require_cuda(flag)
    if flag.dtype != torch.int32 or not flag.is_contiguous() or tuple(flag.shape) != (Q,):
        raise L.RganError(f"nn_covered: out must be contiguous int32 [{Q}]")
    self_offset = NN_NO_SELF if self_offset is None else int(self_offset)
    L.check(L.lib().rgan_nn_covered(L.ptr(a), L.ptr(na), Q, L.ptr(b), L.ptr(nb), L.ptr(radius), R, row_bytes,
                                    self_offset, L.ptr(flag), L.stream()), "rgan_nn_covered")
    return flag
