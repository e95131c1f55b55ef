"""The C-ABI call stream of one fused layer, pinned against a recorded fixture.

``ConvLayerFn`` routes a layer's forward and backward over some twenty rgan_* entry points,
depending on BatchNorm, batch segments, the image-side patch GEMMs, G's first layer, spectral
norm, who owns the weight gradient and the hand-offs between consecutive layers (LayerLink).
Each case below runs one forward + backward through ``nets._Layer`` (a two-layer ``_Net``
chain where a link is needed) under relativisticgan_amd.abi_record.Recorder and compares the
rows -- entry point, scalars, decoded descriptors, pointers as p / 0 -- with
tests/golden/layer_abi_calls.json.  Call rows only: values are the business of the parity,
drift and fp64 tests.

A refactor of the host layer leaves the fixture alone.  A deliberate change of the routing
regenerates it (``python -m tests.test_layer_calls_gpu --write``, on the GPU) and shows the diff
in review.
"""
import json
import os
import sys

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_abi_calls.json")
DEV = "cuda"


def _layer(cin=16, cout=32, k=4, s=2, p=1, bn=True, act="lrelu", alpha=0.2, bias=False, transposed=False,
           spectral=False, upsample=1, nchw_out=False):
    from relativisticgan_amd import nets
    if transposed:
        conv = nets.ConvTranspose2d(cin, cout, k, s, p, bias=bias, spectral=spectral)
    else:
        conv = nets.Conv2d(cin, cout, k, s, p, bias=bias, spectral=spectral, upsample=upsample)
    norm = nets.BatchNorm2d(cout) if bn else None
    conv.to(DEV)
    if norm is not None:
        norm.to(DEV)
    return nets._Layer(conv, norm, act, alpha, nchw_out=nchw_out)


def _x(B=4, C=16, H=8, W=8, nhwc=True, grad=True):
    x = torch.randn(B, C, H, W, device=DEV)
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
    return x.requires_grad_(grad)


def _params(layer):
    return [p for m in (layer.conv, layer.bn) if m is not None for p in m.parameters()]


def _step(layer, x, own, segs=1, gsegs=None, da=None, training=True):
    """One forward + backward of the layer; inside ``owning_grads`` when ``own``."""
    from relativisticgan_amd import autograd as AG
    a = layer.run(x, training, segs, gsegs=gsegs)
    da = torch.randn_like(a) if da is None else da(a)
    if own:
        with AG.owning_grads():
            a.backward(da)
    else:
        a.backward(da)
    return a


# ---------------------------------------------------------------- the cases
def own_grad_set_then_accumulate():
    layer, x = _layer(), _x()
    _step(layer, x, own=True)
    assert layer.conv.weight.grad is not None
    _step(layer, x, own=True)


def autograd_grad():
    _step(_layer(), _x(), own=False)


def autograd_grad_bias():
    _step(_layer(bias=True), _x(), own=False)


def segs2():
    _step(_layer(), _x(), own=True, segs=2)


def segs2_gsegs1():
    """The G step's restricted backward: the rows of the second segment carry no gradient.  NaN
    in those rows of the output gradient reaches nothing, and (anomaly mode off) the second
    half of the input gradient is not written: where the allocator hands the backward the
    NaN-filled block freed just before it, that half still holds the NaN."""
    assert not torch.is_anomaly_enabled()
    layer, x0 = _layer(), _x()
    x = x0 * 1.0  # not a leaf: its gradient is the layer's own output buffer
    got = []
    x.register_hook(got.append)

    def da(a):
        g = torch.randn_like(a)
        g[2:] = float("nan")
        return g
    a = layer.run(x, True, 2, gsegs=1)
    g = da(a)
    poison = torch.full_like(x0, float("nan"))
    ptr = poison.data_ptr()
    del poison
    a.backward(g)
    dx, = got
    assert torch.isfinite(dx[:2]).all()
    assert all(torch.isfinite(p.grad).all() for p in _params(layer))
    if dx.data_ptr() == ptr:
        assert torch.isnan(dx[2:]).all()


def act_only():
    _step(_layer(bn=False), _x(), own=True)


def act_none():
    _step(_layer(bn=False, act="none", alpha=0.0), _x(), own=True)


def image_conv():
    _step(_layer(cin=3, bn=False), _x(C=3, nhwc=False), own=True)


def image_conv_bias():
    _step(_layer(cin=3, bn=False, bias=True), _x(C=3, nhwc=False), own=True)


def image_convt():
    _step(_layer(cin=16, cout=3, bn=False, act="tanh", alpha=0.0, transposed=True, nchw_out=True), _x(), own=True)


def _g1(own):
    layer = _layer(cin=64, cout=16, k=4, s=1, p=0, act="relu", alpha=0.0, transposed=True)
    _step(layer, _x(32, 64, 1, 1, nhwc=False, grad=False), own=own)


def g1_own_grad():
    _g1(True)


def g1_autograd_grad():
    _g1(False)


def spectral_own_grad_set_then_accumulate():
    layer, x = _layer(bn=False, spectral=True), _x()
    _step(layer, x, own=True)
    assert layer.conv.weight_orig.grad is not None
    _step(layer, x, own=True)


def spectral_autograd_grad():
    _step(_layer(bn=False, spectral=True), _x(), own=False)


def nn_conv():
    _step(_layer(k=3, s=1, p=1, act="relu", alpha=0.0, bias=True, upsample=2), _x(), own=True)


def _chain(lower_bn, links=True):
    """16 -> 32 -> 64 from 16x16 as a two-layer nets._Net call."""
    from relativisticgan_amd import autograd as AG
    from relativisticgan_amd import nets

    class _DChain(nets._Net):
        def __init__(self):
            super().__init__()
            self._plan = [_layer(16, 32, bn=lower_bn), _layer(32, 64)]

    net = _DChain()
    prev, AG.LINKS = AG.LINKS, links
    try:
        a = net._run(_x(H=16, W=16))
        with AG.owning_grads():
            a.backward(torch.randn_like(a))
    finally:
        AG.LINKS = prev


def chain_bn_post2():
    _chain(True)


def chain_act_post1():
    _chain(False)


def chain_bn_links_off():
    _chain(True, links=False)


def da_not_nhwc():
    _step(_layer(), _x(), own=True, da=lambda a: torch.randn(a.shape, device=DEV))


def eval_mode():
    layer = _layer()
    a = layer.run(_x(), False)
    with pytest.raises(NotImplementedError):
        a.backward(torch.randn_like(a))


CASES = (own_grad_set_then_accumulate, autograd_grad, autograd_grad_bias, segs2, segs2_gsegs1, act_only, act_none,
         image_conv, image_conv_bias, image_convt, g1_own_grad, g1_autograd_grad,
         spectral_own_grad_set_then_accumulate, spectral_autograd_grad, nn_conv, chain_bn_post2, chain_act_post1,
         chain_bn_links_off, da_not_nhwc, eval_mode)


def record(case):
    """The call rows of one case, from empty weight caches (so the packs are part of them)."""
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd.abi_record import Recorder
    for cache in (K.PACKS, K.FOLDS, K.PATCHW):
        cache.clear()
    torch.manual_seed(0)
    with Recorder() as rec:
        case()
        torch.cuda.synchronize()
    return rec.rows


def write_fixture():
    rows = {case.__name__: record(case) for case in CASES}
    with open(FIXTURE, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_layer_call_rows(case):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(c.__name__ for c in CASES)
    got = record(case)
    assert got == want[case.__name__], "\n".join(["got:"] + got + ["want:"] + want[case.__name__])


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    else:
        sys.exit("usage: python -m tests.test_layer_calls_gpu --write")
