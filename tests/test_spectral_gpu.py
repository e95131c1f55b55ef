"""The spectral-norm kernels of csrc/heads_optim.hip (rgan_spectral_power, _power_batch,
_backward) on every layout branch and loop pass against float64 (tests/spectral_ref.py, which
tests/test_spectral_ref_cpu.py pins to torch.nn.utils.spectral_norm), and the nets' spectral
path (gradient accumulation over two calls, eval mode) against the oracle's modules in float64.

Shapes: spectral_ref.TABLE, one table for the power and the backward tests, each row the
smallest weight that reaches its branch (named beside it there).

Tolerance: rel-L2 <= 1e-5 against float64 for u, v and dW, relative 1e-5 for sigma -- or, where
fp32 itself cannot do better, 4x the error of torch's own fp32 CPU evaluation of the same
formula against float64 (computed here, never taken from the kernel).  Outputs the test
allocates lie between 64-float guard bands that must come back bit-unchanged.

With RGAN_SPECTRAL_REPORT=<file> the worst error per test is appended to that file
(profiles/spectral_mi355x.txt).
"""
import copy
import ctypes
import os

import pytest
import torch

from tests import spectral_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
GUARD = 64
SENTINEL = 12345.0
IDS = [S.case_id(c) for c in S.TABLE]
# one row per branch of sn_bwd_kernel: lo == 16 float4 (Conv2d and ConvTranspose2d), generic
# strided float4, flat float4, scalar (flat-indexed rows do not exist in the scalar branch:
# 3x3 dim 0, 3x3 dim 1, 2-D), rows == 1 and the largest
ACC_ROWS = [((16, 24, 4, 4), False), ((72, 5, 4, 4), True), ((6, 5, 2, 2), True), ((260, 2, 2, 2), True),
            ((3, 1, 4, 2080), False), ((96, 21, 3, 3), False), ((7, 5, 3, 3), True), ((10, 37), False),
            ((4, 30, 3, 3), False), ((1, 300, 4, 4), False), ((512, 256, 4, 4), False)]
ALIGN_ROWS = [((16, 24, 4, 4), False), ((72, 5, 4, 4), True)]
_WORST = {}  # test -> {quantity: worst error}
_REFS = {}


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("RGAN_SPECTRAL_REPORT")
    if path and _WORST:
        with open(path, "a") as fh:
            for test, w in sorted(_WORST.items()):
                fh.write("%-34s %s\n" % (test, "   ".join("%s %.2e" % kv for kv in sorted(w.items()))))


def _close(test, what, got, ref64, ref32, where, tol=TOL, extra=0.0):
    """rel-L2(got, ref64) <= max(tol, 4 x torch's fp32 error) + extra; the figure is noted."""
    e, e32 = S.rel(got, ref64), S.rel(ref32, ref64)
    w = _WORST.setdefault(test, {})
    w[what] = max(w.get(what, 0.0), e)
    print(f"{test} {where} {what}: {e:.2e} (torch fp32 {e32:.2e})")
    assert e == e and e <= max(tol, 4 * e32) + extra, f"{test} {where} {what}: {e:.2e} vs fp64 (torch fp32: {e32:.2e})"


def _sigma_close(test, inv_sigma, sig64, sig32, where):
    got = 1.0 / inv_sigma.double().cpu()
    _close(test, "sigma", got, sig64.reshape(1), sig32.reshape(1), where)


def _guarded(t, offset=0):
    """A device copy of the CPU tensor ``t`` inside a larger sentinel-filled buffer, GUARD
    (+ offset) floats from its start: (buffer, view).  offset = 1 puts the view 4 bytes off
    the 16-byte alignment the float4 branches need."""
    n = t.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_(t.reshape(-1))
    return buf, view.view(t.shape)


def _intact(buf, view, where):
    start = (view.data_ptr() - buf.data_ptr()) // 4
    n = view.numel()
    assert bool((buf[:start] == SENTINEL).all()) and bool((buf[start + n:] == SENTINEL).all()), \
        f"{where}: a guard band was written"


def _power_refs(case, eps):
    """[(u, v, sigma)] after one and two calls, in float64 and in torch fp32."""
    key = ("power", case, eps)
    if key not in _REFS:
        a = S.inputs(case)
        out = {}
        for dt in (torch.float64, torch.float32):
            W, u, v, chain = a["W"].to(dt), a["u"], a["v"], []
            for call in range(2):
                u, v, sigma = S.power(W, u, v, a["transposed"], eps=eps)
                chain.append((u, v, sigma))
            out[dt] = chain
        _REFS[key] = out
    return _REFS[key][torch.float64], _REFS[key][torch.float32]


def _bwd_inputs(case):
    """The (u, v, 1 / sigma) a backward call gets: the float64 power iteration's, rounded to
    fp32 -- the references then start from these very numbers."""
    key = ("bwd_in", case)
    if key not in _REFS:
        u, v, sigma = _power_refs(case, S.EPS)[0][0]
        _REFS[key] = (u.float(), v.float(), (1.0 / sigma).float().reshape(1))
    return _REFS[key]


def _bwd_refs(case, which):
    key = ("bwd", case, which)
    if key not in _REFS:
        a = S.inputs(case)
        u, v, inv = _bwd_inputs(case)
        out = {}
        for dt in (torch.float64, torch.float32):
            sigma = 1.0 / inv.to(dt)[0]
            out[dt] = S.backward(a["W"].to(dt), a[which], u, v, sigma, a["transposed"])
        _REFS[key] = out
    return _REFS[key][torch.float64], _REFS[key][torch.float32]


def _batch_raw(K, layers, eps):
    """rgan_spectral_power_batch with copies the caller allocated (kernels.spectral_power_batch
    allocates them itself): layers of (w, u, v, transposed, u_copy, v_copy, inv_sigma)."""
    from relativisticgan_amd import _lib as L
    arr = (L.RganSnLayer * len(layers))()
    for i, (w, u, v, tr, uc, vc, inv) in enumerate(layers):
        rows, cols, rs, hs, lo = K.sn_view(w, tr)
        arr[i] = L.RganSnLayer(w.data_ptr(), rows, cols, lo, rs, hs, u.data_ptr(), v.data_ptr(), uc.data_ptr(),
                               vc.data_ptr(), inv.data_ptr())
    lib = L.lib()
    p = ctypes.cast(arr, ctypes.c_void_p)
    ws = L.workspace(lib.rgan_spectral_batch_ws_bytes(len(layers), p), DEV)
    L.check(lib.rgan_spectral_power_batch(len(layers), p, float(eps), L.ptr(ws), L.stream()), "rgan_spectral_power_batch")


# ------------------------------------------------------------------ power iteration
@pytest.mark.parametrize("eps", [S.EPS, S.EPS_CLAMP], ids=["eps1e-12", "clamp"])
@pytest.mark.parametrize("case", S.TABLE, ids=IDS)
def test_power_single(K, case, eps):
    """rgan_spectral_power, train mode: two calls, the second from the first's u, v."""
    test = "power_single" + ("_clamp" if eps == S.EPS_CLAMP else "")
    a = S.inputs(case)
    w = a["W"].to(DEV)
    ubuf, u = _guarded(a["u"])
    vbuf, v = _guarded(a["v"])
    r64, r32 = _power_refs(case, eps)
    for call in range(2):
        inv = K.spectral_power(w, u, v, a["transposed"], eps=eps)
        where = f"{S.case_id(case)} call {call}"
        _close(test, "u", u, r64[call][0], r32[call][0], where)
        _close(test, "v", v, r64[call][1], r32[call][1], where)
        _sigma_close(test, inv, r64[call][2], r32[call][2], where)
        _intact(ubuf, u, where + " u")
        _intact(vbuf, v, where + " v")
    assert torch.equal(w.cpu(), a["W"])


@pytest.mark.parametrize("eps", [S.EPS, S.EPS_CLAMP], ids=["eps1e-12", "clamp"])
def test_power_batch(K, eps):
    """rgan_spectral_power_batch over every row of the table in one call (its limit of 16 layers),
    twice; the returned copies are bit-equal to the buffers."""
    test = "power_batch" + ("_clamp" if eps == S.EPS_CLAMP else "")
    assert len(S.TABLE) <= 16
    ins = [S.inputs(c) for c in S.TABLE]
    bufs = [(_guarded(a["u"]), _guarded(a["v"])) for a in ins]
    layers = [(a["W"].to(DEV), ub[1], vb[1], a["transposed"]) for a, (ub, vb) in zip(ins, bufs)]
    for call in range(2):
        outs = K.spectral_power_batch(layers, eps=eps)
        torch.cuda.synchronize()
        for case, (w, u, v, tr), (uc, vc, inv), (ub, vb) in zip(S.TABLE, layers, outs, bufs):
            r64, r32 = _power_refs(case, eps)
            where = f"{S.case_id(case)} call {call}"
            _close(test, "u", u, r64[call][0], r32[call][0], where)
            _close(test, "v", v, r64[call][1], r32[call][1], where)
            _sigma_close(test, inv, r64[call][2], r32[call][2], where)
            assert torch.equal(uc, u) and torch.equal(vc, v), where
            _intact(*ub, where + " u")
            _intact(*vb, where + " v")
    for a, (w, _, _, _) in zip(ins, layers):
        assert torch.equal(w.cpu(), a["W"])


def test_power_batch_guarded_copies_and_offset_weight(K):
    """The batched call with its autograd copies between guard bands, and with every W an
    offset (4 bytes off 16-byte alignment: the scalar branches) view into a larger buffer:
    the aligned run's result, the copies bit-equal to the buffers, no guard touched."""
    test = "power_batch_offset_w"
    ins = [S.inputs(c) for c in S.TABLE]
    for offset in (0, 1):
        bands, layers = [], []
        for a in ins:
            g = [_guarded(a["u"]), _guarded(a["v"]), _guarded(torch.zeros_like(a["u"])),
                 _guarded(torch.zeros_like(a["v"])), _guarded(torch.zeros(1)), _guarded(a["W"], offset)]
            bands.append(g)
            layers.append((g[5][1], g[0][1], g[1][1], a["transposed"], g[2][1], g[3][1], g[4][1]))
        _batch_raw(K, layers, S.EPS)
        torch.cuda.synchronize()
        for case, (w, u, v, tr, uc, vc, inv), g, a in zip(S.TABLE, layers, bands, ins):
            r64, r32 = _power_refs(case, S.EPS)
            where = f"{S.case_id(case)} W offset {offset}"
            assert w.data_ptr() % 16 == 4 * offset
            _close(test, "u", u, r64[0][0], r32[0][0], where)
            _close(test, "v", v, r64[0][1], r32[0][1], where)
            _sigma_close(test, inv, r64[0][2], r32[0][2], where)
            assert torch.equal(uc, u) and torch.equal(vc, v), where
            assert torch.equal(w.cpu(), a["W"]), where
            for buf, view in g:
                _intact(buf, view, where)


@pytest.mark.parametrize("case", S.TABLE, ids=IDS)
def test_power_eval_mode(K, case):
    """do_iter = 0: u and v (random unit vectors unrelated to W, so a kernel that recomputes
    one or reads the wrong one gives another sigma) stay bit-identical, sigma = u . W v."""
    test = "power_eval"
    a = S.inputs(case)
    w = a["W"].to(DEV)
    ubuf, u = _guarded(a["u"])
    vbuf, v = _guarded(a["v"])
    inv = K.spectral_power(w, u, v, a["transposed"], do_iter=False)
    torch.cuda.synchronize()
    assert torch.equal(u.cpu(), a["u"]) and torch.equal(v.cpu(), a["v"])
    _intact(ubuf, u, "u")
    _intact(vbuf, v, "v")
    s64 = S.power(a["W"].double(), a["u"], a["v"], a["transposed"], do_iter=False)[2]
    s32 = S.power(a["W"], a["u"], a["v"], a["transposed"], do_iter=False)[2]
    _sigma_close(test, inv, s64, s32, S.case_id(case))
    # the train-mode sigma of the same inputs is far away: the comparison above can tell
    s_train = _power_refs(case, S.EPS)[0][0][2]
    assert abs(s64.item() - s_train.item()) > 0.1 * s_train.item()


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("which", ["G_rand", "G_aligned"])
@pytest.mark.parametrize("case", S.TABLE, ids=IDS)
def test_backward(K, case, which):
    """dW = G / sigma - (<G, W> / sigma^2) u v^T for a random upstream gradient and for one
    aligned with W, where the rank-one correction is about as large as dW and is compared on
    its own as well.  Accumulating into zeros between guard bands gives the same bits."""
    test = "backward_" + which[2:]
    a = S.inputs(case)
    tr = a["transposed"]
    u32, v32, inv32 = _bwd_inputs(case)
    w, G = a["W"].to(DEV), a[which].to(DEV)
    u, v, inv = u32.to(DEV), v32.to(DEV), inv32.to(DEV)
    (dW64, corr64), (dW32, corr32) = _bwd_refs(case, which)
    where = S.case_id(case)
    dw = K.spectral_backward(w, G, u, v, inv, tr)
    _close(test, "dW", dw, dW64, dW32, where)
    if which == "G_aligned":
        sigma = 1.0 / inv32.double()[0]
        G64 = a[which].double()
        _close(test, "correction", dw.double().cpu() - G64 / sigma, corr64, dW32.double() - G64 / sigma, where)
    obuf, out = _guarded(torch.zeros_like(a["W"]))
    res = K.spectral_backward(w, G, u, v, inv, tr, out=out)
    torch.cuda.synchronize()
    # (0 + dW: the same value, up to one rounding where the compiler contracts the two forms
    # of the expression differently)
    assert res is out and S.rel(out, dw) <= 2.0 ** -23, where
    _intact(obuf, out, where)
    for t, t0 in ((w, a["W"]), (G, a[which]), (u, u32), (v, v32), (inv, inv32)):
        assert torch.equal(t.cpu(), t0), where


@pytest.mark.parametrize("case", ACC_ROWS, ids=[S.case_id(c) for c in ACC_ROWS])
def test_backward_accumulate(K, case):
    """accumulate = 1 adds dW into a random base of dW's size: out - base is dW to the
    tolerance plus one rounding of the sum, 2^-23 ||base|| / ||dW||."""
    test = "backward_accumulate"
    assert case in S.TABLE
    a = S.inputs(case)
    u32, v32, inv32 = _bwd_inputs(case)
    (dW64, _), (dW32, _) = _bwd_refs(case, "G_aligned")
    g = torch.Generator().manual_seed(77)
    base = (torch.randn(a["W"].shape, generator=g, dtype=torch.float64) * dW64.std()).float()
    obuf, out = _guarded(base)
    K.spectral_backward(a["W"].to(DEV), a["G_aligned"].to(DEV), u32.to(DEV), v32.to(DEV), inv32.to(DEV),
                        a["transposed"], out=out)
    torch.cuda.synchronize()
    extra = 2.0 ** -23 * (base.double().norm() / dW64.norm()).item()
    _close(test, "dW", out.double().cpu() - base.double(), dW64, dW32, S.case_id(case), extra=extra)
    _intact(obuf, out, S.case_id(case))


@pytest.mark.parametrize("mis", ["v", "dw_eff", "out", "w"])
@pytest.mark.parametrize("case", ALIGN_ROWS, ids=[S.case_id(c) for c in ALIGN_ROWS])
def test_backward_misaligned(K, case, mis):
    """v, dw_eff, out or W four bytes off 16-byte alignment inside a larger buffer (the kernels
    must leave their float4 branches): the aligned run's result to tolerance, guards intact."""
    test = "backward_misaligned"
    a = S.inputs(case)
    u32, v32, inv32 = _bwd_inputs(case)
    (dW64, _), (dW32, _) = _bwd_refs(case, "G_aligned")
    g = torch.Generator().manual_seed(78)
    base = (torch.randn(a["W"].shape, generator=g, dtype=torch.float64) * dW64.std()).float()
    t = {"v": v32, "dw_eff": a["G_aligned"], "out": base, "w": a["W"]}
    runs = {}
    for offset in (0, 1):
        bands = {k: _guarded(x, offset if k == mis else 0) for k, x in t.items()}
        assert bands[mis][1].data_ptr() % 16 == 4 * offset
        K.spectral_backward(bands["w"][1], bands["dw_eff"][1], u32.to(DEV), bands["v"][1], inv32.to(DEV),
                            a["transposed"], out=bands["out"][1])
        torch.cuda.synchronize()
        for k, (buf, view) in bands.items():
            _intact(buf, view, f"{S.case_id(case)} {mis} offset {offset}: {k}")
            if k != "out":
                assert torch.equal(view.cpu(), t[k])
        runs[offset] = bands["out"][1].double().cpu() - base.double()
    extra = 2.0 ** -23 * (base.double().norm() / dW64.norm()).item()
    _close(test, "dW", runs[1], dW64, dW32, f"{S.case_id(case)} {mis}", extra=extra)
    _close(test, "vs aligned", runs[1], runs[0], runs[0], f"{S.case_id(case)} {mis}", extra=2 * extra)


@pytest.mark.parametrize("mis", ["u", "v"])
@pytest.mark.parametrize("case", ALIGN_ROWS, ids=[S.case_id(c) for c in ALIGN_ROWS])
def test_power_misaligned_buffers(K, case, mis):
    """u or v four bytes off 16-byte alignment, single and batched: the aligned result."""
    test = "power_misaligned"
    a = S.inputs(case)
    r64, r32 = _power_refs(case, S.EPS)
    for batched in (False, True):
        ubuf, u = _guarded(a["u"], int(mis == "u"))
        vbuf, v = _guarded(a["v"], int(mis == "v"))
        w = a["W"].to(DEV)
        if batched:
            inv = K.spectral_power_batch([(w, u, v, a["transposed"])])[0][2]
        else:
            inv = K.spectral_power(w, u, v, a["transposed"])
        torch.cuda.synchronize()
        where = f"{S.case_id(case)} {mis} batched {batched}"
        _close(test, "u", u, r64[0][0], r32[0][0], where)
        _close(test, "v", v, r64[0][1], r32[0][1], where)
        _sigma_close(test, inv, r64[0][2], r32[0][2], where)
        _intact(ubuf, u, where)
        _intact(vbuf, v, where)


# ------------------------------------------------------------------ the nets' spectral path
# batch 2: arch 1 has fixed widths, and the fewer activations a case has, the further its
# nearest pre-activation can be kept from the ReLU / LeakyReLU kink (KINK_MARGIN below)
NET_CASES = {
    "arch0_D": dict(arch=0, image_size=32, batch_size=2, z_size=16, G_h_size=8, D_h_size=8, loss_D=8, spectral=True),
    "arch1_D": dict(arch=1, image_size=32, batch_size=2, z_size=16, loss_D=8, spectral=True, spectral_G=True),
    "arch1_G": dict(arch=1, image_size=32, batch_size=2, z_size=16, loss_D=8, spectral=True, spectral_G=True),
}
# Seeds at which no pre-activation of the two train-mode calls lies within KINK_MARGIN (in units
# of its layer's rms) of 0 in float64.  fp32 pre-activations are within about 1e-6 rms of
# float64's (the outputs' measured rel-L2 is 2e-7 - 6e-7), so no fp32 evaluation flips an
# activation's derivative there; one flip alone moves a weight gradient by about 1e-3.
NET_SEEDS = {"arch0_D": 21, "arch1_D": 105, "arch1_G": 90}
KINK_MARGIN = 8e-6


def _nets(name):
    """(ours on the GPU, the oracle's module in fp32, in fp64, an input maker) of one state."""
    from oracle.reference_cpu import build_D, build_G, make_param as oparam, weights_init as owi
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_D, DCGAN_G
    case = NET_CASES[name]
    is_D = name.endswith("_D")
    net = (DCGAN_D if is_D else DCGAN_G)(make_param(**case))  # (its own draws: before the seed)
    torch.manual_seed(NET_SEEDS[name])
    o32 = (build_D if is_D else build_G)(oparam(cuda=False, **case))
    o32.apply(owi)
    if is_D:
        make = lambda: torch.rand(case["batch_size"], 3, 32, 32) * 2 - 1  # noqa: E731
    else:
        make = lambda: torch.randn(case["batch_size"], case["z_size"], 1, 1)  # noqa: E731
    net.load_state_dict(o32.state_dict())
    net.to(DEV)
    return net, o32, copy.deepcopy(o32).double(), make


def _uv(net):
    return {n: b.detach().clone() for n, b in net.named_buffers() if n.endswith(("weight_u", "weight_v"))}


def _uv_close(test, net, o32, o64, where):
    d32, d64 = dict(o32.named_buffers()), dict(o64.named_buffers())
    names = list(_uv(net))
    assert names and sorted(names) == sorted(n for n in d64 if n.endswith(("weight_u", "weight_v")))
    for n, b in net.named_buffers():
        if n in names:
            _close(test, "u, v", b, d64[n], d32[n], f"{where} {n}")


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_net_two_calls_then_backward(name):
    """Two train-mode calls (each its own power iteration and sigma), then the backward of
    both: weight_orig.grad is the float64 sum of the two calls' gradients (the accumulate
    path into .grad), u and v are the buffers after two iterations."""
    test = "net_two_calls"
    net, o32, o64, make = _nets(name)
    x1, x2 = make(), make()
    pre = []
    hooks = [m.register_forward_pre_hook(lambda mod, i: pre.append(i[0].detach().clone())) for m in o64.modules()
             if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU, torch.nn.SELU))]
    outs = []
    for m, cast in ((net, lambda t: t.to(DEV)), (o32, lambda t: t), (o64, lambda t: t.double())):
        m.train()
        y1, y2 = m(cast(x1)), m(cast(x2))
        outs.append((y1, y2))
    for h in hooks:
        h.remove()
    margin = min((t.abs().min() / t.pow(2).mean().sqrt()).item() for t in pre)
    assert len(pre) >= 6 and margin >= KINK_MARGIN, f"input condition: a pre-activation {margin:.1e} rms from the kink"
    for k in range(2):
        _close(test, "out", outs[0][k], outs[2][k], outs[1][k], f"{name} call {k}", tol=2e-5)
    _uv_close(test, net, o32, o64, name)
    g = torch.Generator().manual_seed(5)
    g1 = torch.randn(outs[2][0].shape, generator=g)
    g2 = torch.randn(outs[2][1].shape, generator=g)
    for (y1, y2), cast in zip(outs, (lambda t: t.to(DEV), lambda t: t, lambda t: t.double())):
        torch.autograd.backward([y1, y2], [cast(g1).reshape(y1.shape), cast(g2).reshape(y2.shape)])
    torch.cuda.synchronize()
    q32, q64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    seen = 0
    for n, q in net.named_parameters():
        if n.endswith("weight_orig"):
            _close(test, "weight_orig.grad", q.grad, q64[n].grad, q32[n].grad, f"{name} {n}", tol=2e-5)
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_net_eval_mode(name):
    """After one train-mode call: .eval() runs no power iteration (u, v bit-unchanged, sigma
    from them: the single-layer do_iter = 0 kernels), the output is float64's; back in
    .train() the buffers move again and match float64."""
    test = "net_eval"
    net, o32, o64, make = _nets(name)
    x0, x1, x2 = make(), make(), make()
    casts = (lambda t: t.to(DEV), lambda t: t, lambda t: t.double())
    ys = []
    for m, cast in zip((net, o32, o64), casts):
        m.train()
        with torch.no_grad():
            m(cast(x0))
        m.eval()
    before = _uv(net)
    for m, cast in zip((net, o32, o64), casts):
        with torch.no_grad():
            ys.append(m(cast(x1)))
    torch.cuda.synchronize()
    _close(test, "out", ys[0], ys[2], ys[1], f"{name} eval", tol=2e-5)
    after = _uv(net)
    assert all(torch.equal(before[n], after[n]) for n in before), "eval mode moved u or v"
    _uv_close(test, net, o32, o64, f"{name} eval")
    ys = []
    for m, cast in zip((net, o32, o64), casts):
        m.train()
        with torch.no_grad():
            ys.append(m(cast(x2)))
    torch.cuda.synchronize()
    _close(test, "out", ys[0], ys[2], ys[1], f"{name} train again", tol=2e-5)
    moved = _uv(net)
    # (a one-row layer -- arch 0's end conv -- has u = +-1 and v = +-W / ||W|| from the first call on)
    one_row = {n[:-1] for n in before if n.endswith("weight_u") and before[n].numel() == 1}
    assert all(not torch.equal(before[n], moved[n]) for n in before if n[:-1] not in one_row), "train mode left u or v"
    _uv_close(test, net, o32, o64, f"{name} train again")
