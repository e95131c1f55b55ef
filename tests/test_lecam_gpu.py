"""--rgan_lecam on the MI355X: the fused kernel, its partial-sums mode and the finish kernel
(csrc/lecam.hip) against the float64 restatement (tests/lecam_ref.py), the wrappers and rgan::
operators, graph capture, and the term through the training step: one iteration against an exact
float64 step, a free-running trajectory, launch accounting, checkpoints, data parallelism, the CLI.

Bounds.  The term and the anchors are double sums of n terms added in another order than numpy's:
at most n * 2^-53 relative to the sum of the absolute terms (1.2e-13 at n = 1025), asserted as
1e-12.  A gradient element is formed in double and rounded once: within 1 fp32 ulp of the
restated float64 value rounded to fp32.  The training step is held to tests/test_parity_gpu.py's
TOL_OUT / TOL_GRAD / TOL_BUF against the exact step.
"""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import lecam_ref as ref
from tests.test_diffaug_gpu import _Counter
from tests.test_ema_gpu import TINY_CLI, _cut
from tests.test_parity_gpu import TOL_BUF, TOL_GRAD, TOL_OUT, _rel
from tests.test_r1r2_gpu import POLICY, STEP, _step_feed, _zc64

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_TOL = 1e-12

LAM, BETA, START = 0.3, 0.9, 3
A_REAL, A_FAKE = 0.25, -0.5
NS = (1, 63, 64, 65, 255, 256, 257, 1025)
SHAPES = ("both", "real", "fake")
CALLS = (0, START - 1, START, START + 2)  # the initialisation, below, at and above the start


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _hyper(lam=LAM, beta=BETA, start=START):
    return torch.tensor([lam, beta, float(start), 0.0], dtype=torch.float64, device=DEV)


def _state(calls, a_real=A_REAL, a_fake=A_FAKE):
    return torch.tensor([a_real, a_fake, float(calls), 0.0], dtype=torch.float64, device=DEV)


_VALUES = {}


def _values(n):
    """(y_real, y_fake) of n rows, fp32 on the host: D-like outputs around +0.7 and -0.4."""
    if n not in _VALUES:
        gen = torch.Generator().manual_seed(77 + n)
        _VALUES[n] = (torch.randn(n, generator=gen) + 0.7, torch.randn(n, generator=gen) * 1.5 - 0.4)
    return _VALUES[n]


def _ulps(got, want64):
    """|got - fl32(want)| in units of fl32(want)'s ulp, elementwise (numpy)."""
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _sum_errors(c0, c1, L, got_L, got_state, yr, yf, n_global, real, fake):
    """The three double results against the restatement ``c1`` (already stepped from ``c0``), each
    relative to the sum of the absolute terms behind it."""
    N = float(n_global)
    a = ref.abs_sums(yr if real else None, yf if fake else None, c0.a_real, c0.a_fake)
    first = c0.calls == 0
    errs = {}
    scale_L = c0.weight() * (a[2] + a[3]) / N
    errs["L"] = abs(got_L - L) / scale_L if scale_L > 0 else abs(got_L - L)
    for k, name, on in ((0, "a_real", real), (1, "a_fake", fake)):
        old = (c0.a_real, c0.a_fake)[k]
        if not on:
            assert got_state[k] == old  # an absent side's anchor is not touched
            continue
        scale = a[k] / N if first else BETA * abs(old) + (1 - BETA) * a[k] / N
        errs[name] = abs(got_state[k] - c1.state[k]) / scale
    assert got_state[2] == c1.state[2] == c0.calls + (1 if fake else 0) and got_state[3] == 0.0
    return errs


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("n", NS)
def test_kernel_matches_restatement(n):
    from relativisticgan_amd import kernels as K
    vr, vf = _values(n)
    hyper = _hyper()
    worst = {"L": 0.0, "a_real": 0.0, "a_fake": 0.0, "ulp": 0.0}
    for misaligned in (False, True):
        rbuf, yr, lead = _cut(vr.to(DEV), misaligned)
        fbuf, yf, _ = _cut(vf.to(DEV), misaligned)
        for n_global in (n, 2 * n):
            for shape in SHAPES:
                real, fake = shape != "fake", shape != "real"
                for calls in CALLS:
                    c0 = ref.LeCam(LAM, BETA, START, A_REAL, A_FAKE, calls)
                    c1 = ref.LeCam(LAM, BETA, START, A_REAL, A_FAKE, calls)
                    L, gr, gf = c1.step(vr.numpy() if real else None, vf.numpy() if fake else None, n_global)
                    runs = []
                    for _ in range(2):  # the same state twice: the same bits
                        state = _state(calls)
                        drbuf, dr, _ = _cut(torch.full((n,), 7.0), misaligned)
                        dfbuf, df, _ = _cut(torch.full((n,), 7.0), misaligned)
                        out, o_dr, o_df = K.lecam(yr if real else None, yf if fake else None, hyper, state,
                                                  n_global, dr=dr if real else None, df=df if fake else None)
                        assert (o_dr is None) == (not real) and (o_df is None) == (not fake)
                        assert not real or o_dr.data_ptr() == dr.data_ptr()
                        assert not fake or o_df.data_ptr() == df.data_ptr()
                        for buf in (drbuf, dfbuf):  # guards stay NaN
                            assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + n:]).all()
                        # an absent side's buffer is not written
                        assert real or (dr == 7.0).all()
                        assert fake or (df == 7.0).all()
                        runs.append((out.clone(), dr.clone(), df.clone(), state.clone()))
                    for a, b in zip(*runs):
                        assert torch.equal(_bits(a), _bits(b)), (n, misaligned, n_global, shape, calls)
                    out, dr, df, state = runs[0]
                    assert out[1:].tolist() == [0.0, 0.0, 0.0]
                    errs = _sum_errors(c0, c1, L, out[0].item(), state.tolist(), vr.numpy(), vf.numpy(), n_global,
                                       real, fake)
                    for k, e in errs.items():
                        worst[k] = max(worst[k], e)
                        assert e <= SUM_TOL, (n, misaligned, n_global, shape, calls, k, e)
                    for on, got, want in ((real, dr, gr), (fake, df, gf)):
                        if not on:
                            continue
                        if c0.weight() == 0:  # exact zeros, and the anchors moved all the same
                            assert (got == 0).all() and out[0].item() == 0.0
                            continue
                        u = _ulps(got.cpu().numpy(), want).max()
                        worst["ulp"] = max(worst["ulp"], u)
                        assert u <= 1.0, (n, misaligned, n_global, shape, calls, u)
                    if c0.weight() == 0:
                        assert state.tolist()[:2] != [A_REAL, A_FAKE]
                    else:
                        assert out[0].item() > 0
        # inputs untouched, their guards too
        for buf, y, v in ((rbuf, yr, vr), (fbuf, yf, vf)):
            assert torch.equal(_bits(y), _bits(v.to(DEV)))
            assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + n:]).all()
    print(f"lecam n={n}: worst rel err L {worst['L']:.2e} a_real {worst['a_real']:.2e} a_fake {worst['a_fake']:.2e}; "
          f"worst gradient error {worst['ulp']:.2f} ulp")


def test_no_gradient_wanted_and_fresh_buffers():
    from relativisticgan_amd import kernels as K
    vr, vf = _values(257)
    yr, yf = vr.to(DEV), vf.to(DEV)
    want, w_dr, w_df = K.lecam(yr, yf, _hyper(), _state(5))
    assert w_dr.shape == yr.shape and w_df.dtype == torch.float32
    out, dr, df = K.lecam(yr, yf, _hyper(), _state(5), need_dr=False, need_df=False)
    assert dr is None and df is None and torch.equal(_bits(out), _bits(want))
    out, dr, df = K.lecam(yr, yf, _hyper(), _state(5), need_dr=False)
    assert dr is None and torch.equal(_bits(df), _bits(w_df))


# ---------------------------------------------------------------- 2. shards add up
@pytest.mark.parametrize("n, cut", [(2, 1), (130, 65), (1025, 300)])
@pytest.mark.parametrize("shape", SHAPES)
def test_shards_add_up(n, cut, shape):
    from relativisticgan_amd import kernels as K
    real, fake = shape != "fake", shape != "real"
    vr, vf = _values(n)
    yr, yf = vr.to(DEV), vf.to(DEV)
    hyper = _hyper()
    for calls in (0, START + 2):
        whole = _state(calls)
        w_out, w_dr, w_df = K.lecam(yr if real else None, yf if fake else None, hyper, whole)
        state = _state(calls)
        sums, drs, dfs = torch.zeros(4, dtype=torch.float64), [], []
        for lo, hi in ((0, cut), (cut, n)):
            part, dr, df = K.lecam(yr[lo:hi] if real else None, yf[lo:hi] if fake else None, hyper, state, n,
                                   partial=True)
            assert state.tolist() == _state(calls).tolist()  # the partial mode leaves the state alone
            # ... and its sums are the restatement's of that shard
            want = ref.shard_sums(vr[lo:hi].numpy() if real else None, vf[lo:hi].numpy() if fake else None,
                                  A_REAL, A_FAKE)
            scale = ref.abs_sums(vr[lo:hi].numpy() if real else None, vf[lo:hi].numpy() if fake else None,
                                 A_REAL, A_FAKE)
            for k in range(4):
                assert abs(part[k].item() - want[k]) <= SUM_TOL * scale[k], (k, part.tolist(), want)
            sums += part.cpu()  # summed on the host, as the all-reduce sums the ranks'
            drs.append(dr), dfs.append(df)
        loss = K.lecam_finish(sums.to(DEV), n, (1 if real else 0) | (2 if fake else 0), hyper, state)
        # gradients bit for bit, the double results within the reordering bound
        if real:
            assert torch.equal(_bits(torch.cat(drs)), _bits(w_dr))
        if fake:
            assert torch.equal(_bits(torch.cat(dfs)), _bits(w_df))
        c0 = ref.LeCam(LAM, BETA, START, A_REAL, A_FAKE, calls)
        c1 = ref.LeCam(LAM, BETA, START, A_REAL, A_FAKE, calls)
        L, _, _ = c1.step(vr.numpy() if real else None, vf.numpy() if fake else None)
        for got_L, got_state in ((loss[0].item(), state.tolist()), (w_out[0].item(), whole.tolist())):
            errs = _sum_errors(c0, c1, L, got_L, got_state, vr.numpy(), vf.numpy(), n, real, fake)
            assert all(e <= SUM_TOL for e in errs.values()), (n, shape, calls, errs)
        a = ref.abs_sums(vr.numpy() if real else None, vf.numpy() if fake else None, A_REAL, A_FAKE)
        scale_L = c0.weight() * (a[2] + a[3]) / n
        assert abs(loss[0].item() - w_out[0].item()) <= SUM_TOL * scale_L
        for k in (0, 1):
            assert abs(state[k].item() - whole[k].item()) <= SUM_TOL * max(abs(whole[k].item()), a[k] / n)


# ---------------------------------------------------------------- 3. wrappers and operators
def test_wrapper_rejects_bad_arguments():
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import kernels as K
    y, z = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    two = torch.zeros(8, 2, device=DEV)
    hyper, state = _hyper(), _state(5)
    d4 = torch.zeros(4, dtype=torch.float64, device=DEV)
    bad = {
        "cpu y_real": dict(y_real=y.cpu(), y_fake=z),
        "cpu y_fake": dict(y_real=y, y_fake=z.cpu()),
        "cpu state": dict(y_real=y, y_fake=z, state=state.cpu()),
        "cpu hyper": dict(y_real=y, y_fake=z, hyper=hyper.cpu()),
        "transposed view": dict(y_real=two.t()[0], y_fake=z),
        "strided gradient": dict(y_real=y, y_fake=z, dr=two.t()[0]),
        "float64 y": dict(y_real=y.double(), y_fake=z),
        "float32 state": dict(y_real=y, y_fake=z, state=state.float()),
        "short hyper": dict(y_real=y, y_fake=z, hyper=hyper[:3]),
        "lengths differ": dict(y_real=y, y_fake=z[:7]),
        "short gradient buffer": dict(y_real=y, y_fake=z, dr=torch.zeros(7, device=DEV)),
        "long gradient buffer": dict(y_real=y, y_fake=z, df=torch.zeros(9, device=DEV)),
        "gradient for the absent side": dict(y_real=None, y_fake=z, dr=torch.zeros(8, device=DEV)),
        "no side": dict(y_real=None, y_fake=None),
        "empty": dict(y_real=y[:0], y_fake=z[:0]),
        "n_global < n": dict(y_real=y, y_fake=z, n_global=7),
        "float32 out": dict(y_real=y, y_fake=z, out=torch.zeros(4, device=DEV)),
        "cpu out": dict(y_real=y, y_fake=z, out=d4.cpu()),
    }
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        for what, kw in bad.items():
            kw = dict(dict(hyper=hyper, state=state), **kw)
            with pytest.raises(L.RganError):
                K.lecam(kw.pop("y_real"), kw.pop("y_fake"), kw.pop("hyper"), kw.pop("state"), **kw)
                pytest.fail(what)
        for args in ((d4.cpu(), 8, 3, hyper, state), (d4, 8, 3, hyper, state.cpu()), (d4.float(), 8, 3, hyper, state),
                     (d4, 0, 3, hyper, state), (d4, 8, 0, hyper, state), (d4, 8, 4, hyper, state),
                     (d4, 8, 3, hyper[:2], state)):
            with pytest.raises(L.RganError):
                K.lecam_finish(*args)
    finally:
        L._LIB = real
    assert proxy.calls == {}, proxy.calls  # refused before any pointer was taken
    assert state.tolist() == _state(5).tolist()


def test_opcheck_both_ops():
    from relativisticgan_amd import ops  # noqa: F401  (registers rgan::)
    vr, vf = _values(65)
    yr, yf = vr.to(DEV), vf.to(DEV)
    utils = ("test_schema", "test_faketensor")
    d4 = lambda: torch.zeros(4, dtype=torch.float64, device=DEV)  # noqa: E731
    torch.library.opcheck(torch.ops.rgan.lecam_.default,
                          (yr, yf, _hyper(), _state(5), torch.empty_like(yr), torch.empty_like(yf), d4(), 65, False),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.rgan.lecam_.default,
                          (yr, None, _hyper(), _state(5), torch.empty_like(yr), None, d4(), 130, True),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.rgan.lecam_.default, (None, yf, _hyper(), _state(5), None, None, d4(), 65, False),
                          test_utils=utils)
    sums = torch.tensor([3.0, -2.0, 10.0, 12.0], dtype=torch.float64, device=DEV)
    torch.library.opcheck(torch.ops.rgan.lecam_finish_.default, (sums, 65, 3, _hyper(), _state(5), d4()),
                          test_utils=utils)
    # the operators are the wrappers
    from relativisticgan_amd import kernels as K
    want, w_dr, w_df = K.lecam(yr, yf, _hyper(), _state(5))
    state, out, dr, df = _state(5), d4(), torch.empty_like(yr), torch.empty_like(yf)
    torch.ops.rgan.lecam_(yr, yf, _hyper(), state, dr, df, out, 65, False)
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(dr), _bits(w_dr))
    assert torch.equal(_bits(df), _bits(w_df)) and state[2].item() == 6.0
    part, loss = d4(), d4()
    torch.ops.rgan.lecam_(yr, yf, _hyper(), _state(5), None, None, part, 65, True)
    state2 = _state(5)
    torch.ops.rgan.lecam_finish_(part, 65, 3, _hyper(), state2, loss)
    assert abs(loss[0].item() - want[0].item()) <= SUM_TOL * want[0].item() and state2[2].item() == 6.0
    assert all(abs(a - b) <= SUM_TOL * abs(b) for a, b in zip(state2.tolist()[:2], state.tolist()[:2]))


def _reg(calls=5, lam=LAM, beta=BETA, start=START, a_real=A_REAL, a_fake=A_FAKE):
    from relativisticgan_amd.lecam import LeCam
    reg = LeCam(torch.device(DEV), lam, beta, start)
    reg.load_state_dict({"a_real": a_real, "a_fake": a_fake, "calls": calls})
    return reg


def test_lecam_object():
    reg = _reg()
    assert reg.hyper.tolist() == [LAM, BETA, float(START), 0.0] and reg.state.tolist() == [A_REAL, A_FAKE, 5.0, 0.0]
    assert reg.hyper.dtype == reg.state.dtype == torch.float64 and reg.state.is_cuda
    assert reg.read() == (A_REAL, A_FAKE)
    assert reg.state_dict() == {"a_real": A_REAL, "a_fake": A_FAKE, "calls": 5.0}
    ptr = reg.state.data_ptr()
    reg.restart()
    assert reg.state.tolist() == [0.0] * 4 and reg.state.data_ptr() == ptr  # in place: a capture keeps its address


@pytest.mark.parametrize("shape", SHAPES)
def test_autograd_of_the_term(shape):
    from relativisticgan_amd import losses
    real, fake = shape != "fake", shape != "real"
    vr, vf = _values(65)
    yr = vr.to(DEV).view(65, 1, 1, 1).requires_grad_(True) if real else None  # D's output shape
    yf = vf.to(DEV).view(65, 1, 1, 1).requires_grad_(True) if fake else None
    ins = [t for t in (yr, yf) if t is not None]
    c = ref.LeCam(LAM, BETA, START, A_REAL, A_FAKE, 5)
    L, gr, gf = c.step(vr.numpy() if real else None, vf.numpy() if fake else None)
    wants = [g for g in (gr, gf) if g is not None]
    reg = _reg()
    term = losses.lecam(yr, yf, reg)
    assert term.dtype == torch.float64 and term.dim() == 0 and abs(term.item() - L) <= SUM_TOL * L
    assert reg.state.tolist()[2] == (6.0 if fake else 5.0)
    for got, want in zip(torch.autograd.grad(term, ins, retain_graph=True), wants):
        assert got.shape == (65, 1, 1, 1) and _ulps(got.reshape(-1).cpu().numpy(), want).max() <= 1.0
    # a unit seed hands the saved gradients on; another upstream gradient scales them (1/4: exactly)
    unit = losses.unit_seed(torch.device(DEV), torch.float64)
    plain = torch.autograd.grad(term, ins, unit, retain_graph=True)
    quarter = torch.autograd.grad(term, ins, torch.tensor(0.25, dtype=torch.float64, device=DEV))
    for p, q, want in zip(plain, quarter, wants):
        assert _ulps(p.reshape(-1).cpu().numpy(), want).max() <= 1.0
        assert torch.equal(_bits(q), _bits(p * 0.25))
    assert reg.state.tolist()[2] == (6.0 if fake else 5.0)  # backward moves nothing
    # no gradient wanted: the term alone
    reg2 = _reg()
    with torch.no_grad():
        term2 = losses.lecam(yr, yf, reg2)
    assert not term2.requires_grad and torch.equal(_bits(term2.reshape(1)), _bits(term.detach().reshape(1)))


def test_joint_form_writes_one_buffer():
    from relativisticgan_amd import losses
    vr, vf = _values(65)
    y = torch.cat([vr, vf]).to(DEV).view(130, 1, 1, 1).requires_grad_(True)
    reg, reg2 = _reg(), _reg()
    term = losses.lecam_cat(y, reg)
    yr, yf = y.detach()[:65].clone().requires_grad_(True), y.detach()[65:].clone().requires_grad_(True)
    want = losses.lecam(yr, yf, reg2)
    assert torch.equal(_bits(term.detach().reshape(1)), _bits(want.detach().reshape(1)))
    assert torch.equal(_bits(reg.state), _bits(reg2.state))
    unit = losses.unit_seed(torch.device(DEV), torch.float64)
    g, = torch.autograd.grad(term, y, unit)
    gr, gf = torch.autograd.grad(want, [yr, yf], unit)
    assert g.shape == y.shape and torch.equal(_bits(g), _bits(torch.cat([gr, gf])))
    with pytest.raises(ValueError):
        losses.lecam_cat(y.detach()[:129], reg)
    with pytest.raises(ValueError):
        losses.lecam(None, None, reg)


# ---------------------------------------------------------------- 4. capture
def test_captured_call_moves_the_anchors_and_follows_lambda():
    from relativisticgan_amd import kernels as K
    n = 65
    gen = torch.Generator().manual_seed(5)
    ys = [(torch.randn(n, generator=gen) + k, torch.randn(n, generator=gen) - k) for k in range(6)]
    yr, yf = ys[0][0].to(DEV), ys[0][1].to(DEV)
    hyper, state = _hyper(start=2), _state(0, 0.0, 0.0)
    dr, df, out = torch.empty_like(yr), torch.empty_like(yf), torch.zeros(4, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.lecam(yr, yf, hyper, _state(0), dr=dr, df=df)  # (first use outside the capture)
        dr.zero_(), df.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        K.lecam(yr, yf, hyper, state, dr=dr, df=df, out=out)
    torch.cuda.synchronize()
    assert state.tolist() == [0.0, 0.0, 0.0, 0.0] and (dr == 0).all() and out.tolist() == [0.0] * 4  # nothing ran
    c = ref.LeCam(LAM, BETA, 2)
    for k in range(1, 6):
        lam = LAM if k < 4 else 1.5  # written between replays
        with torch.cuda.stream(side):
            yr.copy_(ys[k][0]), yf.copy_(ys[k][1])
            hyper[:1].fill_(lam)
            graph.replay()
        torch.cuda.synchronize()
        c.lam = lam
        c0 = ref.LeCam(lam, BETA, 2, c.a_real, c.a_fake, c.calls)
        L, gr, gf = c.step(ys[k][0].numpy(), ys[k][1].numpy())
        errs = _sum_errors(c0, c, L, out[0].item(), state.tolist(), ys[k][0].numpy(), ys[k][1].numpy(), n, True, True)
        assert all(e <= SUM_TOL for e in errs.values()), (k, errs)
        if c0.weight() == 0:
            assert k <= 2 and (dr == 0).all() and (df == 0).all()
        else:
            assert _ulps(dr.cpu().numpy(), gr).max() <= 1.0 and _ulps(df.cpu().numpy(), gf).max() <= 1.0
        # the restatement goes on from the device's anchors, so the bound stays one step's
        c.a_real, c.a_fake = state[0].item(), state[1].item()
    assert state[2].item() == 5.0 and c.calls == 5


# ---------------------------------------------------------------- 5. one iteration against an exact step
LECAM = dict(rgan_lecam=LAM, rgan_lecam_beta=BETA, rgan_lecam_start=START)
PRELOAD = {"a_real": A_REAL, "a_fake": A_FAKE, "calls": 5}
STEP_CASES = {
    "ralsgan_batched": dict(loss_D=7),
    "sgan_unbatched": dict(loss_D=1, rgan_batch_D=False),
    "wgangp": dict(loss_D=3),
    "ralsgan_diffaug_r1": dict(loss_D=7, rgan_diffaug=POLICY, rgan_r1=2.0),
}


def _trainer(kw, lecam=LECAM, preload=PRELOAD):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    cfg = dict(STEP, print_every=10 ** 9)
    cfg.update(kw)
    cfg.update(lecam or {})
    t = Trainer(make_param(**cfg), synthetic_images(64, 32, device=DEV))
    if lecam and preload:
        t.lecam.load_state_dict(preload)
    return t


def _term64(y, anchor, w):
    return w * ((y.reshape(-1) - anchor) ** 2).mean()


def _exact_step(kw, init_G, init_D, feed):
    """tests/test_r1r2_gpu.py's exact float64 iteration with the LeCam term added to the backward
    that carries errD: anchors and weight from the restatement, which each call then moves (the
    two single-side calls of the unbatched heads 1-4 in their order)."""
    from oracle import reference_cpu as O
    from relativisticgan_amd.augment import parse_policy
    from tests import diffaug_ref
    mask = parse_policy(kw.get("rgan_diffaug", ""))
    p = O.make_param(cuda=False, **STEP, **{k: v for k, v in kw.items() if not k.startswith("rgan_")})
    G, D = O.build_G(p).double(), O.build_D(p).double()
    G.load_state_dict({k: v.double() for k, v in init_G.items()})
    D.load_state_dict({k: v.double() for k, v in init_D.items()})
    f = {k: v.double() for k, v in feed.items()}
    kind, B = p.loss_D, p.batch_size
    ones, zeros = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    c = ref.LeCam(LAM, BETA, START, **PRELOAD)
    w = c.weight()
    split = kind <= 4 and kw.get("rgan_batch_D", True) is False

    def T(x, u):
        return diffaug_ref.forward(x, u, mask) if mask else x

    out = {}
    x_t = T(f["x_D"], feed["aug_D"][:B])
    fake_t = T(G(f["z_D"]).detach(), feed["aug_D"][B:])
    y_pred = D(x_t)
    if split:
        err_real = O.head_real(kind, y_pred, ones)
        lc_real = _term64(y_pred, c.a_fake, w)
        (err_real + lc_real).backward()
        c.step(y_pred.detach().numpy(), None)
        y_fake = D(fake_t)
        err_fake = O.head_fake(kind, y_fake, zeros)
        lc_fake = _term64(y_fake, c.a_real, w)  # a_real as the real-only call left it
        (err_fake + lc_fake).backward()
        c.step(None, y_fake.detach().numpy())
        out["errD"], out["lecam"] = (err_real + err_fake).detach(), (lc_real + lc_fake).detach()
    else:
        y_fake = D(fake_t)
        if kind <= 4:
            errD = O.head_real(kind, y_pred, ones) + O.head_fake(kind, y_fake, zeros)
        else:
            errD = O.head_relativistic_D(kind, y_pred, y_fake, ones, zeros)
        lc = _term64(y_pred, c.a_fake, w) + _term64(y_fake, c.a_real, w)
        (errD + lc).backward()
        c.step(y_pred.detach().numpy(), y_fake.detach().numpy())
        out["errD"], out["lecam"] = errD.detach(), lc.detach()
    if kind == 3 or p.grad_penalty:
        gp = O.gradient_penalty(D, x_t, fake_t, f["u"], p.penalty, ones)
        gp.backward()
        out["gp"] = gp.detach()
    for key, point in (("r1", x_t), ("r2", fake_t)):
        gamma = kw.get("rgan_" + key, 0.0)
        if gamma:
            pen = _zc64(D, point, gamma)
            pen.backward()
            out[key] = pen.detach()
    out["gradD"] = {n: q.grad.detach().clone() for n, q in D.named_parameters()}
    out["bufD"] = {k: v.detach().clone() for k, v in D.named_buffers()}
    torch.optim.Adam(D.parameters(), lr=p.lr_D, betas=(p.beta1, p.beta2), weight_decay=p.weight_decay).step()
    out["postD"] = {k: v.detach().float() for k, v in D.state_dict().items()}
    D.load_state_dict({k: v.double() for k, v in out["postD"].items()})
    for q in D.parameters():
        q.requires_grad = False
    y_pred_fake = D(T(G(f["z_G"]), feed["aug_G"][:B]))
    y_real = D(T(f["x_G"], feed["aug_G"][B:])) if kind > 4 else None
    errG = O.head_G(kind, y_pred_fake, y_real, ones, zeros)
    errG.backward()
    out["errG"] = errG.detach()
    out["gradG"] = {n: q.grad.detach().clone() for n, q in G.named_parameters()}
    return out


def _follow(c, rec, split):
    """The restatement moved by a D step's recorded outputs, as the trainer calls the kernel."""
    yr, yf = rec["y_pred"].cpu().numpy(), rec["y_pred_fake"].cpu().numpy()
    if split:
        c.step(yr, None)
        c.step(None, yf)
    else:
        c.step(yr, yf)


def _anchor_err(state, c):
    return max(abs(state[k] - c.state[k]) / max(abs(c.state[k]), 1e-300) for k in (0, 1))


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_iteration_matches_exact_step(name):
    kw = STEP_CASES[name]
    torch.set_num_threads(4)
    t = _trainer(kw)
    split = name == "sgan_unbatched"
    assert t.lecam is not None and t.batch_D == (not split) and bool(t.aug) == ("rgan_diffaug" in kw)
    init_G = {k: v.detach().cpu().clone() for k, v in t.G.state_dict().items()}
    init_D = {k: v.detach().cpu().clone() for k, v in t.D.state_dict().items()}
    feed = _step_feed(kw["loss_D"])
    want = _exact_step(kw, init_G, init_D, feed)
    got = {}

    def hook(tag, r):
        if tag == "D":
            got["D"] = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)}
            got["gradD"] = {n: q.grad.detach().clone() for n, q in t.D.named_parameters()}
            got["bufD"] = {k: v.detach().clone() for k, v in t.D.named_buffers()}
            got["state"] = t.lecam.state.tolist()
        elif tag == "D.post":
            t.D.load_state_dict(want["postD"])
        elif tag == "G":
            got["G"] = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v)}
            got["gradG"] = {n: q.grad.detach().clone() for n, q in t.G.named_parameters()}

    t.iteration(1, feed={k: v.to(DEV) for k, v in feed.items()}, hooks=hook)
    t.flush()
    torch.cuda.synchronize()
    report = []

    def check(label, a, b, tol):
        r = _rel(a, b)
        print(f"{name} {label}: rel L2 {r:.2e} (tol {tol:.0e})")
        if not r <= tol:
            report.append(f"{label}: {r:.2e} > {tol:.0e}")

    check("errD", got["D"]["errD"], want["errD"], TOL_OUT)
    check("errG", got["G"]["errG"], want["errG"], TOL_OUT)
    check("lecam", got["D"]["lecam"], want["lecam"], TOL_OUT)
    assert want["lecam"].item() > 0
    for key in ("gp", "r1", "r2"):
        assert (key in want) == (key in got["D"]), key
        if key in want:
            check(key, got["D"][key], want[key], TOL_OUT)
    assert ("gp" in want) == (name == "wgangp") and ("r1" in want) == (name == "ralsgan_diffaug_r1")
    for side in ("gradD", "gradG"):
        assert list(got[side]) == list(want[side])
        for n in want[side]:
            check(f"{side}.{n}", got[side][n], want[side][n], TOL_GRAD)
    assert list(got["bufD"]) == list(want["bufD"])
    for k, v in want["bufD"].items():
        if v.is_floating_point():
            check(f"bufD.{k}", got["bufD"][k], v, TOL_BUF)
        else:
            assert int(got["bufD"][k]) == int(v), k
    # the anchors after the step: the restatement fed the step's own recorded outputs
    c = ref.LeCam(LAM, BETA, START, **PRELOAD)
    _follow(c, got["D"], split)
    e = _anchor_err(got["state"], c)
    print(f"{name} anchors after the step: rel {e:.2e}")
    assert e <= SUM_TOL and got["state"][2] == 6.0 and t.lecam.state.tolist() == got["state"]
    assert not report, report


# ---------------------------------------------------------------- 6. trajectory
@pytest.mark.parametrize("name", ["ralsgan_batched", "sgan_unbatched"])
def test_trajectory_follows_the_restatement(name):
    kw = dict(STEP_CASES[name], Diters=2)
    t = _trainer(kw, preload=None)
    split = name == "sgan_unbatched"
    c = ref.LeCam(LAM, BETA, START)
    assert t.lecam.state.tolist() == c.state
    terms, worst = [], [0.0]

    def hook(tag, r):
        if tag == "D":
            _follow(c, r, split)
            state = t.lecam.state.tolist()
            worst[0] = max(worst[0], _anchor_err(state, c))
            assert state[2] == float(c.calls) and worst[0] <= SUM_TOL, (len(terms), state, c.state)
            c.a_real, c.a_fake = state[0], state[1]  # go on from the device's anchors
            terms.append(r["lecam"].item())

    for i in range(1, 5):
        t.iteration(i, hooks=hook)
    t.flush()
    torch.cuda.synchronize()
    print(f"{name}: lecam per D step {terms}; worst anchor rel err {worst[0]:.2e}")
    assert len(terms) == 8 and c.calls == 8 and t.lecam.state[2].item() == 8.0
    # calls 0, 1, 2 are below start = 3: with two D steps an iteration, the first two steps (calls 0
    # and 1) weigh nothing, and so does the third (calls 2); positive from calls == 3 on
    assert terms[:2] == [0.0, 0.0] and terms[2] == 0.0 and all(v > 0 for v in terms[3:]), terms
    line = t.log_line(4, 0.0)
    assert line.endswith(" lecam: %.4f a_real: %.4f a_fake: %.4f" % ((terms[-1],) + t.lecam.read())), line


# ---------------------------------------------------------------- 7. launch accounting
OFF_CASES = {"ralsgan_batched": dict(loss_D=7), "wgangp_penalty": dict(loss_D=3),
             "sgan_unbatched": dict(loss_D=1, rgan_batch_D=False), "ralsgan_unbatched": dict(loss_D=7, rgan_batch_D=False)}


def _counted(t, run):
    from relativisticgan_amd import _lib as L
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        run(proxy)
        t.flush()
        torch.cuda.synchronize()
    finally:
        L._LIB = real
    return proxy.calls


@pytest.mark.parametrize("name", sorted(OFF_CASES))
def test_launch_accounting(name):
    kw = OFF_CASES[name]
    off = _trainer(kw, lecam=None)
    assert off.lecam is None
    calls = _counted(off, lambda proxy: off.iteration(1))
    assert calls.get("rgan_conv_fwd", 0) + calls.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    assert not [k for k in calls if k.startswith("rgan_lecam")], calls
    assert "lecam" not in off.last["D"] and "lecam" not in off.state(1)
    line = off.log_line(1, 0.0)
    assert "lecam" not in line and "a_real" not in line and line.endswith("time:0.0000")
    on = _trainer(kw)
    got = _counted(on, lambda proxy: on.iteration(1))
    # no extra pass of D: every conv / BatchNorm entry point as often as with the flag off
    for k in set(calls) | set(got):
        if k.startswith(("rgan_conv_", "rgan_bn_")):
            assert got.get(k, 0) == calls.get(k, 0), (k, got.get(k), calls.get(k))
    assert got.get("rgan_lecam", 0) == (2 if name == "sgan_unbatched" else 1), got
    assert "rgan_lecam_finish" not in got  # one rank: the fused launch
    rest = {k: v for k, v in got.items() if not k.startswith("rgan_lecam")}
    assert rest == calls, {k: (calls.get(k), rest.get(k)) for k in set(calls) | set(rest) if calls.get(k) != rest.get(k)}
    assert on.last["D"]["lecam"].item() > 0 and "lecam" in on.state(1)
    # Diters D steps: one update each
    two = _trainer(dict(kw, Diters=2))
    got2 = _counted(two, lambda proxy: two.iteration(1))
    assert got2.get("rgan_lecam", 0) == 2 * got["rgan_lecam"] and two.lecam.state[2].item() == 7.0


def test_pac2_runs_with_the_term():
    t = _trainer(dict(loss_D=7, pac=2))
    assert t.pac == 2 and not t.batch_D
    c = ref.LeCam(LAM, BETA, START, **PRELOAD)
    t.iteration(1, hooks=lambda tag, r: _follow(c, r, False) if tag == "D" else None)
    t.flush()
    torch.cuda.synchronize()
    assert _anchor_err(t.lecam.state.tolist(), c) <= SUM_TOL and t.last["D"]["lecam"].item() > 0


# ---------------------------------------------------------------- 8. checkpoint
def _feeds(count, seed=41):
    gen = torch.Generator().manual_seed(seed)
    B = STEP["batch_size"]
    out = []
    for _ in range(count):
        f = {"x_D": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, "z_D": torch.randn(B, 16, 1, 1, generator=gen),
             "z_G": torch.randn(B, 16, 1, 1, generator=gen), "x_G": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1}
        out.append({k: v.to(DEV) for k, v in f.items()})
    return out


def test_checkpoint_carries_the_anchors():
    kw = STEP_CASES["ralsgan_batched"]
    feeds = _feeds(5)
    ref_keys = {"i", "current_set_images", "G_state", "D_state", "G_optimizer", "D_optimizer", "G_scheduler",
                "D_scheduler", "z_test"}
    off = _trainer(kw, lecam=None)
    assert set(off.state(0)) == ref_keys
    whole, first = _trainer(kw, preload=None), _trainer(kw, preload=None)
    for i in range(5):
        whole.iteration(i + 1, feed=feeds[i])
    for i in range(3):
        first.iteration(i + 1, feed=feeds[i])
    st = first.state(3, 0)
    assert set(st) == ref_keys | {"lecam"} and set(st["lecam"]) == {"a_real", "a_fake", "calls"}
    assert st["lecam"]["calls"] == 3.0 and st["lecam"]["a_real"] != 0.0
    path = os.path.join(tempfile.mkdtemp(), "state_01.pth")
    torch.save(st, path)
    resumed = _trainer(kw, preload=None)
    assert resumed.load(torch.load(path, weights_only=True)) == (3, 0)
    assert torch.equal(_bits(resumed.lecam.state), _bits(first.lecam.state))
    for i in range(3, 5):
        resumed.iteration(i + 1, feed=feeds[i])
    whole.flush(), resumed.flush()
    torch.cuda.synchronize()
    assert torch.equal(_bits(resumed.lecam.state), _bits(whole.lecam.state)), (resumed.lecam.state, whole.lecam.state)
    assert whole.lecam.state[2].item() == 5.0
    # a checkpoint without the key (the reference's, or the flag was off): the anchors start afresh
    fresh = _trainer(kw)
    assert fresh.lecam.state.tolist() == [A_REAL, A_FAKE, 5.0, 0.0]
    fresh.load({k: v for k, v in st.items() if k != "lecam"})
    assert fresh.lecam.state.tolist() == [0.0, 0.0, 0.0, 0.0]
    # ... and a flag-off trainer ignores the key
    off.load(st)
    assert off.lecam is None and set(off.state(3)) == ref_keys
    # a captured trainer still refuses to checkpoint
    whole.graph_captured = True
    with pytest.raises(RuntimeError, match="captured"):
        whole.state(5)


# ---------------------------------------------------------------- 9. data parallel
DP_OVER = dict(rgan_lecam=LAM, rgan_lecam_beta=BETA, rgan_lecam_start=1)


def test_dp2_syncbn_matches_single_process():
    from tests.test_dp_gpu import _compare, _run, _spawn
    single = _run("ralsgan", 1, 0, overrides=DP_OVER)
    dpres = _spawn("ralsgan", overrides=DP_OVER)
    _compare("ralsgan", dpres, single)


def test_dp2_separate_passes_match_single_process():
    """Heads 1-4 with separate D(x) / D(x_fake) passes: the two single-side calls on every rank."""
    from tests.test_dp_gpu import _compare, _run, _spawn
    single = _run("sgan", 1, 0, batch_D=False, overrides=DP_OVER)
    dpres = _spawn("sgan", batch_D=False, overrides=DP_OVER)
    _compare("sgan", dpres, single)


def test_dp2_per_shard_bn_runs():
    """Per-shard statistics are not the global-batch maths: finite, and shaped like the
    single-process step (the reducer armed exactly once per D step, or finish() would raise)."""
    from tests.test_dp_gpu import _run, _spawn
    single = _run("ralsgan", 1, 0, n_iter=1, overrides=DP_OVER)
    dpres = _spawn("ralsgan", sync_bn=False, n_iter=1, overrides=DP_OVER)
    assert len(dpres) == len(single) == 1
    a, b = dpres[0], single[0]
    assert a["errD"].shape == b["errD"].shape and torch.isfinite(a["errD"]).all()
    assert list(a["gradD"]) == list(b["gradD"])
    for n in b["gradD"]:
        assert a["gradD"][n].shape == b["gradD"][n].shape and torch.isfinite(a["gradD"][n]).all(), n


DP_ITERS = 3


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)  # gloo: both ranks on cuda:0, as tests/test_dp_gpu.py runs its world-2 cases
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import dp
    dp.setup(sync_bn=True)
    try:
        t = _trainer(dict(loss_D=7, rgan_rng="host"), lecam=dict(LECAM, rgan_lecam_start=2), preload=None)
        assert t.B == STEP["batch_size"] // world and dp.active()
        recs, states = [], []

        def hooks(tag, r):
            if tag == "D":
                recs.append((r["y_pred"].detach().cpu().reshape(-1).clone(),
                             r["y_pred_fake"].detach().cpu().reshape(-1).clone(), r["lecam"].item()))
                states.append(t.lecam.state.tolist())

        real = L.lib()
        proxy = L._LIB = _Counter(real)
        try:
            for i in range(1, 1 + DP_ITERS):
                t.iteration(i, hooks=hooks)
            t.flush()
        finally:
            L._LIB = real
        torch.save({"recs": recs, "states": states, "sd": t.lecam.state_dict(),
                    "calls": {k: v for k, v in proxy.calls.items() if k.startswith("rgan_lecam")}},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_dp2_ranks_share_the_anchors():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out_dir = tempfile.mkdtemp()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out_dir)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    r0, r1 = (torch.load(os.path.join(out_dir, f"rank{r}.pt"), weights_only=True) for r in range(2))
    c = ref.LeCam(LAM, BETA, 2)
    half = STEP["batch_size"] // 2
    for i in range(DP_ITERS):
        assert r0["states"][i] == r1["states"][i], i  # bit-identical anchors on both ranks
        assert r0["recs"][i][2] == r1["recs"][i][2]  # ... and the same (global) term
        yr = np.concatenate([r["recs"][i][0].numpy() for r in (r0, r1)])  # the union of the ranks' outputs
        yf = np.concatenate([r["recs"][i][1].numpy() for r in (r0, r1)])
        assert yr.size == 2 * half
        c0 = ref.LeCam(LAM, BETA, 2, c.a_real, c.a_fake, c.calls)
        L = c.step(yr, yf)[0]
        errs = _sum_errors(c0, c, L, r0["recs"][i][2], r0["states"][i], yr, yf, 2 * half, True, True)
        assert all(e <= SUM_TOL for e in errs.values()), (i, errs)
        c.a_real, c.a_fake = r0["states"][i][0], r0["states"][i][1]
    assert r0["sd"] == r1["sd"] and r0["sd"]["calls"] == float(DP_ITERS)
    assert r0["recs"][0][2] == 0.0 and r0["recs"][1][2] == 0.0 and r0["recs"][2][2] > 0
    # per D step and rank: the partial-sums launch and the finish launch (the all-reduce in between)
    assert r0["calls"] == r1["calls"] == {"rgan_lecam": DP_ITERS, "rgan_lecam_finish": DP_ITERS}


# ---------------------------------------------------------------- 10. CLI
def test_train_cli_runs_checkpoints_and_resumes():
    root = tempfile.mkdtemp()
    out, extra = os.path.join(root, "out"), os.path.join(root, "extra")
    common = ["--loss_D", "7", *TINY_CLI, "--batch_size", "8", "--D_h_size", "8", "--seed", "1", "--gen_every", "3",
              "--gen_extra_images", "0", "--output_folder", out, "--extra_folder", extra, "--rgan_synthetic", "64",
              "--print_every", "1", "--Diters", "2", "--rgan_lecam", "0.3", "--rgan_lecam_start", "2"]
    r = subprocess.run([sys.executable, "-m", "relativisticgan_amd.train", *common, "--n_iter", "3"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Models saved" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[") and " loss_D: " in ln]
    assert len(lines) == 3, r.stdout[-2000:]
    for ln in lines:
        tail = ln.split(" time:")[1].split()
        assert tail[1::2] == ["lecam:", "a_real:", "a_fake:"], ln
        assert all(np.isfinite(float(v)) for v in tail[2::2]), ln
    assert float(lines[-1].split(" lecam: ")[1].split()[0]) > 0
    path = os.path.join(extra, "models", "state_01.pth")
    ck = torch.load(path, weights_only=True)
    assert ck["i"] == 3 and set(ck["lecam"]) == {"a_real", "a_fake", "calls"}
    assert ck["lecam"]["calls"] == 6.0  # 3 iterations of 2 D steps
    from relativisticgan_amd.train import main
    t = main([*common, "--n_iter", "6", "--load", path])  # resumed in this process
    assert t.lecam.state[2].item() == 12.0 and " lecam: " in t.log_line(5, 0.0)
    ck2 = torch.load(os.path.join(extra, "models", "state_02.pth"), weights_only=True)
    assert ck2["i"] == 6 and ck2["lecam"]["calls"] == 12.0
