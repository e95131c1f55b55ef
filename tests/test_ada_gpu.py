"""--rgan_aug_p / --rgan_ada_target on the MI355X: the gated transform (rgan_diffaug_p) bit for
bit against the ungated kernel sample by sample, the rank statistic and the controller
(csrc/ada.hip) exactly against the host restatement (tests/ada_ref.py), and the probability
through every layer above them: operators, augment.apply, graph capture, the training step
eager / captured / resumed from a checkpoint / data parallel.

Every comparison here is exact (bits, or ``==`` on doubles): the gated kernels are the ungated
ones with the sample's policy masked, the statistic is a sum of integers, and the controller's
steps are dyadic in these tests.  The one tolerance is the adjoint identity's 1e-5, the bound
tests/test_diffaug_gpu.py uses for the same construction.
"""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

from tests import ada_ref as ref
from tests.test_diffaug_gpu import POLICY, STEP, STEP_CASES, _bits, _Counter, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, H, W): small vectorised, scalar path (W % 4 != 0), more than 4 channels, non-square with
# an odd height, multi-block reduction; "shifted" is (2, 3, 64, 64) at a 4-byte offset (scalar
# kernels on a width that would vectorise).
SHAPES = [(5, 3, 8, 8), (3, 3, 10, 10), (2, 5, 12, 12), (2, 2, 9, 20), (2, 3, 64, 64), "shifted"]
HALF = 0.5
BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _shift(t):
    out = torch.empty(t.numel() + 1, device=DEV)[1:].view_as(t).copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


_CASES = {}


def _case(shape):
    """(x, dy, u) of a shape: test_diffaug_gpu's seeded inputs, or copies of them 4 bytes off."""
    if shape not in _CASES:
        x, dy, us = _inputs((2, 3, 64, 64) if shape == "shifted" else shape)
        _CASES[shape] = (_shift(x), _shift(dy), us["rand"]) if shape == "shifted" else (x, dy, us["rand"])
    return _CASES[shape]


def _p(v):
    return torch.tensor([v], dtype=torch.float64, device=DEV)


def _gate_rounds(B):
    """Gate tables for p = 1/2 whose open masks cover 0..7 across the rounds (sample b of round r
    has mask (r B + b) mod 8).  Closed gates alternate 1/2 itself and 0.9, open ones the float
    below 1/2 and 0.1, so both edge values occur in every table."""
    rounds = []
    for r in range(-(-8 // B)):
        rows, k = [], 0
        for b in range(B):
            mask, row = (r * B + b) % 8, []
            for g in range(3):
                is_open = bool(mask >> g & 1)
                row.append((BELOW, 0.1)[k % 2] if is_open else (HALF, 0.9)[k % 2])
                k += 1
            rows.append(row + [0.0])  # the reserved column opens nothing
        rounds.append(torch.tensor(rows, dtype=torch.float32, device=DEV))
    return rounds


def test_gate_tables_cover_every_mask_and_both_edges():
    for B in (2, 3, 5):
        rounds = _gate_rounds(B)
        masks = [m for g in rounds for m in ref.sub_policy(7, g.cpu().numpy(), HALF)]
        assert set(masks) == set(range(8)), (B, masks)
        assert masks == [(i % 8) for i in range(len(masks))]
        flat = torch.cat([g[:, :3].reshape(-1) for g in rounds]).cpu()
        assert (flat == HALF).any() and (flat == BELOW).any() and BELOW < HALF


# ---------------------------------------------------------------- 1. the gated kernel, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_p1_is_the_ungated_kernel_and_p0_the_input(shape):
    from relativisticgan_amd import kernels as K
    x, dy, u = _case(shape)
    gen = torch.Generator(device=DEV).manual_seed(5)
    gate = torch.rand(x.shape[0], 4, device=DEV, generator=gen)
    one, zero = _p(1.0), _p(0.0)
    for policy in range(8):
        for src, adjoint in ((x, False), (dy, True)):
            want = K.diffaug(src, u, policy, adjoint=adjoint)
            got = K.diffaug(src, u, policy, adjoint=adjoint, gate=gate, p=one)
            assert torch.equal(_bits(got), _bits(want)), (shape, policy, adjoint)
            got = K.diffaug(src, u, policy, adjoint=adjoint, gate=gate, p=zero)
            assert torch.equal(_bits(got), _bits(src)), (shape, policy, adjoint)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_each_sample_is_the_ungated_kernel_with_its_open_groups(shape):
    from relativisticgan_amd import kernels as K
    x, dy, u = _case(shape)
    B = x.shape[0]
    half = _p(HALF)
    seen = set()
    for gate in _gate_rounds(B):
        for policy in range(8):
            masks = ref.sub_policy(policy, gate.cpu().numpy(), HALF)
            seen.update(masks)
            for src, adjoint in ((x, False), (dy, True)):
                got = K.diffaug(src, u, policy, adjoint=adjoint, gate=gate, p=half)
                again = K.diffaug(src, u, policy, adjoint=adjoint, gate=gate, p=half)
                assert torch.equal(_bits(got), _bits(again)), (shape, policy, adjoint)  # two calls, same bits
                for b in range(B):
                    want = K.diffaug(src[b:b + 1], u[b:b + 1], masks[b], adjoint=adjoint)
                    assert torch.equal(_bits(got[b:b + 1]), _bits(want)), (shape, policy, adjoint, b, masks[b])
                    if masks[b] == 0:
                        assert torch.equal(_bits(got[b]), _bits(src[b]))
    assert seen == set(range(8))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_adjoint_identity_of_the_gated_transform(shape):
    """<T_lin x, w> = <x, T^t w>, built as tests/test_diffaug_gpu.py builds it, under p = 1/2."""
    from relativisticgan_amd import kernels as K
    x, noise, u = _case(shape)
    half = _p(HALF)
    for gate in _gate_rounds(x.shape[0]):
        for policy in range(1, 8):
            lin = (K.diffaug(x, u, policy, gate=gate, p=half).double()
                   - K.diffaug(torch.zeros_like(x), u, policy, gate=gate, p=half).double())
            w = (lin + 0.5 * noise.double()).float()
            lhs = (lin * w.double()).sum().item()
            rhs = (x.double() * K.diffaug(w, u, policy, adjoint=True, gate=gate, p=half).double()).sum().item()
            assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (shape, policy, lhs, rhs)


# ---------------------------------------------------------------- 2. operators, autograd node, wrapper
def test_opcheck_and_autograd_is_the_gated_adjoint():
    from relativisticgan_amd import augment
    from relativisticgan_amd import kernels as K
    from relativisticgan_amd import ops  # noqa: F401  (registers rgan::)
    x, dy, u = _case((5, 3, 8, 8))
    gate, half = _gate_rounds(5)[0], _p(HALF)
    xg = x.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.rgan.diffaug_p.default, (xg, u, gate, half, 7),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    torch.library.opcheck(torch.ops.rgan.diffaug_p_backward.default, (dy, u, gate, half, 7),
                          test_utils=("test_schema", "test_faketensor"))
    want_y = K.diffaug(x, u, 7, gate=gate, p=half)
    want_g = K.diffaug(dy, u, 7, adjoint=True, gate=gate, p=half)
    y = torch.ops.rgan.diffaug_p(xg, u, gate, half, 7)
    assert torch.equal(_bits(y), _bits(want_y))
    dyg = dy.clone().requires_grad_(True)
    gx, = torch.autograd.grad(y, xg, dyg, create_graph=True)
    assert torch.equal(_bits(gx), _bits(want_g))
    with pytest.raises(NotImplementedError):  # no double backward, like rgan::diffaug
        torch.autograd.grad(gx.sum(), dyg)
    # the training step's node: the gated adjoint as its gradient, the output in the caller's buffer
    buf = torch.full_like(x, 7.0)
    y2 = augment.apply(xg, u, 7, out=buf, gate=gate, p=half)
    assert y2.data_ptr() == buf.data_ptr() and torch.equal(_bits(buf), _bits(want_y))
    gx2, = torch.autograd.grad(y2, xg, dy)
    assert torch.equal(_bits(gx2), _bits(want_g))
    buf2 = torch.full_like(x, 7.0)
    y3 = augment.apply(x, u, 7, out=buf2, gate=gate, p=half)  # no autograd: straight to the kernel
    assert y3.data_ptr() == buf2.data_ptr() and torch.equal(_bits(buf2), _bits(want_y))


def test_wrapper_rejects_bad_gates_and_p():
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import kernels as K
    x, _, u = _case((5, 3, 8, 8))
    gate, half = _gate_rounds(5)[0], _p(HALF)
    bad = {
        "gate rows": dict(gate=gate[:4], p=half),
        "gate columns": dict(gate=torch.zeros(5, 8, device=DEV), p=half),
        "gate flat": dict(gate=gate.reshape(-1), p=half),
        "gate dtype": dict(gate=gate.double(), p=half),
        "gate strided": dict(gate=torch.zeros(5, 8, device=DEV)[:, ::2], p=half),
        "gate on the cpu": dict(gate=gate.cpu(), p=half),
        "p float32": dict(gate=gate, p=half.float()),
        "p on the cpu": dict(gate=gate, p=half.cpu()),
        "p a number": dict(gate=gate, p=0.5),
        "p two values": dict(gate=gate, p=torch.zeros(2, dtype=torch.float64, device=DEV)),
        "gate alone": dict(gate=gate),
        "p alone": dict(p=half),
    }
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        for what, kw in bad.items():
            with pytest.raises(L.RganError):
                K.diffaug(x, u, 7, **kw)
    finally:
        L._LIB = real
    assert proxy.calls == {}, proxy.calls  # refused before any pointer was taken


def test_captured_gated_call_follows_p_and_the_gates():
    from relativisticgan_amd import kernels as K
    x, _, u = _case((5, 3, 8, 8))
    rounds = _gate_rounds(5)
    gate, p, out = rounds[0].clone(), _p(HALF), torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.diffaug(x, u, 7, out=out, gate=gate, p=p)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        K.diffaug(x, u, 7, out=out, gate=gate, p=p)
    first = K.diffaug(x, u, 7, gate=rounds[0], p=_p(HALF))
    for new_gate, new_p in ((rounds[1], HALF), (rounds[1], 1.0), (rounds[0], 0.0), (rounds[0], 0.05)):
        with torch.cuda.stream(side):
            gate.copy_(new_gate)
            p.fill_(new_p)
            out.zero_()
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(K.diffaug(x, u, 7, gate=new_gate, p=_p(new_p)))), new_p
    assert torch.equal(_bits(K.diffaug(x, u, 7, gate=rounds[0], p=_p(1.0))), _bits(K.diffaug(x, u, 7)))
    assert not torch.equal(first, K.diffaug(x, u, 7))


# ---------------------------------------------------------------- 3. statistic and controller
def _hyper(target, interval, ipu):
    return torch.tensor([target, float(interval), float(ipu), 0.0], dtype=torch.float64, device=DEV)


def _state(p=0.0):
    return torch.tensor([p, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)


def _outputs(n, seed):
    """Two vectors of D outputs with ties, +-inf and NaNs planted where n leaves room."""
    gen = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    inf, nan = float("inf"), float("nan")
    plant = [(1.5, 1.5), (inf, inf), (inf, 0.0), (-inf, 0.0), (0.0, inf), (nan, 0.0), (0.0, nan), (nan, nan),
             (0.0, -0.0), (-inf, -inf)]
    for k, (va, vb) in enumerate(plant):
        i = (7 * k + 3) % n  # spread over the vector (n = 1: the last pair wins)
        a[i], b[i] = va, vb
    if n > 70:
        a[n - 1], b[n - 1] = nan, 1.0  # the last element, in the last thread's stride
        a[64], b[64] = 2.0, 2.0
    return a, b


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_statistic_counts_exactly_and_accumulates(n):
    from relativisticgan_amd import kernels as K
    a, b = _outputs(n, n)
    s1, n1 = ref.rank_counts(a.numpy(), b.numpy())
    if n > 1:
        assert abs(s1) < n  # both signs and zeros occur
    hyper, state = _hyper(0.6, 4, 500000.0), _state(0.25)
    K.ada_update(a.to(DEV), b.to(DEV), hyper, state, adjust=False)
    assert state.tolist() == [0.25, float(s1), float(n1), 0.0]
    a2, b2 = _outputs(n, n + 100)
    s2, _ = ref.rank_counts(a2.numpy(), b2.numpy())
    K.ada_update(a2.to(DEV), b2.to(DEV), hyper, state, adjust=False)
    assert state.tolist() == [0.25, float(s1 + s2), float(2 * n), 0.0]
    # fused with the controller step: the call is counted, not yet due (interval 4), nothing else moves
    K.ada_update(a.to(DEV), b.to(DEV), hyper, state, adjust=True)
    assert state.tolist() == [0.25, float(2 * s1 + s2), float(3 * n), 1.0]


def test_wrapper_rejects_bad_statistic_arguments():
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import kernels as K
    a, b = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    hyper, state = _hyper(0.6, 4, 48.0), _state()
    bad = [(a, b[:7], hyper, state), (a[:0], b[:0], hyper, state), (a.cpu(), b, hyper, state),
           (a.double(), b.double(), hyper, state), (a, b, hyper.float(), state), (a, b, hyper, state[:3]),
           (a, b, hyper.cpu(), state), (a, b, hyper, state.cpu())]
    for args in bad:
        with pytest.raises(L.RganError):
            K.ada_update(*args)
    with pytest.raises(L.RganError):
        K.ada_adjust(hyper, state.float())
    assert state.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_shards_add_exactly():
    """A batch fed whole, in 2 and in 3 uneven shards (each shard into a state of its own, S and N
    summed by hand as the data-parallel step's all-reduce sums them): the same adjustment."""
    from relativisticgan_amd import kernels as K
    a, b = _outputs(4097, 9)
    a, b = a.to(DEV), b.to(DEV)
    hyper = _hyper(0.1, 1, 4.0 * 4097)  # one call per adjustment; the step is N / (4 N) = 1/4
    results = []
    for cuts in ((0, 4097), (0, 1000, 4097), (0, 1, 66, 4097)):
        parts = []
        for lo, hi in zip(cuts, cuts[1:]):
            st = _state(0.5)
            K.ada_update(a[lo:hi], b[lo:hi], hyper, st, adjust=False)
            parts.append(st)
        total = _state(0.5)
        total[1:3] = sum(p[1:3] for p in parts)
        before = total.tolist()
        K.ada_adjust(hyper, total)
        results.append((before, total.tolist()))
    assert results[0] == results[1] == results[2], results
    s, n = ref.rank_counts(a.cpu().numpy(), b.cpu().numpy())
    c = ref.Controller(0.5, 0.1, 1, 4.0 * 4097)
    c.update(a.cpu().numpy(), b.cpu().numpy())
    assert results[0] == ([0.5, float(s), float(n), 0.0], c.state) and c.p in (0.25, 0.75)


def test_controller_sequence_matches_restatement():
    """12 calls, interval 3, 16 pairs a call, 384 images per unit of p: steps of 48 / 384 = 1/8.
    The biases drive r above and below the target, through the clamp at 1 and back."""
    from relativisticgan_amd import kernels as K
    gen = torch.Generator().manual_seed(21)
    hyper, state = _hyper(0.5, 3, 384.0), _state(0.875)
    c = ref.Controller(0.875, 0.5, 3, 384.0)
    seen = []
    for call, bias in enumerate([3.0] * 6 + [-3.0] * 3 + [0.0] * 3, 1):
        a, b = torch.randn(16, generator=gen) + bias, torch.randn(16, generator=gen)
        if bias == 0.0:  # r == target exactly over the three calls: 12 right, 4 wrong in each
            a, b = torch.tensor([1.0] * 12 + [0.0] * 4), torch.tensor([0.0] * 12 + [1.0] * 4)
        K.ada_update(a.to(DEV), b.to(DEV), hyper, state, adjust=True)
        c.update(a.numpy(), b.numpy())
        assert state.tolist() == c.state, call
        seen.append(c.p)
    assert seen == [0.875] * 2 + [1.0] * 3 + [1.0] + [1.0] * 2 + [0.875] * 3 + [0.875], seen


def test_captured_update_counts_replays_and_follows_the_target():
    from relativisticgan_amd import ops  # noqa: F401
    # 3 of 4 pairs right, 1 wrong: r = 1/2, between the two targets used
    a = torch.tensor([1.0, 1.0, 1.0, 0.0], device=DEV)
    b = torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV)
    hyper, state = _hyper(0.25, 1, 32.0), _state(0.5)
    torch.library.opcheck(torch.ops.rgan.ada_update_.default, (a, b, hyper, _state(0.5), True),
                          test_utils=("test_schema", "test_faketensor"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.rgan.ada_update_(a, b, hyper, _state(0.5), True)  # (first use outside the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        torch.ops.rgan.ada_update_(a, b, hyper, state, True)
    assert state.tolist() == [0.5, 0.0, 0.0, 0.0]  # a capture runs nothing
    c = ref.Controller(0.5, 0.25, 1, 32.0)
    ps = []
    for k in range(7):
        target = 0.25 if k < 3 else 0.75
        with torch.cuda.stream(side):
            hyper[:1].fill_(target)
            graph.replay()
        torch.cuda.synchronize()
        c.target = target
        c.update(a.cpu().numpy(), b.cpu().numpy())
        assert state.tolist() == c.state, k
        ps.append(state[0].item())
    assert state[3].item() == 7.0
    assert ps == [0.625, 0.75, 0.875, 0.75, 0.625, 0.5, 0.375]


# ---------------------------------------------------------------- 4. the training step
ADA = dict(rgan_aug_p=0.5, rgan_ada_target=0.6, rgan_ada_interval=2, rgan_ada_kimg=0.048)
B = STEP["batch_size"]


def _trainer(kw, policy=POLICY, ada=ADA, **more):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    p = make_param(print_every=10 ** 9, rgan_diffaug=policy, **STEP, **kw, **(ada or {}), **more)
    return Trainer(p, synthetic_images(64, 32, device=DEV))


def _feed(kind, gen, device=DEV):
    groups = 2 if kind > 4 else 1
    f = {"x_D": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1, "z_D": torch.randn(B, 16, 1, 1, generator=gen),
         "aug_D": torch.rand(2 * B, 8, generator=gen), "gate_D": torch.rand(2 * B, 4, generator=gen),
         "u": torch.rand(B, 1, 1, 1, generator=gen),
         "z_G": torch.randn(B, 16, 1, 1, generator=gen), "x_G": torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1,
         "aug_G": torch.rand(groups * B, 8, generator=gen), "gate_G": torch.rand(groups * B, 4, generator=gen)}
    return {k: v.to(device) for k, v in f.items()}


def test_settings_make_dyadic_steps():
    t = _trainer(STEP_CASES["ralsgan_batched"])
    assert t.ada.hyper.tolist() == [0.6, 2.0, 48.0, 0.0] and t.ada.state.tolist() == [0.5, 0.0, 0.0, 0.0]
    assert 2 * B / 48.0 == 0.25 and all(s / 12 != 0.6 for s in range(-12, 13))


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_eager_iterations_follow_the_restatement(name):
    """Six free-running iterations: after each, p and the counters are the restatement's fed D's
    own outputs of that step, and what D saw is the gated kernel on the recorded batch under the p
    in force during the step."""
    from relativisticgan_amd import kernels as K
    kw = STEP_CASES[name]
    t = _trainer(kw)
    assert t.aug == 7 and t.ada is not None and t.ada.adaptive and t.batch_D == (name != "sgan_unbatched")
    c = ref.Controller(0.5, 0.6, 2, 48.0)
    recs, ps = [], [0.5]

    def hooks(tag, r):
        if tag == "D":
            recs.append({k: r[k].detach().clone() for k in ("x", "aug", "gate", "x_aug", "x_fake_aug", "y_pred",
                                                              "y_pred_fake")})

    for i in range(1, 7):
        t.iteration(i, hooks=hooks)
        t.flush()
        torch.cuda.synchronize()
        assert len(recs) == i
        r = recs[-1]
        assert r["gate"].shape == (2 * B, 4) and r["aug"].shape == (2 * B, 8)
        in_force = _p(c.p)
        want = K.diffaug(r["x"], r["aug"][:B], 7, gate=r["gate"][:B], p=in_force)
        assert torch.equal(_bits(r["x_aug"]), _bits(want)), (name, i)
        masks = ref.sub_policy(7, r["gate"].cpu().numpy(), c.p)
        for b in range(B):  # ... which is the ungated kernel on each sample with its open groups
            one = K.diffaug(r["x"][b:b + 1], r["aug"][b:b + 1], masks[b])
            assert torch.equal(_bits(r["x_aug"][b:b + 1]), _bits(one)), (name, i, b)
        c.update(r["y_pred"].cpu().numpy(), r["y_pred_fake"].cpu().numpy())
        assert t.ada.state.tolist() == c.state, (name, i)
        ps.append(c.p)
    changes = sum(a != b for a, b in zip(ps, ps[1:]))
    print(f"{name}: p = {ps}")
    assert changes >= 2 and t.ada.state[3].item() == 6.0
    assert "G" in t.last and t.last["G"]["gate"].shape == ((2 if kw["loss_D"] > 4 else 1) * B, 4)
    line = t.log_line(6, 0.0)
    assert line.endswith("ada_p: %.4f r: nan" % c.p) and " loss_G: " in line


def test_diters_update_once_per_D_step():
    t = _trainer(dict(loss_D=7, Diters=2))
    c = ref.Controller(0.5, 0.6, 2, 48.0)

    def hooks(tag, r):
        if tag == "D":
            c.update(r["y_pred"].cpu().numpy(), r["y_pred_fake"].cpu().numpy())

    for i in range(1, 3):
        t.iteration(i, hooks=hooks)
    assert c.calls == 4 and t.ada.state.tolist() == c.state


def _count_calls(policy, kw, ada):
    from relativisticgan_amd import _lib as L
    t = _trainer(kw, policy, ada)
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        t.iteration(1)
        t.flush()
        torch.cuda.synchronize()
    finally:
        L._LIB = real
    return proxy.calls


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_flags_unset_make_no_new_call(name):
    kw = STEP_CASES[name]
    off, aug, ada = _count_calls("", kw, None), _count_calls(POLICY, kw, None), _count_calls(POLICY, kw, ADA)
    fixed = _count_calls(POLICY, kw, dict(rgan_aug_p=0.5))
    assert off.get("rgan_conv_fwd", 0) + off.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    # everything off: no augmentation call of either kind, no statistic
    assert not [k for k in off if k.startswith(("rgan_diffaug", "rgan_ada_"))], off
    # --rgan_diffaug alone: the calls it made before (test_diffaug_gpu's count), none of the new ones
    want = (1 if name != "sgan_unbatched" else 2) + (2 if kw["loss_D"] > 4 else 1) + 1
    assert aug.get("rgan_diffaug", 0) == want and aug.get("rgan_diffaug_workspace", 0) == want, aug
    assert not [k for k in aug if k.startswith(("rgan_diffaug_p", "rgan_ada_"))], aug
    assert {k: v for k, v in aug.items() if not k.startswith("rgan_diffaug")} == off
    # gated: the same calls through the gated entry point, one statistic per D step when adapting
    for calls, updates in ((ada, 1), (fixed, 0)):
        assert calls.get("rgan_diffaug_p", 0) == want and "rgan_diffaug" not in calls, calls
        assert calls.get("rgan_ada_update", 0) == updates and "rgan_ada_adjust" not in calls, calls
        rest = {k: v for k, v in calls.items() if not k.startswith(("rgan_diffaug", "rgan_ada_"))}
        assert rest == off, {k: (off.get(k), rest.get(k)) for k in set(off) | set(rest) if off.get(k) != rest.get(k)}


def test_captured_iteration_keeps_adapting_across_replays():
    """One iteration captured as tests/test_ema_gpu.py captures one and replayed 6 times with new
    inputs: the record's output buffers feed the restatement, p follows it, and the device's call
    counter counts every execution."""
    kw = STEP_CASES["ralsgan_batched"]
    gen = torch.Generator().manual_seed(31)
    t = _trainer(kw, rgan_rng="device")
    feeds = [_feed(7, gen) for _ in range(7)]
    c = ref.Controller(0.5, 0.6, 2, 48.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t.iteration(1, feed=feeds[0])
    torch.cuda.synchronize()
    c.update(t.last["D"]["y_pred"].cpu().numpy(), t.last["D"]["y_pred_fake"].cpu().numpy())
    assert t.ada.state.tolist() == c.state
    static = {k: v.clone() for k, v in feeds[0].items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t.iteration(2, feed=static)
    assert t.ada.state.tolist() == c.state  # a capture runs nothing
    ps = [c.p]
    for j in range(1, 7):
        with torch.cuda.stream(side):
            for k, v in feeds[j].items():
                static[k].copy_(v)
            graph.replay()
        torch.cuda.synchronize()
        rec = t.last["D"]
        c.update(rec["y_pred"].cpu().numpy(), rec["y_pred_fake"].cpu().numpy())
        assert t.ada.state.tolist() == c.state, j
        assert t.ada.state[3].item() == 1.0 + j
        ps.append(c.p)
    print(f"captured: p = {ps}")
    assert len(set(ps)) >= 2


def test_checkpoint_carries_the_probability_and_counters():
    kw = STEP_CASES["ralsgan_batched"]
    gen = torch.Generator().manual_seed(41)
    feeds = [_feed(7, gen) for _ in range(6)]
    ref_keys = {"i", "current_set_images", "G_state", "D_state", "G_optimizer", "D_optimizer", "G_scheduler",
                "D_scheduler", "z_test"}
    off = _trainer(kw, ada=None)
    assert off.ada is None and set(off.state(0)) == ref_keys  # --rgan_diffaug alone: the reference's keys
    whole, first = _trainer(kw), _trainer(kw)
    for i in range(6):
        whole.iteration(i + 1, feed=feeds[i])
    for i in range(3):
        first.iteration(i + 1, feed=feeds[i])
    st = first.state(3, 0)
    assert set(st) == ref_keys | {"ada"} and set(st["ada"]) == {"p", "S", "N", "calls"}
    assert st["ada"]["calls"] == 3.0 and st["ada"]["N"] == float(B)  # one step counted since the adjustment
    path = os.path.join(tempfile.mkdtemp(), "state_01.pth")
    torch.save(st, path)
    resumed = _trainer(kw)
    assert resumed.load(torch.load(path, weights_only=True)) == (3, 0)
    assert resumed.ada.state.tolist() == first.ada.state.tolist() and resumed.ada.calls == 3
    for i in range(3, 6):
        resumed.iteration(i + 1, feed=feeds[i])
    torch.cuda.synchronize()
    assert resumed.ada.state.tolist() == whole.ada.state.tolist()
    assert whole.ada.state[3].item() == 6.0 and resumed.ada.calls == 6
    # a fixed probability is the flag's, and a checkpoint without the key leaves the flags' start
    fixed = _trainer(kw, ada=dict(rgan_aug_p=0.25))
    assert "ada" in fixed.state(0)
    fixed.load(st)
    assert fixed.ada.state.tolist() == [0.25, st["ada"]["S"], st["ada"]["N"], 3.0]
    fresh = _trainer(kw)
    fresh.load({k: v for k, v in st.items() if k != "ada"})
    assert fresh.ada.state.tolist() == [0.5, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------- 5. data parallel
DP_ITERS = 4


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)  # gloo: both ranks on cuda:0, as tests/test_dp_gpu.py runs its world-2 cases
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from relativisticgan_amd import dp
    dp.setup(sync_bn=True)
    try:
        t = _trainer(STEP_CASES["ralsgan_batched"], rgan_rng="host")
        assert t.B == B // world and dp.active()
        ys = []

        def hooks(tag, r):
            if tag == "D":
                ys.append((r["y_pred"].detach().cpu().clone(), r["y_pred_fake"].detach().cpu().clone()))

        states = []
        for i in range(1, 1 + DP_ITERS):
            t.iteration(i, hooks=hooks)
            states.append(t.ada.state.tolist())
        t.flush()
        sd = t.ada.state_dict()  # collective: every rank's pair counts
        torch.save({"ys": ys, "states": states, "calls": t.ada.calls, "sd": sd},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_dp2_ranks_share_one_probability():
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
    c = ref.Controller(0.5, 0.6, 2, 48.0)
    for i in range(DP_ITERS):
        for r in (r0, r1):  # the union of both ranks' outputs of the step
            assert r["ys"][i][0].numel() == B // 2
            c.accumulate(r["ys"][i][0].numpy(), r["ys"][i][1].numpy())
        c.adjust()
        if (i + 1) % 2 == 0:  # after an adjustment every rank holds the whole state
            assert r0["states"][i] == r1["states"][i] == c.state, i
        else:  # between them p and the counter agree; S, N are each rank's own share
            assert r0["states"][i][0] == r1["states"][i][0] == c.p and r0["states"][i][3] == r1["states"][i][3] == i + 1
            assert r0["states"][i][1] + r1["states"][i][1] == c.S and r0["states"][i][2] + r1["states"][i][2] == c.N
    assert r0["states"][-1] == r1["states"][-1] == c.state
    assert r0["calls"] == r1["calls"] == DP_ITERS
    assert r0["sd"] == r1["sd"] == {"p": c.p, "S": float(c.S), "N": float(c.N), "calls": float(DP_ITERS)}
    print(f"dp2: p after each iteration = {[s[0] for s in r0['states']]}")
