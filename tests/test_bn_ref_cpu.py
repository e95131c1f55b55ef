"""tests/bn_ref.py (the float64 reference of the first-order BatchNorm / activation kernel tests)
held to torch itself: float64 F.batch_norm(training=True) + torch.autograd.grad and
torch.nn.BatchNorm2d, to 1e-12 relative -- and the conditions its input generators state, so
tests/test_bn_first_order_gpu.py compares every element and masks none.  No GPU.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

TOL = 1e-12
TORCH_ACT = {"none": lambda t: t, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, R.ALPHA), "tanh": torch.tanh,
             "sigmoid": torch.sigmoid, "selu": F.selu}


def _rel(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _nchw(m, B):
    """[P][C] -> [B][C][P/B][1]."""
    P, C = m.shape
    return m.view(B, P // B, 1, C).permute(0, 3, 1, 2)


def _autograd(y, gamma, beta, da, name):
    y64 = _nchw(y.double(), 2).clone().requires_grad_(True)
    g64, b64 = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    out = TORCH_ACT[name](F.batch_norm(y64, None, None, g64, b64, training=True, eps=R.EPS))
    dy, dg, db = torch.autograd.grad(out, [y64, g64, b64], _nchw(da.double(), 2))
    P, C = y.shape
    return out.permute(0, 2, 3, 1).reshape(P, C), dy.permute(0, 2, 3, 1).reshape(P, C), dg, db


@pytest.mark.parametrize("name", R.ACTS)
def test_forward_backward_match_autograd(name):
    d = R.inputs(48, 10, R.mixes(10)[0][1], seed=1)
    out, dy, dg, db = _autograd(d["y"], d["gamma"], d["beta"], d["da"], name)
    mean, inv = R.stats(d["y"])
    assert _rel(R.forward(d["y"], mean, inv, d["gamma"], d["beta"], name), out) < TOL
    b = R.backward(d["da"], d["y"], mean, inv, d["gamma"], d["beta"], name)
    assert _rel(b["dy"], dy) < TOL and _rel(b["dgamma"], dg) < TOL and _rel(b["dbeta"], db) < TOL
    b2 = R.backward(d["da"], d["y"], mean, inv, d["gamma"], d["beta"], name, add=d["add"])
    assert _rel(b2["dy"], dy + d["add"].double()) < TOL
    # gamma / beta absent = 1 / 0
    one, zero = torch.ones(10), torch.zeros(10)
    out1, dy1, _, _ = _autograd(d["y"], one, zero, d["da"], name)
    assert _rel(R.forward(d["y"], mean, inv, None, None, name), out1) < TOL
    assert _rel(R.backward(d["da"], d["y"], mean, inv, None, None, name)["dy"], dy1) < TOL


@pytest.mark.parametrize("name", R.ACTS)
def test_two_shards_with_summed_sums_are_the_whole_batch(name):
    """P_global = 2P: each shard's dy with the two shards' sums added is the whole batch's dy;
    the shards' affine gradients add up to the whole batch's."""
    d = R.inputs(48, 10, R.mixes(10)[0][1], seed=2)
    mean, inv = R.stats(d["y"])
    whole = R.backward(d["da"], d["y"], mean, inv, d["gamma"], d["beta"], name)
    h = [slice(0, 24), slice(24, 48)]
    loc = [R.backward(d["da"][s], d["y"][s], mean, inv, d["gamma"], d["beta"], name) for s in h]
    tot = loc[0]["sums"] + loc[1]["sums"]
    assert _rel(tot, whole["sums"]) < TOL
    for s, lo in zip(h, loc):
        sh = R.backward(d["da"][s], d["y"][s], mean, inv, d["gamma"], d["beta"], name, P_global=48, sums=tot)
        assert _rel(sh["dy"], whole["dy"][s]) < TOL
    assert _rel(loc[0]["dgamma"] + loc[1]["dgamma"], whole["dgamma"]) < TOL
    assert _rel(loc[0]["dbeta"] + loc[1]["dbeta"], whole["dbeta"]) < TOL


@pytest.mark.parametrize("name", ["lrelu", "tanh"])
def test_two_segments_match_two_autograd_calls(name):
    d = R.inputs(64, 10, R.mixes(10)[0][1], seed=3, nseg=2)
    halves = [slice(0, 32), slice(32, 64)]
    seg_stats = [R.stats(d["y"][s]) for s in halves]
    got = R.backward_segments(d["da"], d["y"], seg_stats, d["gamma"], d["beta"], name)
    dg, db = 0, 0
    for s in halves:
        _, dy, g1, b1 = _autograd(d["y"][s], d["gamma"], d["beta"], d["da"][s], name)
        assert _rel(got["dy"][s], dy) < TOL
        dg, db = dg + g1, db + b1
    assert _rel(got["dgamma"], dg) < TOL and _rel(got["dbeta"], db) < TOL


@pytest.mark.parametrize("momentum", [0.1, 1.0, 0.0])
def test_running_statistics_match_batchnorm2d(momentum):
    d = R.inputs(48, 10, R.mixes(10)[0][1], seed=4)
    bn = torch.nn.BatchNorm2d(10, eps=R.EPS, momentum=momentum).double()
    g = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(10, generator=g).double(), torch.rand(10, generator=g).double() + 0.5
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn(_nchw(d["y"].double(), 2))
    n, mean, M2 = R.moments(d["y"])
    rm, rv, nbt = R.running_update(rm0, rv0, torch.zeros((), dtype=torch.long), n, mean, M2, momentum,
                                   dtype=torch.float64)
    assert _rel(rm, bn.running_mean) < TOL and _rel(rv, bn.running_var) < TOL
    assert int(nbt) == int(bn.num_batches_tracked) == 1
    # the fp32 statement differs from it by fp32 roundings only; absent buffers stay absent
    rm32, rv32, none = R.running_update(rm0.float(), rv0.float(), None, n, mean, M2, momentum)
    assert rm32.dtype == torch.float32 and _rel(rm32, rm) < 1e-6 and _rel(rv32, rv) < 1e-6 and none is None
    assert R.running_update(None, None, None, n, mean, M2, momentum) == (None, None, None)


def test_running_variance_of_a_single_row_is_the_biased_one():
    """n == 1 (torch refuses it in training): the kernels use the biased variance, 0."""
    y = torch.tensor([[1.5, -2.0]])
    n, mean, M2 = R.moments(y)
    _, rv, _ = R.running_update(None, torch.ones(2), None, n, mean, M2, 0.25)
    assert n == 1 and torch.equal(M2, torch.zeros(2, dtype=torch.float64)) and torch.equal(rv, torch.full((2,), 0.75))


@pytest.mark.parametrize("sizes", [(48,), (1, 47), (0, 1, 17, 30), (5, 0, 1, 9, 3, 20, 8, 2)])
def test_rank_merge_is_the_concatenated_batch(sizes):
    d = R.inputs(48, 10, R.mixes(10)[1][1], seed=6)
    shards, p = [], 0
    for s in sizes:
        shards.append(R.moments(d["y"][p:p + s]) if s else (0, torch.full((10,), 1e30), torch.full((10,), -1e30)))
        p += s
    N, mean, M2 = R.merge(shards)
    n, m, s2 = R.moments(d["y"])
    assert N == n and _rel(mean, m) < TOL and _rel(M2, s2) < 1e-9  # M2 of a mean-1e3 channel: conditioning 1e6 * 2^-53


def test_segment_sums_are_the_moments():
    d = R.inputs(192, 10, R.mixes(10)[0][1], seed=7)
    for sr in (64, 2):
        part = R.segment_sums(d["y"], sr)
        assert part.shape == (192 // sr, 2, 10) and part.dtype == torch.float64
        S1, S2 = part[:, 0].sum(0), part[:, 1].sum(0)
        y64 = d["y"].double()
        assert _rel(S1, y64.sum(0)) < TOL and _rel(S2, (y64 * y64).sum(0)) < TOL
        n, mean, M2 = R.moments(d["y"])
        assert _rel(S1 / n, mean) < TOL and _rel(S2 - S1 * S1 / n, M2) < 1e-9
    # a segment is its own rows
    assert _rel(R.segment_sums(d["y"], 64)[1, 0], d["y"][64:128].double().sum(0)) < TOL


def test_activation_backward_from_output():
    """act' through the output equals act' through the input, and at an output of exactly 0 it is
    torch's: ReLU' = 0, LeakyReLU' = alpha, SELU' = scale * alpha; tanh' (+-1) = 0."""
    z = torch.linspace(-4, 4, 161, dtype=torch.float64)
    z = z[z.abs() > 1e-9]
    for name in R.ACTS:
        assert _rel(R.act_grad_from_out(R.act(z, name), name), R.act_grad(z, name)) < 1e-11
        x = z.clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(TORCH_ACT[name](x).sum(), x)
        assert _rel(R.act_grad(z, name), gr) < TOL
    zero = torch.zeros(1, dtype=torch.float64)
    for name, want in (("relu", 0.0), ("lrelu", R.ALPHA), ("selu", R.SELU_SCALE * R.SELU_ALPHA), ("sigmoid", 0.0)):
        assert R.act_grad_from_out(zero, name).item() == pytest.approx(want, abs=1e-15)
        if name != "sigmoid":   # torch's own backward through an output of exactly 0
            x = zero.clone().requires_grad_(True)
            (gr,) = torch.autograd.grad(TORCH_ACT[name](x), x)
            assert gr.item() == pytest.approx(want, abs=1e-15)
    assert R.act_grad_from_out(torch.tensor([1.0, -1.0], dtype=torch.float64), "tanh").abs().max().item() == 0.0


def test_small_ops():
    t = torch.randn(7, 5)
    assert _rel(R.channel_sum(t), t.double().sum(0)) < TOL and _rel(R.scale(t, 0.3), t.double() * 0.3) < TOL


def test_generators_leave_no_element_near_a_kink():
    """Every backward input of the GPU module -- bn_ref.bwd_inputs serves both modules the same
    seeded tensors -- with and without gamma / beta: min |z| >= KINK = 1e-3 in float64 with the
    batch statistics of each segment, and |z| above the a-priori fp32 error of the kernels' fused
    affine form (min_margin > 0), so no fp32 evaluation of z takes the other branch of ReLU' /
    LeakyReLU' and the share of masked elements is 0 by construction.  bwd_inputs asserts this
    itself (here it is restated); every regime is present."""
    seen = set()
    for P, C, nseg in R.all_bwd_cases():
        for mix in range(len(R.bwd_mixes(P, C, nseg))):
            for affine_on in (True, False) if (nseg == 1 and mix == 0 and (P, C, nseg) in R.BWD_CASES) else (True,):
                label, kinds, d = R.bwd_inputs(P, C, nseg, mix, affine_on=affine_on)
                Ps = P // nseg
                for k in range(nseg):
                    ys = d["y"][k * Ps:(k + 1) * Ps]
                    z = R.pre_act(ys, *R.stats(ys), d["gamma"], d["beta"])
                    assert z.abs().min().item() >= R.KINK, (P, C, nseg, label)
                assert R.min_margin(d["y"], d["gamma"], d["beta"], nseg=nseg) > 0, (P, C, nseg, label)
                seen.update(kinds)
    assert seen == set(R.WELL + R.OFFSET)


def test_assert_off_kink_refuses_an_element_on_the_kink():
    d = R.inputs(64, 6, R.mixes(6)[0][1], seed=9)
    R.assert_off_kink(d["y"], d["gamma"], d["beta"])
    y = d["y"].clone()
    for _ in range(30):   # z[5, 0] -> 0 (the element moves its own statistics: a fixed point)
        mean, inv = R.stats(y)
        y[5, 0] = (mean[0] - d["beta"][0].double() / (d["gamma"][0].double() * inv[0])).float()
    assert R.pre_act(y, *R.stats(y), d["gamma"], d["beta"])[5, 0].abs().item() < R.KINK
    with pytest.raises(AssertionError):
        R.assert_off_kink(y, d["gamma"], d["beta"])


def test_generator_regimes():
    g = torch.Generator().manual_seed(0)
    P = 4096
    ch = {k: R.channel(k, P, g).double() for k in R.WELL + R.OFFSET}
    assert ch["b0"].var().item() == 0 and ch["b1"].var().item() == 0 and ch["b1"][0].item() == 2.5
    assert abs(ch["c"].mean().item() - 1e3) < 0.1 and abs(ch["c"].std().item() - 1) < 0.1
    assert ch["d0"].var().item() < 0.01 * R.EPS and ch["d1"].var().item() < 0.01 * R.EPS
    rest = ch["e"][1:]
    assert abs(ch["e"][0].item() - rest.mean().item()) > 45 * rest.std().item()
    assert 5e3 < ch["f"].abs().mean().item() < 2e4
    for k in R.WELL:
        mean, inv = R.stats(ch[k][:, None])
        assert R.conditioning(mean, inv).item() < R.COND_MAX, k
    for k in R.OFFSET:
        mean, inv = R.stats(ch[k][:, None])
        assert R.conditioning(mean, inv).item() > R.COND_MAX, k
