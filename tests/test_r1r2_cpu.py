"""--rgan_r1 / --rgan_r2 / --rgan_reg_every without a GPU: the flags and their parser errors, the
lazy-regularisation rule, the C-ABI's exports and host-side argument checks (answered before
any launch, so dummy pointers are never read), and the throughput accounting's extra term."""
import ctypes

import pytest
import torch


def test_flags_default_off_and_parser_errors(capsys):
    from relativisticgan_amd.config import parse
    ns = parse([])
    assert (ns.rgan_r1, ns.rgan_r2, ns.rgan_reg_every) == (0.0, 0.0, 1)
    on = parse(["--rgan_r1", "10", "--rgan_r2", "0.5", "--rgan_reg_every", "16"])
    assert (on.rgan_r1, on.rgan_r2, on.rgan_reg_every) == (10.0, 0.5, 16)
    assert parse(["--rgan_r2", "1", "--rgan_reg_every", "4"]).rgan_reg_every == 4
    # they combine with the other penalties and switches
    parse(["--loss_D", "3", "--grad_penalty", "True", "--rgan_r1", "1", "--rgan_diffaug", "color",
           "--rgan_ema_G", "0.9", "--rgan_batch_D", "False", "--rgan_sync_bn", "True"])
    for argv, msg in ((["--rgan_r1", "-1"], "--rgan_r1 must be >= 0"),
                      (["--rgan_r2", "-0.5"], "--rgan_r2 must be >= 0"),
                      (["--rgan_r1", "nan"], "--rgan_r1 must be >= 0"),
                      (["--rgan_r1", "1", "--rgan_reg_every", "0"], "--rgan_reg_every must be >= 1"),
                      (["--rgan_r1", "1", "--rgan_reg_every", "-3"], "--rgan_reg_every must be >= 1"),
                      (["--rgan_reg_every", "4"], "needs --rgan_r1 or --rgan_r2"),
                      (["--rgan_r1", "1", "--rgan_pac", "2"], "not available with --rgan_pac 2"),
                      (["--rgan_r2", "1", "--rgan_script", "GAN_losses_iter_PAC"], "not available with --rgan_pac 2")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert msg in capsys.readouterr().err, argv


def test_make_param_defaults_unchanged():
    """The new flags default to off and no other default moved: every flag of the reference's
    parser keeps the reference's value."""
    from oracle.reference_cpu import make_parser as oracle_parser
    from relativisticgan_amd.config import make_param
    p = make_param()
    assert (p.rgan_r1, p.rgan_r2, p.rgan_reg_every) == (0.0, 0.0, 1)
    paths = ("input_folder", "output_folder", "inception_folder", "extra_folder", "CIFAR10_input_folder")
    for a in oracle_parser()._actions:
        if a.dest != "help" and a.dest not in paths:
            assert getattr(p, a.dest) == a.default, a.dest
    assert (p.rgan_diffaug, p.rgan_ema_G, p.rgan_ema_warmup, p.rgan_rng, p.rgan_sync_bn, p.pac) == \
        ("", 0.0, True, "host", False, 1)
    assert p.rgan_batch_D is None and p.rgan_batch_G is None


def test_trainer_side_validation():
    from relativisticgan_amd.config import validate_reg
    validate_reg(0.0, 0.0, 1)
    validate_reg(1.0, 0.0, 4)
    for bad in ((-1.0, 0.0, 1), (0.0, -1.0, 1), (1.0, 0.0, 0), (0.0, 0.0, 2)):
        with pytest.raises(ValueError):
            validate_reg(*bad)
    with pytest.raises(ValueError):
        validate_reg(1.0, 0.0, 1, pac=2)


@pytest.mark.parametrize("K", [1, 4])
def test_lazy_rule(K):
    """The penalty runs iff i % K == 0, with weight gamma * K; gamma 0 never runs."""
    from relativisticgan_amd.config import reg_weight
    for i in range(9):
        w = reg_weight(i, K, 2.5)
        assert w == (2.5 * K if i % K == 0 else 0.0), (K, i, w)
        assert reg_weight(i, K, 0.0) == 0.0
    # stateless: a run resumed at iteration 6 continues the schedule
    assert [reg_weight(i, 4, 1.0) > 0 for i in range(6, 10)] == [False, False, True, False]


def test_library_exports_and_rejects_malformed_calls():
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    for name in ("rgan_gp_zc_workspace", "rgan_gp_zc_penalty", "rgan_gp_zc_penalty_backward"):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    p = ctypes.c_void_p(0x1000)
    EINVAL = 1001

    def fwd(g=p, batch=6, per=768, n_global=6, sq=p, loss=p, ws=p):
        return lib.rgan_gp_zc_penalty(g, batch, per, 1.0, n_global, sq, loss, ws, None)

    def bwd(g=p, batch=6, per=768, n_global=6, gscale=p, dg=p):
        return lib.rgan_gp_zc_penalty_backward(g, batch, per, 1.0, n_global, gscale, dg, None)

    for call in (fwd, bwd):
        assert call(g=None) == EINVAL
        assert call(batch=0) == EINVAL and call(batch=-2) == EINVAL
        assert call(per=0) == EINVAL and call(per=-16) == EINVAL
        assert call(n_global=5) == EINVAL
        assert call(batch=65536, n_global=65536) == EINVAL  # the stated bound on batch
    assert fwd(sq=None) == EINVAL and fwd(loss=None) == EINVAL and fwd(ws=None) == EINVAL
    assert bwd(dg=None) == EINVAL
    assert lib.rgan_gp_zc_workspace(6, 768) > 0
    assert lib.rgan_gp_zc_workspace(65, 49152) >= 65 * 8
    assert lib.rgan_gp_zc_workspace(0, 768) == 0 and lib.rgan_gp_zc_workspace(6, 0) == 0


def test_ops_listed():
    from relativisticgan_amd import ops
    for name in ("gp_zc_penalty", "gp_zc_penalty_backward"):
        assert name in ops.OPS and hasattr(torch.ops.rgan, name)
        assert f"rgan::{name}" in ops.__doc__


class _T:
    """What conv_flops_per_iteration reads of a trainer (nets built on the CPU, never run)."""

    def __init__(self, **kw):
        from relativisticgan_amd.config import make_param
        from relativisticgan_amd.nets import DCGAN_D, DCGAN_G
        self.p = make_param(image_size=32, batch_size=8, z_size=16, G_h_size=8, D_h_size=8, **kw)
        state = torch.random.get_rng_state()
        self.G, self.D, self.B = DCGAN_G(self.p), DCGAN_D(self.p), 8
        torch.random.set_rng_state(state)


@pytest.mark.parametrize("base", [dict(loss_D=7), dict(loss_D=3), dict(loss_D=1)], ids=lambda d: f"loss_D={d['loss_D']}")
def test_conv_flops_grow_by_the_engine_pass(base):
    from relativisticgan_amd.perf import conv_flops_per_iteration

    def layer_flops(net, shape):  # the accounting's own definition, restated
        out, (B, cin, H, W) = [], shape
        for layer in net._plan:
            g, w = layer.spec.geom, (layer.conv.w if hasattr(layer.conv, "w") else layer.conv.weight)
            cout = w.shape[1] if g.transposed else w.shape[0]
            Ho, Wo = g.out_hw(H, W)
            out.append(2.0 * B * cin * cout * g.k * g.k * (H * W if g.transposed else Ho * Wo))
            cin, H, W = cout, Ho, Wo
        return out

    off = _T(**base)
    fd, fg = layer_flops(off.D, (8, 3, 32, 32)), layer_flops(off.G, (8, 16, 1, 1))
    today = 9 * sum(fd) + 4 * sum(fg) - 2 * fd[0] - fg[0]
    if base["loss_D"] <= 4:
        today -= sum(fd)
    term = 6 * sum(fd) - fd[0] - 3 * fd[-1]
    if base["loss_D"] == 3:
        today += term
    f0 = conv_flops_per_iteration(off)
    assert f0 == today
    assert conv_flops_per_iteration(_T(rgan_r1=10.0, **base)) == f0 + term
    assert conv_flops_per_iteration(_T(rgan_r2=1.0, **base)) == f0 + term
    assert conv_flops_per_iteration(_T(rgan_r1=10.0, rgan_r2=1.0, **base)) == f0 + term + term
    assert conv_flops_per_iteration(_T(rgan_r1=10.0, rgan_reg_every=4, **base)) == f0 + term / 4
    assert conv_flops_per_iteration(_T(rgan_r1=10.0, rgan_r2=1.0, rgan_reg_every=4, **base)) == f0 + term / 4 + term / 4
