"""The WGAN-GP kernels of csrc/heads_optim.hip (rgan_gp_interp, rgan_gp_penalty,
rgan_gp_penalty_backward) against float64 (tests/heads_ref.py ref_gp: the oracle's penalty
expression under autograd) at the shapes and samples where they can go wrong: per = 1, per no
multiple of the block size, several blocks per sample; a zero sample (the kernel's own branch), a
unit basis vector (norm exactly 1), norms of 1e3 and 1e-3 and a random direction of norm 1, where
norm - 1 cancels; n_global above the local batch; an upstream gradient other than 1; in place.

Tolerances: norms 1e-5 relative each; loss 1e-5 * max(1, |ref|); dg per sample b, elementwise,
1e-5 * max(max |ref_b|, 2 lam / n_global * max |g_b| / norm_b) -- the second term is that
sample's gradient scale were its norm off 1 by O(1), which absorbs the fp32 cancellation in
norm - 1 (torch's own fp32 sits at <= 2.1e-7 of it).  Interpolation: elementwise
4 eps32 (|x u| + |xf (1 - u)|), three roundings and that of 1 - u, with or without FMA.
Measured worst errors: profiles/loss_heads_mi355x.txt.
"""
import os

import pytest
import torch

from tests import heads_ref as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
LAM = 10.0
_WORST = {}  # (what, batch, per) -> worst error in units of its bound's scale


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("RGAN_HEADS_REPORT")
    if path and _WORST:
        with open(path, "a") as fh:
            fh.write("# gp: what batch per worst_error (norms, loss, dg: tolerance %g; interp: 4 eps32 = 1)\n" % TOL)
            for (what, batch, per), e in sorted(_WORST.items()):
                fh.write("%-8s %d %-7d %.3e\n" % (what, batch, per, e))


def _note(what, batch, per, err):
    _WORST[(what, batch, per)] = max(_WORST.get((what, batch, per), 0.0), err)


@pytest.mark.parametrize("batch,per", H.GP_SHAPES)
def test_gp_penalty_and_backward(K, batch, per):
    for mult, gscale, start in H.GP_COMBOS:
        n_global = mult * batch
        rows = H.gp_rows(batch, start)
        g_cpu = H.gp_inputs(batch, per, start)
        g = g_cpu.to(DEV)
        where = f"rows {rows} n_global {n_global} gscale {gscale}"
        ref_loss, ref_norms, ref_dg = H.ref_gp(g_cpu.double().reshape(batch, per, 1, 1), LAM, n_global)
        ref_dg = ref_dg.reshape(batch, per) * gscale

        loss, norms, gc = K.gp_penalty(g, LAM, n_global)
        assert gc.data_ptr() == g.data_ptr()
        nerr = ((norms.double().cpu() - ref_norms).abs() / ref_norms.clamp_min(1e-300)).max().item()
        _note("norms", batch, per, nerr)
        assert nerr <= TOL, f"{where}: norms off by {nerr:.2e}"
        lerr = abs(loss.item() - ref_loss.item()) / max(1.0, abs(ref_loss.item()))
        _note("loss", batch, per, lerr)
        assert lerr <= TOL, f"{where}: loss {loss.item()!r} vs {ref_loss.item()!r}"

        # gscale 1 as a device scalar and as "not given"
        gs = None if (gscale == 1.0 and mult == 4) else torch.full((), gscale, device=DEV)
        dg = K.gp_penalty_backward(gc, norms, LAM, n_global, gs)
        assert dg.data_ptr() != g.data_ptr() and torch.equal(g.cpu(), g_cpu)
        inplace = g.clone()
        assert K.gp_penalty_backward(inplace, norms, LAM, n_global, gs, out=inplace) is inplace
        assert torch.equal(inplace, dg), f"{where}: in place differs from out of place"

        d = dg.double().cpu()
        assert torch.isfinite(d).all(), where
        g64 = g_cpu.double()
        for b, row in enumerate(rows):
            if row in ("zero", "basis"):
                assert not d[b].any() and not ref_dg[b].any(), f"{where}: sample {b} ({row}) is not exactly zero"
                continue
            scale = max(ref_dg[b].abs().max().item(),
                        2 * LAM / n_global * g64[b].abs().max().item() / ref_norms[b].item())
            err = (d[b] - ref_dg[b]).abs().max().item() / scale
            _note("dg", batch, per, err)
            assert err <= TOL, f"{where}: sample {b} ({row}) dg off by {err:.2e} of its scale"


_IMAGES = {(1, 1): (1, 1, 1), (3, 7): (7, 1, 1), (8, 768): (3, 16, 16), (5, 1025): (1, 25, 41),
           (4, 12288): (3, 64, 64), (2, 196608): (3, 256, 256)}


@pytest.mark.parametrize("batch,per", H.GP_SHAPES)
def test_gp_interp(K, batch, per):
    shape = (batch,) + _IMAGES[(batch, per)]
    gen = torch.Generator().manual_seed(batch * 1000 + per)
    x_cpu = torch.randn(shape, generator=gen)
    xf_cpu = torch.randn(shape, generator=gen)
    eps = torch.finfo(torch.float32).eps
    # u holds exactly 0 and exactly 1 (both in one u from batch 2 on); None: every u random
    for first in (0.0, 1.0, None):
        u_cpu = torch.rand(batch, 1, 1, 1, generator=gen)
        if first is not None:
            u_cpu[0] = first
            if batch >= 2:
                u_cpu[1] = 1.0 - first
        x, xf, u = x_cpu.to(DEV), xf_cpu.to(DEV), u_cpu.to(DEV)
        xb = K.gp_interp(x, xf, u)
        assert xb.shape == x.shape and xb.is_contiguous()
        u64 = u_cpu.double()
        a, b = x_cpu.double() * u64, xf_cpu.double() * (1 - u64)
        err = ((xb.double().cpu() - (a + b)).abs() / (a.abs() + b.abs()).clamp_min(1e-300)).max().item() / (4 * eps)
        _note("interp", batch, per, err)
        assert err <= 1.0, f"u[0] = {first}: off by {err:.2f} of 4 eps32 (|x u| + |xf (1 - u)|)"
        for row in range(min(batch, 2) if first is not None else 0):
            want = xf if u_cpu[row].item() == 0.0 else x
            assert torch.equal(xb[row], want[row]), f"row {row} with u = {u_cpu[row].item()} is not a copy"
        # a channels-last x and a given out compute the same values
        out = torch.full(shape, float("nan"), device=DEV)
        got = K.gp_interp(x.contiguous(memory_format=torch.channels_last), xf, u, out=out)
        assert got is out and torch.equal(out, xb)
