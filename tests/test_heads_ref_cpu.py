"""The float64 head / penalty references and their input generators (tests/heads_ref.py) keep
the conditions the GPU tests rely on, and the head wrappers of kernels.py reject arguments the
kernels would read or write out of bounds.  CPU only: no library call is made."""
import pytest
import torch

from oracle.reference_cpu import head_fake, head_G, head_real, head_relativistic_D
from tests import heads_ref as H

KINDS = range(1, 9)


@pytest.mark.parametrize("kind", KINDS)
def test_generators_keep_their_conditions(kind):
    for regime in H.regimes(kind):
        for n in H.ALL_SIZES:
            r, f = H.gen(regime, kind, n)
            r2, f2 = H.gen(regime, kind, n)
            assert torch.equal(r, r2) and torch.equal(f, f2), "seeded"
            for t in (r, f):
                assert t.dtype == torch.float32 and t.shape == (n,) and torch.isfinite(t).all()
            if kind == 1:
                lo, hi = (0.01, 0.99) if regime == "typical" else (0.0, 1.0)
                assert min(r.min(), f.min()) >= lo - 1e-7 and max(r.max(), f.max()) <= hi + 1e-7
            values = {"wide": H.WIDE_PLANTS, "bce_edge": H.BCE_PLANTS}.get(regime)
            if values:
                for which, t in enumerate((r, f)):
                    want = H.planted(values, n, which)
                    assert len(want) == min(n, len(values))
                    if n >= len(values):
                        assert set(want) == set(values)
                    for v in want:
                        assert (t == torch.tensor(v, dtype=torch.float32)).any(), (regime, n, which, v)
            if regime == "offset" and n >= 1023:
                assert abs(r.mean().item() - 50) < 0.2 and abs(f.mean().item() - 49.5) < 0.2
            if kind in H.HINGE:
                mr, mf = H.kink_margins(kind, r.double(), f.double())
                assert min(mr.min().item(), mf.min().item()) >= H.KINK_NEAR, (regime, n)


def test_bce_edge_plants_are_the_fp32_edges():
    """2^-24 and 1 - 2^-24 are float32 numbers (the neighbours of 0's scale and of 1), 1e-30 is a
    normal float32 below the 1e-12 denominator clamp."""
    for v in (2.0 ** -24, 1.0 - 2.0 ** -24):
        assert torch.tensor(v, dtype=torch.float32).double().item() == v
    assert 1.2e-38 < torch.tensor(1e-30, dtype=torch.float32).item() < 1e-12
    assert torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).double().item() == 1.0 - 2.0 ** -24


@pytest.mark.parametrize("kind", H.HINGE)
def test_kink_inputs_are_exact_in_fp32(kind):
    r, f = H.gen("kink", kind, H.KINK_N)
    assert r.shape == f.shape == (H.KINK_N,)
    d = H.KINK_STEP
    for t, kinks in zip((r, f), H.kink_points(kind)):
        t64 = t.double()
        assert t64.abs().max() <= 8 and torch.equal(t64, (t64 / d).round() * d)
        for k in kinks:
            for s in (0, -1, 1):
                assert (t64 == k + s * d).any(), (kind, k, s)
    if kind == 8:
        assert r.double().mean().item() == 0.25 and f.double().mean().item() == -0.5
    mr, mf = H.kink_margins(kind, r.double(), f.double())
    for m in (mr, mf):  # every kink has an element on it and one 2^-9 to either side
        for row in m:
            assert (row == 0).sum() >= 1 and (row == d).sum() >= 2
    for k, side in H.CASES:
        if k != kind:
            continue
        need_r, need_f = H.needs(kind, side)
        loss64, dr64, df64 = H.ref_head(kind, side, r.double() if need_r else None, f.double() if need_f else None)
        # the oracle's expression in float32 (ref_head keeps the dtype it is given)
        loss32, dr32, df32 = H.ref_head(kind, side, r if need_r else None, f if need_f else None)
        assert loss32.dtype == torch.float32 and loss32.double().item() == loss64.item()
        for a, b in ((dr32, dr64), (df32, df64)):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a.double(), b)


def test_ref_head_side_mapping():
    """ref_head is the oracle's four functions under the (kind, side) mapping of the C ABI."""
    torch.manual_seed(0)
    r, f = torch.randn(9, dtype=torch.float64), torch.randn(9, dtype=torch.float64)
    p = torch.rand(9, dtype=torch.float64)
    ones, zeros = torch.ones(9, dtype=torch.float64), torch.zeros(9, dtype=torch.float64)
    for kind in (1, 2, 3, 4):
        t = p if kind == 1 else r
        assert H.ref_head(kind, 0, t, None)[0] == head_real(kind, t, ones)
        assert H.ref_head(kind, 1, None, t)[0] == head_fake(kind, t, zeros)
        assert H.ref_head(kind, 2, None, t)[0] == head_G(kind, t, None, ones, zeros)
        assert H.ref_head(kind, 0, t, None)[2] is None and H.ref_head(kind, 1, None, t)[1] is None
    for kind in (5, 6, 7, 8):
        assert H.ref_head(kind, 0, r, f)[0] == head_relativistic_D(kind, r, f, ones, zeros)
        assert H.ref_head(kind, 2, r, f)[0] == head_G(kind, f, r, ones, zeros)
        with pytest.raises(ValueError):
            H.ref_head(kind, 1, r, f)


@pytest.mark.parametrize("batch,per", H.GP_SHAPES)
def test_ref_gp_is_the_closed_form(batch, per):
    seen = set()
    for mult, _, start in H.GP_COMBOS:
        rows = H.gp_rows(batch, start)
        seen.update(rows)
        g = H.gp_inputs(batch, per, start)
        assert g.dtype == torch.float32 and g.shape == (batch, per) and torch.isfinite(g).all()
        g64 = g.double()
        loss, norms, dg = H.ref_gp(g64.reshape(batch, per, 1, 1), 10.0, mult * batch)
        closs, cnorms, cdg = H.gp_closed_form(g64.reshape(batch, per, 1, 1), 10.0, mult * batch)
        assert abs(loss.item() - closs.item()) <= 1e-12 * max(1.0, abs(closs.item()))
        assert torch.allclose(norms, cnorms, rtol=1e-13, atol=0)
        for b, row in enumerate(rows):
            scale = max(cdg[b].abs().max().item(), 2 * 10.0 / (mult * batch))
            assert (dg[b] - cdg[b]).abs().max().item() <= 1e-12 * scale, (row, b)
            n = norms[b].item()
            if row == "zero":
                assert n == 0 and not dg[b].any()
            elif row == "basis":
                assert n == 1 and (g64[b] != 0).sum() == 1 and not dg[b].any()
            elif row == "unit":
                assert abs(n - 1) <= 1e-6
            elif row == "big":
                assert abs(n - 1e3) <= 1e-3
            elif row == "small":
                assert abs(n - 1e-3) <= 1e-9
    if batch >= 2:
        assert seen == set(H.GP_ROWS)


# ---------------------------------------------------------------- wrapper validation (kernels.py)
def _t(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


def _bad_calls():
    from relativisticgan_amd import kernels as K
    strided = _t(16)[::2]
    assert strided.numel() == 8 and not strided.is_contiguous()
    half, dbl = torch.float16, torch.float64
    calls = {
        # rgan_loss_head
        "head: f shorter than r": ("f", lambda: K.loss_head(7, 0, _t(8), _t(7))),
        "head: f longer than r": ("f", lambda: K.loss_head(7, 0, _t(8), _t(9))),
        "head: strided r": ("r", lambda: K.loss_head(7, 0, strided, _t(8))),
        "head: strided f": ("f", lambda: K.loss_head(2, 1, None, strided)),
        "head: float64 r": ("r", lambda: K.loss_head(2, 0, _t(8, dbl), None)),
        "head: float16 f": ("f", lambda: K.loss_head(7, 2, _t(8), _t(8, half))),
        "head: dr of another size": ("dr", lambda: K.loss_head(7, 0, _t(8), _t(8), dr=_t(7))),
        "head: strided df": ("df", lambda: K.loss_head(7, 0, _t(8), _t(8), df=strided)),
        "head: float64 dr": ("dr", lambda: K.loss_head(7, 0, _t(8), _t(8), dr=_t(8, dbl))),
        "head: n = 0": ("n", lambda: K.loss_head(2, 0, _t(0), None)),
        "head: n above the maximum": ("n", lambda: K.loss_head(2, 0, _t(65537), None)),
        # rgan_loss_head_pair
        "pair: f shorter than r": ("f", lambda: K.loss_head_pair(2, _t(8), _t(7))),
        "pair: strided r": ("r", lambda: K.loss_head_pair(2, strided, _t(8))),
        "pair: float64 f": ("f", lambda: K.loss_head_pair(2, _t(8), _t(8, dbl))),
        "pair: dr of another size": ("dr", lambda: K.loss_head_pair(2, _t(8), _t(8), dr=_t(9))),
        "pair: strided df": ("df", lambda: K.loss_head_pair(2, _t(8), _t(8), df=strided)),
        "pair: n = 0": ("n", lambda: K.loss_head_pair(2, _t(0), _t(0))),
        "pair: n above the maximum": ("n", lambda: K.loss_head_pair(2, _t(65537), _t(65537))),
        # rgan_loss_head_joint
        "joint: odd y": ("y", lambda: K.loss_head_joint(7, _t(9))),
        "joint: strided y": ("y", lambda: K.loss_head_joint(7, strided)),
        "joint: float64 y": ("y", lambda: K.loss_head_joint(7, _t(8, dbl))),
        "joint: empty y": ("n", lambda: K.loss_head_joint(7, _t(0))),
        "joint: n above the maximum": ("n", lambda: K.loss_head_joint(7, _t(2 * 65537))),
        "joint: out of another size": ("out", lambda: K.loss_head_joint(7, _t(8), out=_t(4))),
        "joint: strided out": ("out", lambda: K.loss_head_joint(7, _t(8), out=strided)),
        "joint: float64 out": ("out", lambda: K.loss_head_joint(7, _t(8), out=_t(8, dbl))),
        # rgan_loss_head_dist
        "dist: f shorter than r": ("f", lambda: K.loss_head_dist(7, 0, 0, _t(8), _t(7), 16)),
        "dist: strided r": ("r", lambda: K.loss_head_dist(7, 0, 0, strided, _t(8), 16)),
        "dist: float64 f": ("f", lambda: K.loss_head_dist(2, 1, 0, None, _t(8, dbl), 16)),
        "dist: n = 0": ("n", lambda: K.loss_head_dist(2, 0, 0, _t(0), None, 16)),
        "dist: n above the maximum": ("n", lambda: K.loss_head_dist(2, 0, 0, _t(65537), None, 1 << 20)),
        "dist: empty gsum, heads 1-5": ("gsum", lambda: K.loss_head_dist(5, 0, 2, _t(8), _t(8), 16, gsum=_t(0))),
        "dist: one-float gsum in phase 1": ("gsum", lambda: K.loss_head_dist(6, 0, 1, _t(8), _t(8), 16, gsum=_t(1))),
        "dist: two-float gsum in phase 2": ("gsum", lambda: K.loss_head_dist(7, 0, 2, _t(8), _t(8), 16, gsum=_t(2))),
        "dist: five-float gsum in phase 2": ("gsum", lambda: K.loss_head_dist(8, 2, 2, _t(8), _t(8), 16, gsum=_t(5))),
        "dist: strided gsum": ("gsum", lambda: K.loss_head_dist(7, 0, 2, _t(8), _t(8), 16, gsum=_t(12)[::2])),
        "dist: float64 gsum": ("gsum", lambda: K.loss_head_dist(7, 0, 2, _t(8), _t(8), 16, gsum=_t(6, dbl))),
    }
    return calls


_BAD = sorted(_bad_calls())


@pytest.mark.parametrize("case", _BAD)
def test_head_wrappers_reject(case, monkeypatch):
    """Each bad argument raises RganError naming it, before the library is touched."""
    from relativisticgan_amd import _lib as L

    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "lib", no_lib)
    monkeypatch.setattr(L, "ptr", lambda t: no_lib())
    name, call = _bad_calls()[case]
    with pytest.raises(L.RganError) as e:
        call()
    msg = str(e.value)
    assert msg.split(":")[0] in ("loss_head", "loss_head_pair", "loss_head_joint", "loss_head_dist")
    assert f": {name} " in msg, msg
