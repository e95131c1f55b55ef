"""Every entry point of the eight --loss_D heads (csrc/heads_optim.hip) against the float64
oracle expressions of tests/heads_ref.py, at the sizes and values where such kernels go wrong:
one element, wave and block boundaries, the 65536 maximum; saturated logits, BCE at exactly 0
and 1, a common offset of 50, and elements on and next to every hinge kink.

Tolerance (every comparison is over all elements, none masked):
  loss                    |loss - ref| <= 1e-5 * max(1, |ref|)
  gradients, heads 2-8    max_i |d_i - ref_i| <= 1e-5 * max_i |ref_i|
  gradients, head 1       |d_i - ref_i| <= 1e-5 * |ref_i| + 1e-5 / n_global for every i
                          (BCE gradients span 1/n .. 1e12/n)
1e-5 is at least 6x what torch's float32 evaluation of the oracle expressions itself loses
against float64 in these regimes (worst 1.6e-6 on a loss, 8e-7 of the largest gradient); the
kernels' measured worst errors are in profiles/loss_heads_mi355x.txt.  On the ``kink`` inputs
every intermediate is a float32 number, so the kernels must equal float64 exactly.

With RGAN_HEADS_REPORT=<file> the worst error per (entry form, head, regime), in units of the
tolerance's right-hand side scale, is written there when the module finishes.
"""
import os

import pytest
import torch

from tests import heads_ref as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
_WORST = {}   # (form, kind, regime) -> [worst loss error, worst gradient error]
_REFS = {}    # (regime, kind, n, side) -> float64 reference, computed once


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
            fh.write("# form kind regime worst_loss_error worst_gradient_error (tolerance %g)\n" % TOL)
            for (form, kind, regime), (el, eg) in sorted(_WORST.items()):
                fh.write("%-14s %d %-8s %.3e %.3e\n" % (form, kind, regime, el, eg))


def _inputs(regime, kind, n):
    r, f = H.gen(regime, kind, n)
    return r.to(DEV), f.to(DEV)


def _ref(regime, kind, n, side):
    key = (regime, kind, n, side)
    if key not in _REFS:
        r, f = H.gen(regime, kind, n)
        need_r, need_f = H.needs(kind, side)
        _REFS[key] = H.ref_head(kind, side, r.double() if need_r else None, f.double() if need_f else None)
    return _REFS[key]


def _note(form, kind, regime, which, err):
    w = _WORST.setdefault((form, kind, regime), [0.0, 0.0])
    w[which] = max(w[which], err)


def _loss_close(form, kind, regime, loss, ref, where=""):
    loss = loss.item() if torch.is_tensor(loss) else loss
    ref = ref.item() if torch.is_tensor(ref) else ref
    assert loss == loss and abs(loss) != float("inf"), f"{form} {where}: loss {loss}"
    err = abs(loss - ref) / max(1.0, abs(ref))
    _note(form, kind, regime, 0, err)
    assert err <= TOL, f"{form} head {kind} {regime} {where}: loss {loss!r} vs {ref!r} ({err:.2e})"


def _grad_close(form, kind, regime, d, ref, n_global, where="", gain=1.0):
    """d (device float32) against gain * ref (float64), elementwise."""
    d = d.detach().double().cpu().reshape(-1)
    ref = ref.reshape(-1) * gain
    assert d.shape == ref.shape, f"{form} {where}: {tuple(d.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(d).all(), f"{form} head {kind} {regime} {where}: non-finite gradient"
    diff = (d - ref).abs()
    if kind == 1:
        bound = ref.abs() + abs(gain) / n_global
        err = (diff / bound).max().item()
    else:
        scale = ref.abs().max().item()
        err = diff.max().item() / scale if scale > 0 else (0.0 if diff.max().item() == 0 else float("inf"))
    _note(form, kind, regime, 1, err)
    assert err <= TOL, f"{form} head {kind} {regime} {where}: gradient off by {err:.2e} of its scale"


# ---------------------------------------------------------------- rgan_loss_head
@pytest.mark.parametrize("kind,side", H.CASES)
def test_loss_head(K, kind, side):
    need_r, need_f = H.needs(kind, side)
    for regime in H.regimes(kind):
        for n in H.SIZES:
            r, f = _inputs(regime, kind, n)
            r, f = (r if need_r else None), (f if need_f else None)
            ref, rdr, rdf = _ref(regime, kind, n, side)
            loss, dr, df = K.loss_head(kind, side, r, f)
            where = f"side {side} n {n}"
            _loss_close("head", kind, regime, loss, ref, where)
            assert (dr is None) == (not need_r) and (df is None) == (not need_f)
            if need_r:
                _grad_close("head", kind, regime, dr, rdr, n, where + " dr")
            if need_f:
                _grad_close("head", kind, regime, df, rdf, n, where + " df")
            # the nullable outputs: what remains is unchanged
            for ndr, ndf in ((False, True), (True, False), (False, False)):
                l2, dr2, df2 = K.loss_head(kind, side, r, f, need_dr=ndr, need_df=ndf)
                assert torch.equal(l2, loss), where
                assert dr2 is None if not (ndr and need_r) else torch.equal(dr2, dr), where
                assert df2 is None if not (ndf and need_f) else torch.equal(df2, df), where


# ---------------------------------------------------------------- rgan_loss_head_pair
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_loss_head_pair(K, kind):
    for regime in H.regimes(kind):
        for n in H.SIZES:
            r, f = _inputs(regime, kind, n)
            real, rdr, _ = _ref(regime, kind, n, 0)
            fake, _, rdf = _ref(regime, kind, n, 1)
            where = f"n {n}"
            loss3, dr, df = K.loss_head_pair(kind, r, f)
            for got, want in zip(loss3.tolist(), (real, fake, real + fake)):
                _loss_close("pair", kind, regime, got, want, where)
            _grad_close("pair", kind, regime, dr, rdr, n, where + " dr")
            _grad_close("pair", kind, regime, df, rdf, n, where + " df")
            # the two halves of one [2n] buffer, as _HeadCat hands them over (odd n: df starts
            # at an odd element)
            buf = torch.full((2 * n,), float("nan"), device=DEV)
            l2, dr2, df2 = K.loss_head_pair(kind, r, f, dr=buf[:n], df=buf[n:])
            assert torch.equal(l2, loss3) and torch.equal(buf, torch.cat([dr, df])), where
            assert dr2.data_ptr() == buf.data_ptr() and df2.data_ptr() == buf[n:].data_ptr()
            l3, dr3, df3 = K.loss_head_pair(kind, r, f, need_dr=False)
            assert dr3 is None and torch.equal(l3, loss3) and torch.equal(df3, df), where
            l4, dr4, df4 = K.loss_head_pair(kind, r, f, need_df=False)
            assert df4 is None and torch.equal(l4, loss3) and torch.equal(dr4, dr), where


# ---------------------------------------------------------------- rgan_loss_head_joint
@pytest.mark.parametrize("kind", [5, 6, 7, 8])
def test_loss_head_joint(K, kind):
    for regime in H.regimes(kind):
        for n in H.SIZES:
            r, f = _inputs(regime, kind, n)
            ref, _, rdf = _ref(regime, kind, n, 2)
            y = torch.cat([f, r])
            # a half the kernel left unwritten would keep its NaN
            dy = torch.full((2 * n,), float("nan"), device=DEV)
            loss, out = K.loss_head_joint(kind, y, out=dy)
            where = f"n {n}"
            assert out is dy
            _loss_close("joint", kind, regime, loss, ref, where)
            _grad_close("joint", kind, regime, dy[:n], rdf, n, where)
            assert not dy[n:].any(), f"head {kind} {regime} {where}: the no-grad half is not zero"
            loss2, dy2 = K.loss_head_joint(kind, y)
            assert torch.equal(loss2, loss) and torch.equal(dy2, dy), where


# ---------------------------------------------------------------- rgan_loss_head_dist
def _dist(K, kind, side, shards, n_global):
    """The three-phase head over shards = [(r_k, f_k)] on one device: the sums of each phase
    added in fp32 on the device as dp.all_reduce_sum would.  Returns (losses per shard, dr, df)."""
    s0 = sum(K.loss_head_dist(kind, side, 0, r, f, n_global)[0] for r, f in shards)
    if kind >= 6:
        g = s0[:2].clone()
        s1 = sum(K.loss_head_dist(kind, side, 1, r, f, n_global, gsum=g)[0] for r, f in shards)
        g = torch.cat([g, s1])
    else:
        g = s0[:1].clone()
    outs = [K.loss_head_dist(kind, side, 2, r, f, n_global, gsum=g) for r, f in shards]
    cat = lambda i: None if outs[0][i] is None else torch.cat([o[i] for o in outs])  # noqa: E731
    return [o[1] for o in outs], cat(2), cat(3)


def _split(t, sizes):
    return [None] * len(sizes) if t is None else list(torch.split(t, list(sizes)))


@pytest.mark.parametrize("kind,side", H.CASES)
def test_loss_head_dist(K, kind, side):
    need_r, need_f = H.needs(kind, side)
    for regime in H.regimes(kind):
        for sizes in H.DIST_SPLITS:
            ng = sum(sizes)
            r, f = _inputs(regime, kind, ng)
            r, f = (r if need_r else None), (f if need_f else None)
            shards = [(a.clone() if a is not None else None, b.clone() if b is not None else None)
                      for a, b in zip(_split(r, sizes), _split(f, sizes))]
            losses, dr, df = _dist(K, kind, side, shards, ng)
            ref, rdr, rdf = _ref(regime, kind, ng, side)
            where = f"side {side} shards {len(sizes)} of {ng}"
            for loss in losses:
                assert torch.equal(loss, losses[0])
            _loss_close("dist", kind, regime, losses[0], ref, where)
            if need_r:
                _grad_close("dist", kind, regime, dr, rdr, ng, where + " dr")
            if need_f:
                _grad_close("dist", kind, regime, df, rdf, ng, where + " df")
            if ng <= K.HEAD_MAX_N:  # and the one-launch head on the global batch
                l1, dr1, df1 = K.loss_head(kind, side, r, f)
                _loss_close("dist-vs-head", kind, regime, losses[0], l1.double(), where)
                if need_r:
                    _grad_close("dist-vs-head", kind, regime, dr, dr1.double().cpu(), ng, where + " dr")
                if need_f:
                    _grad_close("dist-vs-head", kind, regime, df, df1.double().cpu(), ng, where + " df")


# ---------------------------------------------------------------- hinge kinks, exactly
def _exact(got, want, what):
    assert torch.equal(got.detach().double().cpu().reshape(-1), want.reshape(-1)), what


@pytest.mark.parametrize("kind", H.HINGE)
def test_hinge_kinks_exact(K, kind):
    n = H.KINK_N
    r, f = _inputs("kink", kind, n)
    for side in [s for k, s in H.CASES if k == kind]:
        need_r, need_f = H.needs(kind, side)
        ref, rdr, rdf = _ref("kink", kind, n, side)
        rr, ff = (r if need_r else None), (f if need_f else None)
        halves = [(a.clone() if a is not None else None, b.clone() if b is not None else None)
                  for a, b in zip(_split(rr, (n // 2, n // 2)), _split(ff, (n // 2, n // 2)))]
        losses, ddr, ddf = _dist(K, kind, side, halves, n)
        for form, (loss, dr, df) in (("head", K.loss_head(kind, side, rr, ff)), ("dist", (losses[0], ddr, ddf))):
            what = f"{form} head {kind} side {side}"
            assert loss.double().item() == ref.item(), what
            if need_r:
                _exact(dr, rdr, what + " dr")
            if need_f:
                _exact(df, rdf, what + " df")
        assert torch.equal(losses[0], losses[1])
    if kind == 4:
        real, rdr, _ = _ref("kink", kind, n, 0)
        fake, _, rdf = _ref("kink", kind, n, 1)
        loss3, dr, df = K.loss_head_pair(kind, r, f)
        assert loss3.double().tolist() == [real.item(), fake.item(), (real + fake).item()]
        _exact(dr, rdr, "pair dr")
        _exact(df, rdf, "pair df")
    else:
        ref, _, rdf = _ref("kink", kind, n, 2)
        dy = torch.full((2 * n,), float("nan"), device=DEV)
        loss, _ = K.loss_head_joint(kind, torch.cat([f, r]), out=dy)
        assert loss.double().item() == ref.item()
        _exact(dy[:n], rdf, "joint dy")
        assert not dy[n:].any()


# ---------------------------------------------------------------- losses.py autograd functions
def _leaf(t):
    return t.reshape(-1, 1, 1, 1).clone().requires_grad_(True)


def _backward_forms(make, unit_seed):
    """make() -> (loss, leaves).  Runs backward(), backward(unit seed) and (2.5 * loss).backward()
    on fresh graphs: [(loss, [grad per leaf])] in that order."""
    out = []
    for form in ("plain", "unit", "scaled"):
        loss, leaves = make()
        if form == "plain":
            loss.backward()
        elif form == "unit":
            loss.backward(unit_seed(DEV))
        else:
            (2.5 * loss).backward()
        out.append((loss.detach(), [x.grad for x in leaves]))
    return out


def _check_forms(form, kind, forms, ref, ref_grads, n, where):
    """Each backward form against the reference; the unit seed bitwise equal to the plain one."""
    (l0, g0), (l1, g1), (l2, g2) = forms
    assert torch.equal(l0, l1) and torch.equal(l0, l2), where
    _loss_close(form, kind, "typical", l0, ref, where)
    for a, b, c, want in zip(g0, g1, g2, ref_grads):
        assert a.shape == (n, 1, 1, 1) and torch.equal(a, b), where + ": unit seed"
        _grad_close(form, kind, "typical", a, want, n, where)
        _grad_close(form, kind, "typical", c, want, n, where + " x2.5", gain=2.5)


@pytest.mark.parametrize("kind", range(1, 9))
def test_losses_autograd(K, kind):
    from relativisticgan_amd import dp, losses as LS
    assert not dp.active()
    for B in H.BATCHES:
        r, f = _inputs("typical", kind, B)
        where = f"B {B}"
        if kind <= 4:
            real, rdr, _ = _ref("typical", kind, B, 0)
            fake, _, rdf = _ref("typical", kind, B, 1)
            gl, _, gdf = _ref("typical", kind, B, 2)

            def one(fn, t):
                def make():
                    x = _leaf(t)
                    return fn(kind, x), [x]
                return _backward_forms(make, LS.unit_seed)

            _check_forms("loss_D_real", kind, one(LS.loss_D_real, r), real, [rdr], B, where)
            _check_forms("loss_D_fake", kind, one(LS.loss_D_fake, f), fake, [rdf], B, where)
            _check_forms("loss_G", kind, one(LS.loss_G, f), gl, [gdf], B, where)

            extras = []

            def make_pair():
                xr, xf = _leaf(r), _leaf(f)
                err, er, ef = LS.loss_D_pair(kind, xr, xf)
                extras.append((er, ef))
                return err, [xr, xf]

            pair = _backward_forms(make_pair, LS.unit_seed)
            _check_forms("loss_D_pair", kind, pair, real + fake, [rdr, rdf], B, where)
            for er, ef in extras:  # the real and the fake loss, detached from the graph
                assert not er.requires_grad and er.grad_fn is None and not ef.requires_grad and ef.grad_fn is None
                _loss_close("loss_D_pair", kind, "typical", er, real, where)
                _loss_close("loss_D_pair", kind, "typical", ef, fake, where)
            ref_D, ref_D_grads = real + fake, [rdr, rdf]
            halves = pair
        else:
            ref_D, rdr, rdf = _ref("typical", kind, B, 0)
            ref_D_grads = [rdr, rdf]
            gl, gdr, gdf = _ref("typical", kind, B, 2)

            def make_D():
                xr, xf = _leaf(r), _leaf(f)
                return LS.loss_D(kind, xr, xf), [xr, xf]

            def make_G():  # D(x) is a no-grad constant of the G step
                xf = _leaf(f)
                return LS.loss_G(kind, xf, r.reshape(-1, 1, 1, 1)), [xf]

            def make_G_both():
                xr, xf = _leaf(r), _leaf(f)
                return LS.loss_G(kind, xf, xr), [xr, xf]

            halves = _backward_forms(make_D, LS.unit_seed)
            _check_forms("loss_D", kind, halves, ref_D, ref_D_grads, B, where)
            g_forms = _backward_forms(make_G, LS.unit_seed)
            _check_forms("loss_G", kind, g_forms, gl, [gdf], B, where)
            _check_forms("loss_G", kind, _backward_forms(make_G_both, LS.unit_seed), gl, [gdr, gdf], B,
                         where + " with a real-side gradient")

            def make_G_cat():
                y = torch.cat([f, r]).reshape(-1, 1, 1, 1).clone().requires_grad_(True)
                return LS.loss_G_cat(kind, y), [y]

            for (lc, (gy,)), (lg, (gf,)), gain in zip(_backward_forms(make_G_cat, LS.unit_seed), g_forms,
                                                      (1.0, 1.0, 2.5)):
                assert gy.shape == (2 * B, 1, 1, 1)
                _loss_close("loss_G_cat", kind, "typical", lc, gl, where)
                _grad_close("loss_G_cat", kind, "typical", gy[:B], gdf, B, where, gain=gain)
                assert torch.equal(lc, lg) and torch.equal(gy[:B], gf), where + ": loss_G_cat vs loss_G"
                assert not gy[B:].any(), where + ": the real half of loss_G_cat's gradient is not zero"

        def make_cat():
            y = torch.cat([r, f]).reshape(-1, 1, 1, 1).clone().requires_grad_(True)
            return LS.loss_D_cat(kind, y), [y]

        for (lc, (gy,)), (lh, (gr, gf)), gain in zip(_backward_forms(make_cat, LS.unit_seed), halves, (1.0, 1.0, 2.5)):
            _loss_close("loss_D_cat", kind, "typical", lc, ref_D, where)
            _grad_close("loss_D_cat", kind, "typical", gy, torch.cat(ref_D_grads), B, where, gain=gain)
            assert torch.equal(lc, lh) and torch.equal(gy, torch.cat([gr, gf])), where + ": loss_D_cat vs the halves"


# ---------------------------------------------------------------- calls the library refuses
def test_library_rejects_without_launching(K):
    """RGAN_EINVAL from the host-side argument check (nothing is launched) surfaces as RganError."""
    from relativisticgan_amd import _lib as L
    r, f = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    g6 = torch.zeros(6, device=DEV)
    bad = {
        "heads 5-8 have no side 1": lambda: K.loss_head(5, 1, r, f),
        "the pair form serves heads 1-4": lambda: K.loss_head_pair(5, r, f),
        "the joint form serves heads 5-8": lambda: K.loss_head_joint(4, torch.cat([f, r])),
        "no phase 1 for head 5": lambda: K.loss_head_dist(5, 0, 1, r, f, 16, gsum=g6),
        "no phase 1 for head 2": lambda: K.loss_head_dist(2, 0, 1, r, None, 16, gsum=g6),
        "n_global < n": lambda: K.loss_head_dist(7, 0, 0, r, f, 7),
    }
    for what, call in bad.items():
        with pytest.raises(L.RganError, match="invalid arguments"):
            call()
            pytest.fail(what)
