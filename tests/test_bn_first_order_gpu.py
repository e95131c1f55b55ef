"""The first-order BatchNorm / activation kernels of csrc/bn_act.hip (and rgan_scale beside them),
entry point by entry point, against tests/bn_ref.py: the float64 formula evaluated on the same
fp32 inputs.  No case compares one kernel with another.

GPU-only (marked ``gpu``).  Activations are NHWC, so a case is its [P][C] matrix (a [P, C, 1, 1]
tensor on the device).  Where a launch rule picks the kernel, the kernels that ran are asserted by
name (torch.profiler; the names are those of bn_act.hip).  The geometry behind the shapes
(bn_geo): vector path (C % 4 == 0, 16-byte aligned) cq = C / 4, tpr = the largest power of two
<= 64 dividing cq, rp = 256 / tpr pixel rows in flight per block, cgroups = ceil(cq / tpr), rows
per chunk = max(ceil(P / (512 / cgroups)), 4 rp); scalar path tpr = min(64, pow2_floor(C)).
BN_UNR = 4, so the unrolled loop's edge BN_UNR * rp is the chunk minimum 4 * rp as well.

Bounds, per channel (the worst channel decides; a norm is over that channel's pixels):
  statistics, moments, running statistics   1e-6 of the reference value
  backward sums                             1e-6 of max(|sum|, ||terms||_2), terms = |da| sup|act'| (and
                                            times |y - mean|): the sums are double sums of fp32 terms
                                            (a few u each, u = 2^-24; absolute for a curved act', whose
                                            1 - t^2 cancels), and a sum that cancels below the L2 norm
                                            of its terms by chance has no relative accuracy to hold
  activations                               1e-5
  dy, dgamma, dbeta                         2e-5 (dgamma / dbeta with the floor of their sums; dy with
                                            4 u times the three terms it is the difference of, which
                                            is all a one-row segment's dy = 0 consists of)
A channel that lies more than bn_ref.COND_MAX standard deviations from 0 (regimes b1, c, d1, and
any channel of a one-row segment) is held in the forward to 1e-5 + the a-priori error of the
kernels' fused y * al + be (bn_ref.affine_error_bound) times the activation's Lipschitz constant:
there y * al and mean * al cancel in fp32; every element of such a channel is held to 1e-5 |ref| +
that figure as well.  In the backward that error cannot reach the act' of a piecewise-linear
activation (bn_ref.bwd_inputs asserts min_margin > 0 for every input; test_bn_ref_cpu.py restates
it), which stays at the plain bounds; a curved act' moves by sup|act''| times it, and the sums, dy
and the affine gradients of such a channel get the slack that follows (ref_backward).  The
statistics meet 1e-6 in every regime.

The issue's plain relative bounds for the backward (1e-6 of |sum|, 2e-5 of ||dy||, |dgamma|,
|dbeta|) were tried first and are not attainable as stated: a one-row segment's dy is exactly 0 and
the kernels return the roundings of its terms (2e-7 absolute); relu dy at P = 4, C = 1008 sat at
2.7e-5 of a channel whose two remaining degrees of freedom nearly cancel; sum_gx reached 1.3e-6
(two shards) and 2.4e-6 - 2.9e-6 (tanh, P = 4 and 147) of sums that cancel among their terms, and
the recorded profile shows cancelling channels at 1e-3 of |sum| inside the floor.  Hence the floors
above: they bite only where the result is small against its own terms.

Set RGAN_BN_RECORD to a file name to have the largest error and its ratio to the bound written
there per entry point, path and regime (profiles/bn_first_order_mi355x.txt).
"""
import math
import os

import pytest
import torch

from tests import bn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORD = {}


@pytest.fixture(scope="module")
def K():
    from relativisticgan_amd import kernels
    yield kernels
    path = os.environ.get("RGAN_BN_RECORD")
    if path:
        write_record(path)


REGIMES = ("a", "b0", "b1", "c", "d0", "d1", "e", "f", "-", "far")


def write_record(path):
    """The table of profiles/bn_first_order_mi355x.txt (below that file's notes): one line per entry
    point, activation class (the six folded into piecewise-linear / curved) and kernel path -- the
    largest per-channel error relative to the channel's reference with its regime, then the ratio
    to the bound per regime (``-``: no channel structure; ``far``: the elementwise bound on channels
    far from 0; ``.``: regime not in that case)."""
    rows = {}
    for (entry, route, kind), (e, r) in RECORD.items():
        parts = entry.split(".")
        cls = ["curved" if a in ("tanh", "sigmoid", "selu") else "piecewise" for a in parts if a in R.ACTS]
        key = (".".join(a for a in parts if a not in R.ACTS), cls[0] if cls else "-", route)
        e0, r0 = rows.setdefault(key, {}).get(kind, (0.0, 0.0))
        rows[key][kind] = (max(e0, e), max(r0, r))
    with open(path, "w") as f:
        f.write(f"{'entry point':36s} {'act':10s} {'path':44s} {'largest error':>16s}   "
                + " ".join(f"{k:>5s}" for k in REGIMES) + "\n")
        for (entry, cls, route), d in sorted(rows.items()):
            wk = max(d, key=lambda k: d[k][0])
            cells = " ".join((f"{d[k][1]:5.2f}" if k in d else "    .") for k in REGIMES)
            f.write(f"{entry:36s} {cls:10s} {route:44s} {d[wk][0]:10.2e} ({wk:>3s})   {cells}\n")


@pytest.fixture(scope="module")
def Lb():
    from relativisticgan_amd import _lib
    return _lib


# ------------------------------------------------------------------ helpers
def dev(m, misaligned=False):
    """[P][C] fp32 on the host -> a dense NHWC [P, C, 1, 1] device tensor; ``misaligned``: its
    data pointer 4 bytes past a 16-byte boundary."""
    P, C = m.shape
    buf = torch.empty(P * C + 4, device=DEV)
    o = 1 if misaligned else 0
    flat = buf[o:o + P * C]
    flat.copy_(m.reshape(-1).float())
    t = flat.as_strided((P, C, 1, 1), (C, 1, C, C))
    assert t.data_ptr() % 16 == (4 if misaligned else 0)
    return t


def empty(P, C, misaligned=False, fill=float("nan")):
    return dev(torch.full((P, C), fill), misaligned)


def vec(v):
    return None if v is None else v.to(DEV)


def host(t):
    return t.detach().double().cpu().reshape(-1, t.shape[1]) if t.dim() == 4 else t.detach().double().cpu()


def ran(fn):
    """(fn(), the rgan kernels it launched, by name without spaces)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in p.events() if "rgan::" in e.name]
    return out, sorted(n.split("rgan::")[1].split("(")[0].replace(" ", "") for n in names)


def check(entry, route, kinds, got, ref, rel, floor=None, slack=None, elementwise=False):
    """Per channel: ||got_c - ref_c|| <= max(rel ||ref_c||, floor_c) + ||slack_c||; prints, records
    and asserts the worst ratio.  A channel whose bound is 0 must be exact.  Where an a-priori
    ``slack`` applies (a channel with any), ``elementwise`` holds every ELEMENT to rel |ref| + slack
    as well (the forward)."""
    got, ref = host(got) if torch.is_tensor(got) else got, ref.detach().double().cpu()
    C = ref.shape[-1]
    got, ref = got.reshape(-1, C), ref.reshape(-1, C)
    err, nrm = (got - ref).norm(dim=0), ref.norm(dim=0)
    bound = rel * nrm
    if floor is not None:
        bound = torch.maximum(bound, floor.double().reshape(-1, C).norm(dim=0))
    if slack is not None:
        bound = bound + slack.double().reshape(-1, C).norm(dim=0)
    exact = torch.where(err > 0, math.inf, 0.0).double()   # a bound of 0: exact or nothing
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), exact)
    relerr = torch.where(nrm > 0, err / nrm.clamp_min(1e-300), exact)
    for kind in set(kinds):
        sel = torch.tensor([k == kind for k in kinds])
        key = (entry, route, kind)
        e0, r0 = RECORD.get(key, (0.0, 0.0))
        RECORD[key] = (max(e0, relerr[sel].max().item()), max(r0, ratio[sel].max().item()))
    worst = int(ratio.argmax())
    print(f"[bn1] {entry} {route} worst channel {worst} ({kinds[worst]}): err {relerr[worst].item():.3e} "
          f"ratio {ratio[worst].item():.3f}")
    assert ratio.max().item() <= 1.0, (entry, route, worst, kinds[worst], relerr[worst].item(), ratio[worst].item())
    if elementwise and slack is not None:
        sl = slack.double().reshape(-1, C)
        far = sl.norm(dim=0) > 0
        if bool(far.any()):
            eb = (rel * ref.abs() + sl)[:, far]
            ee = (got - ref).abs()[:, far]
            el = torch.where(eb > 0, ee / eb.clamp_min(1e-300), torch.where(ee > 0, math.inf, 0.0).double()).max().item()
            key = (entry, route + " elementwise", "far")
            RECORD[key] = (0.0, max(RECORD.get(key, (0.0, 0.0))[1], el))
            print(f"[bn1] {entry} {route} far channels, worst element: ratio {el:.3f}")
            assert el <= 1.0, (entry, route, "elementwise", el)


def offset_slack(y, mean, inv, gamma, beta, name):
    """The a-priori error of the fused affine form, on the channels that lie far from 0 only."""
    far = R.conditioning(mean, inv) > R.COND_MAX
    return R.act_lipschitz(name) * R.affine_error_bound(y, mean, inv, gamma, beta) * far.double()


def running_inputs(mean, C, seed):
    """Running buffers to update: running_mean shares the batch mean's sign (the update then adds
    two terms of one sign, and a relative bound on its result means something), running_var > 0."""
    g = torch.Generator().manual_seed(seed)
    rm = (mean * (0.5 + torch.rand(C, generator=g).double())).float()
    rv = torch.rand(C, generator=g) + 0.5
    return rm, rv


def check_stats(entry, route, kinds, stats, y64, n_mean_M2, momentum=None, rm0=None, rv0=None, bufs=None):
    """Device (mean, invstd) [2C] (+ updated running buffers) against the float64 moments."""
    n, mean, M2 = n_mean_M2
    C = mean.shape[0]
    s = host(stats).view(2, C)
    m_ref, i_ref = R.stats_of(n, mean, M2)
    check(entry + ".mean", route, kinds, s[0], m_ref, 1e-6)
    check(entry + ".invstd", route, kinds, s[1], i_ref, 1e-6)
    if bufs is not None:
        rm_ref, rv_ref, _ = R.running_update(rm0, rv0, None, n, mean, M2, momentum)
        check(entry + ".running_mean", route, kinds, bufs[0], rm_ref, 1e-6)
        check(entry + ".running_var", route, kinds, bufs[1], rv_ref, 1e-6)


# ------------------------------------------------------------------ forward moments and statistics
# (P, C, misaligned) -- vector path: C = 4 tpr 1 rp 256 (4 rp = 1024; 66563 rows = 66 chunks of 1024:
# bn_merge's 64 lanes loop), C = 8 tpr 2 rp 128 (512), C = 256 tpr 64 rp 4 (16; 1001 rows = 63 chunks
# of 16, the last of 9), C = 512 two channel groups, C = 20 tpr 1 and bn_merge's second 16-channel
# block part-filled; scalar path: C = 3 tpr 2 rp 128 (512), C = 6 tpr 4, C = 70 tpr 64 with a
# ragged second group of 6; a vector-eligible tensor 4 bytes off
STATS_CASES = [(1, 4, False), (2, 4, False), (3, 8, False), (1023, 4, False), (1024, 4, False), (1025, 4, False),
               (66563, 4, False), (511, 8, False), (512, 8, False), (513, 8, False), (15, 256, False),
               (16, 256, False), (17, 256, False), (1001, 256, False), (300, 512, False), (37, 20, False),
               (1, 3, False), (511, 3, False), (512, 3, False), (513, 3, False), (200, 6, False), (129, 70, False),
               (100, 8, True), (300, 256, True)]


@pytest.mark.parametrize("P,C,misaligned", STATS_CASES)
def test_stats_and_moments(K, P, C, misaligned):
    q = 4 if C % 4 == 0 and not misaligned else 1
    route = f"moments_partial<{q}>"
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=1000 + i)
        y = dev(d["y"], misaligned)
        mom_ref = R.moments(d["y"])
        for momentum in ((0.1, 1.0, 0.0) if i == 0 else (0.1,)):
            rm0, rv0 = running_inputs(mom_ref[1], C, 7 + i)
            rm, rv, nbt = vec(rm0), vec(rv0), torch.full((), 41, dtype=torch.long, device=DEV)
            stats, names = ran(lambda: K.bn_stats(y, R.EPS, momentum, rm, rv, nbt))
            assert names == sorted([f"bn_moments_partial<{q}>", "bn_merge<2>"]), names
            check_stats("bn_stats", route, kinds, stats, d["y"], mom_ref, momentum, rm0, rv0, (rm, rv))
            assert int(nbt.item()) == 42
        # no buffers: the same statistics, nothing else written
        out = torch.full((2 * C + 2,), float("nan"), device=DEV)
        stats2 = K.bn_stats(y, R.EPS, 0.1, out=out[:2 * C])
        assert torch.equal(stats2, stats) and bool(out[2 * C:].isnan().all())
        mom, names = ran(lambda: K.bn_moments(y))
        assert names == sorted([f"bn_moments_partial<{q}>", "bn_merge<1>"]), names
        mom = host(mom).view(3, C)
        assert torch.equal(mom[0], torch.full((C,), float(P), dtype=torch.float64))
        check("bn_moments.mean", route, kinds, mom[1], mom_ref[1], 1e-6)
        check("bn_moments.M2", route, kinds, mom[2], mom_ref[2], 1e-6)


# ------------------------------------------------------------------ rank merge
# shard sizes: unequal, one of count 0 and one of count 1 from four ranks up
SHARDS = {1: (200,), 2: (1, 199), 4: (0, 1, 71, 128), 8: (5, 0, 1, 64, 33, 128, 7, 2)}


@pytest.mark.parametrize("C", [5, 300])      # 300: two blocks of 256 threads
@pytest.mark.parametrize("nranks", [1, 2, 4, 8])
def test_finalize_rank_merge(K, nranks, C):
    """rgan_bn_finalize over the moments of real shards -- rgan_bn_moments, or, where a shard is a
    whole number of 64-row segments, rgan_bn_segment_moments of its synthesised segment sums; the
    empty shard's block is (0, junk, junk) -- is the float64 statistics of the whole batch."""
    sizes = SHARDS[nranks]
    P = sum(sizes)
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=2000 + i)
        blocks, p = [], 0
        for s in sizes:
            if s == 0:
                blk = torch.tensor([0.0, 1e30, -1e30], dtype=torch.float64, device=DEV).repeat_interleave(C)
            elif s % 64 == 0:
                part = R.segment_sums(d["y"][p:p + s]).to(DEV)
                blk = K.bn_segment_moments(part, 0, s // 64, C)
            else:
                blk = K.bn_moments(dev(d["y"][p:p + s]))
            blocks.append(blk)
            p += s
        mom = torch.cat(blocks)
        whole = R.moments(d["y"])
        for momentum in ((0.1, 1.0, 0.0) if i == 0 else (0.1,)):
            rm0, rv0 = running_inputs(whole[1], C, 9 + i)
            rm, rv, nbt = vec(rm0), vec(rv0), torch.full((), 5, dtype=torch.long, device=DEV)
            stats = K.bn_finalize(mom, nranks, C, R.EPS, momentum, rm, rv, nbt)
            check_stats("bn_finalize", f"nranks{nranks}", kinds, stats, d["y"], whole, momentum, rm0, rv0, (rm, rv))
            assert int(nbt.item()) == 6
        assert torch.equal(K.bn_finalize(mom, nranks, C, R.EPS, 0.1), stats)


# ------------------------------------------------------------------ apply
APPLY_CASES = [(100, 4, False), (33, 8, False), (40, 256, False), (10, 512, False), (50, 3, False), (50, 6, False),
               (20, 70, False), (64, 8, True)]


@pytest.mark.parametrize("P,C,misaligned", APPLY_CASES)
def test_apply(K, P, C, misaligned):
    """rgan_bn_apply with the device's own statistics: every activation, gamma / beta absent,
    out= given (a misaligned y takes the scalar kernel)."""
    q = 4 if C % 4 == 0 and not misaligned else 1
    for i, (label, kinds) in enumerate(R.mixes(C)):
        for affine_on in ((True, False) if i == 0 else (True,)):
            d = R.inputs(P, C, kinds, seed=3000 + i, affine_on=affine_on)
            y = dev(d["y"], misaligned)
            stats = K.bn_stats(y, R.EPS, 0.1)
            mean, inv = host(stats).view(2, C)
            for name in R.ACTS:
                out = empty(P, C)
                got, names = ran(lambda: K.bn_apply(y, stats, vec(d["gamma"]), vec(d["beta"]), name, R.ALPHA, out=out))
                assert got is out and names == [f"bn_apply_kernel<{q},1>"], names
                ref = R.forward(d["y"], mean, inv, d["gamma"], d["beta"], name)
                check("bn_apply." + name, f"apply<{q}>", kinds, got, ref, 1e-5,
                      slack=offset_slack(d["y"], mean, inv, d["gamma"], d["beta"], name), elementwise=True)


# two segments: P = 2 (seg_rows = 1); (40, 256): rp 4, 3 row blocks, step 12 -- a thread's four
# unrolled rows p, p + 12, p + 24, p + 36 straddle seg_rows = 20; (3200, 20): rp 256, 4 row blocks,
# step 1024, rows p .. p + 3072 straddle 1600
@pytest.mark.parametrize("P,C", [(2, 4), (40, 256), (3200, 20), (130, 8)])
def test_apply_segments(K, P, C):
    Ps = P // 2
    for i, (label, kinds) in enumerate(R.mixes(C, R.TINY) if Ps == 1 else R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=3500 + i, nseg=2)
        y = dev(d["y"])
        stats = torch.stack([K.bn_stats(y[:Ps], R.EPS, 0.1), K.bn_stats(y[Ps:], R.EPS, 0.1)])
        st = host(stats).view(2, 2, C)
        for name in R.ACTS:
            got, names = ran(lambda: K.bn_apply_segments(y, stats, vec(d["gamma"]), vec(d["beta"]), name, R.ALPHA,
                                                         empty(P, C)))
            assert names == ["bn_apply_kernel<4,2>"], names
            ref = torch.cat([R.forward(d["y"][k * Ps:(k + 1) * Ps], st[k, 0], st[k, 1], d["gamma"], d["beta"], name)
                             for k in range(2)])
            slack = torch.cat([offset_slack(d["y"][k * Ps:(k + 1) * Ps], st[k, 0], st[k, 1], d["gamma"], d["beta"],
                                            name) for k in range(2)])
            check("bn_apply_segments." + name, "apply<4,2>", kinds, got, ref, 1e-5, slack=slack, elementwise=True)
        one, names = ran(lambda: K.bn_apply_segments(y[:Ps], stats[:1], vec(d["gamma"]), vec(d["beta"]), "lrelu",
                                                     R.ALPHA, empty(Ps, C)))
        assert names == ["bn_apply_kernel<4,1>"], names
        check("bn_apply_segments.lrelu", "apply<4,1>", kinds, one,
              R.forward(d["y"][:Ps], st[0, 0], st[0, 1], d["gamma"], d["beta"], "lrelu"), 1e-5,
              slack=offset_slack(d["y"][:Ps], st[0, 0], st[0, 1], d["gamma"], d["beta"], "lrelu"), elementwise=True)


# ------------------------------------------------------------------ segment sums -> statistics
def seg_stats(K, Lb, part, s0, s1, C, sr, momentum, rm, rv, nbt, moments=False):
    """rgan_bn_segment_stats with any seg_rows (the Python wrappers fix 64)."""
    if sr == 64 and not moments:
        return K.bn_segment_stats(part, s0, s1, C, R.EPS, momentum, rm, rv, nbt)
    if sr == 64:
        return K.bn_segment_moments(part, s0, s1, C)
    out = torch.empty(3 * C, dtype=torch.float64, device=DEV) if moments else torch.empty(2 * C, device=DEV)
    Lb.check(Lb.lib().rgan_bn_segment_stats(Lb.ptr(part), s0, s1, C, sr, R.EPS, float(momentum), Lb.ptr(rm),
                                            Lb.ptr(rv), Lb.ptr(nbt), None if moments else Lb.ptr(out),
                                            Lb.ptr(out) if moments else None, Lb.stream()), "rgan_bn_segment_stats")
    return out


def seg_stats_n(Lb, part, S, nseg, C, sr, momentum, rm, rv, nbt):
    out = torch.empty(nseg, 2 * C, device=DEV)
    Lb.check(Lb.lib().rgan_bn_segment_stats_n(Lb.ptr(part), 0, S, nseg, C, sr, R.EPS, float(momentum), Lb.ptr(rm),
                                              Lb.ptr(rv), Lb.ptr(nbt), Lb.ptr(out), Lb.stream()),
             "rgan_bn_segment_stats_n")
    return out


# S segments of the synthesised [S][2][C] sums: bn_seg_merge's 256 lanes take one segment each up
# to S = 256, loop from 257 and run the unroll-by-4 from 1025 (k + 768 < s1).  Segments of 64 rows
# up to S = 3, of 2 rows above (the kernels take seg_rows as a count only), so y stays small.
@pytest.mark.parametrize("C", [4, 20, 64, 132])
@pytest.mark.parametrize("S", [1, 3, 255, 256, 257, 1025])
def test_segment_stats(K, Lb, S, C):
    sr = 64 if S <= 3 else 2
    P = S * sr
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=4000 + i)
        part = R.segment_sums(d["y"], sr).to(DEV)
        whole = R.moments(d["y"])
        rm0, rv0 = running_inputs(whole[1], C, 11 + i)
        rm, rv, nbt = vec(rm0), vec(rv0), torch.zeros((), dtype=torch.long, device=DEV)
        stats, names = ran(lambda: seg_stats(K, Lb, part, 0, S, C, sr, 0.1, rm, rv, nbt))
        assert names == ["bn_seg_merge<2,1>"], names
        check_stats("bn_segment_stats", "seg_merge<2,1>", kinds, stats, d["y"], whole, 0.1, rm0, rv0, (rm, rv))
        assert int(nbt.item()) == 1
        mom, names = ran(lambda: seg_stats(K, Lb, part, 0, S, C, sr, 0.0, None, None, None, moments=True))
        assert names == ["bn_seg_merge<1,1>"], names
        mom = host(mom).view(3, C)
        assert torch.equal(mom[0], torch.full((C,), float(P), dtype=torch.float64))
        check("bn_segment_moments.mean", "seg_merge<1,1>", kinds, mom[1], whole[1], 1e-6)
        check("bn_segment_moments.M2", "seg_merge<1,1>", kinds, mom[2], whole[2], 1e-6)
        if S >= 3:   # a sub-range [s0, s1) of the segments
            s0, s1 = 1, S - 1 if S > 3 else S
            sub = R.moments(d["y"][s0 * sr:s1 * sr])
            check_stats("bn_segment_stats", "seg_merge<2,1>", kinds,
                        seg_stats(K, Lb, part, s0, s1, C, sr, 0.1, None, None, None), None, sub)


# two batch segments in one launch: statistics per half, running statistics in segment order
@pytest.mark.parametrize("S,C", [(2, 4), (6, 20), (512, 64), (514, 132), (2050, 20)])
def test_segment_stats_two_segments(K, Lb, S, C):
    sr = 64 if S <= 6 else 2
    P, Ps = S * sr, S * sr // 2
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=4500 + i, nseg=2)
        part = R.segment_sums(d["y"], sr).to(DEV)
        halves = [R.moments(d["y"][:Ps]), R.moments(d["y"][Ps:])]
        rm0, rv0 = running_inputs(halves[0][1], C, 13 + i)
        rm, rv, nbt = vec(rm0), vec(rv0), torch.zeros((), dtype=torch.long, device=DEV)
        stats, names = ran(lambda: seg_stats_n(Lb, part, S, 2, C, sr, 0.1, rm, rv, nbt))
        assert names == ["bn_seg_merge<2,2>"], names
        r1 = R.running_update(rm0, rv0, None, *halves[0], 0.1)
        r2 = R.running_update(r1[0], r1[1], None, *halves[1], 0.1)
        for k in range(2):
            check_stats("bn_segment_stats_n", "seg_merge<2,2>", kinds, stats[k], None, halves[k])
        check("bn_segment_stats_n.running_mean", "seg_merge<2,2>", kinds, rm, r2[0], 1e-6,
              floor=1e-6 * r1[0].abs().double())   # the second update may cancel against the first
        check("bn_segment_stats_n.running_var", "seg_merge<2,2>", kinds, rv, r2[1], 1e-6)
        assert int(nbt.item()) == 2
        one = seg_stats_n(Lb, part, S, 1, C, sr, 0.1, None, None, None)
        check_stats("bn_segment_stats_n", "seg_merge<2,1>", kinds, one[0], None, R.moments(d["y"]))


# rgan_bn_segment_apply runs ONE launch iff S / nseg <= 64, nseg == 1 and P * C <= 2^18 (64-row
# segments): each condition from both sides -- S = 64 | 65 at C = 64 (P * C = 2^18 | above) and at
# C = 4 (P * C far below: S alone decides); C = 128 with S = 32 | 33 (P * C = 2^18 | 2^18 + 64 C,
# S far below); nseg = 2 at the one-launch shape
@pytest.mark.parametrize("S,C,nseg,one_launch", [(64, 64, 1, True), (65, 64, 1, False), (64, 4, 1, True),
                                                 (65, 4, 1, False), (32, 128, 1, True), (33, 128, 1, False),
                                                 (64, 64, 2, False), (2, 8, 2, False), (1, 20, 1, True)])
def test_segment_apply(K, S, C, nseg, one_launch):
    P = S * 64
    Ps = P // nseg
    assert one_launch == (S // nseg <= 64 and nseg == 1 and P * C <= 1 << 18)
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=5000 + i, nseg=nseg)
        y, part = dev(d["y"]), R.segment_sums(d["y"]).to(DEV)
        segs = [R.moments(d["y"][k * Ps:(k + 1) * Ps]) for k in range(nseg)]
        rm0, rv0 = running_inputs(segs[0][1], C, 17 + i)
        for name in (R.ACTS if i == 0 else ("lrelu",)):
            rm, rv, nbt = vec(rm0), vec(rv0), torch.zeros((), dtype=torch.long, device=DEV)
            stats = torch.full((nseg, 2 * C), float("nan"), device=DEV)
            got, names = ran(lambda: K.bn_segment_apply(part, S, y, R.EPS, 0.1, rm, rv, nbt, vec(d["gamma"]),
                                                        vec(d["beta"]), name, R.ALPHA, stats, empty(P, C)))
            want = [f"bn_seg_apply_kernel<{nseg}>"] if one_launch else \
                sorted([f"bn_seg_merge<2,{nseg}>", f"bn_apply_kernel<4,{nseg}>"])
            assert names == want, names
            route = "seg_apply(one launch)" if one_launch else f"seg_merge+apply<4,{nseg}>"
            st = host(stats).view(nseg, 2, C)
            run = (rm0, rv0)
            for k in range(nseg):
                check_stats("bn_segment_apply", route, kinds, stats[k], None, segs[k])
                prev = run
                run = R.running_update(run[0], run[1], None, *segs[k], 0.1)[:2]
            check("bn_segment_apply.running_mean", route, kinds, rm, run[0], 1e-6, floor=1e-6 * prev[0].abs().double())
            check("bn_segment_apply.running_var", route, kinds, rv, run[1], 1e-6)
            assert int(nbt.item()) == nseg     # once per batch segment, not once per block
            ref = torch.cat([R.forward(d["y"][k * Ps:(k + 1) * Ps], st[k, 0], st[k, 1], d["gamma"], d["beta"], name)
                             for k in range(nseg)])
            slack = torch.cat([offset_slack(d["y"][k * Ps:(k + 1) * Ps], st[k, 0], st[k, 1], d["gamma"], d["beta"],
                                            name) for k in range(nseg)])
            check("bn_segment_apply." + name, route, kinds, got, ref, 1e-5, slack=slack, elementwise=True)


# ------------------------------------------------------------------ backward
def sums_floor(b, rel):
    """rel * ||terms||_2 of the two backward sums [2][C] (see the module docstring)."""
    return rel * torch.stack([b["gmax"].norm(dim=0), (b["gmax"] * b["ymean"]).norm(dim=0)])


def ref_backward(d, mean, inv, name, sl=slice(None), **kw):
    """bn_ref.backward of rows ``sl`` plus what the a-priori floors need: gmax = |da| sup|act'| (the
    scale of a term da * act'(z) whose act' carries an ABSOLUTE fp32 error of a few u: tanh' = 1 -
    t^2 and its like cancel), ymean = y - mean, and dy_floor = 4 u |al| (gmax + |sum_g / Pg| + |(y -
    mean) invstd^2 sum_gx / Pg|), the rounding of the three terms dy is the difference of."""
    da, y = d["da"][sl].double(), d["y"][sl].double()
    b = R.backward(da, y, mean, inv, d["gamma"], d["beta"], name, **kw)
    mean, inv = mean.double(), inv.double()
    b["ymean"], b["inv"], b["gmax"] = y - mean, inv, da.abs() * R.act_lipschitz(name)
    s = b["sums"] if kw.get("sums") is None else kw["sums"].double().view(2, -1)
    Pg = kw.get("P_global") or y.shape[0]
    al = inv if d["gamma"] is None else d["gamma"].double() * inv
    b["dy_floor"] = 4 * R.U * al.abs() * (b["gmax"] + (s[0] / Pg).abs() + (b["ymean"] * inv ** 2 * s[1] / Pg).abs())
    # a curved activation on a channel far from 0: act'(z) moves by sup|act''| times z's a-priori error, so
    # g by e = |da| sup|act''| affine_error_bound, the sums by sum e and sum e |y - mean|, and dy by
    # |al| (e + sum e / Pg + |y - mean| invstd^2 sum(e |y - mean|) / Pg)   (0 for the piecewise-linear ones)
    far = (R.conditioning(mean, inv) > R.COND_MAX).double()
    e = far * da.abs() * R.act_curvature(name) * R.affine_error_bound(y, mean, inv, d["gamma"], d["beta"])
    b["sums_slack"] = torch.stack([e.sum(0), (e * b["ymean"].abs()).sum(0)])
    n_loc = y.shape[0]
    b["dy_slack"] = al.abs() * (e + b["sums_slack"][0] / n_loc
                                + b["ymean"].abs() * inv ** 2 * b["sums_slack"][1] / n_loc)
    return b


def check_backward(entry, route, kinds, b, dy=None, dgamma=None, dbeta=None, sums=None, dg0=None, db0=None):
    """Device results against one reference dict of bn_ref.backward (dg0 / db0: what the affine
    gradients were accumulated onto)."""
    fl = sums_floor(b, 1.0)
    if sums is not None:
        s = host(sums).view(2, -1)
        check(entry + ".sum_g", route, kinds, s[0], b["sums"][0], 1e-6, floor=1e-6 * fl[0], slack=b["sums_slack"][0])
        check(entry + ".sum_gx", route, kinds, s[1], b["sums"][1], 1e-6, floor=1e-6 * fl[1], slack=b["sums_slack"][1])
    if dy is not None:
        check(entry + ".dy", route, kinds, dy, b["dy"], 2e-5, floor=b["dy_floor"], slack=b["dy_slack"])
    if dgamma is not None:
        base = 0 if dg0 is None else dg0.double()
        check(entry + ".dgamma", route, kinds, host(dgamma) - base, b["dgamma"], 2e-5,
              floor=2e-5 * b["inv"] * fl[1] + (0 if dg0 is None else 4 * R.U * dg0.double().abs()),
              slack=b["inv"] * b["sums_slack"][1])
    if dbeta is not None:
        base = 0 if db0 is None else db0.double()
        check(entry + ".dbeta", route, kinds, host(dbeta) - base, b["dbeta"], 2e-5,
              floor=2e-5 * fl[0] + (0 if db0 is None else 4 * R.U * db0.double().abs()), slack=b["sums_slack"][0])


def bwd_names(P, C, small, q, nseg=1):
    if small:
        return [f"bn_bwd_small<{nseg}>"]
    return sorted([f"bn_bwd_partial<{q},{nseg}>", "bn_merge<0>", f"bn_bwd_apply<{q},{nseg}>"])


# One segment.  bn_bwd_small (one launch) iff P <= 2048 and C % 16 == 0: (2048 | 2049, 16); C = 20
# leaves it at small P; C = 128 is 8 blocks -- the XCD-aware group permutation is on (gridDim % 8
# == 0) -- C = 48 and 144 are 3 and 9 blocks, where it is off; C = 6 and 70 take the scalar kernels
@pytest.mark.parametrize("P,C,nseg", [c for c in R.BWD_CASES if c[2] == 1])
def test_backward(K, P, C, nseg):
    small, q = P <= 2048 and C % 16 == 0, 4 if C % 4 == 0 else 1
    route = "bwd_small<1>" if small else f"partial+merge+apply<{q}>"
    for i in range(len(R.bwd_mixes(P, C, 1))):
        label, kinds, d = R.bwd_inputs(P, C, 1, i)
        y, da, gamma, beta = dev(d["y"]), dev(d["da"]), vec(d["gamma"]), vec(d["beta"])
        stats = K.bn_stats(y, R.EPS, 0.1)       # the true batch statistics, from the device forward
        mean, inv = host(stats).view(2, C)
        for name in R.ACTS:
            b = ref_backward(d, mean, inv, name)
            (dy, dg, db), names = ran(lambda: K.bn_backward(da, y, stats, gamma, beta, name, R.ALPHA, out=empty(P, C)))
            assert names == bwd_names(P, C, small, q), names
            check_backward("bn_backward." + name, route, kinds, b, dy, dg, db)
        if i > 0:
            continue
        # the pieces, LeakyReLU: sums, apply, apply_ex (add separate / aliased, accumulated affine
        # gradients, one of them only, none), affine gradients from the sums, gamma / beta absent
        name = "lrelu"
        b = ref_backward(d, mean, inv, name)
        (sums, _), names = ran(lambda: K.bn_backward_sums(da, y, stats, gamma, beta, name, R.ALPHA))
        assert names == sorted([f"bn_bwd_partial<{q},1>", "bn_merge<0>"]), names
        check_backward("bn_backward_sums", f"partial<{q}>", kinds, b, sums=sums)
        (dy, dg, db), names = ran(lambda: K.bn_backward_apply(da, y, stats, gamma, beta, name, R.ALPHA, sums, P,
                                                              out=empty(P, C)))
        assert names == [f"bn_bwd_apply<{q},1>"], names
        check_backward("bn_backward_apply", f"apply<{q}>", kinds, b, dy, dg, db)
        dy, dg, db = K.bn_backward_apply(da, y, stats, gamma, beta, name, R.ALPHA, sums, P, need_affine=False,
                                         out=empty(P, C))
        assert dg is None and db is None
        check_backward("bn_backward_apply", f"apply<{q}>", kinds, b, dy)
        g = torch.Generator().manual_seed(P + C)
        dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
        b_add = ref_backward(d, mean, inv, name, add=d["add"])
        for aliased in (False, True):
            out = dev(d["add"]) if aliased else empty(P, C)
            dgb, dbb = vec(dg0), vec(db0)
            dy = K.bn_backward_apply_ex(da, y, stats, gamma, beta, name, R.ALPHA, sums, P,
                                        add=out if aliased else dev(d["add"]), out=out, dgamma=dgb, dbeta=dbb,
                                        accumulate_affine=True)
            check_backward("bn_backward_apply_ex", f"apply<{q}>+add", kinds, b_add, dy, dgb, dbb, dg0=dg0, db0=db0)
        only_g, only_b = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        K.bn_backward_apply_ex(da, y, stats, gamma, beta, name, R.ALPHA, sums, P, out=empty(P, C), dgamma=only_g)
        K.bn_backward_apply_ex(da, y, stats, gamma, beta, name, R.ALPHA, sums, P, out=empty(P, C), dbeta=only_b)
        check_backward("bn_backward_apply_ex", f"apply<{q}>", kinds, b, dgamma=only_g, dbeta=only_b)
        ag, ab = vec(dg0), vec(db0)
        K.bn_affine_grads(sums, stats, C, ag, ab, accumulate=True)
        check_backward("bn_affine_grads", "accumulate", kinds, b, dgamma=ag, dbeta=ab, dg0=dg0, db0=db0)
        ag2 = torch.full((C,), float("nan"), device=DEV)
        K.bn_affine_grads(sums, stats, C, dgamma=ag2)
        check_backward("bn_affine_grads", "write", kinds, b, dgamma=ag2)
        _, pk, plain = R.bwd_inputs(P, C, 1, 0, affine_on=False)   # z = xhat: no constant channel (its z is 0)
        yp, dap = dev(plain["y"]), dev(plain["da"])
        st_p = K.bn_stats(yp, R.EPS, 0.1)
        mp, ip = host(st_p).view(2, C)
        dy, dg, db = K.bn_backward(dap, yp, st_p, None, None, name, R.ALPHA, out=empty(P, C))
        assert dg is None and db is None
        check_backward("bn_backward.lrelu", route + " no affine", pk, ref_backward(plain, mp, ip, name), dy)


# P_global = 2 P: two shards, their sums added (the data-parallel all-reduce), applied per shard:
# the whole batch's float64 gradient; the shards' affine gradients add up to the whole batch's
@pytest.mark.parametrize("P,C,nseg", R.TWO_SHARD_CASES)
def test_backward_two_shards(K, P, C, nseg):
    for i in range(len(R.bwd_mixes(P, C, 1))):
        label, kinds, d = R.bwd_inputs(P, C, 1, i)
        y, da, gamma, beta = dev(d["y"]), dev(d["da"]), vec(d["gamma"]), vec(d["beta"])
        stats = K.bn_finalize(torch.cat([K.bn_moments(y[:P // 2]), K.bn_moments(y[P // 2:])]), 2, C, R.EPS, 0.1)
        mean, inv = host(stats).view(2, C)
        for name in R.ACTS:
            whole = ref_backward(d, mean, inv, name)
            loc = [K.bn_backward_sums(da[s], y[s], stats, gamma, beta, name, R.ALPHA)[0]
                   for s in (slice(0, P // 2), slice(P // 2, P))]
            tot = loc[0] + loc[1]
            check_backward("bn_backward_sums", "two shards", kinds, whole, sums=tot)
            dgs = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            for k, s in enumerate((slice(0, P // 2), slice(P // 2, P))):
                dy, dg, db = K.bn_backward_apply(da[s], y[s], stats, gamma, beta, name, R.ALPHA, tot, P,
                                                 need_affine=False, out=empty(P // 2, C))
                check("bn_backward_apply.dy", "P_global=2P", kinds, dy, whole["dy"][s], 2e-5, floor=whole["dy_floor"][s],
                      slack=whole["dy_slack"][s])
                K.bn_affine_grads(loc[k], stats, C, dgs[0], dgs[1], accumulate=True)
            check_backward("bn_affine_grads", "two shards", kinds, whole, dgamma=dgs[0], dbeta=dgs[1])


# Two segments, rows per segment 1 | 127 | 128 | 129 (bn_bwd_small's 128 row lanes) | 1024 | 1025 (the
# two-segment kernel keeps 8 x 128 rows per segment in registers and re-reads the rest) | 2048 | 2049
# (three launches); C = 128 with the group permutation on; C = 20 on the three-launch vector path
@pytest.mark.parametrize("P,C,nseg", [c for c in R.BWD_CASES if c[2] == 2])
def test_backward_segments(K, P, C, nseg):
    Ps = P // 2
    small = Ps <= 2048 and C % 16 == 0
    route = "bwd_small<2>" if small else "partial+merge+apply<4,2>"
    for i in range(len(R.bwd_mixes(P, C, 2))):
        label, kinds, d = R.bwd_inputs(P, C, 2, i)
        y, da, gamma, beta = dev(d["y"]), dev(d["da"]), vec(d["gamma"]), vec(d["beta"])
        stats = torch.stack([K.bn_stats(y[:Ps], R.EPS, 0.1), K.bn_stats(y[Ps:], R.EPS, 0.1)])
        st = host(stats).view(2, 2, C)
        for name in R.ACTS:   # (in a one-row segment every channel is its own mean and lies far from 0)
            bs = [ref_backward(d, st[k, 0], st[k, 1], name, slice(k * Ps, (k + 1) * Ps)) for k in range(2)]
            (dy, dg, db), names = ran(lambda: K.bn_backward_segments(da, y, stats, gamma, beta, name, R.ALPHA, True,
                                                                     True, empty(P, C)))
            assert names == bwd_names(Ps, C, small, 4, 2), names
            for k in range(2):
                check(f"bn_backward_segments.{name}.dy", route, kinds, dy[k * Ps:(k + 1) * Ps], bs[k]["dy"], 2e-5,
                      floor=bs[k]["dy_floor"], slack=bs[k]["dy_slack"])
            fl = [sums_floor(b, 1.0) for b in bs]
            check(f"bn_backward_segments.{name}.dgamma", route, kinds, dg, bs[0]["dgamma"] + bs[1]["dgamma"], 2e-5,
                  floor=2e-5 * torch.hypot(bs[0]["inv"] * fl[0][1], bs[1]["inv"] * fl[1][1]),
                  slack=sum(b["inv"] * b["sums_slack"][1] for b in bs))
            check(f"bn_backward_segments.{name}.dbeta", route, kinds, db, bs[0]["dbeta"] + bs[1]["dbeta"], 2e-5,
                  floor=2e-5 * torch.hypot(fl[0][0], fl[1][0]), slack=sum(b["sums_slack"][0] for b in bs))
        if i == 0:   # one of the affine gradients only
            _, dg, db = K.bn_backward_segments(da, y, stats, gamma, beta, "lrelu", R.ALPHA, True, False, empty(P, C))
            assert db is None and dg is not None


# rgan_bn_backward_sums_apply: ONE launch (bn_bwd_small) iff P <= 2048, C % 16 == 0 and C / 16 >= 64:
# C = 1024 is 64 groups, C = 1008 is 63 (three launches); P = 4 and 147 (ragged over 128 row lanes)
@pytest.mark.parametrize("P,C", R.SUMS_APPLY_CASES)
def test_backward_sums_apply(K, P, C):
    small = C // 16 >= 64
    route = "bwd_small<1>" if small else "partial+merge+apply<4>"
    for i in range(len(R.bwd_mixes(P, C, 1))):
        label, kinds, d = R.bwd_inputs(P, C, 1, i)
        y, da, gamma, beta = dev(d["y"]), dev(d["da"]), vec(d["gamma"]), vec(d["beta"])
        stats = K.bn_stats(y, R.EPS, 0.1)
        mean, inv = host(stats).view(2, C)
        g = torch.Generator().manual_seed(P + C + i)
        dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
        for name in R.ACTS:
            for mode in ("plain", "add", "aliased"):
                b = ref_backward(d, mean, inv, name, add=None if mode == "plain" else d["add"])
                out = dev(d["add"]) if mode == "aliased" else empty(P, C)
                add = None if mode == "plain" else (out if mode == "aliased" else dev(d["add"]))
                dgb, dbb = vec(dg0), vec(db0)
                (sums, dy), names = ran(lambda: K.bn_backward_sums_apply(da, y, stats, gamma, beta, name, R.ALPHA,
                                                                         add=add, out=out, dgamma=dgb, dbeta=dbb,
                                                                         accumulate_affine=mode != "plain"))
                assert names == bwd_names(P, C, small, 4), names
                acc = mode != "plain"
                check_backward("bn_backward_sums_apply." + name, f"{route} {mode}", kinds, b, dy, dgb, dbb, sums,
                               dg0=dg0 if acc else None, db0=db0 if acc else None)


# ------------------------------------------------------------------ sums from a GEMM's post-op
# (B, cin, cout, H, transposed) of test_kernels_gpu.POST_CASES: the smallest split-K shape (1024 rows:
# S / nseg <= 64, merge + apply in one launch) and the smallest unsplit one (65536 rows: bn_part_merge)
@pytest.mark.parametrize("case", [(4, 128, 256, 16, False), (64, 128, 64, 32, True)])
def test_backward_parts(K, case):
    """conv_dgrad(post=Post(2)) + rgan_bn_backward_parts with the true batch statistics of 1 and 2
    batch segments == bn_ref's backward of the float64 conv data gradient."""
    import torch.nn.functional as F
    from relativisticgan_amd.kernels import ConvGeom, Post
    B, cin, cout, H, tr = case
    torch.manual_seed(37)
    geo = ConvGeom(4, 2, 1, tr)
    Ho = H * 2 if tr else H // 2
    P = B * H * H
    kinds = [R.WELL[c % 2 * 3] for c in range(cin)]     # a, e
    d = R.inputs(P, cin, kinds, seed=7000)
    w = (torch.randn(cin, cout, 4, 4) if tr else torch.randn(cout, cin, 4, 4)) * 0.05
    dyo = torch.randn(B, cout, Ho, Ho)
    if tr:
        da64 = F.conv2d(dyo.double(), w.double(), stride=2, padding=1)
    else:
        da64 = F.conv_transpose2d(dyo.double(), w.double(), stride=2, padding=1)
    da64 = da64.permute(0, 2, 3, 1).reshape(P, cin)
    y = K.empty_nhwc(B, cin, H, H, DEV)
    gamma, beta = vec(d["gamma"]), vec(d["beta"])
    dyo_d = dyo.to(DEV).contiguous(memory_format=torch.channels_last)
    for nseg in (1, 2):
        Ps = P // nseg
        d2 = dict(d, y=R.off_kink(d["y"], d["gamma"], d["beta"], nseg=nseg), da=da64)
        R.assert_off_kink(d2["y"], d["gamma"], d["beta"], nseg=nseg)
        y.copy_(d2["y"].view(B, H, H, cin).permute(0, 3, 1, 2))
        stats = torch.stack([K.bn_stats(y[k * B // nseg:(k + 1) * B // nseg], R.EPS, 0.1) for k in range(nseg)])
        st = host(stats).view(nseg, 2, cin)
        post = Post(2, "lrelu", R.ALPHA, y, stats=stats, gamma=gamma, beta=beta, nseg=nseg)
        gz = K.conv_dgrad(dyo_d, w.to(DEV), geo, (B, cin, H, H), post=post)
        assert post.fused and (post.S // nseg <= 64) == (P == 1024)
        (dy, dg, db), names = ran(lambda: K.bn_backward_parts(gz, y, stats, gamma, beta, post, True, True))
        want = [f"bn_parts_apply_kernel<{nseg}>"] if post.S // nseg <= 64 else \
            sorted(["bn_part_merge", f"bn_bwd_apply<4,{nseg}>"])
        assert names == want, names
        route = "parts_apply(one launch)" if post.S // nseg <= 64 else "part_merge+apply"
        bs = [ref_backward(d2, st[k, 0], st[k, 1], "lrelu", slice(k * Ps, (k + 1) * Ps)) for k in range(nseg)]
        # the GEMM's fp32 data gradient (K = cout * 4 products per element) carries 2e-6 (test_kernels_gpu.py);
        # dy is linear in it
        dyh = dy.permute(0, 2, 3, 1).reshape(P, cin)
        for k in range(nseg):
            check("bn_backward_parts.dy", f"{route} nseg{nseg}", kinds, dyh[k * Ps:(k + 1) * Ps], bs[k]["dy"], 2e-5,
                  floor=bs[k]["dy_floor"])
        fl = [sums_floor(b, 1.0) for b in bs]
        check("bn_backward_parts.dgamma", f"{route} nseg{nseg}", kinds, dg, sum(b["dgamma"] for b in bs), 2e-5,
              floor=2e-5 * sum((b["inv"] * f[1]) ** 2 for b, f in zip(bs, fl)).sqrt())
        check("bn_backward_parts.dbeta", f"{route} nseg{nseg}", kinds, db, sum(b["dbeta"] for b in bs), 2e-5,
              floor=2e-5 * sum(f[0] ** 2 for f in fl).sqrt())


# ------------------------------------------------------------------ activation backward, scale, channel sum
def flat(v, misaligned=False):
    buf = torch.empty(v.numel() + 4, device=DEV)
    o = 1 if misaligned else 0
    t = buf[o:o + v.numel()]
    t.copy_(v)
    return t


def act_outputs(n, name, g):
    """An activation OUTPUT in fp32 with exact zeros planted (and exact +-1 for tanh, 1 for sigmoid)."""
    a = R.act(torch.randn(n, generator=g).double() * 2, name).float()
    a[::7] = 0.0
    if name == "tanh":
        a[3::11] = 1.0
        a[5::13] = -1.0
    if name == "sigmoid":
        a[3::11] = 1.0
    return a


# 1 | 3 | 4 (the float4 body's first element) | 1023 | 1025 | 4096 * 1024 + 13: past the 4096 x 256
# threads of the capped grid, so the float4 loop strides a second time
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1025, 4096 * 1024 + 13])
def test_act_backward(K, n):
    g = torch.Generator().manual_seed(n)
    for name in (R.ACTS if n < 1 << 20 else ("lrelu", "tanh")):
        a, da, add = act_outputs(n, name, g), torch.randn(n, generator=g), torch.randn(n, generator=g)
        ref, ref_add = R.act_backward(da, a, name), R.act_backward(da, a, name, add=add)
        # (the large n 4 bytes off once: the scalar body's second sweep)
        for mis in (False, True) if n < 1 << 20 or name == "lrelu" else (False,):
            ad, dad = flat(a, mis), flat(da, mis)
            route = "scalar(4 bytes off)" if mis else "float4"
            check("act_backward." + name, route, ["-"], K.act_backward(dad, ad, name, R.ALPHA).reshape(-1, 1),
                  ref.reshape(-1, 1), 1e-5)
            out = flat(torch.full((n,), float("nan")), mis)
            got = K.act_backward_ex(dad, ad, name, R.ALPHA, add=flat(add, mis), out=out)
            assert got is out
            check("act_backward_ex." + name, route + " add", ["-"], got.reshape(-1, 1), ref_add.reshape(-1, 1), 1e-5)
            out = flat(add, mis)
            K.act_backward_ex(dad, ad, name, R.ALPHA, add=out, out=out)
            check("act_backward_ex." + name, route + " aliased", ["-"], out.reshape(-1, 1), ref_add.reshape(-1, 1), 1e-5)
            check("act_backward_ex." + name, route, ["-"],
                  K.act_backward_ex(dad, ad, name, R.ALPHA).reshape(-1, 1), ref.reshape(-1, 1), 1e-5)


# 8192 * 256 + 5: the capped grid of 8192 blocks strides a second time
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1025, 8192 * 256 + 5])
def test_scale(K, n):
    g = torch.Generator().manual_seed(n)
    t, s = torch.randn(n, generator=g), torch.tensor([0.37], device=DEV)
    for mis in (False, True):
        td = flat(t, mis)
        ref = R.scale(t, s.item()).reshape(-1, 1)
        check("scale", "4 bytes off" if mis else "aligned", ["-"], K.scale(td, s).reshape(-1, 1), ref, 1e-6)
        out = flat(torch.full((n,), float("nan")), mis)
        assert K.scale(td, s, out=out) is out
        check("scale", "out=", ["-"], out.reshape(-1, 1), ref, 1e-6)


# chsum_small (one launch) iff P <= 2048, C % 16 == 0, dense and aligned: (2048 | 2049) x (16 | 20);
# C = 6 scalar; a [B, C, 1, 1] slice with a batch stride (sp != C) leaves it as well
@pytest.mark.parametrize("P,C", [(2048, 16), (2049, 16), (2048, 20), (2049, 20), (130, 6), (1, 16), (5000, 64)])
def test_channel_sum(K, P, C):
    for i, (label, kinds) in enumerate(R.mixes(C)):
        d = R.inputs(P, C, kinds, seed=8000 + i)
        t = dev(d["y"])
        ref = R.channel_sum(d["y"])
        small = P <= 2048 and C % 16 == 0
        q = 4 if C % 4 == 0 else 1
        out, names = ran(lambda: K.channel_sum(t, torch.full((C,), float("nan"), device=DEV)))
        assert names == (["chsum_small"] if small else sorted([f"chsum_partial<{q}>", "chsum_merge"])), names
        route = "chsum_small" if small else f"chsum_partial<{q}>"
        check("channel_sum", route, kinds, out, ref, 1e-6)
        g = torch.Generator().manual_seed(P)
        base = torch.randn(C, generator=g)
        acc = K.channel_sum(t, vec(base), accumulate=True)
        check("channel_sum", route + " accumulate", kinds, host(acc) - base.double(), ref, 1e-6,
              floor=4 * R.U * (base.double().abs() + ref.abs()))   # one fp32 addition onto the buffer
    # a [B, C, 1, 1] slice of a wider tensor: pixel stride 2 C
    wide = torch.randn(P, 2 * C, 1, 1, device=DEV)
    sl = wide[:, :C]
    assert sl.stride()[0] == 2 * C and K.is_nhwc(sl)
    out, names = ran(lambda: K.channel_sum(sl, torch.empty(C, device=DEV)))
    assert names == sorted([f"chsum_partial<1>", "chsum_merge"]), names
    s64 = sl.double().cpu().reshape(P, C)
    check("channel_sum", "batch stride", ["-"] * C, out, s64.sum(0), 1e-6)
