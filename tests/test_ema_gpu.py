"""--rgan_ema_G on the MI355X: rgan_ema_update against float64, and the average through every
layer above it (operator, GeneratorEMA, Trainer eager / HIP graph / deferred data-parallel
step, checkpoints, generate.py, the training CLI).

Bounds.  One update is avg + w (p - avg) with w = (float)(1 - beta_t) taken alike on both
sides: the subtraction, the product-sum (one fma) and the result round once each, at most
2^-24 of a value no larger than 2 max(|avg|, |p|), so an element is within
8 * 2^-24 * max(|avg|, |p|) of the float64 value (BOUND1).  Every beta_t <= 1 makes an update a
convex combination: an error made at one update is not amplified by the next, so n updates stay
within n * BOUND1 with the largest magnitude seen.
"""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 8 * 2.0 ** -24
GOLDEN_CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ralsgan_ckpt_state_01.pth")
TINY = dict(loss_D=7, image_size=32, batch_size=8, z_size=16, G_h_size=8, D_h_size=8, seed=1)
TINY_CLI = ["--image_size", "32", "--z_size", "16", "--G_h_size", "8"]


def _w(beta, warmup, t):
    """The kernel's weight at update t: 1 - beta_t in double, rounded to float."""
    beta_t = min(beta, (1.0 + t) / (10.0 + t)) if warmup else beta
    return float(np.float32(1.0 - beta_t))


def _hyper(beta, warmup):
    return torch.tensor([beta, float(warmup)], dtype=torch.float64, device=DEV)


# ---------------------------------------------------------------- 1. one update against fp64
SIZES = [1, 3, 4, 4095, 4096, 4097, 8197, (16, 8, 4, 4)]
NTENSORS = 50  # > 48: two chunks


def _cut(values, misaligned):
    """``values`` inside a NaN-filled buffer: at float offset 1 (4-byte aligned only) or 4."""
    n, lead = values.numel(), 1 if misaligned else 4
    buf = torch.full((n + 2 * lead,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[lead:lead + n]
    view.copy_(values.reshape(-1))
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return buf, view.view(values.shape), lead


def _multi_case():
    """50 (avg, p) pairs over SIZES; tensor j has avg misaligned when j % 4 == 1, p when
    j % 4 == 2, both when j % 4 == 3.  Host float64 copies of the values come along."""
    gen = torch.Generator().manual_seed(11)
    case = {"bufs": [], "avgs": [], "ps": [], "a64": [], "p64": []}
    for j in range(NTENSORS):
        shape = SIZES[j % len(SIZES)]
        shape = shape if isinstance(shape, tuple) else (shape,)
        a = torch.randn(shape, generator=gen) * (10.0 ** (j % 3 - 1))
        p = torch.randn(shape, generator=gen)
        ba, av, la = _cut(a, j % 4 in (1, 3))
        bp, pv, lp = _cut(p, j % 4 in (2, 3))
        case["bufs"].append((ba, la, bp, lp, a.numel()))
        case["avgs"].append(av)
        case["ps"].append(pv)
        case["a64"].append(a.double())
        case["p64"].append(p.double())
    return case


def _run_multi(beta, warmup):
    from relativisticgan_amd import kernels as K
    case = _multi_case()
    count = torch.zeros(1, device=DEV)
    K.ema_update(case["avgs"], case["ps"], _hyper(beta, warmup), count)
    torch.cuda.synchronize()
    case["count"] = count.item()
    return case


MODES = {"plain": (0.999, False), "ramp": (0.999, True)}  # w = 0.001 (< 1/2) and 9/11 (>= 1/2)
_MULTI = {}


def _multi(mode):
    if mode not in _MULTI:
        _MULTI[mode] = _run_multi(*MODES[mode])
    return _MULTI[mode]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_update_matches_float64(mode):
    case = _multi(mode)
    w = _w(*MODES[mode], 1)
    assert case["count"] == 1.0
    worst = 0.0
    for j in range(NTENSORS):
        ba, la, bp, lp, n = case["bufs"][j]
        a64, p64 = case["a64"][j], case["p64"][j]
        want = a64 + w * (p64 - a64)
        got = case["avgs"][j].double().cpu()
        err = (got - want).abs()
        bound = EPS * torch.maximum(a64.abs(), p64.abs())
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all()), (mode, j, tuple(a64.shape), err.max().item())
        # the guards on both sides of both buffers are still NaN, and p is untouched
        for buf, lead in ((ba, la), (bp, lp)):
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all()), (mode, j)
            assert not bool(torch.isnan(buf[lead:lead + n]).any())
        assert torch.equal(case["ps"][j].cpu().view(torch.int32), p64.float().view(torch.int32)), (mode, j)
    print(f"{mode}: worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------- 2. warm-up, cap, beta = 0
def test_warmup_ramp_and_cap():
    from relativisticgan_amd import kernels as K
    gen = torch.Generator().manual_seed(5)
    n, beta = 8197, 0.5
    assert (1 + 8) / (10 + 8) == beta  # the ramp crosses beta at t = 8: 12 calls cover ramp and clamp
    a64 = torch.randn(n, generator=gen).double()
    avg, count, hyper = a64.float().to(DEV), torch.zeros(1, device=DEV), _hyper(beta, True)
    M = a64.abs().max().item()
    for t in range(1, 13):
        p = torch.randn(n, generator=gen)
        M = max(M, p.abs().max().item())
        K.ema_update([avg], [p.to(DEV)], hyper, count)
        a64 = a64 + _w(beta, True, t) * (p.double() - a64)
        err = (avg.double().cpu() - a64).abs().max().item()
        print(f"t={t} w={_w(beta, True, t):.6f} err={err:.3e} bound={t * EPS * M:.3e}")
        assert err <= t * EPS * M, t
    assert count.item() == 12.0
    assert _w(beta, True, 7) > 0.5 == _w(beta, True, 8) == _w(beta, True, 12)

    # warm-up off: the first call already uses beta
    a0, p = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    avg, count = a0.to(DEV), torch.zeros(1, device=DEV)
    K.ema_update([avg], [p.to(DEV)], _hyper(beta, False), count)
    want = a0.double() + 0.5 * (p.double() - a0.double())
    assert bool(((avg.double().cpu() - want).abs() <= EPS * torch.maximum(a0.abs(), p.abs()).double()).all())
    assert count.item() == 1.0
    # beta = 0: the average is p itself, bit for bit, with and without warm-up
    for warm in (False, True):
        avg, pd = a0.to(DEV), p.to(DEV)
        K.ema_update([avg], [pd], _hyper(0.0, warm), torch.zeros(1, device=DEV))
        assert torch.equal(avg.view(torch.int32), pd.view(torch.int32)), warm


# ---------------------------------------------------------------- 3. determinism
def test_two_runs_give_the_same_bits():
    first, second = _multi("plain"), _run_multi(*MODES["plain"])
    for a, b in zip(first["avgs"], second["avgs"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------- 4. argument checks
class _Counter:
    """The C-ABI library behind a proxy that counts calls per entry point (the approach of
    tools/abi_trace.py and tests/test_diffaug_gpu.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rgan_"):
            return fn

        def wrapped(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return wrapped


def test_argument_checks_raise_before_any_launch():
    from relativisticgan_amd import _lib as L
    from relativisticgan_amd import kernels as K
    a, p = torch.zeros(4, 6, device=DEV), torch.ones(4, 6, device=DEV)
    hyper, count = _hyper(0.9, True), torch.zeros(1, device=DEV)
    bad = {
        "cpu avg": ([a.cpu()], [p]),
        "cpu p": ([a], [p.cpu()]),
        "fp16 avg": ([a.half()], [p]),
        "fp16 p": ([a], [p.half()]),
        "shape": ([torch.zeros(6, 4, device=DEV)], [p]),
        "numel": ([torch.zeros(4, 5, device=DEV)], [p]),
        "strides": ([torch.zeros(6, 4, device=DEV).t()], [p]),
        "count": ([a, a.clone()], [p]),
    }
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        for what, (avgs, ps) in bad.items():
            with pytest.raises(L.RganError):
                K.ema_update(avgs, ps, hyper, count)
        with pytest.raises(L.RganError):
            K.ema_update([a], [p], hyper.float(), count)
        with pytest.raises(L.RganError):
            K.ema_update([a], [p], hyper.cpu(), count)
    finally:
        L._LIB = real
    torch.cuda.synchronize()
    assert proxy.calls == {} and count.item() == 0.0 and not bool(a.any())
    # a transposed pair that shares its strides is walked flat, like Adam's
    at, pt = torch.zeros(6, 4, device=DEV).t(), torch.ones(6, 4, device=DEV).t()
    K.ema_update([at], [pt], _hyper(0.0, False), count)
    assert torch.equal(at, pt) and count.item() == 1.0
    # no tensors: nothing happens, the count stays
    K.ema_update([], [], hyper, count)
    assert count.item() == 1.0


# ---------------------------------------------------------------- 5. the operator
def test_opcheck_ema_update():
    from relativisticgan_amd import ops  # noqa: F401
    ps = [torch.randn(33, device=DEV), torch.randn(4, 8, device=DEV)]
    torch.library.opcheck(torch.ops.rgan.ema_update_.default,
                          ([torch.randn_like(p) for p in ps], ps, _hyper(0.9, True), torch.zeros(1, device=DEV)),
                          test_utils=("test_schema", "test_faketensor"))


# ---------------------------------------------------------------- 6. a captured update
def _tiny_G():
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_G, weights_init
    p = make_param(**TINY)
    torch.manual_seed(1)
    G = DCGAN_G(p)
    G.apply(weights_init)
    return G.to(DEV), p


def _ema_bits(ema):
    sd = ema.state_dict()
    return sd["num_updates"], {k: v.detach().clone() for k, v in sd["G_ema_state"].items()}


def _same_ema(a, b):
    (na, sa), (nb, sb) = _ema_bits(a), _ema_bits(b)
    assert list(sa) == list(sb)
    return na == nb and not [k for k in sa if not torch.equal(sa[k], sb[k])]


def test_captured_update_follows_counter_weights_and_beta():
    from relativisticgan_amd.ema import GeneratorEMA
    G, p = _tiny_G()
    GeneratorEMA(G, p, 0.9).update()  # (first use outside the capture)
    A, B = GeneratorEMA(G, p, 0.9), GeneratorEMA(G, p, 0.9)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        B.update()
    assert B.num_updates == 0  # a capture runs nothing
    gen = torch.Generator(device=DEV)
    gen.manual_seed(2)
    start = {k: v.clone() for k, v in B.shadow.state_dict().items()}
    for k, beta in enumerate((0.9, 0.3, 0.9, 0.99), 1):
        with torch.no_grad():
            for q in G.parameters():
                q.add_(torch.randn(q.shape, device=DEV, generator=gen) * 0.1)
        for e in (A, B):
            e.hyper[:1].fill_(beta)
        A.update()
        graph.replay()
        torch.cuda.synchronize()
        assert A.num_updates == B.num_updates == k
        assert _same_ema(A, B), k
    moved = [k for k, v in B.shadow.state_dict().items() if v.is_floating_point() and not torch.equal(v, start[k])]
    assert len(moved) >= len(list(G.parameters()))


# ---------------------------------------------------------------- 7. trainer: eager vs graph
def _trainer(ema=0.9, **kw):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    cfg = dict(image_size=32, batch_size=8, G_h_size=16, D_h_size=16, seed=1, print_every=10 ** 9,
               rgan_rng="device", loss_D=7)
    cfg.update(kw)
    if ema is not None:
        cfg["rgan_ema_G"] = ema
    return Trainer(make_param(**cfg), synthetic_images(64, 32, device=DEV))


def _feed(t, gen):
    p = t.p
    return {"x_D": torch.rand(8, 3, 32, 32, device=DEV, generator=gen) * 2 - 1,
            "z_D": torch.randn(8, p.z_size, 1, 1, device=DEV, generator=gen),
            "z_G": torch.randn(8, p.z_size, 1, 1, device=DEV, generator=gen),
            "x_G": torch.rand(8, 3, 32, 32, device=DEV, generator=gen) * 2 - 1}


def _state(t):
    out = {f"G.{k}": v.detach().clone() for k, v in t.G.state_dict().items()}
    out.update({f"D.{k}": v.detach().clone() for k, v in t.D.state_dict().items()})
    for name, opt in (("optG", t.optG), ("optD", t.optD)):
        for i, (p, st) in enumerate(opt.state.items()):
            out[f"{name}.{i}.m"] = st["exp_avg"].detach().clone()
            out[f"{name}.{i}.v"] = st["exp_avg_sq"].detach().clone()
    return out


def test_trainer_graph_replay_matches_eager():
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    A, B = _trainer(), _trainer()
    feeds = [_feed(A, gen) for _ in range(4)]
    z = torch.randn(8, A.p.z_size, 1, 1, device=DEV, generator=gen)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.iteration(1, feed=feeds[0])
        B.iteration(1, feed=feeds[0])
        with torch.no_grad():  # B's layouts of the averaged weights are cached from here on
            assert torch.equal(A.ema.generator()(z), B.ema.generator()(z))
    static = {k: v.clone() for k, v in feeds[0].items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        B.iteration(2, feed=static)
    for j in range(1, 4):
        with torch.cuda.stream(side):
            A.iteration(1 + j, feed=feeds[j])
            for k, v in feeds[j].items():
                static[k].copy_(v)
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        assert A.ema.num_updates == B.ema.num_updates == 1 + j
        assert _same_ema(A.ema, B.ema), j
        # the replays moved B's averages under unchanged host-side versions: the layouts cached
        # by the previous forward must not be served again
        with torch.no_grad():
            ya, yb = A.ema.generator()(z), B.ema.generator()(z)
        assert torch.equal(ya, yb), j
        assert any(not torch.equal(a, b) for a, b in zip(B.ema.shadow.parameters(), B.G.parameters()))


# ---------------------------------------------------------------- 8. trainer against the definition
def test_trainer_average_is_the_recursion_and_leaves_training_alone():
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    on, off = _trainer(0.9), _trainer(None)
    assert off.ema is None
    feeds = [_feed(on, gen) for _ in range(3)]
    names = [n for n, _ in on.G.named_parameters()]
    avg = {n: q.detach().double().cpu() for n, q in on.G.named_parameters()}
    big = {n: v.abs().max().item() for n, v in avg.items()}
    snaps = []

    def hooks(tag, rec):
        if tag == "G.post":
            snaps.append({n: q.detach().double().cpu() for n, q in on.G.named_parameters()})

    for i, f in enumerate(feeds):
        on.iteration(1 + i, feed=f, hooks=hooks)
        off.iteration(1 + i, feed=f)
    torch.cuda.synchronize()
    assert len(snaps) == 3 and on.ema.num_updates == 3
    for t, snap in enumerate(snaps, 1):
        w = _w(0.9, True, t)
        for n in names:
            avg[n] = avg[n] + w * (snap[n] - avg[n])
            big[n] = max(big[n], snap[n].abs().max().item())
    got = dict(on.ema.shadow.named_parameters())
    assert list(got) == names
    for n in names:
        err = (got[n].detach().double().cpu() - avg[n]).abs().max().item()
        assert err <= 3 * EPS * big[n], (n, err, 3 * EPS * big[n])
        assert not got[n].requires_grad
    so, sf = _state(on), _state(off)
    assert list(so) == list(sf)
    bad = [k for k in so if not torch.equal(so[k], sf[k])]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- 9. the deferred G step
DP_ITERS = 2


def _dp_run(forced):
    """DP_ITERS free-running iterations (host draws from the seed) without a flush between
    them, then one flush.  Returns the averaged weights, G's weights after each optimizer step
    and the update counts seen on the way."""
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    p = make_param(print_every=10 ** 9, rgan_rng="host", rgan_ema_G=0.9, **TINY)
    t = Trainer(p, synthetic_images(64, 32, device=DEV))
    assert (t.redG is not None) == forced
    snaps, counts, pending = [], [], []

    def hooks(tag, rec):
        if tag == "G.post":
            snaps.append({n: q.detach().cpu().clone() for n, q in t.G.named_parameters()})

    for i in range(1, 1 + DP_ITERS):
        t.iteration(i, hooks=hooks)
        pending.append(t._pending_G is not None)
        counts.append(t.ema.num_updates)
    t.flush()
    sd = t.ema.state_dict()
    return {"avg": {k: v.detach().cpu().clone() for k, v in sd["G_ema_state"].items()},
            "num_updates": sd["num_updates"], "snaps": snaps, "counts": counts, "pending": pending}


def _dp_worker(port, path):
    import torch.distributed as dist
    from relativisticgan_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    dp.setup(sync_bn=False, force=True)
    try:
        torch.save(_dp_run(True), path)
    finally:
        dist.destroy_process_group()


def test_deferred_G_step_updates_the_average():
    """The forced one-rank data-parallel path (as tests/test_dp_gpu.py's
    test_dp1_rccl_forced_matches_single_process) in a fresh child process: G's optimizer step,
    and with it the average's update, waits for the next use of G.  The average is a convex
    combination of the initial weights (the same on both sides) and G's weights after each
    step, so it may differ from the plain run's by no more than those weights do (the
    distributed loss heads sum in another order), plus both sides' rounding."""
    import torch.multiprocessing as mp
    single = _dp_run(False)
    assert single["pending"] == [False] * DP_ITERS and single["counts"] == [1, 2]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    path = os.path.join(tempfile.mkdtemp(), "dp_ema.pt")
    proc = mp.get_context("spawn").Process(target=_dp_worker, args=(port, path))
    proc.start()
    proc.join(300)
    assert proc.exitcode == 0
    forced = torch.load(path, weights_only=True)
    # deferred: after iteration i the i-th G step, and its update, are still pending
    assert forced["pending"] == [True] * DP_ITERS and forced["counts"] == [0, 1]
    assert forced["num_updates"] == single["num_updates"] == DP_ITERS
    assert len(forced["snaps"]) == len(single["snaps"]) == DP_ITERS
    exact = 0
    for n, want in single["avg"].items():
        got = forced["avg"][n]
        if not want.is_floating_point() or n not in single["snaps"][0]:
            continue
        drift = torch.stack([(a[n].double() - b[n].double()).abs()
                             for a, b in zip(forced["snaps"], single["snaps"])]).max(0).values
        big = max(s_[n].abs().max().item() for s_ in single["snaps"] + forced["snaps"])
        err = (got.double() - want.double()).abs()
        exact += int(torch.equal(got, want))
        assert bool((err <= drift + 2 * DP_ITERS * EPS * big).all()), (n, err.max().item(), drift.max().item())
    print(f"bitwise-equal averaged tensors: {exact}")


# ---------------------------------------------------------------- 10. flag off
def _count_calls(ema, **kw):
    from relativisticgan_amd import _lib as L
    t = _trainer(ema, **kw)
    real = L.lib()
    proxy = L._LIB = _Counter(real)
    try:
        t.iteration(1)
        t.flush()
        torch.cuda.synchronize()
    finally:
        L._LIB = real
    return t, proxy.calls


@pytest.mark.parametrize("kw", [dict(loss_D=7), dict(loss_D=1, Giters=2)], ids=["ralsgan", "sgan_giters2"])
def test_flag_off_makes_no_ema_call(kw):
    t_off, off = _count_calls(None, **kw)
    t_on, on = _count_calls(0.999, **kw)
    assert t_off.ema is None and t_on.ema is not None
    assert off.get("rgan_conv_fwd", 0) + off.get("rgan_conv_fwd_bn", 0) > 0  # the proxy sees the step
    assert "rgan_ema_update" not in off, off
    assert on.get("rgan_ema_update", 0) == kw.get("Giters", 1), on
    assert t_on.ema.num_updates == kw.get("Giters", 1)
    rest = {k: v for k, v in on.items() if k != "rgan_ema_update"}
    assert rest == off, {k: (off.get(k), rest.get(k)) for k in set(off) | set(rest) if off.get(k) != rest.get(k)}


# ---------------------------------------------------------------- 11. checkpoints
REF_KEYS = {"i", "current_set_images", "G_state", "D_state", "G_optimizer", "D_optimizer", "G_scheduler",
            "D_scheduler", "z_test"}


def _tiny_trainer(ema=0.9):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    kw = dict(TINY, print_every=10 ** 9)
    if ema is not None:
        kw["rgan_ema_G"] = ema
    return Trainer(make_param(**kw), synthetic_images(64, 32, device=DEV))


@pytest.fixture(scope="module")
def saved():
    """A flag-on trainer after two fed iterations, its checkpoint on disk, and two more feeds."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(6)
    t = _tiny_trainer()
    feeds = [_feed(t, gen) for _ in range(4)]
    for i in range(2):
        t.iteration(i, feed=feeds[i])
    path = os.path.join(tempfile.mkdtemp(), "state_01.pth")
    st = t.state(2, 1)
    assert set(st) == REF_KEYS | {"G_ema"}
    assert set(st["G_ema"]) == {"beta", "warmup", "num_updates", "G_ema_state"}
    assert (st["G_ema"]["beta"], st["G_ema"]["warmup"], st["G_ema"]["num_updates"]) == (0.9, True, 2)
    torch.save(st, path)
    return {"trainer": t, "path": path, "feeds": feeds}


def test_checkpoint_round_trip(saved):
    from relativisticgan_amd.nets import DCGAN_G
    t = saved["trainer"]
    ck = torch.load(saved["path"], weights_only=True)
    plain = DCGAN_G(t.p)
    plain.load_state_dict(ck["G_ema"]["G_ema_state"])  # strict: G's keys
    assert list(ck["G_ema"]["G_ema_state"]) == list(plain.state_dict())
    u = _tiny_trainer()
    assert u.load(ck) == (2, 1)
    assert _same_ema(t.ema, u.ema) and u.ema.num_updates == 2
    assert any(not torch.equal(a, b) for a, b in zip(u.ema.shadow.parameters(), u.G.parameters()))
    for i in (2, 3):
        t.iteration(i, feed=saved["feeds"][i])
        u.iteration(i, feed=saved["feeds"][i])
        assert _same_ema(t.ema, u.ema), i
    assert u.ema.num_updates == 4
    z = torch.randn(8, t.p.z_size, 1, 1, device=DEV)
    with torch.no_grad():
        assert torch.equal(t.ema.generator()(z), u.ema.generator()(z))


def test_flag_off_checkpoint_keeps_the_reference_keys():
    t = _tiny_trainer(None)
    t.iteration(0)
    assert set(t.state(1, 1)) == REF_KEYS


def test_reference_checkpoint_starts_the_average_at_its_G():
    t = _tiny_trainer()
    t.iteration(0)
    assert t.ema.num_updates == 1
    ck = torch.load(GOLDEN_CKPT, weights_only=True)
    assert "G_ema" not in ck
    t.load(ck)
    sd = t.ema.state_dict()
    assert sd["num_updates"] == 0
    assert list(sd["G_ema_state"]) == list(ck["G_state"])
    for k, v in ck["G_state"].items():
        assert torch.equal(sd["G_ema_state"][k].cpu(), v), k


# ---------------------------------------------------------------- 12. generate.py
def test_generate_uses_the_averaged_generator(saved):
    from relativisticgan_amd.generate import main as gen
    from relativisticgan_amd.images import save_images
    root = tempfile.mkdtemp()
    common = ["--load", saved["path"], *TINY_CLI, "--gen_extra_images", "100", "--seed", "3"]
    f_ema = gen(common + ["--extra_folder", os.path.join(root, "ema"), "--rgan_ema_G", "0.9"])
    f_raw = gen(common + ["--extra_folder", os.path.join(root, "raw")])
    names = ["fake_samples_%05d.png" % k for k in range(100)]
    assert sorted(os.listdir(f_ema)) == sorted(os.listdir(f_raw)) == names

    def read(folder, name):
        with open(os.path.join(folder, name), "rb") as f:
            return f.read()

    differ = sum(read(f_ema, n) != read(f_raw, n) for n in names)
    print(f"{differ} of 100 files differ from the flag-off run's")
    assert differ > 0
    # the same images from the trainer-side object: a fresh trainer resumed from the file
    u = _tiny_trainer()
    u.load(torch.load(saved["path"], weights_only=True))
    torch.manual_seed(3)
    z = torch.randn(100, u.p.z_size, 1, 1, device=DEV)
    with torch.no_grad():
        fake = u.ema.generator()(z)
    want = os.path.join(root, "want")
    os.makedirs(want)
    save_images(fake, [os.path.join(want, n) for n in names])
    assert all(read(f_ema, n) == read(want, n) for n in names)
    # a checkpoint without the key: a clear exit, nothing written
    with pytest.raises(SystemExit, match="no averaged generator"):
        gen(["--load", GOLDEN_CKPT, *TINY_CLI, "--gen_extra_images", "100",
             "--extra_folder", os.path.join(root, "none"), "--rgan_ema_G", "0.9"])
    assert not os.path.exists(os.path.join(root, "none"))


# ---------------------------------------------------------------- the training CLI
def test_train_cli_writes_the_averaged_samples_and_checkpoint():
    from PIL import Image
    from relativisticgan_amd.train import main
    root = tempfile.mkdtemp()
    out, extra = os.path.join(root, "out"), os.path.join(root, "extra")
    t = main(["--loss_D", "7", "--image_size", "32", "--batch_size", "8", "--z_size", "16", "--G_h_size", "8",
              "--D_h_size", "8", "--seed", "1", "--n_iter", "3", "--print_every", "2", "--gen_every", "3",
              "--gen_extra_images", "100", "--output_folder", out, "--extra_folder", extra,
              "--rgan_synthetic", "64", "--rgan_ema_G", "0.9"])
    images = os.path.join(out, "RaLSGAN_seed1-0", "images")
    assert sorted(os.listdir(images)) == ["fake_samples_ema_iter00000.png", "fake_samples_ema_iter00002.png",
                                          "fake_samples_iter00000.png", "fake_samples_iter00002.png"]
    for i in (0, 2):
        own = np.asarray(Image.open(os.path.join(images, "fake_samples_iter%05d.png" % i)))
        avg = np.asarray(Image.open(os.path.join(images, "fake_samples_ema_iter%05d.png" % i)))
        assert own.shape == avg.shape == (32 + 2 + 2, 8 * (32 + 2) + 2, 3) and not np.array_equal(own, avg)
    ck = torch.load(os.path.join(extra, "models", "state_01.pth"), weights_only=True)
    assert set(ck) == REF_KEYS | {"G_ema"} and ck["G_ema"]["num_updates"] == 3 == t.ema.num_updates
    assert len(os.listdir(os.path.join(extra, "1"))) == 100
