"""The sliced Wasserstein metric end to end on the MI355X: SlicedWasserstein against the float64
restatement (tests/swd_ref.py) under the bound derived there, its private draws against a host
replay of the stream (tests/rng_ref.py), python -m relativisticgan_amd.evaluate, and
--rgan_swd_every leaving the training state bit for bit what it is without the flag."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

from tests import rng_ref
from tests import swd_ref as ref

pytestmark = pytest.mark.gpu

SMALL = ["--image_size", "32", "--batch_size", "8", "--z_size", "16", "--G_h_size", "8", "--D_h_size", "8",
         "--rgan_synthetic", "64"]
CASES = [dict(N=8, C=3, S=32, P=16, R=2, D=8), dict(N=6, C=1, S=64, P=5, R=1, D=3)]
_CACHE = {}


def _case(i):
    """One configuration's images, metric object, read-back draws and reference value, computed once."""
    if i in _CACHE:
        return _CACHE[i]
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.swd import SlicedWasserstein
    c = CASES[i]
    rng = np.random.default_rng(40 + i)
    # smooth structure plus noise, so the levels differ between the sets and between themselves
    base = rng.integers(0, 256, size=(2, c["N"], c["C"], c["S"] // 8, c["S"] // 8)).repeat(8, axis=3).repeat(8, axis=4)
    noise = rng.integers(-30, 31, size=base.shape)
    real, fake = (np.clip(base[k] + noise[k] * (1 + k), 0, 255).astype(np.uint8) for k in range(2))
    p = make_param(image_size=c["S"], n_colors=c["C"])
    kw = dict(n_images=c["N"], patches=c["P"], repeats=c["R"], dirs=c["D"], seed=5)
    sw = SlicedWasserstein(torch.from_numpy(real).cuda(), p, **kw)
    pos = {s: sw.pos[s].cpu().numpy() for s in sw.sides}
    dirs = [d.cpu().numpy().astype(np.float64) for d in sw.dirs]
    _CACHE[i] = dict(c=c, p=p, kw=kw, real=real, fake=fake, sw=sw, pos=pos, dirs=dirs,
                     want=ref.swd(real, fake, pos, dirs))
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_distance_against_float64(i):
    """|gpu - ref| per level <= the largest projection error of the real set plus that of the
    generated set (sorting is 1-Lipschitz in the max norm), each being ref.metric_bound: the fp32
    accumulation, the roundings of descriptors and directions, and the pyramid level's error through
    the normalisation.  Worst ratios seen on an MI355X: see profiles/swd_mi355x.txt."""
    k = _case(i)
    c, sw = k["c"], k["sw"]
    got = sw.distance(torch.from_numpy(k["fake"]).cuda())
    assert list(got) == ref.sides(c["S"]) + ["avg"]
    da, db = ref.descriptors(k["real"], k["pos"]), ref.descriptors(k["fake"], k["pos"])
    sa, sb = ref.min_std(k["real"], k["pos"]), ref.min_std(k["fake"], k["pos"])
    lev = ref.level_bounds(c["S"])
    total = 0.0
    for s in ref.sides(c["S"]):
        bound = 1000.0 * max(ref.metric_bound(da[s], d, lev[s], sa[s]) + ref.metric_bound(db[s], d, lev[s], sb[s])
                             for d in k["dirs"])
        err = abs(got[s] - k["want"][s])
        print(f"case {i} level {s}: gpu {got[s]:.6f} ref {k['want'][s]:.6f} |diff| {err:.3e} bound {bound:.3e} "
              f"ratio {err / bound:.3e}")
        assert k["want"][s] > 1.0  # the sets differ: the check is not vacuous
        assert err <= bound
        total += bound
    assert abs(got["avg"] - k["want"]["avg"]) <= total / len(ref.sides(c["S"]))
    # HWC bytes (what the PNG writer holds) give the same bits as CHW
    hwc = torch.from_numpy(np.ascontiguousarray(k["fake"].transpose(0, 2, 3, 1))).cuda()
    assert sw.distance(hwc) == got


@pytest.mark.parametrize("i", range(len(CASES)))
def test_zero_on_itself_symmetric_and_repeatable(i):
    from relativisticgan_amd.swd import SlicedWasserstein
    k = _case(i)
    sw = k["sw"]
    real, fake = torch.from_numpy(k["real"]).cuda(), torch.from_numpy(k["fake"]).cuda()
    assert all(v == 0.0 for v in sw.distance(real).values())
    ab = sw.distance(fake)
    assert sw.distance(fake) == ab
    other = SlicedWasserstein(fake, k["p"], **k["kw"])
    assert other.distance(real) == ab
    for s in sw.sides:  # the same seed: the same draws, bit for bit
        assert torch.equal(other.pos[s], sw.pos[s])
    assert all(torch.equal(a, b) for a, b in zip(other.dirs, sw.dirs))
    third = SlicedWasserstein(real, k["p"], **dict(k["kw"], seed=6))
    assert any(not torch.equal(third.pos[s], sw.pos[s]) for s in sw.sides)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_draws_are_a_host_replay_of_the_private_stream(i):
    from relativisticgan_amd import swd
    k = _case(i)
    c, sw = k["c"], k["sw"]
    seed, base = swd.private_seed(5), 0
    assert sw.seed == seed != rng_ref.mix_seed(5)  # never the training stream's key
    for s in sw.sides:
        n = c["N"] * c["P"] * 2
        u = rng_ref.fill_uniform(seed, base, n)
        base += rng_ref.quads(n)
        want = ref.positions(u, s).reshape(c["N"], c["P"], 2)
        assert np.array_equal(k["pos"][s], want), s
        assert want.min() >= 3 and want.max() <= s - 4
    Kd = 49 * c["C"]
    for r in range(c["R"]):
        n = Kd * c["D"]
        z, rad = rng_ref.fill_normal(seed, base, n)
        base += rng_ref.quads(n)
        z = z.reshape(Kd, c["D"])
        norm = np.sqrt((z * z).sum(axis=0))
        # a device normal is within 13 ulp of its radius (tests/test_rng_gpu.py); the norm moves by no more
        tol = 2 * 13 * 2.0 ** -23 * rad.max() / norm.min() + 2.0 ** -22
        assert np.abs(k["dirs"][r] - z / norm).max() <= tol, r
        assert np.abs((k["dirs"][r] ** 2).sum(axis=0) - 1).max() < 1e-6
    assert int(sw.counter.item()) == base  # nothing else was drawn
    before = torch.cuda.get_rng_state().clone(), torch.get_rng_state().clone()
    sw.normal((5, 16, 1, 1))
    assert int(sw.counter.item()) == base + rng_ref.quads(80)
    assert torch.equal(before[0], torch.cuda.get_rng_state()) and torch.equal(before[1], torch.get_rng_state())


def _checkpoint(root):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    p = make_param(loss_D=7, image_size=32, batch_size=8, z_size=16, G_h_size=8, D_h_size=8, seed=1)
    t = Trainer(p, synthetic_images(64, 32))
    t.iteration(0)
    t.iteration(1)
    path = os.path.join(root, "state_01.pth")
    torch.save(t.state(2, 1), path)
    return path


def test_evaluate_cli(capsys):
    from relativisticgan_amd.evaluate import main
    path = _checkpoint(tempfile.mkdtemp())
    capsys.readouterr()
    result = main(["--load", path, *SMALL, "--rgan_swd_images", "64", "--seed", "3"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("SWD x1e3")]
    assert len(line) == 1
    m = re.fullmatch(r"SWD x1e3  32: ([0-9.]+)  16: ([0-9.]+)  avg: ([0-9.]+)", line[0])
    assert m, line[0]
    vals = [float(v) for v in m.groups()]
    assert all(np.isfinite(v) and v > 0 for v in vals) and list(result) == [32, 16, "avg"]
    with pytest.raises(SystemExit, match="holds no averaged generator"):
        main(["--load", path, *SMALL, "--rgan_swd_images", "64", "--rgan_ema_G", "0.999"])


def _same(a, b, where=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for key in a:
            _same(a[key], b[key], f"{where}/{key}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for j, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}/{j}")
    else:
        assert a == b, where


@pytest.mark.parametrize("extra", [[], ["--rgan_ema_G", "0.9", "--rgan_pac", "2"]], ids=["G", "ema_pac2"])
def test_training_state_is_untouched_by_the_metric(extra):
    """With and without --rgan_swd_every: the same Trainer.state() (BN buffers, optimizer state, the
    averaged generator with --rgan_ema_G), the same RNG states, two SWD lines in the log."""
    from relativisticgan_amd.train import main
    root = tempfile.mkdtemp()
    states, rngs, logs = [], [], []
    for name, more in (("plain", []), ("swd", ["--rgan_swd_every", "2", "--rgan_swd_images", "64"])):
        out = os.path.join(root, name)
        t = main(["--loss_D", "7", *SMALL, "--seed", "1", "--n_iter", "4", "--print_every", "2", "--gen_every", "100",
                  "--gen_extra_images", "0", "--output_folder", out, "--extra_folder", os.path.join(root, name + "_x"),
                  *extra, *more])
        states.append(t.state(4, 0))
        rngs.append((torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(),
                     np.random.get_state()[1].copy(), np.random.get_state()[2],
                     None if t.dev_rng is None else int(t.dev_rng.counter.item())))
        logs.append(open(os.path.join(out, "RaLSGAN_seed1-0", "logs", "log.txt")).read())
    _same(states[0], states[1], "state")
    assert any("running_mean" in key for key in states[0]["G_state"])  # BN buffers are part of what was compared
    assert "G_optimizer" in states[0] and "D_optimizer" in states[0] and ("G_ema" in states[0]) == bool(extra)
    for a, b in zip(rngs[0], rngs[1]):
        assert (torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b))
    lines = re.findall(r"^\[(\d+)\] SWD x1e3  32: ([0-9.]+)  16: ([0-9.]+)  avg: ([0-9.]+)$", logs[1], re.M)
    assert [ln[0] for ln in lines] == ["1", "3"] and logs[1].count("SWD") == 2 and "SWD" not in logs[0]
    assert all(float(v) > 0 for ln in lines for v in ln[1:])
