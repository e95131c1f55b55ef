"""The nearest-training-image check end to end on the MI355X: NearestNeighbours against the numpy
restatement (tests/nn_ref.py), exactly; --rgan_nn_every leaving the training state bit for bit what
it is without the flag; python -m relativisticgan_amd.evaluate with and without --rgan_nn."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

from tests import nn_ref as ref

pytestmark = pytest.mark.gpu

SMALL = ["--image_size", "32", "--batch_size", "8", "--z_size", "16", "--G_h_size", "8", "--D_h_size", "8",
         "--rgan_synthetic", "64"]
LINE = (r"NN s(\d+) k(\d+)  fake->real: ([0-9.]+)  real->real: ([0-9.]+)  ratio: ([0-9.]+|inf)  "
        r"precision: ([0-9.]+)  recall: ([0-9.]+)")
_CACHE = {}


def _scenario(name):
    """(images on the device as the trainer holds them, their bytes, the fakes' bytes, side, k, object)."""
    if name in _CACHE:
        return _CACHE[name]
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.images import to_u8
    from relativisticgan_amd.neighbours import NearestNeighbours
    from relativisticgan_amd.train import synthetic_images
    if name == "grey":  # bytes as a decoded folder holds them, C = 1, box means of 2 x 2
        rng = np.random.default_rng(21)
        base = rng.integers(0, 256, size=(2, 40, 1, 8, 8)).repeat(8, axis=3).repeat(8, axis=4)
        real, fake = (np.clip(base[0] + rng.integers(-40, 41, size=base[0].shape) * (1 + j), 0, 255).astype(np.uint8)
                      for j in range(2))
        images, s, k = torch.from_numpy(real).cuda(), 32, 2
    else:  # the synthetic set: floats, compared as the bytes the PNG writer would store
        images, s, k = synthetic_images(64, 32), 16, 3
        real = to_u8(images, 0.5, 0.5).permute(0, 3, 1, 2).cpu().numpy()
        assert np.array_equal(real, ref.to_u8(images.cpu().numpy()))
        if name == "memorised":
            noise = np.random.default_rng(1).integers(-1, 2, size=real.shape)
            fake = np.clip(real.astype(np.int64) + noise, 0, 255).astype(np.uint8)
        else:
            fake = np.random.default_rng(2).integers(0, 256, size=real.shape, dtype=np.uint8)
    p = make_param(image_size=real.shape[2], n_colors=real.shape[1])
    nn = NearestNeighbours(images, p, n_images=real.shape[0], side=s, k=k, seed=5)
    _CACHE[name] = images, real, fake, s, k, nn, ref.report(real, fake, s, k)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["memorised", "independent", "grey"])
def test_report_query_and_grid_equal_the_reference(name):
    images, real, fake, s, k, nn, (want, cross) = _scenario(name)
    assert (nn.s, nn.k, nn.N, nn.D) == (s, k, real.shape[0], real.shape[1] * s * s)
    dev = torch.from_numpy(fake).cuda()
    got = nn.report(dev)
    print(name, got)
    assert list(got) == ["fake_nn", "real_nn", "ratio", "precision", "recall"]
    assert got == want  # float64 from equal integers through equal formulas
    if name == "memorised":
        assert got["ratio"] < 0.05 and got["precision"] == 1.0 and got["recall"] == 1.0
    elif name == "independent":
        assert 0.9 <= got["ratio"] <= 1.1
    hwc = torch.from_numpy(np.ascontiguousarray(fake.transpose(0, 2, 3, 1))).cuda()
    assert nn.report(hwc) == got  # the PNG writer's byte order gives the same numbers
    dist, idx = nn.query(dev)
    assert np.array_equal(dist.cpu().numpy(), cross[0]) and np.array_equal(idx.cpu().numpy(), cross[1])
    if name == "memorised":
        assert np.array_equal(cross[1][:, 0], np.arange(64))
    dist3, idx3 = nn.query(hwc[:3])
    assert np.array_equal(dist3.cpu().numpy(), cross[0][:3]) and np.array_equal(idx3.cpu().numpy(), cross[1][:3])
    rdesc, _ = ref.pack(real, s)
    want_knn = ref.topk(rdesc, rdesc, k, 0)
    assert np.array_equal(nn.real_knn[0].cpu().numpy(), want_knn[0])
    assert np.array_equal(nn.real_knn[1].cpu().numpy(), want_knn[1])
    for view in (dev, hwc):
        g = nn.grid(view, idx)
        S = real.shape[2]
        assert g.dtype == torch.uint8 and tuple(g.shape) == ((S + 2) * 8 + 2, (S + 2) * (k + 1) + 2, real.shape[1])
        assert np.array_equal(g.cpu().numpy(), ref.grid(real, fake, cross[1], k))


def test_chunked_queries_equal_one_call(monkeypatch):
    from relativisticgan_amd.neighbours import NearestNeighbours
    images, real, fake, s, k, nn, (want, cross) = _scenario("independent")
    from relativisticgan_amd.config import make_param
    monkeypatch.setattr(NearestNeighbours, "CHUNK", 24)  # 64 = 24 + 24 + 16: leave-one-out offsets 0, 24, 48
    small = NearestNeighbours(images, make_param(image_size=32, n_colors=3), n_images=64, side=s, k=k, seed=5)
    assert torch.equal(small.real_knn[0], nn.real_knn[0]) and torch.equal(small.real_knn[1], nn.real_knn[1])
    assert small.report(torch.from_numpy(fake).cuda()) == want


def test_private_stream_and_buffers():
    from relativisticgan_amd import neighbours
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_G
    images, real, fake, s, k, nn, _ = _scenario("independent")
    p = make_param(loss_D=7, image_size=32, batch_size=8, z_size=16, G_h_size=8, D_h_size=8, seed=1)
    torch.manual_seed(1)
    G = DCGAN_G(p).cuda()
    before = [b.clone() for b in G.buffers()]
    rng = torch.cuda.get_rng_state().clone(), torch.get_rng_state().clone()
    result, grid = nn.evaluate(G, p.z_size, with_grid=True)
    assert all(torch.equal(a, b) for a, b in zip(before, G.buffers())) and len(before) > 0
    assert torch.equal(rng[0], torch.cuda.get_rng_state()) and torch.equal(rng[1], torch.get_rng_state())
    assert list(result) == list(neighbours.KEYS) and all(np.isfinite(result[key]) for key in ("fake_nn", "real_nn"))
    assert tuple(grid.shape) == (34 * 8 + 2, 34 * 4 + 2, 3) and int(nn.counter.item()) > 0
    assert nn.seed == neighbours.private_seed(5)


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


def _png_size(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    return int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")  # width, height


def test_evaluate_cli(capsys):
    from relativisticgan_amd.evaluate import main
    root = tempfile.mkdtemp()
    path = _checkpoint(root)
    capsys.readouterr()
    base = ["--load", path, *SMALL, "--rgan_swd_images", "64", "--seed", "3", "--output_folder", os.path.join(root, "o")]
    main(base)
    plain = capsys.readouterr().out
    assert plain.startswith("SWD x1e3") and len(plain.splitlines()) == 1 and not os.path.exists(os.path.join(root, "o"))
    main([*base, "--rgan_nn", "True", "--rgan_nn_images", "64", "--rgan_nn_side", "16", "--rgan_nn_k", "2"])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0] + "\n" == plain  # the SWD line is what it is without the flag
    m = re.fullmatch(LINE, lines[1])
    assert m and (m.group(1), m.group(2)) == ("16", "2"), lines[1]
    assert float(m.group(3)) > 0 and float(m.group(4)) > 0 and 0 <= float(m.group(6)) <= 1 and 0 <= float(m.group(7)) <= 1
    assert _png_size(os.path.join(root, "o", "nn.png")) == (34 * 3 + 2, 34 * 8 + 2)


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


@pytest.mark.parametrize("extra", [[], ["--rgan_ema_G", "0.9"]], ids=["G", "ema"])
def test_training_is_untouched_by_the_check(extra):
    """With and without --rgan_nn_every 2 over 4 iterations: the same errD, errG and Trainer.state()
    (every parameter and buffer of G and D, the optimizers, the averaged generator), the same RNG
    states; two NN lines and two grids of the stated size."""
    from relativisticgan_amd.train import main
    root = tempfile.mkdtemp()
    states, errs, rngs, logs = [], [], [], []
    for name, more in (("plain", []), ("nn", ["--rgan_nn_every", "2", "--rgan_nn_images", "64", "--rgan_nn_side", "16"])):
        out = os.path.join(root, name)
        t = main(["--loss_D", "7", *SMALL, "--seed", "1", "--n_iter", "4", "--print_every", "2", "--gen_every", "100",
                  "--gen_extra_images", "0", "--output_folder", out, "--extra_folder", os.path.join(root, name + "_x"),
                  *extra, *more])
        states.append(t.state(4, 0))
        errs.append((t.errD.clone(), t.errG.clone()))
        rngs.append((torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(),
                     None if t.dev_rng is None else int(t.dev_rng.counter.item())))
        logs.append(open(os.path.join(out, "RaLSGAN_seed1-0", "logs", "log.txt")).read())
        images = os.path.join(out, "RaLSGAN_seed1-0", "images")
        grids = sorted(f for f in os.listdir(images) if f.startswith("nn_"))
        assert grids == (["nn_iter00001.png", "nn_iter00003.png"] if more else [])
        for g in grids:
            assert _png_size(os.path.join(images, g)) == (34 * 4 + 2, 34 * 8 + 2)
    _same(states[0], states[1], "state")
    _same(errs[0], errs[1], "err")
    assert any("running_mean" in key for key in states[0]["G_state"]) and ("G_ema" in states[0]) == bool(extra)
    for a, b in zip(rngs[0], rngs[1]):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    loss = [re.findall(r"^\[\d+\] Diff: \S+ loss_D: \S+ loss_G: \S+", log, re.M) for log in logs]
    assert loss[0] == loss[1] and len(loss[0]) == 2
    lines = re.findall(r"^\[(\d+)\] " + LINE + "$", logs[1], re.M)
    assert [ln[0] for ln in lines] == ["1", "3"] and logs[1].count("] NN s16 k3") == 2 and "] NN s" not in logs[0]
    assert all(float(ln[3]) > 0 and float(ln[4]) > 0 for ln in lines)
