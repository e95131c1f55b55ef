"""Sliced Wasserstein distance of a checkpoint's generator against a set of real images.

``python -m relativisticgan_amd.evaluate --load state_NN.pth [reference G flags]
(--input_folder DIR | --rgan_synthetic N) [--rgan_swd_images N] [--rgan_ema_G b]`` rebuilds G as
``relativisticgan_amd.generate`` does (``G_ema`` with ``--rgan_ema_G``), generates N images, 100
per forward in train mode like the extra images (GLI:752-768), quantised as the PNG writer
quantises them, and prints one line::

    SWD x1e3  64: a  32: b  16: c  avg: d

one value per Laplacian-pyramid level (named by its side) and their average
(relativisticgan_amd/swd.py; the reference's own quality number is FID, code/fid.py, which needs
TensorFlow and a downloaded network).  N = min(--rgan_swd_images, the number of real images).
"""
import sys

import torch

from .config import parse
from .nets import DCGAN_G
from .swd import SlicedWasserstein, format_line
from .train import load_images


def main(argv=None):
    p = parse(argv)
    if not p.load:
        raise SystemExit("--load <checkpoint> is required")
    if not torch.cuda.is_available():
        raise SystemExit("the metric runs on the MI355X only")
    if p.seed is not None:
        torch.manual_seed(p.seed)
    G = DCGAN_G(p)
    ck = torch.load(p.load, map_location="cpu", weights_only=True)
    if p.rgan_ema_G > 0:
        # the averaged generator of a --rgan_ema_G run (the flag's value itself is not used here)
        if "G_ema" not in ck:
            raise SystemExit(f"--rgan_ema_G: {p.load} holds no averaged generator (no 'G_ema' key): it was "
                             "written by a run without --rgan_ema_G; drop the flag to sample from G_state")
        G.load_state_dict(ck["G_ema"]["G_ema_state"])
    else:
        G.load_state_dict(ck["G_state"])
    G.to("cuda")
    metric = SlicedWasserstein(load_images(p), p, n_images=p.rgan_swd_images, seed=p.seed)
    result = metric.evaluate(G, p.z_size, keep_buffers=False)
    print(format_line(result), flush=True)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
