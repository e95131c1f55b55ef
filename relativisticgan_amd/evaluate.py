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

With ``--rgan_nn True`` [--rgan_nn_images N] [--rgan_nn_side s] [--rgan_nn_k k] a second line follows::

    NN s64 k3  fake->real: a  real->real: b  ratio: c  precision: d  recall: e

(relativisticgan_amd/neighbours.py: the median RMS pixel difference of a generated image to its
nearest training image, the same among the training images, their ratio, and k-NN precision and
recall in pixel space), and ``nn.png`` is written into ``--output_folder``: 8 generated images,
each next to its k nearest training images.
"""
import os
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
    metric_images = load_images(p)
    metric = SlicedWasserstein(metric_images, p, n_images=p.rgan_swd_images, seed=p.seed)
    result = metric.evaluate(G, p.z_size, keep_buffers=False)
    print(format_line(result), flush=True)
    if p.rgan_nn:
        from .config import validate_nn
        from .images import write_png
        from .neighbours import NearestNeighbours, format_line as nn_format_line
        try:
            validate_nn(0, True, p.rgan_nn_images, p.rgan_nn_side, p.rgan_nn_k, p.image_size)
        except ValueError as e:
            raise SystemExit(str(e))
        check = NearestNeighbours(metric_images, p, n_images=p.rgan_nn_images, side=p.rgan_nn_side, k=p.rgan_nn_k,
                                  seed=p.seed)
        nn_result, grid = check.evaluate(G, p.z_size, keep_buffers=False, with_grid=True)
        print(nn_format_line(nn_result, check.s, check.k), flush=True)
        os.makedirs(p.output_folder, exist_ok=True)
        write_png(os.path.join(p.output_folder, "nn.png"), grid.cpu())
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
