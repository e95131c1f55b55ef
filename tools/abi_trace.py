#!/usr/bin/env python3
"""C-ABI call trace of one eager training iteration: every rgan_* call the host makes, in
order, with its scalar arguments, the RganConv descriptor decoded, and the Python caller
chain (kernels.* -> autograd / gp / nets).  Diagnostic only (GPU box).  The recorder itself is
relativisticgan_amd/abi_record.py.

usage: python tools/abi_trace.py [WORKLOAD] [ITERS_WARMUP]   (workloads of bench.py)
"""
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import ARCH, WORKLOADS  # noqa: E402
from relativisticgan_amd.abi_record import Recorder  # noqa: E402


def _callers():
    st = [f.name for f in traceback.extract_stack(limit=10)[:-2]
          if f.filename.startswith(os.path.join(ROOT, "relativisticgan_amd"))]
    return f"  <- {'/'.join(st[-4:])}"


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C4"
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    loss_D, size, bpg, h = WORKLOADS[name]
    p = make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h, seed=1,
                   print_every=10 ** 9, spectral=name == "C5", rgan_rng="device", arch=ARCH.get(name, 0))
    t = Trainer(p, synthetic_images(1024, size, device="cuda"))
    for i in range(warm):
        t.iteration(i + 1)
    torch.cuda.synchronize()
    with Recorder(_callers) as log:
        t.iteration(warm + 1)
        torch.cuda.synchronize()
    for r in log.rows:
        print(r)
    print(f"# {len(log.rows)} rgan_* calls in one {name} iteration")


if __name__ == "__main__":
    main()
