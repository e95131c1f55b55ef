"""--rgan_ema_G micro-benchmark (diagnostic; GPU): time of rgan_ema_update over the generator's
parameter set of the 256^2 (C3) and 64^2 (C1) workloads, as GB/s on the algorithmic bytes
(12 B/element: p and avg read, avg written), next to the Adam line of bench.py's hbm_kernels
(28 B/element, the closest multi-tensor streaming kernel) measured in the same process.  With
--step N: N eager iterations each of the 256^2 trainer (bench.py's default workload) with the
flag off and on (0.999), in alternating chunks of 5, and the per-step difference.
usage: python tools/ema_micro.py [--reps R] [--step N] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from relativisticgan_amd import kernels as K  # noqa: E402

HBM_ACHIEVABLE = 6.29e12  # float4 copy, the measured HBM rate of the MI355X
BETA = 0.999


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1000.0  # us


def kernels(reps):
    import bench
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_G
    rows = []
    hyper = torch.tensor([BETA, 1.0], dtype=torch.float64, device="cuda")
    for name in ("C3", "C1"):
        loss_D, size, bpg, h = bench.WORKLOADS[name]
        G = DCGAN_G(make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h)).to("cuda")
        ps = [p.detach() for p in G.parameters()]
        avgs = [torch.randn_like(p) for p in ps]
        count = torch.zeros(1, device="cuda")
        n = sum(p.numel() for p in ps)
        us = timeit(lambda: K.ema_update(avgs, ps, hyper, count), reps)
        gbs = 12 * n / us / 1e3
        launches = 1 + -(-len(ps) // 48)
        rows.append({"workload": name, "tensors": len(ps), "elements": n, "launches": launches, "us": us,
                     "GB_s": gbs, "frac_of_6.29TBs": gbs * 1e9 / HBM_ACHIEVABLE})
        print(f"ema_update {name}: {len(ps)} tensors, {n} elements, {launches} launches: {us:8.1f} us "
              f"{gbs:7.0f} GB/s (12 B/elem) = {gbs * 1e9 / HBM_ACHIEVABLE:.2f} of 6.29 TB/s", flush=True)
        del G, ps, avgs
    adam = [r for r in bench.hbm_kernels("C3", K)["kernels"] if r["kernel"].startswith("adam")]
    for r in adam:
        print(f"{r['kernel']} {r['shape']}: {r['us']:8.1f} us {r['GB_s']:7.0f} GB/s (28 B/elem)", flush=True)
    return rows, adam


def steps(iters):
    from bench import DEFAULT_WORKLOAD, WORKLOADS
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    loss_D, size, bpg, h = WORKLOADS[DEFAULT_WORKLOAD]
    images = synthetic_images(1024, size, device="cuda")
    trainers = {}
    for beta in (0.0, BETA):
        p = make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h, seed=1,
                       print_every=10 ** 9, rgan_rng="device", rgan_ema_G=beta)
        trainers[beta] = Trainer(p, images)
        for i in range(3):
            trainers[beta].iteration(i + 1)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    chunk = 5
    for c in range(max(1, iters // chunk)):  # off, on, off, on, ...: drift hits both alike
        for beta, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(chunk):
                t.iteration(10 + c * chunk + i)
            torch.cuda.synchronize()
            ms[beta].append((time.perf_counter() - t0) / chunk * 1e3)
    off, on = (sorted(v)[len(v) // 2] for v in (ms[0.0], ms[BETA]))
    print(f"eager {DEFAULT_WORKLOAD} step: off {off:.2f} ms, on {on:.2f} ms, difference {on - off:+.2f} ms "
          f"(medians of {len(ms[0.0])} chunks of {chunk}); off {['%.2f' % v for v in ms[0.0]]} "
          f"on {['%.2f' % v for v in ms[BETA]]}", flush=True)
    return {"workload": DEFAULT_WORKLOAD, "chunk": chunk, "ms_off": ms[0.0], "ms_on": ms[BETA],
            "median_off": off, "median_on": on, "difference_ms": on - off}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step", type=int, default=0, help="also time this many eager trainer iterations per setting")
    ap.add_argument("--json", default=None, help="write the figures here too")
    args = ap.parse_args()
    rows, adam = kernels(args.reps)
    out = {"kernels": rows, "adam": adam}
    if args.step:
        out["step"] = steps(args.step)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
