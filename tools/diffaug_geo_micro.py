"""Micro-benchmark of the geometric groups of --rgan_diffaug (diagnostic; GPU): time of the
forward and the adjoint of rgan_diffaug_geo at the batched D input of the 256^2 and 64^2
workloads for policies 24 (xflip + rot90: an integer move), 32 (warp) and 63 (all six groups),
next to policies 6 and 7 of rgan_diffaug from the same run, as GB/s on the algorithmic bytes --
12 B/element with the colour bit (x read by the sample sum and by the pass, y written), 8
B/element without it (the four taps of a warped value are neighbours, read from cache).  With
--step N: N eager iterations each of the 256^2 trainer (bench.py's default workload) with
color,translation,cutout and with all six groups, in alternating chunks, and the per-step
difference.
usage: python tools/diffaug_geo_micro.py [--reps R] [--step N] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from relativisticgan_amd import kernels as K  # noqa: E402

SHAPES = [(64, 3, 256, 256), (64, 3, 64, 64)]
POLICIES = ((6, 8), (7, 12), (24, 8), (32, 8), (63, 12))  # (policy, algorithmic bytes per element)
HBM_ACHIEVABLE = 6.29e12  # float4 copy, the measured HBM rate of the MI355X
OLD, ALL_SIX = "color,translation,cutout", "color,translation,cutout,xflip,rot90,warp"


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
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    for shp in SHAPES:
        x = torch.rand(shp, device="cuda", generator=gen) * 2 - 1
        u = torch.rand(shp[0], 8, device="cuda", generator=gen)
        v = torch.rand(shp[0], 8, device="cuda", generator=gen)
        out = torch.empty_like(x)
        n = x.numel()
        for policy, per in POLICIES:
            for adjoint in (False, True):
                geo = v if policy >= 8 else None
                us = timeit(lambda: K.diffaug(x, u, policy, adjoint=adjoint, out=out, geo=geo), reps)
                gbs = per * n / us / 1e3
                rows.append({"shape": list(shp), "policy": policy, "adjoint": adjoint, "bytes_per_element": per,
                             "us": us, "GB_s": gbs, "frac_of_6.29TBs": gbs * 1e9 / HBM_ACHIEVABLE})
                print(f"{str(shp):20s} policy {policy:2d} {'adjoint' if adjoint else 'forward'}: {us:8.1f} us "
                      f"{gbs:7.0f} GB/s ({per:2d} B/elem) = {gbs * 1e9 / HBM_ACHIEVABLE:.2f} of 6.29 TB/s", flush=True)
    return rows


def steps(iters):
    from bench import DEFAULT_WORKLOAD, WORKLOADS
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    loss_D, size, bpg, h = WORKLOADS[DEFAULT_WORKLOAD]
    images = synthetic_images(1024, size, device="cuda")
    trainers = {}
    for policy in (OLD, ALL_SIX):
        p = make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h, seed=1,
                       print_every=10 ** 9, rgan_rng="device", rgan_diffaug=policy)
        trainers[policy] = Trainer(p, images)
        for i in range(3):
            trainers[policy].iteration(i + 1)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    chunk = 5
    for c in range(max(1, iters // chunk)):  # three, six, three, six, ...: drift hits both alike
        for policy, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(chunk):
                t.iteration(10 + c * chunk + i)
            torch.cuda.synchronize()
            ms[policy].append((time.perf_counter() - t0) / chunk * 1e3)
    old, six = (sorted(v)[len(v) // 2] for v in (ms[OLD], ms[ALL_SIX]))
    print(f"eager {DEFAULT_WORKLOAD} step: three groups {old:.2f} ms, six groups {six:.2f} ms, difference "
          f"{six - old:+.2f} ms (medians of {len(ms[OLD])} chunks of {chunk})", flush=True)
    print("  three groups: " + "  ".join(f"{t:.2f}" for t in ms[OLD]), flush=True)
    print("  six groups:   " + "  ".join(f"{t:.2f}" for t in ms[ALL_SIX]), flush=True)
    return {"workload": DEFAULT_WORKLOAD, "chunk": chunk, "ms_three": ms[OLD], "ms_six": ms[ALL_SIX],
            "median_three": old, "median_six": six, "difference_ms": six - old}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step", type=int, default=0, help="also time this many eager trainer iterations per setting")
    ap.add_argument("--json", default=None, help="write the figures here too")
    args = ap.parse_args()
    out = {"kernels": kernels(args.reps)}
    if args.step:
        out["step"] = steps(args.step)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
