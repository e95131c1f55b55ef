"""--rgan_r1 / --rgan_r2 micro-benchmark (diagnostic, timing only; GPU).

Kernels: rgan_gp_zc_penalty and rgan_gp_zc_penalty_backward at batch 32 with per = 3*256*256 and
per = 3*64*64, as GB/s on the algorithmic bytes (forward: g read once, 4 B/element; backward: g
read and dg written, 8 B/element), next to the one-centred rgan_gp_penalty / _backward on the same
inputs.  Each figure is the time of a HIP graph of CALLS back-to-back calls over CALLS (the calls
take a few microseconds: eager calls would time the host's enqueue), median of --reps replays.

--step N: ms per eager iteration of the 64^2 trainer (bench.py's C1: RaLSGAN, B = 32) with the
flags off, with --rgan_r1 10, and with --rgan_r1 10 --rgan_reg_every 16, in alternating chunks of
32 iterations (two lazy periods), N chunks each.  --settings picks a subset; --root DIR imports the
package from another checkout (the parent commit's flags-off figure, from the same session).
usage: python tools/r1r2_micro.py [--reps R] [--step N] [--settings off,r1,r1_lazy16] [--root DIR] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import torch

HBM_ACHIEVABLE = 6.29e12  # float4 copy, the measured HBM rate of the MI355X
CALLS = 20
SHAPES = ((32, 3 * 256 * 256), (32, 3 * 64 * 64))
GAMMA = 10.0
SETTINGS = {"off": {}, "r1": dict(rgan_r1=10.0), "r1_lazy16": dict(rgan_r1=10.0, rgan_reg_every=16)}
CHUNK = 32


def graph_us(fn, reps):
    """Median microseconds per call of ``fn`` inside a graph of CALLS calls."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(CALLS):
            fn()
    times = []
    with torch.cuda.stream(side):
        for _ in range(3):
            graph.replay()
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return sorted(times)[len(times) // 2]


def kernels(reps):
    from relativisticgan_amd import _lib as L
    lib = L.lib()
    rows = []
    for batch, per in SHAPES:
        g = torch.randn(batch, per, device="cuda")
        dg = torch.empty_like(g)
        vec, loss, one = torch.empty(batch, device="cuda"), torch.empty((), device="cuda"), torch.ones((), device="cuda")
        ws = L.workspace(lib.rgan_gp_zc_workspace(batch, per), g.device)
        norms = torch.empty(batch, device="cuda")
        P = L.ptr

        def zc_fwd():
            L.check(lib.rgan_gp_zc_penalty(P(g), batch, per, GAMMA, batch, P(vec), P(loss), P(ws), L.stream()), "zc")

        def zc_bwd():
            L.check(lib.rgan_gp_zc_penalty_backward(P(g), batch, per, GAMMA, batch, P(one), P(dg), L.stream()), "zc_b")

        def oc_fwd():
            L.check(lib.rgan_gp_penalty(P(g), batch, per, GAMMA, batch, P(norms), P(loss), L.stream()), "gp")

        def oc_bwd():
            L.check(lib.rgan_gp_penalty_backward(P(g), P(norms), batch, per, GAMMA, batch, P(one), P(dg), L.stream()),
                    "gp_b")

        for name, fn, bytes_per in (("rgan_gp_zc_penalty", zc_fwd, 4), ("rgan_gp_penalty", oc_fwd, 4),
                                    ("rgan_gp_zc_penalty_backward", zc_bwd, 8),
                                    ("rgan_gp_penalty_backward", oc_bwd, 8)):
            us = graph_us(fn, reps)
            gbs = bytes_per * batch * per / us / 1e3
            rows.append({"kernel": name, "batch": batch, "per": per, "us": us, "GB_s": gbs,
                         "MB": bytes_per * batch * per / 1e6})
            print(f"{name:30s} batch {batch} per {per:7d} ({bytes_per * batch * per / 1e6:6.1f} MB): {us:8.2f} us "
                  f"{gbs:7.0f} GB/s = {gbs * 1e9 / HBM_ACHIEVABLE:.2f} of 6.29 TB/s", flush=True)
    return rows


def steps(chunks, names):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    loss_D, size, bpg, h = 7, 64, 32, 128  # bench.py's C1
    images = synthetic_images(1024, size, device="cuda")
    trainers = {}
    for name in names:
        p = make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h, seed=1,
                       print_every=10 ** 9, rgan_rng="device", **SETTINGS[name])
        trainers[name] = Trainer(p, images)
        for i in range(CHUNK):  # a whole lazy period: both kinds of iteration warmed
            trainers[name].iteration(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for c in range(1, chunks + 1):  # off, r1, lazy, off, r1, lazy, ...: drift hits all alike
        for name, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(CHUNK):
                t.iteration(c * CHUNK + i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / CHUNK * 1e3)
    out = {}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2]
        out[name] = {"ms": v, "median": med, "spread": max(v) - min(v)}
        print(f"eager C1 step, {name:10s}: median {med:.3f} ms, spread {max(v) - min(v):.3f} "
              f"({' '.join('%.3f' % x for x in v)}; chunks of {CHUNK})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", type=int, default=0, help="also time this many chunks of eager iterations per setting")
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="import relativisticgan_amd from this checkout")
    ap.add_argument("--json", default=None, help="write the figures here too")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        raise SystemExit("r1r2_micro: timings need the GPU")
    out = {"root": os.path.abspath(args.root)}
    if not args.no_kernels:
        out["kernels"] = kernels(args.reps)
    if args.step:
        out["step"] = steps(args.step, [s for s in args.settings.split(",") if s])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
