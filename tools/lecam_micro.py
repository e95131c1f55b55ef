"""--rgan_lecam micro-benchmark (diagnostic, timing only; GPU).

Kernel: the fused rgan_lecam launch (both sides, gradients written) at n = 32 and 1024, and the
data-parallel pair (partial-sums launch + rgan_lecam_finish) at n = 32.  Each figure is the time
of a HIP graph of CALLS back-to-back calls over CALLS (the calls take microseconds: eager calls
would time the host's enqueue), median of --reps replays; the table is measured --rounds times,
in alternating order, and every entry is the median over the rounds with their min..max.

--step N: ms per eager iteration of bench.py's C1 (RaLSGAN 64^2, B = 32, h = 128) and C3
(256^2) trainers with the flag off and with --rgan_lecam 0.3, in alternating chunks of CHUNK
iterations, N chunks each.  --workloads picks a subset.
usage: python tools/lecam_micro.py [--reps R] [--rounds N] [--step N] [--workloads C1,C3] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import torch

CALLS = 20
WORKLOADS = {"C1": (7, 64, 32, 128, 32), "C3": (7, 256, 32, 128, 8)}  # loss_D, size, B, h, iterations per chunk
SETTINGS = {"off": {}, "lecam": dict(rgan_lecam=0.3)}


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


def kernels(reps, rounds):
    from relativisticgan_amd import _lib as L
    lib, P = L.lib(), L.ptr
    gen = torch.Generator(device="cuda").manual_seed(0)
    hyper = torch.tensor([0.3, 0.99, 1.0, 0.0], dtype=torch.float64, device="cuda")
    state = torch.tensor([0.25, -0.5, 5.0, 0.0], dtype=torch.float64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    cases = []
    for n in (32, 1024):
        yr, yf = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
        dr, df = torch.empty_like(yr), torch.empty_like(yf)

        def fused(yr=yr, yf=yf, dr=dr, df=df, n=n):
            L.check(lib.rgan_lecam(P(yr), P(yf), n, n, P(hyper), P(state), P(dr), P(df), P(out), 0, L.stream()),
                    "rgan_lecam")
        cases.append((f"rgan_lecam n={n} (fused, one launch)", fused))
        if n == 32:
            def pair(yr=yr, yf=yf, dr=dr, df=df, n=n):
                L.check(lib.rgan_lecam(P(yr), P(yf), n, 2 * n, P(hyper), P(state), P(dr), P(df), P(out), 1,
                                       L.stream()), "rgan_lecam")
                L.check(lib.rgan_lecam_finish(P(out), 2 * n, 3, P(hyper), P(state), P(out), L.stream()),
                        "rgan_lecam_finish")
            cases.append((f"rgan_lecam partial + rgan_lecam_finish n={n} (two launches)", pair))
    us = {label: [] for label, _ in cases}
    for r in range(rounds):
        for label, fn in (cases if r % 2 == 0 else cases[::-1]):
            us[label].append(graph_us(fn, reps))
    rows = []
    for label, _ in cases:
        v = sorted(us[label])
        rows.append({"case": label, "us": us[label], "median": v[len(v) // 2], "min": v[0], "max": v[-1]})
        print(f"{label:60s}: {v[len(v) // 2]:8.2f} us  ({v[0]:.2f} .. {v[-1]:.2f} over {rounds} rounds)", flush=True)
    return rows


def steps(chunks, workload):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.train import Trainer, synthetic_images
    loss_D, size, bpg, h, chunk = WORKLOADS[workload]
    images = synthetic_images(256, size, device="cuda")
    trainers = {}
    for name, flags in SETTINGS.items():
        p = make_param(loss_D=loss_D, image_size=size, batch_size=bpg, G_h_size=h, D_h_size=h, seed=1,
                       print_every=10 ** 9, rgan_rng="device", **flags)
        trainers[name] = Trainer(p, images)
        for i in range(chunk):
            trainers[name].iteration(1 + i)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for c in range(1, chunks + 1):  # off, lecam, off, ...: drift hits both alike
        for name, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(chunk):
                t.iteration(1 + c * chunk + i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / chunk * 1e3)
    out = {}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2]
        out[name] = {"ms": v, "median": med, "spread": max(v) - min(v)}
        extra = ""
        if trainers[name].lecam is not None:
            extra = "; lecam %.4f a_real %.4f a_fake %.4f" % ((trainers[name].last["D"]["lecam"].item(),)
                                                             + trainers[name].lecam.read())
        print(f"eager {workload} step, {name:6s}: median {med:.3f} ms, spread {max(v) - min(v):.3f} "
              f"({' '.join('%.3f' % x for x in v)}; chunks of {chunk}{extra})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=0, help="also time this many chunks of eager iterations per setting")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--json", default=None, help="write the figures here too")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("lecam_micro: timings need the GPU")
    out = {}
    if not args.no_kernels:
        out["kernels"] = kernels(args.reps, args.rounds)
    if args.step:
        out["step"] = {w: steps(args.step, w) for w in args.workloads.split(",") if w}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
