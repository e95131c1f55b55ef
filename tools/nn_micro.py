"""Nearest-training-image check micro-benchmark (diagnostic, timing only; GPU).

rgan_nn_topk and rgan_nn_covered at the check's own size (Q = R = 8192 rows of 12288 bytes, k = 3;
random int8 rows): the median of --reps device-event timings after 3 warm-up calls, as int8
operations per second (2 Q R D / t) and as a fraction of the int8 matrix peak (twice the bf16
figure, 2 x 2.5e15), and rgan_nn_pack_u8 on 8192 images of 3 x 64 x 64.

--report: on bench.py's C1 generator (64^2, h = 128, untrained) and 8192 synthetic images, in one
process: seconds to build NearestNeighbours (pack, the reals' own neighbours), then per call the
seconds of generate and of report, next to SlicedWasserstein's generate and distance at its defaults,
each ending in a synchronise or a read-back.
usage: python tools/nn_micro.py [--reps R] [--rows N] [--report]"""
import argparse
import os
import sys
import time

import torch

INT8_PEAK = 2 * 2.5e15


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def row(label, ms, extra=""):
    print(f"{label:52s}: {ms[0]:9.3f} ms  ({ms[1]:.3f} .. {ms[2]:.3f}){extra}", flush=True)


def kernels(N, reps, D=12288, k=3):
    from relativisticgan_amd import kernels as K
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randint(-128, 128, (N, D), dtype=torch.int8, device="cuda", generator=gen)
    b = torch.randint(-128, 128, (N, D), dtype=torch.int8, device="cuda", generator=gen)
    na, nb = (x.to(torch.int32).square().sum(dim=1, dtype=torch.int32) for x in (a, b))
    out = (torch.empty((N, k), dtype=torch.int32, device="cuda"), torch.empty((N, k), dtype=torch.int32, device="cuda"))
    ops = 2.0 * N * N * D
    print(f"-- Q = R = {N}, row_bytes = {D}, k = {k}, parts = {K.L.lib().rgan_nn_topk_splits(N, N)}", flush=True)
    ms = timed(lambda: K.nn_topk(a, na, b, nb, k, out=out), reps)
    row("nn_topk", ms, f"  {ops / ms[0] / 1e9:8.1f} Tops/s  {ops / ms[0] * 1e3 / INT8_PEAK:6.3f} of the int8 peak")
    for ns in (1, 4, 16):
        ms = timed(lambda: K.nn_topk(a, na, b, nb, k, nsplit=ns, out=out), reps)
        row(f"nn_topk, {ns} part(s)", ms, f"  {ops / ms[0] / 1e9:8.1f} Tops/s")
    radius = torch.zeros(N, dtype=torch.int32, device="cuda")
    flag = torch.empty(N, dtype=torch.int32, device="cuda")
    ms = timed(lambda: K.nn_covered(a, na, b, nb, radius, out=flag), reps)
    row("nn_covered", ms, f"  {ops / ms[0] / 1e9:8.1f} Tops/s")
    u8 = torch.randint(0, 256, (N, 3, 64, 64), dtype=torch.uint8, device="cuda", generator=gen)
    ms = timed(lambda: K.nn_pack_u8(u8, 64), reps)
    row(f"nn_pack_u8 [{N}][3][64][64] -> side 64", ms, f"  {2.0 * u8.numel() / ms[0] / 1e6:8.1f} GB/s")
    ms = timed(lambda: K.nn_pack_u8(u8, 16), reps)
    row(f"nn_pack_u8 [{N}][3][64][64] -> side 16", ms)


def report(N):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.neighbours import NearestNeighbours, format_line
    from relativisticgan_amd.nets import DCGAN_G, weights_init
    from relativisticgan_amd.swd import SlicedWasserstein
    from relativisticgan_amd.train import synthetic_images
    p = make_param(loss_D=7, image_size=64, batch_size=32, G_h_size=128, D_h_size=128, seed=1)
    torch.manual_seed(1)
    G = DCGAN_G(p)
    G.apply(weights_init)
    G.to("cuda")
    images = synthetic_images(N, 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nn = NearestNeighbours(images, p, n_images=N, seed=1)
    torch.cuda.synchronize()
    print(f"-- report(), C1 generator (64^2, h = 128), N = {nn.N}, side {nn.s}, k = {nn.k}")
    print(f"NN build (pack, the reals' neighbours)         : {time.perf_counter() - t0:8.3f} s", flush=True)
    t0 = time.perf_counter()
    sw = SlicedWasserstein(images, p, n_images=N, seed=1)
    torch.cuda.synchronize()
    print(f"SWD build (draws, the real set's descriptors)  : {time.perf_counter() - t0:8.3f} s", flush=True)
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fake = nn.generate(G, p.z_size)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = nn.report(fake)
        t2 = time.perf_counter()
        g = nn.grid(fake, nn.query(fake[:8])[1]).cpu()
        t3 = time.perf_counter()
        print(f"call {k}: NN  generate {t1 - t0:8.3f} s, report {t2 - t1:8.3f} s, grid {t3 - t2:8.3f} s   "
              + format_line(res, nn.s, nn.k), flush=True)
        t0 = time.perf_counter()
        fake = sw.generate(G, p.z_size)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = sw.distance(fake)
        t2 = time.perf_counter()
        print(f"call {k}: SWD generate {t1 - t0:8.3f} s, metric {t2 - t1:8.3f} s   avg: {res['avg']:.3f}", flush=True)
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("nn_micro: timings need the GPU")
    if not args.no_kernels:
        kernels(args.rows, args.reps)
    if args.report:
        report(args.rows)


if __name__ == "__main__":
    main()
