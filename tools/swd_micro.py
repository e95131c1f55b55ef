"""Sliced Wasserstein metric micro-benchmark (diagnostic, timing only; GPU).

Per kernel at the defaults (N = 8192 images, P = 128 patches, D = 128 directions, C = 3) for
image sides 64 and 256: the pyramid and descriptor kernels on one chunk of 512 images (what
SlicedWasserstein runs at a time), normalise / project / sort / L1 on the whole level (M = N P
rows).  Each figure is the median of --reps device-event timings after a warm-up call.  The sort is
also given as keys/s and GB/s of algorithmic traffic (4 passes x 12 B per key), next to a plain
device copy of the same tensor and to torch.sort on it (a yardstick of this tool only: the package
itself never calls torch.sort).

--distance: the whole metric on bench.py's C1 generator (64^2, h = 128, untrained): seconds to
generate the N images and seconds for SlicedWasserstein.distance, each ending in a synchronise.
usage: python tools/swd_micro.py [--reps R] [--sides 64,256] [--images N] [--distance]"""
import argparse
import os
import sys
import time

import torch


def timed(fn, reps):
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
    print(f"{label:58s}: {ms[0]:9.3f} ms  ({ms[1]:.3f} .. {ms[2]:.3f}){extra}", flush=True)


def kernels(S, N, reps, P=128, D=128, C=3, chunk=512):
    from relativisticgan_amd import kernels as K
    gen = torch.Generator(device="cuda").manual_seed(S)
    chunk = min(chunk, N)
    M, Kd = N * P, 49 * C
    print(f"-- side {S}: N = {N}, chunk = {chunk}, M = {M}, K = {Kd}, D = {D}", flush=True)
    u8 = torch.randint(0, 256, (chunk, C, S, S), dtype=torch.uint8, device="cuda", generator=gen)
    row(f"swd_load_u8 [{chunk}][{C}][{S}][{S}]", timed(lambda: K.swd_load_u8(u8), reps))
    g0 = K.swd_load_u8(u8)
    row(f"swd_pyr_down {S} -> {S // 2}", timed(lambda: K.swd_pyr_down(g0), reps))
    g1 = K.swd_pyr_down(g0)
    out = torch.empty_like(g0)
    row(f"swd_laplace side {S}", timed(lambda: K.swd_laplace(g0, g1, out=out), reps))
    pos = K.swd_positions(torch.rand((chunk, P, 2), device="cuda", generator=gen), S)
    desc = torch.empty((M, Kd), device="cuda")
    part = torch.zeros((N, C, 2), dtype=torch.float64, device="cuda")
    row(f"swd_descriptors {chunk} images x {P} patches", timed(
        lambda: K.swd_descriptors(out, pos, desc[:chunk * P], part[:chunk]), reps))
    desc.normal_(generator=gen)
    part[:, :, 0], part[:, :, 1] = 0.0, float(P * 49)
    ms = timed(lambda: K.swd_normalize(desc, part), reps)
    row(f"swd_normalize [{M}][{Kd}]", ms, f"  {2 * desc.numel() * 4 / ms[0] / 1e6:8.1f} GB/s")
    dirs = K.swd_unit_columns(torch.randn((Kd, D), device="cuda", generator=gen))
    proj = torch.empty((D, M), device="cuda")
    ms = timed(lambda: K.swd_project(desc, dirs, out=proj), reps)
    row(f"swd_project [{M}][{Kd}] x [{Kd}][{D}]", ms, f"  {2.0 * M * Kd * D / ms[0] / 1e9:8.2f} TFLOP/s")
    keys = proj.clone()
    sorted_, tmp = torch.empty_like(keys), torch.empty_like(keys)
    ms = timed(lambda: K.sort_segments(keys, out=sorted_, tmp=tmp), reps)
    n = keys.numel()
    row(f"sort_segments [{D}][{M}]", ms, f"  {n / ms[0] / 1e6:8.2f} Gkeys/s {48.0 * n / ms[0] / 1e6:8.1f} GB/s")
    cp = timed(lambda: tmp.copy_(keys), reps)
    row(f"device copy of [{D}][{M}] floats", cp, f"  {8.0 * n / cp[0] / 1e6:8.1f} GB/s")
    ts = timed(lambda: torch.sort(keys, dim=1), reps)
    row(f"torch.sort [{D}][{M}] (yardstick)", ts, f"  ours / torch.sort = {ms[0] / ts[0]:.2f}")
    assert torch.equal(sorted_, torch.sort(keys, dim=1).values)
    ms = timed(lambda: K.swd_l1(sorted_, keys), reps)
    row(f"swd_l1 {n} floats", ms, f"  {8.0 * n / ms[0] / 1e6:8.1f} GB/s")


def distance(N):
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.nets import DCGAN_G, weights_init
    from relativisticgan_amd.swd import SlicedWasserstein
    from relativisticgan_amd.train import synthetic_images
    p = make_param(loss_D=7, image_size=64, batch_size=32, G_h_size=128, D_h_size=128, seed=1)
    torch.manual_seed(1)
    G = DCGAN_G(p)
    G.apply(weights_init)
    G.to("cuda")
    t0 = time.perf_counter()
    sw = SlicedWasserstein(synthetic_images(N, 64), p, n_images=N, seed=1)
    torch.cuda.synchronize()
    print(f"-- distance(), C1 generator (64^2, h = 128), N = {sw.N}, P = {sw.P}, R = {sw.R}, D = {sw.D}")
    print(f"build (draws, the real set's descriptors)      : {time.perf_counter() - t0:8.3f} s", flush=True)
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fake = sw.generate(G, p.z_size)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = sw.distance(fake)
        t2 = time.perf_counter()
        print(f"call {k}: generate {t1 - t0:8.3f} s, metric {t2 - t1:8.3f} s   "
              + "  ".join(f"{a}: {b:.3f}" for a, b in res.items()), flush=True)
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sides", default="64,256")
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--distance", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("swd_micro: timings need the GPU")
    if not args.no_kernels:
        for s in args.sides.split(","):
            kernels(int(s), args.images, args.reps)
    if args.distance:
        distance(args.images)


if __name__ == "__main__":
    main()
