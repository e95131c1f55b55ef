"""--rgan_aug_p / --rgan_ada_target micro-benchmark (diagnostic, timing only; GPU).

Kernels: rgan_diffaug and rgan_diffaug_p (p = 1, 1/2, 0) at 32 x 3 x 256^2 and 32 x 3 x 64^2,
policy 7, forward and adjoint, next to a plain copy of the same tensor, and rgan_ada_update at
n = 32 and 64.  Each figure is the time of a HIP graph of CALLS back-to-back calls over CALLS
(the calls take microseconds: eager calls would time the host's enqueue), median of --reps
replays; the whole table is measured --rounds times, in alternating order, and every entry is
given as the median over the rounds with their min..max (the spread).  --parent-lib FILE times
rgan_diffaug of another build of the library (the parent commit's) in the same rounds.

--step N: ms per eager iteration of the 64^2 trainer (bench.py's C1: RaLSGAN, B = 32) with the
flags off, with --rgan_diffaug alone, and with adaptation on, in alternating chunks of 32
iterations, N chunks each.  --settings picks a subset; --root DIR imports the package from another
checkout (the parent commit's flags-off figure, from the same session).
usage: python tools/ada_micro.py [--reps R] [--rounds N] [--parent-lib FILE] [--step N]
                                 [--settings off,diffaug,ada] [--root DIR] [--json FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

CALLS = 20
SHAPES = ((32, 3, 256, 256), (32, 3, 64, 64))
POLICY = "color,translation,cutout"
SETTINGS = {"off": {}, "diffaug": dict(rgan_diffaug=POLICY),
            "ada": dict(rgan_diffaug=POLICY, rgan_ada_target=0.6)}
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


def _parent(path):
    lib = ctypes.CDLL(path)
    v = ctypes.c_void_p
    lib.rgan_diffaug.restype = ctypes.c_int
    lib.rgan_diffaug.argtypes = [v, v] + [ctypes.c_int] * 6 + [v, v, v]
    return lib


def kernels(reps, rounds, parent_lib):
    from relativisticgan_amd import _lib as L
    lib, P = L.lib(), L.ptr
    parent = _parent(parent_lib) if parent_lib else None
    gen = torch.Generator(device="cuda").manual_seed(0)
    cases = []  # (label, fn)
    for shp in SHAPES:
        B, C, H, W = shp
        x = torch.rand(shp, device="cuda", generator=gen) * 2 - 1
        u = torch.rand(B, 8, device="cuda", generator=gen)
        gate = torch.rand(B, 4, device="cuda", generator=gen)
        out = torch.empty_like(x)
        ws = torch.empty(int(lib.rgan_diffaug_workspace(B, C, H, W)), device="cuda")
        ps = {v: torch.tensor([v], dtype=torch.float64, device="cuda") for v in (1.0, 0.5, 0.0)}

        def plain(which, adjoint, x=x, u=u, ws=ws, out=out, shp=shp):
            def fn():
                L.check(which.rgan_diffaug(P(x), P(u), *shp, 7, adjoint, P(ws), P(out), L.stream()), "rgan_diffaug")
            return fn

        def gated(p, adjoint, x=x, u=u, gate=gate, ws=ws, out=out, shp=shp):
            def fn():
                L.check(lib.rgan_diffaug_p(P(x), P(u), P(gate), P(p), *shp, 7, adjoint, P(ws), P(out), L.stream()),
                        "rgan_diffaug_p")
            return fn

        tag = "x".join(map(str, shp))
        for adjoint in (0, 1):
            side = "adjoint" if adjoint else "forward"
            cases.append((f"{tag} {side} rgan_diffaug", plain(lib, adjoint)))
            if parent is not None:
                cases.append((f"{tag} {side} rgan_diffaug (parent build)", plain(parent, adjoint)))
            for v in (1.0, 0.5, 0.0):
                cases.append((f"{tag} {side} rgan_diffaug_p p={v:g}", gated(ps[v], adjoint)))
        cases.append((f"{tag} copy_", lambda x=x, out=out: out.copy_(x)))
    hyper = torch.tensor([0.6, 4.0, 500000.0, 0.0], dtype=torch.float64, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    for n in (32, 64):
        a, b = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)

        def upd(a=a, b=b, n=n):
            L.check(lib.rgan_ada_update(P(a), P(b), n, P(hyper), P(state), 1, L.stream()), "rgan_ada_update")
        cases.append((f"rgan_ada_update n={n} (one launch)", upd))
    us = {label: [] for label, _ in cases}
    for r in range(rounds):
        for label, fn in (cases if r % 2 == 0 else cases[::-1]):
            us[label].append(graph_us(fn, reps))
    rows = []
    for label, _ in cases:
        v = sorted(us[label])
        rows.append({"case": label, "us": us[label], "median": v[len(v) // 2], "min": v[0], "max": v[-1]})
        print(f"{label:52s}: {v[len(v) // 2]:8.2f} us  ({v[0]:.2f} .. {v[-1]:.2f} over {rounds} rounds)", flush=True)
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
        for i in range(CHUNK):
            trainers[name].iteration(1 + i)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for c in range(1, chunks + 1):  # off, diffaug, ada, off, ...: drift hits all alike
        for name, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(CHUNK):
                t.iteration(1 + c * CHUNK + i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / CHUNK * 1e3)
    out = {}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2]
        out[name] = {"ms": v, "median": med, "spread": max(v) - min(v)}
        extra = ""
        if getattr(trainers[name], "ada", None) is not None:
            extra = "; ada_p %.4f r %.4f" % trainers[name].ada.read()
        print(f"eager C1 step, {name:8s}: median {med:.3f} ms, spread {max(v) - min(v):.3f} "
              f"({' '.join('%.3f' % x for x in v)}; chunks of {CHUNK}{extra})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="also time rgan_diffaug of this build of the library")
    ap.add_argument("--step", type=int, default=0, help="also time this many chunks of eager iterations per setting")
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="import relativisticgan_amd from this checkout")
    ap.add_argument("--json", default=None, help="write the figures here too")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        raise SystemExit("ada_micro: timings need the GPU")
    out = {"root": os.path.abspath(args.root)}
    if not args.no_kernels:
        out["kernels"] = kernels(args.reps, args.rounds, args.parent_lib)
    if args.step:
        out["step"] = steps(args.step, [s for s in args.settings.split(",") if s])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
