"""Build the gfx950 HIP library in-tree: relativisticgan_amd/librgan.so.

One hipcc invocation per translation unit (compiled in parallel), then one link.  The
.so is plain C-ABI (include/rgan.h) with no torch dependency; Python loads it with
ctypes (relativisticgan_amd/_lib.py).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "librgan.so")
BUILD = os.path.join(HERE, "build")
ARCH = os.environ.get("RGAN_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"),
         "-Wno-unused-result", "-munsafe-fp-atomics"]
# by measured compile time, slowest first (one at a time: gemm_wgrad 28 s, gemm_conv and conv_narrow 23 s,
# gemm_convt2 21 s, bn_act 12 s, then augment_geo, first_layer, conv_pack, conv_reduce and heads_optim at
# 3-5 s and the rest, the host-only conv_gemm / conv_plan / conv_prof among them, under 2 s each; the pool
# below starts them in this order)
SOURCES = ["gemm_wgrad.hip", "gemm_conv.hip", "conv_narrow.hip", "gemm_convt2.hip", "bn_act.hip", "augment_geo.hip",
           "first_layer.hip", "conv_pack.hip", "conv_reduce.hip", "heads_optim.hip", "conv_gemm.hip", "conv_plan.hip",
           "conv_prof.hip", "images.hip", "augment.hip", "ema.hip", "sampling.hip", "patches.hip", "upsample.hip",
           "gp_zc.hip", "ada.hip", "lecam.hip", "swd.hip", "sort.hip", "nn.hip"]


def _stale(obj, src):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps.append(os.path.join(ROOT, "include", "rgan.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build(verbose=False, force=False):
    os.makedirs(BUILD, exist_ok=True)
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(BUILD, s.replace(".hip", ".o"))
        if force or _stale(obj, src):
            jobs.append([HIPCC, *FLAGS, "-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        return cmd, r

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        for cmd, r in ex.map(run, jobs):
            if verbose or r.returncode:
                sys.stderr.write(r.stdout + r.stderr)
            if r.returncode:
                raise RuntimeError(f"hipcc failed: {' '.join(cmd)}")
    objs = [os.path.join(BUILD, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or not os.path.exists(OUT) or any(os.path.getmtime(o) > os.path.getmtime(OUT) for o in objs):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError("link failed")
    return OUT


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv, force="-f" in sys.argv))
