"""The conv planner's decisions, pinned on the CPU.

The library loads without a GPU, and its size queries run the planner (csrc/conv_plan.hip) on
placeholder pointers.  For a few hundred layer descriptors this test compares what those queries
answer with tests/golden/conv_plan.json: workspace bytes, packed-weight floats, the BatchNorm
segment counts and the producer post-op segment counts with their phases.  Together they expose
the planner's mode, tile configuration, split count, phases, tap staging, pack layout and the
segment predicates (not the vector / FAST flags: the GPU suite covers those).

A refactor of the planner leaves the fixture alone.  A deliberate change of a planning decision
regenerates it (``python -m tests.test_conv_plan_cpu --write``) and shows the diff in review.
"""
import ctypes
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")

# reference defaults (config.py): z_size, G_h_size, D_h_size, n_colors
Z, GH, DH, COLORS = 128, 128, 128, 3

# (cin, cout, hin, k, stride, pad, transposed)


def _g0(size):
    mult = size // 8
    layers, h = [(Z, GH * mult, 1, 4, 1, 0, True)], 4
    while mult > 1:
        layers.append((GH * mult, GH * (mult // 2), h, 4, 2, 1, True))  # --NN_conv folds to the same k4 s2 p1 ConvT
        mult //= 2
        h *= 2
    return layers + [(GH, COLORS, h, 4, 2, 1, True)]


def _d0(size):
    layers, h, mult = [(COLORS, DH, size, 4, 2, 1, False)], size // 2, 1
    while h > 4:
        layers.append((DH * mult, DH * 2 * mult, h, 4, 2, 1, False))
        h //= 2
        mult *= 2
    return layers + [(DH * mult, 1, 4, 4, 1, 0, False)]


def _arch1():
    g = [(Z, 8192, 1, 1, 1, 0, False), (512, 256, 4, 4, 2, 1, True), (256, 128, 8, 4, 2, 1, True),
         (128, 64, 16, 4, 2, 1, True), (64, COLORS, 32, 3, 1, 1, False)]
    d, h = [], 32
    for cin, cout, k, s in ((COLORS, 64, 3, 1), (64, 64, 4, 2), (64, 128, 3, 1), (128, 128, 4, 2),
                            (128, 256, 3, 1), (256, 256, 4, 2), (256, 512, 3, 1)):
        d.append((cin, cout, h, k, s, 1, False))
        h //= s
    return g + d + [(512, 1, 4, 4, 1, 0, False)]


def _patch1x1(size):
    # image-layer gradients as 1x1 GEMMs over the k4 s2 p1 patch matrix (64 = 16 taps x 4 channels)
    return [(64, DH, size // 2, 1, 1, 0, False), (64, GH, size // 2, 1, 1, 0, False)]


# the planner special cases at the smallest shapes tests/test_kernels_gpu.py lists (SMALL, LAUNCH_NAMES),
# as (batch, cin, cout, hin, k, stride, pad, transposed); the last is a stride-1 ConvT over a map larger than 1 x 1
SPECIAL = [
    (2, 16, 3, 4, 4, 2, 1, True), (2, 3, 128, 32, 4, 2, 1, False), (2, 3, 8, 32, 4, 2, 1, False),
    (2, 16, 1, 4, 4, 1, 0, False), (2, 16, 3, 8, 3, 1, 1, False),
    (2, 8, 16, 16, 4, 2, 1, False), (3, 3, 8, 16, 4, 2, 1, False), (2, 16, 8, 8, 4, 2, 1, True),
    (2, 8, 3, 8, 4, 2, 1, True), (5, 16, 32, 1, 4, 1, 0, True), (4, 64, 32, 1, 4, 1, 0, True),
    (5, 32, 1, 4, 4, 1, 0, False), (2, 12, 20, 8, 3, 1, 1, False), (2, 64, 128, 8, 4, 2, 1, False),
    (2, 128, 64, 4, 4, 2, 1, True), (7, 20, 36, 10, 4, 2, 1, False), (2, 32, 64, 16, 4, 2, 1, False),
    (2, 64, 32, 16, 4, 2, 1, True), (3, 64, 128, 16, 4, 2, 1, False), (2, 8, 16, 4, 3, 1, 1, True),
]


def _edges():
    """The non-square maps and the geometries beyond the networks' three that tests/test_conv_edges_gpu.py runs
    (tests/conv_ref.py: FAMILIES in both orientations, SIZE1, GEOMETRIES), as (..., transposed, win)."""
    from tests import conv_ref
    return [(c.B, c.cin, c.cout, c.H, c.k, c.s, c.p, c.tr, c.W) for c in conv_ref.all_cases()]


def _strides(C, H, W, nchw):
    return (C * H * W, H * W, W, 1) if nchw else (H * W * C, 1, W * C, C)


def descriptors():
    """[(name, fields)]: fields = batch, cin, hin, win, cout, hout, wout, k, stride, pad, transposed, xs, ys."""
    shapes = []
    for size in (32, 64, 128):
        shapes += [(b,) + l for l in _g0(size) + _d0(size) + _patch1x1(size) for b in (32, 2)]
    shapes += [(b,) + l for l in _arch1() for b in (32, 2)]
    shapes += SPECIAL
    n_before = len(shapes)
    shapes += _edges()
    out, seen, first_edge = [], set(), None
    for i, (B, cin, cout, hin, k, s, p, tr, *win) in enumerate(shapes):
        if i == n_before:
            first_edge = len(out)
        win = win[0] if win else hin  # optional: square maps unless given
        hout, wout = ((n - 1) * s - 2 * p + k if tr else (n + 2 * p - k) // s + 1 for n in (hin, win))
        # the image-side tensor: the output of a transposed conv and of a conv down to <= 4 channels, else the input
        y_side = tr or (cout <= 4 and cin > 4)
        for layout in ("nhwc", "nchw"):
            xs = _strides(cin, hin, win, layout == "nchw" and not y_side)
            ys = _strides(cout, hout, wout, layout == "nchw" and y_side)
            hw_in, hw_out = (f"{hin}", f"{hout}") if win == hin else (f"{hin}x{win}", f"{hout}x{wout}")
            name = f"b{B}_{'convt' if tr else 'conv'}_{cin}x{hw_in}_to_{cout}x{hw_out}_k{k}s{s}p{p}_{layout}"
            if name not in seen:
                seen.add(name)
                out.append((name, (B, cin, hin, win, cout, hout, wout, k, s, p, int(tr), xs, ys)))
    # the edge rows go in front of the last earlier row: the fixture's last line carries no comma, so rows
    # added behind it would also change it (a fixture diff of added lines only)
    return out[:first_edge - 1] + out[first_edge:] + out[first_edge - 1:first_edge]


def record():
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    prev = lib.rgan_set_gemm_emulation(0)
    try:
        rows = {}
        for name, (B, cin, hin, win, cout, hout, wout, k, s, p, tr, xs, ys) in descriptors():
            d = _lib.RganConv()
            d.batch, d.cin, d.hin, d.win, d.cout, d.hout, d.wout = B, cin, hin, win, cout, hout, wout
            d.kh = d.kw = k
            d.stride, d.pad, d.transposed = s, p, tr
            for i in range(4):
                d.xs[i], d.ys[i] = xs[i], ys[i]
            ref = ctypes.byref(d)
            post = []
            for which in (0, 1):
                for nseg in (1, 2):
                    ph = ctypes.c_int(0)
                    post.append([int(lib.rgan_conv_post_segments(ref, which, 2, nseg, ctypes.byref(ph))), ph.value])
            rows[name] = {
                "workspace": [int(lib.rgan_conv_workspace(ref, which, pre)) for which in (0, 1, 2) for pre in (0, 1)],
                "pack_floats": [int(lib.rgan_conv_pack_floats(ref, which)) for which in (0, 1)],
                "bn_segments": [int(lib.rgan_conv_bn_segments(ref, segs)) for segs in (1, 2)],
                "post_segments": post,
            }
        return rows
    finally:
        lib.rgan_set_gemm_emulation(prev)


def _dump(rows):
    return "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n"


def write_fixture():
    with open(FIXTURE, "w") as f:
        f.write(_dump(record()))


def test_planner_matches_fixture():
    """Every size query of every descriptor equals the recorded one.  A deliberate planner change
    regenerates the fixture (python -m tests.test_conv_plan_cpu --write) and shows the diff in review."""
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert list(got) == list(want)
    assert len(got) >= 200
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    else:
        sys.exit("usage: python -m tests.test_conv_plan_cpu --write")
