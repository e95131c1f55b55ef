"""Float64 numpy restatement of the sliced Wasserstein metric (relativisticgan_amd/swd.py, DESIGN
"Sliced Wasserstein distance"), written to be read next to the definition, not next to the
kernels: the pyramid goes through an explicitly zero-stuffed image and ``np.pad(mode="reflect")``,
where csrc/swd.hip uses parity and mirrored indices.

Error model used by the tests (derived here, checked on the CPU in tests/test_swd_cpu.py before a
GPU sees it):

* a pyramid stage (``down`` or ``laplace``) has 25 taps; a stage that rounds every product and sum
  to fp32 is within (taps + 1) u max|value| of the exact result on the same inputs, u = 2^-24 and
  values in [0, 255]: STAGE = 26 * 2^-24 * 255.  (The kernels add in double and round once, which
  is inside this.)  Both filters are averages (``down``'s weights sum to 1, and so do the weights
  of each parity class of ``up`` times 4), so an input error passes through no larger:
  err(G_k) <= k STAGE and err(L_k) <= err(G_k) + err(G_{k+1}) + STAGE.
* ``representable(x)``: where a float64 value is an fp32 number.  For u8 images G_1 lies on the
  grid 2^-8 and G_2 on 2^-16, both exactly in fp32 with every partial sum (value < 2^8, so at most
  24 bits), so the first two ``down`` levels are exact; from G_3 on they are not.
* a projection of K terms accumulated in fp32 in a fixed order is within
  1.01 (K + 8) u sum_k |desc dir| (the form of tests/conv_ref.py).
* sorting is 1-Lipschitz in the max norm: max_i |sort(a)_i - sort(b)_i| <= max_i |a_i - b_i|, so the
  mean |sort A - sort B| moves by at most the largest projection error of A plus that of B.
"""
import numpy as np

W5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
U = 2.0 ** -24
TAPS = 25
STAGE = (TAPS + 1) * U * 255.0


def blur(x):
    """5x5 binomial filter over the last two axes, the border mirrored without repeating the edge."""
    H, W = x.shape[-2:]
    p = np.pad(np.asarray(x, dtype=np.float64), [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode="reflect")
    h = sum(W5[j] * p[..., :, j:j + W] for j in range(5))
    return sum(W5[i] * h[..., i:i + H, :] for i in range(5))


def down(x):
    return blur(x)[..., ::2, ::2]


def up(x):
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]))
    z[..., ::2, ::2] = x
    return 4.0 * blur(z)


def sides(S):
    out = []
    while S >= 16:
        out.append(S)
        S //= 2
    return out


def gaussian(img, rounder=None):
    """[G_0, G_1, ...] down to side 16; ``rounder`` (e.g. fp32 rounding) is applied after a stage."""
    r = rounder or (lambda a: a)
    g = [np.asarray(img, dtype=np.float64)]
    while g[-1].shape[-1] > 16:
        g.append(r(down(g[-1])))
    return g


def laplacian(img, rounder=None):
    """{side: L_k} of images [N][C][S][S] (values 0..255); the last level is G_last itself."""
    r = rounder or (lambda a: a)
    g = gaussian(img, rounder)
    return {g[k].shape[-1]: (r(g[k] - up(g[k + 1])) if k + 1 < len(g) else g[k]) for k in range(len(g))}


def to32(a):
    return a.astype(np.float32).astype(np.float64)


def representable(x64):
    """Elementwise: the float64 value is an fp32 number."""
    x64 = np.asarray(x64, dtype=np.float64)
    return x64.astype(np.float32).astype(np.float64) == x64


def level_bounds(S):
    """{side: bound on |fp32 level - float64 level|} from the stage constant."""
    ss = sides(S)
    return {s: (k + (k + 1) + 1 if k + 1 < len(ss) else k) * STAGE for k, s in enumerate(ss)}


def positions(u, side):
    """3 + floor(u (side - 6)) for u = j 2^-24, in integers."""
    j = np.floor(np.asarray(u, dtype=np.float64) * 2.0 ** 24).astype(np.int64)
    return (3 + ((j * (side - 6)) >> 24)).astype(np.int32)


def gather(level, pos):
    """Rows [N P][49 C] of level [N][C][S][S] around pos [N][P][2] (y, x): k = 49 c + 7 dy + dx."""
    N, C = level.shape[:2]
    P = pos.shape[1]
    out = np.empty((N, P, C, 7, 7), dtype=level.dtype)
    for n in range(N):
        for p in range(P):
            y, x = int(pos[n, p, 0]), int(pos[n, p, 1])
            out[n, p] = level[n, :, y - 3:y + 4, x - 3:x + 4]
    return out.reshape(N * P, C * 49)


def channel_stats(desc, C):
    d = np.asarray(desc, dtype=np.float64).reshape(desc.shape[0], C, 49)
    mean = d.mean(axis=(0, 2))
    std = np.sqrt(((d - mean[None, :, None]) ** 2).mean(axis=(0, 2)))
    return mean, std


def normalize(desc, C):
    d = np.asarray(desc, dtype=np.float64).reshape(desc.shape[0], C, 49)
    mean, std = channel_stats(desc, C)
    safe = np.where(std > 0, std, 1.0)
    out = (d - mean[None, :, None]) / safe[None, :, None]
    out[:, std == 0, :] = 0.0
    return out.reshape(desc.shape[0], C * 49)


def unit_columns(dirs):
    d = np.asarray(dirs, dtype=np.float64)
    return d / np.sqrt((d * d).sum(axis=0, keepdims=True))


def project(desc, dirs):
    """[D][M], float64."""
    return (np.asarray(desc, dtype=np.float64) @ np.asarray(dirs, dtype=np.float64)).T


def project_bound(desc, dirs):
    """[D][M]: 1.01 (K + 8) u sum_k |desc dir|."""
    K = desc.shape[1]
    return 1.01 * (K + 8) * U * (np.abs(np.asarray(desc, dtype=np.float64)) @ np.abs(np.asarray(dirs, dtype=np.float64))).T


def sliced(pa, pb):
    """mean |sort A - sort B| over [D][M] projections."""
    return float(np.abs(np.sort(pa, axis=1) - np.sort(pb, axis=1)).mean())


def descriptors(images, pos, rounder=None):
    """{side: normalised float64 rows} of uint8 images [N][C][S][S] with pos = {side: [N][P][2]}."""
    C = images.shape[1]
    lap = laplacian(images.astype(np.float64), rounder)
    return {s: normalize(gather(lap[s], pos[s]), C) for s in lap}


def min_std(images, pos):
    """{side: the smallest non-zero channel standard deviation of the raw descriptors}."""
    C = images.shape[1]
    lap = laplacian(images.astype(np.float64))
    out = {}
    for s in lap:
        std = channel_stats(gather(lap[s], pos[s]), C)[1]
        out[s] = float(std[std > 0].min()) if (std > 0).any() else 1.0
    return out


def metric_bound(desc, dirs, level_err, std_min):
    """Largest error of one set's fp32 projections against float64: the fp32 accumulation
    (project_bound); the roundings of the descriptors and of the directions to fp32, 2 ulp each at
    the most, so 8 u relative per product; and the pyramid level's error passed through the
    normalisation: level_err / std_min per element, times the direction's 1-norm."""
    d = np.abs(np.asarray(dirs, dtype=np.float64))
    acc = project_bound(desc, dirs).max()
    rounding = 8 * U * (np.abs(np.asarray(desc, dtype=np.float64)) @ d).max()
    return float(acc + rounding + level_err / std_min * d.sum(axis=0).max())


def swd(real, fake, pos, dirs):
    """{side: 1000 x mean over the repeats of sliced(...)}, "avg": their mean; dirs = [R] of unit [K][D]."""
    da, db = descriptors(real, pos), descriptors(fake, pos)
    out = {}
    for s in da:
        out[s] = 1000.0 * float(np.mean([sliced(project(da[s], d), project(db[s], d)) for d in dirs]))
    out["avg"] = float(np.mean([out[s] for s in da]))
    return out


def total_order_keys(x32):
    """uint32 keys whose unsigned order is the sort's: negatives with all bits flipped, the rest with
    the sign bit flipped."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def keys_to_floats(k):
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return u.view(np.float32)
