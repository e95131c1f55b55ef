"""Sliced Wasserstein distance between real and generated images (Karras et al., "Progressive
Growing of GANs", ICLR 2018, section 5): a quality number that needs no pretrained network.  The
reference judges quality with FID (code/fid.py: TensorFlow 1 and a downloaded Inception net, ruled
out in DESIGN section 1); this metric has no counterpart there.

Definition (DESIGN "Sliced Wasserstein distance"; the kernels are csrc/swd.hip and csrc/sort.hip,
declared in include/rgan.h).  For two sets of N uint8 images of side S:

1. a Laplacian pyramid per image, levels of side S, S/2, ..., 16 (fp32, values 0..255);
2. per image and level P patches of 7x7xC around centres uniform on [3, side - 4]^2, the same
   for the real and the generated image of equal index; a set's N P descriptors of a level are
   normalised per channel (mean and population standard deviation over the whole set, in double);
3. R repeats of D unit directions; the projections of both sets on each;
4. per direction both sets' N P values sorted; level value = 1000 x the mean |difference|,
   averaged over the repeats.  ``avg`` is the plain mean of the levels.

The centres and directions come from ``rgan_rng_fill`` under a private seed and counter, drawn once
when the object is built, so every ``distance`` of a run uses the same ones and the training streams
are never touched; ``normal`` (the z of ``generate``) continues that private stream.
"""
import torch

from . import kernels as K

_MASK = (1 << 64) - 1
SEED_TAG = 0x5357445F52474131  # mixed into the seed: never the training stream's key
DEFAULT_SEED = 20180430
DEFAULTS = dict(n_images=8192, patches=128, repeats=4, dirs=128)


def private_seed(seed):
    """The Philox key of the metric's stream for a run's ``--seed`` (or the fixed constant)."""
    seed = DEFAULT_SEED if seed is None else int(seed)
    return ((seed * 0x9E3779B97F4A7C15) ^ SEED_TAG) & _MASK


def level_sides(size):
    if size < 32 or size & (size - 1):
        raise ValueError(f"the sliced Wasserstein metric needs an image side that is a power of two >= 32, got {size}")
    sides = []
    while size >= 16:
        sides.append(size)
        size //= 2
    return sides


def format_line(result):
    return "SWD x1e3  " + "  ".join(f"{k}: {result[k]:.4f}" for k in result)


class SlicedWasserstein:
    CHUNK = 512  # images per pyramid pass: bounds the fp32 pyramid (512 x 3 x 256^2 floats = 400 MB)

    def __init__(self, images_u8, p, n_images=None, patches=None, repeats=None, dirs=None, seed=None):
        if not (torch.is_tensor(images_u8) and images_u8.is_cuda and images_u8.dim() == 4
                and images_u8.dtype in (torch.uint8, torch.float32)):
            raise K.L.RganError("SlicedWasserstein: the real images must be a [N][C][S][S] device tensor, uint8 (a "
                                "decoded folder) or float32 in [-1, 1] (the synthetic set)")
        n_images = DEFAULTS["n_images"] if not n_images else int(n_images)
        self.P = DEFAULTS["patches"] if not patches else int(patches)
        self.R = DEFAULTS["repeats"] if not repeats else int(repeats)
        self.D = DEFAULTS["dirs"] if not dirs else int(dirs)
        self.N = min(n_images, images_u8.shape[0])
        self.C, self.S = int(images_u8.shape[1]), int(images_u8.shape[2])
        if (self.C, self.S) != (p.n_colors, p.image_size) or images_u8.shape[3] != self.S:
            raise ValueError(f"SlicedWasserstein: images {tuple(images_u8.shape)} do not go with n_colors "
                             f"{p.n_colors}, image_size {p.image_size}")
        if min(self.N, self.P, self.R, self.D) < 1 or self.D > 512:
            raise ValueError("SlicedWasserstein: needs >= 1 image, patch, repeat and direction, and <= 512 directions")
        self.sides = level_sides(self.S)
        self.Kdim = 49 * self.C
        self.M = self.N * self.P
        if self.M * max(self.D, self.Kdim) >= 2 ** 31:
            raise ValueError("SlicedWasserstein: images x patches x directions must stay below 2^31")
        self.device = images_u8.device
        self.seed = private_seed(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        # the fixed draws, in this order: the centres level by level (finest first), then the directions
        self.pos = {s: K.swd_positions(self._fill((self.N, self.P, 2), 1), s) for s in self.sides}
        self.dirs = [K.swd_unit_columns(self._fill((self.Kdim, self.D), 0)) for _ in range(self.R)]
        real = images_u8[:self.N]
        if real.dtype != torch.uint8:  # normalised floats: the bytes the PNG writer would store for them
            from .images import to_u8
            real = to_u8(real, 0.5, 0.5).permute(0, 3, 1, 2)
        self.real, self.real_stats = self._descriptors(real)

    # ---- the private stream
    def _fill(self, shape, kind):
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        K.L.check(K.L.lib().rgan_rng_fill(K.L.ptr(out), out.numel(), kind, self.seed, K.L.ptr(self.counter),
                                          K.L.stream()), "rgan_rng_fill")
        return out

    def normal(self, shape):
        return self._fill(shape, 0)

    # ---- steps 1 and 2
    def _descriptors(self, u8):
        """Normalised descriptors {side: [M][K]} and their statistics {side: float64 [C][2]} of a
        uint8 [N][C][S][S] view (any strides)."""
        desc = {s: torch.empty((self.M, self.Kdim), dtype=torch.float32, device=self.device) for s in self.sides}
        part = {s: torch.empty((self.N, self.C, 2), dtype=torch.float64, device=self.device) for s in self.sides}
        for lo in range(0, self.N, self.CHUNK):
            hi = min(lo + self.CHUNK, self.N)
            g = [K.swd_load_u8(u8[lo:hi])]
            for _ in self.sides[1:]:
                g.append(K.swd_pyr_down(g[-1]))
            for k, s in enumerate(self.sides):
                lap = K.swd_laplace(g[k], g[k + 1], out=g[k]) if k + 1 < len(g) else g[k]
                K.swd_descriptors(lap, self.pos[s][lo:hi], desc[s][lo * self.P:hi * self.P], part[s][lo:hi])
        stats = {s: K.swd_normalize(desc[s], part[s]) for s in self.sides}
        return desc, stats

    def as_planes(self, u8):
        """A uint8 batch as the [N][C][S][S] view the kernels read: CHW as it is, HWC (the PNG
        writer's bytes, images.to_u8) permuted."""
        if u8.dim() != 4 or u8.dtype != torch.uint8 or u8.shape[0] < self.N:
            raise ValueError(f"SlicedWasserstein: needs at least {self.N} uint8 images, got {tuple(u8.shape)} {u8.dtype}")
        if tuple(u8.shape[1:]) == (self.C, self.S, self.S):
            return u8[:self.N]
        if tuple(u8.shape[1:]) == (self.S, self.S, self.C):
            return u8[:self.N].permute(0, 3, 1, 2)
        raise ValueError(f"SlicedWasserstein: images {tuple(u8.shape)} are neither CHW nor HWC of side {self.S}")

    # ---- steps 3 and 4
    def distance(self, fake_u8):
        """{side: 1000 x level distance, ..., "avg": their mean} between the real set and ``fake_u8``
        (uint8, CHW or HWC).  One repeat at a time: two projection buffers and the sort's scratch."""
        fake, _ = self._descriptors(self.as_planes(fake_u8))
        return self._distance(self.real, fake)

    def _distance(self, a, b):
        sums = torch.zeros((len(self.sides), self.R), dtype=torch.float64, device=self.device)
        pa = torch.empty((self.D, self.M), dtype=torch.float32, device=self.device)
        pb, tmp = torch.empty_like(pa), torch.empty_like(pa)
        for li, s in enumerate(self.sides):
            for r in range(self.R):
                for desc, buf in ((a[s], pa), (b[s], pb)):
                    K.swd_project(desc, self.dirs[r], out=buf)
                    K.sort_segments(buf, out=buf, tmp=tmp)
                K.swd_l1(pa, pb, out=sums[li, r:r + 1])
        host = sums.cpu()  # the only read-back
        out = {}
        for li, s in enumerate(self.sides):
            out[s] = 1000.0 * sum(float(v) / (self.D * self.M) for v in host[li]) / self.R
        out["avg"] = sum(out[s] for s in self.sides) / len(self.sides)
        return out

    # ---- a generator's images
    def generate(self, G, z_size, batch=100):
        """N images of ``G`` as the PNG writer would store them (fake * .5 + .5 quantised,
        images.to_u8), uint8 [N][S][S][C]; ``batch`` per forward, G as it is (train mode: its
        buffers move, see ``evaluate``), z from the private stream."""
        from .images import to_u8
        out = torch.empty((self.N, self.S, self.S, self.C), dtype=torch.uint8, device=self.device)
        with torch.no_grad():
            for lo in range(0, self.N, batch):
                n = min(batch, self.N - lo)
                out[lo:lo + n] = to_u8(G(self.normal((n, z_size, 1, 1))), 0.5, 0.5)
        return out

    def evaluate(self, G, z_size, keep_buffers=True):
        """``distance`` of G's images.  ``keep_buffers``: G's buffers (BatchNorm running statistics
        and counts, spectral-norm vectors) are saved before and put back after, so the forwards
        leave no trace in G's state."""
        saved = [b.clone() for b in G.buffers()] if keep_buffers else None
        fake = self.generate(G, z_size)
        if saved is not None:
            with torch.no_grad():
                for b, s in zip(G.buffers(), saved):
                    b.copy_(s)
        return self.distance(fake)
