"""Nearest training images of generated images, and k-NN precision / recall in pixel space
(Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative Models",
NeurIPS 2019): whether G has memorised a small training set, and how much of it G covers.  The
paper measures in the feature space of a pretrained network; none can be had here (DESIGN section
1), so distances are between box-averaged pixels.  The reference has no counterpart.

Definition (DESIGN "Nearest training images"; the kernels are csrc/nn.hip, declared in
include/rgan.h).  An image [C][S][S] of bytes becomes a descriptor of D = C s s int8 values: the
rounded mean of each f x f box (f = S / s, halves up) minus 128.  d2 is the exact integer squared
distance of two descriptors.  For N real and N generated images and k neighbours:

* ``real_knn`` / ``fake_knn``: each real's (fake's) k nearest among the other reals (fakes);
  ``cross``: each fake's k nearest reals;
* ``fake_nn`` / ``real_nn``: the median of sqrt(d2 / D) to the nearest real over the fakes / over
  the reals (leave-one-out): an RMS difference per pixel in grey levels; ``ratio`` of the two;
* ``precision``: the share of fakes within some real's k-th-neighbour distance of that real;
  ``recall``: the share of reals within some fake's k-th-neighbour distance of that fake.

The integers are read back once; medians, square roots and means are float64 on the host.  z (of
``generate``) comes from a private ``rgan_rng_fill`` stream keyed apart from the training streams
and from the sliced Wasserstein metric's, so neither moves.
"""
import math

import torch

from . import kernels as K

_MASK = (1 << 64) - 1
SEED_TAG = 0x4E4E5F5247414E31  # mixed into the seed: neither the training stream's key nor swd.SEED_TAG
DEFAULT_SEED = 20191208
DEFAULTS = dict(n_images=8192, side=64, k=3)
GRID_ROWS = 8
KEYS = ("fake_nn", "real_nn", "ratio", "precision", "recall")
_LABELS = {"fake_nn": "fake->real", "real_nn": "real->real"}


def private_seed(seed):
    """The Philox key of the check's stream for a run's ``--seed`` (or the fixed constant)."""
    seed = DEFAULT_SEED if seed is None else int(seed)
    return ((seed * 0x9E3779B97F4A7C15) ^ SEED_TAG) & _MASK


def format_line(result, s, k):
    return f"NN s{s} k{k}  " + "  ".join(f"{_LABELS.get(key, key)}: {result[key]:.4f}" for key in KEYS)


def median(values):
    """Median of a sequence of floats; an even count gives the mean of the two middle values."""
    v = sorted(float(x) for x in values)
    n = len(v)
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def rms(d2, D):
    """sqrt(d2 / D) of a sequence of integers as Python floats (float64, each step correctly rounded
    whatever the array library)."""
    return [math.sqrt(int(v) / D) for v in d2]


class NearestNeighbours:
    CHUNK = 2048  # queries per top-k call and float images per conversion: bounds every scratch buffer

    def __init__(self, images, p, n_images=None, side=None, k=None, seed=None):
        if not (torch.is_tensor(images) and images.is_cuda and images.dim() == 4
                and images.dtype in (torch.uint8, torch.float32)):
            raise K.L.RganError("NearestNeighbours: the real images must be a [N][C][S][S] device tensor, uint8 (a "
                                "decoded folder) or float32 in [-1, 1] (the synthetic set)")
        n_images = DEFAULTS["n_images"] if not n_images else int(n_images)
        side = DEFAULTS["side"] if not side else int(side)
        self.k = DEFAULTS["k"] if not k else int(k)
        self.N = min(n_images, images.shape[0])
        self.C, self.S = int(images.shape[1]), int(images.shape[2])
        if (self.C, self.S) != (p.n_colors, p.image_size) or images.shape[3] != self.S:
            raise ValueError(f"NearestNeighbours: images {tuple(images.shape)} do not go with n_colors "
                             f"{p.n_colors}, image_size {p.image_size}")
        if not 1 <= self.k <= 8 or self.N < self.k + 1:
            raise ValueError(f"NearestNeighbours: needs 1 <= k <= 8 and at least k + 1 images, got k {self.k}, "
                             f"{self.N} images")
        self.s = min(side, self.S)
        self.row_bytes = K.nn_row_bytes(self.C, self.s)
        if self.S % self.s or self.S // self.s > 32:
            raise ValueError(f"NearestNeighbours: side {self.s} must divide the image side {self.S}, by at most 32")
        self.D = self.C * self.s * self.s
        self.device = images.device
        self.seed = private_seed(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.images = images  # the set itself (already resident); only the grid's few are ever converted
        self.real, self.real_norm = self._pack_reals()
        self.real_knn = self._topk(self.real, self.real_norm, self.real, self.real_norm, leave_one_out=True)

    # ---- the private stream
    def normal(self, shape):
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        K.L.check(K.L.lib().rgan_rng_fill(K.L.ptr(out), out.numel(), 0, self.seed, K.L.ptr(self.counter),
                                          K.L.stream()), "rgan_rng_fill")
        return out

    # ---- descriptors
    def _real_u8(self, x):
        """Reals as a uint8 [n][C][S][S] view: bytes as they are, normalised floats as the bytes the
        PNG writer would store for them."""
        if x.dtype == torch.uint8:
            return x
        from .images import to_u8
        return to_u8(x, 0.5, 0.5).permute(0, 3, 1, 2)

    def _pack_reals(self):
        if self.images.dtype == torch.uint8:
            return K.nn_pack_u8(self.images[:self.N], self.s)
        desc = torch.empty((self.N, self.row_bytes), dtype=torch.int8, device=self.device)
        norm = torch.empty(self.N, dtype=torch.int32, device=self.device)
        for lo in range(0, self.N, self.CHUNK):
            hi = min(lo + self.CHUNK, self.N)
            desc[lo:hi], norm[lo:hi] = K.nn_pack_u8(self._real_u8(self.images[lo:hi]), self.s)
        return desc, norm

    def as_planes(self, u8, need=1):
        """A uint8 batch as the [n][C][S][S] view the kernels read: CHW as it is, HWC (the PNG
        writer's bytes, images.to_u8) permuted."""
        if u8.dim() != 4 or u8.dtype != torch.uint8 or u8.shape[0] < need:
            raise ValueError(f"NearestNeighbours: needs at least {need} uint8 images, got {tuple(u8.shape)} {u8.dtype}")
        if tuple(u8.shape[1:]) == (self.C, self.S, self.S):
            return u8
        if tuple(u8.shape[1:]) == (self.S, self.S, self.C):
            return u8.permute(0, 3, 1, 2)
        raise ValueError(f"NearestNeighbours: images {tuple(u8.shape)} are neither CHW nor HWC of side {self.S}")

    # ---- neighbours, CHUNK queries at a time
    def _topk(self, a, na, b, nb, leave_one_out=False):
        Q = a.shape[0]
        dist = torch.empty((Q, self.k), dtype=torch.int32, device=self.device)
        idx = torch.empty((Q, self.k), dtype=torch.int32, device=self.device)
        for lo in range(0, Q, self.CHUNK):
            hi = min(lo + self.CHUNK, Q)
            K.nn_topk(a[lo:hi], na[lo:hi], b, nb, self.k, self_offset=lo if leave_one_out else None,
                      out=(dist[lo:hi], idx[lo:hi]))
        return dist, idx

    def _covered(self, a, na, b, nb, radius):
        Q = a.shape[0]
        flag = torch.empty(Q, dtype=torch.int32, device=self.device)
        for lo in range(0, Q, self.CHUNK):
            hi = min(lo + self.CHUNK, Q)
            K.nn_covered(a[lo:hi], na[lo:hi], b, nb, radius, out=flag[lo:hi])
        return flag

    def query(self, fake_u8):
        """``(dist, idx)``, int32 [n][k]: the k nearest reals of each image of ``fake_u8`` (uint8, CHW
        or HWC), squared descriptor distances ascending."""
        f, fn = K.nn_pack_u8(self.as_planes(fake_u8), self.s)
        return self._topk(f, fn, self.real, self.real_norm)

    def _report(self, fake_u8):
        f, fn = K.nn_pack_u8(self.as_planes(fake_u8, self.N)[:self.N], self.s)
        k, N = self.k, self.N
        cross = self._topk(f, fn, self.real, self.real_norm)
        fake_knn = self._topk(f, fn, f, fn, leave_one_out=True)
        prec = self._covered(f, fn, self.real, self.real_norm, self.real_knn[0][:, k - 1].contiguous())
        rec = self._covered(self.real, self.real_norm, f, fn, fake_knn[0][:, k - 1].contiguous())
        host = torch.stack((cross[0][:, 0], self.real_knn[0][:, 0], prec, rec)).cpu()  # the only read-back
        out = {"fake_nn": median(rms(host[0].tolist(), self.D)), "real_nn": median(rms(host[1].tolist(), self.D))}
        out["ratio"] = out["fake_nn"] / out["real_nn"] if out["real_nn"] > 0 else float("inf")
        out["precision"] = float(host[2].sum()) / N
        out["recall"] = float(host[3].sum()) / N
        return out, cross

    def report(self, fake_u8):
        """{fake_nn, real_nn, ratio, precision, recall} of the first N images of ``fake_u8`` (uint8,
        CHW or HWC) against the N reals."""
        return self._report(fake_u8)[0]

    def grid(self, fake_u8, idx):
        """uint8 [(S + 2) 8 + 2][(S + 2)(k + 1) + 2][C] on the device: row i is fake i at full size and
        then reals ``idx[i][0..k-1]`` (as ``query`` returns them; -1 leaves the cell black), each
        cell 2 pixels from the next, pad value 0."""
        S, k, C = self.S, self.k, self.C
        fake = self.as_planes(fake_u8)
        rows = min(GRID_ROWS, fake.shape[0], idx.shape[0])
        ids = idx[:rows, :k].to("cpu", torch.int64)
        shown = sorted({int(v) for v in ids.reshape(-1) if v >= 0})
        reals = {}
        if shown:
            u8 = self._real_u8(self.images.index_select(0, torch.tensor(shown, device=self.device)))
            reals = {r: u8[n] for n, r in enumerate(shown)}
        out = torch.zeros(((S + 2) * GRID_ROWS + 2, (S + 2) * (k + 1) + 2, C), dtype=torch.uint8, device=self.device)
        for i in range(rows):
            cells = [fake[i]] + [reals.get(int(r)) for r in ids[i]]
            for j, cell in enumerate(cells):
                if cell is not None:
                    y, x = 2 + i * (S + 2), 2 + j * (S + 2)
                    out[y:y + S, x:x + S] = cell.permute(1, 2, 0)
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

    def evaluate(self, G, z_size, keep_buffers=True, with_grid=False):
        """``report`` of G's images, or ``(report, grid)`` with ``with_grid``.  ``keep_buffers``: G's
        buffers (BatchNorm running statistics and counts, spectral-norm vectors) are saved before
        and put back after, so the forwards leave no trace in G's state."""
        saved = [b.clone() for b in G.buffers()] if keep_buffers else None
        fake = self.generate(G, z_size)
        if saved is not None:
            with torch.no_grad():
                for b, s in zip(G.buffers(), saved):
                    b.copy_(s)
        result, cross = self._report(fake)
        return (result, self.grid(fake, cross[1])) if with_grid else result
