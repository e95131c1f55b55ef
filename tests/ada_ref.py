"""The adaptive augmentation probability restated on the host (include/rgan.h rgan_ada_update,
rgan_ada_adjust, rgan_diffaug_p): the rank statistic in Python ints, the controller in float64
with the kernel's order of operations, and the per-sample open mask of the gated transform."""
import math

import numpy as np


def rank_counts(y_real, y_fake):
    """(#(real > fake) - #(real < fake), rows) as Python ints; ties and NaNs count 0."""
    a = np.asarray(y_real, dtype=np.float32).reshape(-1)
    b = np.asarray(y_fake, dtype=np.float32).reshape(-1)
    assert a.shape == b.shape
    with np.errstate(invalid="ignore"):
        return int((a > b).sum()) - int((a < b).sum()), int(a.size)


class Controller:
    """state {p, S, N, calls} and hyper {target, interval, images_per_unit_p} of the kernels."""

    def __init__(self, p=0.0, target=0.6, interval=4, images_per_unit_p=500000.0):
        self.p, self.S, self.N, self.calls = float(p), 0, 0, 0
        self.target, self.interval, self.ipu = float(target), interval, float(images_per_unit_p)

    def accumulate(self, y_real, y_fake):
        s, n = rank_counts(y_real, y_fake)
        self.S += s
        self.N += n

    def adjust(self):
        self.calls += 1
        if not (math.fmod(self.calls, self.interval) == 0.0 and self.N > 0):
            return
        d = self.S / self.N - self.target  # int / int: the correctly rounded quotient, as the doubles'
        step = self.N / self.ipu
        p = self.p + step if d > 0 else (self.p - step if d < 0 else self.p)
        self.p = min(max(p, 0.0), 1.0)
        self.S = self.N = 0

    def update(self, y_real, y_fake):
        self.accumulate(y_real, y_fake)
        self.adjust()

    @property
    def state(self):
        return [self.p, float(self.S), float(self.N), float(self.calls)]


def sub_policy(policy, gate, p):
    """Per sample, ``policy`` restricted to the groups whose gate is open: gate[b][g] < float32(p)."""
    g = np.asarray(gate, dtype=np.float32).reshape(-1, 4)
    pf = np.float32(p)
    with np.errstate(invalid="ignore"):
        return [int(policy) & (int(r[0] < pf) | int(r[1] < pf) << 1 | int(r[2] < pf) << 2) for r in g]
