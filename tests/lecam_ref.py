"""A float64 numpy restatement of the LeCam term (--rgan_lecam), written from the
definition and sharing nothing with the product: the term, both gradients, the move of the
anchors, the call counter, single-side calls, and the shard sums of the data-parallel exchange.
tests/test_lecam_cpu.py checks its gradients against torch float64 autograd."""
import numpy as np


def _vec(y):
    return None if y is None else np.asarray(y, dtype=np.float64).reshape(-1)


def shard_sums(y_real, y_fake, a_real, a_fake):
    """{sum y_real, sum y_fake, sum (y_real - a_fake)^2, sum (y_fake - a_real)^2} of one shard
    (an absent side adds 0)."""
    r, f = _vec(y_real), _vec(y_fake)
    return np.array([0.0 if r is None else r.sum(), 0.0 if f is None else f.sum(),
                     0.0 if r is None else ((r - a_fake) ** 2).sum(),
                     0.0 if f is None else ((f - a_real) ** 2).sum()], dtype=np.float64)


def abs_sums(y_real, y_fake, a_real, a_fake):
    """The sums of absolute terms behind ``shard_sums`` (the scale of its rounding error)."""
    r, f = _vec(y_real), _vec(y_fake)
    return np.array([0.0 if r is None else np.abs(r).sum(), 0.0 if f is None else np.abs(f).sum(),
                     0.0 if r is None else ((r - a_fake) ** 2).sum(),
                     0.0 if f is None else ((f - a_real) ** 2).sum()], dtype=np.float64)


class LeCam:
    """state = {a_real, a_fake, calls}; hyper = {lam, beta, start}."""

    def __init__(self, lam, beta=0.99, start=1, a_real=0.0, a_fake=0.0, calls=0):
        self.lam, self.beta, self.start = float(lam), float(beta), float(start)
        self.a_real, self.a_fake, self.calls = float(a_real), float(a_fake), int(calls)

    @property
    def state(self):
        return [self.a_real, self.a_fake, float(self.calls), 0.0]

    def weight(self):
        return self.lam if self.calls >= self.start else 0.0

    def grads(self, y_real, y_fake, n_global=None):
        """(dL/dy_real, dL/dy_fake) in float64 under the current anchors (None for an absent side)."""
        r, f = _vec(y_real), _vec(y_fake)
        N = float(n_global if n_global is not None else (r if r is not None else f).size)
        w = self.weight()
        gr = None if r is None else (np.zeros_like(r) if w == 0 else 2.0 * w / N * (r - self.a_fake))
        gf = None if f is None else (np.zeros_like(f) if w == 0 else 2.0 * w / N * (f - self.a_real))
        return gr, gf

    def finish(self, sums, n_global, real, fake):
        """The term from the global sums, then the move of the anchors of the sides present;
        the call is counted with the fake side."""
        N = float(n_global)
        w = self.weight()
        L = 0.0
        if w != 0:
            L = w * ((sums[2] / N if real else 0.0) + (sums[3] / N if fake else 0.0))
        first = self.calls == 0
        if real:
            m = sums[0] / N
            self.a_real = m if first else self.beta * self.a_real + (1.0 - self.beta) * m
        if fake:
            m = sums[1] / N
            self.a_fake = m if first else self.beta * self.a_fake + (1.0 - self.beta) * m
            self.calls += 1
        return L

    def step(self, y_real, y_fake, n_global=None):
        """One call on one rank's rows: (L, dL/dy_real, dL/dy_fake), state moved."""
        r, f = _vec(y_real), _vec(y_fake)
        n_global = n_global if n_global is not None else (r if r is not None else f).size
        gr, gf = self.grads(r, f, n_global)
        L = self.finish(shard_sums(r, f, self.a_real, self.a_fake), n_global, r is not None, f is not None)
        return L, gr, gf
