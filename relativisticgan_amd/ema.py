"""Exponential moving average of the generator's weights (--rgan_ema_G; not in the reference).

``GeneratorEMA`` owns a second ``DCGAN_G`` whose parameters are the averages
``avg <- avg + (1 - beta_t) (p - avg)`` of G's, stepped by one multi-tensor HIP launch
(csrc/ema.hip, rgan_ema_update) right after every G optimizer step.  ``beta_t`` is ``beta``,
or with warm-up ``min(beta, (1 + t) / (10 + t))`` at update t (the TF ``num_updates`` ramp, so
the first averages are not dominated by the initial weights).  beta, the warm-up switch and the
update count live in device memory, like Adam's step count and the device LR: an update
captured in a HIP graph keeps counting across replays.

Only parameters are averaged.  Buffers (BatchNorm running statistics, num_batches_tracked,
spectral u / v) are copied from G whenever the averaged generator is handed out; its forward
runs in train mode like every G forward of the reference, through the same kernels and
GEMM-layout cache as G itself.
"""
import torch
from torch.autograd.graph import increment_version

from . import ops  # noqa: F401  (registers rgan::ema_update_)
from .nets import DCGAN_G


class GeneratorEMA:
    def __init__(self, G, param, beta, warmup=True):
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"moving-average beta must lie in [0, 1), got {beta}")
        self.G = G
        device = next(G.parameters()).device
        # the second net's construction draws from the CPU generator (torch's layer init):
        # fork it, so a run with the average draws what a run without it draws
        with torch.random.fork_rng(devices=[]):
            self.shadow = DCGAN_G(param)
        self.shadow.to(device)
        with torch.no_grad():
            for q, p in zip(self.shadow.parameters(), G.parameters()):
                if q.stride() != p.stride():  # the kernel walks avg and p with one flat index
                    q.data = torch.empty_like(p)
                q.requires_grad_(False)
        self.beta, self.warmup = float(beta), bool(warmup)
        self.hyper = torch.tensor([self.beta, float(self.warmup)], dtype=torch.float64).to(device)
        self.count = torch.zeros(1, dtype=torch.float32, device=device)
        self.restart()

    def restart(self):
        """The average starts (again) at G's current weights, with no update taken."""
        with torch.no_grad():
            for q, p in zip(self.shadow.parameters(), self.G.parameters()):
                q.copy_(p)
            self.count.zero_()
        self._sync_buffers()

    @torch.no_grad()
    def update(self):
        """One step of the average over G's parameters, in G.parameters() order (one
        rgan::ema_update_: the count bump and one launch per 48 tensors)."""
        torch.ops.rgan.ema_update_(list(self.shadow.parameters()), [p.detach() for p in self.G.parameters()],
                                   self.hyper, self.count)

    @torch.no_grad()
    def _sync_buffers(self):
        for b, src in zip(self.shadow.buffers(), self.G.buffers()):
            b.copy_(src)

    def generator(self):
        """The averaged generator, ready for a forward: G's current buffers, and every cached
        GEMM layout of the averaged weights marked stale.  The layouts are keyed by the weights'
        host-side version counters, which a HIP-graph replay of ``update`` does not move, so
        the versions are bumped here on every call and the next forward repacks."""
        self._sync_buffers()
        for q in self.shadow.parameters():
            increment_version(q)
        return self.shadow

    @property
    def num_updates(self):
        return int(self.count.item())  # the device counter: replays of a captured update count too

    def state_dict(self):
        """``G_ema_state`` loads into a plain ``DCGAN_G`` (G's keys, in G's order)."""
        self._sync_buffers()
        return {"beta": self.beta, "warmup": self.warmup, "num_updates": self.num_updates,
                "G_ema_state": self.shadow.state_dict()}

    def load_state_dict(self, sd):
        """Weights, count, beta and warm-up of ``state_dict()`` (the saved beta replaces the
        constructor's, as a loaded optimizer's learning rate does)."""
        beta, warmup = float(sd["beta"]), bool(sd["warmup"])
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"moving-average beta must lie in [0, 1), got {beta}")
        self.shadow.load_state_dict(sd["G_ema_state"])
        self.beta, self.warmup = beta, warmup
        with torch.no_grad():
            self.hyper.copy_(torch.tensor([beta, float(warmup)], dtype=torch.float64))
            self.count.fill_(float(sd["num_updates"]))
        for q in self.shadow.parameters():
            increment_version(q)
