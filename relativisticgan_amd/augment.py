"""Differentiable augmentation of D's inputs (``--rgan_diffaug``; the reference has none).

The same family of random transforms -- colour (brightness, saturation, contrast), translation,
cutout, and the geometric x-flip, quarter turns and warp (zoom with rotation) -- is applied to
every image D sees, reals and fakes alike, each sample with its own parameters, and the
generator's gradient flows back through it (DESIGN §3 has the algebra, include/rgan.h
rgan_diffaug / rgan_diffaug_geo the kernels).  This module holds the policy parsing, the draw
of the per-sample uniforms and the autograd node the training step uses.

``--rgan_aug_p`` / ``--rgan_ada_target`` set the augmentation's strength: each of a sample's
three transform groups is applied with probability p (one more row of uniforms per sample, the
gates; rgan_diffaug_p), and ``AdaptiveP`` moves p during training from how well D ranks the
(real, fake) pairs of its own steps (csrc/ada.hip).
"""
import torch

from . import dp
from . import kernels as K
from . import ops  # noqa: F401  (registers rgan::ada_update_)

BITS = {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16, "warp": 32}
GEO = 8 | 16 | 32  # the groups of rgan_diffaug_geo: they take a row of uniforms of their own
COLUMNS = 8  # uniforms per sample: 0..6 used, 7 reserved
GEO_COLUMNS = 8  # flip, quarter turns, zoom, angle, the three gates, reserved
GATE_COLUMNS = 4  # gates per sample: colour, translation, cutout, reserved


def parse_policy(policy):
    """``"color,translation,cutout,xflip,rot90,warp"`` or any subset -> the kernel's bitmask
    ('' / None: 0, off)."""
    mask = 0
    for name in (policy or "").split(","):
        name = name.strip()
        if not name:
            continue
        if name not in BITS:
            raise ValueError(f"--rgan_diffaug: unknown augmentation {name!r} (choose from {', '.join(BITS)})")
        mask |= BITS[name]
    return mask


def validate(policy, pac=1):
    """The mask of ``policy``; PacGAN packing is not supported together with it."""
    mask = parse_policy(policy)
    if mask and pac != 1:
        raise ValueError("--rgan_diffaug with --rgan_pac 2 is not supported: D's packed input holds two samples "
                         "per row, and the transform is drawn per sample")
    return mask


def draw(rows, host, dev_rng=None):
    """[rows][8] uniforms in [0, 1) for the GLOBAL batch: the CPU generator (``host``) or the
    device generator; the caller shards them like its other draws."""
    if host:
        return torch.rand(rows, COLUMNS)
    return dev_rng.uniform((rows, COLUMNS))


def draw_geo(rows, host, dev_rng=None):
    """[rows][8] uniforms in [0, 1) of the geometric groups for the GLOBAL batch, from the
    generator ``draw`` uses (the caller draws them last, after the gates, and only when the
    policy has a geometric bit, so the other policies keep their random-number stream)."""
    if host:
        return torch.rand(rows, GEO_COLUMNS)
    return dev_rng.uniform((rows, GEO_COLUMNS))


def draw_gates(rows, host, dev_rng=None):
    """[rows][4] gate uniforms in [0, 1) for the GLOBAL batch, from the generator ``draw`` uses
    (the caller draws them directly after it and shards them the same way)."""
    if host:
        return torch.rand(rows, GATE_COLUMNS)
    return dev_rng.uniform((rows, GATE_COLUMNS))


class _DiffAug(torch.autograd.Function):
    """T(x) written into ``out`` (e.g. half of the batched D input); backward = the adjoint,
    under the forward's gates and p when it was gated."""

    @staticmethod
    def forward(ctx, x, u, policy, out, gate, p, geo):
        ctx.policy = policy
        ctx.gated, ctx.geo = gate is not None, geo is not None
        ctx.save_for_backward(*(t for t in (u, gate, p, geo) if t is not None))
        return K.diffaug(x, u, policy, out=out, gate=gate, p=p, geo=geo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        u = saved.pop(0)
        gate, p = (saved.pop(0), saved.pop(0)) if ctx.gated else (None, None)
        geo = saved.pop(0) if ctx.geo else None
        return (K.diffaug(g, u, ctx.policy, adjoint=True, gate=gate, p=p, geo=geo), None, None, None, None, None,
                None)


def apply(x, u, policy, out=None, gate=None, p=None, geo=None):
    """T(x); carries autograd back to ``x`` when it requires grad (the G step's T(G(z))).
    ``gate`` ([B][4] uniforms) and ``p`` (a device double) apply each group with probability p;
    ``geo`` ([B][8] uniforms) goes with a policy that has a geometric bit."""
    if x.requires_grad and torch.is_grad_enabled():
        return _DiffAug.apply(x, u, policy, out, gate, p, geo)
    return K.diffaug(x, u, policy, out=out, gate=gate, p=p, geo=geo)


class AdaptiveP:
    """The augmentation probability and its controller: two device arrays, ``state`` =
    double[4] {p, S, N, calls} and ``hyper`` = double[4] {target, interval, images_per_unit_p, 0}
    (include/rgan.h rgan_ada_update).  ``target`` 0: p stays where it was put and ``update`` does
    nothing.  Everything the kernels need is read on the device, so an iteration captured in a
    HIP graph keeps adapting across replays."""

    def __init__(self, device, p=0.0, target=0.0, interval=4, kimg=500.0):
        self.adaptive = target > 0
        self.interval = int(interval)
        self.state = torch.tensor([float(p), 0.0, 0.0, 0.0], dtype=torch.float64).to(device)
        self.hyper = torch.tensor([float(target), float(interval), float(kimg) * 1000.0, 0.0],
                                  dtype=torch.float64).to(device)
        self.p = self.state[:1]  # what the gated transform reads
        self.p0 = float(p)
        self.calls = 0  # host mirror of state[3]: schedules the data-parallel exchange (never captured)

    def restart(self):
        """Back to the constructor's probability with nothing counted."""
        with torch.no_grad():
            self.state.copy_(torch.tensor([self.p0, 0.0, 0.0, 0.0], dtype=torch.float64))
        self.calls = 0

    @torch.no_grad()
    def update(self, y_real, y_fake):
        """After a D step's heads: D's outputs on the real and on the generated batch, row by row.
        One rank: one fused launch.  Data parallel: every rank adds its shard, the integer sums
        S, N are all-reduced on the steps where the adjustment is due, and every rank takes the
        controller step on every call, so all of them hold the same counter and the same p."""
        if not self.adaptive:
            return
        y_real, y_fake = y_real.detach().reshape(-1), y_fake.detach().reshape(-1)
        if not dp.active():
            torch.ops.rgan.ada_update_(y_real, y_fake, self.hyper, self.state, True)
        else:
            torch.ops.rgan.ada_update_(y_real, y_fake, self.hyper, self.state, False)
            if (self.calls + 1) % self.interval == 0:
                dp.all_reduce_sum(self.state[1:3])
            K.ada_adjust(self.hyper, self.state)
        self.calls += 1

    def read(self):
        """(p, r) with r = S / N of the pairs counted since the last adjustment (nan before the
        first): one small device read."""
        p, S, N, _ = self.state.tolist()
        return p, (S / N if N > 0 else float("nan"))

    def state_dict(self):
        sn = self.state[1:3].clone()
        if dp.active():  # the pairs every rank has counted since the last adjustment
            dp.all_reduce_sum(sn)
        p, _, _, calls = self.state.tolist()
        S, N = sn.tolist()
        return {"p": p, "S": S, "N": N, "calls": calls}

    def load_state_dict(self, sd):
        """The counters, and under adaptation p (a fixed p is the flag's, not the file's).  The
        saved S, N are sums over all ranks: rank 0 takes them, the others start from 0."""
        lead = dp.rank() == 0
        p = float(sd["p"]) if self.adaptive else float(self.state[0].item())
        with torch.no_grad():
            self.state.copy_(torch.tensor([p, float(sd["S"]) if lead else 0.0, float(sd["N"]) if lead else 0.0,
                                           float(sd["calls"])], dtype=torch.float64))
        self.calls = int(sd["calls"])
