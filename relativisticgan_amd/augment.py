"""Differentiable augmentation of D's inputs (``--rgan_diffaug``; the reference has none).

The same family of random transforms -- colour (brightness, saturation, contrast), translation,
cutout -- is applied to every image D sees, reals and fakes alike, each sample with its own
parameters, and the generator's gradient flows back through it (DESIGN §3 has the algebra,
include/rgan.h rgan_diffaug the kernel).  This module holds the policy parsing, the draw of
the per-sample uniforms and the autograd node the training step uses.
"""
import torch

from . import kernels as K

BITS = {"color": 1, "translation": 2, "cutout": 4}
COLUMNS = 8  # uniforms per sample: 0..6 used, 7 reserved


def parse_policy(policy):
    """``"color,translation,cutout"`` or any subset -> the kernel's bitmask ('' / None: 0, off)."""
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


class _DiffAug(torch.autograd.Function):
    """T(x) written into ``out`` (e.g. half of the batched D input); backward = the adjoint."""

    @staticmethod
    def forward(ctx, x, u, policy, out):
        ctx.policy = policy
        ctx.save_for_backward(u)
        return K.diffaug(x, u, policy, out=out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        u, = ctx.saved_tensors
        return K.diffaug(g, u, ctx.policy, adjoint=True), None, None, None


def apply(x, u, policy, out=None):
    """T(x); carries autograd back to ``x`` when it requires grad (the G step's T(G(z)))."""
    if x.requires_grad and torch.is_grad_enabled():
        return _DiffAug.apply(x, u, policy, out)
    return K.diffaug(x, u, policy, out=out)
