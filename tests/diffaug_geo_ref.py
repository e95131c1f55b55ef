"""Torch restatement of the geometric groups of --rgan_diffaug (include/rgan.h rgan_diffaug_geo,
DESIGN §3), composed with tests/diffaug_ref.py's colour, move and cutout:

    y = cutout( translate( Warp( Rot90^k( Flip( col(x) ) ) ) ) )

written step by step -- torch.flip, torch.rot90, an explicit four-tap gather -- one sample at a
time.  Device- and dtype-agnostic: values are computed in x's dtype on x's device; the
parameters are always derived in float64 from the float32 uniforms.  The adjoint is
torch.autograd's derivative of that forward (the transform is affine in x), so it shares
nothing with the kernel's gather-window argument.
"""
import math

import torch

from tests import diffaug_ref as base

XFLIP, ROT90, WARP = 8, 16, 32


def params(v, policy):
    """Per-sample flip (bool), k (int64 in 0..3), s and theta (float64); a group whose bit is
    clear has its identity value."""
    vd = v.detach().double()
    B = vd.shape[0]
    flip = vd[:, 0] >= 0.5 if policy & XFLIP else torch.zeros(B, dtype=torch.bool, device=v.device)
    k = torch.floor(vd[:, 1] * 4).long().clamp(max=3) if policy & ROT90 else torch.zeros(B, dtype=torch.int64,
                                                                                          device=v.device)
    if policy & WARP:
        s, theta = torch.pow(2.0, (vd[:, 2] - 0.5) / 2), (2 * vd[:, 3] - 1) * math.pi
    else:
        s, theta = torch.ones(B, dtype=torch.float64, device=v.device), torch.zeros(B, dtype=torch.float64,
                                                                                    device=v.device)
    return dict(flip=flip, k=k, s=s, theta=theta)


def open_masks(policy, gate, v, p):
    """The policy restricted, sample by sample, to the groups whose gate is below (float32) p:
    colour / translation / cutout from gate[:, 0..2], xflip / rot90 / warp from v[:, 4..6]."""
    pf = torch.tensor(float(p), dtype=torch.float64).float()
    cols = torch.cat([gate[:, :3].cpu(), v[:, 4:7].cpu()], dim=1)
    is_open = cols < pf
    return [policy & sum(1 << g for g in range(6) if is_open[b, g]) for b in range(gate.shape[0])]


def warp_coords(H, W, s, theta, device=None):
    """(r, c), float64 [H][W]: where output (i, j) of Warp samples its input."""
    ci, cj = (H - 1) / 2, (W - 1) / 2
    di = torch.arange(H, dtype=torch.float64, device=device)[:, None] - ci
    dj = torch.arange(W, dtype=torch.float64, device=device)[None, :] - cj
    cs, sn = math.cos(theta), math.sin(theta)
    return ci + (cs * di + sn * dj) / s, cj + (-sn * di + cs * dj) / s


def warp(z, s, theta):
    """Warp(z) for one sample z [C][H][W]: the four lattice neighbours of (r, c) that lie inside
    the image, each with weight max(0, 1 - |r - q_r|) max(0, 1 - |c - q_c|)."""
    C, H, W = z.shape
    r, c = warp_coords(H, W, s, theta, z.device)
    r0, c0 = torch.floor(r), torch.floor(c)
    out = torch.zeros_like(z)
    for dr in (0, 1):
        for dc in (0, 1):
            qr, qc = r0 + dr, c0 + dc
            w = (1 - (r - qr).abs()).clamp_min(0) * (1 - (c - qc).abs()).clamp_min(0)
            inside = (qr >= 0) & (qr < H) & (qc >= 0) & (qc < W)
            w = torch.where(inside, w, torch.zeros_like(w)).to(z.dtype)
            out = out + w * z[:, qr.clamp(0, H - 1).long(), qc.clamp(0, W - 1).long()]
    return out


def forward(x, u, v, policy, affine=True):
    """y = T(x); ``affine=False``: the linear part alone (no brightness offset)."""
    B, C, H, W = x.shape
    g = params(v, policy)
    col = base.forward(x, u, policy & 1, affine)  # the colour map alone: its means are those of x
    rows = []
    for b in range(B):
        z = col[b]
        if g["flip"][b]:
            z = torch.flip(z, (2,))
        z = torch.rot90(z, int(g["k"][b]), (1, 2))
        if policy & WARP:
            z = warp(z, float(g["s"][b]), float(g["theta"][b]))
        rows.append(z)
    p = base.params(u, H, W, policy & 6)
    return base._moved(torch.stack(rows), p["tx"], p["ty"], False, p)[0]


def adjoint(dy, u, v, policy):
    """dx = T^t dy, as autograd's derivative of the (affine) forward."""
    x = torch.zeros_like(dy, requires_grad=True)
    return torch.autograd.grad(forward(x, u, v, policy, affine=False), x, dy)[0]


def keep_mask(u, shape, policy):
    """The output positions translation and cutout leave a value at (tests/diffaug_ref.py's)."""
    return base.keep_mask(u, shape, policy & 6)
