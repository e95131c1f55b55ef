"""Torch restatement of the --rgan_diffaug transform (include/rgan.h rgan_diffaug):
the forward, its explicit adjoint, and the masks.  Device- and dtype-agnostic: values are
computed in x's dtype on x's device.  The integer parameters (shift, box) are defined on exact
real arithmetic; u * n is exact in float64 for a float32 u and a small integer n, so they are
always derived in float64, whatever x's dtype.
"""
import torch


def params(u, H, W, policy):
    """Per-sample (beta, sat, con) in float64 and integer (tx, ty, r0, r1, c0, c1); a disabled
    part has its identity value (empty box: r1 < r0)."""
    ud = u.detach().double()
    B = ud.shape[0]
    zero = torch.zeros(B, dtype=torch.float64, device=u.device)
    one = zero + 1
    izero = torch.zeros(B, dtype=torch.int64, device=u.device)
    beta, sat, con = (ud[:, 0] - 0.5, 2 * ud[:, 1], ud[:, 2] + 0.5) if policy & 1 else (zero, one, one)

    def pick(col, n):  # min(floor(u n), n - 1)
        return torch.floor(ud[:, col] * n).long().clamp(max=n - 1)

    tx = ty = izero
    if policy & 2:
        Rh, Rw = int(H / 8 + 0.5), int(W / 8 + 0.5)
        tx, ty = pick(3, 2 * Rh + 1) - Rh, pick(4, 2 * Rw + 1) - Rw
    r0 = c0 = izero
    r1 = c1 = izero - 1
    if policy & 4:
        Kh, Kw = int(H / 2 + 0.5), int(W / 2 + 0.5)
        r0 = pick(5, H + 1 - Kh % 2) - Kh // 2
        c0 = pick(6, W + 1 - Kw % 2) - Kw // 2
        r1, c1 = r0 + Kh - 1, c0 + Kw - 1
    return dict(beta=beta, sat=sat, con=con, tx=tx, ty=ty, r0=r0, r1=r1, c0=c0, c1=c1)


def _moved(t, di, dj, cut_at_source, p):
    """out[b,c,i,j] = t[b,c,i+di_b,j+dj_b] where that source exists and the cutout box does not
    cover the position it is tested at (the source, or the output position), else 0; and the
    mask of the positions that received a value."""
    B, C, H, W = t.shape
    dev = t.device
    i, j = torch.arange(H, device=dev)[None, :], torch.arange(W, device=dev)[None, :]
    si, sj = i + di[:, None], j + dj[:, None]                      # [B][H], [B][W]
    row_in, col_in = (si >= 0) & (si < H), (sj >= 0) & (sj < W)
    ci, cj = (si, sj) if cut_at_source else (i.expand(B, H), j.expand(B, W))
    row_cut = (ci >= p["r0"][:, None]) & (ci <= p["r1"][:, None])
    col_cut = (cj >= p["c0"][:, None]) & (cj <= p["c1"][:, None])
    keep = (row_in[:, :, None] & col_in[:, None, :]) & ~(row_cut[:, :, None] & col_cut[:, None, :])  # [B][H][W]
    b = torch.arange(B, device=dev)[:, None, None, None]
    c = torch.arange(C, device=dev)[None, :, None, None]
    src = t[b, c, si.clamp(0, H - 1)[:, None, :, None], sj.clamp(0, W - 1)[:, None, None, :]]
    keep = keep[:, None].expand(B, C, H, W)
    return torch.where(keep, src, torch.zeros((), dtype=t.dtype, device=dev)), keep


def _bc(v, t):
    return v.to(t.dtype)[:, None, None, None]


def keep_mask(u, shape, policy):
    """[B][C][H][W] bool: the forward's output positions that receive a value (the others,
    cut out or with their source outside the image, are 0)."""
    B, C, H, W = shape
    p = params(u, H, W, policy)
    return _moved(torch.zeros(shape, device=u.device), p["tx"], p["ty"], False, p)[1]


def forward(x, u, policy, affine=True):
    """y = T(x); ``affine=False``: the linear part alone (no brightness offset)."""
    p = params(u, x.shape[2], x.shape[3], policy)
    col = x
    if policy & 1:
        mu, m = x.mean(dim=(1, 2, 3), keepdim=True), x.mean(dim=1, keepdim=True)
        col = _bc(p["con"], x) * (_bc(p["sat"], x) * (x - m) + m - mu) + mu
        if affine:
            col = col + _bc(p["beta"], x)
    return _moved(col, p["tx"], p["ty"], False, p)[0]


def adjoint(dy, u, policy):
    """dx = T^t dy: dy scattered back through the move, then the colour map's (symmetric)
    linear part."""
    p = params(u, dy.shape[2], dy.shape[3], policy)
    g = _moved(dy, -p["tx"], -p["ty"], True, p)[0]
    if not policy & 1:
        return g
    sat, con = _bc(p["sat"], g), _bc(p["con"], g)
    return con * (sat * g + (1 - sat) * g.mean(dim=1, keepdim=True)) + (1 - con) * g.mean(dim=(1, 2, 3), keepdim=True)
