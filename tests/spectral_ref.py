"""One plain statement of spectral normalisation (torch/nn/utils/spectral_norm.py: the power
iteration of compute_weight and the gradient of W / sigma(W) with u, v held constant), the
weight-shape table the spectral kernel tests run on, and their seeded inputs.

Nothing here goes through relativisticgan_amd: the weight comes in its own 2-D or 4-D shape with
a ``transposed`` flag (ConvTranspose2d: torch's dim = 1) and is reshaped with torch's permute /
reshape.  Every function computes in the dtype of ``W``: float64 is the reference, float32 is
torch's own fp32 evaluation of the same formula (the yardstick of the ``env`` bound).
tests/test_spectral_ref_cpu.py pins the float64 results to torch.nn.utils.spectral_norm.
"""
import torch

# (weight shape, transposed): the smallest shapes that reach each branch of the spectral kernels
# of csrc/heads_optim.hip.  In the kernels' view (rows, cols, lo) a Conv2d weight [co][ci][kh][kw]
# has rows = co, cols = ci*kh*kw, a ConvTranspose2d weight [ci][co][kh][kw] has rows = co,
# cols = ci*kh*kw in runs of lo = kh*kw contiguous columns.  A 4x4 kernel gives lo == 16 for
# both kinds, so 4x4 Conv2d weights run the ``lo == 16`` branches as well (with hs = 16 the
# runs are back to back); the ``lo >= cols`` ("flat") branches need one input channel.
TABLE = [
    ((16, 24, 4, 4), False),    # baseline: lo == 16 float4 branches, every loop one pass
    ((8, 80, 4, 4), False),     # cols = 1280: second pass of `e += 256` (cols/4 = 320) in sn_bwd, of
                                # `c += 1024` in sn_norm_v, two column chunks in sn_batch_v
    ((4, 520, 4, 4), False),    # cols = 8320, nq = 2080: partial second pass of `e0 += 2048` in sn_batch_u
    ((72, 5, 4, 4), True),      # ConvT lo == 16 (hs != 16), cols/4 = 288: second pass of `e += 256`
    ((520, 3, 4, 4), True),     # ConvT lo == 16, nq = 2080: second pass of `e0 += 2048` in sn_batch_u
    ((6, 5, 2, 2), True),       # lo = 4: generic strided float4 branch of sn_bwd and sn_batch_v; scalar sn_batch_u
    ((96, 21, 3, 3), False),    # scalar branches, odd cols = 189, two row chunks
    ((7, 5, 3, 3), True),       # lo = 9 strided scalar; 315 elements: the float tail of sn_dot_kernel
    ((70, 3, 1, 1), False),     # 1x1, 3 columns, two row chunks (64 + 6)
    ((10, 37), False),          # 2-D weight: lo = 1
    ((1, 300, 4, 4), False),    # rows == 1
    ((1100, 3, 1, 1), False),   # rows > 1024: sn_norm_u and sn_batch_fin loops; 1100 = 17*64+12 = 68*16+12:
                                # chunk tails; nrc = 69: unrolled-by-16 loop plus tail in sn_batch_t
    ((512, 256, 4, 4), False),  # 2 M elements: the 512-partial cap and four grid-stride passes of sn_dot_kernel
    # beyond that: the branches no conv weight of more than one input channel reaches, and the scalar loops' second pass
    ((3, 1, 4, 2080), False),   # lo = cols = 8320 ("flat" float4 branch of sn_bwd, nine passes of `c += 1024`;
                                # partial second pass of `c0 += 8192` in sn_batch_u)
    ((260, 2, 2, 2), True),     # lo = 4, cols = 1040: partial second pass of `c += 1024`, generic strided float4
    ((4, 30, 3, 3), False),     # scalar, cols = 270: partial second pass of `c += 256` in sn_bwd, sn_batch_u and sn_wtu
]
EPS = 1e-12
EPS_CLAMP = 1e3   # above every norm of the table's inputs (test_spectral_ref_cpu.py): the clamp is taken


def case_id(case):
    shape, tr = case
    return "x".join(map(str, shape)) + ("T" if tr else "")


def matrix(W, transposed):
    """torch's reshape_weight_to_matrix: dim 1 first for a transposed conv, then flattened."""
    if transposed:
        W = W.permute(1, 0, *range(2, W.dim()))
    return W.reshape(W.shape[0], -1)


def unmatrix(M, shape, transposed):
    """The inverse of ``matrix``: a [rows][cols] matrix back in the weight's own layout."""
    if not transposed:
        return M.reshape(shape)
    s = (shape[1], shape[0]) + tuple(shape[2:])
    return M.reshape(s).permute(1, 0, *range(2, len(shape))).contiguous()


def _normalize(x, eps):
    return x / x.norm().clamp_min(eps)


def power(W, u, v, transposed, eps=EPS, do_iter=True):
    """(u1, v1, sigma) of one spectral_norm call: with ``do_iter`` one power iteration
    v1 = normalize(W^T u), u1 = normalize(W v1), else u, v as given; sigma = u1 . (W v1)."""
    M = matrix(W, transposed)
    u, v = u.to(W.dtype), v.to(W.dtype)
    if do_iter:
        v = _normalize(M.t() @ u, eps)
        u = _normalize(M @ v, eps)
    return u, v, torch.dot(u, M @ v)


def backward(W, G, u, v, sigma, transposed):
    """(dW, correction) for W_eff = W / sigma, sigma = u . (W v), u and v constant:
    dW = G / sigma + correction, correction = -(<G, W> / sigma^2) u v^T in W's layout."""
    u, v, G = u.to(W.dtype), v.to(W.dtype), G.to(W.dtype)
    sigma = torch.as_tensor(sigma, dtype=W.dtype)
    corr = unmatrix(-((G * W).sum() / sigma ** 2) * torch.outer(u, v), tuple(W.shape), transposed)
    return G / sigma + corr, corr


def rel(a, b):
    """rel-L2 of a against b in float64 on the host."""
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def inputs(case):
    """Seeded float32 CPU inputs of a table row: W (std 0.1), a random unit u, a random v
    (neither related to W), a random upstream gradient and one aligned with W
    (G = W / W.std() + 0.5 randn: <G, W> is then large and the correction term about as large
    as the whole gradient)."""
    shape, tr = case
    g = torch.Generator().manual_seed(1000 + TABLE.index(case))
    W = 0.1 * torch.randn(shape, generator=g)
    rows, cols = matrix(W, tr).shape
    u = torch.randn(rows, generator=g)
    u = u / u.norm()
    v = torch.randn(cols, generator=g)
    v = v / v.norm()
    G_rand = torch.randn(shape, generator=g)
    G_al = W / W.std() + 0.5 * torch.randn(shape, generator=g)
    return dict(W=W, u=u, v=v, G_rand=G_rand, G_aligned=G_al, transposed=tr)
