"""tests/spectral_ref.py is torch.nn.utils.spectral_norm: the buffers after train-mode and
eval-mode calls, sigma, and autograd's gradient of weight_orig, all in float64 to 1e-12; and
its inputs keep the conditions the GPU tests rely on.  CPU only: no library call is made."""
import pytest
import torch

from tests import spectral_ref as S

TOL = 1e-12

MODULES = {
    "conv": (lambda: torch.nn.Conv2d(5, 7, 3, bias=False), False),
    "conv4x4": (lambda: torch.nn.Conv2d(6, 4, 4, 2, 1), False),
    "convT": (lambda: torch.nn.ConvTranspose2d(5, 7, 4, 2, 1, bias=False), True),
    "convT3x3": (lambda: torch.nn.ConvTranspose2d(3, 6, 3), True),
    "linear": (lambda: torch.nn.Linear(37, 10), False),
}


def _x(m, seed):
    g = torch.Generator().manual_seed(seed)
    if isinstance(m, torch.nn.Linear):
        return torch.randn(3, m.in_features, generator=g, dtype=torch.float64)
    return torch.randn(2, m.in_channels, 6, 6, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(MODULES))
def test_helper_is_torch_spectral_norm(name):
    make, tr = MODULES[name]
    torch.manual_seed(11)
    m = torch.nn.utils.spectral_norm(make().double())
    assert (m.weight_u.dtype, m.weight_v.dtype) == (torch.float64, torch.float64)
    W = m.weight_orig.detach().clone()
    u, v = m.weight_u.clone(), m.weight_v.clone()
    m.train()
    for call in range(3):  # the buffers after one, two and three train-mode calls
        m(_x(m, call))
        u, v, sigma = S.power(W, u, v, tr, eps=1e-12)
        assert S.rel(m.weight_u, u) <= TOL and S.rel(m.weight_v, v) <= TOL, (name, call)
        assert S.rel(m.weight, W / sigma) <= TOL, (name, call)
        if call in (0, 2):
            # autograd's gradient of weight_orig through W / sigma (u, v constant clones)
            G = torch.randn(W.shape, dtype=torch.float64)
            m.weight_orig.grad = None
            m.weight.backward(G)
            dW, corr = S.backward(W, G, u, v, sigma, tr)
            assert S.rel(m.weight_orig.grad, dW) <= TOL, (name, call)
            assert S.rel(m.weight_orig.grad - G / sigma, corr) <= 1e-9, (name, call)
    # eval mode: no power iteration, the buffers stay, sigma from them
    m.eval()
    ub, vb = m.weight_u.clone(), m.weight_v.clone()
    m(_x(m, 9))
    u2, v2, sigma = S.power(W, ub, vb, tr, do_iter=False)
    assert torch.equal(m.weight_u, ub) and torch.equal(m.weight_v, vb)
    assert torch.equal(u2, ub) and torch.equal(v2, vb)
    assert S.rel(m.weight, W / sigma) <= TOL
    # and a sigma from buffers unrelated to W (what the GPU eval-mode test feeds)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        m.weight_u.copy_(torch.nn.functional.normalize(torch.randn(ub.shape, generator=g, dtype=torch.float64), dim=0))
        m.weight_v.copy_(torch.nn.functional.normalize(torch.randn(vb.shape, generator=g, dtype=torch.float64), dim=0))
    m(_x(m, 10))
    _, _, sigma = S.power(W, m.weight_u, m.weight_v, tr, do_iter=False)
    assert S.rel(m.weight, W / sigma) <= TOL
    assert abs(sigma.item()) < 0.5 * S.power(W, u, v, tr)[2].item(), "a recomputed u, v would show"


def test_eps_clamp_matches_torch():
    """With eps above the norms F.normalize divides by eps: the helper does the same."""
    torch.manual_seed(3)
    W = torch.randn(6, 5, 3, 3, dtype=torch.float64)
    u = torch.nn.functional.normalize(torch.randn(6, dtype=torch.float64), dim=0)
    M = W.reshape(6, -1)
    v_t = torch.nn.functional.normalize(M.t() @ u, dim=0, eps=1e3)
    u_t = torch.nn.functional.normalize(M @ v_t, dim=0, eps=1e3)
    u1, v1, sigma = S.power(W, u, torch.zeros(45, dtype=torch.float64), False, eps=1e3)
    assert S.rel(u1, u_t) <= TOL and S.rel(v1, v_t) <= TOL
    assert abs(sigma.item() - torch.dot(u_t, M @ v_t).item()) <= TOL * abs(sigma.item())
    assert v1.norm().item() < 1e-1, "the clamp was taken"


def test_matrix_round_trip():
    for case in S.TABLE:
        shape, tr = case
        W = torch.arange(float(torch.Size(shape).numel()), dtype=torch.float64).reshape(shape)
        M = S.matrix(W, tr)
        assert M.shape[0] == (shape[1] if tr else shape[0])
        assert torch.equal(S.unmatrix(M, shape, tr), W)


@pytest.mark.parametrize("case", S.TABLE, ids=S.case_id)
def test_inputs_keep_their_conditions(case):
    """Seeded; u and v are unit vectors; no tensor above 2 M elements; every norm the power
    iteration divides by is below EPS_CLAMP and far above EPS; with the aligned gradient the
    correction is about as large as the gradient (>= 0.5 of it), with the random one small."""
    a, b = S.inputs(case), S.inputs(case)
    assert all(torch.equal(a[k], b[k]) for k in ("W", "u", "v", "G_rand", "G_aligned"))
    W, tr = a["W"].double(), a["transposed"]
    assert W.numel() <= 2 * 1024 * 1024 and a["W"].dtype == torch.float32
    assert abs(a["u"].double().norm().item() - 1) < 1e-6 and abs(a["v"].double().norm().item() - 1) < 1e-6
    M = S.matrix(W, tr)
    for eps in (S.EPS, S.EPS_CLAMP):
        u, v = a["u"].double(), a["v"].double()
        for call in range(2):
            t = M.t() @ u
            wv = M @ S._normalize(t, eps)
            assert S.EPS < t.norm().item() < S.EPS_CLAMP and S.EPS < wv.norm().item() < S.EPS_CLAMP
            u, v, sigma = S.power(W, u, v, tr, eps=eps)
            assert 1e-30 < sigma.item() < 1e30  # a normal float32, and so is its inverse
            assert wv.abs().max().item() ** 2 > 1e-30  # and so are the squares the norms sum
            if eps == S.EPS_CLAMP:
                assert v.norm().item() < 0.1 and u.norm().item() < 0.1, "the clamp is taken"
    u, v, sigma = S.power(W, a["u"], a["v"], tr)
    ratios = {}
    for key in ("G_rand", "G_aligned"):
        dW, corr = S.backward(W, a[key].double(), u, v, sigma, tr)
        ratios[key] = (corr.norm() / dW.norm()).item()
    assert ratios["G_aligned"] >= 0.5, ratios
    assert ratios["G_rand"] <= 0.5 * ratios["G_aligned"], ratios
