"""The weighted projection loop of ``cmf_amd.ManifoldProjector.complete`` in float64 on the oracle: the loop of
``_projection_reference.project`` -- the same constants, the same strict ``<`` acceptance, the same closing evaluation at lambda = 0
-- on the weighted cost sum_i w_i (y_i - g(z)_i)^2 with the weighted normal equations, and the seeded completion problem the host and
GPU tests share (not collected by pytest)."""
import math

import torch

from _projection_reference import DAMPING, DAMPING_MAX, DAMPING_MIN, DOWN, UP

#: the share of the elements that is observed, the range of their weights, and the size of the perturbation of the hidden ones
OBSERVED, W_LOW, W_HIGH, HIDDEN_REL = 0.5, 0.25, 4.0, 0.1
#: DESIGN 5's x_hat tolerance, as ``TAU`` of the projection tests uses it: the size of the data perturbation of the sensitivity test
DATA_REL = 1e-5
KNOWN_ANSWER = ["c2b_hepmass", "c2a_power", "mini_mnist"]
# End-to-end tolerance of tests/test_gpu_completion.py on ||g(z) - x_on|| / ||x_on|| over ALL elements.  The GPU's x_hat is the
# float64 decoder's within DATA_REL ||x_hat||, so the GPU solves a completion problem whose data is wrong by that much.
# tests/test_completion_host.py measures on the float64 loop how far such a perturbation of the observed data -- DATA_REL ||x_on|| /
# sqrt(D) randn per observed element -- moves the completed point, worst sample per fixture (printed there):
#   c2b_hepmass 1.660e-03, c2a_power 7.487e-03, mini_mnist 4.628e-06
# (the two tabular fixtures observe 11 of 21 and 3 of 6 elements for d = 10 and d = 2: barely more than d, so the weighted Gram matrix
# is poorly conditioned and the data error is amplified a few hundred times; the image fixture observes 392 elements for d = 4)
# and the tolerance is 4 x that, rounded up to a power of two.  The host test re-measures and asserts the factor of four.
E2E_TOL = {"c2b_hepmass": 2.0 ** -7, "c2a_power": 2.0 ** -5, "mini_mnist": 2.0 ** -15}


def cost(w, y, x_hat):
    return (w * (y - x_hat) ** 2).flatten(1).sum(1)


def evaluate(model, w, y, z, lam):
    """The weighted system at z: grad = J^T (w o r), delta = (G_w + lam diag G_w)^-1 grad, grad^T delta, info (0, or 1 where the
    factorisation fails)."""
    _, x_hat, J = model.jacobian(z)
    r = (y - x_hat).flatten(1)
    wf = w.flatten(1)
    G = torch.bmm(J.transpose(1, 2), wf[:, :, None] * J)
    grad = torch.bmm(J.transpose(1, 2), (wf * r)[:, :, None])
    A = G + torch.diag_embed(lam[:, None] * torch.diagonal(G, dim1=1, dim2=2))
    L, info = torch.linalg.cholesky_ex(A)
    ok = info == 0
    eye = torch.eye(G.shape[1], dtype=G.dtype).expand_as(L)
    delta = torch.cholesky_solve(grad, torch.where(ok[:, None, None], L, eye))[:, :, 0]
    grad = grad[:, :, 0]
    delta = torch.where(ok[:, None], delta, torch.full_like(delta, float("nan")))
    return grad, delta, (grad * delta).sum(1), (~ok).int()


def complete(model, y, w, steps=10, z=None):
    """The loop; ``z``: the starting latent (default: the encoder's latent of y).  ``costs``: (steps + 1, B), the cost after
    every step."""
    z = model.encode(y) if z is None else z
    x_hat = model.decode(z)
    c = cost(w, y, x_hat)
    c_0, costs = c.clone(), [c.clone()]
    lam = torch.full_like(c, DAMPING)
    accepted = torch.zeros(len(z), dtype=torch.int32)
    wide = (len(z),) + (1,) * (x_hat.dim() - 1)
    for _ in range(steps):
        _, delta, _, info = evaluate(model, w, y, z, lam)
        solved = info == 0
        z_new = z + torch.where(solved[:, None], delta, torch.zeros_like(delta))
        x_new = model.decode(z_new)
        c_new = cost(w, y, x_new)
        ok = solved & (c_new < c)
        z = torch.where(ok[:, None], z_new, z)
        x_hat = torch.where(ok.view(wide), x_new, x_hat)
        c = torch.where(ok, c_new, c)
        lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
        accepted += ok
        costs.append(c.clone())
    grad, _, tangential2, info = evaluate(model, w, y, z, torch.zeros_like(lam))
    return {"latent": z, "reconstruction_head": x_hat, "cost": c, "initial_cost": c_0, "tangential2": tangential2, "gradient": grad,
            "distance2": ((y - x_hat).flatten(1) ** 2).sum(1), "observed": (w > 0).flatten(1).sum(1).int(), "accepted": accepted,
            "damping": lam, "info": info, "costs": torch.stack(costs)}


def problem(x_on, seed=0, data_rel=0.0):
    """The seeded completion problem on points ``x_on`` (B, ...) of the manifold: per sample a seeded permutation picks the observed
    half of the elements, which get weights uniform in [0.25, 4] and keep their values (plus ``data_rel`` ||x_on|| / sqrt(D) randn);
    the hidden elements get weight 0 and x_on + 0.1 ||x_on|| / sqrt(D) randn.  Returns (y, w) in x_on's dtype, on the CPU."""
    gen = torch.Generator().manual_seed(1000 + seed)
    x64 = x_on.detach().cpu().double()
    B, D = x64.shape[0], x64[0].numel()
    seen = torch.zeros(B, D, dtype=torch.bool)
    for b in range(B):
        seen[b, torch.randperm(D, generator=gen)[:math.ceil(OBSERVED * D)]] = True
    w = torch.where(seen, W_LOW + (W_HIGH - W_LOW) * torch.rand(B, D, dtype=torch.float64, generator=gen), torch.zeros(B, D, dtype=torch.float64))
    unit = x64.flatten(1).norm(dim=1, keepdim=True) / math.sqrt(D)
    noise = torch.randn(B, D, dtype=torch.float64, generator=gen)
    data_noise = torch.randn(B, D, dtype=torch.float64, generator=gen)
    y = x64.flatten(1) + torch.where(seen, data_rel * unit * data_noise, HIDDEN_REL * unit * noise)
    return y.view_as(x64).to(x_on.dtype), w.view_as(x64).to(x_on.dtype)


def rel_distance(x_hat, x_on):
    """||x_hat - x_on|| / ||x_on|| per sample, over all elements, in float64."""
    a, b = x_hat.detach().cpu().double().flatten(1), x_on.detach().cpu().double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))
