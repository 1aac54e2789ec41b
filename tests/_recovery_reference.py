"""The recovery loop of ``cmf_amd.ManifoldProjector.recover`` in float64 on the oracle: the loop of
``_projection_reference.project`` -- the same constants, the same strict ``<`` acceptance, the same closing evaluation at lambda = 0
-- on the measured cost ||y - A g(z)||^2 with K = A J in place of J, and the seeded problems the host and GPU tests share (not
collected by pytest)."""
import math

import torch

from _completion_reference import DATA_REL, pow2_ceil, rel_distance              # noqa: F401  (shared with the tests)
from _projection_reference import DAMPING, DAMPING_MAX, DAMPING_MIN, DOWN, UP

#: the size of the perturbation of the starting input, relative to ||x_on|| / sqrt(D) per element
START_REL = 0.1
#: the known-answer problems: rows M of the seeded Gaussian operator per fixture (D = 21, d = 10; D = 6, d = 2; D = 784, d = 4)
KNOWN_ANSWER = {"c2b_hepmass": 15, "c2a_power": 4, "mini_mnist": 32}
#: the fixtures on which a selection operator and ``complete`` with the matching 0/1 weights end at the same cost well above zero
#: on the float64 loops (tests/test_recovery_host.py).  c1_sphere_d2 does not qualify: it has D = 3 and d = 2, so the seeded half
#: is 2 elements for 2 latents -- both loops fit them exactly, the cost is 0 and a relative comparison has nothing to divide by.
SELECTION = ["c2a_power", "c2b_hepmass"]
#: the underdetermined problem: M < d = 10
UNDERDETERMINED = ("c2b_hepmass", 5)
# End-to-end tolerance of tests/test_gpu_recovery.py on ||g(z) - x_on|| / ||x_on|| over all D elements.  The GPU's x_hat is the
# float64 decoder's within DATA_REL ||x_hat||, so its yhat = A x_hat is off by that much carried through A: the GPU solves
# a recovery problem whose data is wrong by DATA_REL ||yhat|| / sqrt(M) randn per measurement.  tests/test_recovery_host.py measures
# on the float64 loop how far such a perturbation of y moves the recovered point, worst sample per fixture (printed there):
#   c2b_hepmass 1.591e-05, c2a_power 3.570e-05, mini_mnist 5.748e-06
# and the tolerance is 4 x that, rounded up to a power of two.  The host test re-measures and asserts the factor of four.
E2E_TOL = {"c2b_hepmass": 2.0 ** -13, "c2a_power": 2.0 ** -12, "mini_mnist": 2.0 ** -15}


def image(A, x_hat):
    return x_hat.flatten(1) @ A.T


def cost(y, y_hat):
    return ((y - y_hat) ** 2).sum(1)


def evaluate(model, y, A, z, lam):
    """The measured system at z: K = A J, grad = K^T (y - A x_hat), delta = (K^T K + lam diag K^T K)^-1 grad, grad^T delta, info
    (0, or 1 where the factorisation fails)."""
    _, x_hat, J = model.jacobian(z)
    K = torch.matmul(A, J)
    r = y - image(A, x_hat)
    G = torch.bmm(K.transpose(1, 2), K)
    grad = torch.bmm(K.transpose(1, 2), r[:, :, None])
    Ad = G + torch.diag_embed(lam[:, None] * torch.diagonal(G, dim1=1, dim2=2))
    L, info = torch.linalg.cholesky_ex(Ad)
    ok = info == 0
    eye = torch.eye(G.shape[1], dtype=G.dtype).expand_as(L)
    delta = torch.cholesky_solve(grad, torch.where(ok[:, None, None], L, eye))[:, :, 0]
    grad = grad[:, :, 0]
    delta = torch.where(ok[:, None], delta, torch.full_like(delta, float("nan")))
    return grad, delta, (grad * delta).sum(1), (~ok).int()


def recover(model, y, A, z, steps=10):
    """The loop from the starting latent ``z``; y (B, M) and A (M, D) float64.  ``costs``: (steps + 1, B), the cost after every
    step."""
    x_hat = model.decode(z)
    y_hat = image(A, x_hat)
    c = cost(y, y_hat)
    c_0, costs = c.clone(), [c.clone()]
    lam = torch.full_like(c, DAMPING)
    accepted = torch.zeros(len(z), dtype=torch.int32)
    wide = (len(z),) + (1,) * (x_hat.dim() - 1)
    for _ in range(steps):
        _, delta, _, info = evaluate(model, y, A, z, lam)
        solved = info == 0
        z_new = z + torch.where(solved[:, None], delta, torch.zeros_like(delta))
        x_new = model.decode(z_new)
        y_new = image(A, x_new)
        c_new = cost(y, y_new)
        ok = solved & (c_new < c)
        z = torch.where(ok[:, None], z_new, z)
        x_hat = torch.where(ok.view(wide), x_new, x_hat)
        y_hat = torch.where(ok[:, None], y_new, y_hat)
        c = torch.where(ok, c_new, c)
        lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
        accepted += ok
        costs.append(c.clone())
    grad, _, tangential2, info = evaluate(model, y, A, z, torch.zeros_like(lam))
    return {"latent": z, "reconstruction_head": x_hat, "measurement": y_hat, "cost": c, "initial_cost": c_0,
            "tangential2": tangential2, "gradient": grad, "accepted": accepted, "damping": lam, "info": info,
            "costs": torch.stack(costs)}


def gaussian_operator(M, D, seed=0):
    """The seeded operator (M, D): Gaussian scaled by 1 / sqrt(D), float32 values (what the GPU is given), on the CPU."""
    gen = torch.Generator().manual_seed(2000 + 100 * seed + M)
    return (torch.randn(M, D, dtype=torch.float64, generator=gen) / math.sqrt(D)).float()


def selection(D, seed=0):
    """(A (ceil(D / 2), D) float32, w (D,) float32): the rows of the identity for a seeded half of the elements, in ascending
    order, and the matching 0/1 weights."""
    gen = torch.Generator().manual_seed(3000 + seed)
    keep = torch.randperm(D, generator=gen)[:math.ceil(0.5 * D)].sort().values
    w = torch.zeros(D)
    w[keep] = 1.0
    return torch.eye(D)[keep].contiguous(), w


def measure(A, x_on, seed=0, data_rel=0.0):
    """y (B, M) float64 = A x_on in float64 (plus ``data_rel`` ||y|| / sqrt(M) randn per measurement)."""
    y = image(A.double(), x_on.detach().cpu().double())
    if data_rel:
        gen = torch.Generator().manual_seed(4000 + seed)
        y = y + data_rel * y.norm(dim=1, keepdim=True) / math.sqrt(y.shape[1]) * torch.randn(y.shape, dtype=torch.float64, generator=gen)
    return y


def start_input(x_on, seed=0):
    """The crude back-projection the recovery starts from: x_on + 0.1 ||x_on|| / sqrt(D) randn, in x_on's dtype, on the CPU."""
    gen = torch.Generator().manual_seed(5000 + seed)
    x64 = x_on.detach().cpu().double()
    D = x64[0].numel()
    unit = x64.flatten(1).norm(dim=1) / math.sqrt(D)
    noise = torch.randn(x64.shape, dtype=torch.float64, generator=gen)
    return (x64 + START_REL * unit.view(-1, *[1] * (x64.dim() - 1)) * noise).to(x_on.dtype)
