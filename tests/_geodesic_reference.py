"""The relaxation loop of ``cmf_amd.ManifoldGeodesic`` in float64 on the oracle: the same constants as the projection
(lambda_0 = 1e-3, x 10 / x 0.1, clamps 1e-12 / 1e8), the same strict ``<`` acceptance on the energy and the same closing evaluation at
lambda = 0, on the fixtures' own models, with the block tridiagonal system assembled densely.  The host tests establish on it the
conditions the GPU tests assert of the product."""
import torch

from _projection_reference import DAMPING, DAMPING_MAX, DAMPING_MIN, DOWN, UP, Model

POINTS, STEPS = 9, 10
FIXTURES = ["c2b_hepmass", "c2a_power", "c1_sphere_d2", "mini_mnist"]
ONE_CURVE = {"mini_mnist"}


def endpoints(model, name):
    """(y0, y1): the first half of the fixture's batch and the second half (one curve where the model is expensive)."""
    h = len(model.y) // 2
    n = 1 if name in ONE_CURVE else h
    return model.y[:n], model.y[h:h + n]


def segments(x_hat, B, P):
    """||x_{i+1} - x_i||^2 (B, P - 1) of curve-major decoded points."""
    x = x_hat.reshape(B, P, -1)
    return ((x[:, 1:] - x[:, :-1]) ** 2).sum(2)


def evaluate(model, z, lam):
    """At the curves z (B, P, d): grad (B, M, d), delta (B, M, d) = (H + lam diag H)^-1 grad, info (0, or 1 where the factorisation
    fails), and the Jacobians J (B, P, D, d)."""
    B, P, d = z.shape
    M = P - 2
    G, x_hat, J = model.jacobian(z.reshape(B * P, d))
    x, J = x_hat.reshape(B, P, -1), J.reshape(B, P, -1, d)
    s = x[:, :-2] + x[:, 2:] - 2.0 * x[:, 1:-1]
    grad = torch.einsum("birk,bir->bik", J[:, 1:-1], s)
    H = torch.zeros(B, M * d, M * d, dtype=z.dtype)
    for i in range(1, M + 1):
        o = (i - 1) * d
        H[:, o:o + d, o:o + d] = 2.0 * torch.einsum("bra,brc->bac", J[:, i], J[:, i])
        if i < M:
            C = torch.einsum("bra,brc->bac", J[:, i], J[:, i + 1])
            H[:, o:o + d, o + d:o + 2 * d] = -C
            H[:, o + d:o + 2 * d, o:o + d] = -C.transpose(1, 2)
    A = H + torch.diag_embed(lam[:, None] * torch.diagonal(H, dim1=1, dim2=2))
    L, info = torch.linalg.cholesky_ex(A)
    ok = info == 0
    eye = torch.eye(M * d, dtype=z.dtype).expand_as(L)
    delta = torch.cholesky_solve(grad.reshape(B, M * d, 1), torch.where(ok[:, None, None], L, eye))[:, :, 0]
    delta = torch.where(ok[:, None], delta, torch.full_like(delta, float("nan"))).reshape(B, M, d)
    return grad, delta, (~ok).int(), J


def connect(model, z0, z1, points=POINTS, steps=STEPS):
    """The loop between the latents z0 and z1 (B, d).  Beside the product's outputs: ``energies`` (steps + 1, B), the energy after
    every iteration, and ``jacobian`` (B, P, D, d) at the returned curve."""
    B, d = z0.shape
    P, N = points, points - 1
    tt = torch.arange(P, dtype=z0.dtype) / N
    z = z0[:, None, :] + tt[None, :, None] * (z1 - z0)[:, None, :]
    z[:, N] = z1
    decode = lambda zz: model.decode(zz.reshape(B * P, d))
    x_hat = decode(z)
    seg2 = segments(x_hat, B, P)
    energy = N * seg2.sum(1)
    seg2_0, energy_0 = seg2.clone(), energy.clone()
    lam = torch.full_like(energy, DAMPING)
    accepted = torch.zeros(B, dtype=torch.int32)
    history = [energy.clone()]
    for _ in range(steps):
        _, delta, info, _ = evaluate(model, z, lam)
        solved = info == 0
        z_new = z.clone()
        z_new[:, 1:N] += torch.where(solved[:, None, None], delta, torch.zeros_like(delta))
        x_new = decode(z_new)
        seg2_new = segments(x_new, B, P)
        energy_new = N * seg2_new.sum(1)
        ok = solved & (energy_new < energy)
        z = torch.where(ok[:, None, None], z_new, z)
        x_hat = torch.where(ok.view(B, 1, 1), x_new.reshape(B, P, -1), x_hat.reshape(B, P, -1))
        seg2 = torch.where(ok[:, None], seg2_new, seg2)
        energy = torch.where(ok, energy_new, energy)
        lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
        accepted += ok
        history.append(energy.clone())
    grad, _, info, J = evaluate(model, z, torch.zeros_like(lam))
    lengths, lengths_0 = seg2.sqrt(), seg2_0.sqrt()
    return {"latents": z, "path_head": x_hat.reshape(B, P, -1), "energy": energy, "initial_energy": energy_0,
            "length": lengths.sum(1), "initial_length": lengths_0.sum(1), "segment_lengths": lengths, "gradient": grad,
            "gradient_max": grad.abs().flatten(1).max(1).values, "accepted": accepted, "damping": lam, "info": info,
            "energies": torch.stack(history), "jacobian": J}


_CACHE = {}


def reference_run(name):
    """(model, start, end): the fixture's curves on the straight latent line (steps = 0) and after the loop, computed once."""
    if name not in _CACHE:
        model = Model(name)
        y0, y1 = endpoints(model, name)
        z0, z1 = model.encode(y0), model.encode(y1)
        _CACHE[name] = (model, connect(model, z0, z1, steps=0), connect(model, z0, z1))
    return _CACHE[name]
