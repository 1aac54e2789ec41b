"""The relaxation loop of ``cmf_amd.ManifoldGeodesic.mean`` in float64 on the oracle: the same constants as the
projection (lambda_0 = 1e-3, x 10 / x 0.1, clamps 1e-12 / 1e8), the same strict ``<`` acceptance on the energy and the same closing
evaluation at lambda = 0, on the fixtures' own models, with the block-arrow system of every star assembled densely and solved by a
dense Cholesky.  The host tests establish on it the conditions the GPU tests assert of the product."""
import torch

from _geodesic_reference import FIXTURES                                # noqa: F401  (the fixtures of the geodesic tests)
from _projection_reference import DAMPING, DAMPING_MAX, DAMPING_MIN, DOWN, UP, Model

ARMS, POINTS, STEPS = 3, 5, 10
WEIGHTS = (1.0, 2.0, 0.5)
ONE_STAR = {"mini_mnist"}                                                # exactly three samples


def star_inputs(y, name):
    """(stars, K, ...) of the fixture's batch ``y``: star s takes the samples s, S + s and 2 S + s."""
    S = 1 if name in ONE_STAR else y.shape[0] // ARMS
    return torch.stack([y[k * S:(k + 1) * S] for k in range(ARMS)], 1)


def arm_sum(w, t):
    """sum_k w_k t[:, k] in arm order."""
    out = w[:, 0] * t[:, 0]
    for k in range(1, w.shape[1]):
        out = out + w[:, k] * t[:, k]
    return out


def segments(x_hat, B, K, P):
    """||x_{i+1} - x_i||^2 (B, K, P - 1) of star-major decoded points."""
    x = x_hat.reshape(B, K, P, -1)
    return ((x[:, :, 1:] - x[:, :, :-1]) ** 2).sum(3)


def evaluate(model, z, w, lam):
    """At the stars z (B, K, P, d): grad (B, K, M, d) = w_k g_{k,i}, grad_centre (B, d), delta, delta_centre = (H + lam diag H)^-1
    grad on the dense ((K M + 1) d)^2 system, info (0, or 1 where the factorisation fails), and the Jacobians J (B, K, P, D, d)."""
    B, K, P, d = z.shape
    M, N = P - 2, P - 1
    _, x_hat, J = model.jacobian(z.reshape(B * K * P, d))
    x, J = x_hat.reshape(B, K, P, -1), J.reshape(B, K, P, -1, d)
    s = x[:, :, :-2] + x[:, :, 2:] - 2.0 * x[:, :, 1:-1]
    grad = w[:, :, None, None] * torch.einsum("bkirc,bkir->bkic", J[:, :, 1:-1], s)
    gcen = torch.einsum("bkrc,bkr->bkc", J[:, :, N], x[:, :, M] - x[:, :, N])
    grad_centre = (w[:, :, None] * gcen).sum(1)
    n, oc = (K * M + 1) * d, K * M * d
    H = torch.zeros(B, n, n, dtype=z.dtype)
    gram = lambda a, b: torch.einsum("bra,brc->bac", a, b)
    for k in range(K):
        wk = w[:, k, None, None]
        for i in range(1, M + 1):
            o = (k * M + i - 1) * d
            H[:, o:o + d, o:o + d] = 2.0 * wk * gram(J[:, k, i], J[:, k, i])
            o2 = o + d if i < M else oc
            C = wk * gram(J[:, k, i], J[:, k, i + 1])
            H[:, o:o + d, o2:o2 + d] = -C
            H[:, o2:o2 + d, o:o + d] = -C.transpose(1, 2)
        H[:, oc:, oc:] += wk * gram(J[:, k, N], J[:, k, N])
    A = H + torch.diag_embed(lam[:, None] * torch.diagonal(H, dim1=1, dim2=2))
    L, info = torch.linalg.cholesky_ex(A)
    ok = info == 0
    eye = torch.eye(n, dtype=z.dtype).expand_as(L)
    rhs = torch.cat([grad.reshape(B, oc), grad_centre], 1)
    delta = torch.cholesky_solve(rhs[:, :, None], torch.where(ok[:, None, None], L, eye))[:, :, 0]
    delta = torch.where(ok[:, None], delta, torch.full_like(delta, float("nan")))
    return grad, grad_centre, delta[:, :oc].reshape(B, K, M, d), delta[:, oc:], (~ok).int(), J


def mean(model, zs, w, points=POINTS, steps=STEPS):
    """The loop on the latents zs (B, K, d) with the weights w (B, K).  Beside the product's outputs: ``energies`` (steps + 1, B),
    the energy after every iteration, and ``jacobian`` (B, K, P, D, d) at the returned star."""
    B, K, d = zs.shape
    P, N = points, points - 1
    w_sum = arm_sum(w, torch.ones_like(w))
    zc = (w[:, :, None] * zs).sum(1) / w_sum[:, None]
    tt = torch.arange(P, dtype=zs.dtype) / N
    z = zs[:, :, None, :] + tt[None, None, :, None] * (zc[:, None, :] - zs)[:, :, None, :]
    z[:, :, N] = zc[:, None, :]
    decode = lambda zz: model.decode(zz.reshape(B * K * P, d))

    def at(zz):
        x_hat = decode(zz)
        seg2 = segments(x_hat, B, K, P)
        return x_hat.reshape(B, K, P, -1), seg2, N * arm_sum(w, seg2.sum(2))

    x_hat, seg2, energy = at(z)
    seg2_0, energy_0 = seg2.clone(), energy.clone()
    lam = torch.full_like(energy, DAMPING)
    accepted = torch.zeros(B, dtype=torch.int32)
    history = [energy.clone()]
    for _ in range(steps):
        _, _, delta, delta_c, info, _ = evaluate(model, z, w, lam)
        solved = info == 0
        z_new = z.clone()
        z_new[:, :, 1:N] += torch.where(solved[:, None, None, None], delta, torch.zeros_like(delta))
        z_new[:, :, N] += torch.where(solved[:, None], delta_c, torch.zeros_like(delta_c))[:, None, :]
        x_new, seg2_new, energy_new = at(z_new)
        ok = solved & (energy_new < energy)
        z = torch.where(ok[:, None, None, None], z_new, z)
        x_hat = torch.where(ok[:, None, None, None], x_new, x_hat)
        seg2 = torch.where(ok[:, None, None], seg2_new, seg2)
        energy = torch.where(ok, energy_new, energy)
        lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
        accepted += ok
        history.append(energy.clone())
    grad, grad_centre, _, _, info, J = evaluate(model, z, w, torch.zeros_like(lam))
    lengths, lengths_0 = seg2.sqrt(), seg2_0.sqrt()
    gmax = torch.maximum(grad.abs().flatten(1).max(1).values, grad_centre.abs().max(1).values)
    return {"mean_latent": z[:, 0, N], "latents": z, "path_head": x_hat, "energy": energy, "initial_energy": energy_0,
            "variance": energy / w_sum, "distances": lengths.sum(2), "initial_distances": lengths_0.sum(2), "segment_lengths": lengths,
            "gradient": grad, "gradient_centre": grad_centre, "gradient_max": gmax, "accepted": accepted, "damping": lam, "info": info,
            "energies": torch.stack(history), "jacobian": J}


_CACHE = {}


def reference_run(name):
    """(model, weights (stars, K), start, end): the fixture's stars at the start (steps = 0) and after the loop, computed once."""
    if name not in _CACHE:
        model = Model(name)
        ys = star_inputs(model.y, name)
        zs = model.encode(ys.flatten(0, 1)).reshape(ys.shape[0], ARMS, -1)
        w = torch.tensor(WEIGHTS, dtype=torch.float64).expand(ys.shape[0], ARMS).contiguous()
        _CACHE[name] = (model, w) + (mean(model, zs, w, steps=0), mean(model, zs, w))
    return _CACHE[name]
