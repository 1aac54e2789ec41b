"""The robust projection loop of ``cmf_amd.ManifoldProjector.robust`` in float64 on the oracle: the loop of
``_completion_reference.complete`` -- the same constants, the same strict ``<`` acceptance, the same closing evaluation at lambda = 0,
its ``evaluate`` for the weighted system -- on the robust cost 2 s^2 sum p rho(r / s), with the weights w = p omega(r / s) of the
current residual in every trial and the scale s = 1.4826 x the lower median of |r| held for a round; and the seeded outlier problem
the host and GPU tests share (not collected by pytest)."""
import math

import torch

import _completion_reference as CR
from _projection_reference import DAMPING, DAMPING_MAX, DAMPING_MIN, DOWN, UP
from _robust_weights_emulation import MAD_TO_SIGMA, TUNING

#: the outlier problem: the share of the elements replaced per fixture, the range of the outliers' size and the noise on every
#: element, both in units of the RMS element ||x_on|| / sqrt(D)
KNOWN_ANSWER = {"mini_mnist_small": 0.10, "mini_cifar": 0.10, "mini_mnist": 0.03}
SHARE = KNOWN_ANSWER
OUT_LOW, OUT_HIGH, NOISE_REL = 3.0, 6.0, 0.01
# The seed of the known-answer problem.  Whether ten steps from the ENCODER's latent of the corrupted input reach the basin of the
# true point depends on the draw: the encoder is not robust, its latent is 2 - 20 % off, and on these relu decoders the loop can
# stall where ``project`` stalls (then robust ~ project and no outlier is found).  Of the seeds 0 .. 15 this float64 loop meets the
# conditions below on 5 (mini_mnist_small), 7 (mini_cifar) and 9 (mini_mnist) -- wherever it does, it is as good as the true mask:
# ratio (a) 0.94 .. 1.08 -- and 4 is the first seed at which it does on all three.  Seeds 0 .. 3 each fail on at least one.
SEED = 4
#: DESIGN 5's x_hat tolerance: the size of the data perturbation of the sensitivity test
DATA_REL = CR.DATA_REL
#: the conditions tests/test_robust_host.py establishes on this loop and tests/test_gpu_robust.py asserts of the product
MASK_FACTOR, PROJECT_FACTOR, OUTLIER_WEIGHT, GOOD_WEIGHT = 2.0, 5.0, 0.05, 0.2
# End-to-end tolerance of tests/test_gpu_robust.py on ||g(z) - g(z_ref)|| / ||g(z_ref)|| between the product's answer and this
# loop's on the same input.  The GPU's x_hat is the float64 decoder's within DATA_REL ||x_hat||, so the GPU solves a
# problem whose data is wrong by that much.  tests/test_robust_host.py measures on this loop how far a perturbation of every
# element by DATA_REL ||x_on|| / sqrt(D) randn moves the robust answer (Huber, rounds = 1, steps = 10), worst sample per fixture
# (printed there):
#   mini_mnist_small 1.001e-06, mini_cifar 6.355e-07, mini_mnist 8.062e-07
# (a tenth of the perturbation: d parameters average D >> d elements) and the tolerance is 4 x that, rounded up to a power of two.
# The host test re-measures and asserts the factor of four.
E2E_TOL = {"mini_mnist_small": 2.0 ** -17, "mini_cifar": 2.0 ** -18, "mini_mnist": 2.0 ** -18}


def scale_of(r, p):
    """1.4826 x the lower median of |r| over the elements with p > 0, per sample (NaN where there is none)."""
    out = []
    for rb, pb in zip(r.flatten(1), p.flatten(1)):
        a = rb[pb > 0].abs().sort().values
        out.append(MAD_TO_SIGMA * a[(len(a) - 1) // 2] if len(a) else torch.tensor(float("nan"), dtype=r.dtype))
    return torch.stack(out)


def weigh(r, p, loss, c, s):
    """(w = p omega(r / s), cost = 2 s^2 sum p rho(r / s) (B,), sum omega over p > 0 (B,)) with s (B,) broadcast over the elements."""
    sw = s.view(-1, *[1] * (r.dim() - 1))
    u = r / sw
    if loss == "huber":
        inside = u.abs() <= c
        om = torch.where(inside, torch.ones_like(u), c / u.abs())
        rho = torch.where(inside, u * u / 2, c * u.abs() - c * c / 2)
    else:
        t = (1 - (u / c) ** 2).clamp_min(0)
        om, rho = t * t, c * c / 6 * (1 - t ** 3)
    used = (p > 0).to(r.dtype)
    return p * om, 2 * s * s * (p * rho).flatten(1).sum(1), (used * om).flatten(1).sum(1)


def robust(model, y, p=None, loss="huber", tuning=None, scale=None, steps=10, rounds=1, z=None):
    """The loop; ``p``: the known weights (default all one); ``z``: the starting latent (default: the encoder's latent of y).
    ``costs``: (steps + 1, B), the last round's cost after every step."""
    c = TUNING[loss] if tuning is None else tuning
    z = model.encode(y) if z is None else z
    p = torch.ones_like(y) if p is None else p
    x_hat = model.decode(z)
    accepted = torch.zeros(len(z), dtype=torch.int32)
    wide = (len(z),) + (1,) * (x_hat.dim() - 1)
    for _ in range(rounds):
        s = scale_of(y - x_hat, p) if scale is None else scale
        w, cost, eff = weigh(y - x_hat, p, loss, c, s)
        c_0, costs = cost.clone(), [cost.clone()]
        lam = torch.full_like(cost, DAMPING)
        for _ in range(steps):
            _, delta, _, info = CR.evaluate(model, w, y, z, lam)
            solved = info == 0
            z_new = z + torch.where(solved[:, None], delta, torch.zeros_like(delta))
            x_new = model.decode(z_new)
            w_new, c_new, e_new = weigh(y - x_new, p, loss, c, s)
            ok = solved & (c_new < cost)
            z = torch.where(ok[:, None], z_new, z)
            x_hat = torch.where(ok.view(wide), x_new, x_hat)
            w = torch.where(ok.view(wide), w_new, w)
            cost, eff = torch.where(ok, c_new, cost), torch.where(ok, e_new, eff)
            lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
            accepted += ok
            costs.append(cost.clone())
    grad, _, tangential2, info = CR.evaluate(model, w, y, z, torch.zeros_like(lam))
    return {"latent": z, "reconstruction_head": x_hat, "cost": cost, "initial_cost": c_0, "tangential2": tangential2, "gradient": grad,
            "distance2": ((y - x_hat).flatten(1) ** 2).sum(1), "observed": (p > 0).flatten(1).sum(1).int(), "accepted": accepted,
            "damping": lam, "info": info, "weights": w, "scale": s, "effective": eff, "costs": torch.stack(costs)}


def problem(x_on, share, seed=0, data_rel=0.0):
    """The seeded outlier problem on points ``x_on`` (B, ...) of the manifold: per sample a seeded permutation picks ceil(share D)
    elements, each of which gets +-U(3, 6) ||x_on|| / sqrt(D) added; every element gets 0.01 ||x_on|| / sqrt(D) randn (plus
    ``data_rel`` ||x_on|| / sqrt(D) randn of a stream of its own).  Returns (y, planted (bool)) in x_on's dtype / shape, on the CPU."""
    gen = torch.Generator().manual_seed(2000 + seed)
    x64 = x_on.detach().cpu().double()
    B, D = x64.shape[0], x64[0].numel()
    planted = torch.zeros(B, D, dtype=torch.bool)
    for b in range(B):
        planted[b, torch.randperm(D, generator=gen)[:math.ceil(share * D)]] = True
    size = OUT_LOW + (OUT_HIGH - OUT_LOW) * torch.rand(B, D, dtype=torch.float64, generator=gen)
    sign = torch.where(torch.rand(B, D, dtype=torch.float64, generator=gen) < 0.5, -1.0, 1.0)
    noise = torch.randn(B, D, dtype=torch.float64, generator=gen)
    data_noise = torch.randn(B, D, dtype=torch.float64, generator=gen)
    unit = x64.flatten(1).norm(dim=1, keepdim=True) / math.sqrt(D)
    y = x64.flatten(1) + unit * (torch.where(planted, size * sign, torch.zeros_like(size)) + NOISE_REL * noise + data_rel * data_noise)
    return y.view_as(x64).to(x_on.dtype), planted.view_as(x64)


def conditions(rel_robust, rel_mask, rel_project, weights, planted, cost, initial_cost):
    """The conditions (a) - (d) of the known-answer tests as a dict of booleans: (a) the robust answer is within MASK_FACTOR x the
    distance ``complete`` reaches with the true mask, (b) ``project`` is at least PROJECT_FACTOR x farther, (c) every planted outlier
    has weight <= OUTLIER_WEIGHT and every other element >= GOOD_WEIGHT, (d) cost <= initial_cost.  The distances are relative
    ones to x_on (``_completion_reference.rel_distance``) and each side of (a) and (b) is its worst sample."""
    w, planted = weights.detach().cpu().double(), planted.cpu()
    return {"a": bool(rel_robust.max() <= MASK_FACTOR * rel_mask.max()), "b": bool(rel_project.max() >= PROJECT_FACTOR * rel_robust.max()),
            "c": bool((w[planted] <= OUTLIER_WEIGHT).all()) and bool((w[~planted] >= GOOD_WEIGHT).all()),
            "d": bool((cost <= initial_cost).all())}
