"""The projection loop of ``cmf_amd.ManifoldProjector`` in float64 on the oracle: the same constants (lambda_0 =
1e-3, x 10 / x 0.1, clamps 1e-12 / 1e8), the same strict ``<`` acceptance and the same closing evaluation at lambda = 0, on the
fixtures' own models.  The host tests establish on it the conditions the GPU tests assert of the product."""
import torch

from conftest import golden_model, load_golden
from oracle import cmf_oracle as O

DAMPING, UP, DOWN, DAMPING_MIN, DAMPING_MAX = 1e-3, 10.0, 0.1, 1e-12, 1e8


class Model:
    """A fixture's model in float64: the head-space input of its own data, the encoder and the decoder with its Jacobian."""

    def __init__(self, name):
        self.g, meta = load_golden(name)
        _, _, _, ops, self.sd = golden_model(meta, torch.float64)
        self.pre, _, self.flow_ops, self.base, self.prior_ops = O.split_ops(ops)
        x = self.g["x"].double()
        if "noise" in self.g:                       # the input the fixture was computed at; no further noise is drawn
            x = x + self.g["noise"].double()
        self.y = O.prehead(self.pre, x, noise=torch.zeros_like(x))[0]

    def encode(self, y):
        return O.encode(self.sd, self.flow_ops, self.base, self.prior_ops, y)[0]

    def decode(self, z):
        return O.flow_forward(self.sd, self.flow_ops, self.base, z)

    def jacobian(self, z):
        """(G (B, d, d), x_hat, J (B, D, d))"""
        return O.jtj_batched(self.sd, self.flow_ops, self.base, z)


def sqdist(y, x_hat):
    return ((y - x_hat).flatten(1) ** 2).sum(1)


def evaluate(model, y, z, lam):
    """grad = J^T r, delta = (G + lam diag G)^-1 grad, grad^T delta and info (0, or 1 where the factorisation fails) at z."""
    G, x_hat, J = model.jacobian(z)
    r = (y - x_hat).flatten(1)
    grad = torch.bmm(J.transpose(1, 2), r[:, :, None])
    A = G + torch.diag_embed(lam[:, None] * torch.diagonal(G, dim1=1, dim2=2))
    L, info = torch.linalg.cholesky_ex(A)
    ok = info == 0
    eye = torch.eye(G.shape[1], dtype=G.dtype).expand_as(L)
    delta = torch.cholesky_solve(grad, torch.where(ok[:, None, None], L, eye))[:, :, 0]
    grad = grad[:, :, 0]
    nan = torch.full_like(delta, float("nan"))
    delta = torch.where(ok[:, None], delta, nan)
    return grad, delta, (grad * delta).sum(1), (~ok).int()


def project(model, y, steps=10, z=None):
    """The loop; ``z``: the starting latent (default: the encoder's)."""
    z = model.encode(y) if z is None else z
    x_hat = model.decode(z)
    d2 = sqdist(y, x_hat)
    d2_0 = d2.clone()
    lam = torch.full_like(d2, DAMPING)
    accepted = torch.zeros(len(z), dtype=torch.int32)
    wide = (len(z),) + (1,) * (x_hat.dim() - 1)
    for _ in range(steps):
        _, delta, _, info = evaluate(model, y, z, lam)
        solved = info == 0
        z_new = z + torch.where(solved[:, None], delta, torch.zeros_like(delta))
        x_new = model.decode(z_new)
        d2_new = sqdist(y, x_new)
        ok = solved & (d2_new < d2)
        z = torch.where(ok[:, None], z_new, z)
        x_hat = torch.where(ok.view(wide), x_new, x_hat)
        d2 = torch.where(ok, d2_new, d2)
        lam = torch.where(ok, (lam * DOWN).clamp_min(DAMPING_MIN), (lam * UP).clamp_max(DAMPING_MAX))
        accepted += ok
    grad, _, tangential2, info = evaluate(model, y, z, torch.zeros_like(lam))
    return {"latent": z, "reconstruction_head": x_hat, "distance2": d2, "initial_distance2": d2_0, "tangential2": tangential2,
            "gradient": grad, "accepted": accepted, "damping": lam, "info": info}


def tangential_share(out):
    """max over the batch of tangential2 / distance2 (0 where the distance is exactly zero: nothing is left to remove)."""
    d2 = out["distance2"]
    share = torch.where(d2 > 0, out["tangential2"] / torch.where(d2 > 0, d2, torch.ones_like(d2)), torch.zeros_like(d2))
    return float(share.max())


def normal_offset(x_on, J, seed, rel=0.1):
    """The known-answer input: y = x_on + eps n with n a unit normal to range(J) (n = w - J G^-1 J^T w of a seeded w, normalised)
    and eps = rel ||x_on||_2, all in float64.  Returns (y shaped like x_on, eps (B,))."""
    B, D, d = J.shape
    J = J.double()
    w = torch.randn(B, D, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    G = torch.bmm(J.transpose(1, 2), J)
    n = w - torch.bmm(J, torch.linalg.solve(G, torch.bmm(J.transpose(1, 2), w)))
    n = n - torch.bmm(J, torch.linalg.solve(G, torch.bmm(J.transpose(1, 2), n)))      # once more: J^T n = 0 to rounding
    n = n[:, :, 0] / n[:, :, 0].norm(dim=1, keepdim=True)
    eps = rel * x_on.double().flatten(1).norm(dim=1)
    return x_on.double() + (eps[:, None] * n).view_as(x_on), eps
