"""The curvature pipeline of ``cmf_amd.ManifoldCurvature`` on the oracle, in float64 (or with the float32 oracle as the
decoder, the yardstick): the direction sweeps at the shifted latents, their central differences, and from them -- with ``torch.linalg``,
by projection and not by a Schur complement -- the Gram matrix N of the normal components, the Christoffel contractions, the Riemann
tensor, the sectional and scalar curvatures.  The "exact" second derivative is the float64 central difference at h = 2^-13 (its own
h = 2^-11 result agrees with it to <= 5.4e-7 of max |N| over all samples of the MLP fixtures).  The host tests establish on it the conditions the GPU
tests assert of the product."""
import torch

import _shoot_reference as R
from oracle import cmf_oracle as O

MLP = R.MLP
RELU = ["mini_mnist", "mini_cifar"]
EXACT_STEP = 2.0 ** -13
FRAME_SEED = 20
#: the frames of the ReLU fixtures: a seed at which the float64 reference gives asymmetry >= 0.5 on every sample, for m = 2 and m = 4
RELU_SEED = 23


def pairs(m):
    return [(a, b) for a in range(m) for b in range(a, m)]


def latents(name):
    """The float64 encoder's latents of the fixture's own inputs, rounded to float32: values every arithmetic can start from exactly."""
    model = R.model_of(name)
    with torch.no_grad():
        return model.encode(model.y).float()


def frames(B, d, m, seed=FRAME_SEED):
    """Seeded frames (B, d, m) float64 with unit columns."""
    f = torch.randn(B, d, m, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 100 * d + m))
    return f / f.norm(dim=1, keepdim=True)


def sweep(model, z, frame):
    """(x_hat, the columns J(z) u_c as (B, D, m)) in the model's dtype."""
    with torch.no_grad():
        x, jv = O.jvp_forward_multi(model.sd, model.flow_ops, model.base, z, frame.transpose(1, 2).to(z.dtype).contiguous())
    return x, jv.flatten(2).transpose(1, 2)


def mixed_differences(model, z32, frame, h, dtype=torch.float64):
    """D (B, m, m, D) float64: D[:, a, c] = (J(z + h u_a) u_c - J(z - h u_a) u_c) / (2 h), the sweeps in ``dtype`` at the latents
    (z.double() +- h u_a) rounded to ``dtype`` -- the product's own shifted latents when ``dtype`` is float32."""
    m = frame.shape[2]
    rows = []
    for a in range(m):
        plus = sweep(model, (z32.double() + h * frame[:, :, a]).to(dtype), frame)[1].double()
        minus = sweep(model, (z32.double() - h * frame[:, :, a]).to(dtype), frame)[1].double()
        rows.append(((plus - minus) / (2.0 * h)).transpose(1, 2))           # (B, m (c), D)
    return torch.stack(rows, 1)


def forms(J, Dm, frame):
    """From J (B, D, d) and the mixed differences Dm (B, m, m, D), in float64: a dict of ``H`` (B, D, q), ``second_gram`` = the Gram
    matrix of H - J G^-1 J^T H, ``christoffel`` (B, q, d), ``frame_metric``, ``riemann``, ``sectional``, ``scalar``,
    ``normal_curvature``, ``asymmetry``, ``trace_s2``."""
    J, Dm, frame = J.double(), Dm.double(), frame.double()
    m = Dm.shape[1]
    pr = pairs(m)
    H = torch.stack([0.5 * (Dm[:, a, b] + Dm[:, b, a]) for a, b in pr], 2)                  # (B, D, q)
    G = J.transpose(1, 2) @ J
    Gam = torch.linalg.solve(G, J.transpose(1, 2) @ H)                                      # (B, d, q)
    Hn = H - J @ Gam
    Hn = Hn - J @ torch.linalg.solve(G, J.transpose(1, 2) @ Hn)                             # once more: J^T Hn = 0 to rounding
    N = Hn.transpose(1, 2) @ Hn
    N = 0.5 * (N + N.transpose(1, 2))
    g = frame.transpose(1, 2) @ G @ frame
    idx = {p: i for i, p in enumerate(pr)}
    P = lambda a, b: idx[(min(a, b), max(a, b))]
    Rm = torch.zeros(J.shape[0], m, m, m, m, dtype=torch.float64)
    for a in range(m):
        for b in range(m):
            for c in range(m):
                for e in range(m):
                    Rm[:, a, b, c, e] = N[:, P(a, c), P(b, e)] - N[:, P(a, e), P(b, c)]
    K = torch.zeros(J.shape[0], m, m, dtype=torch.float64)
    for a in range(m):
        for b in range(m):
            if a != b:
                K[:, a, b] = Rm[:, a, b, a, b] / (g[:, a, a] * g[:, b, b] - g[:, a, b] ** 2)
    ginv = torch.linalg.inv(g)
    scalar = torch.einsum("nac,nbd,nabcd->n", ginv, ginv, Rm)
    normal = torch.stack([N[:, P(a, a), P(a, a)].clamp_min(0).sqrt() / g[:, a, a] for a in range(m)], 1)
    up = [(a, b) for a in range(m) for b in range(a + 1, m)]
    if up:
        anti = sum(((Dm[:, a, b] - Dm[:, b, a]) ** 2).sum(1) for a, b in up)
        symm = sum((H[:, :, P(a, b)] ** 2).sum(1) for a, b in up)
        asym = torch.where(symm > 0, (anti / symm.clamp_min(1e-300)).sqrt(), torch.zeros_like(symm))
    else:
        asym = torch.zeros(J.shape[0], dtype=torch.float64)
    return {"H": H, "second_gram": N, "christoffel": Gam.transpose(1, 2).contiguous(), "frame_metric": g, "riemann": Rm,
            "sectional": K, "scalar": scalar, "normal_curvature": normal, "asymmetry": asym,
            "trace_s2": torch.diagonal(H.transpose(1, 2) @ H, dim1=1, dim2=2).sum(1)}


_RUNS = {}


def run(name, m, h, dtype=torch.float64, samples=None, seed=FRAME_SEED):
    """(z (B, d) float32, frame (B, d, m) float64, ``forms`` of the fixture at step ``h`` with the sweeps in ``dtype``), computed once."""
    key = (name, m, h, dtype, samples, seed)
    if key not in _RUNS:
        z = latents(name)
        if samples is not None:
            z = z[list(samples)]
        frame = frames(z.shape[0], z.shape[1], m, seed)
        model = R.model_of(name, dtype)
        J = sweep(model, z.to(dtype), torch.eye(z.shape[1], dtype=torch.float64).expand(z.shape[0], -1, -1))[1]
        _RUNS[key] = (z, frame, forms(J, mixed_differences(model, z, frame, h, dtype), frame))
    return _RUNS[key]


def deviation(a, b):
    """max |a - b| / max |b|."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ---------------------------------------------------------------------------------------------------
# a known surface
# ---------------------------------------------------------------------------------------------------


def quadric(k1, k2, x, y):
    """Analytic J (1, 3, 2) and mixed derivatives (1, 2, 2, 3) of the graph x3 = (k1 x^2 + k2 y^2) / 2 at (x, y), in the axis frame, and
    its Gauss curvature k1 k2 / (1 + k1^2 x^2 + k2^2 y^2)^2."""
    J = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [k1 * x, k2 * y]]], dtype=torch.float64)
    Dm = torch.zeros(1, 2, 2, 3, dtype=torch.float64)
    Dm[0, 0, 0, 2], Dm[0, 1, 1, 2] = k1, k2
    return J, Dm, k1 * k2 / (1.0 + (k1 * x) ** 2 + (k2 * y) ** 2) ** 2
