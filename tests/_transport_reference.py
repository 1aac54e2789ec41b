"""Parallel transport of ``cmf_amd.ManifoldGeodesic.transport_latents`` on the oracle, in float64 (or float32, the
yardstick): along a curve z_0 .. z_{P-1} with J_i = J(z_i), G_i = J_i^T J_i and C_i = J_i^T J_{i+1}, per segment
    a = G_{i+1}^-1 C_i^T w_i,   b = C_i^-1 G_i w_i,   w_{i+1} = (a + b) / 2
by ``torch.linalg.solve``, and norm2_i = w_i^T G_i w_i.  The host tests establish on it the conditions the GPU tests assert of the
product."""
import torch

import _geodesic_reference as GR
import _shoot_reference as SR

MLP, FIXTURES = SR.MLP, SR.FIXTURES
STEPS = GR.STEPS


def transport(model, latents, w):
    """Along the curves ``latents`` (B, P, d) with the vectors ``w`` (B, d, m) at point 0, in the dtype of ``latents``: ``vectors``
    (B, P, d, m), ``forward`` and ``backward`` (B, N, d, m), ``norm2`` (B, P, m), ``transported`` = vectors[:, -1], and ``jacobian``
    (B, P, D, d)."""
    B, P, d = latents.shape
    with torch.no_grad():
        G, _, J = model.jacobian(latents.reshape(B * P, d))
    G, J = G.reshape(B, P, d, d), J.reshape(B, P, -1, d)
    w = w.to(latents.dtype)
    vectors, fwd, bwd = [w], [], []
    for i in range(P - 1):
        C = J[:, i].transpose(1, 2) @ J[:, i + 1]
        a = torch.linalg.solve(G[:, i + 1], C.transpose(1, 2) @ w)
        b = torch.linalg.solve(C, G[:, i] @ w)
        w = 0.5 * (a + b)
        fwd.append(a)
        bwd.append(b)
        vectors.append(w)
    vectors = torch.stack(vectors, 1)
    norm2 = torch.einsum("bpim,bpij,bpjm->bpm", vectors, G, vectors)
    return {"vectors": vectors, "forward": torch.stack(fwd, 1), "backward": torch.stack(bwd, 1), "norm2": norm2,
            "transported": vectors[:, -1], "jacobian": J}


def project_only(model, latents, w):
    """The textbook first-order scheme w_{i+1} = G_{i+1}^-1 C_i^T w_i, for comparison: (vectors[:, -1], norm2 (B, P, m))."""
    B, P, d = latents.shape
    with torch.no_grad():
        G, _, J = model.jacobian(latents.reshape(B * P, d))
    G, J = G.reshape(B, P, d, d), J.reshape(B, P, -1, d)
    ws = [w]
    for i in range(P - 1):
        ws.append(torch.linalg.solve(G[:, i + 1], J[:, i + 1].transpose(1, 2) @ (J[:, i] @ ws[-1])))
    ws = torch.stack(ws, 1)
    return ws[:, -1], torch.einsum("bpim,bpij,bpjm->bpm", ws, G, ws)


def end_velocity(latents):
    """N (3 z_{P-1} - 4 z_{P-2} + z_{P-3}) / 2 of a curve (B, P, d): its latent velocity at the far end, second order."""
    z = latents.double()
    return (z.shape[1] - 1) * (3.0 * z[:, -1] - 4.0 * z[:, -2] + z[:, -3]) / 2.0


def start_vectors(latents, seed=11):
    """(B, d, 3) float64: the ``log`` velocity of the curve and two seeded normal vectors."""
    v = SR.log_velocity(latents)
    extra = torch.randn(v.shape[0], v.shape[1], 2, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return torch.cat([v[:, :, None], extra * v.abs().amax(1)[:, None, None]], 2)


_CURVES = {}


def relaxed(name, points):
    """(model, latents (B, P, d) float64): ``_geodesic_reference.connect`` with ``points`` points and 10 steps between the
    fixture's ends (``_shoot_reference.ends``), once; points = 9 is ``_shoot_reference.log_run``'s curve."""
    if (name, points) not in _CURVES:
        if points == GR.POINTS:
            model, _, _, out = SR.log_run(name)
        else:
            model, z0, z1 = SR.ends(name)
            with torch.no_grad():
                out = GR.connect(model, z0, z1, points=points, steps=STEPS)
        _CURVES[(name, points)] = (model, out["latents"])
    return _CURVES[(name, points)]


_RUNS = {}


def run(name, points):
    """(model, latents, w0, ``transport`` of ``start_vectors`` along ``relaxed(name, points)``), once."""
    if (name, points) not in _RUNS:
        model, z = relaxed(name, points)
        w0 = start_vectors(z)
        _RUNS[(name, points)] = (model, z, w0, transport(model, z, w0))
    return _RUNS[(name, points)]


def head_space(out):
    """The end vectors in the head's input space: J_{P-1} w_{P-1} (B, D, m)."""
    return out["jacobian"][:, -1] @ out["transported"]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def drift(out):
    """max |w_i^T G_i w_i / w_0^T G_0 w_0 - 1| over the points, the vectors and the curves."""
    n = out["norm2"]
    return float((n / n[:, :1] - 1.0).abs().max())


def forth_and_back(model, latents, w0, out=None):
    """Transport along the curve and back along the reversed curve: the relative (max-norm) error of what returns."""
    out = transport(model, latents, w0) if out is None else out
    back = transport(model, latents.flip(1), out["transported"])
    return rel(back["transported"], w0.to(latents.dtype))


def own_velocity_error(out, latents):
    """The transported first vector (the ``log`` velocity) against ``end_velocity``, relative in the head's input space."""
    J = out["jacobian"][:, -1].double()
    got = (J @ out["transported"][:, :, :1].double())[:, :, 0]
    want = (J @ end_velocity(latents)[:, :, None])[:, :, 0]
    return float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
