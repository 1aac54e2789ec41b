"""Principal geodesic analysis in float64 on the oracle: the metric G = J^T J of the fixtures' own models at given
latents, the log vectors of a relaxed star's arms and the dual K x K eigenproblem, all by plain torch.  The host tests establish on
it the conditions tests/test_gpu_tangent_pca.py asserts of the product (not a test module)."""
import torch

from _frechet_reference import reference_run                              # noqa: F401  (the stars the reference relaxes)
from _projection_reference import Model                                   # noqa: F401


def metric(model, z):
    """G (B, d, d) float64 at the latents z (B, d)."""
    return model.jacobian(z.double())[0]


def log_vectors(latents):
    """v_k = N (-3 z_{k,N} + 4 z_{k,N-1} - z_{k,N-2}) / 2 of the stars ``latents`` (B, K, P, d), in float64: what
    ``principal_latents`` forms, operation by operation."""
    z = latents.double()
    N = z.shape[2] - 1
    return N * (-3.0 * z[:, :, N] + 4.0 * z[:, :, N - 1] - z[:, :, N - 2]) / 2.0


def dual(G, V, w):
    """(M (B, K, K), its eigenvalues (B, K) descending) of M_kl = sqrt(w_k w_l) v_k^T G v_l / sum_k w_k."""
    sw = w.double().sqrt()
    M = (sw[:, :, None] * sw[:, None, :]) * (V @ G @ V.transpose(1, 2)) / w.double().sum(1)[:, None, None]
    return M, torch.linalg.eigvalsh(0.5 * (M + M.transpose(1, 2))).flip(1)


def analyse(model, star, w):
    """The analysis of a relaxed star of the reference (an output of ``_frechet_reference.mean``) with the weights w (B, K):
    ``variances`` (B, K) descending, ``norm2`` (B, K), ``total`` (B,), ``explained`` (B, K), ``rank`` (B,), ``metric``,
    ``log_velocities``."""
    V = log_vectors(star["latents"])
    G = metric(model, star["mean_latent"])
    d = G.shape[1]
    _, lam = dual(G, V, w)
    norm2 = torch.einsum("bki,bij,bkj->bk", V, G, V)
    total = (w * norm2).sum(1) / w.sum(1)
    rank = (lam > d * 2.0 ** -24 * lam[:, :1]).sum(1)
    return {"variances": lam, "norm2": norm2, "total": total, "explained": lam / total[:, None], "rank": rank, "metric": G,
            "log_velocities": V}
