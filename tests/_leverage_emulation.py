"""A plain numpy emulation of the leverage kernel (csrc/leverage.hip) on one sample, in the kernel's own order: the
float64 copy of the lower triangle of a float32 normal matrix, Cholesky without square roots column by column (pivots p_k on the
diagonal, the multipliers a division), the columns divided by their pivots, the unit-lower factor inverted in place from the right
(W = L^-1), cov_ij = sum_{k >= i} W_ki W_kj / p_k and lev_i = sum_k y_k^2 / p_k with y = W j_i.  Sums that the kernel folds by trees
or fuses into multiply-adds are plain numpy sums here: the two agree to rounding, not bit for bit.

Beside it the reference the bounds are stated against -- the same algebra in ``numpy.longdouble`` (64-bit significand on x86: 2^-11
of float64's unit roundoff; mpmath is not assumed) --, the error ratios, the constants C_COV and C_LEV with the measured values they
come from, and the planted defects the bounds must catch."""
import math

import numpy as np
import torch

import _gn_step_emulation as GN

U = 2.0 ** -53
NAN = float("nan")
WIDTHS, ROWS, BATCH = GN.WIDTHS, GN.ROWS, 3

#: ||G C - I||_max <= C_COV d u || |G| |C| ||_max.  Measured over the well-posed shapes of ``cases()``: the emulation's worst ratio
#: is 2^-0.37 (d = 1, where d u is a single rounding); 4 x that, rounded up to a power of two.
C_COV = 4.0
#: |lev_i - lev_ref,i| <= C_LEV d u kappa_s lev_ref,i with kappa_s the 2-norm condition number of the unit-diagonal scaling of G.
#: Measured: the emulation's worst ratio is 2^0.78 (d = 1 again; 2^-1.09 and below for d >= 3); 4 x that, rounded up to a power of two.
C_LEV = 8.0
DEFECTS = ("float32", "transposed", "no_division")


def pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(v)))


def symmetric(G, dtype=np.float64):
    """The symmetric matrix the kernel reads: the lower triangle of the float32 G, mirrored."""
    L = np.tril(np.asarray(G)).astype(dtype)
    return L + np.tril(L, -1).T


def eliminate(A):
    """Cholesky without square roots on the lower triangle of A (overwritten), in A's dtype: the pivots on the diagonal, column k
    holding the unscaled multipliers.  Returns False at the first pivot that is not positive and below 1e300."""
    d = len(A)
    for k in range(d):
        piv = A[k, k]
        if not float(piv) > 0.0 or not float(piv) < 1.0e300:
            return False
        col = A[k + 1:, k].copy()
        mult = col / piv                            # a division: a duplicate column cancels its pivot exactly
        A[k + 1:, k + 1:] -= np.tril(np.outer(mult, col))
    return True


def unit_lower_inverse(A):
    """From the eliminated A to W = L^-1 below the diagonal (the diagonal keeps the pivots), columns right to left."""
    d = len(A)
    p = np.diag(A).copy()
    A[:] = np.tril(A, -1) / p[None, :] + np.diag(p)
    for j in range(d - 2, -1, -1):
        x = A[j + 1:, j].copy()
        W = np.tril(A[j + 1:, j + 1:], -1) + np.eye(d - j - 1, dtype=A.dtype)
        A[j + 1:, j] = -(W @ x)
    return p


def leverage(J, G, defect=None, dtype=np.float64):
    """One sample.  J (D, d) float32 or None (covariance only), G (d, d) float32 (lower triangle read).  Returns (cov (d, d), lev
    (D,) or None, stats (2,) or None, info).  ``defect``: one of DEFECTS, planted; ``dtype``: numpy.longdouble gives the reference."""
    d = G.shape[0]
    low = np.tril(np.ones((d, d), dtype=bool))
    n = None if J is None else len(J)
    nans = lambda: (np.full((d, d), NAN), None if J is None else np.full(n, NAN), None if J is None else np.full(2, NAN))
    if not np.isfinite(np.asarray(G)[low]).all() or (J is not None and not np.isfinite(J).all()):
        return (*nans(), 2)
    A = np.tril(np.asarray(G)).astype(np.float32 if defect == "float32" else dtype)
    if not eliminate(A):
        return (*nans(), 1)
    A = A.astype(dtype)
    p = unit_lower_inverse(A)
    W = np.tril(A, -1) + np.eye(d, dtype=dtype)
    if defect == "transposed":
        W = W.T.copy()
    q = np.ones(d, dtype=dtype) if defect == "no_division" else 1.0 / p
    cov = (W * q[:, None]).T @ W
    cov = np.tril(cov) + np.tril(cov, -1).T         # (j, i) is written from (i, j)
    if J is None:
        return cov, None, None, 0
    Y = J.astype(dtype) @ W.T
    lev = (Y * Y * q[None, :]).sum(1)
    return cov, lev, np.array([lev.sum(), lev.max()]), 0


def reference(J, G):
    """``leverage`` in numpy.longdouble: what the bounds are stated against."""
    return leverage(J, G, dtype=np.longdouble)


def kappa_s(G):
    """The 2-norm condition number of the unit-diagonal scaling D^-1/2 G D^-1/2 of the symmetric matrix the kernel reads."""
    S = symmetric(G)
    s = 1.0 / np.sqrt(np.diag(S))
    return float(np.linalg.cond(S * s[:, None] * s[None, :]))


def cov_ratio(G, cov):
    """||G C - I||_max / (d u || |G| |C| ||_max), in longdouble."""
    S, C = symmetric(G, np.longdouble), np.asarray(cov, dtype=np.longdouble)
    d = len(S)
    return float(np.abs(S @ C - np.eye(d)).max() / (d * U * (np.abs(S) @ np.abs(C)).max()))


def lev_ratio(G, lev, lev_ref):
    """max_i |lev_i - lev_ref,i| / (d u kappa_s lev_ref,i), in longdouble (rows with lev_ref == 0 must be matched exactly)."""
    ref = np.asarray(lev_ref, dtype=np.longdouble)
    err = np.abs(np.asarray(lev, dtype=np.longdouble) - ref)
    scale = len(G) * U * kappa_s(G) * ref
    if (err[scale == 0] > 0).any():
        return np.inf
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def trace_bound(J, G, cov_ref, lev_ref):
    """The bound on |sum_i lev_i - d| for G = float32(J^T J) of the same J: the per-row bounds, plus what the float32 rounding of G
    moves the exact trace tr(G32^-1 J^T J) = d + tr(G32^-1 (J^T J - G32)) by, <= sum_ij |C_ij| |(J^T J - G32)_ij|."""
    J64 = J.astype(np.longdouble)
    rounding = float((np.abs(np.asarray(cov_ref)) * np.abs(J64.T @ J64 - symmetric(G, np.longdouble))).sum())
    return float(C_LEV * len(G) * U * kappa_s(G) * np.asarray(lev_ref, dtype=np.float64).sum()) + rounding


def cases():
    """(d, D) of the bound tests: every width against every row count; with D < d the Gram matrix is singular and only the info code
    is looked at (``well_posed``)."""
    return [(d, D) for d in WIDTHS for D in ROWS]


def well_posed(d, D):
    return D >= d


def inputs(D, d, B=BATCH, seed=0):
    """(J (B, D, d), G (B, d, d)) float32 of ``_gn_step_emulation.inputs``: column scales over 1e-2 .. 1e2, G = float32(J^T J)."""
    J, G, _, _ = GN.inputs(B, D, d, seed=seed)
    return J, G


# --------------------------------------------------------------------------------------------------
# ManifoldProjector.uncertainty in float64 torch, and what the host and GPU tests share of its tolerance
# --------------------------------------------------------------------------------------------------

#: the relative size DESIGN 5 and tests/test_gpu_parity.py hold the product's Jacobian and Gram matrix to
JACOBIAN_REL = 1e-5
#: the fixtures and the calls ``uncertainty`` is exercised after; "data" is ``recover(space="data")`` on the image fixture alone
FIXTURES = ["c2b_hepmass", "c2a_power", "mini_mnist"]
PATHS = ["project", "complete", "recover"]
E2E_CASES = [(name, path) for name in FIXTURES for path in PATHS] + [("mini_mnist", "data")]
#: the size of the noise of the observed elements (complete) and of the measurements (recover), relative to ||.|| / sqrt(n) per
#: element: a cost well above rounding, so that cost / dof is a noise level and not a rounding residue
MEASUREMENT_REL = 1e-2
# End-to-end tolerance of tests/test_gpu_uncertainty.py on ``latent_std`` and ``reconstruction_std[_head]``, each in the max-norm
# relative to the reference's largest value of the sample.  The product's J and Gram matrix are the float64 ones within JACOBIAN_REL
# (DESIGN 5), so tests/test_uncertainty_host.py measures on the float64 reference how far a perturbation of its Jacobian of that size
# -- JACOBIAN_REL ||J|| / sqrt(D d) randn per entry, the normal matrix formed from the perturbed J -- moves the reference's own answer, worst sample and worst of the two quantities per case (printed there):
#   c2b_hepmass project 6.852e-06, complete 5.440e-03, recover 1.385e-05;  c2a_power project 1.323e-05, complete 3.402e-03, recover
#   2.069e-05;  mini_mnist project 1.554e-06, complete 3.887e-06, recover 6.315e-06, data 1.389e-05, project-data (``project``
#   qualified with space="data": ``reconstruction_std`` joins the comparison) 4.371e-06
# (the two tabular fixtures observe 11 of 21 and 3 of 6 elements for d = 10 and d = 2 in ``complete``: one degree of freedom and a
# poorly conditioned weighted Gram matrix, as tests/_completion_reference.py notes of its own tolerance)
# and the tolerance is 4 x that, rounded up to a power of two.  The host test re-measures and asserts the factor of four.
E2E_TOL = {("c2b_hepmass", "project"): 2.0 ** -15, ("c2b_hepmass", "complete"): 2.0 ** -5, ("c2b_hepmass", "recover"): 2.0 ** -14,
           ("c2a_power", "project"): 2.0 ** -14, ("c2a_power", "complete"): 2.0 ** -6, ("c2a_power", "recover"): 2.0 ** -13,
           ("mini_mnist", "project"): 2.0 ** -17, ("mini_mnist", "complete"): 2.0 ** -15, ("mini_mnist", "recover"): 2.0 ** -15,
           ("mini_mnist", "data"): 2.0 ** -14, ("mini_mnist", "project-data"): 2.0 ** -15}


def uncertainty(J, cost=None, w=None, A=None, s=None, noise_std=None, jitter=None):
    """``ManifoldProjector.uncertainty`` from the float64 Jacobian J (B, D, d) at the latent: ``w`` (B, D) the weights of
    ``complete``, ``A`` (M, D) the operator of ``recover`` and ``s`` (B, D) the wrapper derivative du/dv of space="data"; ``cost``
    (B,) or ``noise_std``.  ``jitter``: dJ added to J before anything is formed from it (the sensitivity measurement)."""
    B, D, d = J.shape
    if jitter is not None:
        J = J + jitter
    if w is not None:
        N = torch.bmm(J.transpose(1, 2), w[:, :, None] * J)
        n_obs = (w > 0).sum(1)
    elif A is not None:
        K = torch.matmul(A, J if s is None else s[:, :, None] * J)
        N = torch.bmm(K.transpose(1, 2), K)
        n_obs = torch.full((B,), A.shape[0])
    else:
        N = torch.bmm(J.transpose(1, 2), J)
        n_obs = torch.full((B,), D)
    C = torch.linalg.inv(N)
    lev = torch.einsum("bik,bkl,bil->bi", J, C, J)
    dof = (n_obs - d).int()
    if noise_std is None:
        sigma2 = torch.where(dof > 0, cost / dof.clamp_min(1), torch.full_like(cost, NAN))
    else:
        sigma2 = torch.as_tensor(noise_std, dtype=torch.float64).expand(B) ** 2
    cov = sigma2[:, None, None] * C
    std_head = (sigma2[:, None] * lev).sqrt()
    out = {"latent_covariance": cov, "latent_std": torch.diagonal(cov, dim1=1, dim2=2).sqrt(), "leverage": lev,
           "reconstruction_std_head": std_head, "noise_variance": sigma2, "dof": dof, "normal": N}
    if s is not None:
        out["reconstruction_std"] = std_head * s.abs()
    return out


def jitter(J, seed=0, rel=JACOBIAN_REL):
    """dJ: ``rel`` ||J_b|| / sqrt(D d) randn per entry of J (the normal matrix follows from the perturbed J)."""
    gen = torch.Generator().manual_seed(7000 + seed)
    B, D, d = J.shape
    return rel * J.flatten(1).norm(dim=1)[:, None, None] / math.sqrt(D * d) * torch.randn(J.shape, dtype=torch.float64, generator=gen)


def rel_max(got, want):
    """max_i |got_i - want_i| / max_i |want_i| per sample, in float64 on the CPU."""
    a, b = got.detach().cpu().double().flatten(1), want.detach().cpu().double().flatten(1)
    return (a - b).abs().amax(1) / b.abs().amax(1)


def std_distance(got, want):
    """The quantity ``E2E_TOL`` bounds: the worst ``rel_max`` over ``latent_std`` and the reconstruction's standard deviations."""
    keys = [k for k in ("latent_std", "reconstruction_std_head", "reconstruction_std") if k in want]
    return torch.stack([rel_max(got[k], want[k]) for k in keys]).amax(0)
