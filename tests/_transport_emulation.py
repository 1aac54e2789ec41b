"""numpy emulation of ``cmf_transport_chain`` (csrc/transport_step.hip), operation by operation in float64 without
contraction: the same sums in the same order (G w with j ascending, C^T w with r ascending, norm2 with r ascending), the same
pivot rule (the largest |entry| of the column at or below the diagonal, the lowest row among equals, rows swapped), multipliers by
division, the same square-root-free elimination of the lower triangle with the right-hand sides as extra rows, the same two back
substitutions, and the same failure codes.  Also the data the kernel tests run on, so that the CPU tests hold the emulation to a
quarter of the kernel's bounds on the very inputs the GPU sees."""
import numpy as np

U = 2.0 ** -53
NAN = float("nan")
FWD_CONSTANT = 32.0        # ||G a - rhs||_inf <= FWD_CONSTANT d u (||G||_inf ||a||_inf + ||rhs||_inf): the projector's bound
BWD_CONSTANT = 64.0        # ||C b - rhs||_inf <= BWD_CONSTANT d u (||C||_inf ||b||_inf + ||rhs||_inf): the band solve's, doubled


def symmetric(Glow):
    """The float64 symmetric matrix of a float32 matrix whose lower triangle counts."""
    L = np.tril(np.asarray(Glow, dtype=np.float64))
    return L + np.tril(L, -1).T


def metric_product(G, w):
    """u[c] = G w[c], j ascending; w (m, d)."""
    u = np.zeros_like(w)
    for j in range(G.shape[0]):
        u = u + G[:, j][None, :] * w[:, j][:, None]
    return u


def cross_product(C, w):
    """rhs[c] = C^T w[c], r ascending."""
    s = np.zeros_like(w)
    for r in range(C.shape[0]):
        s = s + C[r][None, :] * w[:, r][:, None]
    return s


def form(w, u):
    s = np.zeros(w.shape[0])
    for r in range(w.shape[1]):
        s = s + w[:, r] * u[:, r]
    return s


def lu_solve(C, rhs):
    """C^-1 rhs[c] by the kernel's elimination on [C | rhs^T]; None where a pivot is zero or not finite."""
    d = C.shape[0]
    A = np.concatenate([C, rhs.T], axis=1).astype(np.float64)
    for k in range(d):
        col = np.abs(A[k:, k])
        col = np.where(np.isnan(col), -1.0, col)
        p = k + int(np.argmax(col))                       # the first maximum: the lowest row
        best = col[p - k]
        if not (best > 0.0) or not np.isfinite(best):
            return None
        if p != k:
            A[[k, p]] = A[[p, k]]
        piv = A[k, k]
        l = A[k + 1:, k] / piv
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - l[:, None] * A[k, k + 1:][None, :]
    x = np.zeros((rhs.shape[0], d))
    R = A[:, d:]
    for r in range(d - 1, -1, -1):
        x[:, r] = R[r] / A[r, r]
        R[:r] = R[:r] - A[:r, r][:, None] * x[:, r][None, :]
    return x


def chol_solve(G, rhs):
    """G^-1 rhs[c] by the square-root-free elimination of the lower triangle with the right-hand sides as extra rows; None where
    a pivot is not positive and finite."""
    d = G.shape[0]
    A = np.concatenate([np.tril(G), rhs], axis=0).astype(np.float64)
    for k in range(d):
        piv = A[k, k]
        if not (piv > 0.0) or not (piv < 1.0e300):
            return None
        l = A[k + 1:, k] / piv
        upd = l[:, None] * A[k + 1:d, k][None, :]         # row i, column j: A_ik / p_k * A_jk, for k < j <= min(i, d - 1)
        mask = np.arange(k + 1, A.shape[0])[:, None] >= np.arange(k + 1, d)[None, :]
        A[k + 1:, k + 1:d] = np.where(mask, A[k + 1:, k + 1:d] - upd, A[k + 1:, k + 1:d])
    x = np.zeros_like(rhs)
    Wr = A[d:]
    for r in range(d - 1, -1, -1):
        x[:, r] = Wr[:, r] / A[r, r]
        Wr[:, :r] = Wr[:, :r] - A[r, :r][None, :] * x[:, r][:, None]
    return x


def chain(jtj, cross, w0, points):
    """The kernel on numpy inputs: jtj (curves * P, d, d) float32, cross (curves * P - 1, d, d) float32, w0 (curves, m, d) float64
    -> (out (curves, P, m, d), fwd, bwd (curves, N, m, d), norm2 (curves, P, m), info (curves,) int32)."""
    P, N = points, points - 1
    curves, m, d = w0.shape
    out = np.full((curves, P, m, d), NAN)
    fwd, bwd = np.full((curves, N, m, d), NAN), np.full((curves, N, m, d), NAN)
    norm2, info = np.full((curves, P, m), NAN), np.zeros(curves, dtype=np.int32)
    low = np.tril(np.ones((d, d), dtype=bool))
    for c in range(curves):
        G32, C32 = jtj[c * P:(c + 1) * P], cross[c * P:c * P + N]
        if not (np.isfinite(G32[:, low]).all() and np.isfinite(C32).all() and np.isfinite(w0[c]).all()):
            info[c] = 2
            continue
        w = w0[c].astype(np.float64)
        out[c, 0] = w
        for i in range(P):
            G = symmetric(G32[i])
            u = metric_product(G, w)
            norm2[c, i] = form(w, u)
            if i == N:
                break
            C = C32[i].astype(np.float64)
            b = lu_solve(C, u)
            a = None if b is None else chol_solve(symmetric(G32[i + 1]), cross_product(C, w))
            if a is None:
                info[c] = 1
                break
            fwd[c, i], bwd[c, i] = a, b
            w = 0.5 * (a + b)
            out[c, i + 1] = w
    return out, fwd, bwd, norm2, info


# ---------------------------------------------------------------------------------------------------
# the bounds, per segment, on the kernel's own w_i
# ---------------------------------------------------------------------------------------------------


def inf_norm(M):
    return np.abs(M).sum(-1).max(-1)


def residual_ratios(jtj, cross, out, fwd, bwd, norm2, points):
    """(forward, backward, norm2): the largest residual over d u (||M||_inf ||x||_inf + ||rhs||_inf) of the two halves, with the
    right-hand sides formed in float64 from the float32 inputs and the w_i of ``out``, and the largest |norm2 - recomputed| over
    u sum |terms|.  Curves whose ``norm2`` is NaN are skipped where they are NaN."""
    P, N = points, points - 1
    curves, _, m, d = out.shape
    worst = [0.0, 0.0, 0.0]
    for c in range(curves):
        for i in range(P):
            w = out[c, i]
            if not np.isfinite(w).all():
                continue
            G = symmetric(jtj[c * P + i])
            terms = w[:, :, None] * G[None] * w[:, None, :]
            worst[2] = max(worst[2], float((np.abs(norm2[c, i] - terms.sum((1, 2))) / (U * np.abs(terms).sum((1, 2)))).max()))
            if i == N or not np.isfinite(fwd[c, i]).all():
                continue
            C, G1 = cross[c * P + i].astype(np.float64), symmetric(jtj[c * P + i + 1])
            rf, rb = w @ C, w @ G                                        # rows: C^T w, G w
            for k, (M, x, rhs) in enumerate(((G1, fwd[c, i], rf), (C, bwd[c, i], rb))):
                res = np.abs(x @ M.T - rhs).max(1)
                scale = inf_norm(M) * np.abs(x).max(1) + np.abs(rhs).max(1)
                worst[k] = max(worst[k], float((res / (d * U * scale)).max()))
    return tuple(worst)


# ---------------------------------------------------------------------------------------------------
# the data of the kernel tests
# ---------------------------------------------------------------------------------------------------

WIDTHS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128]
POINTS = [2, 3, 5]
CURVES = [1, 3]
VECTORS = [1, 3, 16]


def jacobians(curves, P, d, seed=0, cond=1e3, turn=0.2):
    """Seeded float64 Jacobians (curves, P, D, d) with D = d + 3 and cond(G) ~ ``cond``: J_0 = Q diag(s) V^T, and every next point
    adds a fresh matrix of about 2 ``turn`` times the smallest singular value, so that neighbouring tangent planes differ by
    moderate angles and the condition number stays."""
    rng = np.random.default_rng(100000 * d + 1000 * P + 10 * curves + seed)
    D = d + 3
    s = np.sqrt(np.logspace(0, -np.log10(cond), d)) if d > 1 else np.ones(1)

    def one():
        Q = np.linalg.qr(rng.standard_normal((D, d)))[0]
        V = np.linalg.qr(rng.standard_normal((d, d)))[0]
        return (Q * s) @ V.T

    J = np.zeros((curves, P, D, d))
    for c in range(curves):
        scale = 2.0 ** rng.integers(-3, 4)
        J[c, 0] = one() * scale
        for i in range(1, P):                             # a perturbation of spectral norm ~ 2 turn s_min
            J[c, i] = J[c, i - 1] + (turn * s[-1] * scale / np.sqrt(D)) * rng.standard_normal((D, d))
    return J


def blocks(J):
    """(jtj (curves * P, d, d) float32 with NaN in every strict upper triangle, cross (curves * P - 1, d, d) float32 with NaN in the
    blocks that straddle two curves) of float64 Jacobians (curves, P, D, d), rounded to float32."""
    curves, P, D, d = J.shape
    S = J.reshape(curves * P, D, d)
    jtj = np.einsum("sra,srb->sab", S, S).astype(np.float32)
    cross = np.einsum("sra,srb->sab", S[:-1], S[1:]).astype(np.float32)
    jtj[:, ~np.tril(np.ones((d, d), dtype=bool))] = np.float32(NAN)
    for c in range(1, curves):
        cross[c * P - 1] = np.float32(NAN)
    return jtj, cross


def vectors(curves, m, d, seed=0):
    return np.random.default_rng(7000 * d + 10 * m + curves + seed).standard_normal((curves, m, d))


def case(curves, P, d, m, seed=0):
    jtj, cross = blocks(jacobians(curves, P, d, seed))
    return jtj, cross, vectors(curves, m, d, seed)


# ---------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------


def unimodular(rng, d):
    """An integer matrix of determinant +-1 and its integer inverse: a permutation times up to three unit shears."""
    R, Ri = np.eye(d), np.eye(d)
    perm = rng.permutation(d)
    R, Ri = R[:, perm], Ri[perm, :]
    for _ in range(min(d, 3)):
        a, b = rng.integers(0, d, 2)
        if a != b:
            S, Si = np.eye(d), np.eye(d)
            S[a, b], Si[a, b] = 1.0, -1.0
            R, Ri = R @ S, Si @ Ri
    return R, Ri


def same_plane(d, P, seed=0):
    """Known answer (i): one curve whose points share the tangent plane, J_{i+1} = J_i R_i with small-integer J_0 (D = d + 3) and
    unimodular integer R_i -- G and C are integers that float32 holds exactly, and w_{i+1} = R_i^-1 w_i exactly.  Returns
    (J (1, P, D, d) float64, R^-1 (N, d, d), the float64 condition numbers (N, 2) of G_{i+1} and C_i in the infinity norm)."""
    for attempt in range(100):                            # the first seed whose J_0 has a modest condition number
        rng = np.random.default_rng(31 * d + 7 * P + seed + 1000 * attempt)
        J0 = rng.integers(-2, 3, (d + 3, d)).astype(np.float64)
        if np.linalg.matrix_rank(J0) == d and np.linalg.cond(J0.T @ J0) < 1e3:
            break
    J, inverses, conds = [J0], [], []
    for _ in range(P - 1):
        R, Ri = unimodular(rng, d)
        J.append(J[-1] @ R)
        inverses.append(Ri)
        G1, C = J[-1].T @ J[-1], J[-2].T @ J[-1]
        assert np.abs(G1).max() < 2 ** 24 and np.abs(C).max() < 2 ** 24
        conds.append([np.linalg.cond(G1, np.inf), np.linalg.cond(C, np.inf)])
    return np.stack(J)[None], np.stack(inverses), np.array(conds)


def pivoting_case(d=5):
    """Known answer (iii): two points, J_1 = J_0 Pi with Pi the swap of the first two latent coordinates and the first two columns
    of J_0 orthogonal, so that C_0 = G_0 Pi has an exact zero in its leading entry -- an elimination without pivoting stops there."""
    rng = np.random.default_rng(5)
    J0 = np.zeros((d + 3, d))
    J0[:3, 0], J0[:3, 1] = [1.0, 1.0, 0.0], [1.0, -1.0, 2.0]            # orthogonal; the other columns live in the other rows
    J0[3:, 2:] = rng.integers(-2, 3, (d, d - 2)) + 3.0 * np.eye(d, d - 2)
    assert np.linalg.matrix_rank(J0) == d
    Pi = np.eye(d)
    Pi[:, [0, 1]] = Pi[:, [1, 0]]
    return np.stack([J0, J0 @ Pi])[None], Pi[None]


def turned_planes(d, P, seed=0):
    """Known answer (ii): d two-dimensional ambient blocks, latent direction k turning in its own block by theta_k per segment:
    J_i = Q B_i V with B_i[2k : 2k + 2, k] = s_k (cos i theta_k, sin i theta_k), Q (2d x 2d) and V (d x d) orthogonal.  The
    principal angles between neighbouring planes are theta_k, G_i = V^T S^2 V, C_i = V^T S^2 cos(Theta) V, and the vector
    w0 = V^T e_k keeps its block: norm2_{i+1} / norm2_i = ((cos theta_k + sec theta_k) / 2)^2.  Returns (J (1, P, 2d, d), w0
    (1, d, d) -- row k is V^T e_k --, the ratios (d,), kappa = the largest 2-norm condition number of a G_i or C_i)."""
    rng = np.random.default_rng(17 * d + P + seed)
    theta = rng.uniform(0.1, 0.5, d)
    s = rng.uniform(1.0, 2.0, d)
    Q = np.linalg.qr(rng.standard_normal((2 * d, 2 * d)))[0]
    V = np.linalg.qr(rng.standard_normal((d, d)))[0]
    J = np.zeros((1, P, 2 * d, d))
    for i in range(P):
        Bi = np.zeros((2 * d, d))
        for k in range(d):
            Bi[2 * k, k], Bi[2 * k + 1, k] = s[k] * np.cos(i * theta[k]), s[k] * np.sin(i * theta[k])
        J[0, i] = Q @ Bi @ V
    kappa = float((s ** 2).max() / (s ** 2 * np.cos(theta)).min())
    return J, V[None].copy(), ((np.cos(theta) + 1.0 / np.cos(theta)) / 2.0) ** 2, kappa
