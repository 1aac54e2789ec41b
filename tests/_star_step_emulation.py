"""A plain numpy float64 emulation of the star step kernels (csrc/star_step.hip) on one star, built on the functions
of _curve_step_emulation.py: per arm the block elimination of the curve kernel with one more block -- after block M the window
holds [S_M, . ; -C_M^T, G_N (1 + lambda on the diagonal)] with g^c in the extra row, and eliminating block M leaves the arm's Schur
contribution T_k and its right-hand side r_k --, the centre's sums over the arms in arm order with its elimination, and the back
substitution with delta_centre as the block after block M.  Sums that the kernels fold by trees are plain numpy sums here: the two
agree to rounding, not bit for bit.  Also the seeded inputs the host and GPU tests share, the dense assembly of the
(K M + 1) d system and the join of a two-arm star into one curve.

Stack layout: star-major, then arm-major; point i of arm k of star s is sample (s K + k) P + i, point 0 the fixed end, point
N = P - 1 the arm's own copy of the centre.  C holds the blocks of all neighbouring samples of the stack: C[q] = J_q^T J_{q+1}."""
import numpy as np

import _curve_step_emulation as CE

U, NAN = CE.U, CE.NAN
#: the kernel's residual bound is BOUND_C d 2^-53 (||A|| ||delta|| + ||g||): the band's 64 (_curve_step_emulation.BOUND_C) is the
#: projector's 32 with doubled elimination depth; the centre adds a third level.  The emulation is held to a quarter of it.
BOUND_C = 96.0

WIDTHS = [1, 3, 16, 17, 64, 65, 100, 128]
ROWS = [5, 64, 784]
DAMPINGS = [0.0, 1e-3, 10.0]
ARMS = [1, 2, 3, 5]


def centre_block(G, lam):
    """The lower triangle of G with the diagonal scaled by 1 + lambda: the centre copy counts once (zeros above)."""
    B = 1.0 * np.tril(np.asarray(G, dtype=np.float64))
    k = np.arange(len(B))
    B[k, k] = B[k, k] + lam * B[k, k]
    return B


def arm_forward(J, G, C, xhat, lam):
    """One arm of P points: J (P, D, d), G (P, d, d), C (P - 1, d, d) with C[i] = J_i^T J_{i+1} (C[1 .. M] are read), xhat (P, D).
    Returns a dict: code (0, 1 failed pivot, 2 non-finite), seg2, total, g (M, d), gcen (d,) and, with code 0, T (d, d) lower
    triangle, r (d,) and the saved columns of every block."""
    P, D, d = J.shape
    M, N = P - 2, P - 1
    seg2, total, info = CE.energy(xhat, P)
    low = np.tril(np.ones((d, d), dtype=bool))
    if info != 0 or not np.isfinite(J[1:]).all() or not np.isfinite(np.asarray(G)[1:][:, low]).all() \
            or not np.isfinite(np.asarray(C)[1:M + 1]).all():
        return {"code": 2}
    x = np.asarray(xhat, dtype=np.float64)
    s = (x[:-2] + x[2:]) - 2.0 * x[1:-1]
    g = np.einsum("irk,ir->ik", J[1:-1].astype(np.float64), s)
    gcen = np.einsum("rk,r->k", J[N].astype(np.float64), x[M] - x[N])
    out = {"code": 1, "seg2": seg2, "total": total, "g": g, "gcen": gcen}
    saved = []
    top, gtop = CE.damped_block(G[1], lam), g[0].copy()
    for i in range(1, M + 1):
        W = np.zeros((2 * d + 1, 2 * d))
        W[:d, :d] = top
        W[2 * d, :d] = gtop
        W[d:2 * d, :d] = -np.asarray(C[i], dtype=np.float64).T
        W[d:2 * d, d:] = CE.damped_block(G[i + 1], lam) if i + 1 < N else centre_block(G[N], lam)
        W[2 * d, d:] = g[i] if i + 1 < N else gcen
        if not CE.eliminate(W, d, 2 * d):
            return out
        saved.append((W[:d, :d].copy(), W[d:2 * d, :d].copy(), W[2 * d, :d].copy()))
        top, gtop = W[d:2 * d, d:].copy(), W[2 * d, d:].copy()
    out.update(code=0, T=np.tril(top), r=gtop, saved=saved)
    return out


def centre(arms, w, d):
    """(delta_centre or None at a failed pivot): A_c = sum_k w_k T_k and rhs = sum_k w_k r_k in arm order, eliminated and
    back-substituted as the kernel does."""
    W = np.zeros((d + 1, d))
    for k, arm in enumerate(arms):
        W[:d] += w[k] * arm["T"]
        W[d] += w[k] * arm["r"]
    if not CE.eliminate(W, d, d):
        return None
    rhs, delta = W[d].copy(), np.zeros(d)
    for a in range(d - 1, -1, -1):
        delta[a] = rhs[a] / W[a, a]
        rhs[:a] -= W[a, :a] * delta[a]
    return delta


def arm_backward(arm, G, C, delta_c):
    """(delta (M, d), g^T delta, delta^T H delta) of one arm, with its centre terms."""
    M, d = arm["g"].shape
    N = M + 1
    delta = np.zeros((M + 2, d))                    # rows 1 .. M; row N the centre
    delta[N] = delta_c
    for i in range(M, 0, -1):
        tri, below, w = arm["saved"][i - 1]
        acc = np.zeros(d)
        for r in range(d):
            acc += below[r] * delta[i + 1][r]
        w = w - acc
        for a in range(d - 1, -1, -1):
            delta[i, a] = w[a] / tri[a, a]
            w[:a] -= tri[a, :a] * delta[i, a]
    gd = float(arm["gcen"] @ delta_c) + float((arm["g"] * delta[1:N]).sum())
    terms = np.tril(np.asarray(G[N], dtype=np.float64)) * np.outer(delta_c, delta_c)
    q = np.diag(terms).sum() + 2.0 * np.tril(terms, -1).sum()
    for i in range(M, 0, -1):
        terms = np.tril(np.asarray(G[i], dtype=np.float64)) * np.outer(delta[i], delta[i])
        q += 2.0 * np.diag(terms).sum() + 4.0 * np.tril(terms, -1).sum()
        q -= 2.0 * (np.asarray(C[i], dtype=np.float64) * np.outer(delta[i], delta[i + 1])).sum()
    return delta[1:N], gd, float(q)


def step(J, G, C, xhat, w, lam, P):
    """One star of K = len(w) arms.  J (K P, D, d) float32, G (K P, d, d) float32, C (>= K P - 1, d, d) float32 (block q between the
    samples q and q + 1 of the star), xhat (K P, D) float32, w (K,) float64.  Returns a dict of grad (K, M, d), grad_centre (d,),
    delta (K, M, d), delta_centre (d,), seg2 (K, N), stats (4,), info."""
    K, d = len(w), J.shape[2]
    M, N = P - 2, P - 1
    nan = lambda *shape: np.full(shape, NAN)
    bad = {"grad": nan(K, M, d), "grad_centre": nan(d), "delta": nan(K, M, d), "delta_centre": nan(d), "seg2": nan(K, N),
           "stats": nan(4), "info": 2}
    if not (np.isfinite(w).all() and (w > 0).all()):
        return bad
    sl = lambda k: slice(k * P, (k + 1) * P)
    arms = [arm_forward(J[sl(k)], G[sl(k)], C[k * P:k * P + N], xhat[sl(k)], lam) for k in range(K)]
    if any(arm["code"] == 2 for arm in arms):
        return bad
    gc = np.zeros(d)
    total = 0.0
    for k, arm in enumerate(arms):
        gc += w[k] * arm["gcen"]
        total += w[k] * arm["total"]
    grad = np.stack([w[k] * arm["g"] for k, arm in enumerate(arms)])
    gmax = max(float(np.abs(grad).max()), float(np.abs(gc).max()))
    out = {"grad": grad, "grad_centre": gc, "delta": nan(K, M, d), "delta_centre": nan(d),
           "seg2": np.stack([arm["seg2"] for arm in arms]), "stats": np.array([total, NAN, NAN, gmax]), "info": 1}
    if any(arm["code"] == 1 for arm in arms):
        return out
    delta_c = centre(arms, w, d)
    if delta_c is None:
        return out
    gd = q = 0.0
    for k, arm in enumerate(arms):
        out["delta"][k], gd_k, q_k = arm_backward(arm, G[sl(k)], C[k * P:k * P + N], delta_c)
        gd += w[k] * gd_k
        q += w[k] * q_k
    out["delta_centre"] = delta_c
    out["stats"][1:3] = gd, q
    out["info"] = 0
    return out


def batch(J, G, C, xhat, w, lam, P):
    """``step`` over the stars of a stack: w (stars, K), lam (stars,) -> a dict of stacked outputs."""
    stars, K = w.shape
    n = K * P
    outs = [step(J[s * n:(s + 1) * n], G[s * n:(s + 1) * n], C[s * n:], xhat[s * n:(s + 1) * n], w[s], lam[s], P) for s in range(stars)]
    return {key: np.stack([np.asarray(o[key]) for o in outs]) for key in outs[0]}


def cross_of(J):
    """float64 cross-Gram blocks of all neighbouring samples of the stack J (n, D, d): (n - 1, d, d)."""
    J64 = J.astype(np.float64)
    return np.einsum("qra,qrb->qab", J64[:-1], J64[1:])


def inputs(stars, K, P, D, d, seed=0):
    """Seeded float32 inputs (J, G, C, xhat) for ``stars`` stars of K arms of P points, from _curve_step_emulation.inputs with
    every arm a curve; the K centre copies of a star hold the same Jacobian and the same point (those of its arm 0)."""
    J, _, _, xhat = CE.inputs(stars * K, P, D, d, seed=seed + 7 * K)
    for s in range(stars):
        c0 = s * K * P + P - 1
        for k in range(1, K):
            J[c0 + k * P] = J[c0]
            xhat[c0 + k * P] = xhat[c0]
    J64 = J.astype(np.float64)
    G = (J64.transpose(0, 2, 1) @ J64).astype(np.float32)
    return J, G, cross_of(J).astype(np.float32), xhat


def dense(G, C, w, lam, P):
    """(A, H) of one star as dense ((K M + 1) d)^2 float64 matrices from the float32 inputs the kernels read (G: lower triangles
    symmetrised); unknowns: the interior points arm by arm, then the centre."""
    K, d = len(w), G.shape[1]
    M, N = P - 2, P - 1
    n = (K * M + 1) * d
    H = np.zeros((n, n))
    sym = lambda g: np.tril(np.asarray(g, dtype=np.float64)) + np.tril(np.asarray(g, dtype=np.float64), -1).T
    oc = K * M * d
    for k in range(K):
        for i in range(1, M + 1):
            o = (k * M + i - 1) * d
            H[o:o + d, o:o + d] = w[k] * 2.0 * sym(G[k * P + i])
            o2 = o + d if i < M else oc
            C64 = w[k] * np.asarray(C[k * P + i], dtype=np.float64)
            H[o:o + d, o2:o2 + d] = -C64
            H[o2:o2 + d, o:o + d] = -C64.T
        H[oc:, oc:] += w[k] * sym(G[k * P + N])
    A = H.copy()
    j = np.arange(n)
    A[j, j] = H[j, j] + lam * H[j, j]
    return A, H


def unknowns(arms, centre_row):
    """(K, M, d) and (d,) as the vector of ``dense``."""
    return np.concatenate([np.asarray(arms).reshape(-1), np.asarray(centre_row).reshape(-1)])


def joined(J, G, C, xhat, P):
    """A star of two arms as one curve of 2 P - 1 points: arm 0, the centre, arm 1 reversed.  Returns (J, G, C, xhat) as
    _curve_step_emulation.step takes them (C: the 2 P - 4 blocks of neighbouring interior points; float32 transposes are exact)."""
    N = P - 1
    order = list(range(P)) + [P + i for i in range(N - 1, -1, -1)]
    blocks = [C[i] for i in range(1, N)] + [C[P + i].T for i in range(N - 1, 0, -1)]
    return J[order], G[order], np.stack(blocks), xhat[order]
