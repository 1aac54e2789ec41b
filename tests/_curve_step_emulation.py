"""A plain numpy float64 emulation of the curve step kernel (csrc/curve_step.hip) on one curve: the same inputs
(float32 J, lower triangles of the float32 jtj, float32 cross blocks and xhat, float64 lambda), the same block elimination -- the d
columns of block i eliminated on the window [S_i, . ; -C_i^T, 2 G_{i+1} (1 + lambda on the diagonal)] with the g entries of both
blocks as an extra row, multipliers by division -- the same back substitution and the same outputs.  Sums that the kernel folds by
trees are plain numpy sums here: the two agree to rounding, not bit for bit.  Also the seeded inputs the host and GPU tests share,
the dense assembly of the system and the error ratios their bounds are stated in."""
import numpy as np

U = 2.0 ** -53
NAN = float("nan")
#: the kernel's residual bound is BOUND_C d 2^-53 (||A|| ||delta|| + ||g||): the projector's 32 with the band's doubled elimination
#: depth; the emulation is held to a quarter of it
BOUND_C = 64.0

WIDTHS = [1, 3, 16, 17, 64, 65, 100, 128]
ROWS = [5, 64, 784]
POINTS = [3, 4, 9]
DAMPINGS = [0.0, 1e-3, 10.0]


def energy(xhat, P):
    """Energy-only mode on one curve: xhat (P, D) float32 -> (seg2 (P - 1,), their sum, info)."""
    x = np.asarray(xhat)
    if not np.isfinite(x).all():
        return np.full(P - 1, NAN), NAN, 2
    r = x[1:].astype(np.float64) - x[:-1].astype(np.float64)
    seg2 = (r * r).sum(1)
    total = 0.0
    for s in seg2:
        total += float(s)
    return seg2, total, 0


def damped_block(G, lam):
    """The lower triangle of 2 G with the diagonal scaled by 1 + lambda, as the kernel loads it (zeros above)."""
    B = 2.0 * np.tril(np.asarray(G, dtype=np.float64))
    k = np.arange(len(B))
    B[k, k] = B[k, k] + lam * B[k, k]
    return B


def eliminate(W, d, nw):
    """The d columns of the leading block of the window W ((nw + 1) x nw, lower triangle and the extra row), in place.
    Returns False at a pivot that is not positive and finite."""
    for k in range(d):
        piv = W[k, k]
        if not piv > 0.0 or not piv < 1.0e300:
            return False
        col = W[k + 1:, k].copy()                   # rows k + 1 .. nw; the last one is the extra row
        mult = col / piv
        upd = np.outer(mult, col[:nw - k - 1])      # W_rj -= (W_rk / p_k) W_jk for k < j <= min(r, nw - 1)
        keep = np.tril(np.ones((nw - k, nw - k - 1), dtype=bool))
        keep[-1, :] = True
        W[k + 1:, k + 1:] -= np.where(keep, upd, 0.0)
    return True


def step(J, G, C, xhat, lam):
    """One curve of P points.  J (P, D, d) float32, G (P, d, d) float32 (lower triangles of the interior points read), C
    (P - 3, d, d) float32, xhat (P, D) float32.  Returns (grad (M, d), delta (M, d), stats (4,), seg2 (N,), info)."""
    P, D, d = J.shape
    M = P - 2
    seg2, total, info = energy(xhat, P)
    low = np.tril(np.ones((d, d), dtype=bool))
    bad = info != 0 or not np.isfinite(J[1:-1]).all() or not np.isfinite(np.asarray(G)[1:-1][:, low]).all() \
        or not np.isfinite(np.asarray(C)).all()
    if bad:
        return np.full((M, d), NAN), np.full((M, d), NAN), np.full(4, NAN), np.full(P - 1, NAN), 2
    x = np.asarray(xhat, dtype=np.float64)
    s = (x[:-2] + x[2:]) - 2.0 * x[1:-1]
    g = np.einsum("irk,ir->ik", J[1:-1].astype(np.float64), s)
    stats = np.array([total, NAN, NAN, float(np.abs(g).max())])
    saved = []
    top, gtop = damped_block(G[1], lam), g[0].copy()
    for i in range(1, M + 1):
        last = i == M
        nw = d if last else 2 * d
        W = np.zeros((nw + 1, nw))
        W[:d, :d] = top
        W[nw, :d] = gtop
        if not last:
            W[d:2 * d, :d] = -np.asarray(C[i - 1], dtype=np.float64).T
            W[d:2 * d, d:] = damped_block(G[i + 1], lam)
            W[nw, d:] = g[i]
        if not eliminate(W, d, nw):
            return g, np.full((M, d), NAN), stats, seg2, 1
        saved.append((W[:d, :d].copy(), None if last else W[d:2 * d, :d].copy(), W[nw, :d].copy()))
        if not last:
            top, gtop = W[d:2 * d, d:].copy(), W[nw, d:].copy()
    delta = np.zeros((M, d))
    for i in range(M, 0, -1):
        tri, below, w = saved[i - 1]
        w = w.copy()
        if below is not None:
            acc = np.zeros(d)
            for r in range(d):
                acc += below[r] * delta[i][r]
            w = w - acc
        for a in range(d - 1, -1, -1):
            delta[i - 1, a] = w[a] / tri[a, a]
            w[:a] -= tri[a, :a] * delta[i - 1, a]
    stats[1] = float((g * delta).sum())
    q = 0.0
    for i in range(1, M + 1):
        terms = np.tril(np.asarray(G[i], dtype=np.float64)) * np.outer(delta[i - 1], delta[i - 1])
        q += 2.0 * np.diag(terms).sum() + 4.0 * np.tril(terms, -1).sum()
        if i < M:
            q -= 2.0 * (np.asarray(C[i - 1], dtype=np.float64) * np.outer(delta[i - 1], delta[i])).sum()
    stats[2] = float(q)
    return g, delta, stats, seg2, 0


def batch(J, G, C, xhat, lam, P):
    """``step`` over curve-major curves: J (curves P, D, d), G (curves P, d, d), C (curves, P - 3, d, d), xhat (curves P, D),
    lam (curves,) -> stacked outputs."""
    curves = len(xhat) // P
    out = [step(J[c * P:(c + 1) * P], G[c * P:(c + 1) * P], C[c], xhat[c * P:(c + 1) * P], lam[c]) for c in range(curves)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4)) + (np.array([o[4] for o in out], dtype=np.int32),)


def cross_of(J, P):
    """float64 cross-Gram blocks of curve-major J (curves P, D, d): (curves, P - 3, d, d)."""
    B, D, d = J.shape
    J64 = J.astype(np.float64).reshape(B // P, P, D, d)
    return np.einsum("cira,cirb->ciab", J64[:, 1:P - 2], J64[:, 2:P - 1])


def inputs(curves, P, D, d, seed=0):
    """Seeded float32 inputs: J (curves P, D, d) = randn with the columns scaled over 1e-2 .. 1e2 (log-spaced, shuffled), its Gram
    and cross-Gram matrices rounded to float32 from the float64 products, xhat a noisy straight line per curve."""
    rng = np.random.default_rng(1000003 * d + 1009 * D + 31 * P + curves + seed)
    scale = 10.0 ** np.linspace(-2.0, 2.0, d) if d > 1 else np.ones(1)
    rng.shuffle(scale)
    B = curves * P
    J = (rng.standard_normal((B, D, d)) * scale).astype(np.float32)
    J64 = J.astype(np.float64)
    G = (J64.transpose(0, 2, 1) @ J64).astype(np.float32)
    C = cross_of(J, P).astype(np.float32)
    a, b = rng.standard_normal((curves, 1, D)), rng.standard_normal((curves, 1, D))
    tt = np.linspace(0.0, 1.0, P)[None, :, None]
    xhat = (a + tt * b + 0.1 * rng.standard_normal((curves, P, D))).reshape(B, D).astype(np.float32)
    return J, G, C, xhat


def dense(G, C, lam):
    """(A, H) of one curve as dense (M d, M d) float64 matrices from the float32 inputs the kernel reads: G (P, d, d) (lower
    triangles symmetrised), C (P - 3, d, d)."""
    P, d = G.shape[0], G.shape[1]
    M = P - 2
    H = np.zeros((M * d, M * d))
    for i in range(1, M + 1):
        G64 = np.asarray(G[i], dtype=np.float64)
        S = np.tril(G64) + np.tril(G64, -1).T
        o = (i - 1) * d
        H[o:o + d, o:o + d] = 2.0 * S
        if i < M:
            C64 = np.asarray(C[i - 1], dtype=np.float64)
            H[o:o + d, o + d:o + 2 * d] = -C64
            H[o + d:o + 2 * d, o:o + d] = -C64.T
    A = H.copy()
    k = np.arange(M * d)
    A[k, k] = H[k, k] + lam * H[k, k]
    return A, H


def residual_ratio(A, d, g, delta):
    """||A delta - g||_inf / (d 2^-53 (||A||_inf ||delta||_inf + ||g||_inf)): to be held against BOUND_C (or a quarter of it)."""
    g, delta = g.reshape(-1), delta.reshape(-1)
    scale = d * U * (np.abs(A).sum(1).max() * np.abs(delta).max() + np.abs(g).max())
    return float(np.abs(A @ delta - g).max() / scale) if scale > 0 else 0.0
