"""A plain numpy float64 emulation of the Gauss-Newton step kernel (csrc/gn_step.hip) on one sample: the same
inputs (float32 J, lower triangle of a float32 G, float32 x and x_hat, float64 lambda), the same elimination -- Cholesky without
square roots on the lower triangle, column by column, with g carried as row d so that the forward substitution happens inside it --
the same back substitution and the same outputs.  Sums that the kernel folds by trees are plain numpy sums here: the two agree to
rounding, not bit for bit.  Also the seeded inputs the host and GPU tests share, and the error ratios their bounds are stated in."""
import numpy as np

U = 2.0 ** -53
NAN = float("nan")
#: the kernel's residual bound is BOUND_C d 2^-53 (||A|| ||delta|| + ||g||); the emulation is held to a quarter of it
BOUND_C = 32.0

WIDTHS = [1, 3, 16, 17, 64, 100, 128]
ROWS = [5, 64, 784]
DAMPINGS = [0.0, 1e-3, 10.0]


def step(J, G, x, xhat, lam):
    """One sample.  J (D, d) float32 or None (residual-only), G (d, d) float32 (lower triangle read), x, xhat (D,) float32.
    Returns (grad (d,), delta (d,), stats (4,), info); residual-only: (None, None, stats with only [0] set, info)."""
    x, xhat = np.asarray(x), np.asarray(xhat)
    r = x.astype(np.float64) - xhat.astype(np.float64)
    bad = not (np.isfinite(x).all() and np.isfinite(xhat).all())
    stats = np.full(4, NAN)
    if J is None:
        if not bad:
            stats[0] = float(r @ r)
        return None, None, stats, 2 if bad else 0
    d = J.shape[1]
    low = np.tril(np.ones((d, d), dtype=bool))
    if bad or not np.isfinite(J).all() or not np.isfinite(np.asarray(G)[low]).all():
        return np.full(d, NAN), np.full(d, NAN), stats, 2
    g = J.astype(np.float64).T @ r
    G64 = np.where(low, np.asarray(G, dtype=np.float64), 0.0)
    A = np.zeros((d + 1, d))
    A[:d] = G64
    A[d] = g
    k = np.arange(d)
    A[k, k] = A[k, k] + lam * A[k, k]
    stats[0], stats[3] = float(r @ r), float(np.abs(g).max())
    for k in range(d):
        piv = A[k, k]
        if not piv > 0.0 or not piv < 1.0e300:
            return g, np.full(d, NAN), stats, 1
        col = A[k + 1:, k].copy()                   # rows k + 1 .. d; the last one belongs to g
        mult = col / piv                            # a division: a duplicate column cancels its pivot exactly
        upd = np.outer(mult, col[:d - k - 1])       # A_ij -= (A_ik / p_k) A_jk for k < j <= min(i, d - 1)
        keep = np.tril(np.ones((d - k, d - k - 1), dtype=bool))
        keep[-1, :] = True
        A[k + 1:, k + 1:] -= np.where(keep, upd, 0.0)
    w = A[d].copy()
    delta = np.zeros(d)
    for i in range(d - 1, -1, -1):
        delta[i] = w[i] / A[i, i]
        w[:i] -= A[i, :i] * delta[i]
    stats[1] = float(g @ delta)
    terms = G64 * np.outer(delta, delta)
    stats[2] = float(np.diag(terms).sum() + 2.0 * np.tril(terms, -1).sum())
    return g, delta, stats, 0


def batch(J, G, x, xhat, lam):
    """``step`` over a batch: J (B, D, d) or None, G (B, d, d), x, xhat (B, D), lam (B,) -> stacked outputs."""
    B = len(x)
    out = [step(None if J is None else J[b], None if J is None else G[b], x[b], xhat[b], None if J is None else lam[b])
           for b in range(B)]
    if J is None:
        return None, None, np.stack([o[2] for o in out]), np.array([o[3] for o in out], dtype=np.int32)
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], dtype=np.int32))


def inputs(B, D, d, seed=0):
    """Seeded float32 inputs: J (B, D, d) = randn with the columns scaled over 1e-2 .. 1e2 (log-spaced, shuffled), its Gram
    matrix rounded to float32 from the float64 product, x and x_hat ~ randn."""
    rng = np.random.default_rng(100000 * d + 100 * D + B + seed)
    scale = 10.0 ** np.linspace(-2.0, 2.0, d) if d > 1 else np.ones(1)
    rng.shuffle(scale)
    J = (rng.standard_normal((B, D, d)) * scale).astype(np.float32)
    J64 = J.astype(np.float64)
    G = (J64.transpose(0, 2, 1) @ J64).astype(np.float32)
    x = rng.standard_normal((B, D)).astype(np.float32)
    xhat = (x + 0.1 * rng.standard_normal((B, D))).astype(np.float32)
    return J, G, x, xhat


def gram_by_dots(J):
    """float32(J^T J) of one sample, every entry by the same float64 dot-product routine: equal columns give bit-equal entries."""
    cols = [np.ascontiguousarray(J[:, k], dtype=np.float64) for k in range(J.shape[1])]
    return np.array([[np.dot(a, b) for b in cols] for a in cols]).astype(np.float32)


def damped(G, lam):
    """A = G + lam diag(G) in float64 from the lower triangle of the float32 G (symmetrised), as the kernel forms it."""
    G64 = np.asarray(G, dtype=np.float64)
    S = np.tril(G64) + np.tril(G64, -1).T
    dg = np.diag(S).copy()
    S[np.arange(len(dg)), np.arange(len(dg))] = dg + lam * dg
    return S


def residual_ratio(G, lam, g, delta):
    """||A delta - g||_inf / (d 2^-53 (||A||_inf ||delta||_inf + ||g||_inf)): to be held against BOUND_C (or a quarter of it)."""
    A = damped(G, lam)
    d = len(g)
    scale = d * U * (np.abs(A).sum(1).max() * np.abs(delta).max() + np.abs(g).max())
    return float(np.abs(A @ delta - g).max() / scale) if scale > 0 else 0.0
