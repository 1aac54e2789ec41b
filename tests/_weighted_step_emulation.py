"""A numpy emulation of the weighted Gauss-Newton step kernel (csrc/weighted_step.hip) on one sample, the seeded
weight patterns the host and GPU tests share, and the Gram bound's constant with its derivation (not collected by pytest).

The emulation does what the kernel does where it matters for the error: the live rows (w > 0) are compacted in row order; G_w is
accumulated in float32, four live rows per step (one v_mfma_f32_16x16x4_f32), the left operand rounded to float32(w_r J_ri); only the
lower triangle is computed and the rest mirrored; g_w = J^T (w o r) and the cost sum w r^2 are float64; the float64 elimination
(``_gn_step_emulation``'s, restated for a given g) runs on the float32 G_w.  Sums the kernel folds by trees are plain numpy sums:
the two agree to rounding, not bit for bit.  Rows with w == 0 are never touched: they may hold NaN."""
import numpy as np

import _gn_step_emulation as GN

U = GN.U
NAN = float("nan")
PATTERNS = ["ones", "half", "third", "few", "zero"]

# Gram bound:  |G_w - G_w64| <= C_WGRAM * S,  S = |J|^T diag(w) |J|  over the live rows.  An element is a sum of n_live products of
# float32(w_r J_ri) -- one rounding, 2^-24 relative -- with J_rj, accumulated in float32: as for the unweighted Gram kernels
# (tests/_gram_head.py, C_GRAM) the k-th partial sum is rounded at its own magnitude <= S, worst case ~n_live 2^-24 S, random signs
# ~sqrt(n_live) 2^-24 |G|.  The constant is 4 x (rounded up to a power of two) what ``gram32`` reaches against float64 on the inputs
# of tests/test_gpu_completion.py -- ``inputs(B, D, d)`` with ``weights(B, D, d)`` over GN.ROWS x GN.WIDTHS --: 2^-20.55 of S.
# tests/test_completion_host.py re-measures it, asserts the factor of four, and asserts that the same emulation with a planted
# defect (weights ignored, w^2 for w, one live row dropped) lands above the constant.  It does not come from a kernel's output.
C_WGRAM = 2.0 ** -18


def weights(B, D, d, seed=0):
    """(B, D) float32, sample b in pattern PATTERNS[b % 5]: all ones; a random 0 / 1 half mask; uniform [0.25, 4] with a random
    third of the rows zero; exactly min(D, d - 1) live rows (uniform [0.25, 4]); all zero."""
    rng = np.random.default_rng(7000003 * d + 1009 * D + B + 17 * seed)
    w = np.zeros((B, D), dtype=np.float32)
    for b in range(B):
        kind = PATTERNS[b % len(PATTERNS)]
        order = rng.permutation(D)
        u = rng.uniform(0.25, 4.0, D).astype(np.float32)
        if kind == "ones":
            w[b] = 1.0
        elif kind == "half":
            w[b, order[:(D + 1) // 2]] = 1.0
        elif kind == "third":
            w[b] = u
            w[b, order[:D // 3]] = 0.0
        elif kind == "few":
            live = order[:min(D, d - 1)]
            w[b, live] = u[live]
    return w


def batch_size():
    """Every pattern with every damping of GN.DAMPINGS: patterns cycle with period 5, dampings with period 3."""
    return len(PATTERNS) * len(GN.DAMPINGS)


def gram32(J, w, mode="kernel"):
    """G_w of one sample in float32 the way the kernel accumulates it (see the module docstring).  ``mode``: a planted defect --
    "unweighted" ignores w (but keeps the live rows), "squared" uses w^2, "dropped" loses the last live row."""
    live = np.flatnonzero(w > 0)
    if mode == "dropped":
        live = live[:-1]
    Jl, wl = J[live].astype(np.float32), w[live].astype(np.float32)
    if mode == "unweighted":
        wl = np.ones_like(wl)
    elif mode == "squared":
        wl = wl * wl
    d = J.shape[1]
    n = len(live)
    pad = -n % 4
    left = np.concatenate([wl[:, None] * Jl, np.zeros((pad, d), np.float32)]).reshape(-1, 4, d)      # float32(w J)
    right = np.concatenate([Jl, np.zeros((pad, d), np.float32)]).reshape(-1, 4, d)
    acc = np.zeros((d, d), dtype=np.float32)
    for g in range(left.shape[0]):
        acc = acc + left[g].T @ right[g]
    low = np.tril(acc)
    return low + np.tril(acc, -1).T


def gram64(J, w):
    """(G_w, S) in float64 from the float32 inputs: J^T diag(w) J and |J|^T diag(w) |J| over the live rows."""
    live = w > 0
    Jl, wl = J[live].astype(np.float64), w[live].astype(np.float64)
    return Jl.T @ (wl[:, None] * Jl), np.abs(Jl).T @ (wl[:, None] * np.abs(Jl))


def gram_ratio(G, G64, S):
    """max over the elements of |G - G64| / S (0 / 0 = 0, x / 0 = inf): to be held against C_WGRAM."""
    err = np.abs(np.asarray(G, dtype=np.float64) - G64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, err / S, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def solve(G, g, lam):
    """delta = (G + lam diag G)^-1 g by the kernel's elimination on the lower triangle of the float32 G (``GN.step``'s, for a
    given g): (delta, [g^T delta, delta^T G delta], info 0 / 1)."""
    d = len(g)
    low = np.tril(np.ones((d, d), dtype=bool))
    G64 = np.where(low, np.asarray(G, dtype=np.float64), 0.0)
    A = np.zeros((d + 1, d))
    A[:d] = G64
    A[d] = g
    k = np.arange(d)
    A[k, k] = A[k, k] + lam * A[k, k]
    for k in range(d):
        piv = A[k, k]
        if not piv > 0.0 or not piv < 1.0e300:
            return np.full(d, NAN), [NAN, NAN], 1
        col = A[k + 1:, k].copy()
        mult = col / piv
        upd = np.outer(mult, col[:d - k - 1])
        keep = np.tril(np.ones((d - k, d - k - 1), dtype=bool))
        keep[-1, :] = True
        A[k + 1:, k + 1:] -= np.where(keep, upd, 0.0)
    rhs = A[d].copy()
    delta = np.zeros(d)
    for i in range(d - 1, -1, -1):
        delta[i] = rhs[i] / A[i, i]
        rhs[:i] -= A[i, :i] * delta[i]
    terms = G64 * np.outer(delta, delta)
    return delta, [float(g @ delta), float(np.diag(terms).sum() + 2.0 * np.tril(terms, -1).sum())], 0


def step(J, w, x, xhat, lam):
    """One sample.  J (D, d) float32 or None (cost-only), w, x, xhat (D,) float32.  Returns (gram (d, d) float32, grad (d,),
    delta (d,), stats (4,), info); cost-only: (None, None, None, stats with only [0] set, info)."""
    w, x, xhat = np.asarray(w), np.asarray(x), np.asarray(xhat)
    live = w > 0
    bad = not (np.isfinite(w).all() and (w >= 0).all() and np.isfinite(x[live]).all() and np.isfinite(xhat[live]).all())
    stats = np.full(4, NAN)
    w64 = w[live].astype(np.float64)
    r = x[live].astype(np.float64) - xhat[live].astype(np.float64)
    if J is None:
        if not bad:
            stats[0] = float((w64 * r) @ r)
        return None, None, None, stats, 2 if bad else 0
    d = J.shape[1]
    if bad or not np.isfinite(J[live]).all():
        return np.full((d, d), np.float32(NAN)), np.full(d, NAN), np.full(d, NAN), stats, 2
    G = gram32(J, w)
    g = J[live].astype(np.float64).T @ (w64 * r)
    stats[0], stats[3] = float((w64 * r) @ r), float(np.abs(g).max())
    delta, stats[1:3], info = solve(G, g, lam)
    return G, g, delta, stats, info


def batch(J, w, x, xhat, lam):
    """``step`` over a batch -> stacked (gram, grad, delta, stats, info); J None: (None, None, None, stats, info)."""
    out = [step(None if J is None else J[b], w[b], x[b], xhat[b], None if J is None else lam[b]) for b in range(len(x))]
    info = np.array([o[4] for o in out], dtype=np.int32)
    if J is None:
        return None, None, None, np.stack([o[3] for o in out]), info
    return tuple(np.stack([o[i] for o in out]) for i in range(4)) + (info,)
