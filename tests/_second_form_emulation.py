"""numpy emulation of ``cmf_second_form`` (csrc/second_form.hip), operation by operation in float64 without contraction:
the same sums in the same order (the row groups of the J^T E stream and their fold, the per-thread rows, wave trees and wave order of the S2 / asymmetry sums, G u with
j ascending, the forms with r ascending), the division by the step where the kernel has it (once per folded sum), the square-root-free
elimination of ``_transport_emulation.chol_solve`` with the q right-hand sides as extra rows, the Schur complement from the
forward-substituted rows (k ascending, the multiplier by division), the same back substitution and the same failure codes.  Also the
data the kernel tests run on and the bound forms, so that the CPU tests hold the emulation to the kernel's bounds on the very inputs the
GPU sees.

Bound forms, per sample (u = 2^-53; "terms" are the exact float64 products of the float32 inputs, divided by the step):
    A, S2, the two asymmetry sums:  |err| <= 2 (D + 4) u sum |terms|           (A is no output: the emulation holds it; on the GPU it is
                                                                              inside the N bound, and the Gamma form has room for it)
    Gamma:  ||G Gamma_p - A_p||_inf <= 32 d u (||G||_inf ||Gamma_p||_inf + ||A_p||_inf), A_p exact           (the projector's form)
    N:      |err_pp'| <= 2 (D + 4) u sum_r |H_p H_p'| + sum_i (dA_p[i] |Gamma_p'[i]| + |Gamma_p[i]| dA_p'[i]) + 4 (d + 2) u F_p F_p',
            F_p = sum_i |Gamma_p[i]| sqrt(G_ii)
            -- the contraction error of S2, the A bound dA carried through A^T G^-1 A, and the elimination: the computed factors satisfy
            L D L^T = G + dG with |dG| <= (d + 1) u |L||D||L^T|, either forward substitution perturbs L by d u |L|, the k sum with its
            divisions adds (d + 2) u sum_k |y_k y'_k|; with y = L^T Gamma each of the four is at most its constant times
            |Gamma_p|^T (|L||L|^T) |Gamma_p'|, and (|L||L|^T)_ij <= sqrt(G_ii G_jj) by Cauchy-Schwarz: (4 d + 5) u F_p F_p' in all.  The
            form is the absolute-value version of Gamma^T G Gamma = A^T G^-1 A: it scales with what is subtracted, not with N.
    frame_metric:  |err| <= 2 (d + 2) u sum |terms|."""
import numpy as np

import _transport_emulation as TE

U = 2.0 ** -53
NAN = float("nan")
NT = 256
SUM_CONSTANT = 2.0            # x (D + 4) u
GAMMA_CONSTANT = 32.0         # x d u
ELIM_CONSTANT = 4.0           # x (d + 2) u
METRIC_CONSTANT = 2.0         # x (d + 2) u


def pairs(m):
    return [(a, b) for a in range(m) for b in range(a, m)]


def lanes(nc):
    lp = 4
    while 4 * lp < nc and lp < 32:
        lp <<= 1
    return lp


def forward(G, rhs):
    """The forward half of ``_transport_emulation.chol_solve``: the eliminated window (d + q, d) -- pivots on the diagonal, the
    forward-substituted right-hand sides as rows d .. -- or None where a pivot is not positive and finite."""
    d = G.shape[0]
    A = np.concatenate([np.tril(G), rhs], axis=0).astype(np.float64)
    for k in range(d):
        piv = A[k, k]
        if not (piv > 0.0) or not (piv < 1.0e300):
            return None
        l = A[k + 1:, k] / piv
        upd = l[:, None] * A[k + 1:d, k][None, :]
        mask = np.arange(k + 1, A.shape[0])[:, None] >= np.arange(k + 1, d)[None, :]
        A[k + 1:, k + 1:d] = np.where(mask, A[k + 1:, k + 1:d] - upd, A[k + 1:, k + 1:d])
    return A


def back(A, d):
    """The back substitution of ``chol_solve`` on the rows d .. of an eliminated window (a copy is worked on)."""
    A = A.copy()
    Wr = A[d:]
    x = np.zeros_like(Wr)
    for r in range(d - 1, -1, -1):
        x[:, r] = Wr[:, r] / A[r, r]
        Wr[:, :r] = Wr[:, :r] - A[r, :r][None, :] * x[:, r][:, None]
    return x


def sample(J, Glow, S, frame, h, nc):
    """The kernel on one sample: J (D, d) float32, Glow (d, d) float32 (lower triangle), S (2 m, D, m) float32 (index 2 a + sign),
    frame (m, d) float64, h.  Returns (second_gram, christoffel, frame_metric, stats, info, A (d, q))."""
    D, d = J.shape
    m = frame.shape[0]
    pr = pairs(m)
    q = len(pr)
    nan = lambda *s: np.full(s, NAN)
    low = np.tril(np.ones((d, d), dtype=bool))
    if not (np.isfinite(J).all() and np.isfinite(S).all() and np.isfinite(Glow[low]).all() and np.isfinite(frame).all()
            and np.isfinite(h) and h > 0):
        return nan(q, q), nan(q, d), nan(m, m), nan(4), 2, nan(d, q)
    w = 4.0 * h
    w2 = w * w
    J64, S64 = J.astype(np.float64), S.astype(np.float64)
    delta = S64[0::2] - S64[1::2]                                    # (m, D, m): delta[a][:, c]
    E = np.stack([delta[a][:, b] + delta[b][:, a] for a, b in pr], 1)                        # (D, q)
    # 1. the row groups and their fold
    RG = NT // lanes(nc)
    araw = np.zeros((d, q))
    for rg in range(RG):
        acc = np.zeros((d, q))
        for r in range(rg, D, RG):
            acc = acc + J64[r][:, None] * E[r][None, :]
        araw = araw + acc
    A = araw / w
    # 2. S2 and the asymmetry sums: thread t takes the rows t, t + 256, ...; the xor tree of each wave; the waves in order
    acc, a0, a1 = np.zeros((NT, q, q)), np.zeros(NT), np.zeros(NT)
    for r0 in range(0, D, NT):
        n = min(NT, D - r0)
        Er = E[r0:r0 + n]
        acc[:n] = acc[:n] + Er[:, :, None] * Er[:, None, :]
        for a in range(m):
            for c in range(a + 1, m):
                x, y = delta[a][r0:r0 + n, c], delta[c][r0:r0 + n, a]
                a0[:n] = a0[:n] + (x - y) * (x - y)
                a1[:n] = a1[:n] + (x + y) * (x + y)

    def waves(v):
        v = v.reshape(4, 64, *v.shape[1:])
        lane = np.arange(64)
        for sh in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ sh]
        return v[:, 0]

    part, pa, ph = waves(acc), waves(a0), waves(a1)
    fold = lambda p: ((p[0] + p[1]) + p[2]) + p[3]
    S2 = fold(part) / w2
    st0, st1 = fold(pa) / (0.25 * w2), fold(ph) / w2
    tr2 = 0.0
    for p in range(q):
        tr2 = tr2 + S2[p, p]
    # 3. the frame's metric
    G = TE.symmetric(Glow)
    gu = TE.metric_product(G, frame)                                 # (m, d), j ascending
    fm = np.zeros((m, m))
    for a in range(m):
        for c in range(a + 1):
            s = 0.0
            for r in range(d):
                s = s + frame[a, r] * gu[c, r]
            fm[a, c] = fm[c, a] = s
    # 4. - 6.
    win = forward(G, A.T.copy())
    if win is None:
        return nan(q, q), nan(q, d), fm, np.array([st0, st1, tr2, NAN]), 1, A
    Wr, piv = win[d:], np.diagonal(win[:d]).copy()
    acc = np.zeros((q, q))
    for k in range(d):
        acc = acc + (Wr[:, k] / piv[k])[:, None] * Wr[:, k][None, :]
    N = np.tril(S2 - acc)
    N = N + np.tril(N, -1).T
    trn = 0.0
    for p in range(q):
        trn = trn + N[p, p]
    return N, back(win, d), fm, np.array([st0, st1, tr2, trn]), 0, A


def batch(Jd, jtj, Sd, frame, step, nc):
    """``sample`` over a batch: Jd (B, D, d), jtj (B, d, d), Sd (B 2 m, D, m), frame (B, m, d), step (B,) -> stacked outputs."""
    B, m = frame.shape[0], frame.shape[1]
    outs = [sample(Jd[b], jtj[b], Sd[2 * m * b:2 * m * (b + 1)], frame[b], step[b], nc) for b in range(B)]
    return tuple(np.stack([np.asarray(o[i]) for o in outs]) for i in range(6))


# ---------------------------------------------------------------------------------------------------
# the exact values and the bound ratios
# ---------------------------------------------------------------------------------------------------

LD = np.longdouble


def exact(J, Glow, S, frame, h):
    """One sample in extended precision on the same float32 inputs: a dict of H (D, q), A (d, q), S2, N, Gamma (q, d), frame_metric,
    the two asymmetry sums, and the absolute-value sums the bounds scale with.  The solves are float64 ``numpy.linalg`` with two steps
    of iterative refinement whose residuals are taken in extended precision."""
    m = frame.shape[0]
    pr = pairs(m)
    w = LD(4.0) * LD(h)
    Jl, Sl = J.astype(LD), S.astype(LD)
    delta = Sl[0::2] - Sl[1::2]
    H = np.stack([delta[a][:, b] + delta[b][:, a] for a, b in pr], 1) / w
    A = Jl.T @ H
    S2 = H.T @ H
    G = TE.symmetric(Glow)
    Gl = G.astype(LD)
    X = np.linalg.solve(G, A.astype(np.float64)).astype(LD)
    for _ in range(2):
        X = X + np.linalg.solve(G, (A - Gl @ X).astype(np.float64)).astype(LD)
    anti = [(delta[a][:, c] - delta[c][:, a]) / (LD(2.0) * LD(h)) for a in range(m) for c in range(a + 1, m)]
    symm = [(delta[a][:, c] + delta[c][:, a]) / w for a in range(m) for c in range(a + 1, m)]
    fl = frame.astype(LD)
    return {"H": H, "A": A, "S2": S2, "N": S2 - A.T @ X, "Gamma": X.T, "G": Gl, "fm": fl @ Gl @ fl.T,
            "st0": sum((v * v).sum() for v in anti) if anti else LD(0), "st1": sum((v * v).sum() for v in symm) if symm else LD(0),
            "A_abs": np.abs(Jl).T @ np.abs(H), "S2_abs": np.abs(H).T @ np.abs(H),
            "fm_abs": np.abs(fl) @ np.abs(Gl) @ np.abs(fl).T}


def ratios(ex, got, D, d):
    """error / bound for one sample: ``got`` = (second_gram, christoffel, frame_metric, stats[, info, A]) of the kernel or the emulation, ``ex``
    the dict of ``exact``.  Returns a dict of the worst ratio per bound form; 0 / 0 counts as 0."""
    N, Gam, fm, st = (np.asarray(v).astype(LD) for v in got[:4])
    su, q = SUM_CONSTANT * (D + 4) * U, N.shape[0]

    def worst(err, bound):
        err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
        return float(np.where(err == 0, LD(0), err / np.where(bound > 0, bound, np.finfo(LD).tiny)).max())

    out = {}
    dA = su * ex["A_abs"]                                            # (d, q)
    if len(got) > 5:
        out["A"] = worst(np.abs(np.asarray(got[5]).astype(LD) - ex["A"]), dA)
    out["S2"] = worst(np.abs(st[2] - np.trace(ex["S2"])), su * np.trace(ex["S2_abs"]))
    out["asym"] = max(worst(np.abs(st[0] - ex["st0"]), su * ex["st0"]), worst(np.abs(st[1] - ex["st1"]), su * ex["st1"]))
    G, A = ex["G"], ex["A"]
    res = np.abs(Gam @ G - A.T).max(1)                               # rows p
    scale = TE.inf_norm(np.abs(G)) * np.abs(Gam).max(1) + np.abs(A).max(0)
    out["Gamma"] = worst(res, GAMMA_CONSTANT * d * U * scale)
    aG = np.abs(ex["Gamma"])                                         # (q, d)
    F = aG @ np.sqrt(np.diagonal(G))
    carried = aG @ dA
    bound = su * ex["S2_abs"] + carried + carried.T + ELIM_CONSTANT * (d + 2) * U * np.outer(F, F)
    out["N"] = worst(np.abs(N - ex["N"]), bound)
    out["trace"] = worst(np.abs(st[3] - np.trace(ex["N"])), np.trace(bound) + q * U * np.abs(np.diagonal(ex["N"])).sum())
    out["metric"] = worst(np.abs(fm - ex["fm"]), METRIC_CONSTANT * (d + 2) * U * ex["fm_abs"])
    return out


def exacts(case_):
    """``exact`` of every sample of a ``case``."""
    Jd, jtj, Sd, frame, step, nc = case_
    m = frame.shape[1]
    return [exact(Jd[b], jtj[b], Sd[2 * m * b:2 * m * (b + 1)], frame[b], step[b]) for b in range(frame.shape[0])]


def worst_ratios(case_, got, exs=None):
    """``ratios`` over the batch of a ``case``: the largest per form.  ``exs``: the ``exacts`` of the case where the caller holds them."""
    tot = {}
    for b, ex in enumerate(exacts(case_) if exs is None else exs):
        for k, v in ratios(ex, [g[b] for g in got], case_[0].shape[1], case_[0].shape[2]).items():
            tot[k] = max(tot.get(k, 0.0), v)
    return tot


# ---------------------------------------------------------------------------------------------------
# the data of the kernel tests
# ---------------------------------------------------------------------------------------------------

WIDTHS = [1, 2, 3, 16, 17, 64, 65, 127, 128]
FRAMES = [1, 2, 3, 4]
BATCHES = [1, 3]
STEPS = [2.0 ** -7, 0.01, 2.0 ** -5]                 # per sample, cyclically: the middle one makes (4 h)^2 round


def rows_of(d):
    return [d + 3, 50 + d]


def ceil16(n):
    return (n + 15) // 16 * 16


def case(B, d, m, D, seed=0, cond=1e3, asym=1e-3):
    """Seeded inputs of the kernel: (Jd (B, D, d) float32, jtj (B, d, d) float32 with NaN in every strict upper triangle, Sd
    (B 2 m, D, m) float32, frame (B, m, d) float64 of unit rows, step (B,), nc).  Jacobians with cond(G) ~ ``cond`` (for D >= d);
    shifted columns = centre columns +- h (a seeded symmetric second-derivative stack of order one + an antisymmetric part of relative
    size ``asym``), rounded to float32."""
    rng = np.random.default_rng(100000 * d + 1000 * D + 10 * m + B + seed)
    s = np.sqrt(np.logspace(0, -np.log10(cond), d)) if d > 1 else np.ones(1)
    Jd = np.zeros((B, D, d), dtype=np.float32)
    for b in range(B):
        Q = np.linalg.qr(rng.standard_normal((D, d)))[0]
        V = np.linalg.qr(rng.standard_normal((d, d)))[0]
        Jd[b] = ((Q * s) @ V.T * 2.0 ** rng.integers(-3, 4)).astype(np.float32)
    J64 = Jd.astype(np.float64)
    jtj = np.einsum("bra,brc->bac", J64, J64).astype(np.float32)
    jtj[:, ~np.tril(np.ones((d, d), dtype=bool))] = np.float32(NAN)
    frame = rng.standard_normal((B, m, d))
    frame /= np.sqrt((frame * frame).sum(2, keepdims=True))
    step = np.array([STEPS[b % len(STEPS)] for b in range(B)])
    sym = rng.standard_normal((B, m, m, D))
    sym = 0.5 * (sym + sym.transpose(0, 2, 1, 3))
    anti = rng.standard_normal((B, m, m, D))
    anti = asym * 0.5 * (anti - anti.transpose(0, 2, 1, 3))
    centre = np.einsum("brj,bcj->bcr", J64, frame)                   # (B, m, D): column c
    Sd = np.zeros((B, m, 2, D, m), dtype=np.float32)
    for a in range(m):
        for sg, sign in enumerate((1.0, -1.0)):
            cols = centre + sign * step[:, None, None] * (sym[:, a] + anti[:, a])           # (B, m, D): column c of the shift along a
            Sd[:, a, sg] = cols.transpose(0, 2, 1).astype(np.float32)
    return Jd, jtj, Sd.reshape(B * m * 2, D, m), frame, step, ceil16(d)


# ---------------------------------------------------------------------------------------------------
# known answers: every input exact in float32, the central difference exact
# ---------------------------------------------------------------------------------------------------


def from_jacobians(J0, Jshift, frame, h):
    """The kernel's inputs from exact Jacobians: J0 (D, d) at z, Jshift(a, sign) -> (D, d) at z +- h u_a, integer frame (m, d) whose rows
    need not be unit.  Returns a one-sample case; every value must be exact in float32 (asserted)."""
    m, d = frame.shape
    D = J0.shape[0]
    Sd = np.zeros((m, 2, D, m))
    for a in range(m):
        for sg, sign in enumerate((1.0, -1.0)):
            Sd[a, sg] = Jshift(a, sign) @ frame.T
    G = J0.T @ J0
    for v in (J0, Sd, G):
        assert (v.astype(np.float32).astype(np.float64) == v).all()
    jtj = G.astype(np.float32)
    jtj[~np.tril(np.ones((d, d), dtype=bool))] = np.float32(NAN)
    return (J0.astype(np.float32)[None], jtj[None], Sd.reshape(2 * m, D, m).astype(np.float32), frame.astype(np.float64)[None],
            np.array([h]), ceil16(d))


def quadratic_graph(Q, z, frame, h):
    """Known answer (i): the graph g(z) = (z, 1/2 z^T Q_k z) of K small-integer quadratic forms Q (K, d, d): J(z) = [I; z^T Q_k], so that
    J(z +- h u) - J(z) is +- h u^T Q_k exactly and H_ab = (0, u_a^T Q_k u_b).  Returns (case, H (q, d + K))."""
    K, d, _ = Q.shape
    jac = lambda zz: np.concatenate([np.eye(d), np.einsum("j,kji->ki", zz, Q)], 0)
    cs = from_jacobians(jac(z), lambda a, sign: jac(z + sign * h * frame[a]), frame, h)
    H = np.array([np.concatenate([np.zeros(d), np.einsum("i,kij,j->k", frame[a], Q, frame[b])]) for a, b in pairs(frame.shape[0])])
    return cs, H


def flat(d, m, D, h, seed=0):
    """Known answer (ii): a flat manifold, J(z) = J0 R(z) with small-integer J0 (D, d) and R(z +- h u_a) = I +- h M_a for integer
    M_a: the shifted columns stay inside the column space of J0, so N = 0 while S2 is of order one."""
    rng = np.random.default_rng(977 * d + 13 * m + D + seed)
    for attempt in range(100):
        J0 = rng.integers(-2, 3, (D, d)).astype(np.float64)
        if np.linalg.matrix_rank(J0) == d and np.linalg.cond(J0.T @ J0) < 1e3:
            break
    M = rng.integers(-2, 3, (m, d, d)).astype(np.float64)
    frame = np.zeros((m, d))
    frame[np.arange(m), rng.permutation(d)[:m]] = 1.0
    return from_jacobians(J0, lambda a, sign: J0 @ (np.eye(d) + sign * h * M[a]), frame, h)
