"""A plain numpy float64 emulation of csrc/tangent_pca.hip, the inputs of its tests and the bounds they hold it to
(no GPU, not a test module).

``emulate(G32, V, w, r)`` runs the kernel's operation sequence on a batch: y_k = G v_k with j ascending, q_kl = sum_i y_k[i] v_l[i]
with i ascending, M = ((sqrt(w_k) sqrt(w_l)) q_kl) / W, ``_jacobi_emulation.jacobi`` for M = P Lambda P^T (the kernel runs the
spectrum kernel's sweeps; its descending ranks are the reverse of the ascending ones there, and the sign ``jacobi`` gives a column
of P cancels in the sign rule on u_j, because u_j and the scores are odd in that column operation by operation), the rank, the
directions with k ascending, the sign rule and the scores.  Every step is one rounded float64 operation, as the kernel is built
without fused multiply-adds.

``check(G32, V, w, out)`` gives the reached fractions of the bounds (u = 2^-53, C = _jacobi_emulation.BOUND_C), against numpy
float64 -- the dual matrix and the recomputations from the outputs in longdouble where the platform has one -- on the same float32
``jtj`` (lower triangle mirrored), ``V`` and ``w``:
    Mabs = D^1/2 |V| |G| |V^T| D^1/2 / W entrywise,  E = (C K max |lambda_ref| + 2 (2 d + 6) K max Mabs) u
        (the backward error of the Jacobi method plus the rounding of a two-stage contraction of length d, carried to the 2-norm);
    eigenvalues      |lambda_j - lambda_ref,j| <= E
    orthonormality   |u_j^T G u_l - delta_jl| <= E / sqrt(lambda_j lambda_l)                 j, l < rank
    scores           |s_kj - v_k^T G u_j| <= E sqrt(W / w_k) / sqrt(lambda_j)                j < rank
    covectors, norm2 2 (d + 4) u sum |terms|
    total            2 (d + K + 4) u sum |terms|: behind the two-stage contraction of length d stand the K-term sums of the numerator
                     and of W and a division, 2 d + 2 (K - 1) + 2 roundings in all; without the K the form is below what
                     sequential float64 sums can reach at small d and K = 64 (this emulation came to 0.40 of 2 (d + 4) u at d = 2)
    rank             = #{ own variances > (d 2^-24) lambda_1 }  (where all K variances are returned)
and, where rank = K, the reconstruction sum_j s_kj u_j = v_k: in exact arithmetic it is sum_l sqrt(w_l / w_k) (P P^T)_kl v_l, so it
fails by the departure of P from orthogonality (C K u entrywise, the bound of _jacobi_emulation) and the rounding of two K-term sums
(below C K u of their magnitudes):
    reconstruction   |sum_j s_kj u_j[i] - v_k[i]| <= C K u (sum_l sqrt(w_l / w_k) |v_l[i]| + sum_j |s_kj| |u_j[i]|)."""
import functools

import numpy as np
import torch

import _jacobi_emulation as J

U = J.U
BOUND_C = J.BOUND_C
MAX_SWEEPS = J.MAX_SWEEPS
MAX_ARMS = 64
WEIGHT_CYCLE = (1.0, 2.0, 0.5, 3.0, 0.25)
WIDTHS = (1, 2, 16, 17, 64, 65, 128)
ARMS = (1, 2, 3, 5, 63, 64)
KEYS = ("variances", "directions", "scores", "covectors", "norm2", "total")
LONG = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64


def emulate(G32, V, w, r=None):
    """The kernel on jtj ``G32`` (B, d, d) float32, ``V`` (B, K, d) and ``w`` (B, K) float64, ``r`` components (default K): a dict
    of numpy arrays named like ``engine.TangentPcaResult``."""
    G32, V, w = np.asarray(G32, dtype=np.float32), np.asarray(V, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, d = G32.shape[0], G32.shape[1]
    K = V.shape[1]
    r = K if r is None else r
    low = np.tril(np.ones((d, d), dtype=bool))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(G32[:, low]).all(1) & np.isfinite(V).reshape(B, -1).all(1) & (np.isfinite(w) & (w > 0)).all(1))
        G = np.where(bad[:, None, None], 0.0, J.symmetric64(np.where(np.isfinite(G32), G32, 0.0)))
        V_ = np.where(bad[:, None, None], 0.0, V)
        w_ = np.where(bad[:, None], 1.0, w)
        sw = np.sqrt(w_)
        W = w_[:, 0].copy()
        for k in range(1, K):
            W = W + w_[:, k]
        Y = np.zeros((B, K, d))
        for j in range(d):
            Y = Y + G[:, None, :, j] * V_[:, :, None, j]
        Q = np.zeros((B, K, K))
        for i in range(d):
            Q = Q + Y[:, :, None, i] * V_[:, None, :, i]
        norm2 = np.einsum("bkk->bk", Q).copy()
        M = ((sw[:, :, None] * sw[:, None, :]) * Q) / W[:, None, None]
        total = w_[:, 0] * norm2[:, 0]
        for k in range(1, K):
            total = total + w_[:, k] * norm2[:, k]
        total = total / W
        eig, vec, sweeps, info = J.jacobi(M)                       # reads the lower triangles
        lam, P = eig[:, ::-1], vec[:, :, ::-1]
        rank = (lam > (d * 2.0 ** -24) * lam[:, :1]).sum(1).astype(np.int32)
        live = np.arange(K)[None, :] < rank[:, None]
        den = np.sqrt(W[:, None] * np.where(live, lam, 1.0))
        acc = np.zeros((B, K, d))
        for k in range(K):
            acc = acc + (sw[:, k, None, None] * P[:, k, :, None]) * V_[:, k, None, :]
        Um = np.where(live[:, :, None], acc / den[:, :, None], 0.0)
        top = np.abs(Um).argmax(2)
        sgn = np.where(np.take_along_axis(Um, top[:, :, None], 2)[:, :, 0] < 0.0, -1.0, 1.0)
        Um = sgn[:, :, None] * Um
        S = np.where(live[:, None, :], sgn[:, None, :] * ((den[:, None, :] * P) / sw[:, :, None]), 0.0)
    out = {"variances": lam[:, :r].copy(), "directions": Um[:, :r].copy(), "scores": S[:, :, :r].copy(), "covectors": Y, "norm2": norm2,
           "total": total, "rank": rank, "sweeps": sweeps.astype(np.int32), "info": info.astype(np.int32)}
    for key in KEYS:
        out[key][bad] = np.nan
    out["rank"][bad], out["sweeps"][bad], out["info"][bad] = 0, 0, 2
    return out


# --------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------


def column_scale(d):
    return 2.0 ** torch.linspace(-2, 2, d).round()


def gram(B, d, seed=0):
    """float32 Gram matrices A^T A of A = randn(B, d + 3, d) with the columns scaled by powers of two spanning 2^-2 .. 2^2."""
    gen = torch.Generator().manual_seed(1000 * d + B + seed)
    A = torch.randn(B, d + 3, d, generator=gen) * column_scale(d)
    return torch.bmm(A.transpose(1, 2), A).contiguous().numpy()


def vectors(B, K, d, seed=0):
    """(B, K, d) float64 randn, scaled like the columns of ``gram``."""
    gen = torch.Generator().manual_seed(77 * d + 1000 * K + B + seed)
    return (torch.randn(B, K, d, generator=gen, dtype=torch.float64) * column_scale(d).double()).contiguous().numpy()


def weights(B, K):
    """(B, K) float64 cycled from (1, 2, 0.5, 3, 0.25), group b starting at entry b of the cycle."""
    return np.array([[WEIGHT_CYCLE[(b + k) % len(WEIGHT_CYCLE)] for k in range(K)] for b in range(B)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def inputs(B, K, d):
    return gram(B, d), vectors(B, K, d), weights(B, K)


def design_ranks(K, d):
    m = min(K, d)
    return sorted({1, m // 2, m} - {0})


def designed(d, K, r0, seed=0):
    """One group (jtj (1, d, d) float32, V (1, K, d), w (1, K)) whose dual matrix has the r0 eigenvalues 10^linspace(0, -2, r0) and
    K - r0 zeros: with G = L L^T, v_k = L^-T row k of D^-1/2 P0 diag(sqrt(W sigma)) E^T, P0 (K, r0) and E (d, r0) orthonormal."""
    rng = np.random.default_rng(10000 * d + 100 * K + r0 + seed)
    G32 = gram(1, d, seed=5 + seed)
    w = weights(1, K)
    L = np.linalg.cholesky(J.symmetric64(G32)[0])
    P0, _ = np.linalg.qr(rng.standard_normal((K, r0)))
    E0, _ = np.linalg.qr(rng.standard_normal((d, r0)))
    sigma = 10.0 ** np.linspace(0.0, -2.0, r0)
    R = (P0 * np.sqrt(w[0].sum() * sigma)) @ E0.T / np.sqrt(w[0])[:, None]           # (K, d)
    V = np.linalg.solve(L.T, R.T).T
    return G32, np.ascontiguousarray(V[None]), w, sigma


# --------------------------------------------------------------------------------------------------
# the reference and the bounds
# --------------------------------------------------------------------------------------------------


def reference(G32, V, w):
    """Per group in float64 (the products in longdouble where there is one): (lambda_ref (B, K) descending, max Mabs (B,), W (B,))."""
    G = J.symmetric64(G32).astype(LONG)
    Vl, wl = V.astype(LONG), w.astype(LONG)
    W = wl.sum(1)
    sw = np.sqrt(wl)
    M = (sw[:, :, None] * sw[:, None, :]) * (Vl @ G @ np.transpose(Vl, (0, 2, 1))) / W[:, None, None]
    Mabs = (sw[:, :, None] * sw[:, None, :]) * (np.abs(Vl) @ np.abs(G) @ np.abs(np.transpose(Vl, (0, 2, 1)))) / W[:, None, None]
    M = M.astype(np.float64)
    lam = np.linalg.eigvalsh(0.5 * (M + np.transpose(M, (0, 2, 1))))[:, ::-1]
    return lam, Mabs.reshape(len(M), -1).max(1).astype(np.float64), W.astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference_inputs(B, K, d):
    """``reference`` on ``inputs(B, K, d)`` (computed once per process)."""
    return reference(*inputs(B, K, d))


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 (an exact result meets a zero bound)."""
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.where(err == 0.0, 0.0, err / bound).max())


def check(G32, V, w, out, ref=None):
    """The reached fractions of the bounds, the largest over the batch, as a dict; ``rank`` is 1.0 where the rank is not the count of
    the group's own variances above the threshold (only judged where all K variances are there), else 0.  Groups with info != 0 are
    not looked at."""
    G32, V, w = np.asarray(G32), np.asarray(V, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, d, K = G32.shape[0], G32.shape[1], V.shape[1]
    r = out["variances"].shape[1]
    lam_ref, mabs, W = reference(G32, V, w) if ref is None else ref
    G = J.symmetric64(G32).astype(LONG)
    worst = dict.fromkeys(("eigenvalues", "orthonormality", "scores", "covectors", "norm2", "total", "rank", "reconstruction"), 0.0)
    for b in range(B):
        if out["info"][b] != 0:
            continue
        E = (BOUND_C * K * np.abs(lam_ref[b]).max() + 2.0 * (2 * d + 6) * K * mabs[b]) * U
        lam, rank = out["variances"][b], int(out["rank"][b])
        Ud, S, Vb, wb = out["directions"][b].astype(LONG), out["scores"][b].astype(LONG), V[b].astype(LONG), w[b]
        m = min(rank, r)
        worst["eigenvalues"] = max(worst["eigenvalues"], _ratio(np.abs(lam - lam_ref[b, :r]), E))
        if m:
            root = np.sqrt(lam[:m])
            gram_u = Ud[:m] @ G[b] @ Ud[:m].T
            worst["orthonormality"] = max(worst["orthonormality"], _ratio(np.abs(gram_u - np.eye(m)), E / (root[:, None] * root[None, :])))
            proj = Vb @ G[b] @ Ud[:m].T                                                         # (K, m): v_k^T G u_j
            worst["scores"] = max(worst["scores"], _ratio(np.abs(S[:, :m] - proj),
                                                          E * np.sqrt(W[b] / wb)[:, None] / root[None, :]))
        aG, aV = np.abs(G[b]), np.abs(Vb)
        tol = 2.0 * (d + 4) * U
        worst["covectors"] = max(worst["covectors"], _ratio(np.abs(out["covectors"][b].astype(LONG) - Vb @ G[b]),
                                                            tol * (aV @ aG).astype(np.float64)))
        q, qa = np.einsum("ki,ki->k", Vb @ G[b], Vb), np.einsum("ki,ki->k", aV @ aG, aV)
        worst["norm2"] = max(worst["norm2"], _ratio(np.abs(out["norm2"][b].astype(LONG) - q), tol * qa.astype(np.float64)))
        wl = wb.astype(LONG)
        worst["total"] = max(worst["total"], _ratio(abs(LONG(out["total"][b]) - (wl * q).sum() / wl.sum()),
                                                    2.0 * (d + K + 4) * U * float((wl * qa).sum() / wl.sum())))
        if r == K:
            own = int((lam > (d * 2.0 ** -24) * lam[0]).sum())
            worst["rank"] = max(worst["rank"], 0.0 if own == rank else 1.0)
            if rank == K:
                back = S @ Ud                                                                   # (K, d)
                sw = np.sqrt(wl)
                bound = BOUND_C * K * U * (((sw[None, :] / sw[:, None]) @ aV) + np.abs(S) @ np.abs(Ud)).astype(np.float64)
                worst["reconstruction"] = max(worst["reconstruction"], _ratio(np.abs(back - Vb), bound))
    return worst


def contract_holds(out, d, K, r):
    """Shapes and dtypes, descending variances, 1 <= sweeps <= MAX_SWEEPS, exact zeros beyond the rank, the sign rule (info 0)."""
    B = out["info"].shape[0]
    ok = out["variances"].shape == (B, r) and out["directions"].shape == (B, r, d) and out["scores"].shape == (B, K, r)
    ok &= out["covectors"].shape == (B, K, d) and out["norm2"].shape == (B, K) and out["total"].shape == (B,)
    ok &= all(out[k].dtype == np.float64 for k in KEYS) and all(out[k].dtype == np.int32 and out[k].shape == (B,)
                                                                for k in ("rank", "sweeps", "info"))
    if not ok:
        return False
    for b in np.flatnonzero(out["info"] == 0):
        lam, rank, Ud = out["variances"][b], int(out["rank"][b]), out["directions"][b]
        ok &= bool((lam[:-1] >= lam[1:]).all()) and 1 <= out["sweeps"][b] <= MAX_SWEEPS and 0 <= rank <= min(K, d)
        ok &= not Ud[rank:].any() and not out["scores"][b][:, rank:].any()
        m = min(rank, r)
        top = np.abs(Ud[:m]).argmax(1)
        ok &= bool((Ud[np.arange(m), top] > 0.0).all())
    return bool(ok)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
