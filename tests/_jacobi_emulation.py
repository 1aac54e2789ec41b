"""A plain numpy float64 emulation of csrc/gram_spectrum.hip and the inputs of its tests (no GPU, not a test module).

``jacobi(G)`` runs the kernel's algorithm on a batch: the round-robin ordering, the relative rotation rule, the rotation from
t = sign(theta) / (|theta| + sqrt(1 + theta^2)), the column update, the row update with a_pq = a_qp = 0 and the closed-form
diagonal, the stop after the first rotation-free sweep, the ranking by counting and the sign rule.  Every step is the same
sequence of single float64 operations the kernel performs (which is built without fused multiply-adds), vectorised over the
disjoint pairs of a step and over the batch.

``cases(B, d)`` is the input list of tests/test_gpu_metric_spectrum.py and tests/test_metric_spectrum_host.py."""
import functools

import numpy as np
import torch

U = 2.0 ** -53
MAX_SWEEPS = 64
#: the constant of the three bounds  C d 2^-53 (max |lambda_ref| or 1); the host test holds the emulation to a quarter of it
BOUND_C = 32.0

#: (B, d) of the kernel test: odd and even d, d not a multiple of the wave, both sides of d = 64 (where V moves from LDS to the
#: output slice), the LDS limit
SHAPES = [(1, 1), (3, 2), (5, 3), (4, 10), (3, 16), (3, 17), (2, 63), (2, 64), (2, 65), (2, 100), (2, 127), (2, 128)]


def pairs(d, s):
    """The index pairs (p < q) of step ``s`` of a sweep at width d: the round-robin on n = d rounded up to even players, pairs
    with the player that does not exist (odd d) left out."""
    n = d + (d & 1)
    n1 = n - 1
    k = np.arange(1, n // 2)
    u = np.concatenate(([n1], (s + k) % n1))
    v = np.concatenate(([s], (s + n1 - k) % n1))
    p, q = np.minimum(u, v), np.maximum(u, v)
    keep = q < d
    return p[keep], q[keep]


def steps(d):
    return d - 1 + (d & 1)


def _sweep(A, V, order):
    """One sweep in place on the batch A, V (n, d, d); returns which samples rotated at least once."""
    n = A.shape[0]
    bi = np.arange(n)[:, None]
    rotated = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for p, q in order:
            if p.size == 0:
                continue
            apq, app, aqq = A[:, q, p], A[:, p, p], A[:, q, q]                     # (n, m), before the rotation
            rot = np.abs(apq) > U * np.sqrt(np.abs(app * aqq))
            if not rot.any():
                continue
            rotated |= rot.any(1)
            th = (aqq - app) / (2.0 * apq)
            t = np.where(th >= 0.0, 1.0, -1.0) / (np.abs(th) + np.sqrt(1.0 + th * th))
            c = 1.0 / np.sqrt(1.0 + t * t)
            sn = t * c
            h = t * apq
            for M in (A, V):                                                          # (b) columns
                X, Y = M[:, :, p], M[:, :, q]                                         # (n, d, m)
                M[:, :, p] = np.where(rot[:, None, :], c[:, None, :] * X - sn[:, None, :] * Y, X)
                M[:, :, q] = np.where(rot[:, None, :], sn[:, None, :] * X + c[:, None, :] * Y, Y)
            X, Y = A[:, p, :], A[:, q, :]                                             # (c) rows, (n, m, d)
            A[:, p, :] = np.where(rot[:, :, None], c[:, :, None] * X - sn[:, :, None] * Y, X)
            A[:, q, :] = np.where(rot[:, :, None], sn[:, :, None] * X + c[:, :, None] * Y, Y)
            A[bi, p, p] = np.where(rot, app - h, A[bi, p, p])
            A[bi, q, q] = np.where(rot, aqq + h, A[bi, q, q])
            A[bi, p, q] = np.where(rot, 0.0, A[bi, p, q])
            A[bi, q, p] = np.where(rot, 0.0, A[bi, q, p])
    return rotated


def jacobi(G, max_sweeps=MAX_SWEEPS):
    """(eigenvalues (B, d) ascending, vectors (B, d, d), sweeps (B,), info (B,)) of the symmetric matrices whose LOWER triangles
    ``G`` (B, d, d) holds; float64 throughout."""
    G = np.asarray(G, dtype=np.float64)
    B, d = G.shape[0], G.shape[1]
    low = np.tril(G)
    A = low + np.transpose(np.tril(G, -1), (0, 2, 1))
    V = np.broadcast_to(np.eye(d), (B, d, d)).copy()
    sweeps = np.zeros(B, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    order = [pairs(d, s) for s in range(steps(d))]
    for sweep in range(max_sweeps):
        act = np.flatnonzero(~done)            # a sample that has converged no longer changes: its later sweeps would be no-ops
        if act.size == 0:
            break
        Aa, Va = A[act], V[act]
        rotated = _sweep(Aa, Va, order)
        A[act], V[act] = Aa, Va
        sweeps[act] += 1
        done[act] = ~rotated
    lam = np.einsum("bkk->bk", A)
    idx = np.arange(d)
    rank = ((lam[:, None, :] < lam[:, :, None]) | ((lam[:, None, :] == lam[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))).sum(2)
    eig = np.empty_like(lam)
    np.put_along_axis(eig, rank, lam, axis=1)
    top = np.abs(V).argmax(1)                                  # first row of the largest magnitude, per column
    sign = np.where(np.take_along_axis(V, top[:, None, :], 1)[:, 0, :] < 0.0, -1.0, 1.0)
    vec = np.empty_like(V)
    np.put_along_axis(vec, np.broadcast_to(rank[:, None, :], V.shape), V * sign[:, None, :], axis=2)
    return eig, vec, sweeps, np.where(done, 0, 1).astype(np.int32)


# --------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------


def gram(B, d, seed=0, rows=None):
    """Gram matrices A^T A of A = randn(B, rows, d) (rows = d + 3 unless given) with the columns scaled by powers of two spanning
    2^-6 .. 2^6: the ``synthetic`` of tests/test_gpu_metric_stats.py."""
    gen = torch.Generator().manual_seed(1000 * d + B + seed)
    scale = 2.0 ** torch.linspace(-6, 6, d).round()
    A = torch.randn(B, d + 3 if rows is None else rows, d, generator=gen) * scale
    return torch.bmm(A.transpose(1, 2), A).contiguous()


def rotated(spectrum, seed):
    """Q diag(spectrum) Q^T with a seeded random orthogonal Q (float64 product, rounded to float32)."""
    d = len(spectrum)
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    M = (Q * np.asarray(spectrum, dtype=np.float64)) @ Q.T
    return torch.from_numpy(0.5 * (M + M.T)).float()


@functools.lru_cache(maxsize=None)
def cases(B, d):
    """(labels, (n, d, d) float32) of one shape: B scaled Gram matrices and one each of the special inputs."""
    out = [(f"gram{i}", g) for i, g in enumerate(gram(B, d))]
    out.append(("identity", torch.eye(d)))
    out.append(("repeated_diagonal", torch.diag(torch.tensor([(3.0, 1.0, 2.0, 1.0)[k % 4] for k in range(d)]))))
    out.append(("rank_deficient", gram(1, d, seed=7, rows=max(d - 2, 0))[0]))
    out.append(("two_clusters", rotated([1.0 if k % 2 else 4.0 for k in range(d)], 100 + d)))
    out.append(("geometric_1e12", rotated(10.0 ** np.linspace(-6.0, 6.0, d) if d > 1 else [1.0], 200 + d)))
    out.append(("zero", torch.zeros(d, d)))
    if d == 2:
        out.append(("equal_diagonal", torch.tensor([[2.0, 1.0], [1.0, 2.0]])))
    return [k for k, _ in out], torch.stack([g for _, g in out]).contiguous()


@functools.lru_cache(maxsize=None)
def emulated(B, d):
    """``jacobi`` on ``cases(B, d)`` (computed once per process)."""
    return jacobi(cases(B, d)[1].numpy())


def symmetric64(G32):
    """The float64 matrices the kernel and ``eigvalsh`` both see: the lower triangle of the float32 input, mirrored."""
    G = np.asarray(G32, dtype=np.float64)
    return np.tril(G) + np.transpose(np.tril(G, -1), (0, 2, 1))


def error_ratios(G32, eig, vec=None, ref=None):
    """Per sample, in units of d 2^-53: (max |lambda - lambda_ref| / max |lambda_ref|, max |G V - V Lambda| / max |lambda_ref|,
    max |V^T V - I|) against ``ref`` (numpy's eigvalsh on the same input unless given); a zero matrix has to be met exactly (ratio 0 or inf).  The last
    two are None without ``vec``."""
    G = symmetric64(G32)
    d = G.shape[1]
    ref = np.linalg.eigvalsh(G) if ref is None else np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max(1)

    def ratio(err, s):
        with np.errstate(all="ignore"):
            return np.where(err == 0.0, 0.0, err / (d * U * s))

    e_val = ratio(np.abs(eig - ref).max(1), scale)
    if vec is None:
        return e_val, None, None
    res = np.abs(G @ vec - vec * eig[:, None, :]).reshape(len(G), -1).max(1)
    orth = np.abs(np.transpose(vec, (0, 2, 1)) @ vec - np.eye(d)).reshape(len(G), -1).max(1)
    return e_val, ratio(res, scale), ratio(orth, np.ones_like(scale))


def sign_rule_holds(vec):
    """Every column's component of largest magnitude (lowest row on ties) is positive."""
    vec = np.asarray(vec)
    top = np.abs(vec).argmax(1)
    return bool((np.take_along_axis(vec, top[:, None, :], 1) > 0.0).all())
