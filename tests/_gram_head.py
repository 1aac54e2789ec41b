"""Helpers shared by tests/test_gpu_gram_head.py and tests/test_gram_head_host.py (not collected by pytest).

The Jacobian head (``cmf_gram_cholesky`` + ``cmf_cholesky_retry``, ``cmf_gram_backward`` / ``_matrix``) is one C entry point in front
of five kernels.  This module holds, from shapes and inputs alone and never from a kernel's output,

* the dispatch predicate restated in exact Python integers (``family`` / ``ring_top``) and a literal walk of the ring kernels'
  offset arithmetic (``ring_offsets_walk``),
* input builders: ``J = Q diag(s) R^T`` with a prescribed condition number of ``J^T J`` and unequal row magnitudes,
* float64 references (Gram, L1 terms, log-det, pivots, ``dJ`` by autograd) and the oracle's jitter loop,
* float32 CPU emulations of the two arithmetic pieces (Gram accumulation in 4-row groups with the 4-plane sum; the pivot-only
  elimination) and of the backward kernel (Gauss-Jordan sweep, ``dJ = J M``),
* the per-element bounds and their constants with the derivation,
* strided, NaN-surrounded device layouts of ``J`` and guard-banded outputs.

LAYOUT CONTRACT of the head kernels (include/cmf_amd.h): row r of sample b is the ``nc`` floats at ``t + b t_b + r t_r``; nothing
outside them is read; the padding columns ``d .. nc - 1`` hold ZEROS (``gram_chol64_kernel`` sums |G_ij| over whole 4 x 4 register
blocks and relies on the padding rows / columns of G being exact zeros).  Every builder here obeys it.
"""
import math

import torch

from _persistent_items import Guarded          # noqa: F401  (re-exported: guard-banded output buffers)

# cmf_gram_cholesky_family (include/cmf_amd.h): 1 .. 8 = gram_chol_kernel<NT>
INVALID, RING64, DIRECT128, WIDE = 0, 64, 128, 512
RING_LIMIT = 0x7FFFFF00
PF = 8                                          # groups the ring kernels load ahead (CMF_DBG_GRAMPF)
KC = 32                                         # J rows per LDS slab of the staged kernel

# ---------------------------------------------------------------------------------------------------------------------------
# Bounds.  Each constant is 4 x (rounded up to a power of two) what the float32 CPU emulation below reaches against float64 on
# the inputs of tests/test_gpu_gram_head.py (the persistent-items convention; the factor absorbs another summation order and
# FMA contraction).  tests/test_gram_head_host.py re-measures the emulation on those inputs, asserts the factor of four, and
# asserts that the same emulation with a planted defect lands above every constant.  None comes from a kernel's output.
#
# Gram:  |G - G64| <= C_GRAM * A,  A = |J|^T |J|.  An element is a sum of n_rows products accumulated in float32: the k-th partial
# sum is rounded at its own magnitude <= A, so the worst case is ~n_rows 2^-24 A (2^-16 at 257 rows) and random signs give
# ~sqrt(n_rows) 2^-24 |G|; |G| << A off the diagonal.  The emulation reaches 2^-21.45 of A over all forward inputs.
C_GRAM = 2.0 ** -19
# Matrix backward:  |dJ - dJ64| <= C_BWD_MATRIX * (|J| |M + M^T|): a float32 sum of d <= 128 products.  Emulation: 2^-21.72.
C_BWD_MATRIX = 2.0 ** -19
# Backward through the inverse:  |dJ - dJ64| <= C_BWD * (|J| |M|abs) with |M|abs = 2 (|ga| |G64^-1| + |go or gd| |sign G|)
# (``backward_M_abs``: term by term, so a cancellation inside M does not shrink the scale).  The kernel inverts ITS float32 Gram
# matrix by an unpivoted Gauss-Jordan sweep in float32: the error of G^-1 is ~cond(G) 2^-24 d^(1/2) |G^-1|, so the constant holds
# for the backward inputs only (BWD_COND = 4).  Emulation: 2^-21.18.
BWD_COND = 4.0
C_BWD = 2.0 ** -19
# Log-det, per sample:  |ld - ld64| <= C_LOGDET * (sum_ij |G64^-1|_ij A_ij + sum_k |log p_k|): the first term is the first-order
# movement of log det under |dG| <= A (tr(G^-1 dG)), the second the float32 logs and their sum.  Emulation: 2^-22.83.
C_LOGDET = 2.0 ** -20


def l1_sum_depth(d):
    """Additions an L1 term goes through in float32: d^2 elements dealt to 256 threads, then an 8-level tree."""
    return -(-d * d // 256) + 8


# ---------------------------------------------------------------------------------------------------------------------------
# Dispatch predicate in exact integers
def ring_top(n_rows, nc, t_r):
    """1 + the largest byte offset gram_chol64_kernel (nc 32 / 48 / 64) or gram_chol_direct_kernel<8> (nc 128) forms for one
    sample's panel: the wave-uniform group offset after the last load (the ring runs PF groups past the last group consumed),
    plus the largest lane offset and the 16 bytes of its load.  Closed form; ``ring_offsets_walk`` walks the kernels' loops."""
    row_bytes = 4 * t_r
    ngroups_all = (n_rows + 3) >> 2
    if nc <= 64:
        ng0 = (ngroups_all + 3) // 4
        loads = PF + PF * (ng0 // PF)
        return loads * 16 * row_bytes + 15 * row_bytes + 15 * 16 + 16
    loads = PF + PF * (-(-ngroups_all // PF))
    return loads * 4 * row_bytes + 3 * row_bytes + 15 * 32 + 16 + 16


def ring_offsets_walk(n_rows, nc, t_r):
    """The same quantity by walking the kernels' own loops (gram_chol.hip), every wave and lane: (largest value any 32-bit
    variable takes + the bytes read there, the descriptor range of the first load)."""
    row_bytes = 4 * t_r
    panel_bytes = n_rows * row_bytes
    ngroups_all = (n_rows + 3) >> 2
    top = panel_bytes
    if nc <= 64:
        group_bytes = 16 * row_bytes
        for wave in range(4):
            ngroups = (ngroups_all + 3 - wave) // 4
            voff = max((wave * 4 + kq) * row_bytes + cl * 16 for kq in range(4) for cl in range(16) if cl * 4 < nc)
            goff = 0
            for _ in range(PF):
                goff += group_bytes
            g0 = 0
            while g0 + PF <= ngroups:
                for _ in range(PF):
                    goff += group_bytes
                g0 += PF
            top = max(top, goff + voff + 16, group_bytes)
    else:
        group_bytes = 4 * row_bytes
        voff = max(kq * row_bytes + cl * 32 + 16 * v for kq in range(4) for cl in range(16) for v in range(2))
        goff = 0
        for _ in range(PF):
            goff += group_bytes
        g0 = 0
        while g0 < ngroups_all:
            for _ in range(PF):
                goff += group_bytes
            g0 += PF
        top = max(top, goff + voff + 16, group_bytes)
    return top, panel_bytes


def family(n_rows, nc, t_r):
    """cmf_gram_cholesky_family restated: a ring kernel only if ``ring_top`` < RING_LIMIT (< 2^31)."""
    if n_rows <= 0 or nc <= 0 or nc % 16 or nc > 512 or t_r < nc or t_r % 4:
        return INVALID
    if nc > 128:
        return WIDE
    if 32 <= nc <= 64 and ring_top(n_rows, nc, t_r) < RING_LIMIT:
        return RING64
    if nc == 128 and ring_top(n_rows, nc, t_r) < RING_LIMIT:
        return DIRECT128
    return nc // 16


def family_name(f):
    return {INVALID: "invalid", RING64: "gram64", DIRECT128: "direct128", WIDE: "wide"}.get(f, f"staged<{f}>")


def ceil16(d):
    return -(-d // 16) * 16


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs
ROW_WEIGHTS = (1.0, 0.5, 2.0, 1.0, 2.0, 0.5, 1.0)


def build_J(n_rows, d, cond, gen, scale=1.0):
    """(n_rows, d) float64: Q diag(s) R^T with orthonormal Q (n_rows x r), R (d x r), r = min(n_rows, d) and s from 1 down to
    cond^-1/2, so the non-zero spectrum of J^T J spans exactly ``cond``.  Q is the orthonormal basis of a row-weighted Gaussian
    matrix (weights 0.5 / 1 / 2 in a period of 7), so rows differ in magnitude by up to 4 and none is negligible."""
    r = min(n_rows, d)
    w = torch.tensor([ROW_WEIGHTS[i % len(ROW_WEIGHTS)] for i in range(n_rows)], dtype=torch.float64)
    Q = torch.linalg.qr(w[:, None] * torch.randn(n_rows, r, generator=gen, dtype=torch.float64))[0]
    R = torch.linalg.qr(torch.randn(d, r, generator=gen, dtype=torch.float64))[0]
    s = torch.logspace(0, -0.5 * math.log10(cond), r, dtype=torch.float64) if r > 1 else torch.ones(1, dtype=torch.float64)
    return scale * (Q * s) @ R.T


SCALE_EXP = 3                                   # sample B - 1 = sample 0 * 2^SCALE_EXP


def build_batch(n_rows, d, cond, seed, B=4, scale=1.0):
    """(B, n_rows, nc) float32 with zero padding columns; sample B - 1 is sample 0 times 2^SCALE_EXP (exact)."""
    gen = torch.Generator().manual_seed(seed)
    nc = ceil16(d)
    J = torch.zeros(B, n_rows, nc)
    for b in range(B - 1):
        J[b, :, :d] = build_J(n_rows, d, cond, gen, scale).float()
    J[B - 1] = J[0] * 2.0 ** SCALE_EXP
    return J


def case_seed(*key):
    return sum(int(k) * m for k, m in zip(key, (1, 1009, 100003, 7))) % (2 ** 31)


COND_CYCLE = (4.0, 1e2, 1e4)                    # not 1: J^T J would be the identity and its off-diagonal L1 sum pure rounding noise


def case_cond(d, n_rows):
    return COND_CYCLE[(d + n_rows) % 3]


# Forward shapes: the smallest at which each code path changes behaviour (n_rows 160: the one full-rank shape of the wide classes)
FORWARD = {
    "staged1": ([1, 3, 15, 16], [1, 31, 32, 33, 64, 65, 100]),
    "gram64": ([17, 32, 33, 47, 48, 49, 63, 64], [1, 3, 4, 5, 16, 17, 127, 128, 129, 132, 257]),
    "staged567": ([65, 79, 80, 81, 95, 96, 97, 100, 111, 112], [1, 31, 32, 33, 100, 160]),
    "direct128": ([113, 127, 128], [1, 3, 4, 29, 32, 33, 35, 100, 160]),
}
FORWARD_CASES = [(fam, d, n) for fam, (ds, ns) in FORWARD.items() for d in ds for n in ns]
BACKWARD_D = [1, 16, 20, 32, 33, 48, 64, 65, 80, 96, 100, 112, 128]
BACKWARD_ROWS = [1, 31, 32, 33, 100, 160]       # 160: full rank at every width (the cotangent form needs G^-1)


def expected_family(name, d):
    nc = ceil16(d)
    return {"staged1": 1, "gram64": RING64, "staged567": nc // 16, "direct128": DIRECT128}[name]


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references
def gram64(J, d):
    """(G, A) in float64 from the float32 batch: G = J^T J, A = |J|^T |J| over the first d columns."""
    Jd = J[:, :, :d].double()
    return torch.einsum("bni,bnj->bij", Jd, Jd), torch.einsum("bni,bnj->bij", Jd.abs(), Jd.abs())


def l1_terms(G):
    diag = torch.diagonal(G, dim1=1, dim2=2).abs().sum(1)
    return G.abs().sum((1, 2)) - diag, diag


def pivots(G):
    """Pivots of the symmetric elimination = squared diagonal of the Cholesky factor ((B, d); NaN rows where it fails)."""
    L, info = torch.linalg.cholesky_ex(G)
    p = torch.diagonal(L, dim1=1, dim2=2) ** 2
    p[info != 0] = float("nan")
    return p


def logdet_scale(G, A):
    """Per-sample magnitude the log-det bound is relative to: sum |G^-1| A + sum |log p_k|."""
    Ginv = torch.linalg.inv(G)
    return (Ginv.abs() * A).sum((1, 2)) + torch.log(pivots(G)).abs().sum(1)


def backward_reference(J, d, terms=True):
    """float64 autograd of the three unit terms: (dlogdet, dl1off, dl1diag), each (B, n_rows, d): the gradient of the term of
    sample b with respect to J_b.  A launch's reference is their per-sample linear combination."""
    out = []
    for which in range(3):
        Jd = J[:, :, :d].double().requires_grad_(True)
        G = torch.einsum("bni,bnj->bij", Jd, Jd)
        diag = torch.diagonal(G, dim1=1, dim2=2).abs().sum(1)
        term = (torch.linalg.slogdet(G)[1], G.abs().sum((1, 2)) - diag, diag)[which]
        term.sum().backward()
        out.append(Jd.grad)
    return out


def backward_M(G, ga, go, gd):
    """float64 M = 2 dG of the backward kernel's product phase (for the bound's |J| |M|)."""
    d = G.shape[1]
    eye = torch.eye(d, dtype=torch.bool)
    sg = torch.sign(G)
    return 2 * (ga[:, None, None] * torch.linalg.inv(G) + torch.where(eye, gd[:, None, None] * sg, go[:, None, None] * sg))


def backward_M_abs(G, ga, go, gd):
    """The magnitude the cotangent bound is relative to: 2 (|ga| |G^-1| + |go or gd| |sign G|), term by term, so that a
    cancellation between the log-det and the L1 terms of M does not shrink the scale the roundings are measured against."""
    d = G.shape[1]
    eye = torch.eye(d, dtype=torch.bool)
    sg = torch.sign(G).abs()
    return 2 * (ga.abs()[:, None, None] * torch.linalg.inv(G).abs()
                + torch.where(eye, gd.abs()[:, None, None] * sg, go.abs()[:, None, None] * sg))


def jitter_loop(jtj, eps0=1e-6, max_attempts=6):
    """The oracle's jitter loop (oracle/cmf_oracle.py ``cholesky_logdet``, non_square.py:262-296) restated in jtj's own dtype:
    factorise the whole batch; while any sample fails add eps to EVERY sample's diagonal, eps *= 10.  -> (logdet (B,), jittered
    jtj, attempts).  The factorisation is the pivot-only elimination (``eliminate``), whose verdict on an exactly singular matrix
    is an exact zero pivot in every precision; LAPACK's potrf takes a square root and divides, so its pivot there is rounding
    noise of either sign and its attempt count on such a matrix is not a property of the input.  On every matrix that is not
    singular to rounding the two agree (tests/test_gram_head_host.py compares them)."""
    eps = torch.tensor(eps0, dtype=jtj.dtype)
    eye = torch.eye(jtj.shape[1], dtype=jtj.dtype)
    attempts = 1
    while True:
        ld, info = eliminate(jtj)
        if int(info.max()) == 0:
            return ld, jtj, attempts
        if attempts >= max_attempts:
            raise RuntimeError("not positive definite after %d attempts" % max_attempts)
        jtj = jtj + eps * eye
        attempts += 1
        eps = eps * 10


def jitters(attempts, eps0=1e-6):
    """The float32 jitters cmf_cholesky_retry adds in attempts 1 .. attempts - 1 (eps0, then * 10.f each, in float32)."""
    out, eps = [], torch.tensor(eps0, dtype=torch.float32)
    for _ in range(attempts - 1):
        out.append(eps.clone())
        eps = eps * torch.tensor(10.0, dtype=torch.float32)
    return out


# Failure / retry inputs for the kernels that divide in IEEE: (family, d, n_rows, j): one sample has columns j - 1 and j equal.
# j on a 16-tile boundary wherever the width has one.  scale 2^-4: G ~ 2^-8, so the first jitter (1e-6) is ~3e-4 of the diagonal,
# three orders above float32 rounding: the second attempt succeeds in float32 and in float64 alike.
FAILURE_CASES = [("staged1", 16, 33, 8), ("staged1", 3, 65, 2), ("staged567", 80, 100, 16), ("staged567", 81, 100, 80),
                 ("staged567", 96, 160, 80), ("staged567", 100, 160, 16), ("staged567", 112, 160, 80),
                 ("direct128", 113, 160, 112), ("direct128", 128, 160, 16), ("direct128", 128, 160, 112)]
FAILURE_SAMPLE = 1
FAILURE_SCALE = 2.0 ** -4


def build_failure_batch(n_rows, d, j, singular=True):
    J = build_batch(n_rows, d, BWD_COND, case_seed(d, n_rows, 2), scale=FAILURE_SCALE)
    if singular:
        J[FAILURE_SAMPLE, :, j] = J[FAILURE_SAMPLE, :, j - 1]
    return J


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulations
def emulate_gram(J, d, planes):
    """J^T J in float32 the way the kernels accumulate it: 4-row groups (one v_mfma_f32_16x16x4_f32 step each), added one after
    the other; ``planes`` = 4: group g goes to plane g % 4 and the planes are summed (p0 + p1) + (p2 + p3) (gram_chol64_kernel);
    1: one accumulator (staged and direct kernels)."""
    B, N, _ = J.shape
    ng = (N + 3) // 4
    Jp = torch.zeros(B, ng * 4, d)
    Jp[:, :N] = J[:, :, :d]
    P = torch.einsum("bgki,bgkj->bgij", Jp.view(B, ng, 4, d), Jp.view(B, ng, 4, d))
    acc = [torch.zeros(B, d, d) for _ in range(planes)]
    for g in range(ng):
        acc[g % planes] = acc[g % planes] + P[:, g]
    return acc[0] if planes == 1 else (acc[0] + acc[1]) + (acc[2] + acc[3])


def eliminate(G):
    """Pivot-only elimination G_ij -= (G_ik / p_k) G_jk in G's own dtype on (B, d, d): (logdet (B,) with NaN where a pivot is
    not positive and finite, info (B,) = 0 or k + 1 of the first bad pivot)."""
    G = G.clone()
    B, d, _ = G.shape
    ld = torch.zeros(B, dtype=G.dtype)
    info = torch.zeros(B, dtype=torch.int64)
    for k in range(d):
        piv = G[:, k, k]
        bad = ~((piv > 0) & (piv < 3.0e38))
        info = torch.where((info == 0) & bad, torch.full_like(info, k + 1), info)
        ld = ld + torch.log(piv)
        l = G[:, k + 1:, k] / piv[:, None]
        G[:, k + 1:, k + 1:] = G[:, k + 1:, k + 1:] - l[:, :, None] * G[:, None, k + 1:, k]
    ld[info != 0] = float("nan")
    return ld, info


def emulate_elimination(G):
    """``eliminate`` in float32: the arithmetic of block_cholesky / block_cholesky_reg."""
    return eliminate(G.float())


def emulate_gauss_jordan(G):
    """The in-place unpivoted Gauss-Jordan inverse of gram_backward_kernel in float32."""
    A = G.clone().float()
    d = A.shape[1]
    for k in range(d):
        p = 1.0 / A[:, k, k]
        rowk = A[:, k, :] * p[:, None]
        colk = A[:, :, k].clone()
        A = A - colk[:, :, None] * rowk[:, None, :]
        A[:, k, :] = rowk
        A[:, :, k] = -colk * p[:, None]
        A[:, k, k] = p
    return A


def emulate_backward(J, d, G32, ga, go, gd):
    """gram_backward_kernel in float32: M = 2 (ga G^-1 + (gd on / go off the diagonal) sign G), dJ = J M."""
    eye = torch.eye(d, dtype=torch.bool)
    sg = torch.sign(G32)
    M = 2.0 * (ga[:, None, None] * emulate_gauss_jordan(G32) + torch.where(eye, gd[:, None, None] * sg, go[:, None, None] * sg))
    return J[:, :, :d] @ M, M


def backward_store_map(nc, nr, mutant=False):
    """(slab row, 4-column group) of every store the product phase of gram_backward_kernel makes for a slab of ``nr`` rows, thread
    by thread; ``mutant``: the guard ``rg < rpp`` read as ``rg <= rpp``."""
    nq = nc // 4
    rpp = 256 // nq
    out = []
    for tid in range(256):
        q, rg = tid % nq, tid // nq
        if rg < rpp or (mutant and rg == rpp):
            out += [(r, q) for r in range(rg, nr, rpp)]
    return out


def swap_pair(d):
    """Two different columns < d inside one 16-column tile (the last tile that holds two)."""
    c1 = 16 * ((d - 1) // 16)
    if c1 == d - 1:
        c1 -= 16
    return c1, min(c1 + 5, d - 1)


def ratio(err, scale):
    """max err / scale over the elements (0 / 0 = 0, x / 0 = inf)."""
    err, scale = err.double().abs(), scale.double()
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# Device layouts
PAD = 64                                        # NaN floats in front of and behind the panel (256 bytes: keeps the base aligned)


class DevicePanel:
    """J (B, n_rows, nc) on the device inside a NaN-filled allocation.  ``layout``: 'guarded' (t_r = nc + 12, t_b = n_rows t_r + 20:
    NaN between rows and between samples), 'guarded2' (t_r = nc + 4, t_b = n_rows t_r + 36), 'panel' (contiguous
    [B][n_rows][nc]) or 'fmajor' (contiguous [n_rows][B][nc])."""

    def __init__(self, J, layout, fill=float("nan")):
        B, N, nc = J.shape
        self.B, self.N, self.nc, self.layout = B, N, nc, layout
        if layout == "guarded":
            self.t_r, self.t_b = nc + 12, N * (nc + 12) + 20
        elif layout == "guarded2":                                   # another pair of strides: the cotangent's dt_r, dt_b
            self.t_r, self.t_b = nc + 4, N * (nc + 4) + 36
        elif layout == "panel":
            self.t_r, self.t_b = nc, N * nc
        else:
            self.t_r, self.t_b = B * nc, nc
        span = (B - 1) * self.t_b + (N - 1) * self.t_r + nc
        host = torch.full((PAD + span + PAD,), fill)
        self.index = (PAD + torch.arange(B)[:, None, None] * self.t_b + torch.arange(N)[None, :, None] * self.t_r
                      + torch.arange(nc)[None, None, :])
        host[self.index.reshape(-1)] = J.reshape(-1)
        self.host = host
        self.raw = host.cuda()
        self.ptr = self.raw.data_ptr() + 4 * PAD
        assert self.ptr % 16 == 0 and self.t_r % 4 == 0 and self.t_b % 4 == 0

    def dense(self):
        """(B, n_rows, nc) read back from the device."""
        return self.raw.cpu()[self.index.reshape(-1)].view(self.B, self.N, self.nc)

    def untouched_outside(self):
        """True if every float outside the B x n_rows x nc payload still has its initial bits."""
        now, was = self.raw.cpu().view(torch.int32).clone(), self.host.view(torch.int32).clone()
        now[self.index.reshape(-1)] = 0
        was[self.index.reshape(-1)] = 0
        return bool(torch.equal(now, was))


class HeadOutputs:
    """jtj, logdet, l1_off, l1_diag (NaN-filled), info, fail (sentinel-filled) as views between guard bands."""
    SENTINEL = -0x5A5A5A5B

    def __init__(self, B, d):
        self.B, self.d = B, d
        self.jtj, self.logdet, self.l1_off, self.l1_diag = Guarded(B * d * d), Guarded(B), Guarded(B), Guarded(B)
        self.info, self.fail = Guarded(B, torch.int32, self.SENTINEL), Guarded(8, torch.int32, self.SENTINEL)

    def pointers(self):
        return [g.t.data_ptr() for g in (self.jtj, self.logdet, self.l1_off, self.l1_diag, self.info, self.fail)]

    def check_guards(self):
        for name in ("jtj", "logdet", "l1_off", "l1_diag", "info", "fail"):
            getattr(self, name).check(name)

    def read(self):
        return dict(jtj=self.jtj.t.cpu().view(self.B, self.d, self.d), logdet=self.logdet.t.cpu(), l1_off=self.l1_off.t.cpu(),
                    l1_diag=self.l1_diag.t.cpu(), info=self.info.t.cpu(), fail=self.fail.t.cpu())
