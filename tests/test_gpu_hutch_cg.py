"""The Hutchinson kernels per element against float64: the CG iterates and the stopping rule of ``cmf_hutch_cg`` (hutch_cg_kernel
for d, S <= 128, hutch_wide_kernel<1|4|16> above) against the float64 model of tests/_hutch_cg_reference.py on its whole case
list, and ``cmf_hutch_metric``, the narrow ``cmf_hutch_cotangent`` and ``cmf_hutch_lowrank_cotangent`` against plain float64
restatements.  Every call goes through ``cmf_amd.engine``.

Bounds of the CG test (per element; ``it`` = the iteration count of the element's work item, rho_item = the float32 yardstick of
that work item from the model's four summation orders, m = ``MARGIN`` = 4):
    |u - u64|  <= (m rho_item + (it + 2) 2^-24) max_k |u64_s|
    |w - w64|  <= (d + 1) 2^-24 (|G| |eps|)
    |val - mean_s sum_k u w of the kernel's own u, w| <= (d S + 1) 2^-24 sum |u w| / S,   and the model's value within that plus the
    u and w bounds propagated;  iters equal;  zero probe columns exact zeros;  everything finite.

Worst  |u - u64| / (rho_item max_k |u64_s|)  measured on the MI355X over the list: see ``test_cg_matches_the_float64_model``."""
import itertools

import pytest
import torch

import _hutch_cg_reference as R

pytestmark = pytest.mark.gpu

EPS32 = R.EPS32


def _run_cg(c):
    from cmf_amd import engine as E
    val, u, w, iters = E.hutch_cg(torch.from_numpy(c.G).cuda(), torch.from_numpy(c.eps).cuda(), c.max_iter, c.tol, c.min_iter)
    torch.cuda.synchronize()
    return val.cpu().numpy(), u.cpu().numpy(), w.cpu().numpy(), iters.cpu().numpy()


@pytest.mark.parametrize("name", list(R.cases()))
def test_cg_matches_the_float64_model(name):
    """``iters`` exactly, ``u``, ``w`` per element and ``val`` per sample within the bounds of the module docstring, on every case of
    the list: the production rule (tol 1, max_iter = d: the 11th iterate) at every width class of both kernels, tolerance, minimum
    count and cap stops, work items that mix fast and slow probes, zero probe columns and the zero matrix.

    Measured on the MI355X: the worst |u - u64| / (rho_item max_k |u64_s|) over the list is 1.54
    (small_d5_S3, where rho_item is 2.3e-7: four roundings of u), then 1.35 (default_d21_S130, the chunked wide kernel), 1.25
    (mixed_c_d100); 0.85 - 1.15 on most cases.  The kernels sit where the model's own summation orders sit, well inside m = 4."""
    c = R.cases()[name]
    val, u, w, iters = _run_cg(c)
    worst = R.check_outputs(name, val, u, w, iters)
    print(f"hutch_cg {name}: iters {iters.tolist()}, worst |u - u64| / (rho_item max|u64_s|) = {worst:.3f} (margin {R.MARGIN})")


def test_default_min_iter_is_the_default_of_the_launch():
    """``min_iter=None`` takes the documented default on the device too: the same outputs as passing ``default_min_iter``."""
    from cmf_amd import engine as E
    c = R.cases()["default_d65_S5"]
    G, eps = torch.from_numpy(c.G).cuda(), torch.from_numpy(c.eps).cuda()
    a = E.hutch_cg(G, eps, c.max_iter, c.tol)
    b = E.hutch_cg(G, eps, c.max_iter, c.tol, R.default_min_iter(c.max_iter))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[3].tolist() == [11, 11]


# ----------------------------------------------------------------------------------------------------------------------
# metric term and cotangents
# ----------------------------------------------------------------------------------------------------------------------


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _with_zeros(w):
    """A few entries exactly 0 and -0.0, on and off the diagonal of every sample."""
    w = w.clone()
    B, d, S = w.shape
    flat = w.view(B, -1)
    flat[:, 0] = 0.0                                                  # (0, 0): diagonal
    flat[:, -1] = -0.0                                                # (d - 1, S - 1): diagonal when S == d
    if d * S > 4:
        flat[:, 1 if S > 1 else 2] = -0.0
        flat[:, (d * S) // 2] = 0.0
    return w


@pytest.mark.parametrize("d,S", [(5, 5), (21, 40), (40, 21), (128, 128), (64, 1)])
def test_hutch_metric_per_sample(d, S):
    """l1_diag = sum_{k < min(d, S)} |W_kk| and (S = d only) l1_off = sum_{i != j} |W_ij| against float64 within
    (n + 1) 2^-24 sum |w|, n = d S (a float32 sum of n terms in any order); ``off`` is None unless S = d."""
    from cmf_amd import engine as E
    w = _randn(100 * d + S, 2, d, S)
    off, diag = E.hutch_metric(w.cuda())
    a = w.double().abs()
    bound = (d * S + 1) * EPS32 * a.sum((1, 2))
    want_diag = torch.diagonal(a, dim1=1, dim2=2).sum(1)
    assert bool(torch.isfinite(diag).all()) and bool(((diag.cpu().double() - want_diag).abs() <= bound).all()), (diag, want_diag)
    if S == d:
        assert bool(((off.cpu().double() - (a.sum((1, 2)) - want_diag)).abs() <= bound).all())
    else:
        assert off is None


@pytest.mark.parametrize("d,S", [(3, 3), (21, 40), (64, 17), (100, 100), (128, 128), (128, 1)])
def test_narrow_hutch_cotangent_per_element(d, S):
    """hutch_cotangent_kernel (d, S <= 128: two LDS panels [d][S + 1]) against  left eps^T  in float64, left = g_val / S u +
    (g_off [i != s] + g_diag [i == s]) sign(w), within (S + 2) 2^-24 (|left| |eps|^T) per element: S for the dot product, 2 for
    forming left.  Every admissible combination of the three cotangents being None (g_off needs S = d), with entries of w that are
    exactly 0 and -0.0 (sign 0)."""
    from cmf_amd import engine as E
    B = 2
    u, eps, w = _randn(7 * d + S, B, d, S), _randn(11 * d + S, B, d, S), _with_zeros(_randn(13 * d + S, B, d, S))
    g = _randn(17 * d + S, 3, B)
    sign = torch.sign(w.double())
    assert float(sign[0, 0, 0]) == 0.0 and float(sign[0, -1, -1]) == 0.0
    eye = torch.eye(d, S, dtype=torch.float64)
    ug, eg, wg = u.cuda(), eps.cuda(), w.cuda()
    for use in itertools.product((False, True), repeat=3):
        if use[1] and S != d:
            continue
        gv, go, gd = [g[i] if on else None for i, on in enumerate(use)]
        M = E.hutch_cotangent(ug, eg, wg, *[None if x is None else x.cuda() for x in (gv, go, gd)]).cpu().double()
        left = torch.zeros(B, d, S, dtype=torch.float64)
        if gv is not None:
            left += (gv.double() / S).view(B, 1, 1) * u.double()
        if go is not None:
            left += go.double().view(B, 1, 1) * (1.0 - eye) * sign
        if gd is not None:
            left += gd.double().view(B, 1, 1) * eye * sign
        want = left @ eps.double().transpose(1, 2)
        bound = (S + 2) * EPS32 * (left.abs() @ eps.double().abs().transpose(1, 2))
        err = (M - want).abs()
        assert bool(torch.isfinite(M).all()) and bool((err <= bound).all()), (use, float((err - bound).max()), float(err.max()))
        if not any(use):
            assert not bool(M.any())


@pytest.mark.parametrize("S", [1, 4, 12])
@pytest.mark.parametrize("diag", [False, True])
def test_lowrank_cotangent_is_the_sparse_matrix_of_the_header(S, diag):
    """C[s][S + s] = g_val / S (s < S) and, with g_diag, C[2 S + k][S + k] = g_diag sign(W_kk) (k < min(d, S)), zero elsewhere:
    exact equality (copies and one float32 division), with W_kk = 0 and -0.0 among the diagonal entries."""
    from cmf_amd import engine as E
    B, d = 3, 10
    w = _randn(50 + S, B, d, S)
    w[0, 0, 0] = 0.0
    if S > 1:
        w[1, 1, 1] = -0.0
    g_val, g_diag = _randn(60 + S, B), _randn(70 + S, B)
    K = min(d, S) if diag else 0
    n = 2 * S + K
    for gv in (g_val, None):
        C = E.hutch_lowrank_cotangent(w.cuda(), S, None if gv is None else gv.cuda(), g_diag.cuda() if diag else None).cpu()
        want = torch.zeros(B, n, n)
        for s in range(S):
            want[:, s, S + s] = 0.0 if gv is None else gv / torch.tensor(float(S))
        for k in range(K):
            want[:, 2 * S + k, S + k] = g_diag * torch.sign(w[:, k, k])
        assert C.shape == (B, n, n) and torch.equal(C, want)
