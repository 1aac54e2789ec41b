"""A numpy float64 model of the robust weights kernel (csrc/robust_weights.hip), the seeded inputs the host and GPU
tests share, and the checks the GPU test applies to the kernel's outputs (not collected by pytest).

The model does what the kernel does, operation by operation, in IEEE float64 (one rounded operation per multiply, add and divide:
the kernel is compiled without contraction): r = float64(x) - float64(xhat), exact; the lower median of |r| over the used elements
by a sort; s = 1.4826 med; u = r / s; omega and rho by the formulas of the header; w = float32(float64(prior) omega).

Bounds (u = 2^-53; m used elements, terms a_i = prior_i rho_i >= 0):
  scale, used, info: bit for bit -- an order statistic is one of the inputs' own |r|, and 1.4826 med is one rounded product.
  w: the model's value within 1 float32 ulp (the operations are the same; the ulp is room for a division that differs in its
    last bit).
  cost = 2 s^2 sum a_i: the kernel and the model add the same m non-negative terms in different orders.  A float64 sum of m terms
    in any order is within (m - 1) u sum |a_i| of the exact sum (first order), so two orders differ by at most 2 (m - 1) u sum a_i;
    the factor 2 s^2 is two more rounded products on either side, 4 u relative: 2 (m + 3) u sum a_i in all, the form of the
    weighted step's 2 (D + 3) u.  To that comes an allowance for terms that are not the same bits on both sides, 8 u kappa_i per
    term for its at most six rounded operations, with kappa_i = a_i for Huber (no cancellation: c |u| - c^2 / 2 >= c^2 / 2 outside
    c) and kappa_i = prior_i c^2 / 6 for Tukey (1 - t^3 cancels for small u: the error is absolute, relative to the factor in front):
        |cost - cost_model| <= 2 s^2 (2 (m + 3) u sum a_i + 8 u sum kappa_i).
  effective = sum omega_i, omega_i in [0, 1] with an absolute error of at most 4 u each:
        |effective - effective_model| <= 2 (m + 1) u sum omega_i + 8 u m.
A planted defect (tests/test_robust_host.py) moves these quantities by parts in ten, not in 10^15."""
import numpy as np

U = 2.0 ** -53
MAD_TO_SIGMA = 1.4826
TUNING = {"huber": 1.345, "tukey": 4.685}

SIZES = [1, 2, 3, 64, 255, 256, 257, 784, 1100, 3072]
BATCH = 11
PATTERNS = ("gauss", "ties", "zeros", "denormal", "signed_zero", "huge")
PRIORS = ("none", "third", "positive", "allzero")
DEFECTS = ("upper_median", "median_ignores_prior", "no_mad_factor", "psi_not_weight", "tukey_no_square", "cost_without_prior")


def sample(x, xhat, prior, loss, c, scale_in=None, defect=None):
    """One sample: (w (n,) float32, stats (4,) float64 = [s, cost, m, sum omega], info, (cost bound, effective bound))."""
    n = len(x)
    p = np.ones(n, dtype=np.float32) if prior is None else prior
    used = p > 0
    nan_w, nan4 = np.full(n, np.nan, dtype=np.float32), np.full(4, np.nan)
    with np.errstate(invalid="ignore"):
        bad = (~(p >= 0) | ~np.isfinite(p)).any() or (~np.isfinite(x[used])).any() or (~np.isfinite(xhat[used])).any()
    if bad:
        return nan_w, nan4, 2, (0.0, 0.0)
    r = x[used].astype(np.float64) - xhat[used].astype(np.float64)
    p64 = p[used].astype(np.float64)
    m = int(used.sum())
    if scale_in is not None:
        s = float(scale_in)
    else:
        a = np.sort(np.abs(r if defect != "median_ignores_prior" else x.astype(np.float64) - xhat.astype(np.float64)))
        rank = (len(a) - 1) // 2 if defect != "upper_median" else len(a) // 2
        s = np.float64(MAD_TO_SIGMA if defect != "no_mad_factor" else 1.0) * a[rank] if len(a) else np.float64("nan")
    if not (s > 0 and np.isfinite(s)):
        return nan_w, np.array([s, np.nan, np.nan, np.nan]), 3, (0.0, 0.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        u = r / s
        au = np.abs(u)
        if loss == "huber":
            inside = au <= c
            om = np.where(inside, 1.0, c / au)
            rho = np.where(inside, u * u / 2.0, c * au - c * c / 2.0)
            kappa = p64 * rho
        else:
            q = u / c
            t = np.maximum(1.0 - q * q, 0.0)
            om = t * t if defect != "tukey_no_square" else t
            rho = c * c / 6.0 * (1.0 - t * t * t)
            kappa = p64 * (c * c / 6.0)
        if defect == "psi_not_weight":
            om = om * u
    terms = p64 * rho if defect != "cost_without_prior" else rho
    total = float(terms.sum())
    w = np.zeros(n, dtype=np.float32)
    w[used] = (p64 * om).astype(np.float32)
    stats = np.array([s, 2.0 * s * s * total, float(m), float(om.sum())])
    bounds = (2.0 * s * s * (2 * (m + 3) * U * total + 8 * U * float(kappa.sum())), 2 * (m + 1) * U * float(np.abs(om).sum()) + 8 * U * m)
    return w, stats, 0, bounds


def batch(x, xhat, prior, loss, c, scale_in=None, defect=None):
    """``sample`` over a batch: (w (B, n), stats (B, 4), info (B,), bounds (B, 2))."""
    out = [sample(x[b], xhat[b], None if prior is None else prior[b], loss, c, None if scale_in is None else scale_in[b], defect)
           for b in range(len(x))]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out]))


def residual_pair(kind, n, gen):
    """(x, xhat) float32 (n,) of the residual pattern ``kind``; every pattern's residual x - xhat is exact in float32 arithmetic
    where the pattern needs it to be (ties, zeros)."""
    grid = lambda: (gen.integers(-256, 257, n) / 64.0).astype(np.float32)           # multiples of 1/64 in [-4, 4]
    if kind == "gauss":
        return gen.standard_normal(n).astype(np.float32), gen.standard_normal(n).astype(np.float32)
    if kind == "ties":                                                              # |r| in {0.5, 1, 1.5}: ties across the median rank
        xhat = grid()
        r = gen.choice([0.5, 1.0, 1.5], n) * gen.choice([-1.0, 1.0], n)
        return (xhat + r).astype(np.float32), xhat
    if kind == "zeros":                                                             # more than half exact zeros: a zero median
        xhat = grid()
        r = gen.standard_normal(n)
        r[gen.permutation(n)[:n // 2 + 1]] = 0.0
        return (xhat.astype(np.float64) + np.round(r * 64) / 64).astype(np.float32), xhat
    if kind == "denormal":                                                          # whole multiples of the smallest denormal
        tiny = np.float32(2.0 ** -149)
        return gen.integers(-1000, 1001, n).astype(np.float32) * tiny, gen.integers(-1000, 1001, n).astype(np.float32) * tiny
    if kind == "signed_zero":                                                       # 40 % zero residuals, written as +-0.0 - +-0.0
        x, xhat = gen.standard_normal(n).astype(np.float32), gen.standard_normal(n).astype(np.float32)
        z = gen.permutation(n)[:(2 * n) // 5]
        x[z] = gen.choice([-0.0, 0.0], len(z)).astype(np.float32)
        xhat[z] = gen.choice([-0.0, 0.0], len(z)).astype(np.float32)
        return x, xhat
    if kind == "huge":
        x, xhat = gen.standard_normal(n).astype(np.float32), gen.standard_normal(n).astype(np.float32)
        x[gen.integers(n)] = np.float32(3e30)
        return x, xhat
    raise ValueError(kind)


def prior_of(kind, B, n, gen):
    if kind == "none":
        return None
    if kind == "third":                                                             # 0 / 1, zero at a third of the elements
        p = np.ones((B, n), dtype=np.float32)
        for b in range(B):
            p[b, gen.permutation(n)[:(n + 2) // 3]] = 0.0
        return p
    if kind == "positive":
        return (0.25 + 3.75 * gen.random((B, n))).astype(np.float32)
    if kind == "allzero":
        return np.zeros((B, n), dtype=np.float32)
    raise ValueError(kind)


def inputs(n, prior_kind, seed=0, B=BATCH):
    """(x, xhat (B, n) float32, prior (B, n) float32 or None, scale (B,) float64 for the given-scale runs, pattern names)."""
    gen = np.random.default_rng([seed, n, PRIORS.index(prior_kind)])
    kinds = [PATTERNS[b % len(PATTERNS)] for b in range(B)]
    pairs = [residual_pair(k, n, gen) for k in kinds]
    x, xhat = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    scale = 0.25 + gen.random(B)
    for b, k in enumerate(kinds):
        if k == "denormal":
            scale[b] *= 2.0 ** -140
    return x, xhat, prior_of(prior_kind, B, n, gen), scale, kinds


def ulp_distance(a, b):
    """The distance in float32 units in the last place between the finite, same-signed arrays a and b (int64)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def mismatches(got, ref, prior):
    """The checks tests/test_gpu_robust.py applies to a kernel output ``got`` = (w, stats, info) against the model's ``ref`` =
    (w, stats, info, bounds): the list of (sample, what failed) -- empty when the output passes."""
    (w, stats, info), (w_ref, s_ref, i_ref, bounds) = got, ref
    out = []
    for b in range(len(info)):
        if info[b] != i_ref[b]:
            out.append((b, "info"))
            continue
        if not np.array_equal(stats[b, [0, 2]], s_ref[b, [0, 2]], equal_nan=True):
            out.append((b, "scale or used"))
        if i_ref[b] != 0:
            if not (np.isnan(w[b]).all() and np.isnan(stats[b, 1:]).all()):
                out.append((b, "NaN rows"))
            continue
        if not (np.isfinite(w[b]).all() and (np.signbit(w[b]) == np.signbit(w_ref[b])).all() and (ulp_distance(w[b], w_ref[b]) <= 1).all()):
            out.append((b, "w"))
        if prior is not None and not (w[b][prior[b] == 0].view(np.int32) == 0).all():
            out.append((b, "w where the prior is zero"))
        if not abs(stats[b, 1] - s_ref[b, 1]) <= bounds[b, 0]:
            out.append((b, "cost"))
        if not abs(stats[b, 3] - s_ref[b, 3]) <= bounds[b, 1]:
            out.append((b, "effective"))
    return out
