"""The data-space operator kernel (cmf_operator_apply_wrapped, csrc/operator_apply.hip) on the host: the fused pre-head
wrapper's inverse u and its derivative s in float64, the numpy float32 emulation of K = a diag(s) J -- ``_operator_apply_emulation``
with the one extra rounding of s J --, the seeded inputs the host and GPU tests share and the bounds they are held to (not collected
by pytest).

The wrapper is v = [logit](wa x + wc) with the triple (wa, wc, logit) as float32 values, which is what the kernel is given.  For a
head-space value v:  p = sigmoid(v) or v,  u = (p - wc) / wa,  s = du/dv = [p (1 - p)] / wa.  The float64 evaluation below goes
through e = exp(-|v|): p = 1 / (1 + e) or e / (1 + e) and p (1 - p) = e / (1 + e)^2.  The textbook p (1 - p) is the same number but
not the same float64: next to p = 1 the subtraction 1 - p keeps no more than the 2^-53 that 1 + e kept of e (at v = 30 a relative
1e-3), which is no reference for a 2^-23 bound.  tests/test_data_recovery_host.py holds the two forms together where both are good."""
import numpy as np

import _operator_apply_emulation as OA

#: (M, D, d) of tests/test_gpu_wrapped_operator.py, the smallest that reach every branch: one row more than a row tile; a row of a
#: that is not 16-byte aligned; D no multiple of either slab depth; C3's 13 row tiles at the shallow slab; two row groups; 17 row
#: tiles as groups of 9 and 8 over two column slabs
SHAPES = [(17, 64, 17), (1, 5, 3), (33, 1100, 33), (196, 784, 100), (300, 1100, 33), (260, 64, 128)]
BATCH = 3
#: the wrappers: mini_mnist's (scalar-mult 0.00390624, scalar-add 1e-6, logit) and one without a logit
TRIPLES = {"mini_mnist": (np.float32(0.00390624), np.float32(1e-6), 1), "affine": (np.float32(-2.5), np.float32(0.75), 0)}
IDENTITY = (np.float32(1.0), np.float32(0.0), 0)
#: the planted defects; "s_wrong_row" is one only where s varies from row to row: under a wrapper with a logit
DEFECTS = ("bf16", "s_dropped", "s_wrong_row")
#: x_hat is drawn uniformly from [-V_MAX, V_MAX]: s >= e^-30 / |wa| stays a normal float32
V_MAX = 30.0
# |K - K64| <= C_WRAPPED (|a| |s| |J|), elementwise, K64 = a diag(s64) J in float64.  tests/test_data_recovery_host.py measures the
# emulation's worst ratio on the inputs below over SHAPES and TRIPLES (2^-20.97, printed there); the constant is 4 x that, rounded up
# to a power of two -- the convention of C_OPERATOR -- and the host test re-measures it and asserts the equality.
C_WRAPPED = 2.0 ** -18
# What the float64 evaluation of u and the product a u add to the (D + 2) 2^-53 of ``OA.image_bound`` per term, in units of 2^-53
# |a| |u|: p carries 4 (exp within one unit in the last place: 2; 1 + e: 1; the division: 1), and the subtraction p - wc, the
# division by wa and the product with a -- no longer exact: u has 53 bits -- one each: 3.  The error of p passes the subtraction
# unreduced: 4 2^-53 p / |wa| <= 4 2^-53 (|u| + |wc / wa|), and sum |a| |wc / wa| <= sum |a| |u| on these inputs (next to p = wc a
# single u is small, a row's sum is not: the host test asserts it for every row), so it counts 4 + 4.
WRAPPER_OPS = 3 + 4 + 4


def wrapper64(v, triple):
    """(u, s) in float64 of the head-space values ``v`` under the wrapper ``triple``."""
    wa, wc, logit = float(triple[0]), float(triple[1]), int(triple[2])
    v = np.asarray(v, dtype=np.float64)
    if not logit:
        return (v - wc) / wa, np.full_like(v, 1.0 / wa)
    e = np.exp(-np.abs(v))
    p = np.where(v >= 0, 1.0, e) / (1.0 + e)
    return (p - wc) / wa, e / (1.0 + e) ** 2 / wa


def inputs(M, D, d, B=BATCH, seed=0):
    """(a (M, D), J (B, D, d), xhat (B, D)), float32: ``OA.inputs``' operator and Jacobian, and x_hat uniform in [-V_MAX, V_MAX]."""
    a, J, _ = OA.inputs(M, D, d, B=B, seed=seed)
    rng = np.random.default_rng(9000000 + 10000 * M + 10 * D + B + seed)
    return a, J, rng.uniform(-V_MAX, V_MAX, (B, D)).astype(np.float32)


def apply32(a, J, s, defect=None):
    """K (M, d) float32 = a (s J) of one sample: s (D,) float64 rounded to float32, every element of J times its row's s rounded to
    float32, then ``OA.apply32``.  ``defect``: "s_dropped" leaves J as it is, "s_wrong_row" takes s one row on, "bf16" rounds the
    operands of the products to bfloat16."""
    s32 = np.asarray(s, dtype=np.float64).astype(np.float32)
    if defect == "s_dropped":
        return OA.apply32(a, J)
    if defect == "s_wrong_row":
        s32 = np.roll(s32, 1)
    elif defect not in (None, "bf16"):
        raise ValueError(defect)
    return OA.apply32(a, s32[:, None] * np.asarray(J, dtype=np.float32), "bf16" if defect == "bf16" else None)


def apply64(a, J, s):
    """(K64, S): a diag(s) J and |a| |s| |J| of one sample in float64."""
    return OA.apply64(a, np.asarray(s, dtype=np.float64)[:, None] * np.asarray(J, dtype=np.float64))


def image64(a, u):
    """(yhat64, S): a u and |a| |u| of a batch u (B, D) float64, (B, M) each."""
    a64 = np.asarray(a, dtype=np.float64)
    return u @ a64.T, np.abs(u) @ np.abs(a64).T


def image_bound(y64, S, D):
    """|yhat - yhat64| <= 2^-24 |yhat64| + (D + 2 + WRAPPER_OPS) 2^-53 sum |a| |u|."""
    return 2.0 ** -24 * np.abs(y64) + (D + 2 + WRAPPER_OPS) * 2.0 ** -53 * S


def scale_bound(s64):
    """|scale - s64| <= 2^-23 |s64|: one float32 rounding (2^-24) of a float64 evaluation, doubled because a difference in the last
    place of the device's exp can carry the float64 value across a rounding boundary."""
    return 2.0 ** -23 * np.abs(s64)
