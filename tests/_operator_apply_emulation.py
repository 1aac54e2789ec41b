"""A numpy float32 emulation of the operator kernel (csrc/operator_apply.hip) -- K = a J with fp32 products and fp32
accumulation, four terms of the sum over D at a time as the MFMA takes them -- the seeded inputs the host and GPU tests share, and
the error ratio their bound is stated in (not collected by pytest).  The emulation and the kernel agree to rounding, not bit for
bit: the hardware runs one chain of fused multiply-adds in the order of D, the emulation rounds every product and sums four at a
time -- another summation order and FMA contraction, which the factor of four in C_OPERATOR is there to absorb."""
import numpy as np

import _gn_step_emulation as GN

#: (M, D, d) of tests/test_gpu_recovery.py: a single row and a row of a that is not 16-byte aligned (D = 5), M = D, one row more
#: than a row tile, whole tiles, the C3 shapes (one row group up to M = 256, four at M = 784), D no multiple of the slab depth
SHAPES = [(1, 5, 3), (5, 5, 1), (17, 64, 17), (16, 64, 16), (100, 784, 64), (196, 784, 100), (784, 784, 128), (33, 1100, 33)]
BATCH = 3
# |K - K64| <= C_OPERATOR (|a| |J|), elementwise.  tests/test_recovery_host.py measures the emulation's worst ratio on the inputs
# below over SHAPES (2^-22.61, printed there); the constant is 4 x that, rounded up to a power of two -- the factor of four absorbs
# another summation order and FMA contraction (the convention of tests/_gram_head.py) -- and the host test re-measures it and asserts
# the equality.  It never comes from the kernel's output.
C_OPERATOR = 2.0 ** -20
DEFECTS = ("bf16", "dropped", "transposed")


def operator(M, D, seed=0):
    """The seeded operator a (M, D) float32: Gaussian, scaled by 1 / sqrt(D)."""
    rng = np.random.default_rng(7000000 + 10000 * M + 10 * D + seed)
    return (rng.standard_normal((M, D)) / np.sqrt(D)).astype(np.float32)


def inputs(M, D, d, B=BATCH, seed=0):
    """(a (M, D), J (B, D, d), xhat (B, D)), float32: ``GN.inputs``' Jacobian and x_hat, and the seeded operator."""
    J, _, _, xhat = GN.inputs(B, D, d, seed=seed)
    return operator(M, D, seed), J, xhat


def bf16(v):
    """float32 values rounded to bfloat16 (to nearest even), as float32."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    bits = (bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return bits.view(np.float32)


def apply32(a, J, defect=None):
    """K (M, d) float32 = a J of one sample: fp32 products, summed four at a time in fp32, the groups accumulated in fp32 in the
    order of D.  ``defect``: "bf16" rounds both operands to bfloat16, "dropped" leaves out the term D // 2 of every sum,
    "transposed" applies a^T (M == D)."""
    a, J = np.asarray(a, dtype=np.float32), np.asarray(J, dtype=np.float32)
    if defect == "bf16":
        a, J = bf16(a), bf16(J)
    elif defect == "dropped":
        a = a.copy()
        a[:, a.shape[1] // 2] = 0.0
    elif defect == "transposed":
        assert a.shape[0] == a.shape[1]
        a = np.ascontiguousarray(a.T)
    elif defect is not None:
        raise ValueError(defect)
    M, D = a.shape
    pad = -D % 4
    if pad:
        a = np.concatenate((a, np.zeros((M, pad), dtype=np.float32)), axis=1)
        J = np.concatenate((J, np.zeros((pad, J.shape[1]), dtype=np.float32)), axis=0)
    acc = np.zeros((M, J.shape[1]), dtype=np.float32)
    for i in range(0, D + pad, 4):
        p = a[:, i:i + 4, None] * J[None, i:i + 4, :]               # (M, 4, d) float32 products
        acc = acc + ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]))
    return acc


def apply64(a, J):
    """(K64, S): a J and |a| |J| of one sample in float64."""
    a64, J64 = np.asarray(a, dtype=np.float64), np.asarray(J, dtype=np.float64)
    return a64 @ J64, np.abs(a64) @ np.abs(J64)


def ratio(K, K64, S):
    """max |K - K64| / S over the elements (S > 0 on these inputs): to be held against C_OPERATOR."""
    return float((np.abs(np.asarray(K, dtype=np.float64) - K64) / S).max())


def image64(a, xhat):
    """(yhat64, S): a xhat and |a| |xhat| of a batch (B, D) in float64, (B, M) each."""
    a64, x64 = np.asarray(a, dtype=np.float64), np.asarray(xhat, dtype=np.float64)
    return x64 @ a64.T, np.abs(x64) @ np.abs(a64).T


def image_bound(y64, S, D):
    """|yhat - yhat64| <= 2^-24 |yhat64| + (D + 2) 2^-53 sum |a| |xhat|: one rounding to float32 of a float64 sum of D exact
    products."""
    return 2.0 ** -24 * np.abs(y64) + (D + 2) * 2.0 ** -53 * S
