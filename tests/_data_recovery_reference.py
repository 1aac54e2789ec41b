"""The recovery loop of ``cmf_amd.ManifoldProjector.recover(..., space="data")`` in float64 on the oracle: the loop
of ``_recovery_reference.recover`` itself, run on the fixture's model seen from DATA space -- its decoder followed by the inverse
u of the pre-head wrapper, its Jacobian scaled row by row with s = du/dv, so that K = A diag(s) J and yhat = A u --, and the seeded
problems the host and GPU tests share (not collected by pytest)."""
import torch

import _recovery_reference as RR
from _recovery_reference import DATA_REL, pow2_ceil, rel_distance                # noqa: F401  (shared with the tests)

#: the fixture (D = 784, d = 4; the only known-answer fixture with a wrapper in front of its head), its batch and input shape
NAME, BATCH, SHAPE = "mini_mnist", 3, (1, 28, 28)
#: rows of the seeded Gaussian operator
M_GAUSSIAN = 32
# End-to-end tolerance of tests/test_gpu_data_recovery.py on ||u(g(z)) - u_on|| / ||u_on|| over all D data-space elements, built as
# ``RR.E2E_TOL`` is: tests/test_data_recovery_host.py measures on the float64 loop how far a perturbation of the measurements by
# DATA_REL ||y|| / sqrt(M) randn moves the recovered data-space point, worst sample per operator (printed there):
#   gaussian (M = 32) 7.390e-06, built (downsample 2 of a 3 x 3 box blur, M = 196) 1.059e-05
# and the tolerance is 4 x that, rounded up to a power of two.  The host test re-measures and asserts the factor of four.
DATA_E2E_TOL = {"gaussian": 2.0 ** -15, "built": 2.0 ** -14}


def triple(pre):
    """(wa, wc, logit) in float64 of the oracle's pre-head ops: v = [logit](wa x + wc); dequantisation is the identity at
    evaluation."""
    wa, wc, logit = 1.0, 0.0, False
    for op in pre:
        assert not logit, "nothing follows a logit in the image pre-processing chain"
        if op["kind"] == "scalar-mult":
            wa, wc = wa * op["value"], wc * op["value"]
        elif op["kind"] == "scalar-add":
            wc = wc + op["value"]
        elif op["kind"] == "logit":
            logit = True
        else:
            assert op["kind"] == "dequant", op["kind"]
    return wa, wc, logit


class DataModel:
    """A ``_projection_reference.Model`` seen from data space, with the interface ``RR.recover`` asks of a model.  ``wrapper``:
    the triple (wa, wc, logit) where it is not the model's own -- the GPU test has the product's and needs no model."""

    def __init__(self, model, wrapper=None):
        self.model = model
        self.wa, self.wc, self.logit = triple(model.pre) if wrapper is None else wrapper

    def to_head(self, x):
        v = self.wa * x + self.wc
        return torch.log(v) - torch.log1p(-v) if self.logit else v

    def wrapper(self, v):
        """(u, s) in float64 of the head-space tensor v: the data-space value and du/dv, through e = exp(-|v|) (see
        ``_wrapped_operator_emulation``)."""
        if not self.logit:
            return (v - self.wc) / self.wa, torch.full_like(v, 1.0 / self.wa)
        e = torch.exp(-v.abs())
        p = torch.where(v >= 0, torch.ones_like(e), e) / (1.0 + e)
        return (p - self.wc) / self.wa, e / (1.0 + e) ** 2 / self.wa

    def encode(self, x):
        return self.model.encode(self.to_head(x))

    def decode(self, z):
        return self.wrapper(self.model.decode(z))[0]

    def jacobian(self, z):
        """(None, u (B, *shape), diag(s) J (B, D, d)) at z."""
        _, x_hat, J = self.model.jacobian(z)
        u, s = self.wrapper(x_hat)
        return None, u, s.flatten(1)[:, :, None] * J


def built_operator():
    """downsample(2) of a 3 x 3 box blur on the fixture's shape: (196, 784) float32, on the CPU."""
    import cmf_amd
    return cmf_amd.downsample(SHAPE, 2) @ cmf_amd.blur(SHAPE, torch.full((3, 3), 1.0 / 9.0))


def operator(kind):
    return RR.gaussian_operator(M_GAUSSIAN, SHAPE[0] * SHAPE[1] * SHAPE[2]) if kind == "gaussian" else built_operator()


def start_input(dm, x_on):
    """The data-space input the recovery starts from: ``RR.start_input`` of the head-space point x_on, mapped to data space."""
    return dm.wrapper(RR.start_input(x_on).double())[0]


def known_answer(dm, kind, data_rel=0.0, steps=10):
    """(u_on, out): the data-space image of g(z_0) at the encoder's latent z_0 of the fixture's input, and ``RR.recover`` on y = A
    u_on (plus ``data_rel`` ||y|| / sqrt(M) randn) from the encoder's latent of ``start_input``.  ``out["reconstruction_head"]`` is
    the loop's x_hat: here the DATA-space reconstruction."""
    m = dm.model
    x_on = m.decode(m.encode(m.y)[:BATCH])
    u_on = dm.wrapper(x_on)[0]
    A = operator(kind).double()
    y = RR.measure(A, u_on, data_rel=data_rel)
    return u_on, RR.recover(dm, y, A, dm.encode(start_input(dm, x_on)), steps=steps)
