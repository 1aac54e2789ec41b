"""Host-side checks of the recovery in data space (no GPU): the float64 wrapper and its derivative against a central
difference, the numpy emulation of the wrapped operator kernel against float64 with the bound's constant and the planted defects it
must catch, the float64 reference loop on ``mini_mnist`` -- the conditions tests/test_gpu_data_recovery.py asserts of the product are
established here on the reference alone --, the data sensitivity its end-to-end tolerances are derived from, ``data_space_wrapper``
on synthetic chains, the operator builders against torch's own ops, and the ``space`` argument's refusal."""
import math

import numpy as np
import pytest
import torch

import _data_recovery_reference as DR
import _projection_reference as R
import _recovery_reference as RR
import _wrapped_operator_emulation as WO
from test_projection_host import small_density


@pytest.fixture(scope="module")
def dm():
    return DR.DataModel(R.Model(DR.NAME))


# --------------------------------------------------------------------------------------------------
# the wrapper in float64
# --------------------------------------------------------------------------------------------------


def test_wrapper_forms_agree_and_invert_the_pre_head(dm):
    """p (1 - p) through e = exp(-|v|) against the textbook form where that one is good (|v| <= 5: 1 - p >= 6e-3), and u against
    the forward wrapper; the fixture's triple is the one the issue names."""
    assert (dm.wa, dm.wc, dm.logit) == (pytest.approx(0.00390624, rel=1e-5), 1e-6, True)
    v = np.linspace(-5.0, 5.0, 2001)
    for triple in WO.TRIPLES.values():
        wa, wc, logit = float(triple[0]), float(triple[1]), triple[2]
        u, s = WO.wrapper64(v, triple)
        p = 1.0 / (1.0 + np.exp(-v)) if logit else v
        assert np.allclose(s, (p * (1.0 - p) if logit else 1.0) / wa, rtol=1e-13, atol=0.0)
        assert np.allclose(u, (p - wc) / wa, rtol=1e-13, atol=1e-13 * abs(wc / wa))
    vt = torch.linspace(-5.0, 5.0, 2001, dtype=torch.float64)
    u, s = dm.wrapper(vt)
    assert torch.allclose(dm.to_head(u), vt, rtol=0.0, atol=1e-9)
    un, sn = WO.wrapper64(vt.numpy(), (dm.wa, dm.wc, 1))
    assert np.allclose(u.numpy(), un, rtol=1e-14) and np.allclose(s.numpy(), sn, rtol=1e-14)
    assert WO.wrapper64(np.float32(1.7), WO.IDENTITY) == (np.float64(np.float32(1.7)), 1.0)


def test_reference_jacobian_matches_a_central_difference(dm):
    """The reference's own K = A diag(s) J against (f(z + h e_j) - f(z - h e_j)) / 2h of f(z) = A u(g(z)) in float64, per sample and
    latent direction in the max-norm over the M measurements.  The tolerance comes from the step: the truncation error of a central
    difference falls by four when the step is halved, so that of the step h is (D(2h) - D(h)) / 3 -- held with a factor of four --,
    and its rounding error is that of f, D 2^-53 sum |A| |u| for the D-term float64 sums, over h -- with a factor of four as well
    (g itself is a deep network; its own rounding is not modelled).  The decoder has kinks (relu), so the estimate is taken per
    direction.  The step is h = 2^-20: small, so that a kink seldom falls inside it and the one that does moves the quotient by
    less than the rounding term allows (at h = 2^-14 one of the twelve quotients misses the derivative by 9e-4 for that reason,
    the others by 1e-9); the tolerance is then the rounding bound, about 1e-3 of the derivative, and must stay below
    1 % of it for the check to mean something: a dropped or misplaced s is off by tens of per cent, which the last line shows."""
    m = dm.model
    z = m.encode(m.y)[:DR.BATCH]
    A = DR.operator("gaussian").double()
    f = lambda zz: RR.image(A, dm.decode(zz))
    _, u, SJ = dm.jacobian(z)
    K = torch.matmul(A, SJ)                                           # (B, M, d)
    h = 2.0 ** -20
    noise = 4 * u[0].numel() * 2.0 ** -53 * (u.abs().flatten(1) @ A.abs().T).max(dim=1).values / h
    worst = 0.0
    for j in range(z.shape[1]):
        e = torch.zeros_like(z)
        e[:, j] = 1.0
        d1 = (f(z + h * e) - f(z - h * e)) / (2 * h)
        d2 = (f(z + 2 * h * e) - f(z - 2 * h * e)) / (4 * h)
        tol = 4 * (d2 - d1).abs().max(dim=1).values / 3 + noise
        err = (K[:, :, j] - d1).abs().max(dim=1).values
        size = K[:, :, j].abs().max(dim=1).values
        worst = max(worst, float((err / tol).max()))
        assert bool((tol <= 1e-2 * size).all()), (j, (tol / size).tolist())
        assert bool((err <= tol).all()), (j, err.tolist(), tol.tolist())
        # without s the "derivative" is off by far more than the tolerance
        _, _, J = m.jacobian(z)
        assert bool(((torch.matmul(A, J)[:, :, j] - d1).abs().max(dim=1).values > 10 * tol).all())
    print(f"central difference, h = 2^-20: worst error / tolerance = {worst:.2e}")


# --------------------------------------------------------------------------------------------------
# the emulation and the bound's constant
# --------------------------------------------------------------------------------------------------


def test_wrapped_constant_and_planted_defects():
    """C_WRAPPED is 4 x (rounded up to a power of two) the emulation's worst error on the GPU test's own inputs, and the emulation
    with a planted defect lands above it on every sample (a misplaced s only where s varies: under the logit)."""
    worst, least = 0.0, {k: math.inf for k in WO.DEFECTS}
    for triple in WO.TRIPLES.values():
        for M, D, d in WO.SHAPES:
            a, J, xhat = WO.inputs(M, D, d)
            _, s = WO.wrapper64(xhat, triple)
            assert (np.abs(s).astype(np.float32) >= np.finfo(np.float32).tiny).all()      # a normal float32
            for b in range(WO.BATCH):
                K64, S = WO.apply64(a, J[b], s[b])
                assert (S > 0).all()
                worst = max(worst, WO.OA.ratio(WO.apply32(a, J[b], s[b]), K64, S))
                for defect in WO.DEFECTS:
                    if defect == "s_wrong_row" and not triple[2]:
                        continue
                    least[defect] = min(least[defect], WO.OA.ratio(WO.apply32(a, J[b], s[b], defect), K64, S))
    print(f"emulation against float64: worst |K - K64| / (|a| |s| |J|) = 2^{math.log2(worst):.2f} (C_WRAPPED = "
          f"2^{math.log2(WO.C_WRAPPED):g}); planted defects, least: " + ", ".join(f"{k} 2^{math.log2(v):.2f}" for k, v in least.items()))
    assert WO.C_WRAPPED == DR.pow2_ceil(4 * worst)
    assert all(v > WO.C_WRAPPED for v in least.values())


def test_identity_triple_is_the_plain_emulation():
    a, J, xhat = WO.inputs(17, 64, 17)
    u, s = WO.wrapper64(xhat, WO.IDENTITY)
    assert np.array_equal(u, xhat.astype(np.float64)) and (s == 1.0).all()
    assert np.array_equal(WO.apply32(a, J[0], s[0]), WO.OA.apply32(a, J[0]))


def test_image_bound_and_what_its_constant_assumes():
    """A float32 rounding of the float64 sum is inside the bound, and on the GPU test's inputs sum |a| |wc / wa| <= sum |a| |u| for
    every row: what lets the error of p, which the subtraction p - wc does not reduce, count as 4 more units (WO.WRAPPER_OPS)."""
    share = 0.0
    for triple in WO.TRIPLES.values():
        for M, D, d in WO.SHAPES:
            a, _, xhat = WO.inputs(M, D, d)
            u, _ = WO.wrapper64(xhat, triple)
            y64, S = WO.image64(a, u)
            rounded = y64.astype(np.float32).astype(np.float64)
            assert (np.abs(rounded - y64) <= WO.image_bound(y64, S, D)).all()
            offset = abs(float(triple[1]) / float(triple[0])) * np.abs(a.astype(np.float64)).sum(1)
            share = max(share, float((offset[None, :] / S).max()))
    print(f"worst sum |a| |wc / wa| / sum |a| |u| = {share:.3e}")
    assert share <= 1.0


# --------------------------------------------------------------------------------------------------
# the float64 reference loop in data space
# --------------------------------------------------------------------------------------------------


def test_reference_loop_finds_the_known_answer(dm):
    """y = A u(g(z_0)), seeded Gaussian A with M = 32: ten steps from the encoder's latent of ``RR.start_input`` bring the
    data-space relative error down by at least 10^6, every sample."""
    m = dm.model
    x_on = m.decode(m.encode(m.y)[:DR.BATCH])
    u_on, out = DR.known_answer(dm, "gaussian")
    start = DR.rel_distance(dm.decode(dm.encode(DR.start_input(dm, x_on))), u_on)
    rel = DR.rel_distance(out["reconstruction_head"], u_on)
    print(f"{DR.NAME}: M = {DR.M_GAUSSIAN}: ||u - u_on|| / ||u_on|| {start.tolist()} -> {rel.tolist()}; accepted "
          f"{out['accepted'].tolist()}; cost {out['initial_cost'].tolist()} -> {out['cost'].tolist()}; data values "
          f"{float(u_on.min()):.3g} .. {float(u_on.max()):.3g}")
    assert bool((rel * 1e6 <= start).all())
    assert bool((out["info"] == 0).all()) and bool((out["costs"][1:] <= out["costs"][:-1]).all())
    assert torch.equal(out["reconstruction_head"], dm.decode(out["latent"]))
    assert torch.equal(out["measurement"], RR.image(DR.operator("gaussian").double(), out["reconstruction_head"]))


@pytest.mark.parametrize("kind", list(DR.DATA_E2E_TOL))
def test_data_sensitivity_sets_the_gpu_tolerance(kind, dm):
    """How far a DATA_REL perturbation of the measurements moves the recovered data-space point: the measurement the GPU end-to-end
    tolerance ``DR.DATA_E2E_TOL`` is 4 x (rounded up to a power of two) of.  The unperturbed loop reaches the answer for both
    operators."""
    u_on, clean = DR.known_answer(dm, kind)
    assert float(DR.rel_distance(clean["reconstruction_head"], u_on).max()) <= 1e-11 and bool((clean["info"] == 0).all())
    u_on, out = DR.known_answer(dm, kind, data_rel=DR.DATA_REL)
    worst = float(DR.rel_distance(out["reconstruction_head"], u_on).max())
    print(f"{kind}: worst ||u - u_on|| / ||u_on|| under a {DR.DATA_REL:g} measurement perturbation = {worst:.3e}; "
          f"DATA_E2E_TOL = 2^{math.log2(DR.DATA_E2E_TOL[kind]):g} = {DR.DATA_E2E_TOL[kind]:.3e}")
    assert bool((out["info"] == 0).all())
    assert DR.DATA_E2E_TOL[kind] == DR.pow2_ceil(4 * worst)


# --------------------------------------------------------------------------------------------------
# data_space_wrapper
# --------------------------------------------------------------------------------------------------


def test_data_space_wrapper_on_the_image_chain():
    """The mnist configuration's chain gives the triple the density's own fused pre-head gives."""
    import cmf_amd
    from cmf_amd.densities import BijectionDensity
    from cmf_amd.projection import data_space_wrapper
    dens = small_density("mnist", g_hidden_channels=[8], latent_dimension=4)
    proj = cmf_amd.ManifoldProjector(dens)
    fused = next(f for f in (n._fused_prehead() for n in dens.modules() if isinstance(n, BijectionDensity)) if f is not None)
    assert fused[3] is proj.head and fused[2]
    wa, wc, logit, perm = data_space_wrapper(proj.chain)
    assert (wa, wc, logit) == fused[:3] and logit is True and perm is None


def test_data_space_wrapper_on_synthetic_chains():
    from cmf_amd import bijections as Bj
    from cmf_amd.projection import data_space_wrapper
    shape = (2, 4, 6)
    assert data_space_wrapper([]) == (1.0, 0.0, False, None)
    mult, add, logit = Bj.ScalarMultiplicationBijection(shape, 0.25), Bj.ScalarAdditionBijection(shape, 0.5), Bj.LogitBijection(shape)
    assert data_space_wrapper([mult, add]) == (0.25, 0.5, False, None)
    assert data_space_wrapper([add, mult]) == (0.25, 0.125, False, None)          # 0.25 (x + 0.5)
    assert data_space_wrapper([mult, add, logit, Bj.ViewBijection(shape, (48,))]) == (0.25, 0.5, True, None)
    for after in (mult, add, Bj.LogitBijection(shape)):
        with pytest.raises(NotImplementedError, match=type(after).__name__):
            data_space_wrapper([mult, logit, after])
    with pytest.raises(NotImplementedError, match="AffineBijection"):
        data_space_wrapper([mult, Bj.AffineBijection(shape)])
    # a squeeze: head element r is data element perm[r], the map its own x_to_z applies to data
    squeeze = Bj.Squeeze2dBijection(shape, 2)
    wa, wc, lg, perm = data_space_wrapper([mult, squeeze, add])
    assert (wa, wc, lg) == (0.25, 0.5, False) and perm.dtype == torch.int64 and perm.shape == (48,)
    x = torch.randn(3, *shape, generator=torch.Generator().manual_seed(0))
    z = squeeze._reshape_x(x)
    assert z.shape == (3, 8, 2, 3) and torch.equal(x.flatten(1)[:, perm], z.flatten(1))
    # ... so that A[:, perm] acts on the head-ordered elements as A acts on the data
    A = torch.randn(5, 48, generator=torch.Generator().manual_seed(1))
    assert torch.equal(z.flatten(1) @ A[:, perm].T, z.flatten(1) @ A.index_select(1, perm).T)
    assert torch.allclose(z.flatten(1).double() @ A[:, perm].double().T, x.flatten(1).double() @ A.double().T, rtol=0, atol=1e-12)
    # two squeezes compose; a squeeze by 1 is the flat order itself
    second = Bj.Squeeze2dBijection((8, 2, 3), 1)
    assert data_space_wrapper([second])[3] is None
    wide = Bj.Squeeze2dBijection((1, 4, 4), 2)
    again = Bj.Squeeze2dBijection((4, 2, 2), 2)
    perm2 = data_space_wrapper([wide, again])[3]
    x = torch.randn(2, 1, 4, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(x.flatten(1)[:, perm2], again._reshape_x(wide._reshape_x(x)).flatten(1))


# --------------------------------------------------------------------------------------------------
# the operator builders
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape,ksize", [((1, 28, 28), (3, 3)), ((3, 8, 10), (3, 5)), ((2, 5, 4), (1, 1)), ((1, 3, 3), (5, 7))])
def test_blur_is_conv2d_per_channel(shape, ksize):
    import cmf_amd
    from cmf_amd import operators
    assert cmf_amd.blur is operators.blur and cmf_amd.downsample is operators.downsample
    gen = torch.Generator().manual_seed(10 * shape[1] + ksize[1])
    kernel = torch.randn(ksize, generator=gen)
    x = torch.randn(4, *shape, generator=gen)
    A = cmf_amd.blur(shape, kernel)
    D = shape[0] * shape[1] * shape[2]
    assert A.shape == (D, D) and A.dtype == torch.float32 and A.is_contiguous()
    want = torch.nn.functional.conv2d(x.double().view(-1, 1, *shape[1:]), kernel.double()[None, None],
                                      padding=(ksize[0] // 2, ksize[1] // 2)).view(4, *shape)
    got = (x.flatten(1).double() @ A.double().T).view(4, *shape)
    assert torch.allclose(got, want, rtol=0.0, atol=1e-12 * float(want.abs().max()))


@pytest.mark.parametrize("shape,factor", [((1, 28, 28), 2), ((3, 8, 12), 4), ((2, 6, 4), 1)])
def test_downsample_is_avg_pool2d(shape, factor):
    import cmf_amd
    x = torch.randn(4, *shape, generator=torch.Generator().manual_seed(shape[2] + factor))
    A = cmf_amd.downsample(shape, factor)
    C, H, W = shape
    assert A.shape == (C * (H // factor) * (W // factor), C * H * W) and A.dtype == torch.float32 and A.is_contiguous()
    want = torch.nn.functional.avg_pool2d(x.double(), factor)
    got = (x.flatten(1).double() @ A.double().T).view_as(want)
    assert torch.allclose(got, want, rtol=0.0, atol=1e-12 * float(want.abs().max()))


def test_builder_refusals():
    import cmf_amd
    with pytest.raises(ValueError, match="odd"):
        cmf_amd.blur((1, 4, 4), torch.ones(2, 3))
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        cmf_amd.blur((4, 4), torch.ones(3, 3))
    with pytest.raises(ValueError, match="divides"):
        cmf_amd.downsample((1, 6, 4), 3)
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        cmf_amd.downsample((6, 4), 2)


# --------------------------------------------------------------------------------------------------
# the public method
# --------------------------------------------------------------------------------------------------


def test_recover_refuses_an_unknown_space():
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(small_density())
    A, y = torch.zeros(4, 6), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="space must be 'head' or 'data'"):
        proj.recover(y, A, space="bogus")
    # a known space goes on to the usual checks: every argument in order and nothing on the GPU
    for space in ("head", "data"):
        with pytest.raises(ValueError, match="no CPU fallback"):
            proj.recover(y, A, space=space)
    with pytest.raises(ValueError, match=r"operator must be a contiguous float32 \(M, 6\)"):
        proj.recover(y, torch.zeros(4, 5), space="data")
