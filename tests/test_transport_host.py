"""Parallel transport on the CPU: the conditions the GPU tests assert of the product, established for the float64
reference (tests/_transport_reference.py) alone on the oracle, and the numpy emulation of the kernel's arithmetic
(tests/_transport_emulation.py) held to a quarter of the kernel's solve bounds on the inputs the GPU tests use.

Curves: ``_geodesic_reference.connect`` (10 steps) between the fixtures' own ends; vectors: the ``log`` velocity of the 9-point
curve and two seeded normal vectors.  Reached on this reference (the bound in brackets):
    (a) end vector in the head's input space against P = 33, P = 5 / 9 / 17: sphere 1.4e-3 / 3.4e-4 / 6.8e-5, power 6.6e-5 /
        1.6e-5 / 3.3e-6, hepmass 7.7e-5 / 1.9e-5 / 3.8e-6; ratios 0.24 - 0.25 and 0.20 (<= 1/3)
    (b) norm2 drift at P = 9: 1.4e-4, 3.4e-7, 1.9e-8, mini_mnist 5.8e-4, mini_cifar 1.0e-4 (<= 2e-3); P = 17 over P = 9 on the
        MLPs 0.13 (<= 1/4); the projection-only scheme drifts by 4.8e-2 on the sphere, 5.8e-2 on mini_mnist
    (c) forth and back at P = 9: 1.3e-4, 5.2e-7, 2.0e-8, 1.1e-3, 8.4e-5 (<= 3e-3)
    (d) the transported log velocity against the one-sided end difference at P = 17: 2.6e-3, 8.4e-4, 1.6e-3, 3.2e-3, 4.6e-3 (<= 1e-2)
    (e) a curve of identical points: <= 2e-15 (<= 1e-12)
Emulation (u = 2^-53): forward residual <= 0.67 d u scale (a quarter of 32 is 8), backward <= 0.56 d u scale (a quarter of 64 is
16): the doubled band-solve constant stays.  norm2 is held to its a-priori bound 2 (d + 2) u sum |terms| itself -- the rounding
error of a sum of d^2 products of three factors in this order is up to (2 d + 1) u sum |terms|, more than a quarter of the bound at
every d (reached: 3.2 u at d = 3), so no implementation of the sum can be held to a quarter."""
import numpy as np
import pytest
import torch

import _transport_emulation as M
import _transport_reference as T


# --------------------------------------------------------------------------------------------------
# the scheme, in float64 on the oracle
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", T.MLP)
def test_the_scheme_is_second_order(name):
    w0 = T.run(name, 9)[2]                                           # one set of vectors for every P
    ends = {}
    for P in (5, 9, 17, 33):
        model, z = T.relaxed(name, P)
        ends[P] = T.head_space(T.transport(model, z, w0))
    dev = {P: T.rel(ends[P], ends[33]) for P in (5, 9, 17)}
    print(f"{name}: deviation from P = 33: {dev[5]:.2e} / {dev[9]:.2e} / {dev[17]:.2e}; ratios {dev[9] / dev[5]:.3f}, "
          f"{dev[17] / dev[9]:.3f}")
    assert dev[9] <= dev[5] / 3.0 and dev[17] <= dev[9] / 3.0


@pytest.mark.parametrize("name", T.FIXTURES)
def test_metric_norms_are_kept(name):
    model, z, w0, out = T.run(name, 9)
    d9 = T.drift(out)
    _, pn = T.project_only(model, z, w0)
    print(f"{name}: drift at P = 9 {d9:.2e} (projection only {float((pn / pn[:, :1] - 1.0).abs().max()):.2e})")
    assert d9 <= 2e-3
    assert out["vectors"].shape == z.shape + (3,) and out["forward"].shape == (z.shape[0], 8, z.shape[2], 3)
    assert torch.equal(out["vectors"][:, 0], w0) and torch.equal(out["transported"], out["vectors"][:, -1])
    assert torch.equal(out["vectors"][:, 1:], 0.5 * (out["forward"] + out["backward"]))
    if name in T.MLP:
        d17 = T.drift(T.run(name, 17)[3])
        print(f"{name}: drift at P = 17 {d17:.2e}, ratio {d17 / d9:.3f}")
        assert d17 <= d9 / 4.0


@pytest.mark.parametrize("name", T.FIXTURES)
def test_forth_and_back_returns_the_vector(name):
    model, z, w0, out = T.run(name, 9)
    err = T.forth_and_back(model, z, w0, out)
    print(f"{name}: forth and back {err:.2e}")
    assert err <= 3e-3


@pytest.mark.parametrize("name", T.FIXTURES)
def test_a_geodesics_own_velocity_is_parallel(name):
    model, z, w0, out = T.run(name, 17)
    err = T.own_velocity_error(out, z)
    print(f"{name}: transported log velocity against the end difference {err:.2e}")
    assert err <= 1e-2


@pytest.mark.parametrize("name", T.FIXTURES)
def test_a_curve_of_one_point_transports_nothing(name):
    model, z, w0, _ = T.run(name, 9)
    out = T.transport(model, z[:, :1].expand(-1, 9, -1).contiguous(), w0)
    err = T.rel(out["transported"], w0)
    print(f"{name}: zero-length curve {err:.2e}")
    assert err <= 1e-12
    assert T.rel(out["norm2"], out["norm2"][:, :1].expand_as(out["norm2"])) <= 1e-12


# --------------------------------------------------------------------------------------------------
# the emulation of the kernel
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", M.WIDTHS)
def test_emulation_stays_within_a_quarter_of_the_solve_bounds(d):
    for curves, P, m in ((1, 2, 1), (3, 3, 3), (3, 5, 16)):
        jtj, cross, w0 = M.case(curves, P, d, m)
        out, fwd, bwd, norm2, info = M.chain(jtj, cross, w0, P)
        assert (info == 0).all()
        assert np.array_equal(out[:, 0], w0) and np.array_equal(out[:, 1:], 0.5 * (fwd + bwd))
        rf, rb, rn = M.residual_ratios(jtj, cross, out, fwd, bwd, norm2, P)
        print(f"d={d} curves={curves} P={P} m={m}: forward {rf:.3f} (bound {M.FWD_CONSTANT / 4}), backward {rb:.3f} "
              f"(bound {M.BWD_CONSTANT / 4}), norm2 {rn:.3f} u (bound {2 * (d + 2)})")
        assert rf <= M.FWD_CONSTANT / 4.0 and rb <= M.BWD_CONSTANT / 4.0
        assert rn <= 2 * (d + 2)
        if d > 1:                                                    # the planes really turn: the halves differ
            assert np.abs(fwd - bwd).max() > 1e-6 * np.abs(out).max()


def test_emulation_pivots_like_a_reference_solver():
    rng = np.random.default_rng(3)
    for d in (2, 7, 33):
        C, rhs = rng.standard_normal((d, d)), rng.standard_normal((4, d))
        C[0, 0] = 0.0                                                # an elimination without pivoting stops here
        assert np.allclose(M.lu_solve(C, rhs), np.linalg.solve(C, rhs.T).T, rtol=1e-9, atol=1e-12)
    assert M.lu_solve(np.zeros((1, 1)), np.ones((1, 1))) is None
    assert M.lu_solve(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones((1, 2))) is None
    G = np.array([[4.0, np.nan], [2.0, 3.0]])                        # the strict upper triangle is not looked at
    assert np.allclose(M.chol_solve(G, np.array([[1.0, 2.0]])), np.linalg.solve(np.array([[4.0, 2.0], [2.0, 3.0]]), [1.0, 2.0]))
    assert M.chol_solve(np.array([[1.0, 0.0], [2.0, 4.0]]), np.ones((1, 2))) is None


def test_emulation_known_answers_and_failure_codes():
    for d in (3, 16):
        J, inverse, _ = M.same_plane(d, 5)
        jtj, cross = M.blocks(J)
        w0 = np.random.default_rng(d).integers(-3, 4, (1, 3, d)).astype(np.float64)
        out, fwd, bwd, norm2, info = M.chain(jtj, cross, w0, 5)
        assert info[0] == 0
        want = w0[0]
        for i in range(4):
            want = want @ inverse[i].T
        assert np.allclose(out[0, -1], want, rtol=0, atol=1e-6 * np.abs(want).max())
        assert np.allclose(norm2[0], norm2[0, 0], rtol=1e-6)
    J, Pi = M.pivoting_case()
    jtj, cross = M.blocks(J)
    assert cross[0, 0, 0] == 0.0
    w0 = np.arange(15.0).reshape(1, 3, 5) - 7.0
    out, _, _, _, info = M.chain(jtj, cross, w0, 2)
    assert info[0] == 0 and np.allclose(out[0, 1], w0[0] @ Pi[0], rtol=0, atol=1e-12)
    J, w0, ratio, kappa = M.turned_planes(6, 4)
    jtj, cross = M.blocks(J)
    out, _, _, norm2, info = M.chain(jtj, cross, w0, 4)
    assert info[0] == 0
    assert np.abs(norm2[0, 1:] / norm2[0, :-1] / ratio[None] - 1.0).max() <= 16 * kappa * np.sqrt(6) * 2.0 ** -24
    # failures: a zero Jacobian column at point 2 of curve 1; NaN in the vectors of curve 2
    Jf = M.jacobians(3, 5, 4)
    Jf[1, 2, :, 1] = 0.0
    jtj, cross = M.blocks(Jf)
    w0 = M.vectors(3, 2, 4)
    w0[2, 1, 3] = np.nan
    out, fwd, bwd, norm2, info = M.chain(jtj, cross, w0, 5)
    assert info.tolist() == [0, 1, 2]
    assert np.isfinite(out[1, :2]).all() and np.isnan(out[1, 2:]).all() and np.isfinite(norm2[1, :2]).all()
    assert np.isfinite(fwd[1, 0]).all() and np.isnan(fwd[1, 1:]).all() and np.isnan(bwd[1, 1:]).all() and np.isnan(norm2[1, 2:]).all()
    assert np.isnan(out[2]).all() and np.isnan(fwd[2]).all() and np.isnan(norm2[2]).all()


def test_the_entry_point_is_declared():
    from cmf_amd import _lib
    assert "cmf_transport_chain" in _lib.SIGNATURES and len(_lib.SIGNATURES["cmf_transport_chain"][1]) == 13
    import cmf_amd
    for method in ("transport_latents", "transport", "analogy"):
        assert callable(getattr(cmf_amd.ManifoldGeodesic, method))
