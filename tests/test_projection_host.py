"""Host-side checks of the manifold projection (no GPU): the numpy emulation of the Gauss-Newton step kernel against
float64 torch, the float64 reference loop on the fixtures -- the conditions tests/test_gpu_projection.py asserts of the product are
established here on the reference alone -- and the refusals of the public API.

Emulation bound: ||A delta - g||_inf <= 8 d 2^-53 (||A||_inf ||delta||_inf + ||g||_inf), a quarter of the kernel's (BOUND_C / 4), as
tests/test_metric_spectrum_host.py holds the Jacobi emulation to a quarter of its kernel's."""
import numpy as np
import pytest
import torch

import _gn_step_emulation as GN
import _projection_reference as R

SMOOTH = ["c2a_power", "c2b_hepmass", "c1_sphere_d2"]               # tanh MLP couplers: Gauss-Newton converges quadratically
KINKED = ["mini_mnist", "mini_mnist_small", "mini_cifar"]           # relu ResNet couplers: it stalls at kinks
KNOWN_ANSWER = ["c2b_hepmass", "c2a_power", "mini_mnist"]
#: the GPU test's tolerance on the known answer: 2 (1e-5 ||x_on||) / rho with rho = 0.1 ||x_on||
TAU = 2e-4


@pytest.mark.parametrize("d", GN.WIDTHS)
@pytest.mark.parametrize("D", GN.ROWS)
def test_emulation_solves_the_damped_normal_equations(D, d):
    J, G, x, xhat = GN.inputs(len(GN.DAMPINGS), D, d)
    lam = np.array(GN.DAMPINGS)
    grad, delta, stats, info = GN.batch(J, G, x, xhat, lam)
    r = x.astype(np.float64) - xhat.astype(np.float64)
    for b, lb in enumerate(GN.DAMPINGS):
        g_ref = J[b].astype(np.float64).T @ r[b]
        assert np.abs(grad[b] - g_ref).max() <= 2 * (D + 2) * GN.U * (np.abs(J[b].astype(np.float64)).T @ np.abs(r[b])).max()
        assert stats[b, 0] == pytest.approx(float(r[b] @ r[b]), rel=1e-13) and stats[b, 3] == np.abs(grad[b]).max()
        if D < d and lb == 0.0:
            # G = J^T J has rank D < d: with no damping either a pivot is refused or the factorisation of the float32-rounded
            # matrix completes; both are legitimate, and a completed solve still owes the backward-error bound
            assert info[b] in (0, 1)
        else:
            assert info[b] == 0
        if info[b] == 1:
            assert np.isnan(delta[b]).all() and np.isnan(stats[b, 1:3]).all()
            continue
        ratio = GN.residual_ratio(G[b], lb, grad[b], delta[b])
        A = torch.from_numpy(GN.damped(G[b], lb))
        solved = torch.linalg.solve(A, torch.from_numpy(grad[b]))
        ratio_ref = GN.residual_ratio(G[b], lb, grad[b], solved.numpy())
        print(f"D={D} d={d} lambda={lb:g}: residual / (d 2^-53 scale) = {ratio:.3f} (torch.linalg.solve: {ratio_ref:.3f}; bound "
              f"{GN.BOUND_C / 4:g}), max |delta - solve| / max |solve| = "
              f"{float(np.abs(delta[b] - solved.numpy()).max() / np.abs(solved.numpy()).max()):.2e}")
        assert ratio <= GN.BOUND_C / 4
        terms = np.abs(GN.damped(G[b], 0.0) * np.outer(delta[b], delta[b])).sum()
        assert abs(stats[b, 1] - grad[b] @ delta[b]) <= 2 * (d + 2) * GN.U * np.abs(grad[b] * delta[b]).sum()
        assert abs(stats[b, 2] - delta[b] @ GN.damped(G[b], 0.0) @ delta[b]) <= 2 * (d + 2) * GN.U * terms


def test_emulation_info_codes():
    J, G, x, xhat = GN.inputs(4, 64, 5, seed=1)
    J[1, :, 3] = J[1, :, 1]                                          # a duplicate column: G is singular, the pivot cancels exactly
    G[1] = GN.gram_by_dots(J[1])
    x[2, 7] = np.inf
    lam = np.zeros(4)
    grad, delta, stats, info = GN.batch(J, G, x, xhat, lam)
    assert info.tolist() == [0, 1, 2, 0]
    assert np.isnan(delta[1]).all() and np.isnan(stats[1, 1:3]).all() and np.isfinite(grad[1]).all() and np.isfinite(stats[1, [0, 3]]).all()
    assert np.isnan(grad[2]).all() and np.isnan(delta[2]).all() and np.isnan(stats[2]).all()
    # the damping lifts the duplicate column's pivot: lambda G_kk > 0
    _, delta_d, _, info_d = GN.batch(J, G, x, xhat, np.full(4, 1e-3))
    assert info_d.tolist() == [0, 0, 2, 0] and np.isfinite(delta_d[1]).all()
    # every other place a non-finite value may sit; the upper triangle of G is never read
    for where in ("xhat", "J", "G"):
        Jn, Gn, hn = J.copy(), G.copy(), xhat.copy()
        if where == "xhat":
            hn[0, 0] = np.nan
        elif where == "J":
            Jn[0, 3, 4] = np.nan
        else:
            Gn[0, 4, 2] = np.nan
        assert GN.batch(Jn, Gn, np.where(np.isfinite(x), x, 0).astype(np.float32), hn, lam)[3].tolist() == [2, 1, 0, 0]
    Gu = G.copy()
    Gu[0, 2, 4] = np.nan
    assert GN.batch(J, Gu, x, xhat, lam)[3].tolist() == [0, 1, 2, 0]
    # residual-only mode: ||r||^2 and info 0 / 2 alone
    _, _, s, i = GN.batch(None, None, x, xhat, None)
    assert i.tolist() == [0, 0, 2, 0] and np.isnan(s[2, 0]) and np.array_equal(s[[0, 1, 3], 0], stats[[0, 1, 3], 0])


@pytest.fixture(scope="module")
def models():
    cache = {}
    return lambda name: cache.setdefault(name, R.Model(name))


@pytest.mark.parametrize("name", SMOOTH + KINKED)
def test_reference_loop_removes_the_tangential_residual(name, models):
    m = models(name)
    start, end = R.project(m, m.y, steps=0), R.project(m, m.y, steps=10)
    s0, s10 = R.tangential_share(start), R.tangential_share(end)
    need = 100.0 if name in SMOOTH else 10.0
    print(f"{name}: max tangential2 / distance2 {s0:.3e} -> {s10:.3e} (x {s0 / max(s10, 1e-300):.3g}, required x {need:g}); accepted "
          f"{end['accepted'].tolist()}")
    assert s10 * need <= s0
    assert torch.equal(start["distance2"], start["initial_distance2"]) and torch.equal(start["initial_distance2"], end["initial_distance2"])
    assert bool((end["distance2"] <= end["initial_distance2"]).all()) and bool((end["accepted"] <= 10).all())
    assert bool((start["accepted"] == 0).all()) and bool((end["info"] == 0).all())
    assert torch.equal(end["reconstruction_head"], m.decode(end["latent"]))


@pytest.mark.parametrize("name", KNOWN_ANSWER)
def test_reference_loop_finds_the_known_answer(name, models):
    """y = g(z_0) + eps n with n normal to range(J(z_0)): z_0 is exactly stationary with distance^2 = eps^2.  The encoder starts
    above it (for at least one sample of the batch by more than the 5 tau the GPU test asks) and the loop ends on it."""
    m = models(name)
    z0 = m.encode(m.y)
    _, x_on, J = m.jacobian(z0)
    y, eps = R.normal_offset(x_on, J, seed=0)
    out = R.project(m, y, steps=10)
    excess0, excess = out["initial_distance2"] / eps ** 2 - 1, out["distance2"] / eps ** 2 - 1
    print(f"{name}: initial_distance2 / eps^2 - 1 in [{float(excess0.min()):.3e}, {float(excess0.max()):.3e}]; after ten steps "
          f"max |distance2 / eps^2 - 1| = {float(excess.abs().max()):.3e}")
    assert float(excess.abs().max()) <= 3e-9
    assert float(excess0.max()) > 5 * TAU and bool((excess0 > 0).all())


def small_density(dataset="power", **overrides):
    import cmf_amd
    cfg = cmf_amd.get_config(dataset, **overrides)
    shape = cmf_amd.DATA_SHAPES[dataset]
    return cmf_amd.get_density(cmf_amd.get_schema(cfg), torch.zeros(2, *shape))


def test_api_refusals():
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.densities import NonSquareHeadDensity
    assert E.PROJECT_MAX_WIDTH == 128
    dens = small_density()
    proj = cmf_amd.ManifoldProjector(dens)
    assert (proj.steps, proj.damping, proj.up, proj.down) == (10, 1e-3, 10.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proj.project(torch.zeros(2, 6))
    with pytest.raises(ValueError, match="GPU"):
        E.residual_sqnorm(torch.zeros(2, 6), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="GPU"):
        E.gauss_newton_step(E.Tangent(2, 6, 16, "panel", "cpu"), torch.zeros(2, 2, 2), torch.zeros(2, 6), torch.zeros(2, 6),
                            torch.zeros(2, dtype=torch.float64))
    # wider than the kernel's LDS matrix
    head = next(m for m in dens.modules() if isinstance(m, NonSquareHeadDensity))
    wide = small_density("mnist", latent_dimension=130)
    with pytest.raises(ValueError, match="1 <= latent_dimension <= 128"):
        cmf_amd.ManifoldProjector(wide)
    # not exactly one non-square head
    with pytest.raises(ValueError, match="one non-square head"):
        cmf_amd.ManifoldProjector(head.prior)
    # the M-flow baseline head
    with pytest.raises(NotImplementedError, match="M-flow"):
        cmf_amd.ManifoldProjector(small_density(m_flow=True))
    with pytest.raises(ValueError, match="one non-square head"):
        cmf_amd.ManifoldProjector(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="steps >= 0"):
        cmf_amd.ManifoldProjector(dens, steps=-1)
