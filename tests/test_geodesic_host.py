"""Host-side checks of the manifold geodesics (no GPU): the numpy emulation of the curve step kernel against float64
numpy on the dense system, the float64 reference loop on the fixtures -- the conditions tests/test_gpu_geodesic.py asserts of the
product are established here on the reference alone -- and the refusals of the public API.

Emulation bounds, a quarter of the kernel's: |g - g_ref| <= (D + 4) / 2 2^-53 sum |J| |s| and ||A delta - g||_inf <= 16 d 2^-53
(||A||_inf ||delta||_inf + ||g||_inf) on the dense (M d)^2 matrix A (BOUND_C / 4)."""
import numpy as np
import pytest
import torch

import _curve_step_emulation as CE
import _geodesic_reference as R


def damping_family(D, d):
    """The dampings a shape is run at: D < d (a rank-deficient H) only with lambda > 0."""
    return [lam for lam in CE.DAMPINGS if D >= d or lam > 0.0]


def check_curve(J, G, C, xhat, lam, grad, delta, stats, seg2, bound_c, label):
    """One curve's outputs (info 0) against float64 numpy on the same float32 inputs; returns the residual ratio."""
    P, D, d = J.shape
    M = P - 2
    x = xhat.astype(np.float64)
    s = (x[:-2] + x[2:]) - 2.0 * x[1:-1]
    J64 = J[1:-1].astype(np.float64)
    g_ref = np.einsum("ir,irk->ik", s, J64)
    g_abs = np.einsum("ir,irk->ik", np.abs(s), np.abs(J64))
    assert (np.abs(grad - g_ref) <= bound_c / CE.BOUND_C * 2 * (D + 4) * CE.U * g_abs).all(), label
    r = x[1:] - x[:-1]
    assert (np.abs(seg2 - (r * r).sum(1)) <= 2 * (D + 2) * CE.U * (r * r).sum(1)).all(), label
    total = 0.0
    for v in seg2:
        total += float(v)
    assert stats[0] == total and stats[3] == np.abs(grad).max(), label
    A, H = CE.dense(G, C, lam)
    ratio = CE.residual_ratio(A, d, grad, delta)
    assert ratio <= bound_c, label
    gv, dv = grad.reshape(-1), delta.reshape(-1)
    assert abs(stats[1] - gv @ dv) <= 2 * (M * d + 2) * CE.U * np.abs(gv * dv).sum(), label
    assert abs(stats[2] - dv @ H @ dv) <= 2 * (M * d + 2) * CE.U * np.abs(H * np.outer(dv, dv)).sum(), label
    return ratio


@pytest.mark.parametrize("P", CE.POINTS)
@pytest.mark.parametrize("d", CE.WIDTHS)
@pytest.mark.parametrize("D", CE.ROWS)
def test_emulation_solves_the_block_tridiagonal_system(D, d, P):
    lams = damping_family(D, d)
    J, G, C, xhat = CE.inputs(len(lams), P, D, d)
    grad, delta, stats, seg2, info = CE.batch(J, G, C, xhat, np.array(lams), P)
    assert (info == 0).all()
    worst = 0.0
    for c, lam in enumerate(lams):
        sl = slice(c * P, (c + 1) * P)
        worst = max(worst, check_curve(J[sl], G[sl], C[c], xhat[sl], lam, grad[c], delta[c], stats[c], seg2[c], CE.BOUND_C / 4,
                                       f"curve {c}"))
        e_seg2, e_sum, e_info = CE.energy(xhat[sl], P)
        assert e_info == 0 and np.array_equal(e_seg2, seg2[c]) and e_sum == stats[c, 0]
    print(f"D={D} d={d} P={P}: worst residual / (d 2^-53 scale) = {worst:.3f} (bound {CE.BOUND_C / 4:g})")


def test_emulation_info_codes():
    P, D, d = 4, 64, 5
    J, G, C, xhat = CE.inputs(3, P, D, d, seed=1)
    lam = np.zeros(3)
    clean = CE.batch(J, G, C, xhat, lam, P)
    assert clean[4].tolist() == [0, 0, 0]
    # an all-zero Jacobian column at an interior point: its pivot is exactly 0 at every lambda
    Jz = J.copy()
    Jz[P + 2, :, 3] = 0.0
    Gz = (Jz.astype(np.float64).transpose(0, 2, 1) @ Jz.astype(np.float64)).astype(np.float32)
    Cz = CE.cross_of(Jz, P).astype(np.float32)
    for value in CE.DAMPINGS:
        grad, delta, stats, seg2, info = CE.batch(Jz, Gz, Cz, xhat, np.full(3, value), P)
        assert info.tolist() == [0, 1, 0]
        assert np.isnan(delta[1]).all() and np.isnan(stats[1, 1:3]).all()
        assert np.isfinite(grad[1]).all() and np.isfinite(stats[1, [0, 3]]).all() and np.isfinite(seg2[1]).all()
    # every place a non-finite value may sit
    for where in ("xhat", "xhat_end", "J", "G", "C"):
        Jn, Gn, Cn, hn = J.copy(), G.copy(), C.copy(), xhat.copy()
        if where == "xhat":
            hn[P + 1, 0] = np.nan
        elif where == "xhat_end":
            hn[2 * P - 1, 3] = np.inf
        elif where == "J":
            Jn[P + 2, 3, 4] = np.nan
        elif where == "G":
            Gn[P + 1, 4, 2] = np.nan
        else:
            Cn[1, 0, 2, 4] = np.nan
        out = CE.batch(Jn, Gn, Cn, hn, lam, P)
        assert out[4].tolist() == [0, 2, 0]
        assert all(np.isnan(o[1]).all() for o in out[:4])
        assert all(np.array_equal(o[[0, 2]], w[[0, 2]]) for o, w in zip(out[:4], clean[:4]))
    # the end points' jtj and Jacobians and the upper triangles are never read
    Jn, Gn = J.copy(), G.copy()
    Gn[P] = np.nan
    Gn[2 * P - 1] = np.nan
    Jn[P] = np.nan
    Gn[P + 1, 2, 4] = np.nan
    out = CE.batch(Jn, Gn, C, xhat, lam, P)
    assert all(np.array_equal(o, w) for o, w in zip(out, clean))
    assert CE.energy(np.where(np.arange(P)[:, None] == 1, np.nan, xhat[:P]).astype(np.float32), P)[2] == 2


def known_answer(P, D, d, seed):
    """Every point of the curve has the same Jacobian J (small integers: J^T J is exact in float32) and xhat_i = float32(J z_i +
    c) for scattered z_i: one undamped step must land z_i + delta_i on the uniformly spaced line from z_0 to z_{P-1}.  Returns
    (J (P, D, d), G (P, d, d), C (P - 3, d, d), xhat (P, D), z (P, d) float64, line (P, d) float64, tol): tol bounds |z + delta -
    line| by the float32 rounding e_i of xhat carried through the least-squares solve -- ||K^+|| ||De||_2 with K = T (x) J, T the
    N x M difference matrix (sigma_min = 2 sin(pi / 2N)), ||De||_2 <= 2 sqrt(sum ||e_i||^2), |e_i| <= 2^-24 |xhat_i| -- plus the
    float64 solve's own residual bound carried through A^-1."""
    rng = np.random.default_rng(7919 * d + 13 * D + P + seed)
    J1 = rng.integers(-2, 3, size=(D, d)).astype(np.float32)
    J1[np.arange(d) % D, np.arange(d)] += 3.0                        # keep every column away from zero
    z = rng.standard_normal((P, d))
    z[1:-1] += 0.5 * rng.standard_normal((P - 2, d))
    x64 = z @ J1.astype(np.float64).T + rng.standard_normal(D)
    xhat = x64.astype(np.float32)
    G1 = (J1.astype(np.float64).T @ J1.astype(np.float64))
    assert np.array_equal(G1.astype(np.float32).astype(np.float64), G1)
    J = np.broadcast_to(J1, (P, D, d)).copy()
    G = np.broadcast_to(G1.astype(np.float32), (P, d, d)).copy()
    C = np.broadcast_to(G1.astype(np.float32), (max(P - 3, 0), d, d)).copy()
    line = z[0] + np.linspace(0.0, 1.0, P)[:, None] * (z[-1] - z[0])
    sigma = np.linalg.svd(J1.astype(np.float64), compute_uv=False)
    rounding = 2.0 * 2.0 ** -24 * np.sqrt((xhat.astype(np.float64) ** 2).sum()) / (2.0 * np.sin(np.pi / (2 * (P - 1))) * sigma[-1])
    A, _ = CE.dense(G, C, 0.0)
    step = np.abs(line - z).max()
    solve = 2.0 * CE.BOUND_C * d * CE.U * np.linalg.cond(A, np.inf) * step
    return J, G, C, xhat, z, line, rounding + solve


@pytest.mark.parametrize("P,D,d", [(3, 5, 3), (4, 64, 17), (9, 64, 16), (9, 784, 64), (4, 784, 100)])
def test_emulation_finds_the_known_answer(P, D, d):
    J, G, C, xhat, z, line, tol = known_answer(P, D, d, seed=0)
    grad, delta, stats, seg2, info = CE.step(J, G, C, xhat, 0.0)
    assert info == 0
    err = np.abs(z[1:-1] + delta - line[1:-1]).max()
    print(f"P={P} D={D} d={d}: max |z + delta - line| = {err:.3e} (tolerance {tol:.3e}; the step itself {np.abs(line - z).max():.3e})")
    assert err <= tol < 1e-3 * np.abs(line - z).max()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_reference_loop_relaxes_the_straight_line(name):
    model, start, end = R.reference_run(name)
    N = R.POINTS - 1
    fall = start["gradient_max"] / end["gradient_max"]
    gain = 1.0 - end["energy"] / end["initial_energy"]
    spread = end["segment_lengths"].max(1).values / end["segment_lengths"].min(1).values - 1.0
    print(f"{name}: accepted {end['accepted'].tolist()}; max |gradient| fell by {float(fall.min()):.3g} .. {float(fall.max()):.3g}; "
          f"energy gain {float(gain.min()):.3e} .. {float(gain.max()):.3e}; segment spread {float(spread.max()):.3e}")
    assert bool((end["info"] == 0).all()) and bool((start["info"] == 0).all())
    assert bool((end["energies"][1:] <= end["energies"][:-1]).all()) and bool((end["energy"] <= end["initial_energy"]).all())
    assert torch.equal(end["energies"][0], end["initial_energy"]) and torch.equal(end["energies"][-1], end["energy"])
    assert torch.equal(start["energy"], start["initial_energy"]) and torch.equal(start["initial_energy"], end["initial_energy"])
    assert bool((start["accepted"] == 0).all()) and bool((end["accepted"] <= R.STEPS).all())
    for out in (start, end):
        assert bool((out["length"] ** 2 <= out["energy"] * (1 + 1e-12)).all())
        assert torch.allclose(out["energy"], N * (out["segment_lengths"] ** 2).sum(1), rtol=1e-13, atol=0)
    assert bool((end["gradient_max"] * 1e6 <= start["gradient_max"]).all())
    assert torch.equal(end["latents"][:, 0], start["latents"][:, 0]) and torch.equal(end["latents"][:, -1], start["latents"][:, -1])


def small_density(dataset="power", **overrides):
    import cmf_amd
    cfg = cmf_amd.get_config(dataset, **overrides)
    shape = cmf_amd.DATA_SHAPES[dataset]
    return cmf_amd.get_density(cmf_amd.get_schema(cfg), torch.zeros(2, *shape))


def test_api_refusals():
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.densities import NonSquareHeadDensity
    assert E.GEODESIC_MAX_WIDTH == 128
    dens = small_density()
    geo = cmf_amd.ManifoldGeodesic(dens)
    assert (geo.points, geo.steps, geo.damping, geo.up, geo.down) == (17, 10, 1e-3, 10.0, 0.1)
    d = geo.head.program.d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.connect(torch.zeros(2, 6), torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.connect_latents(torch.zeros(2, d), torch.zeros(2, d))
    with pytest.raises(ValueError, match="GPU"):
        E.curve_energy(torch.zeros(6, 6), 3)
    with pytest.raises(ValueError, match="GPU"):
        E.cross_gram(E.Tangent(6, 6, 16, "panel", "cpu"), 2, 3)
    with pytest.raises(ValueError, match="GPU"):
        E.curve_step(E.Tangent(6, 6, 16, "panel", "cpu"), torch.zeros(6, 2, 2), torch.zeros(2, 0, 2, 2), torch.zeros(6, 6), 3,
                     torch.zeros(2, dtype=torch.float64))
    for bad in (2, 0, -1):
        with pytest.raises(ValueError, match="points >= 3"):
            cmf_amd.ManifoldGeodesic(dens, points=bad)
    with pytest.raises(ValueError, match="steps >= 0"):
        cmf_amd.ManifoldGeodesic(dens, steps=-1)
    for kw in ({"damping": -1.0}, {"up": 0.5}, {"down": 0.0}, {"down": 2.0}):
        with pytest.raises(ValueError, match="damping >= 0"):
            cmf_amd.ManifoldGeodesic(dens, **kw)
    # wider than the curve step kernel's window
    wide = small_density("mnist", latent_dimension=130)
    with pytest.raises(ValueError, match="1 <= latent_dimension <= 128"):
        cmf_amd.ManifoldGeodesic(wide)
    # not exactly one non-square head
    head = next(m for m in dens.modules() if isinstance(m, NonSquareHeadDensity))
    with pytest.raises(ValueError, match="one non-square head"):
        cmf_amd.ManifoldGeodesic(head.prior)
    with pytest.raises(ValueError, match="one non-square head"):
        cmf_amd.ManifoldGeodesic(torch.nn.Linear(2, 2))
    # the M-flow baseline head
    with pytest.raises(NotImplementedError, match="M-flow"):
        cmf_amd.ManifoldGeodesic(small_density(m_flow=True))
