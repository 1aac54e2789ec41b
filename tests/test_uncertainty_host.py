"""Host-side checks of the error bars of a Gauss-Newton fit (no GPU): the numpy emulation of the leverage kernel against
its numpy.longdouble reference, the bounds' constants and the planted defects they must catch; the covariance formula itself against
a Monte-Carlo run of the float64 reference loops; the Jacobian sensitivity tests/test_gpu_uncertainty.py takes its tolerance from;
and the host logic of ``ManifoldProjector.uncertainty`` and ``engine.tangent_leverage`` -- refusals, the timer entry, the noise level."""
import math

import numpy as np
import pytest
import torch

import _completion_reference as CR
import _data_recovery_reference as DR
import _leverage_emulation as LE
import _projection_reference as R
import _recovery_reference as RR
from test_projection_host import small_density

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def models():
    cache = {}
    return lambda name: cache.setdefault(name, R.Model(name))


# --------------------------------------------------------------------------------------------------
# the emulation and the bounds' constants
# --------------------------------------------------------------------------------------------------


def test_constants_and_planted_defects():
    """C_COV and C_LEV are 4 x (rounded up to a power of two) the emulation's worst ratios on the GPU test's own inputs, and the
    emulation with a planted defect lands above both bounds on every sample that has a factor to get wrong (d >= 2: at d = 1 there
    is no elimination step and no off-diagonal entry)."""
    worst_c = worst_l = 0.0
    least = {k: [math.inf, math.inf] for k in LE.DEFECTS}
    for d, D in LE.cases():
        J, G = LE.inputs(D, d)
        for b in range(LE.BATCH):
            cov, lev, stats, info = LE.leverage(J[b], G[b])
            if not LE.well_posed(d, D):
                assert info in (0, 1)
                continue
            cov_ref, lev_ref, _, info_ref = LE.reference(J[b], G[b])
            assert info == 0 and info_ref == 0
            assert np.array_equal(cov, cov.T) and not np.signbit(lev).any() and stats[1] == lev.max()
            worst_c, worst_l = max(worst_c, LE.cov_ratio(G[b], cov)), max(worst_l, LE.lev_ratio(G[b], lev, lev_ref))
            assert abs(lev.sum() - d) <= LE.trace_bound(J[b], G[b], cov_ref, lev_ref)
            if d < 2:
                continue
            for defect in LE.DEFECTS:
                cov_d, lev_d, _, info_d = LE.leverage(J[b], G[b], defect)
                assert info_d == 0
                least[defect][0] = min(least[defect][0], LE.cov_ratio(G[b], cov_d))
                least[defect][1] = min(least[defect][1], LE.lev_ratio(G[b], lev_d, lev_ref))
    print(f"emulation against longdouble: worst cov ratio 2^{math.log2(worst_c):.2f} (C_COV = {LE.C_COV:g}), worst lev ratio "
          f"2^{math.log2(worst_l):.2f} (C_LEV = {LE.C_LEV:g}); planted defects, least (cov, lev): "
          + ", ".join(f"{k} 2^{math.log2(v[0]):.1f} 2^{math.log2(v[1]):.1f}" for k, v in least.items()))
    assert LE.C_COV == LE.pow2_ceil(4 * worst_c) and LE.C_LEV == LE.pow2_ceil(4 * worst_l)
    assert all(v[0] > LE.C_COV and v[1] > LE.C_LEV for v in least.values())


def test_emulation_reports_failures_and_the_cov_only_mode():
    J, G = LE.inputs(64, 5, seed=1)
    cov, lev, stats, info = LE.leverage(J[0], G[0])
    cov_only, lev_only, stats_only, info_only = LE.leverage(None, G[0])
    assert info == info_only == 0 and np.array_equal(cov, cov_only) and lev_only is None and stats_only is None
    Jd = J[1].copy()
    Jd[:, 3] = Jd[:, 1]                                              # a duplicate column: the pivot cancels exactly
    out = LE.leverage(Jd, LE.GN.gram_by_dots(Jd))
    assert out[3] == 1 and np.isnan(out[0]).all() and np.isnan(out[1]).all() and np.isnan(out[2]).all()
    Jn, Gn = J[2].copy(), G[2].copy()
    Jn[40, 4] = np.nan
    assert LE.leverage(Jn, G[2])[3] == 2 and LE.leverage(None, G[2])[3] == 0
    Gn[4, 2] = np.nan
    assert LE.leverage(J[2], Gn)[3] == 2
    Gn = G[2].copy()
    Gn[2, 4] = np.nan                                                # the upper triangle is never read
    assert np.array_equal(LE.leverage(J[2], Gn)[1], LE.leverage(J[2], G[2])[1])


# --------------------------------------------------------------------------------------------------
# the formula is the right one: Monte Carlo on the float64 reference loops
# --------------------------------------------------------------------------------------------------

DRAWS = 400
#: noise per element, relative to ||g(z_0)|| / sqrt(D)
SIGMA_REL = 1e-3


def chi2_band(dof_total):
    """Five standard deviations of a chi-square of ``dof_total`` degrees of freedom, relative to its mean."""
    return 5.0 * math.sqrt(2.0 / dof_total)


def monte_carlo(m, A=None, seed=0):
    """DRAWS fits of y = A g(z_0) + sigma eps at the encoder's latent z_0 of the fixture's first input (A the identity for the
    projection), the draws as the batch, from z_0; and the reference's covariance at z_0.  Returns the three statistics as
    (value, expectation, degrees of freedom)."""
    z0 = m.encode(m.y[:1])
    x0 = m.decode(z0)
    D, d = x0[0].numel(), z0.shape[1]
    sigma = SIGMA_REL * float(x0.norm()) / math.sqrt(D)
    gen = torch.Generator().manual_seed(9000 + seed)
    zs = z0.expand(DRAWS, d).contiguous()
    _, _, J = m.jacobian(z0)
    if A is None:
        y = x0 + sigma * torch.randn(DRAWS, *x0.shape[1:], dtype=F64, generator=gen)
        out = R.project(m, y, steps=10, z=zs)
        cost, n_obs = out["distance2"], D
        ref = LE.uncertainty(J, noise_std=sigma)
    else:
        y = RR.image(A, x0) + sigma * torch.randn(DRAWS, A.shape[0], dtype=F64, generator=gen)
        out = RR.recover(m, y, A, zs, steps=10)
        cost, n_obs = out["cost"], A.shape[0]
        ref = LE.uncertainty(J, A=A, noise_std=sigma)
    assert bool((out["info"] == 0).all()) and bool((out["accepted"] >= 1).all())
    dz = out["latent"] - z0
    N = ref["normal"][0]
    mahalanobis = float(torch.einsum("bi,ij,bj->", dz, N, dz)) / sigma ** 2
    moved = float(((out["reconstruction_head"] - x0).flatten(1) ** 2).sum())
    return ((mahalanobis, DRAWS * d, DRAWS * d),
            (moved, sigma ** 2 * DRAWS * float(ref["leverage"].sum()), DRAWS * d),
            (float((cost / (n_obs - d)).mean()), sigma ** 2, DRAWS * (n_obs - d)))


@pytest.mark.parametrize("name,M", [("c2b_hepmass", None), ("c2a_power", None), ("c2b_hepmass", 15)])
def test_covariance_matches_a_monte_carlo_run_of_the_reference_loop(name, M, models):
    """sum (z - z_0)^T C^-1 (z - z_0) / sigma^2 ~ chi2(N d), sum ||x_hat - g(z_0)||^2 against sigma^2 N sum_i lev_i, and the mean of
    cost / (n_obs - d) against sigma^2 ~ chi2(N (n_obs - d)) / (N (n_obs - d)): each within five standard deviations."""
    m = models(name)
    A = None if M is None else RR.gaussian_operator(M, m.y[0].numel()).double()
    for label, (value, expect, dof) in zip(("mahalanobis", "reconstruction", "noise level"), monte_carlo(m, A)):
        print(f"{name}{'' if M is None else f', M = {M}'}: {label}: {value:.6e} against {expect:.6e}: off by {value / expect - 1:+.4f} "
              f"(band {chi2_band(dof):.4f})")
        assert abs(value / expect - 1.0) <= chi2_band(dof), label


# --------------------------------------------------------------------------------------------------
# the Jacobian sensitivity the GPU tolerance is taken from
# --------------------------------------------------------------------------------------------------


def reference_case(m, name, path):
    """The float64 reference loop of ``path`` on the fixture, as tests/test_gpu_uncertainty.py sets the problem, and the arguments
    of ``LE.uncertainty`` at its latent: (J, keywords)."""
    y = m.y if name != "mini_mnist" else m.y[:DR.BATCH]
    z0 = m.encode(y)
    x_on = m.decode(z0)
    D = x_on[0].numel()
    if path in ("project", "project-data"):
        out = R.project(m, y, steps=10)
        kw = dict(cost=out["distance2"])
        if path == "project-data":                                   # qualified in pixel values: du/dv at the projection
            kw["s"] = DR.DataModel(m).wrapper(out["reconstruction_head"])[1].flatten(1)
    elif path == "complete":
        yc, w = CR.problem(x_on, data_rel=LE.MEASUREMENT_REL)
        out = CR.complete(m, yc, w, steps=10, z=m.encode(yc))
        kw = dict(cost=out["cost"], w=w.flatten(1))
    elif path == "recover":
        A = RR.gaussian_operator(RR.KNOWN_ANSWER[name], D).double()
        meas = RR.measure(A, x_on, data_rel=LE.MEASUREMENT_REL)
        out = RR.recover(m, meas, A, m.encode(RR.start_input(x_on)), steps=10)
        kw = dict(cost=out["cost"], A=A)
    else:
        dm = DR.DataModel(m)
        A = DR.operator("built").double()
        u_on = dm.wrapper(x_on)[0]
        meas = RR.measure(A, u_on, data_rel=LE.MEASUREMENT_REL)
        out = RR.recover(dm, meas, A, dm.encode(DR.start_input(dm, x_on)), steps=10)
        kw = dict(cost=out["cost"], A=A, s=dm.wrapper(m.decode(out["latent"]))[1].flatten(1))
    assert bool((out["info"] == 0).all())
    return m.jacobian(out["latent"])[2], kw


@pytest.mark.parametrize("name,path", list(LE.E2E_TOL))
def test_jacobian_sensitivity_sets_the_gpu_tolerance(name, path, models):
    """How far DESIGN 5's Jacobian tolerance moves the reference's own standard deviations: the measurement ``LE.E2E_TOL``
    is 4 x (rounded up to a power of two) of."""
    J, kw = reference_case(models(name), name, path)
    clean = LE.uncertainty(J, **kw)
    moved = LE.uncertainty(J, jitter=LE.jitter(J), **kw)
    assert bool(torch.isfinite(clean["latent_std"]).all()) and bool((clean["dof"] > 0).all())
    worst = float(LE.std_distance(moved, clean).max())
    print(f"{name}, {path}: worst relative change of the standard deviations under a {LE.JACOBIAN_REL:g} perturbation of J = "
          f"{worst:.3e}; E2E_TOL = 2^{math.log2(LE.E2E_TOL[name, path]):g}; dof {clean['dof'].tolist()}")
    assert LE.E2E_TOL[name, path] == LE.pow2_ceil(4 * worst)


# --------------------------------------------------------------------------------------------------
# host logic: the noise level, the refusals, the timer entry
# --------------------------------------------------------------------------------------------------


class FakeGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True (the technique of tests/test_engine_wrappers_host.py)."""

    @property
    def is_cuda(self):
        return True


class OtherGpu(FakeGpu):
    @property
    def device(self):
        return torch.device("cuda", 1)


def gpu(*shape, dtype=F32, cls=FakeGpu):
    return torch.zeros(*shape, dtype=dtype).as_subclass(cls)


class StubTimer:
    def __init__(self):
        self.records = []

    def wrap(self, name, flops, nbytes, launch):
        self.records.append((name, flops, nbytes))


def test_noise_level_and_degrees_of_freedom():
    from cmf_amd.projection import noise_level
    n_obs = torch.tensor([21, 11, 10, 4, 0])
    cost = torch.tensor([22.0, 3.0, 5.0, 1.0, 0.0], dtype=F64)
    sigma2, dof = noise_level(n_obs, 10, cost=cost)
    assert dof.dtype == torch.int32 and dof.tolist() == [11, 1, 0, -6, -10]
    assert sigma2.dtype == F64 and sigma2[:2].tolist() == [2.0, 3.0] and bool(torch.isnan(sigma2[2:]).all())
    given = torch.tensor([0.25, 0.0, 1.0, 4.0, 9.0], dtype=F64)
    sigma2, dof = noise_level(n_obs, 10, variance=given)
    assert sigma2 is given and dof.tolist() == [11, 1, 0, -6, -10]    # a known noise level needs no degrees of freedom


def test_wrapper_derivative():
    from cmf_amd.projection import wrapper_derivative
    v = torch.tensor([[-3.0, 0.0, 2.5, 30.0]])
    e = torch.exp(-v.double().abs())
    got = wrapper_derivative((0.5, 0.1, True), v)
    assert torch.equal(got, (e / (1 + e) ** 2 / 0.5).float())
    p = torch.sigmoid(v.double())
    assert bool(((got.double() - p * (1 - p) / 0.5)[:, :3].abs() <= 1e-6 * got.double()[:, :3]).all())   # the textbook form, away from p = 1
    assert torch.equal(wrapper_derivative((-4.0, 0.1, False), v), torch.full((1, 4), 0.25))


def test_uncertainty_refusals():
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(small_density())
    d = proj.head.program.d
    lat, cost = torch.zeros(2, d), torch.zeros(2, dtype=F64)
    ok = {"latent": lat, "cost": cost}
    with pytest.raises(ValueError, match="space must be 'head' or 'data'"):
        proj.uncertainty(ok, space="pixels")
    with pytest.raises(ValueError, match="not both"):
        proj.uncertainty(ok, weights=torch.ones(2, 6), operator=torch.zeros(4, 6))
    for bad in (None, {"cost": cost}, {"latent": lat.double()}, {"latent": torch.zeros(2, d + 1)}, {"latent": torch.zeros(d, 2).t()},
                {"latent": lat.numpy()}):
        with pytest.raises(ValueError, match=rf"result\['latent'\] must be a contiguous float32 \(B, {d}\)"):
            proj.uncertainty(bad)
    with pytest.raises(ValueError, match="at least one sample"):
        proj.uncertainty({"latent": lat[:0], "cost": cost[:0]})
    for bad in ({"latent": lat}, {"latent": lat, "cost": cost.float()}, {"latent": lat, "cost": cost[:1]},
                {"latent": lat, "distance2": torch.zeros(2, 1, dtype=F64)}):
        with pytest.raises(ValueError, match=r"result\['cost'\] \(or 'distance2'\) must be a float64 \(2,\) tensor when noise_std is None"):
            proj.uncertainty(bad)
    with pytest.raises(ValueError, match="noise_std must be >= 0"):
        proj.uncertainty(ok, noise_std=-1.0)
    with pytest.raises(ValueError, match="noise_std must be >= 0"):
        proj.uncertainty(ok, noise_std=float("nan"))
    with pytest.raises(ValueError, match=r"noise_std must be a float or a floating point \(2,\) tensor"):
        proj.uncertainty(ok, noise_std=torch.zeros(3))
    with pytest.raises(ValueError, match=r"noise_std must be a float or a floating point \(2,\) tensor"):
        proj.uncertainty(ok, noise_std=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="weights must be a floating point or bool tensor"):
        proj.uncertainty(ok, weights=torch.ones(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="weights must be a floating point or bool tensor"):
        proj.uncertainty(ok, weights=[1.0] * 6)
    with pytest.raises(ValueError, match=r"weights must have x's shape \(2, 6\) or broadcast over its batch, got \(2, 5\)"):
        proj.uncertainty(ok, weights=torch.ones(2, 5))
    with pytest.raises(ValueError, match=r"operator must be a contiguous float32 \(M, 6\)"):
        proj.uncertainty(ok, operator=torch.zeros(4, 5))
    with pytest.raises(ValueError, match="operator must be a contiguous float32"):
        proj.uncertainty(ok, operator=torch.zeros(4, 6).double())
    with pytest.raises(ValueError, match="not contiguous"):
        proj.uncertainty(ok, operator=torch.zeros(6, 4).t())
    for name, kw in (("weights", dict(weights=torch.ones(2, 6, device="meta"))), ("operator", dict(operator=torch.zeros(4, 6, device="meta"))),
                     ("noise_std", dict(noise_std=torch.zeros(2, device="meta")))):
        with pytest.raises(ValueError, match=f"{name} must be on result\\['latent'\\]'s device cpu"):
            proj.uncertainty(ok, **kw)
    with pytest.raises(ValueError, match=r"result\['cost'\] must be on result\['latent'\]'s device"):
        proj.uncertainty({"latent": lat, "cost": torch.zeros(2, dtype=F64, device="meta")})
    # every argument in order and nothing on the GPU; neither cost nor distance2 is needed beside a noise_std
    for kw in ({}, {"weights": torch.ones(6)}, {"weights": torch.ones(1, 6, dtype=torch.bool)}, {"operator": torch.zeros(4, 6)},
               {"operator": torch.zeros(4, 6), "space": "data"}, {"noise_std": 0.5}, {"noise_std": torch.ones(2, dtype=F64)}):
        with pytest.raises(ValueError, match="no CPU fallback"):
            proj.uncertainty(ok if "noise_std" not in kw else {"latent": lat}, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        proj.uncertainty({"latent": lat, "distance2": cost})
    assert proj.data_shape() == (6,)


def test_tangent_leverage_refusals_and_timer_entry():
    from cmf_amd import engine as E
    B, N, d, nc = 2, 5, 3, 16
    T = E.Tangent(B, N, nc, "panel", "cpu", data=gpu(B * N * nc))
    with pytest.raises(ValueError, match="T must be an engine.Tangent"):
        E.tangent_leverage(gpu(B, N, nc), gpu(B, d, d))
    with pytest.raises(ValueError, match="jtj must be on the GPU"):
        E.tangent_leverage(T, torch.zeros(B, d, d))
    with pytest.raises(ValueError, match="jtj must be float32"):
        E.tangent_leverage(T, gpu(B, d, d, dtype=F64))
    with pytest.raises(ValueError, match=r"jtj must be a contiguous \(B, d, d\) tensor"):
        E.tangent_leverage(T, gpu(B, d, d + 1))
    for width in (0, 129):
        with pytest.raises(ValueError, match=rf"d = {width}: the leverage kernel supports 1 <= d <= 128"):
            E.tangent_leverage(E.Tangent(B, N, 144, "panel", "cpu", data=gpu(B * N * 144)), gpu(B, width, width))
    for bad in (E.Tangent(B + 1, N, nc, "panel", "cpu", data=gpu((B + 1) * N * nc)), E.Tangent(B, N, 8, "panel", "cpu", data=gpu(B * N * 8)),
                E.Tangent(B, N, nc, "panel", "cpu", data=gpu(B * N * nc, cls=OtherGpu))):
        with pytest.raises(ValueError, match=r"must hold d = 3 <= nc columns, nc % 16 == 0, for the 2 samples of jtj \(2, 3, 3\) on cpu"):
            E.tangent_leverage(bad, gpu(B, d, d))
    with pytest.raises(ValueError, match="must hold d = 17 <= nc columns"):
        E.tangent_leverage(T, gpu(B, 17, 17))
    entries = {}
    for rows in (True, False):
        stub = StubTimer()
        with E._use_timer(stub):
            r = E.tangent_leverage(T, gpu(B, d, d), rows=rows)
        assert len(stub.records) == 1 and stub.records[0][0] == "tangent_leverage"
        entries[rows] = stub.records[0]
        assert r.cov.shape == (B, d, d) and r.cov.dtype == F64 and r.info.dtype == torch.int32
        assert (r.lev is None and r.stats is None) if not rows else (r.lev.shape == (B, N) and r.stats.shape == (B, 2))
    # flops: elimination, inverse and cov 7 d^3 / 6 per sample, d^2 + 3 d per row; bytes: the live quarter-rows of J once, the
    # triangle in, cov and lev out, stats and info
    assert entries[False][1:] == (B * 7.0 * d ** 3 / 6.0, B * (2.0 * d * (d + 1) + 8.0 * d * d + 4.0))
    assert entries[True][1:] == (B * (7.0 * d ** 3 / 6.0 + N * (d * d + 3.0 * d)),
                                 B * (4.0 * N * 4 + 2.0 * d * (d + 1) + 8.0 * d * d + 8.0 * N + 16.0 + 4.0))
    # without a timer the cost is never evaluated and B = 0 launches nothing
    r = E.tangent_leverage(E.Tangent(0, N, nc, "panel", "cpu", data=gpu(0)), gpu(0, d, d))
    assert r.cov.shape == (0, d, d) and r.lev.shape == (0, N) and r.stats.shape == (0, 2) and r.info.shape == (0,)
