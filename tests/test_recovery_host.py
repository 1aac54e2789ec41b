"""Host-side checks of the recovery of linear inverse problems (no GPU): the numpy emulation of the operator kernel
against float64, the bound's constant and the planted defects it must catch, the float64 reference loop on the fixtures -- the
conditions tests/test_gpu_recovery.py asserts of the product are established here on the reference alone --, the data sensitivity
its end-to-end tolerance is derived from, and the refusals of ``ManifoldProjector.recover`` and of the two engine wrappers."""
import math

import numpy as np
import pytest
import torch

import _completion_reference as CR
import _operator_apply_emulation as OA
import _projection_reference as R
import _recovery_reference as RR
from test_gpu_projection import TAU
from test_projection_host import small_density


@pytest.fixture(scope="module")
def models():
    cache = {}
    return lambda name: cache.setdefault(name, R.Model(name))


# --------------------------------------------------------------------------------------------------
# the emulation and the bound's constant
# --------------------------------------------------------------------------------------------------


def test_operator_constant_and_planted_defects():
    """C_OPERATOR is 4 x (rounded up to a power of two) the emulation's worst error on the GPU test's own inputs, and the emulation
    with a planted defect lands above it on every sample."""
    worst, least = 0.0, {k: math.inf for k in OA.DEFECTS}
    for M, D, d in OA.SHAPES:
        a, J, _ = OA.inputs(M, D, d)
        for b in range(OA.BATCH):
            K64, S = OA.apply64(a, J[b])
            assert (S > 0).all()
            worst = max(worst, OA.ratio(OA.apply32(a, J[b]), K64, S))
            for defect in OA.DEFECTS:
                if defect == "transposed" and M != D:
                    continue
                least[defect] = min(least[defect], OA.ratio(OA.apply32(a, J[b], defect), K64, S))
    print(f"emulation against float64: worst |K - K64| / (|a| |J|) = 2^{math.log2(worst):.2f} (C_OPERATOR = "
          f"2^{math.log2(OA.C_OPERATOR):g}); planted defects, least: " + ", ".join(f"{k} 2^{math.log2(v):.2f}" for k, v in least.items()))
    assert OA.C_OPERATOR == CR.pow2_ceil(4 * worst)
    assert all(v > OA.C_OPERATOR for v in least.values())


def test_emulation_keeps_columns_apart_and_the_identity_exact():
    a, J, _ = OA.inputs(17, 64, 17)
    Jn = np.concatenate((J[0], np.full((64, 15), np.nan, dtype=np.float32)), axis=1)      # the padding columns of a stack
    K = OA.apply32(a, Jn)
    assert np.array_equal(K[:, :17], OA.apply32(a, J[0])) and np.isnan(K[:, 17:]).all()
    eye = np.eye(64, dtype=np.float32)
    assert np.array_equal(OA.apply32(eye, J[0]), J[0])
    perm = np.random.default_rng(0).permutation(64)
    assert np.array_equal(OA.apply32(eye[perm], J[0]), J[0][perm])


def test_image_bound_holds_for_a_float32_rounding_of_the_float64_sum():
    for M, D, d in OA.SHAPES:
        a, _, xhat = OA.inputs(M, D, d)
        y64, S = OA.image64(a, xhat)
        rounded = y64.astype(np.float32).astype(np.float64)
        assert (np.abs(rounded - y64) <= OA.image_bound(y64, S, D)).all()
        # an fp32 accumulation does not fit it: the reason the kernel sums in float64
        if D >= 64:
            y32 = np.zeros_like(y64, dtype=np.float32)
            for i in range(D):
                y32 = y32 + a[None, :, i] * xhat[:, i, None]
            assert not (np.abs(y32.astype(np.float64) - y64) <= OA.image_bound(y64, S, D)).all()


# --------------------------------------------------------------------------------------------------
# the float64 reference loop
# --------------------------------------------------------------------------------------------------


def known_answer(m, name, data_rel=0.0):
    z0 = m.encode(m.y)
    x_on = m.decode(z0)
    A = RR.gaussian_operator(RR.KNOWN_ANSWER[name], x_on[0].numel()).double()
    y = RR.measure(A, x_on, data_rel=data_rel)
    out = RR.recover(m, y, A, m.encode(RR.start_input(x_on)), steps=10)
    return z0, x_on, out


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_reference_loop_finds_the_known_answer(name, models):
    """y = A g(z_0) for the seeded Gaussian operator; ten steps from the encoder's latent of x_on + 0.1 ||x_on|| / sqrt(D) randn
    reconstruct x_on over all D elements, every sample."""
    m = models(name)
    z0, x_on, out = known_answer(m, name)
    rel = RR.rel_distance(out["reconstruction_head"], x_on)
    drop = float((out["initial_cost"] / out["cost"].clamp_min(1e-300)).min())
    print(f"{name}: M = {RR.KNOWN_ANSWER[name]}: ||g(z) - x_on|| / ||x_on|| <= {float(rel.max()):.2e}; max |z - z0| = "
          f"{float((out['latent'] - z0).abs().max()):.2e}; accepted {out['accepted'].tolist()}; initial_cost / cost >= {drop:.2e}")
    assert float(rel.max()) <= 1e-11
    assert bool((out["info"] == 0).all()) and bool((out["costs"][1:] <= out["costs"][:-1]).all())
    assert bool((out["cost"] * 1e6 < out["initial_cost"]).all())
    assert torch.equal(out["reconstruction_head"], m.decode(out["latent"]))
    assert torch.equal(out["measurement"], RR.image(RR.gaussian_operator(RR.KNOWN_ANSWER[name], x_on[0].numel()).double(),
                                                    out["reconstruction_head"]))


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_data_sensitivity_sets_the_gpu_tolerance(name, models):
    """How far DESIGN 5's x_hat tolerance, carried through A as a perturbation of the measurements, moves the recovered point: the
    measurement the GPU end-to-end tolerance ``RR.E2E_TOL`` is 4 x (rounded up to a power of two) of."""
    m = models(name)
    _, x_on, out = known_answer(m, name, data_rel=RR.DATA_REL)
    worst = float(RR.rel_distance(out["reconstruction_head"], x_on).max())
    print(f"{name}: worst ||g(z) - x_on|| / ||x_on|| under a {RR.DATA_REL:g} measurement perturbation = {worst:.3e}; "
          f"E2E_TOL = 2^{math.log2(RR.E2E_TOL[name]):g} = {RR.E2E_TOL[name]:.3e}")
    assert bool((out["info"] == 0).all())
    assert RR.E2E_TOL[name] == RR.pow2_ceil(4 * worst)


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass", "c1_sphere_d2"])
def test_selection_operator_reaches_the_cost_of_complete(name, models):
    """The rows of the identity for a seeded half of the elements against ``complete`` with the matching 0/1 weights, on the fixtures'
    own inputs (off the manifold: the cost stays well above zero), both from the encoder's latent: the two float64 loops end at
    costs within TAU / 4 of each other.  The fixtures that hold this are ``RR.SELECTION``, the GPU test's."""
    m = models(name)
    y = m.y
    A, w = RR.selection(y[0].numel())
    A = A.double()
    z = m.encode(y)
    rec = RR.recover(m, RR.image(A, y), A, z, steps=10)
    com = CR.complete(m, y, w.double().view(1, *y.shape[1:]).expand_as(y), steps=10, z=z)
    rel = ((rec["cost"] - com["cost"]).abs() / com["cost"])
    print(f"{name}: |cost - complete's| / complete's <= {float(rel.max()):.3e} (TAU / 4 = {TAU / 4:g}); cost >= "
          f"{float(com['cost'].min()):.3e}; accepted {rec['accepted'].tolist()} against {com['accepted'].tolist()}")
    above_zero = bool((com["cost"] > 1e-6 * (y.flatten(1) ** 2).sum(1)).all())
    holds = above_zero and bool((rel <= TAU / 4).all()) and bool((rec["info"] == 0).all()) and bool((com["info"] == 0).all())
    assert holds == (name in RR.SELECTION)
    if not holds:                                                    # c1_sphere_d2: 2 observed elements for d = 2, both costs are 0
        assert not above_zero and bool((rec["cost"] <= 1e-20).all()) and bool((com["cost"] <= 1e-20).all())


def test_at_least_two_selection_fixtures_qualify():
    assert len(RR.SELECTION) >= 2 and set(RR.SELECTION) <= {"c2a_power", "c2b_hepmass", "c1_sphere_d2"}


def test_underdetermined_problem_on_the_reference(models):
    """M = 5 < d = 10 on c2b_hepmass: the damped steps are solvable and lower the cost -- at least one accepted per sample --, while
    K^T K has rank M, so the closing system at lambda = 0 is singular."""
    name, M = RR.UNDERDETERMINED
    m = models(name)
    z0 = m.encode(m.y)
    x_on = m.decode(z0)
    A = RR.gaussian_operator(M, x_on[0].numel()).double()
    y = RR.measure(A, x_on)
    out = RR.recover(m, y, A, m.encode(RR.start_input(x_on)), steps=10)
    _, _, J = m.jacobian(out["latent"])
    G = torch.matmul(A, J)
    G = torch.bmm(G.transpose(1, 2), G)
    ev = torch.linalg.eigvalsh(G)
    print(f"{name}: M = {M}: accepted {out['accepted'].tolist()}; cost {float(out['initial_cost'].max()):.3e} -> "
          f"{float(out['cost'].max()):.3e}; eigenvalue {M + 1} from the top / largest <= {float((ev[:, -M - 1].abs() / ev[:, -1]).max()):.2e}")
    assert bool((out["costs"][1:] <= out["costs"][:-1]).all()) and bool((out["accepted"] >= 1).all())
    assert bool(torch.isfinite(out["latent"]).all())
    assert bool((ev[:, -M - 1].abs() <= 1e-12 * ev[:, -1]).all())     # rank M: the closing Cholesky has nothing to stand on


# --------------------------------------------------------------------------------------------------
# the public method and the engine wrappers: refusals
# --------------------------------------------------------------------------------------------------


def test_recover_refusals():
    import cmf_amd
    dens = small_density()
    proj = cmf_amd.ManifoldProjector(dens)
    d = proj.head.program.d
    A, y = torch.zeros(4, 6), torch.zeros(2, 4)
    with pytest.raises(ValueError, match=r"operator must be a contiguous float32 \(M, 6\)"):
        proj.recover(y, torch.zeros(4, 5))
    with pytest.raises(ValueError, match="operator must be a contiguous float32"):
        proj.recover(y, A.double())
    with pytest.raises(ValueError, match="operator must be a contiguous float32"):
        proj.recover(y, torch.zeros(6, 4).t())
    with pytest.raises(ValueError, match="operator must be a contiguous float32"):
        proj.recover(y, A.numpy())
    with pytest.raises(ValueError, match=r"measurements must be a contiguous float32 \(B, 4\)"):
        proj.recover(torch.zeros(2, 5), A)
    with pytest.raises(ValueError, match="measurements must be a contiguous float32"):
        proj.recover(y.double(), A)
    with pytest.raises(ValueError, match="not contiguous"):
        proj.recover(torch.zeros(4, 2).t(), A)
    with pytest.raises(ValueError, match="at least one sample"):
        proj.recover(y[:0], A)
    with pytest.raises(ValueError, match="steps >= 0"):
        proj.recover(y, A, steps=-1)
    with pytest.raises(ValueError, match="not both"):
        proj.recover(y, A, init=torch.zeros(2, d), x_init=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="init must be a contiguous float32"):
        proj.recover(y, A, init=torch.zeros(2, d + 1))
    with pytest.raises(ValueError, match="init must be a contiguous float32"):
        proj.recover(y, A, init=torch.zeros(2, d, dtype=torch.float64))
    with pytest.raises(ValueError, match="x_init must hold the 2 samples"):
        proj.recover(y, A, x_init=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="measurements must be on operator's device"):
        proj.recover(torch.zeros(2, 4, device="meta"), A)
    with pytest.raises(ValueError, match="init must be on operator's device"):
        proj.recover(y, A, init=torch.zeros(2, d, device="meta"))
    with pytest.raises(ValueError, match="x_init must be on operator's device"):
        proj.recover(y, A, x_init=torch.zeros(2, 6, device="meta"))
    # every argument in order and nothing on the GPU
    for kwargs in ({}, {"init": torch.zeros(2, d)}, {"x_init": torch.zeros(2, 6)}):
        with pytest.raises(ValueError, match="no CPU fallback"):
            proj.recover(y, A, **kwargs)


def test_engine_wrapper_refusals():
    from cmf_amd import engine as E
    T = E.Tangent(2, 6, 16, "panel", "cpu")
    with pytest.raises(ValueError, match="engine.Tangent"):
        E.operator_apply(T.data, torch.zeros(4, 6), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="a must be on the GPU"):
        E.operator_apply(T, torch.zeros(4, 6), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="a must be on the GPU"):
        E.operator_image(torch.zeros(4, 6), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.operator_image(np.zeros((4, 6), dtype=np.float32), torch.zeros(2, 6))
