"""Geodesic shooting on the float64 reference loop (tests/_shoot_reference.py), CPU only: the conditions the GPU tests
assert of ``cmf_amd.ManifoldGeodesic.shoot`` / ``log`` are established here first.  Measured values in brackets.

    p' against central differences of H = 1/2 p^T G^-1 p (step 1e-5), c1_sphere_d2 and c2a_power:   relative <= 1e-8   [5e-10]
    end point change from S = 8 to 16 over the change from 4 to 8 (fourth order), tanh-MLP fixtures:  <= 1/8             [1/16]
    max |speed2 / speed2_0 - 1| at S = 8, tanh-MLP fixtures:                                          <= 1e-4            [<= 2.3e-5]
    shoot to time 1, shoot back with -v from the end, tanh-MLP fixtures: return to z_0 within         1e-5 ||v_0||       [9e-7]
    shoot(log) at S = 8, all five fixtures (points = 9, steps = 10): ||g(z_S) - g(z_1)|| / length     <= 2e-2            [2.9e-3 .. 1.05e-2]
    that miss over the miss of the straight chord z_1 - z_0, tanh-MLP fixtures:                       <= 0.1             [<= 0.047]
    sqrt(speed2_0) / relaxed length, all five fixtures:                                                within 1 % of 1    [0.993 .. 1.002]

No energy conservation is asserted on the ResNet fixtures: their couplers are piecewise linear and ``speed2`` jumps at ReLU
boundaries by amounts that do not shrink with the step (mini_mnist 2 - 3 %, mini_cifar 0.6 - 0.8 %)."""
import pytest
import torch

import _shoot_reference as R


@pytest.fixture(autouse=True, scope="module")
def product_has_the_loop():
    """The conditions are those of the product's loop: without it they establish nothing."""
    from cmf_amd import ManifoldGeodesic
    from cmf_amd import engine as E
    assert E.SHOOT_MAX_WIDTH == 128 and callable(E.metric_solve)
    for method in ("shoot", "shoot_latents", "shoot_evaluate", "log", "log_latents"):
        assert callable(getattr(ManifoldGeodesic, method))


def miss(model, run, z1):
    """||g(z_S) - g(z_1)|| per trajectory."""
    with torch.no_grad():
        return (run["path_head"][:, -1] - model.decode(z1).flatten(1)).norm(dim=1)


@pytest.mark.parametrize("name", ["c1_sphere_d2", "c2a_power"])
def test_momentum_rate_is_minus_the_gradient_of_the_hamiltonian(name):
    model, z0, z1 = R.ends(name)
    p = torch.bmm(R.metric(model, z0), (z1 - z0)[:, :, None])[:, :, 0]
    dp = R.evaluate(model, z0, p)[0]
    fd, eps = torch.zeros_like(dp), 1e-5
    for k in range(z0.shape[1]):
        e = torch.zeros_like(z0)
        e[:, k] = eps
        fd[:, k] = -(R.hamiltonian(model, z0 + e, p) - R.hamiltonian(model, z0 - e, p)) / (2 * eps)
    rel = float((dp - fd).abs().max() / fd.abs().max())
    print(f"{name}: |p' + dH/dz| / |dH/dz| = {rel:.2e}")
    assert rel <= 1e-8


@pytest.mark.parametrize("name", R.MLP)
def test_fourth_order_and_conserved_speed(name):
    model, z0, z1 = R.ends(name)
    end = {S: (R.chord_run(name)[3] if S == R.STEPS else R.shoot(model, z0, z1 - z0, steps=S)) for S in (4, 8, 16)}
    fine = (end[16]["latents"][:, -1] - end[8]["latents"][:, -1]).norm(dim=1)
    coarse = (end[8]["latents"][:, -1] - end[4]["latents"][:, -1]).norm(dim=1)
    s2 = end[8]["speed2"]
    drift = float((s2 / s2[:, :1] - 1).abs().max())
    print(f"{name}: end point change 8 -> 16 over 4 -> 8: max {float((fine / coarse).max()):.4f}; max |speed2 / speed2_0 - 1| = {drift:.2e}")
    assert bool((fine <= coarse / 8).all())
    assert drift <= 1e-4
    length = end[8]["length"]
    assert bool(((length - s2[:, 0].sqrt()).abs() <= 1e-4 * length).all())          # constant speed: length = speed x time


@pytest.mark.parametrize("name", R.MLP)
def test_shooting_back_returns_to_the_start(name):
    model, z0, z1, out = R.chord_run(name)
    back = R.shoot(model, out["latents"][:, -1], -out["velocity"][:, -1])
    gap = (back["latents"][:, -1] - z0).norm(dim=1) / (z1 - z0).norm(dim=1)
    print(f"{name}: ||z_back - z_0|| / ||v_0|| max {float(gap.max()):.2e}")
    assert bool((gap <= 1e-5).all())


@pytest.mark.parametrize("name", R.FIXTURES)
def test_shooting_the_logarithm_arrives(name):
    model, z0, z1, relaxed = R.log_run(name)
    v0 = R.log_velocity(relaxed["latents"])
    out = R.shoot(model, z0, v0)
    rel = miss(model, out, z1) / relaxed["length"]
    speed = out["speed2"][:, 0].sqrt() / relaxed["length"]
    print(f"{name}: miss / length in [{float(rel.min()):.2e}, {float(rel.max()):.2e}]; sqrt(speed2_0) / length in "
          f"[{float(speed.min()):.4f}, {float(speed.max()):.4f}]")
    assert bool((rel <= 2e-2).all())
    assert bool(((speed - 1).abs() <= 0.01).all())
    if name in R.MLP:
        chord = miss(model, R.shoot(model, z0, z1 - z0), z1)
        print(f"{name}: miss over the straight chord's in [{float((rel * relaxed['length'] / chord).min()):.3f}, "
              f"{float((rel * relaxed['length'] / chord).max()):.3f}]; the chord misses by "
              f"{float((chord / relaxed['length']).min()):.3f} .. {float((chord / relaxed['length']).max()):.3f} of the length")
        assert bool((rel * relaxed["length"] <= 0.1 * chord).all())


def test_refusals_without_a_gpu():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    assert "cmf_metric_solve" in _lib.SIGNATURES and len(_lib.SIGNATURES["cmf_metric_solve"][1]) == 10
    with pytest.raises(ValueError, match="GPU"):
        E.metric_solve(torch.zeros(2, 3, 3), torch.zeros(2, 3, dtype=torch.float64))
