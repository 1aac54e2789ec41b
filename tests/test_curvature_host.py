"""Curvature on the CPU, no GPU: the conditions the GPU tests assert of the product, established on the float64
reference pipeline (tests/_curvature_reference.py), and the numpy emulation of the kernel (tests/_second_form_emulation.py) held to
the kernel's bound forms on the very inputs the GPU tests use.

Truncation error of N at the default step against the exact second derivative, measured when this test was written (all samples, the
seeded frames, relative to max |N|):
    c1_sphere_d2 m=2 1.47e-4;  c2a_power m=2 3.06e-5;  c2b_hepmass m=2 8.74e-6, m=4 1.44e-5.
Reference asymmetry on the ReLU fixtures at the default step (float64): mini_mnist m=2 1.50, 2.00, 1.35; m=4 0.94,
1.55, 1.06; mini_cifar m=2 1.10, 1.51; m=4 0.59, 0.78 -- the frames' seed was chosen from the reference alone so that each is >= 0.5.

Emulation bounds: a quarter of the kernel's form wherever the a-priori rounding allows.  It does not for the row sums (trace S2 and the two asymmetry sums,
no other form) when D < 24 (a
chain of ceil(D / 256) + 6 + 3 additions, a product and two divisions against the quarter's (D + 4) / 2), for A at any D (its fold over
up to 64 row groups: D / RG + RG + 2 roundings a priori) and for ``frame_metric`` (two nested sums, (2 d + 1) u a priori against the
quarter's (d + 2) u / 2): those are held to the whole form."""
import numpy as np
import pytest
import torch

import _curvature_reference as CR
import _second_form_emulation as SE
import _transport_emulation as TE
from cmf_amd import engine as E
from cmf_amd.curvature import ManifoldCurvature

#: the product's own: every test below runs at the class's default step and within the engine's limits
DEFAULT_STEP = ManifoldCurvature.DEFAULT_STEP
WIDTHS = [d for d in SE.WIDTHS if d <= E.CURVATURE_MAX_WIDTH]
FRAMES = [m for m in SE.FRAMES if m <= E.CURVATURE_MAX_FRAME]
#: (fixture, m) -> the truncation error measured at DEFAULT_STEP
TRUNCATION = {("c1_sphere_d2", 2): 1.47e-4, ("c2a_power", 2): 3.06e-5, ("c2b_hepmass", 2): 8.74e-6, ("c2b_hepmass", 4): 1.44e-5}
#: the ReLU fixtures: every sample, the frames of ``_curvature_reference.RELU_SEED`` -- a seed picked from the float64 reference alone
RELU_CASES = [("mini_mnist", 2), ("mini_mnist", 4), ("mini_cifar", 2), ("mini_cifar", 4)]


def test_default_step_is_the_class_constant():
    assert ManifoldCurvature.DEFAULT_STEP == 2.0 ** -7                 # the step the recorded figures above were measured at
    assert E.CURVATURE_MAX_WIDTH == 128 and E.CURVATURE_MAX_FRAME == 4
    assert WIDTHS == SE.WIDTHS and FRAMES == SE.FRAMES


@pytest.mark.parametrize("name,m", sorted(TRUNCATION))
def test_truncation_error_at_the_default_step(name, m):
    exact = CR.run(name, m, CR.EXACT_STEP)[2]["second_gram"]
    at = CR.run(name, m, DEFAULT_STEP)[2]["second_gram"]
    err = CR.deviation(at, exact)
    print(f"{name} m={m}: truncation error of N at h = 2^-7: {err:.3e} (recorded {TRUNCATION[(name, m)]:.3e})")
    assert err <= 4.0 * TRUNCATION[(name, m)]


@pytest.mark.parametrize("name,m", sorted(TRUNCATION))
def test_riemann_symmetries(name, m):
    from cmf_amd.curvature import curvatures
    ref = CR.run(name, m, DEFAULT_STEP)[2]
    N, g = ref["second_gram"], ref["frame_metric"]
    stats = torch.stack([torch.zeros(len(N), dtype=torch.float64), torch.ones(len(N), dtype=torch.float64), ref["trace_s2"],
                         torch.diagonal(N, dim1=1, dim2=2).sum(1)], 1)
    out = curvatures(N, g, stats, m)
    Rm = out["riemann"]
    assert torch.equal(Rm, -Rm.transpose(1, 2)) and torch.equal(Rm, -Rm.transpose(3, 4)) and torch.equal(Rm, Rm.permute(0, 3, 4, 1, 2))
    bianchi = Rm + Rm.permute(0, 1, 3, 4, 2) + Rm.permute(0, 1, 4, 2, 3)                  # R_abcd + R_acdb + R_adbc
    assert float(bianchi.abs().max()) <= 8 * 2.0 ** -53 * float(N.abs().max())
    # the product's torch helpers against the reference's loops
    assert float((Rm - ref["riemann"]).abs().max()) == 0.0
    for key in ("sectional", "scalar", "normal_curvature"):
        assert float((out[key] - ref[key]).abs().max()) <= 1e-12 * float(ref[key].abs().max()) + 1e-300, key
    if m == 2 and g.shape[1] == 2:
        assert float((out["scalar"] - 2.0 * out["sectional"][:, 0, 1]).abs().max()) <= 1e-12 * float(out["scalar"].abs().max())


@pytest.mark.parametrize("k1,k2,x,y", [(1.0, 2.0, 0.5, -0.25), (2.0, -1.0, 0.25, 0.5), (0.5, 0.5, 0.0, 0.0), (3.0, 0.0, 1.0, 1.0)])
def test_gauss_theorem_on_a_quadric(k1, k2, x, y):
    J, Dm, want = CR.quadric(k1, k2, x, y)
    ref = CR.forms(J, Dm, torch.eye(2, dtype=torch.float64)[None])
    K = float(ref["sectional"][0, 0, 1])
    assert abs(K - want) <= 1e-13 * max(abs(want), 1.0)
    assert abs(float(ref["scalar"][0]) - 2.0 * want) <= 1e-13 * max(abs(want), 1.0)
    assert float(ref["asymmetry"][0]) == 0.0


@pytest.mark.parametrize("d", WIDTHS)
def test_emulation_meets_the_kernel_bounds(d):
    worst = {}
    for m in FRAMES:
        if m > d:
            continue
        for D in SE.rows_of(d):
            cs = SE.case(SE.BATCHES[-1], d, m, D)
            got = SE.batch(*cs)
            assert (got[4] == 0).all()
            for k, v in SE.worst_ratios(cs, got).items():
                whole = k in ("metric", "A") or (k in ("S2", "asym") and D < 24)
                assert v <= (1.0 if whole else 0.25), (m, D, k, v)
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"d={d}: emulation, worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_emulation_elimination_is_the_transport_emulations():
    cs = SE.case(1, 17, 3, 20)
    got = SE.batch(*cs)
    assert np.array_equal(TE.chol_solve(TE.symmetric(cs[1][0]), got[5][0].T.copy()), got[1][0])


def test_emulation_known_answers_and_codes():
    Q = np.diag([1.0, 2.0])[None]
    z = np.array([0.5, -0.25])
    cs, _ = SE.quadratic_graph(Q, z, np.eye(2), 2.0 ** -3)
    N, _, g, st, info, _ = (v[0] for v in SE.batch(*cs))
    K = (N[0, 2] - N[1, 1]) / (g[0, 0] * g[1, 1] - g[0, 1] ** 2)
    assert info == 0 and st[0] == 0.0 and abs(K - 2.0 / (1.0 + z[0] ** 2 + 4.0 * z[1] ** 2) ** 2) <= 1e-14
    cs = SE.flat(5, 3, 9, 2.0 ** -4)
    got = SE.batch(*cs)
    assert got[4][0] == 0 and got[3][0, 2] >= 1.0 and SE.worst_ratios(cs, got)["N"] <= 0.25
    Jd, jtj, Sd, frame, step, nc = (np.array(v) if isinstance(v, np.ndarray) else v for v in SE.case(3, 5, 2, 8))
    Jd[0, :, 1] = 0.0
    jtj[0, 1, :2] = 0.0
    jtj[0, 1:, 1] = 0.0
    step[1] = -1.0
    got = SE.batch(Jd, jtj, Sd, frame, step, nc)
    assert got[4].tolist() == [1, 2, 0]
    assert np.isnan(got[0][0]).all() and np.isfinite(got[2][0]).all() and np.isnan(got[3][0, 3]) and np.isfinite(got[3][0, :3]).all()
    assert all(np.isnan(got[i][1]).all() for i in range(4))


@pytest.mark.parametrize("name,m", RELU_CASES)
def test_relu_fixtures_are_flagged_by_the_reference(name, m):
    asym = CR.run(name, m, DEFAULT_STEP, seed=CR.RELU_SEED)[2]["asymmetry"]
    print(f"{name} m={m}: reference asymmetry at h = 2^-7: {[round(float(a), 3) for a in asym]}")
    assert float(asym.min()) >= 0.5
