"""Host-side checks of the weighted projection (no GPU): the numpy emulation of the weighted step kernel against
float64, the Gram bound's constant and the planted defects it must catch, the float64 reference loop on the fixtures -- the
conditions tests/test_gpu_completion.py asserts of the product are established here on the reference alone --, the data sensitivity
its end-to-end tolerance is derived from, the refusals of ``ManifoldProjector.complete`` and the weight mapping through the wrapper
chain."""
import math

import numpy as np
import pytest
import torch

import _completion_reference as CR
import _gn_step_emulation as GN
import _projection_reference as R
import _weighted_step_emulation as WS
from test_projection_host import small_density

FIXTURES = ["c2b_hepmass", "c2a_power", "c1_sphere_d2", "mini_mnist", "mini_mnist_small", "mini_cifar"]


@pytest.fixture(scope="module")
def models():
    cache = {}
    return lambda name: cache.setdefault(name, R.Model(name))


# --------------------------------------------------------------------------------------------------
# the emulation and the Gram constant
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", GN.WIDTHS)
@pytest.mark.parametrize("D", GN.ROWS)
def test_emulation_solves_the_weighted_normal_equations(D, d):
    B = WS.batch_size()
    J, _, x, xhat = GN.inputs(B, D, d)
    w = WS.weights(B, D, d)
    lam = np.array([GN.DAMPINGS[b % len(GN.DAMPINGS)] for b in range(B)])
    # the rows with w == 0 are never touched
    dead = w == 0
    Jn, xn, hn = J.copy(), x.copy(), xhat.copy()
    Jn[dead], xn[dead], hn[dead] = np.nan, np.nan, np.nan
    gram, grad, delta, stats, info = WS.batch(Jn, w, xn, hn, lam)
    r = x.astype(np.float64) - xhat.astype(np.float64)
    for b in range(B):
        J64, w64 = J[b].astype(np.float64), w[b].astype(np.float64)
        G64, S = WS.gram64(J[b], w[b])
        assert WS.gram_ratio(gram[b], G64, S) <= WS.C_WGRAM / 4 and np.array_equal(gram[b], gram[b].T)
        g_ref, g_abs = J64.T @ (w64 * r[b]), np.abs(J64).T @ (w64 * np.abs(r[b]))
        assert (np.abs(grad[b] - g_ref) <= 2 * (D + 3) * GN.U * g_abs).all()
        assert stats[b, 0] == pytest.approx(float((w64 * r[b]) @ r[b]), rel=1e-13) and stats[b, 3] == np.abs(grad[b]).max()
        n_live = int((w[b] > 0).sum())
        if n_live == 0:
            assert info[b] == 1 and (gram[b] == 0).all() and (grad[b] == 0).all() and stats[b, 0] == 0
        elif n_live < d and lam[b] == 0.0:
            assert info[b] in (0, 1)               # G_w of rank < d: a refused pivot and a completed factorisation are both legitimate
        else:
            assert info[b] == 0
        if info[b] == 1:
            assert np.isnan(delta[b]).all() and np.isnan(stats[b, 1:3]).all()
            continue
        assert GN.residual_ratio(gram[b], lam[b], grad[b], delta[b]) <= GN.BOUND_C / 4


def test_gram_constant_and_planted_defects():
    """C_WGRAM is 4 x (rounded up to a power of two) the emulation's worst error on the GPU test's own inputs, and the emulation with
    a planted defect lands above it on every sample the defect changes."""
    worst, least = 0.0, {"unweighted": math.inf, "squared": math.inf, "dropped": math.inf}
    for D in GN.ROWS:
        for d in GN.WIDTHS:
            B = WS.batch_size()
            J = GN.inputs(B, D, d)[0]
            w = WS.weights(B, D, d)
            for b in range(B):
                G64, S = WS.gram64(J[b], w[b])
                worst = max(worst, WS.gram_ratio(WS.gram32(J[b], w[b]), G64, S))
                kind = WS.PATTERNS[b % len(WS.PATTERNS)]
                n_live = int((w[b] > 0).sum())
                if n_live == 0:
                    continue
                for defect in least:
                    if defect != "dropped" and kind not in ("third", "few"):
                        continue                    # weights of 0 / 1: ignoring or squaring them changes nothing
                    least[defect] = min(least[defect], WS.gram_ratio(WS.gram32(J[b], w[b], defect), G64, S))
    print(f"emulation against float64: worst |G_w - G_w64| / S = 2^{math.log2(worst):.2f} (C_WGRAM = 2^{math.log2(WS.C_WGRAM):g}); "
          f"planted defects, least: " + ", ".join(f"{k} 2^{math.log2(v):.2f}" for k, v in least.items()))
    assert WS.C_WGRAM == CR.pow2_ceil(4 * worst)
    assert all(v > WS.C_WGRAM for v in least.values())


def test_emulation_info_codes():
    J, _, x, xhat = GN.inputs(8, 64, 5, seed=1)
    w = np.ones((8, 64), dtype=np.float32)
    w[:, ::3] = 0.0                                                  # rows 0, 3, 6, ... are dead
    lam = np.zeros(8)
    clean = WS.batch(J, w, x, xhat, lam)
    assert (clean[4] == 0).all()
    w[1, 4] = -1.0
    w[2, 5] = np.nan
    x[3, 7] = np.inf                                                 # live rows
    xhat[4, 1] = np.nan
    J[5, 2, 4] = np.nan
    x[6, 3], xhat[6, 6], J[6, 9, 1] = np.nan, np.inf, np.nan         # dead rows: not an error
    w[7] = 0.0
    gram, grad, delta, stats, info = WS.batch(J, w, x, xhat, lam)
    assert info.tolist() == [0, 2, 2, 2, 2, 2, 0, 1]
    for b in (1, 2, 3, 4, 5):
        assert all(np.isnan(o[b]).all() for o in (gram, grad, delta, stats))
    for got, want in zip((gram, grad, delta, stats), clean):
        assert np.array_equal(got[[0, 6]], want[[0, 6]])
    assert np.isnan(delta[7]).all() and (gram[7] == 0).all() and stats[7, 0] == 0 and stats[7, 3] == 0
    _, _, _, s, i = WS.batch(None, w, x, xhat, None)
    assert i.tolist() == [0, 2, 2, 2, 2, 0, 0, 0] and np.array_equal(s[[0, 6, 7], 0], stats[[0, 6, 7], 0])


# --------------------------------------------------------------------------------------------------
# the float64 reference loop
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_loop_finds_the_known_answer(name, models):
    """Half of the elements observed with weights in [0.25, 4], the hidden ones off by 0.1 ||x_on|| / sqrt(D) randn: ten steps from
    the encoder's latent of that input end on the true latent."""
    m = models(name)
    z0 = m.encode(m.y)
    x_on = m.decode(z0)
    y, w = CR.problem(x_on, seed=0)
    out = CR.complete(m, y, w, steps=10)
    err = float((out["latent"] - z0).abs().max())
    drop = float((out["initial_cost"] / out["cost"].clamp_min(1e-300)).min())
    print(f"{name}: max |z - z0| = {err:.2e}; accepted {out['accepted'].tolist()}; initial_cost / cost >= {drop:.2e}")
    assert err <= 1e-11
    assert bool((out["info"] == 0).all()) and bool((out["costs"][1:] <= out["costs"][:-1]).all())
    assert bool((out["cost"] * 1e6 < out["initial_cost"]).all())
    assert out["observed"].tolist() == [math.ceil(0.5 * x_on[0].numel())] * len(x_on)
    assert torch.equal(out["reconstruction_head"], m.decode(out["latent"]))


@pytest.mark.parametrize("name", CR.KNOWN_ANSWER)
def test_data_sensitivity_sets_the_gpu_tolerance(name, models):
    """How far DESIGN 5's x_hat tolerance, as a perturbation of the observed data, moves the completed point: the measurement
    the GPU end-to-end tolerance ``CR.E2E_TOL`` is 4 x (rounded up to a power of two) of."""
    m = models(name)
    z0 = m.encode(m.y)
    x_on = m.decode(z0)
    y, w = CR.problem(x_on, seed=0, data_rel=CR.DATA_REL)
    out = CR.complete(m, y, w, steps=10)
    worst = float(CR.rel_distance(out["reconstruction_head"], x_on).max())
    print(f"{name}: worst ||g(z) - x_on|| / ||x_on|| under a {CR.DATA_REL:g} data perturbation = {worst:.3e}; "
          f"E2E_TOL = 2^{math.log2(CR.E2E_TOL[name]):g} = {CR.E2E_TOL[name]:.3e}")
    assert bool((out["info"] == 0).all())
    assert CR.E2E_TOL[name] == CR.pow2_ceil(4 * worst)


# --------------------------------------------------------------------------------------------------
# the public method: refusals and the weight mapping
# --------------------------------------------------------------------------------------------------


def test_complete_refusals():
    import cmf_amd
    from cmf_amd import bijections as Bj
    dens = small_density()
    proj = cmf_amd.ManifoldProjector(dens)
    d = proj.head.program.d
    x = torch.zeros(2, 6)
    with pytest.raises(ValueError, match="x's shape"):
        proj.complete(x, torch.ones(2, 5))
    with pytest.raises(ValueError, match="x's shape"):
        proj.complete(x, torch.ones(3, 6))
    with pytest.raises(ValueError, match="floating point or bool"):
        proj.complete(x, torch.ones(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="x's device"):
        proj.complete(x, torch.ones(2, 6, device="meta"))
    with pytest.raises(ValueError, match="init must be"):
        proj.complete(x, torch.ones(2, 6), init=torch.zeros(2, d + 1))
    with pytest.raises(ValueError, match="init must be"):
        proj.complete(x, torch.ones(2, 6), init=torch.zeros(2, d, dtype=torch.float64))
    with pytest.raises(ValueError, match="x's device"):
        proj.complete(x, torch.ones(2, 6), init=torch.zeros(2, d, device="meta"))
    with pytest.raises(ValueError, match="steps >= 0"):
        proj.complete(x, torch.ones(2, 6), steps=-1)
    # every argument in order and nothing on the GPU: the same refusal as ``project``
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proj.complete(x, torch.ones(6, dtype=torch.bool), init=torch.zeros(2, d))
    # a chain element that mixes elements
    proj.chain = [Bj.LULinearBijection(6)]
    with pytest.raises(NotImplementedError, match="weights cannot be carried"):
        proj.complete(x, torch.ones(2, 6))


def test_weights_follow_the_data_through_the_wrapper_chain():
    from cmf_amd import bijections as Bj
    from cmf_amd.projection import to_head_space_weights
    gen = torch.Generator().manual_seed(5)
    # elementwise bijections: the same tensor
    w = torch.rand(3, 2, 4, 4, generator=gen)
    chain = [Bj.ScalarAdditionBijection((2, 4, 4), 0.5), Bj.ScalarMultiplicationBijection((2, 4, 4), 1 / 256), Bj.LogitBijection((2, 4, 4)),
             Bj.AffineBijection((2, 4, 4))]
    assert to_head_space_weights(chain, w) is w
    # squeeze, then flatten: the permutation x_to_z applies to data (z[r] = x[x2z[r]], the index map its gather kernel takes)
    squeeze, flat = Bj.Squeeze2dBijection((2, 4, 4), 2), Bj.ViewBijection((8, 2, 2), (32,))
    got = to_head_space_weights([chain[0], squeeze, chain[2], flat], w)
    x2z = torch.from_numpy(squeeze._maps._host["x2z"]).long()
    assert got.shape == (3, 32) and torch.equal(got, w.reshape(3, -1)[:, x2z])
    # the index map is the bijection's own reshaping of positions: element (c, 2 i + a, 2 j + b) lands in channel 4 c + 2 a + b
    ids = torch.arange(32.0).view(1, 2, 4, 4)
    moved = to_head_space_weights([squeeze], ids)
    assert torch.equal(moved, squeeze._reshape_x(ids)) and moved[0, 4 * 1 + 2 * 1 + 0, 1, 1] == ids[0, 1, 2 * 1 + 1, 2 * 1 + 0]
    assert torch.equal(squeeze._reshape_z(moved), ids)               # and z_to_x undoes it
    # bool masks and a single-sample batch go the same way
    mask = torch.rand(1, 2, 4, 4, generator=gen) < 0.5
    assert torch.equal(to_head_space_weights([squeeze, flat], mask), mask.reshape(1, -1)[:, x2z])
    with pytest.raises(NotImplementedError, match="weights cannot be carried"):
        to_head_space_weights([Bj.LULinearBijection(32)], w.reshape(3, 32))
