"""Host-side checks of the robust projection (no GPU): the numpy model of the robust weights kernel against direct
numpy, the planted defects the GPU test's checks must catch, the float64 reference loop on the fixtures -- the conditions
tests/test_gpu_robust.py asserts of the product are established here on the reference alone --, the data sensitivity its end-to-end
tolerance is derived from, the refusals of ``ManifoldProjector.robust`` and the weight mapping back through the wrapper chain."""
import math

import numpy as np
import pytest
import torch

import _completion_reference as CR
import _projection_reference as R
import _robust_reference as RR
import _robust_weights_emulation as RW
from test_projection_host import small_density


@pytest.fixture(scope="module")
def models():
    cache = {}
    return lambda name: cache.setdefault(name, R.Model(name))


# --------------------------------------------------------------------------------------------------
# the model of the kernel
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prior_kind", RW.PRIORS)
@pytest.mark.parametrize("n", RW.SIZES)
def test_model_against_direct_numpy(n, prior_kind):
    x, xhat, prior, scale, kinds = RW.inputs(n, prior_kind)
    for loss in ("huber", "tukey"):
        c = RW.TUNING[loss]
        w, stats, info, _ = RW.batch(x, xhat, prior, loss, c)
        for b in range(len(x)):
            p = np.ones(n) if prior is None else prior[b].astype(np.float64)
            used = p > 0
            r = (x[b].astype(np.float64) - xhat[b].astype(np.float64))[used]
            m = int(used.sum())
            assert info[b] in (0, 3)
            if m == 0:
                assert info[b] == 3 and np.isnan(stats[b]).all() and np.isnan(w[b]).all()
                continue
            a = np.abs(r)
            med = np.partition(a, (m - 1) // 2)[(m - 1) // 2]
            if m % 2:
                assert med == np.median(a)
            assert (a <= med).sum() >= (m - 1) // 2 + 1 and (a < med).sum() <= (m - 1) // 2
            assert stats[b, 0] == 1.4826 * med and not np.signbit(stats[b, 0])
            if med == 0:
                assert info[b] == 3 and np.isnan(stats[b, 1:]).all() and np.isnan(w[b]).all()
                continue
            # (with a third of the elements unused, the zeros among the used ones need not be more than half)
            assert info[b] == 0 and stats[b, 2] == m and (kinds[b] != "zeros" or prior_kind == "third")
            u = r / stats[b, 0]
            if loss == "huber":
                om = np.minimum(1.0, c / np.maximum(np.abs(u), 1e-300))
                rho = np.where(np.abs(u) <= c, 0.5 * u ** 2, c * (np.abs(u) - 0.5 * c))
            else:
                om = np.where(np.abs(u) < c, (1 - (u / c) ** 2) ** 2, 0.0)
                rho = np.where(np.abs(u) < c, c * c / 6 * (1 - (1 - (u / c) ** 2) ** 3), c * c / 6)
            assert np.allclose(w[b][used], p[used] * om, rtol=1e-6, atol=0) and (w[b][~used].view(np.int32) == 0).all()
            assert stats[b, 1] == pytest.approx(2 * stats[b, 0] ** 2 * float((p[used] * rho).sum()), rel=1e-12)
            assert stats[b, 3] == pytest.approx(float(om.sum()), rel=1e-12)


def test_the_cost_is_the_weighted_sum_of_squares_where_nothing_is_down_weighted():
    x, xhat, prior, scale, _ = RW.inputs(784, "positive")
    w, stats, info, _ = RW.batch(x, xhat, prior, "huber", 1e100, scale)      # the "huge" pattern has |u| ~ 1e31
    r = x.astype(np.float64) - xhat.astype(np.float64)
    assert (info == 0).all() and np.array_equal(w, prior)
    assert np.allclose(stats[:, 1], (prior * r * r).sum(1), rtol=1e-12) and (stats[:, 3] == 784).all()


def test_model_info_codes():
    x, xhat, prior, scale, _ = RW.inputs(64, "third", B=6)
    x[:, :], xhat[:, :] = np.float32(1.0), np.float32(0.5)
    x[:, ::2] = 2.0
    clean = RW.batch(x, xhat, prior, "huber", 1.345)
    assert (clean[2] == 0).all()
    prior[1, int(np.nonzero(prior[1])[0][0])] = -1.0
    prior[2, 0] = np.nan
    x[3, int(np.nonzero(prior[3])[0][0])] = np.inf
    xhat[4, int(np.nonzero(prior[4] == 0)[0][0])] = np.nan         # an unused element: not an error
    prior[5] = 0.0
    w, stats, info, _ = RW.batch(x, xhat, prior, "huber", 1.345)
    assert info.tolist() == [0, 2, 2, 2, 0, 3]
    assert all(np.isnan(w[b]).all() and np.isnan(stats[b]).all() for b in (1, 2, 3, 5))
    assert np.array_equal(w[[0, 4]], clean[0][[0, 4]]) and np.array_equal(stats[[0, 4]], clean[1][[0, 4]])
    _, stats, info, _ = RW.batch(x, xhat, prior, "huber", 1.345, np.array([1.0, 1.0, 1.0, 1.0, 0.0, 1.0]))
    assert info.tolist() == [0, 2, 2, 2, 3, 0] and stats[4, 0] == 0.0 and stats[5].tolist() == [1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("defect", RW.DEFECTS)
def test_planted_defects_break_the_gpu_checks(defect):
    """The model with a planted defect, judged as the GPU test judges the kernel -- ``RW.mismatches`` against the sound model --
    fails on at least one generated sample, and the sound model passes on all of them."""
    caught = []
    for n in RW.SIZES:
        for prior_kind in RW.PRIORS:
            x, xhat, prior, scale, _ = RW.inputs(n, prior_kind)
            for loss in ("huber", "tukey"):
                c = RW.TUNING[loss]
                for given in (None, scale):
                    ref = RW.batch(x, xhat, prior, loss, c, given)
                    assert RW.mismatches(ref[:3], ref, prior) == []
                    caught += [(n, prior_kind, loss, given is not None, b, what)
                               for b, what in RW.mismatches(RW.batch(x, xhat, prior, loss, c, given, defect)[:3], ref, prior)]
    print(f"{defect}: caught on {len(caught)} samples, e.g. {caught[:3]}")
    assert caught
    if defect in ("upper_median", "median_ignores_prior", "no_mad_factor"):
        assert any(what == "scale or used" for *_, what in caught) and not any(given for _, _, _, given, _, _ in caught)
    if defect == "tukey_no_square":
        assert all(loss == "tukey" for _, _, loss, *_ in caught)
    if defect == "cost_without_prior":
        assert {what for *_, what in caught} == {"cost"} and {k for _, k, *_ in caught} == {"positive"}


# --------------------------------------------------------------------------------------------------
# the float64 reference loop
# --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def solved(models):
    cache = {}

    def get(name):
        if name not in cache:
            m = models(name)
            x_on = m.decode(m.encode(m.y))
            y, planted = RR.problem(x_on, RR.KNOWN_ANSWER[name], seed=RR.SEED)
            out = RR.robust(m, y, steps=10)
            cache[name] = {"x_on": x_on, "y": y, "planted": planted, "robust": out,
                           "mask": CR.complete(m, y, (~planted).double(), steps=10), "project": R.project(m, y, steps=10),
                           "tukey": RR.robust(m, y, loss="tukey", steps=10, z=out["latent"])}
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_reference_loop_finds_the_outliers_nobody_marked(name, models, solved):
    s = solved(name)
    out, x_on, planted = s["robust"], s["x_on"], s["planted"]
    rel = {k: CR.rel_distance(s[k]["reconstruction_head"], x_on) for k in ("robust", "mask", "project", "tukey")}
    w = out["weights"]
    cond = RR.conditions(rel["robust"], rel["mask"], rel["project"], w, planted, out["cost"], out["initial_cost"])
    cond["e"] = bool(rel["tukey"].max() <= RR.MASK_FACTOR * rel["mask"].max())
    print(f"{name}: worst ||g(z) - x_on|| / ||x_on||: robust {float(rel['robust'].max()):.3e}, complete with the true mask "
          f"{float(rel['mask'].max()):.3e}, project {float(rel['project'].max()):.3e}, tukey from the Huber latent "
          f"{float(rel['tukey'].max()):.3e}; (a) {float(rel['robust'].max() / rel['mask'].max()):.2f} (b) "
          f"{float(rel['project'].max() / rel['robust'].max()):.1f}; weights: planted <= {float(w[planted].max()):.3e}, others >= "
          f"{float(w[~planted].min()):.3e}; accepted {out['accepted'].tolist()}")
    assert cond == {k: True for k in "abcde"}
    assert bool((out["info"] == 0).all()) and bool((out["costs"][1:] <= out["costs"][:-1]).all())
    assert torch.equal(out["reconstruction_head"], models(name).decode(out["latent"]))
    assert int(planted.flatten(1).sum(1)[0]) == math.ceil(RR.KNOWN_ANSWER[name] * x_on[0].numel())
    # the Tukey weights of the planted outliers are exactly zero
    assert bool((s["tukey"]["weights"][planted] == 0).all())


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_rounds_keep_the_cost_monotone_within_a_round(name, models, solved):
    s = solved(name)
    out = RR.robust(models(name), s["y"], steps=4, rounds=2)
    assert bool((out["costs"][1:] <= out["costs"][:-1]).all()) and bool((out["cost"] <= out["initial_cost"]).all())
    assert bool((out["accepted"] <= 8).all())


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_data_sensitivity_sets_the_gpu_tolerance(name, models, solved):
    """How far DESIGN 5's x_hat tolerance, as a perturbation of the data, moves the robust answer: the measurement the GPU
    end-to-end tolerance ``RR.E2E_TOL`` is 4 x (rounded up to a power of two) of."""
    s = solved(name)
    y, _ = RR.problem(s["x_on"], RR.KNOWN_ANSWER[name], seed=RR.SEED, data_rel=RR.DATA_REL)
    out = RR.robust(models(name), y, steps=10)
    worst = float(CR.rel_distance(out["reconstruction_head"], s["robust"]["reconstruction_head"]).max())
    print(f"{name}: worst movement of g(z) under a {RR.DATA_REL:g} data perturbation = {worst:.3e}; "
          f"E2E_TOL = 2^{math.log2(RR.E2E_TOL[name]):g} = {RR.E2E_TOL[name]:.3e}")
    assert bool((out["info"] == 0).all())
    assert RR.E2E_TOL[name] == CR.pow2_ceil(4 * worst)


@pytest.mark.parametrize("name", ["c2b_hepmass", "c2a_power"])
def test_without_redundancy_the_reference_loop_cannot_separate_outliers(name, models):
    """D = 21, d = 10 and D = 6, d = 2: what ``robust``'s docstring says of the tabular configurations, measured -- even started at
    the true latent, the float64 loop ends where ``project`` ends, far from where the true mask leads."""
    m = models(name)
    z0 = m.encode(m.y)
    x_on = m.decode(z0)
    y, planted = RR.problem(x_on, 0.10, seed=0)
    out, proj = RR.robust(m, y, steps=10, z=z0), R.project(m, y, steps=10, z=z0)
    mask = CR.complete(m, y, (~planted).double(), steps=10, z=z0)
    rr, rp, rm = (float(CR.rel_distance(o["reconstruction_head"], x_on).max()) for o in (out, proj, mask))
    print(f"{name}: robust {rr:.2e}, project {rp:.2e}, complete with the true mask {rm:.2e}")
    assert rr > 0.5 * rp and rr > 5 * rm


# --------------------------------------------------------------------------------------------------
# the public method: refusals and the weight mapping
# --------------------------------------------------------------------------------------------------


def test_robust_refusals():
    import cmf_amd
    from cmf_amd import bijections as Bj
    dens = small_density()
    proj = cmf_amd.ManifoldProjector(dens)
    d = proj.head.program.d
    x = torch.zeros(2, 6)
    with pytest.raises(ValueError, match="loss must be"):
        proj.robust(x, loss="cauchy")
    for tuning in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="tuning must be > 0"):
            proj.robust(x, tuning=tuning)
    for rounds in (0, -1, 1.5):
        with pytest.raises(ValueError, match="rounds must be"):
            proj.robust(x, rounds=rounds)
    with pytest.raises(ValueError, match="needs rounds == 1"):
        proj.robust(x, scale=0.1, rounds=2)
    for scale in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale must be > 0"):
            proj.robust(x, scale=scale)
    with pytest.raises(ValueError, match="scale must be a float"):
        proj.robust(x, scale=torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="scale must be a float"):
        proj.robust(x, scale=torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="x's device"):
        proj.robust(x, scale=torch.ones(2, device="meta"))
    with pytest.raises(ValueError, match="x's shape"):
        proj.robust(x, weights=torch.ones(2, 5))
    with pytest.raises(ValueError, match="floating point or bool"):
        proj.robust(x, weights=torch.ones(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="x's device"):
        proj.robust(x, weights=torch.ones(2, 6, device="meta"))
    with pytest.raises(ValueError, match="init must be"):
        proj.robust(x, init=torch.zeros(2, d + 1))
    with pytest.raises(ValueError, match="x's device"):
        proj.robust(x, init=torch.zeros(2, d, device="meta"))
    with pytest.raises(ValueError, match="steps >= 0"):
        proj.robust(x, steps=-1)
    with pytest.raises(ValueError, match="at least one sample"):
        proj.robust(x[:0])
    # every argument in order and nothing on the GPU: the same refusal as ``project``
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proj.robust(x, loss="tukey", tuning=3.0, scale=torch.ones(2), weights=torch.ones(6, dtype=torch.bool), init=torch.zeros(2, d), rounds=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proj.robust(x, rounds=3)
    # a chain element that mixes elements
    proj.chain = [Bj.LULinearBijection(6)]
    with pytest.raises(NotImplementedError, match="weights cannot be carried"):
        proj.robust(x)


def test_weights_come_back_through_the_wrapper_chain():
    from cmf_amd import bijections as Bj
    from cmf_amd.projection import to_data_space_weights, to_head_space_weights
    gen = torch.Generator().manual_seed(6)
    w = torch.rand(3, 2, 4, 4, generator=gen)
    elementwise = [Bj.ScalarAdditionBijection((2, 4, 4), 0.5), Bj.ScalarMultiplicationBijection((2, 4, 4), 1 / 256),
                   Bj.LogitBijection((2, 4, 4)), Bj.AffineBijection((2, 4, 4))]
    assert to_data_space_weights(elementwise, w) is w
    squeeze, flat = Bj.Squeeze2dBijection((2, 4, 4), 2), Bj.ViewBijection((8, 2, 2), (32,))
    for chain in ([squeeze], [flat.__class__((2, 4, 4), (32,))], [elementwise[0], squeeze, elementwise[2], flat], [squeeze, flat]):
        head = to_head_space_weights(chain, w)
        back = to_data_space_weights(chain, head)
        assert back.shape == w.shape and torch.equal(back, w)
        assert torch.equal(to_head_space_weights(chain, back), head)
    # it is the bijection's own z_to_x reshaping of positions
    ids = torch.arange(32.0).view(1, 8, 2, 2)
    assert torch.equal(to_data_space_weights([squeeze], ids), squeeze._reshape_z(ids))
    with pytest.raises(NotImplementedError, match="weights cannot be carried"):
        to_data_space_weights([Bj.LULinearBijection(32)], w.reshape(3, 32))
