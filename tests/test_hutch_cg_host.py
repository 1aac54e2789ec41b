"""The float64 model of the Hutchinson CG kernels (tests/_hutch_cg_reference.py) checked on the CPU: its three conditions on the
whole case list, the model itself against numpy's solve and against ``oracle.cmf_oracle.cg_documented``, the default ``min_iter``
of ``engine.hutch_cg``, and the variant spread the GPU bound's margin rests on."""
import numpy as np
import pytest
import torch

import _hutch_cg_reference as R


@pytest.mark.parametrize("name", list(R.cases()))
def test_conditions_hold(name):
    """Conditions 1 - 3 on every work item (``emulated`` raises otherwise), and what the case promises about its stops."""
    c, ems = R.cases()[name], R.emulated(name)
    iters = [em.ref.iters for em in ems]
    if "iters" in c.expect:
        assert iters == c.expect["iters"]
    if name.startswith("default_"):
        assert iters == [11, 11] and all(s == 11 for em in ems for s in em.ref.stops)         # the production rule: the 11th iterate
    if name.startswith("mixed_a"):                                     # a max rule or a per-probe rule would go on to >= 5
        assert all(em.ref.history[0][1] < c.tol / 2 and em.ref.history[0][0] > 2 * c.tol for em in ems)
    if name.startswith("mixed_b"):                                     # chunk 0 holds 2-step iterates, chunk 1 its own count
        assert all(em.ref.stops[0] == 2 and em.ref.stops[1] >= 4 and em.ref.iters == em.ref.stops[1] for em in ems)
    if name.startswith("mixed_c"):                                     # per sample, no batch-wide mean
        assert iters[0] == 2 and iters[2] == 2 and iters[1] >= 4
    if name.startswith("mixed_d") or name.startswith("zero_probe"):
        assert all(not em.ref.u[:, ~c.eps[b].any(0)].any() for b, em in enumerate(ems))
    if name == "zero_matrix":
        assert all(not em.ref.u.any() and not em.ref.w.any() for em in ems)


def _case(d, S, hi, tol, seed=1):
    rng = np.random.default_rng(seed)
    G = R._spd(R._orthogonal(d, rng), np.geomspace(1.0, hi, d))
    return R.Case("probe", np.stack([G, G]), R._f32(rng.standard_normal((2, d, S))), d, tol, R.default_min_iter(d), {})


def test_conditions_trip_on_inputs_that_decide_nothing():
    """tol = 1 on the [1, 1e3] spectrum leaves the mean residual within a few percent of tol where the rule inspects it
    (condition 1); [1, 100] at d = 12 leaves the 11th float32 iterate 1e-2 away from the float64 one (condition 3)."""
    with pytest.raises(AssertionError, match="condition 1"):
        R._emulate(_case(128, 16, 1e3, 1.0))
    with pytest.raises(AssertionError, match="condition 3"):
        R._emulate(_case(12, 16, 100.0, 1.0))


@pytest.mark.parametrize("name", ["default_d12_S16", "default_d65_S5", "default_d128_S17", "cluster_d64_S16_m6_tol", "mixed_b_d100"])
def test_converged_model_is_the_solve(name):
    c = R.cases()[name]
    G, eps = c.G[0].astype(np.float64), c.eps[0].astype(np.float64)
    ref = R.reference(G, eps, 4 * G.shape[0], 1e-13, 1, order="pair")
    want = np.linalg.solve(G, eps)
    assert (np.abs(ref.u - want).max(0) <= 1e-10 * np.abs(want).max(0)).all()
    assert (np.abs(ref.w - G @ eps).max() <= 1e-13 * np.abs(G @ eps).max())


@pytest.mark.parametrize("name", [n for n, c in R.cases().items() if c.eps.shape[2] <= R.CHUNK and c.eps.any(1).all() and c.G.any()])
def test_model_is_cg_documented_within_one_chunk(name):
    """For S <= 16 a sample is one work item and the model is ``cg_documented`` (which divides by the probe norm and by p^T q
    unguarded: zero probes and the zero matrix are left to the model)."""
    from oracle import cmf_oracle as O
    c, ems = R.cases()[name], R.emulated(name)
    u, iters = O.cg_documented(torch.from_numpy(c.G).double(), torch.from_numpy(c.eps).double(), c.max_iter, c.tol, c.min_iter)
    assert iters.tolist() == [em.ref.iters for em in ems]
    for b, em in enumerate(ems):
        assert (np.abs(u[b].numpy() - em.ref.u).max(0) <= 1e-12 * np.abs(em.ref.u).max(0)).all()


@pytest.mark.parametrize("d", R.MIXED_D)
def test_chunk_rule_differs_from_cg_documented_beyond_one_chunk(d):
    """S = 32 (mixed case b): ``cg_documented`` takes the mean over all 32 probes of the sample and runs chunk 0's probes on past
    their work item's stop at 2 -- the difference is the chunk rule."""
    from oracle import cmf_oracle as O
    c, ems = R.cases()[f"mixed_b_d{d}"], R.emulated(f"mixed_b_d{d}")
    u, iters = O.cg_documented(torch.from_numpy(c.G).double(), torch.from_numpy(c.eps).double(), c.max_iter, c.tol, c.min_iter)
    for b, em in enumerate(ems):
        assert em.ref.stops[0] == 2 < int(iters[b])
        diff = np.abs(u[b].numpy() - em.ref.u).max(0) / np.abs(em.ref.u).max(0)
        assert diff[R.SLOW_SLOT] > 1e-2                                # the slow probe of chunk 0 holds its 2-step iterate


def test_engine_default_min_iter(monkeypatch):
    """``engine.hutch_cg(min_iter=None)`` passes ``default_min_iter(max_iter)`` to the launch, max_iter = 1 .. 600 (a recorded
    launch on CPU tensors: no kernel runs)."""
    from cmf_amd import engine as E
    seen = []

    class Recorder:
        def cmf_hutch_cg(self, jtj, eps, d, S, B, max_iter, min_iter, *rest):
            seen.append((max_iter, min_iter))
            return 0

    monkeypatch.setattr(E._lib, "load", lambda: Recorder())
    monkeypatch.setattr(E, "_stream", lambda: None)
    jtj, eps = torch.zeros(1, 2, 2), torch.zeros(1, 2, 1)
    for max_iter in range(1, 601):
        E.hutch_cg(jtj, eps, max_iter, 1.0)
    assert seen == [(k, R.default_min_iter(k)) for k in range(1, 601)]
    assert R.default_min_iter(1) == 1 and R.default_min_iter(5) == 5 and R.default_min_iter(11) == 11 and R.default_min_iter(512) == 11


def test_margin_is_the_recorded_variant_spread():
    """The widest ratio between two summation orders' rho on one work item of the list is the number recorded in the helper, and
    the margin of the GPU bound is that number rounded up, at least 2 and at most 4."""
    spread = {n: max([s for em in R.emulated(n) for s in em.spread if s is not None], default=0.0) for n in R.cases()}
    worst = max(spread, key=spread.get)
    rho = [r for n in R.cases() for em in R.emulated(n) for r in em.rho]
    print(f"variant spread: widest {spread[worst]:.2f} ({worst}); rho_item {min(r for r in rho if r > 0):.1e} .. {max(rho):.1e}")
    assert abs(spread[worst] - R.VARIANT_SPREAD_MEASURED) <= 0.05 * R.VARIANT_SPREAD_MEASURED
    assert R.MARGIN == min(4, max(2, int(np.ceil(spread[worst])))) and 2 <= R.MARGIN <= 4
