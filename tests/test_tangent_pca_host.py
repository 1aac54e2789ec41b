"""Host-side checks of the principal geodesic analysis (no GPU): the numpy emulation of csrc/tangent_pca.hip
(tests/_tangent_pca_emulation.py) against numpy float64 / longdouble on the same inputs at A QUARTER of the bounds the kernel is
held to (stated in that module), its ranks on designed inputs, its info codes and exact zeros, the float64 reference on the fixtures
-- the conditions tests/test_gpu_tangent_pca.py asserts of the product are established here on the reference alone -- and the
refusals of the engine wrapper and of the public API.

The bounds are the forms of DESIGN 4.3l.  One of them carries K: ``total`` stands behind two K-term sums and a division on top of
the length-d contraction, so its form is 2 (d + K + 4) u sum |terms| (as the centre gradient of the star kernels, tests/test_star_host.py); with
2 (d + 4) u this emulation reaches 0.40 at d = 2, K = 64, which sequential float64 sums may.  Reached by the emulation, the largest
over all shapes: eigenvalues 0.053, orthonormality 0.076, scores 0.043, covectors 0.146, norm2 0.233 (d = 2: 2.8 u of the worst
case 4 u against the form's 12 u), total 0.132, reconstruction 0.060."""
import numpy as np
import pytest
import torch

import _frechet_reference as FR
import _pga_reference as PR
import _tangent_pca_emulation as TE
from test_geodesic_host import small_density

QUARTER = 0.25


def merge(worst, got):
    for key, value in got.items():
        worst[key] = max(worst.get(key, 0.0), value)
    return worst


@pytest.mark.parametrize("d", TE.WIDTHS)
def test_emulation_meets_a_quarter_of_the_bounds(d):
    worst = {}
    for K in TE.ARMS:
        for B in (1, 3):
            G, V, w = TE.inputs(B, K, d)
            ref = TE.reference(G, V, w)
            out = TE.emulate(G, V, w)
            assert (out["info"] == 0).all() and TE.contract_holds(out, d, K, K), (d, K, B)
            merge(worst, TE.check(G, V, w, out, ref))
            one = TE.emulate(G, V, w, 1)
            assert TE.contract_holds(one, d, K, 1)
            assert TE.same_bits(one["variances"], out["variances"][:, :1]) and TE.same_bits(one["directions"], out["directions"][:, :1])
            assert TE.same_bits(one["scores"], out["scores"][:, :, :1]) and TE.same_bits(one["rank"], out["rank"])
            merge(worst, TE.check(G, V, w, one, ref))
    print(f"d={d}: reached fractions of the bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= QUARTER for v in worst.values()), worst


@pytest.mark.parametrize("d", TE.WIDTHS)
def test_emulation_finds_the_designed_rank(d):
    worst, zero = {}, 0.0
    for K in TE.ARMS:
        for r0 in TE.design_ranks(K, d):
            G, V, w, sigma = TE.designed(d, K, r0)
            ref = TE.reference(G, V, w)
            rel = np.abs(ref[0][0]) / ref[0][0, 0]
            assert ((rel >= 1e-3) | (rel <= 1e-10)).all(), (d, K, r0, rel)       # the design, from the reference alone
            zero = max(zero, float(rel[r0:].max()) if r0 < K else 0.0)
            out = TE.emulate(G, V, w)
            assert out["info"].tolist() == [0] and out["rank"].tolist() == [r0] and TE.contract_holds(out, d, K, K), (d, K, r0)
            merge(worst, TE.check(G, V, w, out, ref))                            # with the reconstruction where rank = K
    print(f"d={d}: largest structural zero {zero:.1e} lambda_1; reached fractions: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= QUARTER for v in worst.values()), worst


def test_emulation_info_codes_and_exact_zeros():
    B, K, d = 3, 5, 17
    G, V, w = TE.inputs(B, K, d)
    clean = TE.emulate(G, V, w)
    assert clean["info"].tolist() == [0, 0, 0]
    for where in ("G", "G_inf", "V", "w_nan", "w_zero", "w_negative", "w_inf"):
        Gn, Vn, wn = G.copy(), V.copy(), w.copy()
        if where == "G":
            Gn[1, 4, 2] = np.nan
        elif where == "G_inf":
            Gn[1, 3, 3] = np.inf
        elif where == "V":
            Vn[1, 2, 7] = np.nan
        else:
            wn[1, 3] = {"w_nan": np.nan, "w_zero": 0.0, "w_negative": -1.0, "w_inf": np.inf}[where]
        out = TE.emulate(Gn, Vn, wn)
        assert out["info"].tolist() == [0, 2, 0] and out["rank"][1] == 0 and out["sweeps"][1] == 0, where
        assert all(np.isnan(out[key][1]).all() for key in TE.KEYS), where
        assert all(TE.same_bits(out[key][[0, 2]], clean[key][[0, 2]]) for key in TE.KEYS + ("rank", "sweeps")), where
    Gn = G.copy()
    Gn[1, 2, 4] = np.nan                                             # the upper triangle is never read
    out = TE.emulate(Gn, V, w)
    assert all(TE.same_bits(out[key], clean[key]) for key in clean)
    # no spread at all: rank 0 and exact zeros; one vector: rank 1
    out = TE.emulate(G, np.zeros_like(V), w)
    assert out["info"].tolist() == [0, 0, 0] and out["rank"].tolist() == [0, 0, 0] and out["sweeps"].tolist() == [1, 1, 1]
    assert all(not out[key].any() for key in TE.KEYS)
    Vn = np.zeros_like(V)
    Vn[:, 2] = V[:, 2]
    out = TE.emulate(G, Vn, w)
    assert out["rank"].tolist() == [1, 1, 1] and TE.contract_holds(out, d, K, K)
    assert max(TE.check(G, Vn, w, out).values()) <= QUARTER


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_reference_meets_the_conditions_of_the_product(name):
    model, w, _, end = FR.reference_run(name)
    K, d = w.shape[1], end["mean_latent"].shape[1]
    ref = PR.analyse(model, end, w)
    assert bool((ref["rank"] <= min(K, d)).all()) and bool((ref["rank"] >= 1).all())
    assert bool(((ref["explained"].sum(1) - 1.0).abs() <= 4 * K * TE.U).all())           # trace M = total
    assert bool((ref["variances"][:, :-1] >= ref["variances"][:, 1:]).all())
    if d < K:
        assert bool((ref["variances"][:, d:].abs() <= 1e-12 * ref["variances"][:, :1]).all())
    # the end differences against the arm lengths: a discretisation gap, recorded, not asserted
    gap5 = (ref["norm2"].sqrt() / end["distances"] - 1.0).abs()
    nine = FR.mean(model, end["latents"][:, :, 0], w, points=9)
    ref9 = PR.analyse(model, nine, w)
    gap9 = (ref9["norm2"].sqrt() / nine["distances"] - 1.0).abs()
    print(f"{name}: rank {ref['rank'].tolist()} of min(K, d) = {min(K, d)}; explained {ref['explained'][0].tolist()}; "
          f"|sqrt(norm2) / distances - 1| max {float(gap5.max()):.3e} at P = 5, {float(gap9.max()):.3e} at P = 9")


def test_api_refusals():
    import cmf_amd
    from cmf_amd import engine as E
    dens = small_density()
    geo = cmf_amd.ManifoldGeodesic(dens, points=5)
    d = geo.head.program.d
    zs = torch.zeros(2, 3, d)
    most = min(3, d)
    # the refusals of mean / mean_latents, in their words
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.principal(torch.zeros(2, 3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.principal_latents(zs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.principal_latents(zs, components=most)
    for bad in (torch.zeros(2, 6), torch.zeros(0, 3, 6), torch.zeros(2, 0, 6)):
        with pytest.raises(ValueError, match="xs|at least one"):
            geo.principal(bad)
    for bad in (torch.zeros(2, d), torch.zeros(2, 3, d + 1), torch.zeros(2, 3, d, dtype=torch.float64)):
        with pytest.raises(ValueError, match="zs must be"):
            geo.principal_latents(bad)
    for bad in (torch.zeros(0, 3, d), torch.zeros(2, 0, d), torch.zeros(2, 65, d)):
        with pytest.raises(ValueError, match="at least one group"):
            geo.principal_latents(bad)
    with pytest.raises(ValueError, match="steps >= 0"):
        geo.principal_latents(zs, steps=-1)
    with pytest.raises(ValueError, match="weights must be a floating point tensor"):
        geo.principal_latents(zs, weights=torch.ones(2))
    with pytest.raises(ValueError, match="finite and > 0"):
        geo.principal_latents(zs, weights=torch.tensor([1.0, 0.0, 1.0]))
    # components
    for bad in (0, -1, most + 1, 1.0, "1", True):
        with pytest.raises(ValueError, match="components"):
            geo.principal_latents(zs, components=bad)
    with pytest.raises(ValueError, match=r"min\(K, d\) = 1"):
        geo.principal_latents(zs[:, :1], components=2)
    # principal_paths
    result = {"mean_latent": torch.zeros(2, d), "mean_head": torch.zeros(2, 6), "mean": torch.zeros(2, 6),
              "variances": torch.ones(2, 2, dtype=torch.float64), "directions": torch.zeros(2, 2, d, dtype=torch.float64)}
    with pytest.raises(ValueError, match="result must be"):
        geo.principal_paths({k: v for k, v in result.items() if k != "directions"})
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="component = "):
            geo.principal_paths(result, component=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="extent"):
            geo.principal_paths(result, extent=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.principal_paths(result)
    # the engine
    assert E.TANGENT_PCA_MAX_WIDTH == 128
    G, V, w = torch.zeros(2, 3, 3), torch.zeros(2, 4, 3, dtype=torch.float64), torch.ones(2, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        E.tangent_pca(G, V, w)
