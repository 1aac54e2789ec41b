"""Host side of the metric spectrum: the numpy emulation of csrc/gram_spectrum.hip (tests/_jacobi_emulation.py) against LAPACK on
the inputs of the GPU test, ``SpectrumState``, ``effective_rank`` and the constructor's refusals.  No GPU.

The emulation has to stay within a QUARTER of the bounds tests/test_gpu_metric_spectrum.py grants the kernel,
    |lambda - lambda_ref| <= C d 2^-53 max |lambda_ref|,   max |G V - V Lambda| <= C d 2^-53 max |lambda_ref|,
    max |V^T V - I| <= C d 2^-53,   C = 32
-- the form backward stability gives for Jacobi and LAPACK alike.  Measured here: the worst ratios to d 2^-53 are 2.5 (eigenvalues,
d = 3), 0.7 (residual, d = 2) and 7.1 (orthogonality, d = 128, the spectrum spread over 10^12), at most 20 sweeps."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jacobi_emulation as J                                       # noqa: E402

SWEEPS_FILE = os.path.join(ROOT, "tests", "golden", "jacobi_emulation_sweeps.json")


@pytest.mark.parametrize("B,d", J.SHAPES)
def test_emulation_meets_a_quarter_of_the_kernel_bounds(B, d):
    labels, G = J.cases(B, d)
    eig, vec, sweeps, info = J.emulated(B, d)
    e_val, e_res, e_orth = J.error_ratios(G.numpy(), eig, vec)
    print(f"B={B} d={d}: ratios to d 2^-53: eigenvalues {e_val.max():.2f}, residual {e_res.max():.2f}, orthogonality "
          f"{e_orth.max():.2f}; sweeps {dict(zip(labels, sweeps.tolist()))}")
    quarter = J.BOUND_C / 4
    assert (e_val <= quarter).all() and (e_res <= quarter).all() and (e_orth <= quarter).all()
    assert (info == 0).all() and (sweeps >= 1).all() and (sweeps <= J.MAX_SWEEPS).all()
    assert (np.diff(eig, axis=1) >= 0).all() and J.sign_rule_holds(vec)
    for name in ("identity", "repeated_diagonal", "zero"):
        assert sweeps[labels.index(name)] == 1
    assert np.array_equal(eig[labels.index("repeated_diagonal")], np.sort(np.diag(G[labels.index("repeated_diagonal")].numpy())))
    # the recorded sweep counts the GPU test prints beside the kernel's (regenerate the file from this test's output if an input changes)
    recorded = json.load(open(SWEEPS_FILE))
    assert recorded[f"{B}x{d}"] == sweeps.tolist()


def test_ordering_covers_every_pair_once_per_sweep():
    for d in (1, 2, 3, 10, 17, 64, 127, 128):
        seen = set()
        for s in range(J.steps(d)):
            p, q = J.pairs(d, s)
            assert len(p) == d // 2 and (p < q).all() and len(set(p) | set(q)) == 2 * len(p)          # disjoint within a step
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == d * (d - 1) // 2


def test_emulation_reads_the_lower_triangle_and_ties_keep_diagonal_order():
    G = J.cases(4, 10)[1][:2].numpy().copy()
    want = J.jacobi(G)
    G[:, np.triu_indices(10, 1)[0], np.triu_indices(10, 1)[1]] = np.nan
    got = J.jacobi(G)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    eig, vec, sweeps, _ = J.jacobi(np.diag([2.0, 1.0, 2.0, 1.0])[None])
    assert eig[0].tolist() == [1.0, 1.0, 2.0, 2.0] and sweeps[0] == 1
    assert np.array_equal(vec[0], np.eye(4)[:, [1, 3, 0, 2]])         # equal values in the order of their diagonal positions


# --------------------------------------------------------------------------------------------------
# SpectrumState
# --------------------------------------------------------------------------------------------------


def make_state(d, count, skipped=0, seed=0):
    """A SpectrumState holding the sums of ``count`` random positive spectra, and the spectra (count, d)."""
    from cmf_amd.metric_spectrum import SpectrumState
    rng = np.random.default_rng(seed)
    lam = np.sort(np.exp(rng.standard_normal((count, d)) * 3), axis=1)
    pr = lam.sum(1) ** 2 / (lam ** 2).sum(1)
    s = SpectrumState(d)
    s.flat.copy_(torch.from_numpy(np.concatenate((np.log(lam).sum(0), lam.sum(0), [pr.sum(), count, skipped]))))
    return s, lam


@pytest.mark.parametrize("d", [1, 2, 5])
def test_finalisation_matches_numpy(d):
    s, lam = make_state(d, count=7, skipped=2, seed=d)
    r = s.result()
    assert r["count"] == 7 and r["skipped"] == 2 and isinstance(r["count"], int)
    for key, want in (("mean_log_eigenvalues", np.log(lam).mean(0)), ("mean_eigenvalues", lam.mean(0))):
        assert r[key].dtype == torch.float64 and r[key].device.type == "cpu" and r[key].shape == (d,)
        np.testing.assert_allclose(r[key].numpy(), want, rtol=1e-14, atol=0)
    assert r["mean_participation_ratio"] == pytest.approx((lam.sum(1) ** 2 / (lam ** 2).sum(1)).mean(), rel=1e-14)
    assert r["mean_log_volume"] == pytest.approx(0.5 * np.log(lam).sum(1).mean(), rel=1e-13)


def test_update_arithmetic_on_cpu_tensors():
    """The masked reductions ``MetricSpectrum.update`` runs behind the kernel, on hand-made spectra: which samples count, and
    what each per-sample number is where it does not."""
    from cmf_amd.metric_spectrum import SpectrumState, accumulate, summarize
    nan, inf = float("nan"), float("inf")
    lam = torch.tensor([[1.0, 2.0, 4.0], [-1.0, 1.0, 2.0], [0.5, 0.5, 8.0], [nan, nan, nan], [0.0, 1.0, 1.0]], dtype=torch.float64)
    info = torch.tensor([0, 0, 1, 2, 0], dtype=torch.int32)
    out = summarize(lam, info)
    assert out["valid"].tolist() == [True, False, False, False, False]
    assert out["log_volume"][0] == pytest.approx(0.5 * np.log(8.0)) and bool(torch.isnan(out["log_volume"][1:]).all())
    assert out["condition"][:3].tolist() == [4.0, inf, 16.0] and bool(torch.isnan(out["condition"][3])) and out["condition"][4] == inf
    assert out["participation_ratio"][0] == pytest.approx(49.0 / 21.0)
    s = SpectrumState(3)
    accumulate(s.flat, out)
    accumulate(s.flat, out)
    r = s.result()
    assert r["count"] == 2 and r["skipped"] == 8
    assert r["mean_eigenvalues"].tolist() == [1.0, 2.0, 4.0]
    assert r["mean_log_volume"] == pytest.approx(0.5 * np.log(8.0))


def test_no_sample_raises():
    from cmf_amd.metric_spectrum import SpectrumState
    s = SpectrumState(3)
    with pytest.raises(ValueError):
        s.result()
    s.flat[-1] = 4                                       # only skipped samples
    with pytest.raises(ValueError):
        s.result()


def test_merge_is_additive_and_reset_clears():
    from cmf_amd.metric_spectrum import SpectrumState
    a, _ = make_state(4, count=3, skipped=1, seed=1)
    b, _ = make_state(4, count=5, skipped=0, seed=2)
    want = a.flat + b.flat
    assert a.merge(b) is a and torch.equal(a.flat, want)
    assert a.result()["count"] == 8 and a.result()["skipped"] == 1
    with pytest.raises(ValueError):
        a.merge(SpectrumState(3))
    a.reset()
    assert torch.equal(a.flat, torch.zeros(2 * 4 + 3, dtype=torch.float64))


def _reduce_worker(rank, world, store, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    try:
        from test_metric_spectrum_host import make_state
        s, _ = make_state(5, count=3 + rank, skipped=rank, seed=10 + rank)
        s.all_reduce()
        q.put((rank, s.flat.numpy().copy()))             # plain numpy through the queue (see test_distributed_gloo.py)
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_gloo_equals_merge(tmp_path):
    world, store = 2, str(tmp_path / "rendezvous")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, store, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    merged, _ = make_state(5, count=3, skipped=0, seed=10)
    merged.merge(make_state(5, count=4, skipped=1, seed=11)[0])
    for _, flat in res:
        assert np.array_equal(flat, merged.flat.numpy())
    assert merged.result()["count"] == 7 and merged.result()["skipped"] == 1


# --------------------------------------------------------------------------------------------------
# effective_rank, constructor
# --------------------------------------------------------------------------------------------------


def test_effective_rank():
    import cmf_amd
    lam = torch.tensor([[1e-9, 1e-3, 1.0, 10.0], [0.0, 0.0, 0.0, 0.0], [-1.0, 2.0, 2.0, 2.0], [float("nan")] * 4], dtype=torch.float64)
    assert cmf_amd.effective_rank(lam, 1e-6).tolist() == [3, 0, 3, 0]
    assert cmf_amd.effective_rank(lam, 0.5).tolist() == [1, 0, 3, 0]
    assert cmf_amd.effective_rank(lam[0], 1e-12).item() == 4 and cmf_amd.effective_rank(lam, 1e-6).dtype == torch.int64


def _density(dataset="sphere", **overrides):
    import cmf_amd
    cfg = cmf_amd.get_config(dataset, **overrides)
    x = torch.zeros(4, *cmf_amd.DATA_SHAPES[dataset])
    return cmf_amd.get_density(cmf_amd.get_schema(cfg), x), x


def test_argument_errors():
    import cmf_amd
    from cmf_amd import engine as E
    dens, x = _density()
    with pytest.raises(ValueError, match="coordinates"):
        cmf_amd.MetricSpectrum(dens, coordinates="earliest")
    with pytest.raises(NotImplementedError, match="M-flow"):
        cmf_amd.MetricSpectrum(_density(m_flow=True)[0])
    with pytest.raises(ValueError, match="non-square head"):
        cmf_amd.MetricSpectrum(torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="prior layer"):
        cmf_amd.MetricSpectrum(_density("power", prior="nsf")[0], coordinates="noise")
    assert E.SPECTRUM_MAX_WIDTH == 128
    with pytest.raises(ValueError, match="1 <= latent_dimension <= 128"):
        cmf_amd.MetricSpectrum(_density("mnist", latent_dimension=130)[0])
    cmf_amd.MetricStatistics(_density("mnist", latent_dimension=130)[0])     # the statistics take the wide head as before
    for coordinates in ("latent", "noise"):
        spec = cmf_amd.MetricSpectrum(dens, coordinates=coordinates, vectors=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            spec.update(x)
        assert torch.equal(spec.state.flat, torch.zeros(2 * spec.state.d + 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="GPU"):
        E.gram_spectrum(torch.zeros(2, 3, 3))
