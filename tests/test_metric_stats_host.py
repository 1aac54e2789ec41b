"""Host side of the metric statistics (cmf_amd/metric_stats.py): finalisation of hand-built states against numpy, ``merge``,
``all_reduce`` over gloo at world size 2, and the argument errors.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_state(d, count, skipped=0, seed=0, diagonal=None):
    """A MetricState holding the sums of ``count`` random SPD matrices (or with a prescribed summed diagonal)."""
    from cmf_amd.metric_stats import MetricState
    rng = np.random.default_rng(seed)
    sg, sc = np.zeros((d, d)), np.zeros((d, d))
    for _ in range(count):
        a = rng.standard_normal((d + 3, d))
        g = a.T @ a
        n = np.sqrt(np.diag(g)) + 1e-8
        sg += g
        sc += g / np.outer(n, n)
    if diagonal is not None:
        sg[np.arange(d), np.arange(d)] = diagonal
    s = MetricState(d)
    s.flat.copy_(torch.from_numpy(np.concatenate((sg.ravel(), sc.ravel(), [count, skipped]))))
    return s, sg, sc


@pytest.mark.parametrize("d", [1, 2, 5])
def test_finalisation_matches_numpy(d):
    s, sg, sc = make_state(d, count=7, skipped=2, seed=d)
    r = s.result()
    assert r["count"] == 7 and r["skipped"] == 2 and isinstance(r["count"], int)
    mm, mc = sg / 7, sc / 7
    for key, want in (("mean_metric", mm), ("mean_diagonal", np.diag(mm)), ("mean_metric_normalized", mm / np.abs(mm).max()),
                      ("mean_diagonal_normalized", np.diag(mm) / np.abs(np.diag(mm)).max()), ("mean_cosine", mc)):
        assert r[key].dtype == torch.float64 and r[key].device.type == "cpu"
        np.testing.assert_allclose(r[key].numpy(), want, rtol=1e-15, atol=0)
    assert r["macs"] == pytest.approx(np.abs(mc).mean(), rel=1e-14)
    off = np.abs(mc)[~np.eye(d, dtype=bool)]
    assert r["macs_offdiag"] == pytest.approx(off.mean() if d > 1 else 0.0, rel=1e-14)
    assert r["ranking"].tolist() == np.argsort(np.abs(np.diag(mm)), kind="stable").tolist()


def test_ranking_is_stable_on_ties():
    s, _, _ = make_state(5, count=4, diagonal=[8.0, 2.0, 8.0, 2.0, 1.0])
    assert s.result()["ranking"].tolist() == [4, 1, 3, 0, 2]
    s.flat[0] = -8.0                                     # the ranking is by |mean g_kk| (visualizer.py:395)
    assert s.result()["ranking"].tolist() == [4, 1, 3, 0, 2]


def test_no_sample_raises():
    from cmf_amd.metric_stats import MetricState
    s = MetricState(3)
    with pytest.raises(ValueError):
        s.result()
    s.flat[-1] = 4                                       # only skipped samples
    with pytest.raises(ValueError):
        s.result()


def test_merge_is_additive_and_reset_clears():
    from cmf_amd.metric_stats import MetricState
    a, _, _ = make_state(4, count=3, skipped=1, seed=1)
    b, _, _ = make_state(4, count=5, skipped=0, seed=2)
    want = a.flat + b.flat
    assert a.merge(b) is a and torch.equal(a.flat, want)
    assert a.result()["count"] == 8 and a.result()["skipped"] == 1
    with pytest.raises(ValueError):
        a.merge(MetricState(3))
    a.reset()
    assert torch.equal(a.flat, torch.zeros_like(a.flat))


def _reduce_worker(rank, world, store, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    try:
        from test_metric_stats_host import make_state
        s, _, _ = make_state(5, count=3 + rank, skipped=rank, seed=10 + rank)
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
    merged, _, _ = make_state(5, count=3, skipped=0, seed=10)
    merged.merge(make_state(5, count=4, skipped=1, seed=11)[0])
    for _, flat in res:
        assert np.array_equal(flat, merged.flat.numpy())
    assert merged.result()["count"] == 7 and merged.result()["skipped"] == 1


def _density(dataset="sphere", **overrides):
    import cmf_amd
    cfg = cmf_amd.get_config(dataset, **overrides)
    x = torch.zeros(4, *cmf_amd.DATA_SHAPES[dataset])
    return cmf_amd.get_density(cmf_amd.get_schema(cfg), x), x


def test_argument_errors():
    import cmf_amd
    dens, x = _density()
    with pytest.raises(ValueError, match="coordinates"):
        cmf_amd.MetricStatistics(dens, coordinates="earliest")
    with pytest.raises(NotImplementedError, match="M-flow"):
        cmf_amd.MetricStatistics(_density(m_flow=True)[0])
    with pytest.raises(ValueError, match="non-square head"):
        cmf_amd.MetricStatistics(torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="prior layer"):
        cmf_amd.MetricStatistics(_density("power", prior="nsf")[0], coordinates="noise")
    for coordinates in ("latent", "noise"):
        stats = cmf_amd.MetricStatistics(dens, coordinates=coordinates)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            stats.update(x)
        assert torch.equal(stats.state.flat, torch.zeros(2 * stats.state.d ** 2 + 2, dtype=torch.float64))
