"""Principal geodesic analysis on the GPU: the kernel (csrc/tangent_pca.hip) against numpy float64 / longdouble on the
same inputs within the bounds stated in tests/_tangent_pca_emulation.py (the emulation is held to a quarter of them by
tests/test_tangent_pca_host.py), its ranks on designed inputs, its output contract, isolation, determinism and refusals, and
``cmf_amd.ManifoldGeodesic.principal`` / ``principal_paths`` end to end on the reference-generated fixtures under the conditions the
host test establishes on the float64 reference.  Needs an MI355X: run with ``-m gpu``.

The bounds are the forms of DESIGN 4.3l, ``total`` at 2 (d + K + 4) u sum |terms| (derived in tests/_tangent_pca_emulation.py)."""
import numpy as np
import pytest
import torch

import _frechet_reference as FR
import _pga_reference as PR
import _tangent_pca_emulation as TE
from conftest import kink_tolerance
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits
from test_tangent_pca_host import merge

pytestmark = pytest.mark.gpu

NAN = float("nan")
ALL = TE.KEYS + ("rank", "sweeps", "info")
F64, I32 = torch.float64, torch.int32


def run(G, V, w, r=None):
    """``engine.tangent_pca`` on CPU inputs -> a dict of numpy arrays (the TangentPcaResult's fields)."""
    from cmf_amd import engine as E
    res = E.tangent_pca(torch.as_tensor(G).cuda(), torch.as_tensor(V).cuda(), torch.as_tensor(w).cuda(), r)
    torch.cuda.synchronize()
    return {key: getattr(res, key).cpu().numpy() for key in ALL}


def fractions(worst):
    return ", ".join(f"{k} {v:.3f}" for k, v in worst.items())


@pytest.mark.parametrize("d", TE.WIDTHS)
def test_tangent_pca_matches_float64(d):
    worst = {}
    for K in TE.ARMS:
        for B in (1, 3):
            G, V, w = TE.inputs(B, K, d)
            ref = TE.reference_inputs(B, K, d)
            out = run(G, V, w)
            assert (out["info"] == 0).all() and TE.contract_holds(out, d, K, K), (K, B)
            merge(worst, TE.check(G, V, w, out, ref))
            one = run(G, V, w, 1)
            assert TE.contract_holds(one, d, K, 1), (K, B)
            assert same_bits(one["variances"], out["variances"][:, :1]) and same_bits(one["directions"], out["directions"][:, :1])
            assert same_bits(one["scores"], out["scores"][:, :, :1])
            assert all(same_bits(one[key], out[key]) for key in ("covectors", "norm2", "total", "rank", "sweeps", "info"))
    print(f"d={d}: reached fractions of the bounds: {fractions(worst)}")
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("d", TE.WIDTHS)
def test_designed_inputs_have_the_designed_rank(d):
    worst = {}
    for K in TE.ARMS:
        for r0 in TE.design_ranks(K, d):
            G, V, w, sigma = TE.designed(d, K, r0)
            ref = TE.reference(G, V, w)
            rel = np.abs(ref[0][0]) / ref[0][0, 0]
            assert ((rel >= 1e-3) | (rel <= 1e-10)).all(), (K, r0, rel)          # the design, from the reference alone
            out = run(G, V, w)
            assert out["info"].tolist() == [0] and out["rank"].tolist() == [r0], (K, r0, out["rank"], out["variances"])
            assert TE.contract_holds(out, d, K, K), (K, r0)                      # exact zeros beyond the rank among it
            assert not out["directions"][0, r0:].any() and not out["scores"][0, :, r0:].any()
            merge(worst, TE.check(G, V, w, out, ref))                            # with the reconstruction where rank = K
    print(f"d={d}: designed ranks: reached fractions of the bounds: {fractions(worst)}")
    assert all(v <= 1.0 for v in worst.values()), worst


def test_kernel_against_the_emulation():
    """Not asserted by bits (the project pins the Jacobi kernel to its emulation through the bounds, not the bits): printed."""
    for B, K, d in ((3, 5, 17), (3, 3, 2), (1, 17, 16)):
        G, V, w = TE.inputs(B, K, d) if K in TE.ARMS else (TE.gram(B, d), TE.vectors(B, K, d), TE.weights(B, K))
        out, emu = run(G, V, w), TE.emulate(G, V, w)
        print(f"B={B} K={K} d={d}: bit-equal to the emulation: " + ", ".join(f"{key} {same_bits(out[key], emu[key])}" for key in ALL))
        assert same_bits(out["rank"], emu["rank"]) and same_bits(out["info"], emu["info"])
        assert max(TE.check(G, V, w, out).values()) <= 1.0


def test_failures_are_reported_and_confined():
    B, K, d = 3, 5, 17
    G, V, w = TE.inputs(B, K, d)
    clean = run(G, V, w)
    assert clean["info"].tolist() == [0, 0, 0]
    for where in ("G", "G_inf", "V", "V_inf", "w_nan", "w_zero", "w_negative", "w_inf"):
        Gn, Vn, wn = G.copy(), V.copy(), w.copy()
        if where == "G":
            Gn[1, 4, 2] = NAN
        elif where == "G_inf":
            Gn[1, 3, 3] = np.inf
        elif where == "V":
            Vn[1, 2, 7] = NAN
        elif where == "V_inf":
            Vn[1, 4, 16] = -np.inf
        else:
            wn[1, 3] = {"w_nan": NAN, "w_zero": 0.0, "w_negative": -1.0, "w_inf": np.inf}[where]
        out = run(Gn, Vn, wn)
        assert out["info"].tolist() == [0, 2, 0] and out["rank"][1] == 0 and out["sweeps"][1] == 0, where
        assert all(np.isnan(out[key][1]).all() for key in TE.KEYS), where
        assert all(same_bits(out[key][[0, 2]], clean[key][[0, 2]]) for key in ALL), where
    Gn = G.copy()
    Gn[1, 2, 4] = NAN                                                # the upper triangle is never read
    out = run(Gn, V, w)
    assert all(same_bits(out[key], clean[key]) for key in ALL)
    # no spread: rank 0 and exact zeros
    out = run(G, np.zeros_like(V), w)
    assert out["info"].tolist() == [0, 0, 0] and out["rank"].tolist() == [0, 0, 0] and out["sweeps"].tolist() == [1, 1, 1]
    assert all(not out[key].any() for key in TE.KEYS)


@pytest.mark.parametrize("K,d", [(5, 17), (64, 16), (3, 128), (63, 65)])
def test_position_independence_and_repeatability(K, d):
    G, V, w = TE.gram(3, d, seed=3), TE.vectors(3, K, d, seed=3), TE.weights(3, K)
    order = [0, 1, 2, 2, 0, 1, 1]
    base = run(G, V, w)
    batch, again = run(G[order], V[order], w[order]), run(G[order], V[order], w[order])
    for key in ALL:
        assert same_bits(base[key][order], batch[key]) and same_bits(batch[key], again[key]), key
    for b in range(3):                                               # a group alone: B = 1
        alone = run(G[b:b + 1], V[b:b + 1], w[b:b + 1])
        for key in ALL:
            assert same_bits(base[key][b:b + 1], alone[key]), key


def buffers(B, K, d, r):
    return {"variances": guarded((B, r), F64), "directions": guarded((B, r, d), F64), "scores": guarded((B, K, r), F64),
            "covectors": guarded((B, K, d), F64), "norm2": guarded((B, K), F64), "total": guarded((B,), F64),
            "rank": guarded((B,), I32), "sweeps": guarded((B,), I32), "info": guarded((B,), I32)}


@pytest.mark.parametrize("K,d,r", [(5, 17, 5), (5, 17, 2), (64, 128, 64), (3, 65, 1), (63, 2, 63), (1, 1, 1)])
def test_outputs_stay_inside_their_buffers(K, d, r):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    B = 2
    G, V, w = TE.gram(B, d, seed=2), TE.vectors(B, K, d, seed=2), TE.weights(B, K)
    Gc, Vc, wc = torch.as_tensor(G).cuda(), torch.as_tensor(V).cuda(), torch.as_tensor(w).cuda()
    bufs = buffers(B, K, d, r)
    _lib.check(_lib.load().cmf_tangent_pca(E._p(Gc), E._p(Vc), E._p(wc), d, K, r, B, *(E._p(bufs[key][1]) for key in ALL), E._stream()),
               "cmf_tangent_pca")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    out = run(G, V, w, r)
    for key in ALL:
        assert same_bits(bufs[key][1].cpu().numpy(), out[key]), key
    # a group with a non-finite input fills its own slices and nothing else
    Vc[1, 0, 0] = NAN
    bufs = buffers(B, K, d, r)
    _lib.check(_lib.load().cmf_tangent_pca(E._p(Gc), E._p(Vc), E._p(wc), d, K, r, B, *(E._p(bufs[key][1]) for key in ALL), E._stream()),
               "cmf_tangent_pca")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    assert bufs["info"][1].tolist() == [0, 2]
    assert all(same_bits(bufs[key][1][0].cpu().numpy(), out[key][0]) for key in ALL)
    assert all(bool(torch.isnan(bufs[key][1][1]).all()) for key in TE.KEYS)


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, K, d, r = 2, 4, 3, 2
    Gc, Vc, wc = (torch.as_tensor(t).cuda() for t in (TE.gram(B, d), TE.vectors(B, K, d), TE.weights(B, K)))
    z64 = lambda n: torch.zeros(n, dtype=F64, device="cuda")
    outs = [z64(B * r + 1), z64(B * r * d), z64(B * K * r), z64(B * K * d), z64(B * K), z64(B)]
    ints = [torch.zeros(B, dtype=I32, device="cuda") for _ in range(3)]
    odd = E._p(outs[0].view(torch.float32)[1:])                     # 4 bytes past an 8-byte boundary
    ok = [E._p(Gc), E._p(Vc), E._p(wc), d, K, r, B] + [E._p(t) for t in outs + ints]
    assert lib.cmf_tangent_pca(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) > 0 for t in outs) and ints[2].tolist() == [0, 0] and min(ints[1].tolist()) >= 1
    for t in outs + ints:
        t.zero_()
    bad = [(3, 0), (3, 129), (3, -1), (4, 0), (4, 65), (5, 0), (5, K + 1), (6, 0), (6, -1)]
    bad += [(i, None) for i in (0, 1, 2) + tuple(range(7, 16))] + [(i, odd) for i in (1, 2, 7, 8, 9, 10, 11, 12)]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_tangent_pca(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in outs + ints)


def test_engine_refusals_and_empties():
    from cmf_amd import engine as E
    B, K, d = 2, 4, 3
    G, V, w = (torch.as_tensor(t).cuda() for t in (TE.gram(B, d), TE.vectors(B, K, d), TE.weights(B, K)))
    with pytest.raises(ValueError, match="contiguous"):
        E.tangent_pca(G.transpose(1, 2), V, w)
    with pytest.raises(ValueError, match="float32"):
        E.tangent_pca(G.double(), V, w)
    with pytest.raises(ValueError, match="jtj must be"):
        E.tangent_pca(G[:, :, :2].contiguous(), V, w)
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.tangent_pca(torch.zeros(1, 129, 129, device="cuda"), torch.zeros(1, 2, 129, dtype=F64, device="cuda"), w[:1, :2].contiguous())
    with pytest.raises(ValueError, match="float64"):
        E.tangent_pca(G, V.float(), w)
    for bad in (V[:1], V[:, :, :2].contiguous(), V[:, 0], V.transpose(1, 2).contiguous().transpose(1, 2)):
        with pytest.raises(ValueError, match="vectors must be"):
            E.tangent_pca(G, bad, w)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        E.tangent_pca(G, torch.zeros(B, 65, d, dtype=F64, device="cuda"), torch.ones(B, 65, dtype=F64, device="cuda"))
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        E.tangent_pca(G, V[:, :0], w[:, :0])
    with pytest.raises(ValueError, match="float64"):
        E.tangent_pca(G, V, w.float())
    for bad in (w[:, :3].contiguous(), w[:1], w.t().contiguous().t()):
        with pytest.raises(ValueError, match="weights must be"):
            E.tangent_pca(G, V, bad)
    for bad in (0, K + 1, -1):
        with pytest.raises(ValueError, match="components"):
            E.tangent_pca(G, V, w, bad)
    for cpu in ((G.cpu(), V, w), (G, V.cpu(), w), (G, V, w.cpu())):
        with pytest.raises(ValueError, match="GPU"):
            E.tangent_pca(*cpu)
    # no group: empties, no launch
    with E.timing(lambda name: True) as timer:
        r = E.tangent_pca(G[:0], V[:0], w[:0], 2)
    assert timer.by_name() == {}
    assert r.variances.shape == (0, 2) and r.directions.shape == (0, 2, d) and r.scores.shape == (0, K, 2)
    assert r.covectors.shape == (0, K, d) and r.norm2.shape == (0, K) and r.total.shape == (0,)
    assert r.rank.shape == r.sweeps.shape == r.info.shape == (0,) and r.rank.dtype == I32


def test_kernel_timer_entry():
    from cmf_amd import engine as E
    G, V, w = (torch.as_tensor(t).cuda() for t in TE.inputs(3, 5, 17))
    with E.timing(lambda name: True) as timer:
        E.tangent_pca(G, V, w)
    by = timer.by_name()
    assert set(by) == {"tangent_pca"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------
MEAN_KEYS = ("mean_latent", "mean_head", "mean", "latents", "path_head", "path", "distances", "initial_distances", "segment_lengths",
             "energy", "initial_energy", "variance", "gradient", "gradient_centre", "gradient_max", "accepted", "damping", "info")


def run_principal(dens, head, xs, weights, steps, components=None, points=FR.POINTS):
    """One ``principal`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    geo = cmf_amd.ManifoldGeodesic(dens, points=points, steps=steps)
    keep, marker = xs.clone(), object()
    head.last_gram = marker
    out = geo.principal(xs, weights, components)
    assert head.last_gram is marker and torch.equal(xs, keep)
    B, K, d = xs.shape[0], xs.shape[1], head.program.d
    r = min(K, d) if components is None else components
    assert set(MEAN_KEYS) < set(out) and all(v.is_cuda for v in out.values())
    assert out["log_velocities"].shape == (B, K, d) and out["log_velocities"].dtype == F64
    assert out["metric"].shape == (B, d, d) and out["metric"].dtype == torch.float32
    for key, shape in (("variances", (B, r)), ("directions", (B, r, d)), ("scores", (B, K, r)), ("covectors", (B, K, d)),
                       ("norm2", (B, K)), ("total_variance", (B,)), ("explained", (B, r))):
        assert out[key].shape == shape and out[key].dtype == F64, key
    for key in ("rank", "pga_info"):
        assert out[key].shape == (B,) and out[key].dtype == I32, key
    return geo, out


def as_kernel_output(out):
    """The product's values under the kernel's names, as numpy."""
    names = {"variances": "variances", "directions": "directions", "scores": "scores", "covectors": "covectors", "norm2": "norm2",
             "total": "total_variance", "rank": "rank", "info": "pga_info"}
    return {key: out[name].cpu().numpy() for key, name in names.items()}


def star_weights(B):
    return torch.tensor(FR.WEIGHTS, dtype=F64).expand(B, len(FR.WEIGHTS)).contiguous()


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_principal_on_the_fixtures(name):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    xs = FR.star_inputs(x, name).contiguous()
    weights = torch.tensor(FR.WEIGHTS, dtype=F64, device="cuda")
    B, K, d, N = xs.shape[0], xs.shape[1], head.program.d, FR.POINTS - 1
    geo, out = run_principal(dens, head, xs, weights, FR.STEPS)
    r = min(K, d)
    # the mean, unchanged
    mean = geo.mean(xs, weights)
    assert set(mean) == set(MEAN_KEYS) and all(torch.equal(out[key], mean[key]) for key in MEAN_KEYS)
    # the log vectors: the difference formula on the returned latents, by bits
    assert torch.equal(out["log_velocities"], PR.log_vectors(out["latents"]))
    # the metric: the bits of one Gram attempt on a fresh decode at the mean
    with torch.no_grad(), E.scope(head.kernels):
        fresh = E.gram_cholesky(head.program.decode(out["mean_latent"], tangents=True)[1], d, 1).jtj
    assert torch.equal(out["metric"], fresh)
    # the kernel bounds on the product's own metric, log vectors and weights
    assert bool((out["pga_info"] == 0).all()) and bool((out["info"] == 0).all())
    G32, V, w = out["metric"].cpu().numpy(), out["log_velocities"].cpu().numpy(), star_weights(B).numpy()
    got = as_kernel_output(out)
    worst = TE.check(G32, V, w, got)
    lam = got["variances"]
    assert (lam[:, :-1] >= lam[:, 1:]).all() and (got["rank"] <= min(K, d)).all() and (got["rank"] >= 1).all()
    for b in range(B):
        assert not got["directions"][b, got["rank"][b]:].any() and not got["scores"][b][:, got["rank"][b]:].any()
    # explained: variances / total, summing to 1 over r = min(K, d)
    total = out["total_variance"]
    assert torch.equal(out["explained"], out["variances"] / total[:, None])
    one = float((out["explained"].sum(1) - 1.0).abs().max())
    # against the float64 reference at the GPU's own mean
    model = PR.Model(name)
    tol = kink_tolerance(g)
    G_ref = PR.metric(model, out["mean_latent"].cpu())
    g_max = G_ref.abs().flatten(1).max(1).values
    m_err = (out["metric"].cpu().double() - G_ref).abs().flatten(1).max(1).values
    Vt, wt = out["log_velocities"].cpu(), star_weights(B)
    lam_ref = PR.dual(G_ref, Vt, wt)[1][:, :r]
    allowed = tol * g_max * (wt * Vt.abs().sum(2) ** 2).sum(1) / wt.sum(1)
    l_err = (out["variances"].cpu() - lam_ref).abs().max(1).values
    gap = float((out["norm2"].sqrt() / out["distances"] - 1.0).abs().max())
    print(f"{name}: rank {got['rank'].tolist()} of min(K, d) = {r}; kernel bounds reached: {fractions(worst)}; |sum explained - 1| "
          f"{one:.2e} (allowed {4 * K * TE.U:.2e}); metric err / allowed {float((m_err / (tol * g_max)).max()):.3e}; variance err / "
          f"allowed {float((l_err / allowed).max()):.3e}; explained {out['explained'][0].tolist()}; |sqrt(norm2) / distances - 1| max "
          f"{gap:.3e}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert one <= 4 * K * TE.U
    assert bool((m_err <= tol * g_max).all())
    assert bool((l_err <= allowed).all())
    # fewer components: the leading columns, by bits
    _, first = run_principal(dens, head, xs, weights, FR.STEPS, components=1)
    assert torch.equal(first["variances"], out["variances"][:, :1]) and torch.equal(first["directions"], out["directions"][:, :1])
    assert torch.equal(first["scores"], out["scores"][:, :, :1]) and torch.equal(first["rank"], out["rank"])


def test_copies_of_one_input_have_rank_zero():
    g, meta, dens, head, x = build("c2a_power")
    xs = x[:3, None].expand(3, 3, *x.shape[1:]).contiguous()
    weights = torch.tensor(FR.WEIGHTS, dtype=F64, device="cuda")
    for steps in (0, 3):
        _, out = run_principal(dens, head, xs, weights, steps)
        assert bool((out["pga_info"] == 0).all()) and bool((out["rank"] == 0).all())
        for key in ("log_velocities", "variances", "directions", "scores", "covectors", "norm2", "total_variance", "explained"):
            assert bool((out[key] == 0).all()), key


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_groups_of_one_call(name, monkeypatch):
    """Nine groups of two inputs at three points per arm, under a budget of one star per sub-batch of ``mean`` and less than the
    nine centres per sub-batch of the metric sweep."""
    import cmf_amd
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    K, P, steps = 2, 3, 2
    pairs = [(i, j) for i in range(3) for j in range(3)]
    xs = torch.stack([x[[i for i, _ in pairs]], x[[j for _, j in pairs]]], 1).contiguous()
    B = len(pairs)
    weights = torch.tensor([1.0, 2.0], dtype=F64, device="cuda")
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", K * P * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(B * K * P) // (K * P) == 1 and prog.tangent_chunk(B) < B
    geo, out = run_principal(dens, head, xs, weights, steps, points=P)
    mean = geo.mean(xs, weights)
    assert all(torch.equal(out[key], mean[key]) for key in MEAN_KEYS)
    assert bool((out["pga_info"] == 0).all())
    with torch.no_grad(), E.scope(head.kernels):
        alone = torch.cat([E.gram_cholesky(prog.decode(out["mean_latent"][b:b + 1], tangents=True)[1], prog.d, 1).jtj for b in range(B)])
    assert torch.equal(alone, out["metric"])                         # the sub-batched sweep: one decode per centre, by bits
    # the analysis of every group is that of one launch over the nine
    w = weights.expand(B, K).contiguous()
    direct = E.tangent_pca(out["metric"], out["log_velocities"], w, min(K, prog.d))
    for key, name_ in (("variances", "variances"), ("directions", "directions"), ("scores", "scores"), ("covectors", "covectors"),
                       ("norm2", "norm2"), ("total", "total_variance"), ("rank", "rank"), ("info", "pga_info")):
        assert torch.equal(getattr(direct, key), out[name_]), key
    worst = TE.check(out["metric"].cpu().numpy(), out["log_velocities"].cpu().numpy(), w.cpu().numpy(), as_kernel_output(out))
    assert all(v <= 1.0 for v in worst.values()), worst
    same = [b for b, (i, j) in enumerate(pairs) if i == j]
    assert bool((out["rank"][same] == 0).all()) and bool((out["variances"][same] == 0).all())
    assert bool((out["rank"][[b for b in range(B) if b not in same]] >= 1).all())


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_principal_paths(name):
    g, meta, dens, head, x = build(name)
    star = FR.star_inputs(x, name)[:2]
    xs = torch.cat([star, x[:1, None].expand(1, FR.ARMS, *x.shape[1:])]).contiguous()          # the last group: copies of one input
    weights = torch.tensor(FR.WEIGHTS, dtype=F64, device="cuda")
    B, d, S, extent = xs.shape[0], head.program.d, 2, 2.0
    geo, res = run_principal(dens, head, xs, weights, 4)
    assert res["rank"].tolist()[-1] == 0 and min(res["rank"].tolist()[:-1]) >= 1
    tol = kink_tolerance(g)
    for j in (0, min(FR.ARMS, d) - 1):
        out = geo.principal_paths(res, component=j, extent=extent, steps=S)
        assert out["path"].shape == (B, 2 * S + 1, *xs.shape[2:]) and out["path_head"].shape == (B, 2 * S + 1, *head.x_shape)
        assert out["latents"].shape == (B, 2 * S + 1, d) and out["latents"].dtype == torch.float32
        assert out["speed2"].shape == (B, 2, S + 1) and out["speed2"].dtype == F64
        assert out["info"].shape == (B, 2) and out["info"].dtype == I32 and bool((out["info"] == 0).all())
        assert torch.equal(out["path_head"][:, S], res["mean_head"]) and torch.equal(out["path"][:, S], res["mean"])
        assert torch.equal(out["latents"][:, S], res["mean_latent"])
        # the speed at the mean: extent^2 lambda_j, the two G's from different decode paths
        lam = res["variances"][:, j]
        v0 = (extent * lam.clamp_min(0).sqrt())[:, None] * res["directions"][:, j]
        want = extent ** 2 * torch.where(res["rank"] > j, lam, torch.zeros_like(lam))
        allowed = 2 * d * tol * res["metric"].abs().flatten(1).max(1).values.double() * v0.abs().sum(1) ** 2
        err = (out["speed2"][:, :, 0] - want[:, None]).abs().max(1).values
        live = want > 0
        print(f"{name} component {j}: speed2 at the mean {out['speed2'][:, :, 0].tolist()} against extent^2 lambda_j {want.tolist()}: err / "
              f"allowed {float((err[live] / allowed[live]).max()) if bool(live.any()) else 0.0:.3e}; speed2 along the halves "
              f"{out['speed2'][0].tolist()}")
        assert bool((err <= allowed).all())
        # rank <= component: zero velocity, the group stays at the mean
        still = res["rank"] <= j
        assert bool(still[-1])
        assert bool((out["latents"][still] == res["mean_latent"][still][:, None]).all()) and bool((out["speed2"][still] == 0).all())
        moved = (out["path_head"][still] - res["mean_head"][still][:, None]).abs().flatten(1).max(1).values
        assert bool((moved <= 1e-5 * res["mean_head"][still].abs().flatten(1).max(1).values).all())
        # the two halves leave the mean in opposite latent directions
        lead = out["latents"][~still].double()
        assert bool((((lead[:, S + 1] - lead[:, S]) * (lead[:, S - 1] - lead[:, S])).sum(1) < 0).all())
    with pytest.raises(ValueError, match="component = "):
        geo.principal_paths(res, component=min(FR.ARMS, d))


def test_api_refusals_on_the_gpu():
    import cmf_amd
    g, meta, dens, head, x = build("c2a_power")
    geo = cmf_amd.ManifoldGeodesic(dens, points=4, steps=1)
    xs = x[:6].view(2, 3, *x.shape[1:]).contiguous()
    d = head.program.d
    for bad in (0, min(3, d) + 1, 2.0, "1"):
        with pytest.raises(ValueError, match="components"):
            geo.principal(xs, components=bad)
    with pytest.raises(ValueError, match="finite and > 0"):
        geo.principal(xs, weights=torch.tensor([1.0, -1.0, 1.0], device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.principal(xs.cpu())
    out = geo.principal(xs, components=np.int64(1))
    assert out["variances"].shape == (2, 1)
