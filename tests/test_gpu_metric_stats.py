"""Metric statistics on the GPU: the accumulate kernel (csrc/metric_stats.hip) against float64 torch on the same float32 input,
its determinism and skip rule, and ``cmf_amd.MetricStatistics`` end to end against the reference-generated fixtures in both
coordinate systems.  Needs an MI355X: run with ``-m gpu``.

Kernel bound, every element of S_G, S_cos and sample_macs:  |got - want| <= (2 B + 12) 2^-53 sum_b |term_b|.  Both sides do the
same <= 6 correctly rounded float64 operations per term plus a B-term sum, and the build uses no fast-math flags; sample_macs is
rounded to float32 on output, which adds 2^-24 |want|.  count and skipped are exact."""
import math

import numpy as np
import pytest
import torch

from conftest import COND, FULL, SMALL, golden_model, kink_tolerance, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
NAN = float("nan")


def synthetic(B, d, seed=0):
    """SPD Gram matrices G = A^T A of A = randn(B, d + 3, d) with the columns scaled by powers of two spanning 2^-6 .. 2^6."""
    gen = torch.Generator().manual_seed(1000 * d + B + seed)
    scale = 2.0 ** torch.linspace(-6, 6, d).round()
    A = torch.randn(B, d + 3, d, generator=gen) * scale
    return torch.bmm(A.transpose(1, 2), A).contiguous()


def reference(G32):
    """float64 torch on the same float32 input: (S_G, S_cos, count, skipped, sample_macs) and the sums of |term| of each."""
    G = G32.double()
    B, d = G.shape[0], G.shape[1]
    diag = torch.diagonal(G, dim1=1, dim2=2)
    valid = (torch.isfinite(diag) & (diag > 0)).all(1)
    n = diag.sqrt() + 1e-8
    cos = G / (n[:, :, None] * n[:, None, :])
    off = ~torch.eye(d, dtype=torch.bool)
    macs = (cos.abs() * off).sum((1, 2)) / (d * (d - 1)) if d > 1 else torch.zeros(B, dtype=torch.float64)
    macs = torch.where(valid, macs, torch.full_like(macs, NAN))
    Gv, cv = G[valid], cos[valid]
    return {"S_G": Gv.sum(0), "S_cos": cv.sum(0), "abs_G": Gv.abs().sum(0), "abs_cos": cv.abs().sum(0),
            "count": int(valid.sum()), "skipped": int((~valid).sum()), "macs": macs}


def guarded(n, dtype):
    """A zeroed tensor of n elements between two NaN-filled guard bands: (whole buffer, the view)."""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n]
    view.zero_()
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def accumulate(batches):
    """Run the kernel over ``batches`` (CPU float32 tensors) into one guarded state: (state on the CPU, [sample_macs on the CPU])."""
    from cmf_amd import engine as E
    d = batches[0].shape[1]
    sbuf, state = guarded(E.metric_stats_state_size(d), torch.float64)
    out = []
    for G in batches:
        mbuf, macs = guarded(G.shape[0], torch.float32)
        ws_n = E.metric_stats_workspace_size(G.shape[0], d)
        wbuf, ws = guarded(ws_n, torch.float64)
        E.metric_stats_accumulate(G.cuda(), state, workspace=ws, sample_macs=macs)
        torch.cuda.synchronize()
        assert guards_intact(mbuf) and guards_intact(wbuf)
        out.append(macs.cpu())
    assert guards_intact(sbuf)
    return state.cpu(), out


def check_state(state, want, B, label=""):
    """``state`` against ``reference`` output ``want`` within the kernel bound for B accumulated samples."""
    dd = want["S_G"].numel()
    d = int(math.isqrt(dd))
    got_G, got_cos = state[:dd].view(d, d), state[dd:2 * dd].view(d, d)
    k = (2 * B + 12) * U
    err_G, err_cos = (got_G - want["S_G"]).abs(), (got_cos - want["S_cos"]).abs()
    print(f"{label} B={B} d={d}: S_G err/bound {float((err_G / (k * want['abs_G']).clamp_min(1e-300)).max()):.3f}, "
          f"S_cos err/bound {float((err_cos / (k * want['abs_cos']).clamp_min(1e-300)).max()):.3f}")
    assert bool((err_G <= k * want["abs_G"]).all())
    assert bool((err_cos <= k * want["abs_cos"]).all())
    assert float(state[2 * dd]) == want["count"] and float(state[2 * dd + 1]) == want["skipped"]


def check_macs(got, want, B):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    err = (got.double() - want).abs()[~nan]
    bound = ((2 * B + 12) * U + 2.0 ** -24) * want.abs()[~nan]
    print(f"sample_macs err/bound {float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0:.3f}")
    assert bool((err <= bound).all())


def chunk():
    from cmf_amd import engine as E
    return E.METRIC_STATS_CHUNK


SHAPES = [(1, 1), (3, 2), (5, 3), (33, 10), (64, 16), (7, 64), (33, 100), (2, 128), (3, 130), (2, 512)]


@pytest.mark.parametrize("B,d", SHAPES + [("L", 10), ("L+1", 10), ("2L+1", 10)])
def test_kernel_matches_float64_torch(B, d):
    L = chunk()
    B = {"L": L, "L+1": L + 1, "2L+1": 2 * L + 1}.get(B, B)
    G = synthetic(B, d)
    want = reference(G)
    assert want["count"] == B
    state, (macs,) = accumulate([G])
    check_state(state, want, B, "single call")
    check_macs(macs, want["macs"], B)
    if d == 1:
        assert torch.equal(macs, torch.zeros(B))


def test_same_call_sequence_is_bit_identical_and_streams():
    L = chunk()
    A, Bm = synthetic(L + 5, 10, seed=1), synthetic(2 * L + 3, 10, seed=2)
    s1, m1 = accumulate([A, Bm])
    s2, m2 = accumulate([A, Bm])
    assert torch.equal(s1, s2) and all(torch.equal(a, b) for a, b in zip(m1, m2))
    both = torch.cat((A, Bm))
    want = reference(both)
    check_state(s1, want, both.shape[0], "two calls")
    s3, (m3,) = accumulate([both])
    check_state(s3, want, both.shape[0], "one call")
    dd = 100
    k = (2 * both.shape[0] + 12) * U
    assert bool(((s1[:dd] - s3[:dd]).abs() <= k * want["abs_G"].reshape(-1)).all())
    assert bool(((s1[dd:2 * dd] - s3[dd:2 * dd]).abs() <= k * want["abs_cos"].reshape(-1)).all())
    assert torch.equal(s1[2 * dd:], s3[2 * dd:])
    check_macs(torch.cat(m1), want["macs"], both.shape[0])
    check_macs(m3, want["macs"], both.shape[0])


def test_skip_rule():
    G = synthetic(6, 5, seed=3)
    G[1, 2, 2] = 0.0
    G[3, 0, 0] = NAN
    G[4, 4, 4] = float("inf")
    clean = G[[0, 2, 5]].contiguous()
    state, (macs,) = accumulate([G])
    want = reference(G)
    assert want["count"] == 3 and want["skipped"] == 3
    check_state(state, want, 6, "skip rule")
    assert float(state[50]) == 3 and float(state[51]) == 3
    alone, (macs_alone,) = accumulate([clean])
    assert torch.equal(state[:50], alone[:50]) and float(alone[50]) == 3 and float(alone[51]) == 0
    assert bool(torch.isnan(macs[[1, 3, 4]]).all()) and torch.equal(macs[[0, 2, 5]], macs_alone)
    check_macs(macs, want["macs"], 6)


def test_engine_refuses_wrong_buffers():
    from cmf_amd import engine as E
    G = synthetic(2, 3).cuda()
    state = torch.zeros(E.metric_stats_state_size(3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        E.metric_stats_accumulate(G, state[:-1])
    with pytest.raises(ValueError):
        E.metric_stats_accumulate(G, state.float())
    with pytest.raises(ValueError):
        E.metric_stats_accumulate(G, state, workspace=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        E.metric_stats_accumulate(G, state, sample_macs=torch.zeros(3, device="cuda"))
    with pytest.raises(RuntimeError):
        E.metric_stats_accumulate(G.cpu(), state)
    assert float(state.abs().sum()) == 0.0


# --------------------------------------------------------------------------------------------------
# end to end against the fixtures
# --------------------------------------------------------------------------------------------------


def build(name):
    import cmf_amd
    from cmf_amd.densities import NonSquareHeadDensity
    from cmf_amd.recipe import fill_state_dict
    g, meta = load_golden(name)
    cfg = cmf_amd.get_config(meta["dataset"], **meta["overrides"])
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), g["x"])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=meta["recipe_seed"], gain=meta.get("recipe_gain")), strict=True)
    dens = dens.cuda().eval()
    head = next(m for m in dens.modules() if isinstance(m, NonSquareHeadDensity))
    x = ((g["x"] + g["noise"]) if "noise" in g else g["x"]).float().cuda()      # the input the fixture's jtj was computed at
    return g, meta, dens, head, x


def check_against(result, G_ref, tol, label):
    """The finalised statistics against the float64 Gram matrices ``G_ref`` (B, d, d) of the reference, whose own tolerance is
    ``tol`` relative to max |G_b| (conftest.kink_tolerance): the mean metric in the max-norm, the mean cosines per element under
    the first-order propagation of delta_b = tol max |G_b| through cos_ij = G_ij / (n_i n_j)."""
    G = G_ref.double().numpy()
    B, d = G.shape[0], G.shape[1]
    assert result["skipped"] == 0 and result["count"] == B
    mm = G.mean(0)
    got = result["mean_metric"].numpy()
    rel = np.abs(got - mm).max() / np.abs(mm).max()
    diag = np.einsum("bkk->bk", G)
    n = np.sqrt(diag) + 1e-8
    nn_ = n[:, :, None] * n[:, None, :]
    cos = G / nn_
    delta = tol * np.abs(G).reshape(B, -1).max(1)
    bound = (delta[:, None, None] / nn_
             + np.abs(cos) * delta[:, None, None] * (0.5 / diag[:, :, None] + 0.5 / diag[:, None, :])).mean(0)
    mc = cos.mean(0)
    err = np.abs(result["mean_cosine"].numpy() - mc)
    off = ~np.eye(d, dtype=bool)
    macs, macs_off = np.abs(mc).mean(), (np.abs(mc)[off].mean() if d > 1 else 0.0)
    print(f"{label}: mean_metric rel {rel:.2e} (tol {tol:.2e}); mean_cosine err/bound {(err / bound).max():.3f}, max bound "
          f"{bound.max():.2e}; macs {result['macs']:.6f} want {macs:.6f}; offdiag {result['macs_offdiag']:.6f} want {macs_off:.6f}")
    assert rel <= tol
    assert (err <= bound).all()
    assert abs(result["macs"] - macs) <= bound.mean()
    assert abs(result["macs_offdiag"] - macs_off) <= (bound[off].mean() if d > 1 else 0.0)
    md = result["mean_diagonal"]
    assert torch.equal(md, torch.diagonal(result["mean_metric"]))
    assert torch.equal(result["ranking"], torch.argsort(md.abs(), stable=True))
    assert float(result["mean_metric_normalized"].abs().max()) == 1.0 and float(result["mean_diagonal_normalized"].abs().max()) == 1.0


def run_update(dens, head, x, coordinates):
    """One ``update`` with the side-effect checks every end-to-end case makes: x untouched, ``last_gram`` left alone."""
    import cmf_amd
    stats = cmf_amd.MetricStatistics(dens, coordinates=coordinates)
    keep, marker = x.clone(), object()
    head.last_gram = marker
    macs = stats.update(x)
    assert head.last_gram is marker and torch.equal(x, keep)
    assert macs.shape == (x.shape[0],) and macs.is_cuda and macs.dtype == torch.float32 and bool(torch.isfinite(macs).all())
    return stats, macs


@pytest.mark.parametrize("name", SMALL + COND + FULL)
def test_latent_coordinates_match_the_fixture(name):
    g, meta, dens, head, x = build(name)
    stats, macs = run_update(dens, head, x, "latent")
    check_against(stats.result(), g["jtj"], kink_tolerance(g), name)
    # a second batch streams onto the first: twice the sums, the same means
    stats.update(x)
    twice = stats.result()
    assert twice["count"] == 2 * x.shape[0]
    check_against({**twice, "count": x.shape[0]}, g["jtj"], kink_tolerance(g), name + " (two updates)")
    stats.reset()
    with pytest.raises(ValueError):
        stats.result()


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_single_piece_state(name, monkeypatch):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    x = x[:3].contiguous()
    whole, macs_whole = run_update(dens, head, x, "latent")
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    pieces, macs_pieces = run_update(dens, head, x, "latent")
    # sum_b |term_b| of the bound: from the Gram matrices the single-piece update accumulated, recomputed through the same calls
    with torch.no_grad():
        _, T = prog.decode(dens.extract_latent(x, earliest_latent=False), tangents=True)
        want = reference(E.gram_cholesky(T, prog.d, 1).jtj.cpu())
    a, b = whole.state.flat.cpu(), pieces.state.flat.cpu()
    check_state(a, want, 3, name + " whole")
    check_state(b, want, 3, name + " pieces")
    dd, k = prog.d ** 2, (2 * 3 + 12) * U
    assert bool(((a[:dd] - b[:dd]).abs() <= k * want["abs_G"].reshape(-1)).all())
    assert bool(((a[dd:2 * dd] - b[dd:2 * dd]).abs() <= k * want["abs_cos"].reshape(-1)).all())
    assert torch.equal(a[2 * dd:], b[2 * dd:])
    check_macs(macs_whole.cpu(), want["macs"], 3)
    check_macs(macs_pieces.cpu(), want["macs"], 3)


def prior_jacobians(meta, u):
    """P_b = d z_low / d u (d, d) in float64 per sample: autograd through the oracle's prior inverse at the fixture's earliest latent."""
    from oracle import cmf_oracle as O
    _, _, _, ops, sd = golden_model(meta, dtype=torch.float64)
    prior_ops = O.split_ops(ops)[4]
    f = lambda v: O.prior_inverse(sd, prior_ops, v[None])[0]
    return torch.stack([torch.autograd.functional.jacobian(f, ub) for ub in u.double()])


@pytest.mark.parametrize("name", SMALL + ["c3_mnist_full"])
def test_noise_coordinates_match_the_fixture(name):
    g, meta, dens, head, x = build(name)
    P = prior_jacobians(meta, g["earliest_latent"])
    G_ref = P.transpose(1, 2) @ g["jtj"].double() @ P
    stats, macs = run_update(dens, head, x, "noise")
    check_against(stats.result(), G_ref, kink_tolerance(g), name + " (noise)")


def test_noise_coordinates_refuse_an_nsf_prior():
    import cmf_amd
    cfg = cmf_amd.get_config("power", prior="nsf")
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), torch.zeros(2, 6))
    with pytest.raises(NotImplementedError, match="RandomChannelwisePermutationBijection|LULinearBijection|Autoregressive"):
        cmf_amd.MetricStatistics(dens, coordinates="noise")
    cmf_amd.MetricStatistics(dens, coordinates="latent")           # the latent coordinates need no prior tangent
