"""The weighted projection on the GPU: the weighted Gauss-Newton step kernel (csrc/weighted_step.hip) against float64
numpy on the same float32 inputs, its output contract -- rows with w == 0 are never read --, isolation, determinism and refusals, and
``cmf_amd.ManifoldProjector.complete`` end to end on the reference-generated fixtures under the conditions
tests/test_completion_host.py establishes on the float64 reference loop.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds, per sample (u = 2^-53, sums over the rows with w > 0):
    |G_w - G_w64| <= C_WGRAM |J|^T diag(w) |J|                              tests/_weighted_step_emulation.py, from the emulation
    |g_k - g_ref_k| <= 2 (D + 3) u sum_i |J_ik| w_i |r_i|                   two float64 sums of D products of three factors
    ||A delta - g||_inf <= 32 d u (||A||_inf ||delta||_inf + ||g||_inf)     with the kernel's own gram and grad (GN.BOUND_C)
    cost: 2 (D + 3) u relative;  g^T delta, delta^T G_w delta: 2 (d + 2) u sum |terms|, against recomputation from the outputs.
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN."""
import math

import numpy as np
import pytest
import torch

import _completion_reference as CR
import _gn_step_emulation as GN
import _weighted_step_emulation as WS
from _gram_head import C_GRAM
from test_gpu_metric_stats import build
from test_gpu_projection import TAU, guarded, guards_intact, same_bits, stack

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
NAMES = ("gram", "grad", "delta", "stats", "info", "cost", "info_c")


def run(J, w, x, xhat, lam, layout="panel", nan_padding=True):
    """``engine.weighted_gauss_newton_step`` and ``engine.weighted_residual_sqnorm`` on CPU inputs -> numpy, in the order of NAMES."""
    from cmf_amd import engine as E
    d = J.shape[2]
    T = stack(J, layout) if nan_padding else E.Tangent.from_dense(torch.as_tensor(J).cuda(), E.ceil16(d), layout)
    wc, xc, hc = torch.as_tensor(w).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    r = E.weighted_gauss_newton_step(T, wc, xc, hc, torch.as_tensor(lam, dtype=torch.float64).cuda(), d=d)
    c, info_c = E.weighted_residual_sqnorm(wc, xc, hc)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r.gram, r.grad, r.delta, r.stats, r.info, c, info_c))


def dampings(B):
    return np.array([GN.DAMPINGS[b % len(GN.DAMPINGS)] for b in range(B)])


def check_sample(J, w, x, xhat, lam, gram, grad, delta, stats, info, label):
    """One sample's outputs against float64 numpy on the same float32 inputs, within the bounds of the module docstring."""
    D, d = J.shape
    live = w > 0
    J64, w64 = J[live].astype(np.float64), w[live].astype(np.float64)
    r = x[live].astype(np.float64) - xhat[live].astype(np.float64)
    G64, S = WS.gram64(J, w)
    ratio_g = WS.gram_ratio(gram, G64, S)
    assert ratio_g <= WS.C_WGRAM, label
    assert same_bits(gram, gram.T), label
    g_ref, g_abs = J64.T @ (w64 * r), np.abs(J64).T @ (w64 * np.abs(r))
    assert (np.abs(grad - g_ref) <= 2 * (D + 3) * U * g_abs).all(), label
    c_ref = float((w64 * r) @ r)
    assert abs(stats[0] - c_ref) <= 2 * (D + 3) * U * c_ref, label
    assert stats[3] == (np.abs(grad).max() if d else 0.0), label
    n_live = int(live.sum())
    if n_live == 0:
        assert info == 1 and (gram == 0).all() and (grad == 0).all() and stats[0] == 0, label
    elif n_live < d and lam == 0.0:
        assert info in (0, 1), label               # G_w of rank < d: a refused pivot and a completed factorisation are both legitimate
    else:
        assert info == 0, label
    if info == 1:
        assert np.isnan(delta).all() and np.isnan(stats[1:3]).all(), label
        return ratio_g, None
    ratio = GN.residual_ratio(gram, lam, grad, delta)
    assert ratio <= GN.BOUND_C, label
    Gs = GN.damped(gram, 0.0)
    assert abs(stats[1] - grad @ delta) <= 2 * (d + 2) * U * np.abs(grad * delta).sum(), label
    assert abs(stats[2] - delta @ Gs @ delta) <= 2 * (d + 2) * U * np.abs(Gs * np.outer(delta, delta)).sum(), label
    return ratio_g, ratio


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("d", GN.WIDTHS)
@pytest.mark.parametrize("D", GN.ROWS)
def test_kernel_matches_float64(D, d, layout):
    B = WS.batch_size()                                              # every weight pattern with every damping
    J, _, x, xhat = GN.inputs(B, D, d)
    w, lam = WS.weights(B, D, d), dampings(B)
    gram, grad, delta, stats, info, cost, info_c = run(J, w, x, xhat, lam, layout)
    out = [check_sample(J[b], w[b], x[b], xhat[b], lam[b], gram[b], grad[b], delta[b], stats[b], info[b],
                        f"sample {b} ({WS.PATTERNS[b % 5]}, lambda {lam[b]:g})") for b in range(B)]
    print(f"D={D} d={d} {layout}: worst |G_w - G_w64| / S = 2^{math.log2(max(max(o[0] for o in out), 1e-300)):.2f} (bound "
          f"2^{math.log2(WS.C_WGRAM):g}); worst residual / (d 2^-53 scale) = {max([o[1] for o in out if o[1] is not None], default=0.0):.3f} "
          f"(bound {GN.BOUND_C:g}); info {info.tolist()}")
    assert same_bits(cost, stats[:, 0]) and (info_c == 0).all()     # the cost-only mode: the same bits


@pytest.mark.parametrize("D,d,layout", [(5, 3, "panel"), (64, 17, "fmajor"), (784, 64, "panel"), (784, 128, "fmajor"), (64, 100, "panel")])
def test_zero_weight_rows_are_not_read(D, d, layout):
    B = WS.batch_size()
    J, _, x, xhat = GN.inputs(B, D, d, seed=4)
    w, lam = WS.weights(B, D, d, seed=4), dampings(B)
    dead = w == 0
    Jn, xn, hn = J.copy(), x.copy(), xhat.copy()
    Jn[dead], xn[dead], hn[dead] = NAN, NAN, NAN
    Jo, xo, ho = J.copy(), x.copy(), xhat.copy()
    Jo[dead], xo[dead], ho[dead] = 3.0e30, -1.0e30, 7.0
    base, poisoned, other = run(J, w, x, xhat, lam, layout), run(Jn, w, xn, hn, lam, layout), run(Jo, w, xo, ho, lam, layout)
    for name, a, b, c in zip(NAMES, base, poisoned, other):
        assert same_bits(a, b) and same_bits(b, c), name
    gram, grad, delta, stats, info, cost, info_c = poisoned
    assert (info_c == 0).all() and np.isfinite(cost).all() and np.isfinite(gram).all() and np.isfinite(grad).all()
    assert set(info.tolist()) <= {0, 1} and np.isfinite(delta[info == 0]).all() and np.isfinite(stats[info == 0]).all()
    assert np.isfinite(stats[:, [0, 3]]).all()


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("D,d", [(5, 3), (64, 17), (784, 64), (784, 100), (64, 128), (5, 16)])
def test_unit_weights_agree_with_the_unweighted_kernels(D, d, layout):
    """To bounds, not to bits: the two Gram kernels sum in different orders, and so do the two float64 gradients."""
    from cmf_amd import engine as E
    B = 3
    J, _, x, xhat = GN.inputs(B, D, d, seed=5)
    w, lam = np.ones((B, D), dtype=np.float32), np.array([0.0, 1e-3, 10.0])
    gram, grad, delta, stats, info, cost, _ = run(J, w, x, xhat, lam, layout, nan_padding=False)
    T = E.Tangent.from_dense(torch.as_tensor(J).cuda(), E.ceil16(d), layout)       # zero padding columns: the Gram head's contract
    jtj = E.gram_cholesky(T, d, 1).jtj
    r = E.gauss_newton_step(T, jtj, torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda(), torch.as_tensor(lam).cuda())
    torch.cuda.synchronize()
    jtj, grad_u, stats_u = jtj.cpu().numpy(), r.grad.cpu().numpy(), r.stats.cpu().numpy()
    J64 = J.astype(np.float64)
    res = x.astype(np.float64) - xhat.astype(np.float64)
    for b in range(B):
        S = np.abs(J64[b]).T @ np.abs(J64[b])
        assert (np.abs(gram[b].astype(np.float64) - jtj[b]) <= (WS.C_WGRAM + C_GRAM) * S).all()
        g_abs = np.abs(J64[b]).T @ np.abs(res[b])
        assert (np.abs(grad[b] - grad_u[b]) <= (2 * (D + 3) + 2 * (D + 2)) * U * g_abs).all()
        assert abs(stats[b, 0] - stats_u[b, 0]) <= (2 * (D + 3) + 2 * (D + 2)) * U * stats_u[b, 0]


@pytest.mark.parametrize("B,D,d,layout", [(5, 64, 17, "panel"), (5, 784, 64, "fmajor"), (5, 5, 100, "panel"), (5, 64, 128, "fmajor")])
def test_outputs_stay_inside_their_buffers(B, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    J, _, x, xhat = GN.inputs(B, D, d, seed=2)
    w, lam = WS.weights(B, D, d, seed=2), np.full(B, 1e-3)
    T = stack(J, layout)
    wc, xc, hc, lc = (torch.as_tensor(v).cuda() for v in (w, x, xhat, lam))
    bufs = {"gram": guarded((B, d, d), torch.float32), "grad": guarded((B, d), torch.float64), "delta": guarded((B, d), torch.float64),
            "stats": guarded((B, 4), torch.float64), "info": guarded((B,), torch.int32), "stats_c": guarded((B, 4), torch.float64),
            "info_c": guarded((B,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    lib = _lib.load()
    _lib.check(lib.cmf_weighted_gauss_newton_step(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(wc), E._p(xc), E._p(hc), E._p(lc),
                                                  p("gram"), p("grad"), p("delta"), p("stats"), p("info"), E._stream()), "weighted step")
    _lib.check(lib.cmf_weighted_gauss_newton_step(None, 0, 0, D, 0, 0, B, E._p(wc), E._p(xc), E._p(hc), None, None, None, None,
                                                  p("stats_c"), p("info_c"), E._stream()), "weighted step")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    gram, grad, delta, stats, info, cost, info_c = run(J, w, x, xhat, lam, layout)
    got = lambda name: bufs[name][1].cpu().numpy()
    assert same_bits(got("gram"), gram) and same_bits(got("grad"), grad) and same_bits(got("delta"), delta)
    assert same_bits(got("stats"), stats) and (got("info") == info).all() and (got("info_c") == 0).all()
    sc = got("stats_c")
    assert same_bits(sc[:, 0], cost) and np.isnan(sc[:, 1:]).all()  # the cost-only mode writes stats[b][0] alone


@pytest.mark.parametrize("D,d,layout", [(64, 17, "panel"), (784, 100, "panel"), (64, 17, "fmajor"), (1100, 33, "fmajor")])
def test_position_independence_and_repeatability(D, d, layout):
    """(1100, 33): more rows than one scan chunk of 1024, so the carry of live rows from chunk to chunk is on the path."""
    J, _, x, xhat = GN.inputs(5, D, d, seed=3)
    w, lam = WS.weights(5, D, d, seed=3), np.array([0.0, 1e-3, 10.0, 1e-3, 0.0])
    where = [0, 1, 2, 2, 4, 3, 1, 2, 0, 0, 3]
    base = run(J, w, x, xhat, lam, layout)
    batch = run(J[where], w[where], x[where], xhat[where], lam[where], layout)
    again = run(J[where], w[where], x[where], xhat[where], lam[where], layout)
    for a, b, c in zip(base, batch, again):
        assert same_bits(a[where], b) and same_bits(b, c)
    for b in range(4):
        check_sample(J[b], w[b], x[b], xhat[b], lam[b], *(o[b] for o in base[:5]), f"sample {b}")


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
def test_failures_are_reported_and_confined(layout):
    D, d = 64, 5
    J, _, x, xhat = GN.inputs(8, D, d, seed=1)
    w = np.ones((8, D), dtype=np.float32)
    w[:, ::3] = 0.0                                                  # rows 0, 3, 6, ... are dead
    w[:, 1::3] = 2.5
    lam = np.zeros(8)
    clean = run(J, w, x, xhat, lam, layout)
    assert (clean[4] == 0).all()
    w[1, 4] = -1.0
    w[2, 5] = NAN
    x[3, 7] = np.inf                                                 # live rows
    xhat[4, 1] = NAN
    J[5, 2, 4] = NAN
    x[6, 3], xhat[6, 6], J[6, 9, 1] = NAN, np.inf, NAN               # dead rows: not an error
    w[7] = 0.0
    gram, grad, delta, stats, info, cost, info_c = run(J, w, x, xhat, lam, layout)
    assert info.tolist() == [0, 2, 2, 2, 2, 2, 0, 1] and info_c.tolist() == [0, 2, 2, 2, 2, 0, 0, 0]
    for b in (1, 2, 3, 4, 5):
        assert all(np.isnan(o[b]).all() for o in (gram, grad, delta, stats))
    assert np.isnan(cost[[1, 2, 3, 4]]).all() and same_bits(cost[[0, 5, 6]], clean[5][[0, 5, 6]])
    for got, want in zip((gram, grad, delta, stats), clean):
        assert same_bits(got[[0, 6]], want[[0, 6]])
    assert np.isnan(delta[7]).all() and np.isnan(stats[7, 1:3]).all() and (gram[7] == 0).all() and (grad[7] == 0).all()
    assert stats[7, 0] == 0 and stats[7, 3] == 0 and cost[7] == 0
    assert WS.batch(J, w, x, xhat, lam)[4].tolist() == info.tolist()
    w[1, 4] = np.inf                                                 # a weight that is not finite
    assert run(J, w, x, xhat, lam, layout)[4].tolist() == [0, 2, 2, 2, 2, 2, 0, 1]


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, D, d = 2, 8, 3
    J, _, x, xhat = GN.inputs(B, D, d)
    T = stack(J, "panel")
    wc, xc, hc = torch.ones(B, D, device="cuda"), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    lc = torch.zeros(B, dtype=torch.float64, device="cuda")
    gram = torch.zeros(B * d * d, device="cuda")
    grad, delta = torch.zeros(B * d + 1, dtype=torch.float64, device="cuda"), torch.zeros(B * d, dtype=torch.float64, device="cuda")
    stats, info = torch.zeros(B * 4, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    odd = grad.view(torch.float32)[1:]                              # 4 bytes past an 8-byte boundary
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(wc), E._p(xc), E._p(hc), E._p(lc), E._p(gram), E._p(grad), E._p(delta),
          E._p(stats), E._p(info)]
    assert lib.cmf_weighted_gauss_newton_step(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(delta.abs().sum()) > 0 and float(gram.abs().sum()) > 0
    for t in (gram, grad, delta, stats):
        t.zero_()
    bad = [(1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (3, 0), (4, 24), (4, 0), (5, 0), (5, 129), (5, 17), (6, 0), (7, None), (8, None),
           (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None),
           (0, E._p(T.data.view(torch.float32)[1:])), (10, E._p(odd)), (12, E._p(odd)), (13, E._p(odd)), (14, E._p(odd))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_weighted_gauss_newton_step(*args, E._stream()) == -1, (i, value)
    # cost-only mode: w, x, xhat, stats and info are still required
    res = [None, 0, 0, D, 0, 0, B, E._p(wc), E._p(xc), E._p(hc), None, None, None, None, E._p(stats), E._p(info)]
    for i, value in ((3, 0), (6, 0), (7, None), (8, None), (9, None), (14, None), (15, None), (14, E._p(odd))):
        args = list(res)
        args[i] = value
        assert lib.cmf_weighted_gauss_newton_step(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in (gram, grad, delta, stats))


def test_engine_refusals():
    from cmf_amd import engine as E
    J, _, x, xhat = GN.inputs(2, 8, 3)
    T, xc, hc = stack(J, "panel"), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    wc, lam = torch.ones(2, 8, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.weighted_gauss_newton_step(E.Tangent(2, 8, 144, "panel", "cuda"), wc, xc, hc, lam)
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.weighted_gauss_newton_step(T, wc, xc, hc, lam, d=0)
    with pytest.raises(ValueError, match="must hold"):
        E.weighted_gauss_newton_step(T, wc, xc, hc, lam, d=17)
    with pytest.raises(ValueError, match="contiguous"):
        E.weighted_gauss_newton_step(T, wc.t().contiguous().t(), xc, hc, lam, d=3)
    with pytest.raises(ValueError, match="contiguous"):
        E.weighted_residual_sqnorm(wc[:, :7], xc[:, :7].contiguous(), hc[:, :7].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        E.weighted_gauss_newton_step(T, wc[:1].contiguous(), xc, hc, lam, d=3)
    with pytest.raises(ValueError, match="float32"):
        E.weighted_gauss_newton_step(T, wc.double(), xc, hc, lam, d=3)
    with pytest.raises(ValueError, match="float32"):
        E.weighted_residual_sqnorm(wc > 0, xc, hc)
    with pytest.raises(ValueError, match="float64"):
        E.weighted_gauss_newton_step(T, wc, xc, hc, lam.float(), d=3)
    with pytest.raises(ValueError, match="must agree"):
        E.weighted_residual_sqnorm(wc, xc, hc[:, :7].contiguous())
    with pytest.raises(ValueError, match="must hold"):
        E.weighted_gauss_newton_step(T, wc[:, :7].contiguous(), xc[:, :7].contiguous(), hc[:, :7].contiguous(), lam, d=3)
    with pytest.raises(ValueError, match="engine.Tangent"):
        E.weighted_gauss_newton_step(T.data, wc, xc, hc, lam, d=3)
    for cpu in ((T, wc.cpu(), xc, hc, lam), (T, wc, xc.cpu(), hc, lam), (T, wc, xc, hc.cpu(), lam)):
        with pytest.raises(ValueError, match="GPU"):
            E.weighted_gauss_newton_step(*cpu, d=3)
    # B == 0: empties, no launch
    r = E.weighted_gauss_newton_step(E.Tangent(0, 8, 16, "panel", "cuda"), wc[:0], xc[:0], hc[:0], lam[:0], d=3)
    assert r.gram.shape == (0, 3, 3) and r.grad.shape == (0, 3) and r.delta.shape == (0, 3) and r.stats.shape == (0, 4)
    assert r.info.shape == (0,)
    c, info = E.weighted_residual_sqnorm(wc[:0], xc[:0], hc[:0])
    assert c.shape == (0,) and c.dtype == torch.float64 and info.shape == (0,)


def test_kernel_timer_entries():
    from cmf_amd import engine as E
    J, _, x, xhat = GN.inputs(2, 8, 3)
    T, xc, hc = stack(J, "panel"), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    wc = torch.ones(2, 8, device="cuda")
    with E.timing(lambda name: True) as timer:
        E.weighted_gauss_newton_step(T, wc, xc, hc, torch.zeros(2, dtype=torch.float64, device="cuda"), d=3)
        E.weighted_residual_sqnorm(wc, xc, hc)
    by = timer.by_name()
    assert set(by) == {"weighted_gauss_newton_step", "weighted_residual_sqnorm"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())
    # the cost model counts the live rows, once: half of them dead is about half the Jacobian bytes
    wc[:, ::2] = 0.0
    with E.timing(lambda name: True) as half:
        E.weighted_gauss_newton_step(T, wc, xc, hc, torch.zeros(2, dtype=torch.float64, device="cuda"), d=3)
    assert half.by_name()["weighted_gauss_newton_step"][3] < by["weighted_gauss_newton_step"][3]


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------


def run_complete(dens, head, x, w, steps, init=None):
    """One ``complete`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(dens, steps=steps)
    keep, keep_w, marker = x.clone(), w.clone(), object()
    head.last_gram = marker
    out = proj.complete(x, w, init=init)
    assert head.last_gram is marker and torch.equal(x, keep) and torch.equal(w, keep_w)
    B, d = x.shape[0], head.program.d
    assert set(out) == {"latent", "reconstruction_head", "reconstruction", "cost", "initial_cost", "tangential2", "gradient",
                        "distance2", "observed", "accepted", "damping", "info"}
    assert out["latent"].shape == (B, d) and out["latent"].dtype == torch.float32 and out["gradient"].shape == (B, d)
    assert out["reconstruction_head"].shape == (B, *head.x_shape) and out["reconstruction"].shape == x.shape
    for key in ("cost", "initial_cost", "tangential2", "distance2", "damping"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64
    for key in ("accepted", "info", "observed"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["accepted"] <= steps).all())
    assert bool((out["accepted"] >= 0).all())
    return proj, out


@pytest.mark.parametrize("name", CR.KNOWN_ANSWER)
def test_completion_finds_the_known_answer(name):
    """x_on = the GPU's own g(z_0) at the encoder's latent of the fixture's input; half of its elements are observed exactly with
    weights in [0.25, 4], the hidden ones are off by 0.1 ||x_on|| / sqrt(D) randn.  z_0 is a minimiser with cost 0, and ten steps
    from the encoder's latent of that input must reconstruct x_on -- the hidden elements included -- within the tolerance
    tests/test_completion_host.py derives from the project's x_hat tolerance (CR.E2E_TOL)."""
    g, meta, dens, head, x = build(name)
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on = head.flow_forward(z0)
    y, w = CR.problem(x_on, seed=0)
    seen = w > 0
    assert torch.equal(y[seen], x_on.cpu()[seen]) and not torch.equal(y, x_on.cpu())
    _, out = run_complete(head, head, y.cuda().contiguous(), w.cuda().contiguous(), 10)
    rel = CR.rel_distance(out["reconstruction_head"], x_on)
    start = CR.rel_distance(y, x_on)
    print(f"{name}: ||g(z) - x_on|| / ||x_on|| <= {float(rel.max()):.3e} (tolerance {CR.E2E_TOL[name]:.3e}; the input is off by "
          f"{float(start.min()):.3e} .. {float(start.max()):.3e}); cost {float(out['initial_cost'].max()):.3e} -> "
          f"{float(out['cost'].max()):.3e}; accepted {out['accepted'].tolist()}")
    assert bool((rel <= CR.E2E_TOL[name]).all())
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["info"] == 0).all())
    assert out["observed"].cpu().tolist() == seen.flatten(1).sum(1).tolist()
    assert out["observed"].cpu().tolist() == [math.ceil(0.5 * x_on[0].numel())] * len(x_on)
    with torch.no_grad():
        assert torch.equal(out["reconstruction_head"], head.flow_forward(out["latent"]))


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass", "c1_sphere_d2"])
def test_unit_weights_reach_the_distance_of_project(name):
    """With every weight one the cost is the distance, and ``complete`` -- through the density's wrapper chain, with the Gram matrix
    of its own kernel -- must end where ``project`` ends.  On the smooth fixtures, where Gauss-Newton converges to the minimiser from
    the encoder's latent (tests/test_projection_host.py); on the relu fixtures both loops stall at kinks, at points that depend on
    rounding-level differences of the steps, so the two distances there are not comparable to TAU."""
    import cmf_amd
    g, meta, dens, head, x = build(name)
    ones = torch.ones_like(x)
    _, out = run_complete(dens, head, x, ones, 10)
    ref = cmf_amd.ManifoldProjector(dens, steps=10).project(x)
    rel = ((out["distance2"] - ref["distance2"]).abs() / ref["distance2"]).cpu()
    print(f"{name}: |distance2 - project's| / project's <= {float(rel.max()):.3e} (tau {TAU:g}); accepted {out['accepted'].tolist()} "
          f"against {ref['accepted'].tolist()}")
    assert bool((rel <= TAU).all()) and bool((out["info"] == 0).all())
    D = x[0].numel()
    assert bool(((out["cost"] - out["distance2"]).abs() <= 4 * (D + 3) * U * out["distance2"]).all())
    assert torch.equal(out["initial_cost"], ref["initial_distance2"]) or bool(
        ((out["initial_cost"] - ref["initial_distance2"]).abs() <= 4 * (D + 3) * U * ref["initial_distance2"]).all())
    assert out["observed"].cpu().tolist() == [D] * len(x)
    # weights that broadcast over the batch, and a bool mask, are the same problem
    _, again = run_complete(dens, head, x, torch.ones(x.shape[1:], dtype=torch.bool, device="cuda"), 10)
    assert all(same_bits(out[k].cpu().numpy(), again[k].cpu().numpy()) for k in out)


def test_init_is_honoured():
    g, meta, dens, head, x = build("c2b_hepmass")
    w = torch.ones_like(x)
    w[:, ::3] = 0.0
    with torch.no_grad():
        z_enc = dens.extract_latent(x.clone(), earliest_latent=False)
    init = (z_enc + 0.05).contiguous()
    _, at_init = run_complete(dens, head, x, w, 0, init=init)
    _, at_enc = run_complete(dens, head, x, w, 0)
    assert torch.equal(at_init["latent"], init) and torch.equal(at_enc["latent"], z_enc)
    assert torch.equal(at_init["cost"], at_init["initial_cost"]) and not torch.equal(at_init["cost"], at_enc["cost"])
    with torch.no_grad():
        assert torch.equal(at_init["reconstruction_head"], head.flow_forward(init))
    assert bool((at_init["accepted"] == 0).all())
    _, moved = run_complete(dens, head, x, w, 10, init=init)
    assert bool((moved["cost"] <= at_init["cost"]).all()) and bool((moved["accepted"] > 0).any())


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_rows_of_one_call(name, monkeypatch):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    x = x[:3].contiguous()
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on = head.flow_forward(z0)
    y, w = CR.problem(x_on, seed=1)
    for b in range(3):                                               # a different number of observed elements per sample:
        hidden = torch.nonzero(w.flatten(1)[b] == 0)[:b, 0]          # sample b also observes its first b hidden elements, exactly
        w.flatten(1)[b, hidden] = 1.0
        y.flatten(1)[b, hidden] = x_on.cpu().flatten(1)[b, hidden]
    y, w = y.cuda().contiguous(), w.cuda().contiguous()
    init = (z0 + 0.01 * torch.arange(1, 4, device="cuda")[:, None]).contiguous()
    _, whole = run_complete(head, head, y, w, 10, init=init)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    _, pieces = run_complete(head, head, y, w, 10, init=init)
    c0 = whole["initial_cost"]
    print(f"{name}: pieces against whole: bit-equal latent {torch.equal(pieces['latent'], whole['latent'])}, cost rel "
          f"{float(((pieces['cost'] - whole['cost']).abs() / c0).max()):.2e}")
    assert float(((pieces["initial_cost"] - c0).abs() / c0).max()) <= 1e-5
    assert float(((pieces["cost"] - whole["cost"]).abs() / c0).max()) <= 1e-5
    assert torch.equal(pieces["observed"], whole["observed"])
    assert whole["observed"].cpu().tolist() == (w > 0).flatten(1).sum(1).cpu().tolist() and len(set(whole["observed"].cpu().tolist())) == 3
    assert bool((pieces["info"] == 0).all()) and bool((whole["info"] == 0).all())


def test_the_log_density_path_is_untouched():
    import cmf_amd
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    w = (torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) < 0.5).cuda()
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        out = cmf_amd.ManifoldProjector(dens, steps=3).complete(x, w)
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
    assert out["observed"].cpu().tolist() == w.flatten(1).sum(1).cpu().tolist() and bool((out["info"] == 0).all())
