"""The manifold projection on the GPU: the Gauss-Newton step kernel (csrc/gn_step.hip) against float64 torch on the
same float32 inputs, its output contract, isolation, determinism and refusals, and ``cmf_amd.ManifoldProjector`` end to end on the
reference-generated fixtures under the conditions tests/test_projection_host.py establishes on the float64 reference loop.  Needs
an MI355X: run with ``-m gpu``.

Kernel bounds, per sample (u = 2^-53):
    |g_k - g_ref_k| <= 2 (D + 2) u sum_i |J_ik| |r_i|                       two float64 sums of D products, in different orders
    ||A delta - g||_inf <= 32 d u (||A||_inf ||delta||_inf + ||g||_inf)     with the kernel's own g; the form backward stability
                                                                            gives (the emulation stays inside a quarter of it)
    ||r||^2: 2 (D + 2) u relative;  g^T delta, delta^T G delta: 2 (d + 2) u sum |terms|, against recomputation from the outputs.
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN."""
import numpy as np
import pytest
import torch

import _gn_step_emulation as GN
import _projection_reference as R
from test_gpu_metric_stats import build

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
NAN = float("nan")
SMOOTH = ["c2a_power", "c2b_hepmass", "c1_sphere_d2"]
KINKED = ["mini_mnist", "mini_mnist_small", "mini_cifar"]
KNOWN_ANSWER = ["c2b_hepmass", "c2a_power", "mini_mnist"]
TAU = 2e-4                                     # 2 (1e-5 ||x_on||) / rho with rho = 0.1 ||x_on||: DESIGN 5's x_hat tolerance, first order


def stack(J, layout):
    """A CPU (B, D, d) float32 Jacobian as an ``engine.Tangent`` on the GPU whose padding columns are NaN."""
    from cmf_amd import engine as E
    B, D, d = J.shape
    nc = E.ceil16(d)
    T = E.Tangent.from_dense(torch.as_tensor(J).cuda(), nc, layout)
    view = T.data.view(B, D, nc) if layout == "panel" else T.data.view(D, B, nc)
    view[:, :, d:] = NAN
    return T


def run(J, G, x, xhat, lam, layout="panel"):
    """``engine.gauss_newton_step`` and ``engine.residual_sqnorm`` on CPU inputs -> numpy (grad, delta, stats, info, r2, info_r)."""
    from cmf_amd import engine as E
    xc, hc = torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    r = E.gauss_newton_step(stack(J, layout), torch.as_tensor(G).cuda(), xc, hc, torch.as_tensor(lam, dtype=torch.float64).cuda())
    r2, info_r = E.residual_sqnorm(xc, hc)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r.grad, r.delta, r.stats, r.info, r2, info_r))


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_sample(J, G, x, xhat, lam, grad, delta, stats, info, label):
    """One sample's outputs against float64 numpy on the same float32 inputs, within the bounds of the module docstring."""
    D, d = J.shape
    J64 = J.astype(np.float64)
    r = x.astype(np.float64) - xhat.astype(np.float64)
    g_ref, g_abs = J64.T @ r, np.abs(J64).T @ np.abs(r)
    assert (np.abs(grad - g_ref) <= 2 * (D + 2) * U * g_abs).all(), label
    assert abs(stats[0] - r @ r) <= 2 * (D + 2) * U * (r @ r), label
    assert stats[3] == np.abs(grad).max(), label
    if D < d and lam == 0.0:
        assert info in (0, 1), label               # G of rank D < d: a refused pivot and a completed factorisation are both legitimate
    else:
        assert info == 0, label
    if info == 1:
        assert np.isnan(delta).all() and np.isnan(stats[1:3]).all(), label
        return None
    ratio = GN.residual_ratio(G, lam, grad, delta)
    assert ratio <= GN.BOUND_C, label
    Gs = GN.damped(G, 0.0)
    assert abs(stats[1] - grad @ delta) <= 2 * (d + 2) * U * np.abs(grad * delta).sum(), label
    assert abs(stats[2] - delta @ Gs @ delta) <= 2 * (d + 2) * U * np.abs(Gs * np.outer(delta, delta)).sum(), label
    return ratio


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("d", GN.WIDTHS)
@pytest.mark.parametrize("D", GN.ROWS)
def test_kernel_matches_float64(D, d, layout):
    B = 2 * len(GN.DAMPINGS) + 1 if (D, d) != (64, 17) else 33      # every damping at least twice; once the largest batch
    J, G, x, xhat = GN.inputs(B, D, d)
    lam = np.array([GN.DAMPINGS[b % len(GN.DAMPINGS)] for b in range(B)])
    grad, delta, stats, info, r2, info_r = run(J, G, x, xhat, lam, layout)
    ratios = [check_sample(J[b], G[b], x[b], xhat[b], lam[b], grad[b], delta[b], stats[b], info[b], f"sample {b}") for b in range(B)]
    print(f"D={D} d={d} {layout}: worst residual / (d 2^-53 scale) = {max([q for q in ratios if q is not None], default=0.0):.3f} "
          f"(bound {GN.BOUND_C:g}); info {info.tolist()}")
    assert same_bits(r2, stats[:, 0]) and (info_r == 0).all()       # the residual-only mode: the same bits


def guarded(shape, dtype):
    n = int(np.prod(shape))
    fill = NAN if dtype.is_floating_point else -77
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape), fill


def guards_intact(buf, fill):
    edge = torch.cat((buf[:GUARD], buf[-GUARD:]))
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == fill).all())


@pytest.mark.parametrize("B,D,d,layout", [(3, 64, 17, "panel"), (2, 784, 64, "fmajor"), (3, 5, 100, "panel"), (2, 64, 128, "fmajor")])
def test_outputs_stay_inside_their_buffers(B, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    J, G, x, xhat = GN.inputs(B, D, d, seed=2)
    lam = np.full(B, 1e-3)
    T = stack(J, layout)
    Gc, xc, hc, lc = torch.as_tensor(G).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda(), torch.as_tensor(lam).cuda()
    bufs = {"grad": guarded((B, d), torch.float64), "delta": guarded((B, d), torch.float64), "stats": guarded((B, 4), torch.float64),
            "info": guarded((B,), torch.int32), "stats_r": guarded((B, 4), torch.float64), "info_r": guarded((B,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    lib = _lib.load()
    _lib.check(lib.cmf_gauss_newton_step(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(Gc), E._p(xc), E._p(hc), E._p(lc), p("grad"),
                                         p("delta"), p("stats"), p("info"), E._stream()), "cmf_gauss_newton_step")
    _lib.check(lib.cmf_gauss_newton_step(None, 0, 0, D, 0, 0, B, None, E._p(xc), E._p(hc), None, None, None, p("stats_r"), p("info_r"),
                                         E._stream()), "cmf_gauss_newton_step")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    grad, delta, stats, info, r2, info_r = run(J, G, x, xhat, lam, layout)
    got = lambda name: bufs[name][1].cpu().numpy()
    assert same_bits(got("grad"), grad) and same_bits(got("delta"), delta) and same_bits(got("stats"), stats)
    assert (got("info") == info).all() and (got("info_r") == 0).all()
    sr = got("stats_r")
    assert same_bits(sr[:, 0], r2) and np.isnan(sr[:, 1:]).all()    # the residual-only mode writes stats[b][0] alone


@pytest.mark.parametrize("D,d,layout", [(64, 17, "panel"), (784, 100, "panel"), (64, 17, "fmajor")])
def test_position_independence_and_repeatability(D, d, layout):
    J, G, x, xhat = GN.inputs(3, D, d, seed=3)
    lam = np.array([0.0, 1e-3, 10.0])
    where = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2]
    base = run(J, G, x, xhat, lam, layout)
    batch = run(J[where], G[where], x[where], xhat[where], lam[where], layout)
    again = run(J[where], G[where], x[where], xhat[where], lam[where], layout)
    for a, b, c in zip(base, batch, again):
        assert same_bits(a[where], b) and same_bits(b, c)
    # the upper triangle of jtj is never read
    upper = np.triu(np.ones((d, d), dtype=bool), 1)
    for a, b in zip(base, run(J, np.where(upper, np.float32(NAN), G), x, xhat, lam, layout)):
        assert same_bits(a, b)


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
def test_failures_are_reported_and_confined(layout):
    D, d = 64, 5
    J, G, x, xhat = GN.inputs(7, D, d, seed=1)
    lam = np.zeros(7)
    clean = run(J, G, x, xhat, lam, layout)
    assert (clean[3] == 0).all()
    J[1, :, 3] = J[1, :, 1]                                          # a duplicate column: the pivot cancels exactly
    G[1] = GN.gram_by_dots(J[1])
    x[2, 7] = np.inf
    xhat[3, 0] = NAN
    J[4, 3, 4] = NAN
    G[5, 4, 2] = NAN
    grad, delta, stats, info, r2, info_r = run(J, G, x, xhat, lam, layout)
    assert info.tolist() == [0, 1, 2, 2, 2, 2, 0] and info_r.tolist() == [0, 0, 2, 2, 0, 0, 0]
    assert np.isnan(delta[1]).all() and np.isnan(stats[1, 1:3]).all() and np.isfinite(grad[1]).all() and np.isfinite(stats[1, [0, 3]]).all()
    for b in (2, 3, 4, 5):
        assert np.isnan(grad[b]).all() and np.isnan(delta[b]).all() and np.isnan(stats[b]).all()
    assert np.isnan(r2[[2, 3]]).all() and same_bits(r2[[0, 1, 4, 5, 6]], clean[4][[0, 1, 4, 5, 6]])
    for got, want in zip((grad, delta, stats), clean):
        assert same_bits(got[[0, 6]], want[[0, 6]])
    e_info = GN.batch(J, G, x, xhat, lam)[3]
    assert e_info.tolist() == info.tolist()
    # the damping lifts the duplicate column's pivot
    assert run(J, G, x, xhat, np.full(7, 1e-3), layout)[3].tolist() == [0, 0, 2, 2, 2, 2, 0]


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, D, d = 2, 8, 3
    J, G, x, xhat = GN.inputs(B, D, d)
    T = stack(J, "panel")
    Gc, xc, hc = torch.as_tensor(G).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    lc = torch.zeros(B, dtype=torch.float64, device="cuda")
    grad, delta = torch.zeros(B * d + 1, dtype=torch.float64, device="cuda"), torch.zeros(B * d, dtype=torch.float64, device="cuda")
    stats, info = torch.zeros(B * 4, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    odd = grad.view(torch.float32)[1:]                              # 4 bytes past an 8-byte boundary
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(Gc), E._p(xc), E._p(hc), E._p(lc), E._p(grad), E._p(delta), E._p(stats),
          E._p(info)]
    assert lib.cmf_gauss_newton_step(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(delta.abs().sum()) > 0
    for t in (grad, delta, stats):
        t.zero_()
    bad = [(1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (3, 0), (4, 24), (4, 0), (5, 0), (5, 129), (5, 17), (6, 0), (7, None), (8, None),
           (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (0, E._p(T.data.view(torch.float32)[1:])),
           (10, E._p(odd)), (11, E._p(odd)), (12, E._p(odd)), (13, E._p(odd))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_gauss_newton_step(*args, E._stream()) == -1, (i, value)
    # residual-only mode: x, xhat, stats and info are still required
    res = [None, 0, 0, D, 0, 0, B, None, E._p(xc), E._p(hc), None, None, None, E._p(stats), E._p(info)]
    for i, value in ((3, 0), (6, 0), (8, None), (9, None), (13, None), (14, None), (13, E._p(odd))):
        args = list(res)
        args[i] = value
        assert lib.cmf_gauss_newton_step(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert float(grad.abs().sum()) == 0.0 and float(delta.abs().sum()) == 0.0 and float(stats.abs().sum()) == 0.0


def test_engine_refusals():
    from cmf_amd import engine as E
    J, G, x, xhat = GN.inputs(2, 8, 3)
    T, Gc, xc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    lam = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.gauss_newton_step(E.Tangent(1, 8, 144, "panel", "cuda"), torch.zeros(1, 129, 129, device="cuda"), xc[:1], hc[:1], lam[:1])
    with pytest.raises(ValueError, match="contiguous"):
        E.gauss_newton_step(T, Gc.transpose(1, 2), xc, hc, lam)
    with pytest.raises(ValueError, match="contiguous"):
        E.gauss_newton_step(T, Gc, xc.t().contiguous().t(), hc, lam)
    with pytest.raises(ValueError, match="float32"):
        E.gauss_newton_step(T, Gc.double(), xc, hc, lam)
    with pytest.raises(ValueError, match="float32"):
        E.residual_sqnorm(xc.double(), hc)
    with pytest.raises(ValueError, match="float64"):
        E.gauss_newton_step(T, Gc, xc, hc, lam.float())
    with pytest.raises(ValueError, match="must agree"):
        E.residual_sqnorm(xc, hc[:, :7].contiguous())
    with pytest.raises(ValueError, match="must hold"):
        E.gauss_newton_step(T, Gc, xc[:, :7].contiguous(), hc[:, :7].contiguous(), lam)
    for cpu in ((T, Gc.cpu(), xc, hc, lam), (T, Gc, xc.cpu(), hc, lam), (T, Gc, xc, hc.cpu(), lam)):
        with pytest.raises(ValueError, match="GPU"):
            E.gauss_newton_step(*cpu)
    # B == 0: empties, no launch
    r = E.gauss_newton_step(E.Tangent(0, 8, 16, "panel", "cuda"), Gc[:0], xc[:0], hc[:0], lam[:0])
    assert r.grad.shape == (0, 3) and r.delta.shape == (0, 3) and r.stats.shape == (0, 4) and r.info.shape == (0,)
    r2, info = E.residual_sqnorm(xc[:0], hc[:0])
    assert r2.shape == (0,) and r2.dtype == torch.float64 and info.shape == (0,)


def test_kernel_timer_entries():
    from cmf_amd import engine as E
    J, G, x, xhat = GN.inputs(2, 8, 3)
    T, Gc, xc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(xhat).cuda()
    with E.timing(lambda name: True) as timer:
        E.gauss_newton_step(T, Gc, xc, hc, torch.zeros(2, dtype=torch.float64, device="cuda"))
        E.residual_sqnorm(xc, hc)
    by = timer.by_name()
    assert set(by) == {"gauss_newton_step", "residual_sqnorm"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------


def share(out):
    return R.tangential_share({k: out[k].cpu() for k in ("distance2", "tangential2")})


def run_project(dens, head, x, steps):
    """One ``project`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(dens, steps=steps)
    keep, marker = x.clone(), object()
    head.last_gram = marker
    out = proj.project(x)
    assert head.last_gram is marker and torch.equal(x, keep)
    B, d = x.shape[0], head.program.d
    assert out["latent"].shape == (B, d) and out["latent"].dtype == torch.float32 and out["gradient"].shape == (B, d)
    assert out["reconstruction_head"].shape == (B, *head.x_shape) and out["reconstruction"].shape == x.shape
    for key in ("distance2", "initial_distance2", "tangential2", "damping"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64
    for key in ("accepted", "info"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    assert bool((out["distance2"] <= out["initial_distance2"]).all()) and bool((out["accepted"] <= steps).all())
    assert bool((out["accepted"] >= 0).all())
    return proj, out


@pytest.mark.parametrize("name", SMOOTH + KINKED)
def test_projection_removes_the_tangential_residual(name):
    g, meta, dens, head, x = build(name)
    _, start = run_project(dens, head, x, 0)
    _, end = run_project(dens, head, x, 10)
    s0, s10 = share(start), share(end)
    need = 100.0 if name in SMOOTH else 10.0
    print(f"{name}: max tangential2 / distance2 {s0:.3e} -> {s10:.3e} (x {s0 / max(s10, 1e-300):.3g}, required x {need:g}); accepted "
          f"{end['accepted'].tolist()}; damping {end['damping'].tolist()}")
    assert bool((end["info"] == 0).all()) and bool((start["info"] == 0).all())
    assert s10 * need <= s0
    assert torch.equal(start["distance2"], start["initial_distance2"]) and torch.equal(start["initial_distance2"], end["initial_distance2"])
    assert bool((start["accepted"] == 0).all())
    # the encoder's distance is the reference's reconstruction-error, at the project's reconstruction tolerance
    with torch.no_grad():
        rec = dens.ood(x.clone())["reconstruction-error"].reshape(-1).double()
    rel = float((end["initial_distance2"] - rec).abs().max() / rec.abs().max())
    print(f"{name}: initial_distance2 against ood's reconstruction-error: rel {rel:.2e}")
    assert rel <= 1e-5
    with torch.no_grad():
        assert torch.equal(end["reconstruction_head"], head.flow_forward(end["latent"]))
    # mapped back to data space through the wrappers fixed_sample inverts (oracle.fixed_sample's tail, in float64)
    want = end["reconstruction_head"].cpu().double()
    for op in reversed(R.Model(name).pre):
        if op["kind"] == "logit":
            want = torch.sigmoid(want)
        elif op["kind"] == "scalar-add":
            want = want - op["value"]
        elif op["kind"] == "scalar-mult":
            want = want / op["value"]
    err = float((end["reconstruction"].cpu().double() - want).abs().max() / want.abs().max())
    print(f"{name}: reconstruction against the float64 inverse of the pre-head chain: rel {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("name", KNOWN_ANSWER)
def test_projection_finds_the_known_answer(name):
    """y = g(z_0) + eps n with n normal to range(J(z_0)), from the GPU's own decoder and Jacobian at the encoder's latent z_0 of the
    fixture's input; the normal is formed in float64 torch and rho^2 = ||float32(y) - x_on||^2 is recomputed exactly.  z_0 is
    stationary with distance rho up to the project's x_hat tolerance, so the projection must end within (1 + tau) of rho^2 for
    every sample, from a start that lies above (1 + 5 tau) rho^2 for the batch's worst sample (the reference's encoder is above it
    by 0.6 - 7 %, up to 4 % and 0.1 - 0.5 % on these fixtures; single samples of c2a_power start closer than 5 tau)."""
    import cmf_amd
    g, meta, dens, head, x = build(name)
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on, J = head.jacobian(z0)
    y64, _ = R.normal_offset(x_on.cpu(), J.cpu(), seed=0)
    y = y64.float()
    rho2 = ((y.double() - x_on.cpu().double()).flatten(1) ** 2).sum(1)
    out = cmf_amd.ManifoldProjector(head, steps=10).project(y.cuda().contiguous())
    excess0, excess = out["initial_distance2"].cpu() / rho2 - 1, out["distance2"].cpu() / rho2 - 1
    print(f"{name}: initial_distance2 / rho^2 - 1 in [{float(excess0.min()):.3e}, {float(excess0.max()):.3e}]; reached "
          f"distance2 / rho^2 - 1 in [{float(excess.min()):.3e}, {float(excess.max()):.3e}] (tau {TAU:g}); accepted {out['accepted'].tolist()}")
    assert bool((out["distance2"].cpu() <= rho2 * (1 + TAU)).all())
    assert float(excess0.max()) > 5 * TAU
    assert bool((out["distance2"] <= out["initial_distance2"]).all()) and bool((out["info"] == 0).all())


def test_zero_residual_is_a_result():
    """c1_sphere has D = d: every input is on the manifold, the residual is rounding."""
    g, meta, dens, head, x = build("c1_sphere")
    assert int(np.prod(head.x_shape)) == head.program.d
    for steps in (0, 3):
        _, out = run_project(dens, head, x, steps)
        assert bool((out["info"] == 0).all())
        assert all(bool(torch.isfinite(out[k]).all()) for k in out if out[k].is_floating_point())
        # the project's x_hat tolerance: ||x_hat - y|| <= 1e-5 ||x_hat|| for a point of the manifold
        scale = (out["reconstruction_head"].double().flatten(1) ** 2).sum(1)
        assert bool((out["distance2"] <= 1e-10 * scale).all())
    # an exactly zero residual: g = delta = 0, info 0, no division by the distance anywhere
    from cmf_amd import engine as E
    J, G, xx, _ = GN.inputs(2, 3, 3)
    grad, delta, stats, info, r2, info_r = run(J, G, xx, xx, np.zeros(2))
    assert (info == 0).all() and (grad == 0).all() and (delta == 0).all() and (stats == 0).all() and (r2 == 0).all()


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_rows_of_one_call(name, monkeypatch):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    x = x[:3].contiguous()
    _, whole0 = run_project(dens, head, x, 0)
    _, whole = run_project(dens, head, x, 10)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    _, pieces0 = run_project(dens, head, x, 0)
    _, pieces = run_project(dens, head, x, 10)
    need = 100.0 if name in SMOOTH else 10.0
    d0 = whole["initial_distance2"]
    print(f"{name}: pieces against whole: bit-equal latent {torch.equal(pieces['latent'], whole['latent'])}, distance2 rel "
          f"{float(((pieces['distance2'] - whole['distance2']).abs() / d0).max()):.2e}")
    assert float(((pieces["initial_distance2"] - d0).abs() / d0).max()) <= 1e-5
    assert float(((pieces["distance2"] - whole["distance2"]).abs() / d0).max()) <= 1e-5
    assert share(pieces) * need <= share(pieces0) and share(whole) * need <= share(whole0)
    assert bool((pieces["info"] == 0).all())


def test_the_log_density_path_is_untouched():
    import cmf_amd
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    with torch.no_grad():
        before = cmf_amd.MetricStatistics(dens)
        macs_before = before.update(x)
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        cmf_amd.ManifoldProjector(dens, steps=3).project(x)
        after = cmf_amd.MetricStatistics(dens)
        macs_after = after.update(x)
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert torch.equal(before.state.flat, after.state.flat) and torch.equal(macs_before, macs_after)
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
