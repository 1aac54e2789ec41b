"""The recovery of linear inverse problems on the GPU: the operator kernel (csrc/operator_apply.hip) against float64
numpy on the same float32 inputs, its output contract -- columns stay apart, an identity or permutation operator is exact --,
isolation, determinism and refusals, and ``cmf_amd.ManifoldProjector.recover`` end to end on the reference-generated fixtures under
the conditions tests/test_recovery_host.py establishes on the float64 reference loop.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds, per sample and element:
    |K - K64| <= C_OPERATOR (|a| |J|)                                       tests/_operator_apply_emulation.py, from the emulation
    |yhat - yhat64| <= 2^-24 |yhat64| + (D + 2) 2^-53 sum_i |a_mi| |xhat_i|  one float32 rounding of a float64 sum of exact products
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN."""
import math

import numpy as np
import pytest
import torch

import _gn_step_emulation as GN
import _operator_apply_emulation as OA
import _recovery_reference as RR
from test_gpu_metric_stats import build
from test_gpu_projection import TAU, guarded, guards_intact, same_bits, stack

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUTS = ["panel", "fmajor"]


def run(a, J, xhat, layout):
    """``engine.operator_apply`` and ``engine.operator_image`` on CPU inputs -> numpy (K (B, M, nc), yhat (B, M), image (B, M))."""
    from cmf_amd import engine as E
    T = stack(J, layout)
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    K, yhat = E.operator_apply(T, ac, hc)
    image = E.operator_image(ac, hc)
    torch.cuda.synchronize()
    assert isinstance(K, E.Tangent) and (K.B, K.N, K.nc, K.layout) == (T.B, a.shape[0], T.nc, layout)
    return K.to_dense(K.nc).contiguous().cpu().numpy(), yhat.cpu().numpy(), image.cpu().numpy()


# --------------------------------------------------------------------------------------------------
# the kernel
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,D,d", OA.SHAPES)
def test_kernel_matches_float64(M, D, d, layout):
    a, J, xhat = OA.inputs(M, D, d)
    K, yhat, image = run(a, J, xhat, layout)
    worst = 0.0
    for b in range(OA.BATCH):
        K64, S = OA.apply64(a, J[b])
        r = OA.ratio(K[b, :, :d], K64, S)
        worst = max(worst, r)
        assert r <= OA.C_OPERATOR, f"sample {b}"
    assert np.isnan(K[:, :, d:]).all()                               # what the padding columns held stays in the padding columns
    y64, S = OA.image64(a, xhat)
    err = np.abs(yhat.astype(np.float64) - y64)
    print(f"M={M} D={D} d={d} {layout}: worst |K - K64| / (|a| |J|) = 2^{math.log2(max(worst, 1e-300)):.2f} (bound "
          f"2^{math.log2(OA.C_OPERATOR):g}); worst |yhat - yhat64| / bound = {float((err / OA.image_bound(y64, S, D)).max()):.3f}")
    assert (err <= OA.image_bound(y64, S, D)).all()
    assert same_bits(image, yhat)                                    # the image-only mode: the same bits


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D,d", [(64, 17), (784, 64)])
def test_identity_and_permutation_operators_are_exact(D, d, layout):
    """Adding exact zeros in fp32 changes nothing (``==`` treats +-0 alike): K is J and yhat is xhat, row for row."""
    J, _, _, xhat = GN.inputs(3, D, d, seed=6)
    eye = np.eye(D, dtype=np.float32)
    K, yhat, image = run(eye, J, xhat, layout)
    assert torch.equal(torch.as_tensor(K[:, :, :d]), torch.as_tensor(J)) and torch.equal(torch.as_tensor(yhat), torch.as_tensor(xhat))
    perm = np.random.default_rng(D + d).permutation(D)
    K, yhat, image = run(np.ascontiguousarray(eye[perm]), J, xhat, layout)
    assert torch.equal(torch.as_tensor(K[:, :, :d]), torch.as_tensor(J[:, perm])) and torch.equal(torch.as_tensor(yhat),
                                                                                                   torch.as_tensor(xhat[:, perm]))
    assert same_bits(image, yhat)


@pytest.mark.parametrize("B,M,D,d,layout", [(3, 17, 64, 17, "panel"), (2, 196, 784, 100, "fmajor"), (3, 1, 5, 3, "panel"),
                                            (2, 33, 1100, 33, "fmajor"), (2, 260, 64, 128, "panel")])
def test_outputs_stay_inside_their_buffers(B, M, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    a, J, xhat = OA.inputs(M, D, d, B=B, seed=2)
    T = stack(J, layout)
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    bufs = {"k": guarded((B * M * T.nc,), torch.float32), "yhat": guarded((B, M), torch.float32), "image": guarded((B, M), torch.float32)}
    K = E.Tangent(B, M, T.nc, layout, "cuda", data=bufs["k"][1])
    p = lambda name: E._p(bufs[name][1])
    lib = _lib.load()
    _lib.check(lib.cmf_operator_apply(E._p(ac), M, D, E._p(T.data), T.t_b, T.t_r, T.nc, B, E._p(hc), p("k"), K.t_b, K.t_r, p("yhat"),
                                      E._stream()), "cmf_operator_apply")
    _lib.check(lib.cmf_operator_apply(E._p(ac), M, D, None, 0, 0, 0, B, E._p(hc), None, 0, 0, p("image"), E._stream()),
               "cmf_operator_apply")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    want_k, want_y, want_i = run(a, J, xhat, layout)
    assert same_bits(K.to_dense(K.nc).contiguous().cpu().numpy(), want_k)      # every element of k is written
    assert same_bits(bufs["yhat"][1].cpu().numpy(), want_y) and same_bits(bufs["image"][1].cpu().numpy(), want_i)


@pytest.mark.parametrize("M,D,d,layout", [(17, 64, 17, "panel"), (196, 784, 100, "panel"), (17, 64, 17, "fmajor"), (300, 1100, 33, "fmajor")])
def test_position_independence_and_repeatability(M, D, d, layout):
    """(300, 1100, 33): two row groups of a, and D no multiple of the slab depth."""
    a, J, xhat = OA.inputs(M, D, d, B=5, seed=3)
    batch, again = run(a, J, xhat, layout), run(a, J, xhat, layout)
    for x, y in zip(batch, again):
        assert same_bits(x, y)
    for b in range(5):
        alone = run(a, J[b:b + 1], xhat[b:b + 1], layout)
        for x, y in zip(alone, batch):
            assert same_bits(x[0], y[b]), f"sample {b}"
    where = [4, 0, 2, 2, 1, 3, 0]
    for x, y in zip(run(a, J[where], xhat[where], layout), batch):
        assert same_bits(x, y[where])


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, M, D, d = 2, 5, 8, 3
    a, J, xhat = OA.inputs(M, D, d, B=B)
    T = stack(J, "panel")
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    k, yhat = torch.zeros(B * M * T.nc + 4, device="cuda"), torch.zeros(B * M, device="cuda")
    ok = [E._p(ac), M, D, E._p(T.data), T.t_b, T.t_r, T.nc, B, E._p(hc), E._p(k), M * T.nc, T.nc, E._p(yhat)]
    assert lib.cmf_operator_apply(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(yhat.abs().sum()) > 0 and bool(torch.isnan(k).any())
    k.zero_()
    yhat.zero_()
    bad = [(0, None), (1, 0), (2, 0), (4, T.t_b + 2), (5, T.t_r + 2), (5, 8), (4, 8), (6, 24), (6, 0), (7, 0), (8, None), (9, None),
           (10, M * T.nc + 2), (11, T.nc + 2), (11, 8), (10, 8), (12, None), (3, E._p(T.data[1:])), (9, E._p(k[1:]))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_operator_apply(*args, E._stream()) == -1, (i, value)
    # wider than the sweep can produce: nc = 528 with strides that would hold it (refused before anything is read)
    wide = [E._p(ac), M, D, E._p(T.data), D * 528, 528, 528, B, E._p(hc), E._p(k), M * 528, 528, E._p(yhat)]
    assert lib.cmf_operator_apply(*wide, E._stream()) == -1
    # image-only mode: a, xhat and yhat are still required
    image = [E._p(ac), M, D, None, 0, 0, 0, B, E._p(hc), None, 0, 0, E._p(yhat)]
    for i, value in ((0, None), (1, 0), (2, 0), (7, 0), (8, None), (12, None)):
        args = list(image)
        args[i] = value
        assert lib.cmf_operator_apply(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert float(k.abs().sum()) == 0.0 and float(yhat.abs().sum()) == 0.0


def test_engine_refusals():
    from cmf_amd import engine as E
    a, J, xhat = OA.inputs(5, 8, 3, B=2)
    T, ac, hc = stack(J, "panel"), torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    with pytest.raises(ValueError, match="engine.Tangent"):
        E.operator_apply(T.data, ac, hc)
    with pytest.raises(ValueError, match="float32"):
        E.operator_apply(T, ac.double(), hc)
    with pytest.raises(ValueError, match="float32"):
        E.operator_image(ac, hc.double())
    with pytest.raises(ValueError, match="not contiguous"):
        E.operator_apply(T, torch.as_tensor(a).cuda().t().contiguous().t(), hc)
    with pytest.raises(ValueError, match="not contiguous"):
        E.operator_image(ac, hc.t().contiguous().t())
    with pytest.raises(ValueError, match=r"contiguous \(M, D\)"):
        E.operator_image(ac[0], hc)
    with pytest.raises(ValueError, match="8 elements per sample"):
        E.operator_image(ac, hc[:, :7].contiguous())
    with pytest.raises(ValueError, match="8 elements per sample"):
        E.operator_apply(T, ac, hc[:, :7].contiguous())
    with pytest.raises(ValueError, match="must hold"):
        E.operator_apply(T, ac, hc[:1].contiguous())
    with pytest.raises(ValueError, match="must hold"):
        E.operator_apply(E.Tangent(2, 7, 16, "panel", "cuda"), ac, hc)
    with pytest.raises(ValueError, match="must hold"):
        E.operator_apply(E.Tangent(2, 8, 528, "panel", "cuda"), ac, hc)
    for cpu in ((T, ac.cpu(), hc), (T, ac, hc.cpu())):
        with pytest.raises(ValueError, match="GPU"):
            E.operator_apply(*cpu)
        with pytest.raises(ValueError, match="GPU"):
            E.operator_image(*cpu[1:])
    # B == 0: empties, no launch
    K, yhat = E.operator_apply(E.Tangent(0, 8, 16, "panel", "cuda"), ac, hc[:0])
    assert (K.B, K.N, K.nc, K.layout) == (0, 5, 16, "panel") and yhat.shape == (0, 5) and yhat.dtype == torch.float32
    assert E.operator_image(ac, hc[:0]).shape == (0, 5)


def test_kernel_timer_entries():
    from cmf_amd import engine as E
    a, J, xhat = OA.inputs(5, 8, 3, B=2)
    T, ac, hc = stack(J, "panel"), torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    with E.timing(lambda name: True) as timer:
        E.operator_apply(T, ac, hc)
        E.operator_image(ac, hc)
    by = timer.by_name()
    assert set(by) == {"operator_apply", "operator_image"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())
    assert by["operator_image"][3] < by["operator_apply"][3]


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------

KEYS = {"latent", "reconstruction_head", "reconstruction", "measurement", "cost", "initial_cost", "tangential2", "gradient", "accepted",
        "damping", "info"}


def run_recover(dens, head, y, A, steps, **start):
    """One ``recover`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(dens, steps=steps)
    keep = [None if v is None else v.clone() for v in (y, A, start.get("init"), start.get("x_init"))]
    marker = object()
    head.last_gram = marker
    out = proj.recover(y, A, **start)
    assert head.last_gram is marker
    for v, k in zip((y, A, start.get("init"), start.get("x_init")), keep):
        assert v is None or torch.equal(v, k)
    B, M, d = y.shape[0], A.shape[0], head.program.d
    assert set(out) == KEYS
    assert out["latent"].shape == (B, d) and out["latent"].dtype == torch.float32 and out["gradient"].shape == (B, d)
    assert out["reconstruction_head"].shape == (B, *head.x_shape) and out["reconstruction"].shape[0] == B
    assert out["measurement"].shape == (B, M) and out["measurement"].dtype == torch.float32
    for key in ("cost", "initial_cost", "tangential2", "damping"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64
    for key in ("accepted", "info"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["accepted"] <= steps).all())
    assert bool((out["accepted"] >= 0).all())
    return proj, out


def known_answer_problem(name, head, dens, x, M=None):
    """(x_on, A, y, x_start) on the GPU: x_on the GPU's own g(z_0) at the encoder's latent of the fixture's input, the seeded Gaussian
    operator, y = A x_on formed in float64 on the host, and the perturbed input the recovery starts from."""
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on = head.flow_forward(z0)
    A = RR.gaussian_operator(RR.KNOWN_ANSWER[name] if M is None else M, x_on[0].numel())
    y = RR.measure(A, x_on).float()
    return x_on, A.cuda().contiguous(), y.cuda().contiguous(), RR.start_input(x_on).cuda().contiguous()


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_recovery_finds_the_known_answer(name):
    """y = A g(z_0): z_0 is a minimiser with cost 0, and ten steps from the encoder's latent of x_on + 0.1 ||x_on|| / sqrt(D) randn must
    reconstruct x_on over all D elements within the tolerance tests/test_recovery_host.py derives from the project's x_hat
    tolerance (RR.E2E_TOL), for every sample."""
    g, meta, dens, head, x = build(name)
    x_on, A, y, x_start = known_answer_problem(name, head, dens, x)
    _, out = run_recover(head, head, y, A, 10, x_init=x_start)
    rel = RR.rel_distance(out["reconstruction_head"], x_on)
    start = RR.rel_distance(x_start, x_on)
    print(f"{name}: M = {A.shape[0]}: ||g(z) - x_on|| / ||x_on|| <= {float(rel.max()):.3e} (tolerance {RR.E2E_TOL[name]:.3e}; the start "
          f"is off by {float(start.min()):.3e} .. {float(start.max()):.3e}); cost {float(out['initial_cost'].max()):.3e} -> "
          f"{float(out['cost'].max()):.3e}; accepted {out['accepted'].tolist()}")
    assert bool((rel <= RR.E2E_TOL[name]).all())
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["info"] == 0).all())
    with torch.no_grad():
        assert torch.equal(out["reconstruction_head"], head.flow_forward(out["latent"]))
    from cmf_amd import engine as E
    assert torch.equal(out["measurement"], E.operator_image(A, out["reconstruction_head"]))
    assert torch.equal(out["cost"], E.residual_sqnorm(y, out["measurement"])[0])


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass", "c1_sphere_d2"])
def test_identity_operator_reaches_project(name):
    """K is J and yhat is x_hat in the same layout, and the downstream kernels are the same: bit for bit ``project``."""
    import cmf_amd
    g, meta, dens, head, x = build(name)
    proj = cmf_amd.ManifoldProjector(dens, steps=10)
    hx = proj.head_input(x)
    assert torch.equal(hx, proj.head_input_and_latent(x)[0])
    D = hx[0].numel()
    eye = torch.eye(D, device="cuda")
    _, out = run_recover(dens, head, hx.flatten(1).contiguous(), eye, 10, x_init=x)
    ref = proj.project(x)
    print(f"{name}: accepted {out['accepted'].tolist()} against {ref['accepted'].tolist()}")
    assert torch.equal(out["cost"], ref["distance2"]) and torch.equal(out["initial_cost"], ref["initial_distance2"])
    for key in ("latent", "accepted", "damping", "gradient", "info", "reconstruction_head", "reconstruction"):
        assert torch.equal(out[key], ref[key]), key
    assert same_bits(out["tangential2"].cpu().numpy(), ref["tangential2"].cpu().numpy())
    assert torch.equal(out["measurement"], out["reconstruction_head"].flatten(1))


@pytest.mark.parametrize("name", RR.SELECTION)
def test_selection_operator_reaches_complete(name):
    """The rows of the identity for a seeded half of the elements against ``complete`` with the matching 0/1 weights, on the fixture's
    own input, both from the encoder's latent (the fixtures tests/test_recovery_host.py qualifies)."""
    import cmf_amd
    g, meta, dens, head, x = build(name)
    proj = cmf_amd.ManifoldProjector(dens, steps=10)
    hx = proj.head_input(x)
    A, w = RR.selection(hx[0].numel())
    A = A.cuda().contiguous()
    y = hx.flatten(1)[:, w.bool().cuda()].contiguous()               # the selected elements, exactly
    assert torch.equal(y.double(), hx.flatten(1).double() @ A.double().t())
    _, out = run_recover(dens, head, y, A, 10, x_init=x)
    ref = proj.complete(x, w.view(x.shape[1:]).cuda())
    rel = ((out["cost"] - ref["cost"]).abs() / ref["cost"]).cpu()
    print(f"{name}: |cost - complete's| / complete's <= {float(rel.max()):.3e} (tau {TAU:g}); accepted {out['accepted'].tolist()} "
          f"against {ref['accepted'].tolist()}")
    assert bool((rel <= TAU).all()) and bool((out["info"] == 0).all())


def test_underdetermined_problem_is_a_result():
    """M = 5 < d = 10: every damped step is solvable and the cost falls; the closing evaluation at lambda = 0 meets a singular
    K^T K and says so."""
    name, M = RR.UNDERDETERMINED
    g, meta, dens, head, x = build(name)
    x_on, A, y, x_start = known_answer_problem(name, head, dens, x, M=M)
    assert M < head.program.d
    _, out = run_recover(head, head, y, A, 10, x_init=x_start)
    print(f"{name}: M = {M}: accepted {out['accepted'].tolist()}; cost {float(out['initial_cost'].max()):.3e} -> "
          f"{float(out['cost'].max()):.3e}; info {out['info'].tolist()}")
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["accepted"] >= 1).all())
    assert bool((out["info"] == 1).all()) and bool(torch.isnan(out["tangential2"]).all())
    assert bool(torch.isfinite(out["latent"]).all()) and bool(torch.isfinite(out["gradient"]).all())


def test_init_x_init_and_the_default_start_are_honoured():
    name = "c2b_hepmass"
    g, meta, dens, head, x = build(name)
    x_on, A, y, x_start = known_answer_problem(name, head, dens, x)
    with torch.no_grad():
        z_enc = head.extract_latent(x_start.clone(), earliest_latent=False)
    init = (z_enc + 0.05).contiguous()
    _, at_init = run_recover(head, head, y, A, 0, init=init)
    _, at_enc = run_recover(head, head, y, A, 0, x_init=x_start)
    _, at_zero = run_recover(head, head, y, A, 0)
    assert torch.equal(at_init["latent"], init) and torch.equal(at_enc["latent"], z_enc)
    assert torch.equal(at_zero["latent"], torch.zeros_like(z_enc))
    for out in (at_init, at_enc, at_zero):
        assert torch.equal(out["cost"], out["initial_cost"]) and bool((out["accepted"] == 0).all())
    assert not torch.equal(at_init["cost"], at_enc["cost"]) and not torch.equal(at_zero["cost"], at_enc["cost"])
    with torch.no_grad():
        assert torch.equal(at_init["reconstruction_head"], head.flow_forward(init))
    with pytest.raises(ValueError, match="not both"):
        run_recover(head, head, y, A, 0, init=init, x_init=x_start)
    _, moved = run_recover(head, head, y, A, 10, init=init)
    assert bool((moved["cost"] <= at_init["cost"]).all()) and bool((moved["accepted"] > 0).any())


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_rows_of_one_call(name, monkeypatch):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    x_on, A, y, x_start = known_answer_problem(name, head, dens, x[:3].contiguous())
    _, whole = run_recover(head, head, y, A, 10, x_init=x_start)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    _, pieces = run_recover(head, head, y, A, 10, x_init=x_start)
    c0 = whole["initial_cost"]
    print(f"{name}: pieces against whole: bit-equal latent {torch.equal(pieces['latent'], whole['latent'])}, cost / initial cost "
          f"{float((pieces['cost'] / c0).max()):.2e} against {float((whole['cost'] / c0).max()):.2e}")
    assert float(((pieces["initial_cost"] - c0).abs() / c0).max()) <= 1e-5
    assert float(((pieces["cost"] - whole["cost"]).abs() / c0).max()) <= 1e-5
    assert bool((RR.rel_distance(pieces["reconstruction_head"], x_on) <= RR.E2E_TOL[name]).all())
    assert bool((pieces["info"] == 0).all()) and bool((whole["info"] == 0).all())


def test_the_log_density_path_is_untouched():
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        x_on, A, y, x_start = known_answer_problem("mini_mnist", head, dens, x)
        _, out = run_recover(head, head, y, A, 3, x_init=x_start)
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
    assert bool((out["info"] == 0).all())
