"""The robust projection on the GPU: the robust weights kernel (csrc/robust_weights.hip) against its float64 numpy
model (tests/_robust_weights_emulation.py: the bounds are derived there), its contract -- elements with prior == 0 are never read,
the cost-only mode, isolation, determinism, refusals --, and ``cmf_amd.ManifoldProjector.robust`` end to end on the
reference-generated fixtures under the conditions tests/test_robust_host.py establishes on the float64 reference loop.  Needs an
MI355X: run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import _completion_reference as CR
import _projection_reference as R
import _robust_reference as RR
import _robust_weights_emulation as RW
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
LOSSES = ("huber", "tukey")


def cuda(v):
    return None if v is None else torch.as_tensor(v).cuda()


def run(x, xhat, prior, loss, c, scale=None, weights_out=True):
    """``engine.robust_weights`` on CPU inputs -> numpy (w or None, stats, info)."""
    from cmf_amd import engine as E
    r = E.robust_weights(cuda(x), cuda(xhat), loss, c, prior=cuda(prior), scale=cuda(scale), weights_out=weights_out)
    torch.cuda.synchronize()
    assert all(same_bits(v.cpu().numpy(), r.stats[:, k].cpu().numpy()) for k, v in enumerate((r.scale, r.cost, r.used, r.effective)))
    return None if r.w is None else r.w.cpu().numpy(), r.stats.cpu().numpy(), r.info.cpu().numpy()


@pytest.mark.parametrize("prior_kind", RW.PRIORS)
@pytest.mark.parametrize("n", RW.SIZES)
def test_kernel_matches_the_float64_model(n, prior_kind):
    x, xhat, prior, scale, kinds = RW.inputs(n, prior_kind)
    seen = set()
    for loss in LOSSES:
        c = RW.TUNING[loss]
        for given in (None, scale):
            got = run(x, xhat, prior, loss, c, given)
            ref = RW.batch(x, xhat, prior, loss, c, given)
            assert RW.mismatches(got, ref, prior) == [], (loss, given is not None, kinds)
            seen |= set(ref[2].tolist())
            if loss == "huber":                                       # clearly inside c: the weight is the prior's own bits
                w, (_, stats, info, _) = got[0], ref
                for b in np.nonzero(info == 0)[0]:
                    u = (x[b].astype(np.float64) - xhat[b].astype(np.float64)) / stats[b, 0]
                    p = np.ones(n, dtype=np.float32) if prior is None else prior[b]
                    inside = (np.abs(u) <= c * (1 - 1e-9)) & (p > 0)
                    assert same_bits(w[b][inside], p[inside]), (b, kinds[b])
    print(f"n={n} prior={prior_kind}: info codes seen {sorted(seen)}")
    if prior_kind != "third":                                         # the zero medians / the samples without a used element
        assert seen == {0, 3}


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n", [3, 257, 1100])
def test_zero_prior_elements_are_not_read(n, loss):
    x, xhat, prior, scale, _ = RW.inputs(n, "third", seed=4)
    dead = prior == 0
    xn, hn = x.copy(), xhat.copy()
    xn[dead], hn[dead] = NAN, NAN
    xo, ho = x.copy(), xhat.copy()
    xo[dead], ho[dead] = 3.0e30, -1.0e30
    for given in (None, scale):
        base, poisoned, other = (run(a, h, prior, loss, RW.TUNING[loss], given) for a, h in ((x, xhat), (xn, hn), (xo, ho)))
        for a, b, c in zip(base, poisoned, other):
            assert same_bits(a, b) and same_bits(b, c)
        assert set(base[2].tolist()) <= {0, 3} and (base[2] == 0).any()
        for b in np.nonzero(base[2] == 0)[0]:
            assert np.isfinite(base[0][b]).all() and (base[0][b][dead[b]].view(np.int32) == 0).all()


@pytest.mark.parametrize("n,prior_kind", [(1, "none"), (255, "third"), (784, "positive"), (1100, "none")])
def test_outputs_stay_inside_their_buffers_and_the_cost_only_mode(n, prior_kind):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    x, xhat, prior, scale, _ = RW.inputs(n, prior_kind, seed=2)
    B = len(x)
    xc, hc, pc, sc = cuda(x), cuda(xhat), cuda(prior), cuda(scale)
    lib = _lib.load()
    for loss in (0, 1):
        c = RW.TUNING[LOSSES[loss]]
        for given in (None, sc):
            bufs = {"w": guarded((B, n), torch.float32), "stats": guarded((B, 4), torch.float64), "info": guarded((B,), torch.int32),
                    "stats_c": guarded((B, 4), torch.float64), "info_c": guarded((B,), torch.int32)}
            p = lambda name: E._p(bufs[name][1])
            _lib.check(lib.cmf_robust_weights(E._p(xc), E._p(hc), E._p(pc), n, B, loss, c, E._p(given), p("w"), p("stats"), p("info"),
                                              E._stream()), "robust weights")
            _lib.check(lib.cmf_robust_weights(E._p(xc), E._p(hc), E._p(pc), n, B, loss, c, E._p(given), None, p("stats_c"),
                                              p("info_c"), E._stream()), "robust weights")
            torch.cuda.synchronize()
            for buf, _, fill in bufs.values():
                assert guards_intact(buf, fill)
            got = lambda name: bufs[name][1].cpu().numpy()
            w, stats, info = run(x, xhat, prior, LOSSES[loss], c, None if given is None else scale)
            assert same_bits(got("w"), w) and same_bits(got("stats"), stats) and (got("info") == info).all()
            assert same_bits(got("stats_c"), stats) and (got("info_c") == info).all()      # the cost-only mode: the same bits
            _, stats_e, info_e = run(x, xhat, prior, LOSSES[loss], c, None if given is None else scale, weights_out=False)
            assert same_bits(stats_e, stats) and (info_e == info).all()


@pytest.mark.parametrize("n,prior_kind", [(64, "positive"), (784, "third"), (1100, "none")])
def test_position_independence_and_repeatability(n, prior_kind):
    x, xhat, prior, scale, _ = RW.inputs(n, prior_kind, seed=3, B=6)
    where = [0, 1, 2, 2, 4, 3, 1, 5, 0, 0, 3]
    pick = lambda v: None if v is None else v[where]
    for loss in LOSSES:
        for given in (None, scale):
            base = run(x, xhat, prior, loss, RW.TUNING[loss], given)
            batch = run(x[where], xhat[where], pick(prior), loss, RW.TUNING[loss], pick(given))
            again = run(x[where], xhat[where], pick(prior), loss, RW.TUNING[loss], pick(given))
            for a, b, c in zip(base, batch, again):
                assert same_bits(a[where], b) and same_bits(b, c)


@pytest.mark.parametrize("loss", LOSSES)
def test_failures_are_reported_and_confined(loss):
    n, c = 64, RW.TUNING[loss]
    gen = np.random.default_rng(1)
    x, xhat = gen.standard_normal((9, n)).astype(np.float32), gen.standard_normal((9, n)).astype(np.float32)
    prior = np.ones((9, n), dtype=np.float32)
    prior[:, ::3] = 0.0                                              # elements 0, 3, 6, ... are unused
    prior[:, 1::3] = 2.5
    clean = run(x, xhat, prior, loss, c)
    assert (clean[2] == 0).all()
    prior[1, 4] = -1.0
    prior[2, 5] = NAN
    x[3, 7] = np.inf                                                 # a used element
    x[4, 3], xhat[4, 6] = NAN, np.inf                                # unused elements: not an error
    prior[5] = 0.0                                                   # m = 0: the median of nothing
    x[6, : n // 2 + 12] = xhat[6, : n // 2 + 12]                     # more than half of the used residuals exactly zero
    xhat[7, 1] = NAN                                                 # a used element
    w, stats, info = run(x, xhat, prior, loss, c)
    assert info.tolist() == [0, 2, 2, 2, 0, 3, 3, 2, 0]
    for b in (1, 2, 3, 7):
        assert np.isnan(w[b]).all() and np.isnan(stats[b]).all()
    assert np.isnan(w[[5, 6]]).all() and np.isnan(stats[[5, 6], 1:]).all() and np.isnan(stats[5, 0]) and stats[6, 0] == 0.0
    for got, want in zip((w, stats), clean):
        assert same_bits(got[[0, 4, 8]], want[[0, 4, 8]])
    assert RW.mismatches((w, stats, info), RW.batch(x, xhat, prior, loss, c), prior) == []
    prior[1, 4] = np.inf                                             # a prior that is not finite
    assert run(x, xhat, prior, loss, c)[2].tolist() == [0, 2, 2, 2, 0, 3, 3, 2, 0]
    # a given scale: zero, negative, NaN and infinite ones are info 3 and keep their slot; the zero median is then no obstacle, and
    # a sample with no used element has nothing to weigh -- zero cost, info 0
    scale = np.array([0.7, 0.7, 0.7, 0.7, 0.0, 0.7, 0.7, 0.7, 0.7])
    scale2 = np.array([-1.0, 0.7, 0.7, 0.7, NAN, 0.7, 0.7, 0.7, np.inf])
    w, stats, info = run(x, xhat, prior, loss, c, scale)
    assert info.tolist() == [0, 2, 2, 2, 3, 0, 0, 2, 0] and stats[4, 0] == 0.0 and np.isnan(stats[4, 1:]).all() and np.isnan(w[4]).all()
    assert (w[5] == 0).all() and stats[5].tolist() == [0.7, 0.0, 0.0, 0.0]
    assert RW.mismatches((w, stats, info), RW.batch(x, xhat, prior, loss, c, scale), prior) == []
    w2, stats2, info2 = run(x, xhat, prior, loss, c, scale2)
    assert info2.tolist() == [3, 2, 2, 2, 3, 0, 0, 2, 3] and stats2[0, 0] == -1.0 and np.isnan(stats2[4, 0]) and np.isinf(stats2[8, 0])
    assert same_bits(w2[[5, 6]], w[[5, 6]]) and same_bits(stats2[[5, 6]], stats[[5, 6]])


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, n = 2, 8
    x, xhat, prior, scale, _ = RW.inputs(n, "positive", B=B)
    xc, hc, pc, sc = cuda(x), cuda(xhat), cuda(prior), cuda(scale)
    w = torch.zeros(B * n, device="cuda")
    stats, info = torch.zeros(B * 4 + 1, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    odd = stats.view(torch.float32)[1:]                             # 4 bytes past an 8-byte boundary
    ok = [E._p(xc), E._p(hc), E._p(pc), n, B, 0, 1.345, E._p(sc), E._p(w), E._p(stats), E._p(info)]
    assert lib.cmf_robust_weights(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(w.abs().sum()) > 0 and float(stats.abs().sum()) > 0
    for t in (w, stats, info):
        t.zero_()
    bad = [(0, None), (1, None), (3, 0), (3, -1), (4, 0), (5, 2), (5, -1), (6, 0.0), (6, -1.0), (6, NAN), (9, None), (10, None),
           (7, E._p(odd)), (9, E._p(odd))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_robust_weights(*args, E._stream()) == -1, (i, value)
    for optional in (2, 7, 8):                                      # prior, scale_in and w may be NULL
        args = list(ok)
        args[optional] = None
        if optional != 8:
            args[8] = None                                          # ... and this accepted launch writes no w
        assert lib.cmf_robust_weights(*args, E._stream()) == 0
        stats.zero_()
        info.zero_()
    torch.cuda.synchronize()
    assert float(w.abs().sum()) == 0.0


def test_engine_refusals_and_the_empty_batch():
    from cmf_amd import engine as E
    x, xhat, prior, scale, _ = RW.inputs(8, "positive", B=2)
    xc, hc, pc, sc = cuda(x), cuda(xhat), cuda(prior), cuda(scale)
    with pytest.raises(ValueError, match="loss must be"):
        E.robust_weights(xc, hc, "cauchy", 1.0)
    for tuning in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="tuning must be > 0"):
            E.robust_weights(xc, hc, "huber", tuning)
    with pytest.raises(ValueError, match="contiguous"):
        E.robust_weights(xc.t().contiguous().t(), hc, "huber", 1.0)
    with pytest.raises(ValueError, match="must agree"):
        E.robust_weights(xc, hc[:, :7].contiguous(), "huber", 1.0)
    with pytest.raises(ValueError, match="float32"):
        E.robust_weights(xc.double(), hc, "huber", 1.0)
    with pytest.raises(ValueError, match="prior must be float32"):
        E.robust_weights(xc, hc, "huber", 1.0, prior=pc > 1)
    with pytest.raises(ValueError, match="prior must be a contiguous"):
        E.robust_weights(xc, hc, "huber", 1.0, prior=pc[:1].contiguous())
    with pytest.raises(ValueError, match="scale must be float64"):
        E.robust_weights(xc, hc, "huber", 1.0, scale=sc.float())
    with pytest.raises(ValueError, match="scale must be a contiguous"):
        E.robust_weights(xc, hc, "huber", 1.0, scale=sc[:1])
    for cpu in ((xc.cpu(), hc, None, None), (xc, hc.cpu(), None, None), (xc, hc, pc.cpu(), None), (xc, hc, None, sc.cpu())):
        with pytest.raises(ValueError, match="GPU"):
            E.robust_weights(cpu[0], cpu[1], "huber", 1.0, prior=cpu[2], scale=cpu[3])
    r = E.robust_weights(xc[:0], hc[:0], "tukey", 4.685, prior=pc[:0], scale=sc[:0])
    assert r.w.shape == (0, 8) and r.info.shape == (0,) and r.info.dtype == torch.int32
    assert all(v.shape == (0,) and v.dtype == torch.float64 for v in (r.scale, r.cost, r.used, r.effective))
    assert E.robust_weights(xc[:0], hc[:0], "huber", 1.0, weights_out=False).w is None


def test_kernel_timer_entry():
    from cmf_amd import engine as E
    x, xhat, prior, scale, _ = RW.inputs(64, "third", B=3)
    xc, hc, pc, sc = cuda(x), cuda(xhat), cuda(prior), cuda(scale)
    with E.timing(lambda name: True) as timer:
        E.robust_weights(xc, hc, "huber", 1.345, prior=pc)
    by = timer.by_name()
    assert set(by) == {"robust_weights"}
    n_launch, ms, flops, nbytes = by["robust_weights"]
    assert n_launch == 1 and ms >= 0 and flops > 0 and nbytes > 0
    with E.timing(lambda name: True) as held:                         # a given scale runs no select passes: fewer bytes
        E.robust_weights(xc, hc, "huber", 1.345, prior=pc, scale=sc)
    assert held.by_name()["robust_weights"][3] < nbytes


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------

KEYS = {"latent", "reconstruction_head", "reconstruction", "cost", "initial_cost", "tangential2", "gradient", "distance2", "observed",
        "accepted", "damping", "info", "weights", "scale", "effective"}


def run_robust(dens, head, x, steps, rounds=1, **kw):
    """One ``robust`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    proj = cmf_amd.ManifoldProjector(dens, steps=steps)
    tensors = {k: v.clone() for k, v in kw.items() if isinstance(v, torch.Tensor)}
    keep, marker = x.clone(), object()
    head.last_gram = marker
    out = proj.robust(x, rounds=rounds, **kw)
    assert head.last_gram is marker and torch.equal(x, keep) and all(torch.equal(kw[k], v) for k, v in tensors.items())
    B, d = x.shape[0], head.program.d
    assert set(out) == KEYS
    assert out["latent"].shape == (B, d) and out["latent"].dtype == torch.float32 and out["gradient"].shape == (B, d)
    assert out["reconstruction_head"].shape == (B, *head.x_shape) and out["reconstruction"].shape == x.shape
    assert out["weights"].shape == x.shape and out["weights"].dtype == torch.float32
    for key in ("cost", "initial_cost", "tangential2", "distance2", "damping", "scale", "effective"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64, key
    for key in ("accepted", "info", "observed"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    fine = out["info"] == 0
    assert bool((out["cost"] <= out["initial_cost"])[fine].all()) and bool((out["accepted"] <= rounds * steps).all())
    assert bool((out["accepted"] >= 0).all())
    return proj, out


@pytest.fixture(scope="module")
def solved():
    """Per fixture, once: the outlier problem on the GPU's own x_on, the product's answers and the float64 reference loop's."""
    cache = {}

    def get(name):
        if name not in cache:
            import cmf_amd
            g, meta, dens, head, x = build(name)
            with torch.no_grad():
                z0 = dens.extract_latent(x.clone(), earliest_latent=False)
                x_on = head.flow_forward(z0)
            y, planted = RR.problem(x_on, RR.KNOWN_ANSWER[name], seed=RR.SEED)
            yc = y.cuda().contiguous()
            proj, out = run_robust(head, head, yc, 10)
            cache[name] = {"head": head, "x_on": x_on, "y": yc, "planted": planted, "proj": proj, "robust": out,
                           "mask": proj.complete(yc, (~planted).cuda()), "project": proj.project(yc),
                           "tukey": run_robust(head, head, yc, 10, loss="tukey", init=out["latent"])[1],
                           "reference": RR.robust(R.Model(name), y.double(), steps=10)}
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(RR.KNOWN_ANSWER))
def test_robust_finds_the_outliers_nobody_marked(name, solved):
    """x_on = the GPU's own g(z_0) at the encoder's latent of the fixture's input; a share of its elements is off by 3 .. 6 RMS and
    every element carries 1 % RMS noise.  Ten Huber steps from the encoder's latent of that input, told nothing about the mask,
    must do what tests/test_robust_host.py establishes of the float64 loop -- conditions (a) - (e) -- and land within
    ``RR.E2E_TOL`` of that loop's own answer."""
    s = solved(name)
    out, x_on, planted = s["robust"], s["x_on"], s["planted"]
    rel = {k: CR.rel_distance(s[k]["reconstruction_head"], x_on) for k in ("robust", "mask", "project", "tukey")}
    w = out["weights"].cpu()
    cond = RR.conditions(rel["robust"], rel["mask"], rel["project"], w, planted, out["cost"].cpu(), out["initial_cost"].cpu())
    cond["e"] = RR.conditions(rel["tukey"], rel["mask"], rel["project"], w, planted, out["cost"].cpu(), out["initial_cost"].cpu())["a"]
    to_ref = CR.rel_distance(out["reconstruction_head"], s["reference"]["reconstruction_head"])
    print(f"{name}: ||g(z) - x_on|| / ||x_on|| worst: robust {float(rel['robust'].max()):.3e}, complete with the true mask "
          f"{float(rel['mask'].max()):.3e}, project {float(rel['project'].max()):.3e}, tukey {float(rel['tukey'].max()):.3e}; weights: "
          f"planted <= {float(w[planted].max()):.3e}, others >= {float(w[~planted].min()):.3e}; to the float64 loop "
          f"{float(to_ref.max()):.3e} (tolerance {RR.E2E_TOL[name]:.3e}); cost {float(out['initial_cost'].max()):.3e} -> "
          f"{float(out['cost'].max()):.3e}; accepted {out['accepted'].tolist()} (reference {s['reference']['accepted'].tolist()})")
    assert cond == {k: True for k in "abcde"}
    assert bool((to_ref <= RR.E2E_TOL[name]).all())
    assert bool((out["info"] == 0).all()) and out["observed"].cpu().tolist() == [x_on[0].numel()] * len(x_on)
    with torch.no_grad():
        assert torch.equal(out["reconstruction_head"], s["head"].flow_forward(out["latent"]))
    # the scale and the effective count are those of the float64 loop, to the data tolerance
    ref = s["reference"]
    assert bool(((out["scale"].cpu() - ref["scale"]).abs() <= 1e-3 * ref["scale"]).all())
    assert bool(((out["effective"].cpu() - ref["effective"]).abs() <= 1e-3 * ref["effective"]).all())


def test_uncertainty_takes_the_result(solved):
    s = solved("mini_mnist")
    out = s["robust"]
    u = s["proj"].uncertainty(out, weights=out["weights"], noise_std=out["scale"])
    assert bool((u["info"] == 0).all()) and bool(torch.isfinite(u["latent_covariance"]).all())
    assert bool(torch.isfinite(u["reconstruction_std_head"]).all()) and bool((u["latent_std"] > 0).all())


@pytest.mark.parametrize("name", ["c2b_hepmass", "mini_mnist_small"])
def test_without_down_weighting_it_is_complete(name):
    """Huber with c = 1e30 and a given scale: every omega is exactly 1, the weights are the prior's own bits, the steps are
    ``complete``'s, and the cost is sum p r^2 evaluated as 2 s^2 sum p ((r / s)^2 / 2): four more rounded operations per term and
    another summation order -- (2 (D + 3) + 2 (D + 3) + 8) u relative, the sum of both sides' bounds."""
    import cmf_amd
    g, meta, dens, head, x = build(name)
    p = torch.ones_like(x)
    p.flatten(1)[:, ::3] = 0.0
    p.flatten(1)[:, 1::3] = 2.5
    _, out = run_robust(dens, head, x, 10, loss="huber", tuning=1e30, scale=0.37, weights=p)
    ref = cmf_amd.ManifoldProjector(dens, steps=10).complete(x, p)
    D = x[0].numel()
    tol = (4 * (D + 3) + 8) * U
    print(f"{name}: cost rel {float(((out['cost'] - ref['cost']).abs() / ref['cost']).max()):.2e} (bound {tol:.2e}); accepted "
          f"{out['accepted'].tolist()} against {ref['accepted'].tolist()}")
    assert torch.equal(out["weights"], p) and torch.equal(out["observed"], ref["observed"])
    assert torch.equal(out["accepted"], ref["accepted"]) and torch.equal(out["latent"], ref["latent"])
    assert bool(((out["cost"] - ref["cost"]).abs() <= tol * ref["cost"]).all())
    assert bool(((out["initial_cost"] - ref["initial_cost"]).abs() <= tol * ref["initial_cost"]).all())
    assert torch.equal(out["info"], ref["info"]) and bool((out["scale"] == 0.37).all())      # the closing evaluation is complete's too
    assert same_bits(out["tangential2"].cpu().numpy(), ref["tangential2"].cpu().numpy()) and torch.equal(out["gradient"], ref["gradient"])
    assert torch.equal(out["effective"], ref["observed"].double())


def test_rounds_reestimate_the_scale(solved):
    s = solved("mini_cifar")
    _, one = run_robust(s["head"], s["head"], s["y"], 4)
    _, two = run_robust(s["head"], s["head"], s["y"], 4, rounds=2)
    assert bool((two["accepted"] <= 8).all()) and bool((two["accepted"] >= one["accepted"]).all())
    assert bool((two["info"] == 0).all()) and bool((two["cost"] <= two["initial_cost"]).all())
    assert bool((two["scale"] <= one["scale"]).all())                # the second round's residual is no larger: its cost fell


def test_sub_batches_give_the_rows_of_one_call(solved, monkeypatch):
    """Per-sample arguments -- weights, a scale tensor, init -- are cut with the batch (to the tolerance ``complete``'s test uses)."""
    from cmf_amd import engine as E
    s = solved("mini_mnist")
    y, head = s["y"], s["head"]
    w = torch.ones_like(y)
    w.flatten(1)[1, ::5] = 0.0
    w.flatten(1)[2, ::7] = 0.0
    w.flatten(1)[2, 1::7] = 3.0
    scale = (s["robust"]["scale"] * torch.tensor([1.0, 1.5, 0.75], dtype=torch.float64, device="cuda")).contiguous()
    init = (s["robust"]["latent"] + 0.01 * torch.arange(1, 4, device="cuda")[:, None]).contiguous()
    _, whole = run_robust(head, head, y, 6, weights=w, scale=scale, init=init)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    _, pieces = run_robust(head, head, y, 6, weights=w, scale=scale, init=init)
    c0 = whole["initial_cost"]
    assert float(((pieces["initial_cost"] - c0).abs() / c0).max()) <= 1e-5
    assert float(((pieces["cost"] - whole["cost"]).abs() / c0).max()) <= 1e-5
    assert torch.equal(pieces["observed"], whole["observed"]) and torch.equal(pieces["scale"], scale) and torch.equal(whole["scale"], scale)
    assert len(set(whole["observed"].tolist())) == 3 and bool((pieces["info"] == 0).all()) and bool((whole["info"] == 0).all())
    # x_hat to DESIGN 5's 1e-5 RMS moves u = r / s by 1e-5 RMS / s; s is 0.0115 RMS x 0.75 here, and |d omega / d u| <= 1 / c, p <= 3
    assert float((pieces["weights"] - whole["weights"]).abs().max()) <= 3 * 1e-5 / (0.0115 * 0.75) / 1.345


def test_a_sample_without_a_scale_stays_alone(solved):
    """All weights of sample 1 are zero: no used element, no scale -- ``info`` 3, it never moves -- and its neighbours' bits are
    those of the batch in which it was an ordinary sample."""
    s = solved("mini_mnist")
    y, head = s["y"], s["head"]
    ones = torch.ones_like(y)
    _, base = run_robust(head, head, y, 6, weights=ones)
    holed = ones.clone()
    holed[1] = 0.0
    _, out = run_robust(head, head, y, 6, weights=holed)
    assert out["info"].tolist() == [0, 3, 0] and out["accepted"].tolist()[1] == 0 and out["observed"].tolist()[1] == 0
    assert bool(torch.isnan(out["cost"][1])) and bool(torch.isnan(out["weights"][1]).all()) and bool(torch.isnan(out["scale"][1]))
    for k in KEYS:
        assert same_bits(out[k][[0, 2]].cpu().numpy(), base[k][[0, 2]].cpu().numpy()), k
    _, still = run_robust(head, head, y, 0, weights=holed)
    assert torch.equal(out["latent"][1], still["latent"][1])
