"""``cmf_amd.ManifoldProjector.uncertainty`` on the GPU, end to end on the reference-generated fixtures after all four
fitting calls -- ``project``, ``complete``, ``recover`` in head space and, on the image fixture, ``recover(space="data")`` -- against
the float64 reference evaluated at the product's own latent, within the tolerance tests/test_uncertainty_host.py derives from the
project's Jacobian tolerance (``LE.E2E_TOL``); and what the method promises beside the numbers.  Needs an MI355X: run with ``-m gpu``."""
import pytest
import torch

import _completion_reference as CR
import _data_recovery_reference as DR
import _leverage_emulation as LE
import _projection_reference as R
import _recovery_reference as RR
from test_gpu_metric_stats import build

pytestmark = pytest.mark.gpu

KEYS = {"latent_covariance", "latent_std", "reconstruction_std_head", "leverage", "noise_variance", "dof", "info"}
_MODELS, _FITS = {}, {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = R.Model(name)
    return _MODELS[name]


def run_uncertainty(proj, head, result, **kw):
    """One ``uncertainty`` with the side-effect and shape checks every case makes."""
    tensors = [v for v in (*result.values(), *kw.values()) if isinstance(v, torch.Tensor)]
    keep = [v.clone() for v in tensors]
    marker = object()
    head.last_gram = marker
    err = proj.uncertainty(result, **kw)
    assert head.last_gram is marker
    assert all(torch.equal(v, k) or bool(torch.isnan(k).any()) for v, k in zip(tensors, keep))
    B, d = result["latent"].shape
    assert set(err) == KEYS | ({"reconstruction_std"} if kw.get("space") == "data" else set())
    assert all(v.is_cuda for v in err.values())
    assert err["latent_covariance"].shape == (B, d, d) and err["latent_std"].shape == (B, d)
    assert err["leverage"].shape == (B, *head.x_shape) == err["reconstruction_std_head"].shape
    for key in ("latent_covariance", "latent_std", "leverage", "noise_variance"):
        assert err[key].dtype == torch.float64
    assert err["reconstruction_std_head"].dtype == torch.float32
    for key in ("dof", "info"):
        assert err[key].shape == (B,) and err[key].dtype == torch.int32
    assert err["noise_variance"].shape == (B,)
    return err


def fit(name, path):
    """The fixture, the fitting call of ``path`` on it and what describes the problem to ``uncertainty`` and to the reference:
    (dens, head, proj, out, uncertainty keywords, reference keywords without the Jacobian's).  Computed once per case; nothing
    below modifies it."""
    if (name, path) in _FITS:
        return _FITS[name, path]
    import cmf_amd
    g, meta, dens, head, x = build(name)
    if name == "mini_mnist":
        x = x[:DR.BATCH].contiguous()
    with torch.no_grad():
        x_on = head.flow_forward(dens.extract_latent(x.clone(), earliest_latent=False))
    D = x_on[0].numel()
    if path == "project":
        proj = cmf_amd.ManifoldProjector(dens, steps=10)
        out = proj.project(x)
        kw, ref_kw = {}, dict(cost=out["distance2"].cpu())
    elif path == "complete":                                         # in head space, as tests/test_gpu_completion.py sets it
        proj = cmf_amd.ManifoldProjector(head, steps=10)
        y, w = CR.problem(x_on, data_rel=LE.MEASUREMENT_REL)
        w = w.cuda().contiguous()
        out = proj.complete(y.cuda().contiguous(), w)
        kw, ref_kw = dict(weights=w), dict(cost=out["cost"].cpu(), w=w.cpu().double().flatten(1))
    elif path == "recover":
        proj = cmf_amd.ManifoldProjector(head, steps=10)
        A = RR.gaussian_operator(RR.KNOWN_ANSWER[name], D)
        y = RR.measure(A, x_on, data_rel=LE.MEASUREMENT_REL).float().cuda().contiguous()
        A = A.cuda().contiguous()
        out = proj.recover(y, A, x_init=RR.start_input(x_on).cuda().contiguous())
        kw, ref_kw = dict(operator=A), dict(cost=out["cost"].cpu(), A=A.cpu().double())
    else:                                                            # pixel values behind the logit wrapper
        from cmf_amd.projection import data_space_wrapper
        proj = cmf_amd.ManifoldProjector(dens, steps=10)
        wa, wc, logit, perm = data_space_wrapper(proj.chain)
        assert perm is None and logit
        dm = DR.DataModel(None, (wa, wc, logit))
        A = DR.operator("built")
        y = RR.measure(A, dm.wrapper(x_on.cpu().double())[0], data_rel=LE.MEASUREMENT_REL).float().cuda().contiguous()
        A = A.cuda().contiguous()
        out = proj.recover(y, A, x_init=DR.start_input(dm, x_on.cpu()).float().cuda().contiguous(), space="data")
        kw, ref_kw = dict(operator=A, space="data"), dict(cost=out["cost"].cpu(), A=A.cpu().double(), dm=dm)
    assert bool((out["info"] == 0).all())
    _FITS[name, path] = (dens, head, proj, out, kw, ref_kw)
    return _FITS[name, path]


def reference_at(name, latent, ref_kw, **more):
    """``LE.uncertainty`` with the float64 oracle's Jacobian at the product's ``latent``."""
    m = model(name)
    z = latent.cpu().double()
    ref_kw = dict(ref_kw, **more)
    dm = ref_kw.pop("dm", None)
    if dm is not None:
        ref_kw["s"] = dm.wrapper(m.decode(z))[1].flatten(1)
    return LE.uncertainty(m.jacobian(z)[2], **ref_kw)


@pytest.mark.parametrize("name,path", LE.E2E_CASES)
def test_uncertainty_matches_the_reference_at_the_products_latent(name, path):
    dens, head, proj, out, kw, ref_kw = fit(name, path)
    err = run_uncertainty(proj, head, out, **kw)
    ref = reference_at(name, out["latent"], ref_kw)
    dist = LE.std_distance(err, ref)
    print(f"{name}, {path}: worst relative distance of the standard deviations to the reference {float(dist.max()):.3e} (tolerance "
          f"{LE.E2E_TOL[name, path]:.3e}); dof {err['dof'].tolist()}; sigma^2 {err['noise_variance'].tolist()}")
    assert bool((err["info"] == 0).all()) and torch.equal(err["dof"].cpu(), ref["dof"])
    cost = out["cost"] if "cost" in out else out["distance2"]
    assert torch.equal(err["noise_variance"], cost / err["dof"].double())
    assert bool((dist <= LE.E2E_TOL[name, path]).all())
    assert not bool(torch.signbit(err["leverage"]).any())
    assert torch.equal(err["latent_covariance"], err["latent_covariance"].transpose(1, 2))
    assert torch.equal(err["latent_std"], torch.diagonal(err["latent_covariance"], dim1=1, dim2=2).sqrt())
    # a known noise level: the same covariance shape, another scale, and no cost is read
    given = run_uncertainty(proj, head, {"latent": out["latent"]}, noise_std=0.05, **kw)
    assert torch.equal(given["noise_variance"], torch.full_like(given["noise_variance"], 0.05) ** 2)
    assert torch.equal(given["leverage"], err["leverage"]) and torch.equal(given["dof"], err["dof"])
    ref = reference_at(name, out["latent"], {k: v for k, v in ref_kw.items() if k != "cost"}, noise_std=0.05)
    assert bool((LE.std_distance(given, ref) <= LE.E2E_TOL[name, path]).all())
    per_sample = torch.linspace(0.01, 0.1, out["latent"].shape[0], dtype=torch.float64, device="cuda")
    per_sample[0] = -1.0                                             # a negative level: that sample's answer is NaN, on the device
    given = run_uncertainty(proj, head, {"latent": out["latent"]}, noise_std=per_sample, **kw)
    assert bool(torch.isnan(given["noise_variance"][0])) and bool(torch.isnan(given["latent_std"][0]).all())
    assert torch.equal(given["noise_variance"][1:], per_sample[1:] ** 2) and bool(torch.isfinite(given["latent_std"][1:]).all())


@pytest.mark.parametrize("name", LE.FIXTURES)
def test_leverage_of_a_projection_sums_to_the_latent_dimension(name):
    """With the Gram matrix of the sweep's own J the leverages are the diagonal of a projector of rank d.  The engine calls of the
    method, repeated here, give the method's bits -- and the J and G the kernel bound is stated in."""
    from cmf_amd import engine as E
    dens, head, proj, out, kw, _ = fit(name, "project")
    err = run_uncertainty(proj, head, out)
    d = head.program.d
    with torch.no_grad(), E.scope(head.kernels):
        _, T = head.program.decode(out["latent"], tangents=True)
        G = E.gram_cholesky(T, d, 1).jtj
        r = E.tangent_leverage(T, G)
    assert torch.equal(r.lev, err["leverage"].flatten(1))
    J, G = T.to_dense(d).contiguous().cpu().numpy(), G.cpu().numpy()
    for b in range(J.shape[0]):
        cov_ref, lev_ref, _, info = LE.reference(J[b], G[b])
        total = float(r.lev[b].sum())
        print(f"{name}, sample {b}: |sum lev - d| = {abs(total - d):.3e} (bound {LE.trace_bound(J[b], G[b], cov_ref, lev_ref):.3e})")
        assert info == 0 and abs(total - d) <= LE.trace_bound(J[b], G[b], cov_ref, lev_ref)
        assert LE.lev_ratio(G[b], r.lev[b].cpu().numpy(), lev_ref) <= LE.C_LEV


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass"])
def test_unit_weights_and_the_identity_operator_give_the_plain_case(name):
    """The identity operator: K is J bit for bit in the same layout and the Gram kernel is the same one, so every key is equal by
    ``torch.equal``.  All-ones weights: the weighted step kernel forms its own Gram matrix in another summation order, so the
    answers agree to the Gram kernels' rounding -- within the tolerance of the plain case -- and not to bits."""
    dens, head, proj, out, _, _ = fit(name, "project")
    plain = run_uncertainty(proj, head, out)
    D = out["reconstruction_head"][0].numel()
    through = run_uncertainty(proj, head, out, operator=torch.eye(D, device="cuda"))
    for key in plain:
        assert torch.equal(through[key], plain[key]), key
    for ones in (torch.ones_like(out["reconstruction"]), torch.ones(out["reconstruction"].shape[1:], dtype=torch.bool, device="cuda")):
        weighted = run_uncertainty(proj, head, out, weights=ones)
        assert torch.equal(weighted["dof"], plain["dof"]) and torch.equal(weighted["noise_variance"], plain["noise_variance"])
        assert bool((LE.std_distance(weighted, plain) <= LE.E2E_TOL[name, "project"]).all())
        assert bool((weighted["info"] == 0).all())


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass"])
def test_identity_chain_gives_the_head_space_bits(name):
    """No wrapper in front of the head: the triple is (1, 0, 0) and du/dv is 1.0f exactly, so space="data" is space="head" bit for
    bit, with and without an operator, and ``reconstruction_std`` is ``reconstruction_std_head``."""
    dens, head, proj, out, _, _ = fit(name, "project")
    D = out["reconstruction_head"][0].numel()
    A = RR.gaussian_operator(RR.KNOWN_ANSWER[name], D).cuda().contiguous()
    for kw in ({}, {"operator": A}):
        in_head = run_uncertainty(proj, head, out, **kw)
        in_data = run_uncertainty(proj, head, out, space="data", **kw)
        for key in in_head:
            assert torch.equal(in_data[key], in_head[key]), key
        assert torch.equal(in_data["reconstruction_std"], in_head["reconstruction_std_head"].view_as(in_data["reconstruction_std"]))


def test_data_space_without_an_operator_takes_the_wrapper_derivative():
    """``project`` on the image fixture, qualified in pixel values: the head-space keys are the plain call's bits, and
    ``reconstruction_std`` is |du/dv| times the head-space value, du/dv formed in torch (no operator kernel ran to leave it)."""
    from cmf_amd.projection import data_space_wrapper
    name = "mini_mnist"
    dens, head, proj, out, _, ref_kw = fit(name, "project")
    plain = run_uncertainty(proj, head, out)
    err = run_uncertainty(proj, head, out, space="data")
    for key in plain:
        assert torch.equal(err[key], plain[key]), key
    assert err["reconstruction_std"].shape == out["reconstruction"].shape and err["reconstruction_std"].dtype == torch.float32
    wa, wc, logit, perm = data_space_wrapper(proj.chain)
    assert perm is None and logit
    ref = reference_at(name, out["latent"], dict(ref_kw, dm=DR.DataModel(None, (wa, wc, logit))))
    dist = LE.std_distance(err, ref)
    print(f"{name}, project in data space: worst relative distance {float(dist.max()):.3e} (tolerance {LE.E2E_TOL[name, 'project-data']:.3e})")
    assert bool((dist <= LE.E2E_TOL[name, "project-data"]).all())


def test_weights_travel_through_the_wrapper_chain():
    """On the image fixture through the DENSITY: weights in data shape, mapped by ``to_head_space_weights``, give what the same
    weights give the projector of the head itself."""
    import cmf_amd
    from cmf_amd.projection import to_head_space_weights
    dens, head, proj, out, _, _ = fit("mini_mnist", "project")
    gen = torch.Generator().manual_seed(5)
    w = (torch.rand(out["reconstruction"].shape, generator=gen) > 0.5).float().cuda()
    through = run_uncertainty(proj, head, out, weights=w)
    direct = run_uncertainty(cmf_amd.ManifoldProjector(head), head, out,
                             weights=to_head_space_weights(proj.chain, w).reshape(out["reconstruction_head"].shape).contiguous())
    for key in through:
        assert torch.equal(through[key], direct[key]), key
    assert torch.equal(through["dof"], ((w > 0).flatten(1).sum(1) - head.program.d).int())
    hidden = (w == 0).view_as(through["reconstruction_std_head"])
    assert bool(torch.isfinite(through["reconstruction_std_head"][hidden]).all())      # an unobserved element gets a finite value


def test_underdetermined_problem_is_a_result():
    """M = 5 < d = 10: K^T K is singular -- ``info`` = 1, NaN covariance and leverage, dof = -5 and a NaN noise level."""
    import cmf_amd
    name, M = RR.UNDERDETERMINED
    g, meta, dens, head, x = build(name)
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on = head.flow_forward(z0)
    A = RR.gaussian_operator(M, x_on[0].numel()).cuda().contiguous()
    proj = cmf_amd.ManifoldProjector(head)
    result = {"latent": z0.contiguous(), "cost": torch.ones(z0.shape[0], dtype=torch.float64, device="cuda")}
    err = run_uncertainty(proj, head, result, operator=A)
    assert bool((err["info"] == 1).all()) and bool((err["dof"] == M - head.program.d).all())
    for key in ("latent_covariance", "latent_std", "leverage", "reconstruction_std_head", "noise_variance"):
        assert bool(torch.isnan(err[key]).all()), key
    err = run_uncertainty(proj, head, result, operator=A, noise_std=0.1)
    assert bool((err["info"] == 1).all()) and bool(torch.isnan(err["latent_std"]).all())
    assert torch.equal(err["noise_variance"], torch.full_like(err["noise_variance"], 0.1) ** 2)


@pytest.mark.parametrize("name,path", [("c2a_power", "recover"), ("mini_mnist", "complete"), ("mini_mnist", "data")])
def test_sub_batches_give_the_rows_of_one_call(name, path, monkeypatch):
    from cmf_amd import engine as E
    dens, head, proj, out, kw, _ = fit(name, path)
    out = {k: v[:3].contiguous() for k, v in out.items()}
    kw = {k: (v[:3].contiguous() if k == "weights" else v) for k, v in kw.items()}
    whole = run_uncertainty(proj, head, out, **kw)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    pieces = run_uncertainty(proj, head, out, **kw)
    print(f"{name}, {path}: pieces against whole: bit-equal {all(torch.equal(pieces[k], whole[k]) for k in whole)}")
    assert torch.equal(pieces["dof"], whole["dof"]) and torch.equal(pieces["info"], whole["info"])
    assert torch.equal(pieces["noise_variance"], whole["noise_variance"])
    assert bool((LE.std_distance(pieces, whole) <= LE.E2E_TOL[name, path]).all())


def test_the_log_density_path_is_untouched():
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        _, head_fit, proj, out, kw, _ = fit("mini_mnist", "data")
        err = run_uncertainty(proj, head_fit, out, **kw)
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
    assert bool((err["info"] == 0).all())


def test_refusals_on_the_gpu():
    dens, head, proj, out, _, _ = fit("c2a_power", "project")
    D = out["reconstruction_head"][0].numel()
    with pytest.raises(ValueError, match="not both"):
        proj.uncertainty(out, weights=torch.ones_like(out["reconstruction"]), operator=torch.eye(D, device="cuda"))
    with pytest.raises(ValueError, match="weights must be on"):
        proj.uncertainty(out, weights=torch.ones(out["reconstruction"].shape))
    with pytest.raises(ValueError, match="operator must be on"):
        proj.uncertainty(out, operator=torch.eye(D))
    with pytest.raises(ValueError, match="noise_std must be >= 0"):
        proj.uncertainty(out, noise_std=-0.5)
    with pytest.raises(ValueError, match="space must be"):
        proj.uncertainty(out, space="pixel")
