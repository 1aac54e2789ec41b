"""Wide latents, 128 < ceil16(d) <= 512: the Jacobian head kernels of csrc/head_wide.hip through the C ABI, against float64 torch
on the same panel and the float64 oracle.  Every one of these calls returned CMF_EINVAL before the wide head existed."""
import pytest
import torch

from conftest import fp64_bound
from test_gpu_parity import find_head, rel

pytestmark = pytest.mark.gpu


def _panel(B, N, d, seed, lo=0.5, hi=2.0):
    """(B, N, d) float32 Jacobian panels with singular values log-uniform in [lo, hi] (condition of J^T J <= (hi / lo)^2)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        U, _ = torch.linalg.qr(torch.randn(N, d, generator=gen, dtype=torch.float64))
        V, _ = torch.linalg.qr(torch.randn(d, d, generator=gen, dtype=torch.float64))
        s = torch.exp(torch.empty(d, dtype=torch.float64).uniform_(float(torch.log(torch.tensor(lo))), float(torch.log(torch.tensor(hi))),
                                                                   generator=gen))
        out.append((U * s) @ V.T)
    return torch.stack(out).float()


def _tangent(J, nc, layout):
    from cmf_amd import engine as E
    return E.Tangent.from_dense(J.cuda(), nc, layout)


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("N,nc,d", [(784, 144, 144), (3072, 192, 187), (784, 256, 256), (3072, 512, 500)])
def test_wide_gram_cholesky_matches_fp64(layout, N, nc, d):
    from cmf_amd import engine as E
    B = 3
    J = _panel(B, N, d, seed=nc + d)
    T = _tangent(J, nc, layout)
    gr = E.gram_cholesky(T, d)
    assert gr.fail.tolist()[0] == 0 and gr.info.abs().sum().item() == 0
    J64 = J.double()
    G64 = J64.transpose(1, 2) @ J64
    jtj = gr.jtj.cpu()
    assert torch.equal(jtj, jtj.transpose(1, 2)), "jtj must come back exactly symmetric (the factorisation restores it)"
    assert rel(jtj, G64) < 1e-5                                     # fp32 sums over N rows: ~sqrt(N) 2^-24
    ld64 = torch.linalg.slogdet(G64)[1]
    # what fp32 arithmetic alone costs on this panel: a float32 Gram product (torch's, and our jtj itself, factorised exactly),
    # plus the d rounded pivots of an fp32 elimination
    ld32 = torch.linalg.slogdet(J.transpose(1, 2) @ J)[1].double()
    ldj = torch.linalg.slogdet(jtj.double())[1]
    err = (gr.logdet.cpu().double() - ld64).abs()
    bound = 3 * torch.maximum((ld32 - ld64).abs(), (ldj - ld64).abs()) + 1e-6 * d
    assert bool((err <= bound).all()), (err, bound)
    eye = torch.eye(d, dtype=torch.bool)
    assert rel(gr.l1_diag.cpu(), G64.diagonal(dim1=1, dim2=2).abs().sum(1)) < 1e-5
    assert rel(gr.l1_off.cpu(), G64.masked_select(~eye).view(B, -1).abs().sum(1)) < 1e-5


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
def test_wide_rank_deficient_panel_retries_like_the_reference(layout):
    """A duplicated column makes sample 1 singular: attempt 0 raises fail[0]; the enqueued retries jitter EVERY sample
    (non_square.py:280-288) until the batch factorises; the jittered jtj and its log-det are the reference loop's."""
    from cmf_amd import engine as E
    from oracle import cmf_oracle as O
    B, N, nc, d = 3, 784, 192, 160
    J = _panel(B, N, d, seed=5)
    J[1, :, 7] = J[1, :, 3]
    T = _tangent(J, nc, layout)
    gr = E.gram_cholesky(T, d)
    fail = gr.fail.tolist()
    attempts = 1 + next(i for i, f in enumerate(fail) if not f)
    assert attempts >= 2 and gr.info.tolist()[0] == 0
    G = (J.transpose(1, 2).double() @ J.double())
    added = sum(1e-6 * 10 ** k for k in range(attempts - 1))
    want = G + added * torch.eye(d, dtype=torch.float64)
    assert rel(gr.jtj.cpu(), want) < 1e-5
    # the reference's loop on the jittered matrix factorises at once and gives our log-det on the regular samples (the singular
    # one's smallest pivot is the jitter plus fp32 rounding of J^T J: its log-det is as arbitrary in the reference's float32)
    ld_ref, _, att_ref = O.cholesky_logdet(want)
    assert att_ref == 1
    ld = gr.logdet.cpu().double()
    assert (ld[[0, 2]] - ld_ref.view(-1)[[0, 2]]).abs().max() < 1e-4 * ld_ref.abs().max().clamp_min(10.0)
    assert bool(torch.isfinite(ld).all()) and abs(float(ld[1] - ld_ref.view(-1)[1])) < 0.5


@pytest.mark.parametrize("d", [192, 512])
def test_wide_gram_backward_matches_fp64_autograd(d):
    from cmf_amd import engine as E
    B, N, nc = 2, 3072, E.ceil16(d)
    J = _panel(B, N, d, seed=d)
    T = _tangent(J, nc, "panel")
    gr = E.gram_cholesky(T, d)
    gen = torch.Generator().manual_seed(1)
    ga, go, gd = torch.randn(B, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    dT = E.gram_backward(T, gr.jtj, ga.cuda(), go.cuda(), gd.cuda()).to_dense(nc).cpu()
    J64 = J.double().requires_grad_(True)
    G = J64.transpose(1, 2) @ J64
    eye = torch.eye(d, dtype=torch.bool)
    # |G_ij| differentiated with the signs of the fp32 Gram matrix the kernel saw: off-diagonal entries within rounding of zero
    # flip sign between fp32 and fp64 (a kink, not an error of either)
    sg = torch.sign(gr.jtj.cpu().double())
    obj = (ga.double() * torch.linalg.slogdet(G)[1] + go.double() * (sg * G).masked_select(~eye).view(B, -1).sum(1)
           + gd.double() * (sg * G).diagonal(dim1=1, dim2=2).sum(1)).sum()
    want, = torch.autograd.grad(obj, J64)
    assert rel(dT[:, :, :d], want) < 1e-4
    assert nc == d or dT[:, :, d:].abs().max() == 0
    M = torch.randn(B, d, d, generator=gen)
    dM = E.gram_backward_matrix(T, M.cuda()).to_dense(nc).cpu()
    assert rel(dM[:, :, :d], J.double() @ (M + M.transpose(1, 2)).double()) < 1e-5
    assert nc == d or dM[:, :, d:].abs().max() == 0


@pytest.mark.parametrize("d", [192, 512])
@pytest.mark.parametrize("S", [1, 4, "d"])
def test_wide_hutchinson_matches_torch(d, S):
    from cmf_amd import engine as E
    S = d if S == "d" else S
    B = 2
    J = _panel(B, 1024, d, seed=3 * d + S)
    gr = E.gram_cholesky(_tangent(J, E.ceil16(d), "panel"), d, 1)
    G = gr.jtj.cpu().double()
    gen = torch.Generator().manual_seed(S)
    eps = torch.randn(B, d, S, generator=gen)
    val, u, w, iters = E.hutch_cg(gr.jtj, eps.cuda(), d, 1e-5)
    w64 = G @ eps.double()
    u64 = torch.linalg.solve(G, eps.double())
    assert rel(w.cpu(), w64) < 1e-5
    assert rel(u.cpu(), u64) < 1e-3
    assert rel(val.cpu(), (u64 * w64).sum(1).mean(1)) < 1e-3
    assert int(iters.max()) <= d
    off, diag = E.hutch_metric(w)
    assert rel(diag.cpu(), torch.diagonal(w64, dim1=-2, dim2=-1).abs().sum(1)) < 1e-5
    if S == d:
        eye = torch.eye(d, dtype=torch.bool)
        assert rel(off.cpu(), w64.masked_select(~eye).view(B, -1).abs().sum(1)) < 1e-5
    else:
        assert off is None
    gv, go, gd = torch.randn(B, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    goff = go.cuda() if S == d else None
    M = E.hutch_cotangent(u, eps.cuda(), w, gv.cuda(), goff, gd.cuda()).cpu().double()
    sg = torch.sign(w.cpu().double())
    k = torch.arange(d)[:, None] == torch.arange(S)[None, :]
    left = (gv.double() / S)[:, None, None] * u.cpu().double() + sg * torch.where(k, gd.double()[:, None, None],
                                                                                   (go.double() if S == d else 0 * go.double())[:, None, None])
    assert rel(M, left @ eps.double().transpose(1, 2)) < 1e-5
    Cm = E.hutch_lowrank_cotangent(w, S, gv.cuda(), gd.cuda()).cpu().double()
    K, n = min(d, S), 2 * S + min(d, S)
    want = torch.zeros(B, n, n, dtype=torch.float64)
    idx = torch.arange(S)
    want[:, idx, S + idx] = (gv.double() / S)[:, None]
    kk = torch.arange(K)
    want[:, 2 * S + kk, S + kk] = gd.double()[:, None] * torch.sign(w.cpu().double()[:, kk, kk])
    assert rel(Cm, want) < 1e-6


def _model(dataset, d, method="cholesky", seed=3):
    import cmf_amd
    from cmf_amd.recipe import fill_state_dict
    from oracle import cmf_oracle as O
    cfg = cmf_amd.get_config(dataset, latent_dimension=d, g_hidden_channels=[8] * 2, log_jacobian_method=method)
    schema = cmf_amd.get_schema(cfg)
    shape = cmf_amd.DATA_SHAPES[dataset]
    dens = cmf_amd.get_density(schema, torch.zeros(1, *shape))
    sd = fill_state_dict(dens.state_dict(), seed=seed)
    dens.load_state_dict(sd, strict=True)
    ops = O.compile_schema(schema, shape)
    return dens.cuda().eval(), ops, sd, shape


def _images(B, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, *shape), generator=gen).float() + torch.rand(B, *shape, generator=gen)


@pytest.mark.parametrize("dataset,d", [("cifar10", 144), ("cifar10", 256), ("cifar10", 512), ("mnist", 256)])
def test_wide_elbo_and_ood_match_oracle(dataset, d):
    from oracle import cmf_oracle as O
    dens, ops, sd, shape = _model(dataset, d)
    B = 2
    x = _images(B, shape, seed=d)
    inner = dens.module.density
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    zero = torch.zeros_like(x)
    with torch.no_grad():
        for kw in ({"add_offdiagonal_metric_reg": True}, {"add_diagonal_metric_reg": True}):
            got = inner.elbo(x.cuda(), add_reconstruction=True, **kw)["elbo"].cpu()
            want = O.elbo(sd64, ops, x.double(), noise=zero.double(), **kw)["elbo"]
            want32 = O.elbo(sd, ops, x, noise=zero, **kw)["elbo"]
            bound, _ = fp64_bound(want, want32)
            err = (got.double().reshape(-1) - want.double().reshape(-1)).abs()
            assert bool((err <= bound).all()), (kw, err, bound)
        got = inner.elbo(x.cuda(), add_reconstruction=True, ood=True)
        want = O.elbo(sd64, ops, x.double(), noise=zero.double(), ood=True)
        want32 = O.elbo(sd, ops, x, noise=zero, ood=True)
        for key in ("likelihood", "reconstruction-error"):
            bound, _ = fp64_bound(want[key], want32[key])
            err = (got[key].cpu().double().reshape(-1) - want[key].double().reshape(-1)).abs()
            assert bool((err <= bound).all()), (key, err, bound)
        head = find_head(dens)
        pre, hd, flow_ops, base, prior_ops = O.split_ops(ops)
        z_low = torch.randn(B, d, generator=torch.Generator().manual_seed(0)) * 0.5
        x_hat, T = head.program.decode(z_low.cuda(), tangents=True)
        from cmf_amd import engine as E
        gr = E.gram_cholesky(T, d)
        jtj64, xh64, _ = O.jtj_batched(sd64, flow_ops, base, z_low.double())
        assert rel(x_hat.reshape(B, -1).cpu(), xh64.reshape(B, -1)) < 1e-4
        assert rel(gr.jtj.cpu(), jtj64) < 1e-4


def test_wide_elbo_graph_replays_equal_to_eager():
    from cmf_amd.graphs import ElboGraph
    dens, ops, sd, shape = _model("cifar10", 256)
    x = _images(2, shape, seed=1).cuda()
    inner = dens.module.density
    with torch.no_grad():
        eager = inner.elbo(x, add_reconstruction=True, add_offdiagonal_metric_reg=True)["elbo"].clone()
        g = ElboGraph(inner, x, add_reconstruction=True, add_offdiagonal_metric_reg=True)
        for _ in range(2):
            assert torch.equal(g(x)["elbo"], eager)


@pytest.mark.parametrize("method,S,term", [("cholesky", None, "off"), ("hutch_with_cg", 1, None), ("hutch_with_cg", "d", "off")])
def test_wide_training_gradients_match_oracle_autograd(method, S, term):
    """d = 192 on the mini CIFAR model: head_terms_backward (gram_backward / hutch cotangents through the wide kernels) against
    torch.autograd through the float64 oracle, as test_gpu_round3's low-rank test does."""
    from oracle import cmf_oracle as O
    d, B = 192, 2
    dens, ops, sd, shape = _model("cifar10", d, method)
    head = find_head(dens)
    named = dict(dens.named_parameters())
    gen = torch.Generator().manual_seed(11)
    z_low = 0.5 * torch.randn(B, d, generator=gen)
    a, c = torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    keys = [k for k, v in sd.items() if v.is_floating_point() and k in named]
    pre, hd, flow_ops, base, prior_ops = O.split_ops(ops)
    S = d if S == "d" else S
    eps = torch.randn(B, d, S, generator=gen) if S else None

    def oracle_gradients(dtype):
        sdt = {k: (v.to(dtype).clone().requires_grad_(True) if k in keys else (v.to(dtype) if v.is_floating_point() else v))
               for k, v in sd.items()}
        zt = z_low.to(dtype).requires_grad_(True)
        jtj, xh, J = O.jtj_batched(sdt, flow_ops, base, zt)
        eye = torch.eye(d, dtype=torch.bool)
        if eps is None:
            value = torch.linalg.slogdet(jtj)[1]
            mat = jtj
        else:
            mat = torch.bmm(jtj, eps.to(dtype))
            u = torch.linalg.solve(jtj.detach(), eps.to(dtype)).detach()
            value = (u * mat).sum(1).mean(1)
        obj = (a.to(dtype) * value).sum()
        if term == "off":
            obj = obj + (c.to(dtype) * mat.masked_select(~eye).view(B, -1).abs().sum(1)).sum()
        return torch.autograd.grad(obj, [sdt[k] for k in keys] + [zt], allow_unused=True)

    want, want32 = oracle_gradients(torch.float64), oracle_gradients(torch.float32)
    if eps is not None:
        head.num_hutchinson_samples, head.max_cg_iterations, head.cg_tolerance = S, d, 1e-7
    st = head.head_terms_forward(z_low.cuda(), tangents=True, hutch_eps=None if eps is None else eps.cuda(),
                                 add_off=term == "off")
    out = head.head_terms_backward(z_low.cuda(), None, g_logdet=a.cuda(), g_l1off=c.cuda() if term == "off" else None, state=st)
    worst = 0.0
    for k, wv, w32 in zip(keys, want[:-1], want32[:-1]):
        if wv is None or float(wv.abs().max()) == 0:
            continue
        bound = max(1e-3, 3 * rel(w32, wv))
        err = rel(out["grads"][named[k]], wv.reshape(named[k].shape))
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    assert rel(out["dz_low"], want[-1]) <= max(1e-3, 3 * rel(want32[-1], want[-1]))


def test_latent_wider_than_512_constructs_then_raises_before_any_head_kernel():
    import cmf_amd
    from cmf_amd import _lib
    cfg = cmf_amd.get_config("cifar10", latent_dimension=520, g_hidden_channels=[8] * 2, log_jacobian_method="cholesky")
    shape = cmf_amd.DATA_SHAPES["cifar10"]
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), torch.zeros(1, *shape)).cuda().eval()
    x = _images(2, shape, seed=0).cuda()
    with torch.no_grad(), _lib.trace() as calls:
        with pytest.raises(ValueError, match=r"1 <= latent_dimension <= 512"):
            dens.module.density.elbo(x, add_reconstruction=True)
    assert not [c for c in calls if "gram" in c[0] or "cholesky" in c[0] or "hutch" in c[0]], calls
    with torch.no_grad():
        assert dens.sample(2).shape == (2, *shape)
