"""Precision guard on the GPU (``head.precision_guard``, ``engine.gram_condition``): the condition numbers against
float64 torch, the flag list, and the guarded evaluation against unguarded ones -- at the threshold extremes, on mixed batches,
chunked, nested, lazy, captured -- plus the training path, which the guard must not touch."""
import math

import pytest
import torch

from conftest import load_golden
from test_gpu_parity import build, find_head, inner, rel

pytestmark = pytest.mark.gpu


def _spd(d, kappa, gen):
    """float32 symmetric positive definite matrix: random orthogonal x geometric eigenvalues 1 .. 1/kappa."""
    q, _ = torch.linalg.qr(torch.randn(d, d, generator=gen, dtype=torch.float64))
    ev = torch.logspace(0.0, -math.log10(kappa), d, dtype=torch.float64) if d > 1 else torch.ones(1, dtype=torch.float64)
    a = (q * ev) @ q.T
    return ((a + a.T) / 2).float()


def _kappa1(a):
    a = a.double()
    return float(torch.linalg.matrix_norm(a, ord=1) * torch.linalg.matrix_norm(torch.linalg.inv(a), ord=1))


def _condition(jtj, info, thr):
    from cmf_amd import engine as E
    r = E.GramResult()
    r.jtj, r.info = jtj, info
    return E.gram_condition(r, jtj.shape[1], thr)


@pytest.mark.parametrize("d", [1, 2, 10, 64, 100, 128, 144, 256, 500])
def test_condition_numbers_against_float64(d):
    """Exact kappa_1 (float64 inside the kernel): 1e-4 relative to torch's float64 value of the same float32 matrix for
    kappa up to 1e6; a matrix with a negative eigenvalue and a sample whose factorisation failed (info != 0) give +inf; the flag
    list is ascending and complete for several thresholds; jtj is bit-unchanged."""
    gen = torch.Generator().manual_seed(d)
    kappas = [1.0, 1e2, 1e4, 1e6]
    mats = [_spd(d, k, gen) for k in kappas]
    bad = _spd(d, 1e2, gen)
    bad[0, 0] = -1.0                                          # not positive definite (its first pivot fails)
    mats += [bad, _spd(d, 1e2, gen)]
    jtj = torch.stack(mats).cuda()
    info = torch.zeros(len(mats), dtype=torch.int32, device="cuda")
    info[-1] = 3                                              # the head's factorisation failed on this one
    keep = jtj.clone()
    r = _condition(jtj, info, 1e3)
    cond = r.cond.cpu()
    assert torch.equal(jtj, keep)
    for b, k in enumerate(kappas):
        want = _kappa1(mats[b])
        assert want >= 1.0 and (d == 1 or k / 10 <= want <= 10 * k * d)          # kappa_1 vs the 2-norm kappa: within d
        assert abs(float(cond[b]) - want) <= 1e-4 * want, (d, k, float(cond[b]), want)
    assert cond[-2] == math.inf and cond[-1] == math.inf
    for thr in (0.0, 1.5, 1e1, 1e3, 1e5, 1e7, math.inf):
        r = _condition(jtj, info, thr)
        want = [b for b in range(len(mats)) if float(r.cond[b]) > thr]
        n = int(r.flagged_count.item())
        assert n == len(want) and r.flagged_idx.cpu()[:n].tolist() == want
        assert (r.flagged_idx.cpu()[n:] == -1).all()
        assert thr == math.inf or {len(mats) - 2, len(mats) - 1} <= set(want)   # +inf is above every finite threshold


def test_flag_list_of_large_batches():
    """More samples than the 256 of one compaction chunk: the list is still ascending and complete."""
    gen = torch.Generator().manual_seed(5)
    B, d = 700, 16
    ks = torch.logspace(0, 6, B, dtype=torch.float64)[torch.randperm(B, generator=gen)]
    jtj = torch.stack([_spd(d, float(k), gen) for k in ks]).cuda()
    info = torch.zeros(B, dtype=torch.int32, device="cuda")
    for thr in (1e2, 1e4):
        r = _condition(jtj, info, thr)
        cond = r.cond.cpu()
        want = torch.nonzero(cond > thr).flatten().tolist()
        n = int(r.flagged_count.item())
        assert 0 < n < B and r.flagged_idx.cpu()[:n].tolist() == want


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return torch.equal(a, b)


def _rows(out, rows):
    if isinstance(out, dict):
        return {k: _rows(v, rows) for k, v in out.items()}
    return out[rows]


def _clone(out):
    if isinstance(out, dict):
        return {k: _clone(v) for k, v in out.items()}
    return out.clone()


def _guarded(head, guard, fn):
    head.precision_guard = guard
    try:
        return fn()
    finally:
        head.precision_guard = None


def _with_kernels(head, cfg, fn):
    saved, head.kernels = head.kernels, cfg
    try:
        return fn()
    finally:
        head.kernels = saved


def _gram(head):
    g = head.last_gram
    return {k: getattr(g, k).clone() for k in ("jtj", "logdet", "l1_off", "l1_diag", "info")}


def test_threshold_extremes_on_the_full_size_model():
    """max_condition = inf: every output (and last_gram) is bit-equal to the unguarded evaluation; max_condition = 0: bit-equal to
    the unguarded evaluation with head.kernels = fallback.  Every kwarg combination of test_elbo_matches_reference_vectors, and
    ood."""
    from cmf_amd import PrecisionGuard
    g, meta, cfg, dens = build("c3_mnist_full")
    head, model = find_head(dens), inner(dens, True)
    x = (g["x"] + g["noise"]).cuda()
    fb = PrecisionGuard().fallback
    calls = [dict(likelihood_wt=lw, metric_wt=mw, add_reconstruction=rec, add_offdiagonal_metric_reg=off,
                  add_diagonal_metric_reg=diag) for lw, mw, rec, off, diag in meta["elbo_combos"]] + [dict(ood=True)]
    with torch.no_grad():
        for kw in calls:
            run = lambda: _clone(model.elbo(x, **kw))
            plain = run()
            gram = _gram(head) if kw.get("likelihood_wt", 1.0) else None
            assert _same(_guarded(head, PrecisionGuard(math.inf), run), plain), kw
            if gram is not None:
                assert _same(_gram(head), gram) and head.last_gram.recomputed.numel() == 0
                assert torch.isfinite(head.last_gram.cond).all() and (head.last_gram.cond >= 1).all()
            # (likelihood_wt = 0 builds no Jacobian: nothing to guard, the default evaluation stands)
            fallback = _with_kernels(head, fb, run) if gram is not None else plain
            gram_fb = _gram(head) if gram is not None else None
            assert _same(_guarded(head, PrecisionGuard(0.0), run), fallback), kw
            if gram is not None:
                assert _same(_gram(head), gram_fb)
                assert head.last_gram.recomputed.tolist() == list(range(x.shape[0]))


def _mixed_batch(name, n=32, seed=0):
    g, meta, cfg, dens = build(name)
    gen = torch.Generator().manual_seed(seed)
    base = g["x"].repeat(n // g["x"].shape[0], 1, 1, 1)
    return dens, find_head(dens), (base + torch.rand(base.shape, generator=gen)).cuda()


def _median_threshold(head, model, x, **kw):
    """A threshold between the samples' estimates: cond of an unguarded-equivalent (inf) evaluation, split at the median."""
    from cmf_amd import PrecisionGuard
    with torch.no_grad():
        _guarded(head, PrecisionGuard(math.inf), lambda: model.elbo(x, **kw))
    c = head.last_gram.cond.double().sort().values
    m = c.shape[0] // 2
    assert c[m - 1] < c[m], "the batch needs samples of different conditioning"
    return float((c[m - 1] * c[m]).sqrt()), head.last_gram.cond.clone()


@pytest.mark.parametrize("nested", [False, True])
def test_mixed_batch_reruns_only_the_flagged_rows(nested):
    """Half of a 32-sample batch above the threshold.  Unflagged rows are bit-equal to the default evaluation; flagged rows are
    bit-equal to the fallback evaluation of exactly those rows (the re-run IS that evaluation).  Per-sample arithmetic is NOT
    independent of the batch composition (the primal convs group 16 samples, the f16x3 input scale is a batch maximum, jitter
    retries are whole-batch), so against the fallback evaluation of the whole batch the flagged rows agree to 1e-4 relative."""
    from cmf_amd import PrecisionGuard
    dens, head, x = _mixed_batch("c3_mnist_full")
    model = inner(dens, True)
    head.nested_prior_dict = nested
    kw = dict(add_offdiagonal_metric_reg=True)
    thr, cond = _median_threshold(head, model, x, **kw)
    rows = torch.nonzero(cond > thr).flatten()
    keep = torch.nonzero(cond <= thr).flatten()
    fb = PrecisionGuard().fallback
    with torch.no_grad():
        plain = _clone(model.elbo(x, **kw))
        guarded = _guarded(head, PrecisionGuard(thr), lambda: _clone(model.elbo(x, **kw)))
        g = head.last_gram
        assert g.recomputed.cpu().tolist() == rows.tolist() and int(g.flagged_count.item()) == rows.numel()
        assert torch.equal(g.cond[keep], cond.cuda()[keep])
        gram = _gram(head)
        sub = _with_kernels(head, fb, lambda: _clone(model.elbo(x[rows.cuda()], **kw)))
        sub_gram = _gram(head)
        whole = _with_kernels(head, fb, lambda: _clone(model.elbo(x, **kw)))
    r, k = rows.cuda(), keep.cuda()
    assert _same(_rows(guarded, k), _rows(plain, k))
    assert _same(_rows(guarded, r), sub)
    for name in gram:
        assert torch.equal(gram[name][r], sub_gram[name]), name
    assert rel(guarded["elbo"][r], whole["elbo"][r]) < 1e-4
    if nested:
        assert "bijection-info" in guarded["prior-dict"]


def test_guard_restores_the_reference_tolerance_on_the_conditioned_model():
    """The point of the feature.  On c3_mnist_full_cond (cond(J^T J) ~ 6e2, gains x 2.3) the default primal arithmetic lands
    ~1.3e-4 from the fixture's J^T J (test_gpu_round4 needs a computed 3.9e-4 bound there); with the guard on and its threshold
    below the samples' condition numbers, every sample is re-run on exact fp32 kernels and J^T J, the log-det and the elbo hold
    1e-4 of the fixture.  64 copies of the two samples (128: the grouped primal path the default takes at batch sizes of use)."""
    from cmf_amd import PrecisionGuard
    g, meta, cfg, dens = build("c3_mnist_full_cond")
    head = find_head(dens)
    rep = 64
    x = (g["x"] + g["noise"]).repeat(rep, 1, 1, 1).cuda()
    head.precision_guard = PrecisionGuard(max_condition=1.0)
    with torch.no_grad():
        out = inner(dens, True).elbo(x, add_offdiagonal_metric_reg=True)["elbo"]
    gr = head.last_gram
    assert gr.recomputed.tolist() == list(range(2 * rep))
    assert bool((gr.cond > 1.0).all()) and bool(torch.isfinite(gr.cond).all())
    for i in range(0, 2 * rep, 2):
        assert torch.equal(out[i:i + 2], out[0:2])
    assert rel(gr.jtj[0:2], g["jtj"]) < 1e-4
    assert rel(gr.logdet[0:2].view(-1, 1), g["logdet"]) < 1e-4
    assert rel(out[0:2], g["elbo_0"] if "elbo_0" in g else g["elbo"]) < 1e-4


def test_chunked_evaluation():
    """A batch split into sub-batches (TANGENT_BUDGET lowered on the instance): each chunk is guarded on its own; threshold 0
    equals the chunked fallback evaluation, inf the chunked default one; a median threshold re-runs only flagged rows."""
    from cmf_amd import PrecisionGuard
    from cmf_amd import engine as E
    dens, head, x = _mixed_batch("c3_mnist_full")
    model = inner(dens, True)
    prog = head.program
    prog.TANGENT_BUDGET = prog.tangent_bytes_per_sample(E.ceil16(prog.d)) * 16
    kw = dict(add_offdiagonal_metric_reg=True)
    fb = PrecisionGuard().fallback
    with torch.no_grad():
        run = lambda: _clone(model.elbo(x, **kw))
        plain = run()
        assert head.last_gram.jtj.shape[0] == 16                   # the batch did split
        fallback = _with_kernels(head, fb, run)
        assert _same(_guarded(head, PrecisionGuard(math.inf), run), plain)
        assert _same(_guarded(head, PrecisionGuard(0.0), run), fallback)
        assert head.last_gram.recomputed.tolist() == list(range(16))
        _guarded(head, PrecisionGuard(math.inf), run)
        c = head.last_gram.cond.double().sort().values                 # the last chunk's estimates
        thr = float((c[7] * c[8]).sqrt())
        guarded = _guarded(head, PrecisionGuard(thr), run)
    rows = head.last_gram.recomputed                                   # last chunk (rows 16 .. 31), chunk-relative
    assert 0 < rows.numel() < 16
    keep = torch.tensor([i for i in range(16) if i not in set(rows.tolist())], device="cuda")
    assert torch.equal(guarded["elbo"][16:][keep], plain["elbo"][16:][keep])
    assert rel(guarded["elbo"][16:][rows], fallback["elbo"][16:][rows]) < 1e-4


def test_lazy_mode_records_only():
    """check_cholesky = "lazy": the estimate is left on the device, nothing is re-run, the outputs equal the unguarded lazy
    evaluation bit for bit."""
    from cmf_amd import PrecisionGuard
    dens, head, x = _mixed_batch("c3_mnist_full")
    model = inner(dens, True)
    head.check_cholesky = "lazy"
    kw = dict(add_offdiagonal_metric_reg=True)
    with torch.no_grad():
        plain = _clone(model.elbo(x, **kw))
        guarded = _guarded(head, PrecisionGuard(0.0), lambda: _clone(model.elbo(x, **kw)))
    g = head.last_gram
    assert _same(guarded, plain)
    assert g.recomputed is None and int(g.flagged_count.item()) == x.shape[0]
    assert bool(torch.isfinite(g.cond).all()) and bool((g.cond >= 1).all())


def test_captured_graph_with_a_guard():
    """ElboGraph forces lazy mode during capture: a guarded head captures, and a replay equals the eager lazy evaluation."""
    from cmf_amd import PrecisionGuard
    from cmf_amd.graphs import ElboGraph
    dens, head, x = _mixed_batch("c3_mnist_full")
    model = inner(dens, True)
    kw = dict(add_offdiagonal_metric_reg=True)
    head.precision_guard = PrecisionGuard(0.0)
    graph = ElboGraph(model, x, **kw)
    out = _clone(graph(x))
    cond = head.last_gram.cond.clone()
    head.check_cholesky = "lazy"
    with torch.no_grad():
        eager = _clone(model.elbo(x, **kw))
    assert _same(out, eager)
    assert torch.equal(cond, head.last_gram.cond)


def test_wide_head_through_the_engine():
    """d = 256 from a real Gram + Cholesky (head_wide.hip) on a random Jacobian: the estimate against float64 torch, from the
    workspace path of the kernel."""
    from cmf_amd import engine as E
    gen = torch.Generator().manual_seed(11)
    B, N, d = 3, 784, 256
    J = torch.randn(B, N, d, generator=gen) * torch.logspace(0, -2, d)
    T = E.Tangent.from_dense(J.cuda(), E.ceil16(d), "panel")
    r = E.gram_cholesky(T, d)
    keep = r.jtj.clone()
    E.gram_condition(r, d, 1e3)
    assert torch.equal(r.jtj, keep)
    for b in range(B):
        want = _kappa1(r.jtj[b].cpu())
        assert 1e3 < want and abs(float(r.cond[b]) - want) <= 1e-4 * want
    assert int(r.flagged_count.item()) == B and r.flagged_idx.tolist() == list(range(B))


def test_training_is_not_guarded():
    """loss_and_gradients and elbo(...).backward() give bit-equal losses and gradients with a guard (threshold 0) and without."""
    from cmf_amd import PrecisionGuard
    g, meta, cfg, dens = build("c3_mnist_full")
    head = find_head(dens)
    model = inner(dens, True)
    x = (g["x"] + g["noise"]).cuda()
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        loss, elbo, grads = head.loss_and_gradients(x, add_offdiagonal_metric_reg=True)
        return loss.clone(), elbo.clone(), {k: v.clone() for k, v in grads.items()}

    def backward():
        for p in params:
            p.grad = None
        out = model.elbo(x, add_offdiagonal_metric_reg=True)["elbo"]
        (-out.mean()).backward()
        return out.detach().clone(), [p.grad.clone() for p in params]

    loss0, elbo0, grads0 = step()
    loss1, elbo1, grads1 = _guarded(head, PrecisionGuard(0.0), step)
    assert torch.equal(loss0, loss1) and torch.equal(elbo0, elbo1)
    assert grads0.keys() == grads1.keys() and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
    out0, pg0 = backward()
    out1, pg1 = _guarded(head, PrecisionGuard(0.0), backward)
    assert torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(pg0, pg1))
