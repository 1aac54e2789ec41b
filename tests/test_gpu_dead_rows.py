"""relu-dead rows of the hidden tangent convs (cmf_conv_tangent_bf16x3): a CMF_F_RELU_BITS launch does not FETCH the (channel,
pixel) rows of its input whose mask bit is clear, and a launch with a store filter (``ymask``) does not WRITE the rows of its
output that its only reader will not fetch.  Everything here is bit for bit (``torch.equal``): a dead row used to contribute
``x * 0`` and now contributes an exact 0, nothing else changes.  Every call goes through the C ABI."""
import pytest
import torch

from test_gpu_parity import build, find_head, rel

pytestmark = pytest.mark.gpu

C = 64
SENTINEL = 0x7FC0DEAD                                     # a NaN bit pattern: a reader that multiplies instead of skipping shows it


def _items_per_sample(H, W, nc):
    th, tw = (2, 14) if W % 14 == 0 else (4, 8)
    return (H // th) * (W // tw) * (nc // 16)


def _batch_for(H, W, nc, per_wg):
    """Smallest B whose busiest workgroup streams through ``per_wg`` work items (one persistent workgroup per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = _items_per_sample(H, W, nc)
    B = ((per_wg - 1) * cus) // per + 1
    assert (per_wg - 1) * cus < B * per <= per_wg * cus, (B, per, cus)
    return B


def _problem(B, H, W, nc, seed):
    """x and a residual in the slice-major hidden layout [sample][pixel][slice][channel][16], the primal activation, the weight."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    S, HW = nc // 16, H * W
    x = torch.randn(B, HW, S, C, 16, device="cuda", generator=gen)
    res = torch.randn(B, HW, S, C, 16, device="cuda", generator=gen)
    prim = torch.randn(B, C, H, W, device="cuda", generator=gen)
    w = torch.nn.Parameter(torch.randn(C, C, 3, 3, device="cuda", generator=gen) / 24)
    return x, res, prim, w


def _dead(prim):
    """(B, HW, 1, C, 1) bool: the rows of a slice-major tensor that relu'(prim) switches off."""
    B, _, H, W = prim.shape
    return (prim <= 0).reshape(B, C, H * W).permute(0, 2, 1).reshape(B, H * W, 1, C, 1)


def _launch(E, x, w, y, B, H, W, nc, fk, res=None, live=0, ymask=None):
    HW = H * W
    st, sl = (C * HW * nc, 16, C * nc), C * 16
    yst = (st[0] // 2, st[1], st[2]) if live else st
    E.conv_tangent(x, 0, *st, w, 9, y, *yst, B, C, C, H, W, nc, res_t=res, res_np=st[0], x_sl=sl, y_sl=sl, precision="bf16x3",
                   live=live, ymask=ymask, **fk)
    return y


def _factor(E, prim, kind):
    B, _, H, W = prim.shape
    if kind == "bits":
        m = E.relu_bits(prim)
        return m, dict(fmode=E.F_RELU_BITS, f=m.data, f_np=m.np_bytes)
    return None, dict(fmode=E.F_RELU, f=prim, f_np=C * H * W, f_ci=H * W, f_px=1)


@pytest.mark.parametrize("per_wg", [1, 2, 3])
@pytest.mark.parametrize("live", [0, 1, 2])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("H,W,nc", [(28, 28, 32), (14, 14, 64), (32, 32, 32)])
def test_dead_rows_are_not_used(H, W, nc, with_res, live, per_wg):
    """One bit-mask launch on x and on copies of x whose dead rows hold 0, 1e30 and NaN: the four outputs are identical, and
    identical to the float-factor launch (CMF_F_RELU, the unchanged code path) on the original x.  2 x 14 tiles at 28 x 28 and
    14 x 14, 4 x 8 tiles at 32 x 32; full and checkerboard output; 1, 2 and 3 work items per workgroup (the loader's register
    sets and its mask look-ahead run across item boundaries)."""
    from cmf_amd import engine as E
    B = _batch_for(H, W, nc, per_wg)
    x, res, prim, w = _problem(B, H, W, nc, seed=H * 1000 + nc * 10 + live)
    res = res if with_res else None
    dead = _dead(prim)
    assert 0.4 < float(dead.float().mean()) < 0.6
    _, fbits = _factor(E, prim, "bits")
    _, frelu = _factor(E, prim, "relu")
    shape = (B, H * W // 2 if live else H * W, nc // 16, C, 16)
    new = lambda: torch.full(shape, float("nan"), device="cuda")
    want = _launch(E, x, w, new(), B, H, W, nc, frelu, res, live)
    assert torch.isfinite(want).all()
    got = _launch(E, x, w, new(), B, H, W, nc, fbits, res, live)
    assert torch.equal(got, want), rel(got, want)
    for poison in (0.0, 1e30, float("nan")):
        xp = torch.where(dead, torch.full_like(x, poison), x)
        got = _launch(E, xp, w, new(), B, H, W, nc, fbits, res, live)
        assert torch.equal(got, want), (poison, int((got != want).sum()))


@pytest.mark.parametrize("kind", ["bits", "relu"])
@pytest.mark.parametrize("H,W,nc,B", [(28, 28, 32, 10), (14, 14, 64, 5), (32, 32, 32, 3), (4, 14, 16, 2)])
def test_dead_rows_are_not_written(H, W, nc, B, kind):
    """conv1 with the store filter into a tensor pre-filled with a sentinel bit pattern: live rows == the launch without the filter,
    dead rows still hold the sentinel; conv2 reading that tensor through the same mask (full and checkerboard forms) == conv2
    reading the fully stored one."""
    from cmf_amd import engine as E
    x, res, prim, w = _problem(B, H, W, nc, seed=H + W + nc)
    prim2 = torch.randn(prim.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    _, f1 = _factor(E, prim, kind)                           # conv1's own input factor: float (block 0) or bit mask
    m2, f2 = _factor(E, prim2, "bits")                       # relu'(c1): conv1's store filter = conv2's input factor
    dead = _dead(prim2).expand(x.shape)
    shape = x.shape
    full = _launch(E, x, w, torch.empty(shape, device="cuda"), B, H, W, nc, f1)
    filt = torch.empty(shape, device="cuda")
    filt.view(torch.int32).fill_(SENTINEL)
    _launch(E, x, w, filt, B, H, W, nc, f1, ymask=m2)
    assert torch.equal(filt[~dead], full[~dead])
    assert bool((filt.view(torch.int32)[dead] == SENTINEL).all())
    for live in (0, 1, 2):
        oshape = (B, H * W // 2 if live else H * W, nc // 16, C, 16)
        a = _launch(E, full, w, torch.empty(oshape, device="cuda"), B, H, W, nc, f2, res, live)
        b = _launch(E, filt, w, torch.empty(oshape, device="cuda"), B, H, W, nc, f2, res, live)
        assert torch.isfinite(b).all() and torch.equal(a, b), live


def test_store_filter_is_rejected_where_it_is_not_built():
    """ymask with a residual, with checkerboard output, without an input factor or with too short a mask: CMF_EINVAL."""
    from cmf_amd import engine as E
    B, H, W, nc = 1, 4, 14, 16
    x, res, prim, w = _problem(B, H, W, nc, seed=1)
    m, fbits = _factor(E, prim, "bits")
    y = torch.empty_like(x)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _launch(E, x, w, y, B, H, W, nc, fbits, res=res, ymask=m)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _launch(E, x, w, torch.empty(B, H * W // 2, 1, C, 16, device="cuda"), B, H, W, nc, fbits, live=1, ymask=m)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _launch(E, x, w, y, B, H, W, nc, dict(fmode=E.F_SELF_RELU), ymask=m)
    short = E.BitMask(B, H * W // 2, C, "cuda")
    with pytest.raises(RuntimeError, match="invalid argument"):
        _launch(E, x, w, y, B, H, W, nc, fbits, ymask=short)


def _batch(g, n, seed=11):
    x0 = g["head_input"].float() if "head_input" in g else g["x"].float()
    gen = torch.Generator().manual_seed(seed)
    x = x0[torch.randint(0, x0.shape[0], (n,), generator=gen)]
    return (x + 0.01 * torch.randn(x.shape, generator=gen)).cuda()


def _count_filtered(E, monkeypatch):
    """Counts the conv_tangent calls that carry a store filter."""
    n = [0]
    inner = E.conv_tangent

    def counting(*a, **kw):
        n[0] += kw.get("ymask") is not None
        return inner(*a, **kw)
    monkeypatch.setattr(E, "conv_tangent", counting)
    return n


@pytest.mark.parametrize("tangent", ["bf16x3", "f32"])
@pytest.mark.parametrize("name,B", [("c3_mnist_full", 2), ("c3_mnist_full", 32), ("c5_cifar_full", 16), ("mini_cifar", 16)])
def test_whole_path_is_bit_identical_with_and_without_the_store_filter(name, B, tangent, monkeypatch):
    """elbo dict, x_hat, J, J^T J, log-det and g_ij with ``engine.SKIP_DEAD_ROWS`` on == off, eager and through an ElboGraph replay;
    under the exact-fp32 tangent kernels the filter does not engage at all.  The filter ENGAGES (asserted below) for c3_mnist_full
    B = 32 and c5_cifar_full B = 16 under bf16x3 only: those rows are the coverage.  c3_mnist_full B = 2 (no grouped primal pass, so
    float activations) and mini_cifar (8 hidden channels) only pin that the switch changes nothing where the filter cannot run."""
    from cmf_amd import engine as E
    from cmf_amd.graphs import ElboGraph
    g, meta, cfg, dens = build(name)
    head = find_head(dens)
    head.kernels = E.KernelConfig(tangent=tangent)
    prog = head.program
    x = _batch(g, B)
    kw = dict(add_reconstruction=True, add_offdiagonal_metric_reg=True)
    n = _count_filtered(E, monkeypatch)
    out = {}
    with torch.no_grad():
        z_low = prog.encode(x)[0]
        for on in (True, False):
            monkeypatch.setattr(E, "SKIP_DEAD_ROWS", on)
            n[0] = 0
            x_hat, T = prog.decode(z_low, tangents=True)
            gr = E.gram_cholesky(T, prog.d)
            elbo = {k: v.clone() for k, v in head.elbo(x.clone(), **kw).items() if torch.is_tensor(v)}
            replay = {k: v.clone() for k, v in ElboGraph(head, x, **kw)(x).items() if torch.is_tensor(v)}
            out[on] = dict(x_hat=x_hat.clone(), J=T.to_dense(prog.d).clone(), jtj=gr.jtj.clone(), logdet=gr.logdet.clone(),
                           l1=gr.l1_off.clone(), **{"elbo." + k: v for k, v in elbo.items()}, **{"replay." + k: v for k, v in replay.items()})
            if not on or tangent != "bf16x3":
                assert n[0] == 0, (on, tangent, n[0])
            elif B % 16 == 0 and name.endswith("_full"):            # 64 hidden channels, bit masks from the grouped primal pass
                assert n[0] > 0
    assert set(out[True]) == set(out[False]) and "elbo.elbo" in out[True]
    for k in out[True]:
        assert torch.equal(out[True][k], out[False][k]), (name, B, tangent, k, rel(out[True][k], out[False][k]))


def test_training_keeps_full_stores_and_runs_the_new_loader(monkeypatch):
    """A training step of the full-size C3 model (64 hidden channels, B = 32: the forward tangent sweep takes relu' from the ActList's
    bit masks, 2 - 3 work items per workgroup, every hidden tangent saved for the reverse sweep and the weight gradients).
    * The bit-mask loader runs (CMF_F_RELU_BITS launches > 0) and NO launch carries a store filter, with the switch on or off:
      ``net_cotangent`` and the weight gradients read every row of the saved u.
    * elbo and gradients with the switch on == off (identical where the step itself repeats bit for bit).
    * Against a step that does not go through the new loader -- the activations forced to the float form, so every hidden tangent
      conv takes the float factor CMF_F_RELU (the unchanged code path): the elbo is ``torch.equal`` (the forward sweep's kernels are
      bit-identical between the two factor forms, test_dead_rows_are_not_used), the gradients agree within 1e-4, the tolerance of every
      Cholesky-path gradient test of this suite (the backward passes of the two forms read grouped / per-sample activations through
      different kernels, so they are not bit-identical by construction)."""
    from cmf_amd import engine as E
    g, meta, cfg, dens = build("c3_mnist_full")
    head = find_head(dens)
    x = _batch(g, 32)
    kw = dict(add_offdiagonal_metric_reg=True)
    n = _count_filtered(E, monkeypatch)
    counting = E.conv_tangent
    nbits = [0]

    def counting_bits(*a, **k):
        nbits[0] += k.get("fmode") == E.F_RELU_BITS
        return counting(*a, **k)
    monkeypatch.setattr(E, "conv_tangent", counting_bits)
    monkeypatch.setattr(E, "SKIP_DEAD_ROWS", False)
    _, elbo_a, grads_a = head.loss_and_gradients(x.clone(), **kw)
    _, elbo_a2, grads_a2 = head.loss_and_gradients(x.clone(), **kw)
    assert n[0] == 0 and nbits[0] > 0, (n[0], nbits[0])
    monkeypatch.setattr(E, "SKIP_DEAD_ROWS", True)
    n[0] = nbits[0] = 0
    _, elbo_b, grads_b = head.loss_and_gradients(x.clone(), **kw)
    print(f"training step, switch on: {nbits[0]} bit-mask launches, {n[0]} with a store filter")
    assert n[0] == 0 and nbits[0] >= 100, (n[0], nbits[0])          # 9 couplers x 15 hidden convs behind block 0's conv1
    assert torch.equal(elbo_a, elbo_b) and set(grads_a) == set(grads_b)
    exact = 0
    for p in grads_a:
        spread = rel(grads_a2[p], grads_a[p])
        if spread == 0.0:
            assert torch.equal(grads_b[p], grads_a[p]), (tuple(p.shape), rel(grads_b[p], grads_a[p]))
            exact += 1
        else:
            assert rel(grads_b[p], grads_a[p]) <= 2 * spread, (tuple(p.shape), rel(grads_b[p], grads_a[p]), spread)
    assert exact > 0
    # the same step on float activations: no bit-mask launch, the float-factor loader everywhere
    monkeypatch.setattr(E, "train_acts_mode", lambda *a, **k: True)
    n[0] = nbits[0] = 0
    _, elbo_f, grads_f = head.loss_and_gradients(x.clone(), **kw)
    assert n[0] == 0 and nbits[0] == 0, (n[0], nbits[0])
    worst = max(rel(grads_b[p], grads_f[p]) for p in grads_f)
    print(f"bit-mask loader vs float factor: elbo equal {torch.equal(elbo_b, elbo_f)} (rel {rel(elbo_b, elbo_f):.1e}), worst gradient {worst:.1e}")
    assert torch.equal(elbo_b, elbo_f), rel(elbo_b, elbo_f)
    assert set(grads_f) == set(grads_b) and worst < 1e-4, worst
