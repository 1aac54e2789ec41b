"""The folded block of a coupler's tangent network (csrc/conv_block_head.hip, ``engine.FOLD_BLOCK``): the last residual block's
conv1, its conv2 and the 1x1 output conv as one launch over the block's input h -- against float64, against today's two launches
(conv1 with its store filter + the folded head), across forms and slots, with poisoned dead rows, with a loud border, and through
the whole decode path."""
import functools

import pytest
import torch

from test_fold_block_host import HID as C, dead_rows, direct, live_sel

pytestmark = pytest.mark.gpu


def _to_dev(t, nc):
    """(B, C, H, W, nc) -> slice-major [sample][pixel][slice][channel][16] on the device."""
    B, Cc = t.shape[:2]
    return t.reshape(B, Cc, -1, nc // 16, 16).permute(0, 2, 3, 1, 4).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _case(H, W, B, nc, border=False):
    """Seeded inputs and the float64 reference on every pixel for cout = 4 (cout = 2: its first two rows), computed once.
    ``border``: |h| ~ 1e3 in the outermost two rings of the image, ~ 1 inside."""
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + 100003 * B + nc + (5 if border else 0))
    rn = lambda *s: torch.randn(*s, generator=gen)
    h = rn(B, C, H, W, nc)
    if border:
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[2:-2, 2:-2] = False
        h = h * torch.where(ring, 1e3, 1.0).view(1, 1, H, W, 1)
    a_in, c1, aK = rn(B, C, H, W), rn(B, C, H, W), rn(B, C, H, W)
    w1, w2, wf = rn(C, C, 3, 3) / 24, rn(C, C, 3, 3) / 24, rn(4, C) / 8
    want = direct(h, a_in > 0, c1 > 0, aK > 0, w1, w2, wf)
    return dict(h=h, a_in=a_in, c1=c1, aK=aK, w1=w1, w2=w2, wf=wf, want=want)


def _params(c, cout):
    from torch.nn import Parameter
    key = ("params", cout)
    if key not in c:                                     # the same Parameter objects on every call: the W1 pack stays cached
        c[key] = (Parameter(c["w1"].cuda()), Parameter(c["w2"].cuda()), Parameter(c["wf"][:cout].reshape(cout, C, 1, 1).contiguous().cuda()))
    return c[key]


def _fold_block(h_dev, a_in, c1, aK, w1, w2, wf, H, W, nc, live):
    """The new launch -> (B, cout, pixels (compact under live), nc)."""
    from cmf_amd import engine as E
    B, cout, HWo = h_dev.shape[0], wf.shape[0], H * W // (2 if live else 1)
    ma, m1 = E.relu_bits(a_in.cuda()), E.relu_bits(c1.cuda())
    yt = torch.full((B, cout, HWo, nc), float("nan"), device="cuda")
    st = (C * H * W * nc, 16, C * nc)
    E.conv_tangent(h_dev, 0, *st, w2, 9, yt, cout * HWo * nc, HWo * nc, nc, B, C, C, H, W, nc, x_sl=C * 16, live=live, precision="bf16x3",
                   fmode=E.F_RELU_BITS, f=ma.data, f_np=ma.np_bytes,
                   head=dict(weight=wf, act=aK.cuda().contiguous(), conv1=dict(weight=w1, mask=m1)))
    return yt


def _today(h_dev, a_in, c1, aK, w1, w2, wf, H, W, nc, live):
    """Today's pair: conv1 with c1's store filter, then the folded head -> (B, cout, pixels (compact under live), nc)."""
    from cmf_amd import engine as E
    B, cout, HWo = h_dev.shape[0], wf.shape[0], H * W // (2 if live else 1)
    ma, m1 = E.relu_bits(a_in.cuda()), E.relu_bits(c1.cuda())
    st, sl = (C * H * W * nc, 16, C * nc), C * 16
    u = torch.zeros_like(h_dev)
    E.conv_tangent(h_dev, 0, *st, w1, 9, u, *st, B, C, C, H, W, nc, x_sl=sl, y_sl=sl, precision="bf16x3", fmode=E.F_RELU_BITS, f=ma.data,
                   f_np=ma.np_bytes, ymask=m1)
    yt = torch.full((B, cout, HWo, nc), float("nan"), device="cuda")
    E.conv_tangent(u, 0, *st, w2, 9, yt, cout * HWo * nc, HWo * nc, nc, B, C, C, H, W, nc, res_t=h_dev, res_np=st[0], x_sl=sl, live=live,
                   precision="bf16x3", fmode=E.F_RELU_BITS, f=m1.data, f_np=m1.np_bytes, head=dict(weight=wf, act=aK.cuda().contiguous()))
    return yt


def _both_errors(c, H, W, nc, cout, live, tag):
    w1, w2, wf = _params(c, cout)
    sel = live_sel(H, W, live)
    want = c["want"][:, :cout][:, :, sel]
    h_dev = _to_dev(c["h"], nc)
    got = _fold_block(h_dev, c["a_in"], c["c1"], c["aK"], w1, w2, wf, H, W, nc, live).cpu().double()
    old = _today(h_dev, c["a_in"], c["c1"], c["aK"], w1, w2, wf, H, W, nc, live).cpu().double()
    err, err_old = float((got - want).abs().max()), float((old - want).abs().max())
    print(f"fold_block {tag} {H}x{W} B={c['h'].shape[0]} nc={nc} cout={cout} live={live}: max err {err:.3e}, today's two launches "
          f"{err_old:.3e}, ratio {err / err_old:.2f} (max |want| {float(want.abs().max()):.3e})")
    assert bool(torch.isfinite(got).all())
    return err, err_old


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(2, 14), (4, 14), (14, 14)])
def test_folded_block_against_float64(H, W, B):
    """nc in {16, 48}, cout in {2, 4}, live in {1, 2}: the maximum error against the float64 composition is at most twice that of
    today's two launches on the same inputs against the same reference (the project's factor for a re-ordered sum)."""
    for nc in (16, 48):
        c = _case(H, W, B, nc)
        for cout in (2, 4):
            for live in (1, 2):
                err, err_old = _both_errors(c, H, W, nc, cout, live, "kernel")
                assert err <= 2.0 * err_old, (nc, cout, live, err, err_old)


def test_form_and_slot_independence():
    """Bit identity: compact output = the live pixels of the full output; a column in slot 3 of nc = 16 and in slot 35 of nc = 48;
    a sample alone (B = 1) and inside B = 3."""
    H, W = 14, 14
    c = _case(H, W, 3, 48)
    w1, w2, wf = _params(c, 4)
    run = lambda h_dev, a_in, c1, aK, nc, live: _fold_block(h_dev, a_in, c1, aK, w1, w2, wf, H, W, nc, live)
    h48 = _to_dev(c["h"], 48)
    full = run(h48, c["a_in"], c["c1"], c["aK"], 48, 0)
    assert bool(torch.isfinite(full).all())
    for live in (1, 2):
        assert torch.equal(run(h48, c["a_in"], c["c1"], c["aK"], 48, live), full[:, :, live_sel(H, W, live).cuda()])
    gen = torch.Generator().manual_seed(7)
    h16 = torch.randn(3, C, H, W, 16, generator=gen)
    h16[..., 3] = c["h"][..., 35]
    for live in (0, 1):
        small = run(_to_dev(h16, 16), c["a_in"], c["c1"], c["aK"], 16, live)
        big = full if not live else full[:, :, live_sel(H, W, live).cuda()]
        assert torch.equal(small[..., 3], big[..., 35])
    one = lambda t: t[1:2].contiguous()
    alone = run(one(h48), one(c["a_in"]), one(c["c1"]), one(c["aK"]), 48, 0)
    assert torch.equal(alone[0], full[1])


@pytest.mark.parametrize("live", [0, 1, 2])
def test_dead_rows_are_neither_fetched_nor_multiplied(live):
    """The rows of h the formula multiplies by an exact zero -- relu'(a_in) clear, and not the centre of an output pixel whose
    relu'(a) is set -- filled with 0, 1e30 and NaN: the same bits each time."""
    H, W, nc = 4, 14, 16
    c = _case(H, W, 3, nc)
    w1, w2, wf = _params(c, 2)
    dead = dead_rows(c["a_in"] > 0, c["aK"] > 0, live_sel(H, W, live)).reshape(3, C, H, W, 1)
    assert bool(dead.any())
    outs = [_fold_block(_to_dev(torch.where(dead, torch.full_like(c["h"], fill), c["h"]), nc), c["a_in"], c["c1"], c["aK"], w1, w2, wf,
                        H, W, nc, live) for fill in (0.0, 1e30, float("nan"))]
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("live", [1, 2])
def test_border_rings(live):
    """|h| ~ 1e3 in the outermost two rings only: a contribution from outside the image, or a border row under the wrong offset,
    would stand out.  Same bound as the kernel test."""
    H, W, nc = 14, 14, 16
    c = _case(H, W, 1, nc, True)
    for cout in (2, 4):
        err, err_old = _both_errors(c, H, W, nc, cout, live, "border")
        assert err <= 2.0 * err_old, (cout, err, err_old)


def test_whole_path_with_the_folded_block(monkeypatch):
    """c3_mnist_full repeated to B = 32.  With FOLD_BLOCK on, J, J^T J, log-det and g_ij stay within kink_tolerance(g, 1e-4) of the
    float64 oracle and within twice the error with the switch off; x_hat is bit-identical; the hidden 3x3 launches of a Jacobian
    sweep fall by exactly the number of couplers whose shape is in FOLD_BLOCK_SHAPES; exact-fp32 tangents, B = 2, ``save`` and the
    reverse sweep take none; an ElboGraph replay equals the eager result."""
    from cmf_amd import engine as E
    from cmf_amd.graphs import ElboGraph
    from conftest import kink_tolerance
    from test_gpu_fold_head import _head_input, _oracle64
    from test_gpu_parity import find_head, inner, rel
    name, B = "c3_mnist_full", 32
    g, dens, p64 = _oracle64(name)
    head = find_head(dens)
    dequant = "noise" in g
    x0 = (g["x"] + g["noise"]) if dequant else g["x"]
    n = x0.shape[0]
    x = x0.repeat(B // n, *([1] * (x0.dim() - 1))).cuda()
    z64 = p64["z_low"].float().repeat(B // n, 1).cuda()
    calls, captured, eligible = [], [], []
    conv_tangent, net_tangent = E.conv_tangent, E.net_tangent

    def counting(*a, **k):
        hd = k.get("head")
        calls.append(dict(block=hd is not None and "conv1" in hd, hidden=a[6] == 9 and a[12] == 64 and a[13] == 64))
        return conv_tangent(*a, **k)

    def capturing(net, T, view, acts, **k):
        before = sum(c["block"] for c in calls)
        if net.kind == "resnet":
            conv0, blocks, convf = E._resnet_parts(net)
            eligible.append(view.live is not None and conv0.out_channels == 64 and len(blocks) >= 2
                            and (view.geom.H, view.geom.W, convf.out_channels) in E.FOLD_BLOCK_SHAPES)
        out = net_tangent(net, T, view, acts, **k)
        if sum(c["block"] for c in calls) > before and not captured:
            captured.append((net, T, view, acts))
        return out

    monkeypatch.setattr(E, "conv_tangent", counting)
    monkeypatch.setattr(E, "net_tangent", capturing)
    kw = dict(add_offdiagonal_metric_reg=True)
    out = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(E, "FOLD_BLOCK", on)
            eager = inner(dens, dequant).elbo(x, **kw)
            gr = head.last_gram
            z_low = head.program.encode(_head_input(dens, head, x, dequant))[0]
            del calls[:], eligible[:]
            x_hat, J = head.jacobian(z64)
            out[on] = dict(x_hat=x_hat.clone(), J=J[:n].cpu(), jtj=gr.jtj[:n].cpu(), logdet=gr.logdet[:n].view(-1, 1).cpu(),
                           l1=gr.l1_off[:n].view(-1, 1).cpu(), block=sum(c["block"] for c in calls), hidden=sum(c["hidden"] for c in calls),
                           eligible=sum(eligible), elbo=eager["elbo"].clone())
        errs = {k: (rel(out[True][k], p64[k]), rel(out[False][k], p64[k])) for k in ("J", "jtj", "logdet", "l1")}
        print(f"fold_block whole path {name} B={B}: relative error vs float64, on / off: "
              + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items())
              + f"; folded blocks {out[True]['block']}, hidden launches {out[True]['hidden']} / {out[False]['hidden']}")
        tol = kink_tolerance(g, 1e-4)
        for k in ("J", "jtj", "logdet", "l1"):
            assert errs[k][0] < tol, (k, errs[k], tol)
            assert errs[k][0] <= 2.0 * errs[k][1], (k, errs[k])
        assert torch.equal(out[True]["x_hat"], out[False]["x_hat"])
        assert out[False]["block"] == 0 and out[True]["block"] == out[True]["eligible"]
        assert out[False]["hidden"] - out[True]["hidden"] == out[True]["eligible"]
        assert (out[True]["eligible"] > 0) == bool(E.FOLD_BLOCK_SHAPES)
        # not engaged: exact-fp32 tangents, a batch that is no multiple of 16 (float activations), training (save), the reverse sweep
        monkeypatch.setattr(E, "FOLD_BLOCK", True)
        block = lambda: sum(c["block"] for c in calls)
        del calls[:]
        kernels, head.kernels = head.kernels, E.KernelConfig(tangent="f32")
        try:
            head.jacobian(z_low)
        finally:
            head.kernels = kernels
        assert len(calls) > 0 and block() == 0
        del calls[:]
        head.jacobian(z_low[:2])
        assert len(calls) > 0 and block() == 0
        if captured:
            net, T, view, acts = captured[0]
            del calls[:]
            net_tangent(net, T, view, acts)
            assert block() == 1
            del calls[:]
            net_tangent(net, T, view, acts, save=[])
            assert len(calls) > 0 and block() == 0
        del calls[:]
        head.program.vjp(z_low, torch.randn(B, out[True]["x_hat"][0].numel(), 3, device="cuda"))
        assert len(calls) > 0 and block() == 0
        # ElboGraph replay == eager
        m = inner(dens, dequant)
        eager = {k: v.clone() for k, v in m.elbo(x.clone(), **kw).items() if torch.is_tensor(v)}
        replay = {k: v.clone() for k, v in ElboGraph(m, x, **kw)(x).items() if torch.is_tensor(v)}
        for k in eager:
            assert torch.equal(eager[k], replay[k]), k
