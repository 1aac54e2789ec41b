"""The folded head of a coupler's tangent network (csrc/conv_head.hip, ``engine.FOLD_HEAD``): the last hidden 3x3 conv and the 1x1
output conv behind it as one fp32 launch, against float64, against today's two launches, and through the whole decode path."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
#: first-order bound of a 64-term dot (E) nested in a 640 + 64-term dot, in units of the same formula on absolute values
BOUND = 710 * 2.0 ** -24


def _to_dev(t, nc):
    """(B, C, H, W, nc) -> slice-major [sample][pixel][slice][channel][16] on the device."""
    B, Cc = t.shape[:2]
    return t.reshape(B, Cc, -1, nc // 16, 16).permute(0, 2, 3, 1, 4).contiguous().cuda()


def _sel(H, W, live):
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.ones(H * W, dtype=torch.bool) if not live else ((ii + jj) % 2 == live - 1).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(H, W, B, nc):
    """Inputs (seeded) and the float64 h_K = conv2(relu'(c1) u) + h with its absolute-value twin, shared by every cout / live."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + 100003 * B + nc)
    u = torch.randn(B, C, H, W, nc, generator=gen)
    h = torch.randn(B, C, H, W, nc, generator=gen)
    c1 = torch.randn(B, C, H, W, generator=gen)
    aK = torch.randn(B, C, H, W, generator=gen)
    w2 = torch.randn(C, C, 3, 3, generator=gen) / 24
    wf = torch.randn(8, C, generator=gen) / 8
    m1 = (c1 > 0).unsqueeze(-1)
    img = lambda t: t.permute(0, 4, 1, 2, 3).reshape(B * nc, C, H, W).double()
    back = lambda t: t.reshape(B, nc, C, H * W).permute(0, 2, 3, 1)                    # (B, C, HW, nc)
    hK = back(F.conv2d(img(u * m1), w2.double(), padding=1) + img(h))
    hK_abs = back(F.conv2d(img(u.abs() * m1), w2.abs().double(), padding=1) + img(h.abs()))
    mK = (aK > 0).reshape(B, C, H * W, 1).double()
    u_nan = torch.where(m1, u, torch.full_like(u, float("nan")))                      # dead rows: never to be touched
    return dict(u=u, h=h, c1=c1, aK=aK, w2=w2, wf=wf, hK=hK * mK, hK_abs=hK_abs * mK, u_dev=_to_dev(u_nan, nc), h_dev=_to_dev(h, nc))


def _fold(u_dev, h_dev, c1, aK, w2, wf, H, W, nc, live):
    """The folded launch -> (B, cout, pixels (compact under live), nc)."""
    from cmf_amd import engine as E
    B, cout, HWo = u_dev.shape[0], wf.shape[0], H * W // (2 if live else 1)
    bits = E.relu_bits(c1.cuda())
    yt = torch.full((B, cout, HWo, nc), float("nan"), device="cuda")
    st = (C * H * W * nc, 16, C * nc)
    E.conv_tangent(u_dev, 0, *st, torch.nn.Parameter(w2.cuda()), 9, yt, cout * HWo * nc, HWo * nc, nc, B, C, C, H, W, nc, res_t=h_dev,
                   res_np=st[0], x_sl=C * 16, live=live, precision="bf16x3", fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes,
                   head=dict(weight=torch.nn.Parameter(wf.reshape(cout, C, 1, 1).cuda()), act=aK.cuda().contiguous()))
    return yt


def _two_launches(u_dev, h_dev, c1, aK, w2, wf, H, W, nc):
    """Today's path on every pixel: split-precision conv2 with its residual, then the 1x1 conv -> (B, cout, HW, nc)."""
    from cmf_amd import engine as E
    B, cout, HW = u_dev.shape[0], wf.shape[0], H * W
    bits = E.relu_bits(c1.cuda())
    st, sl = (C * HW * nc, 16, C * nc), C * 16
    hK = torch.empty_like(h_dev)
    E.conv_tangent(u_dev, 0, *st, torch.nn.Parameter(w2.cuda()), 9, hK, *st, B, C, C, H, W, nc, res_t=h_dev, x_sl=sl, y_sl=sl,
                   precision="bf16x3", fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes)
    yt = torch.empty(B, cout, HW, nc, device="cuda")
    E.conv_tangent(hK, 0, *st, torch.nn.Parameter(wf.reshape(cout, C, 1, 1).cuda()), 1, yt, cout * HW * nc, HW * nc, nc, B, C, cout, H, W,
                   nc, fmode=E.F_RELU, f=aK.cuda().contiguous(), x_sl=sl, f_np=C * HW, f_ci=HW, f_px=1)
    return yt


@pytest.mark.parametrize("live", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 14), (14, 14), (8, 8)])
def test_folded_head_against_float64(H, W, B, live):
    """Every nc in {16, 48} and cout in {2, 4, 6}: per element within 710 * 2^-24 of the formula on absolute values, dead rows of u
    holding NaN, and a maximum error no larger than that of the two-launch path against the same float64 reference."""
    sel = _sel(H, W, live)
    for nc in (16, 48):
        c = _case(H, W, B, nc)
        for cout in (2, 4, 6):
            wf = c["wf"][:cout]
            want = torch.einsum("oc,bcpn->bopn", wf.double(), c["hK"])[:, :, sel]
            bound = BOUND * torch.einsum("oc,bcpn->bopn", wf.abs().double(), c["hK_abs"])[:, :, sel]
            got = _fold(c["u_dev"], c["h_dev"], c["c1"], c["aK"], c["w2"], wf, H, W, nc, live).cpu().double()
            old = _two_launches(c["u_dev"], c["h_dev"], c["c1"], c["aK"], c["w2"], wf, H, W, nc).cpu().double()[:, :, sel]
            err, err_old = (got - want).abs(), (old - want).abs()
            print(f"fold_head {H}x{W} B={B} nc={nc} cout={cout} live={live}: max err {float(err.max()):.3e} "
                  f"(worst err / bound {float((err / bound).max()):.3f}), two launches {float(err_old.max()):.3e}")
            assert bool(torch.isfinite(got).all())
            assert bool((err <= bound).all()), (nc, cout, float((err / bound).max()))
            assert float(err.max()) <= float(err_old.max()), (nc, cout)


def test_form_and_slot_independence():
    """Bit identity: compact output = the live pixels of the full output; a column in slot 3 of nc = 16 and in slot 35 of nc = 48;
    a sample alone (B = 1) and inside B = 3."""
    H, W = 14, 14
    c = _case(H, W, 3, 48)
    wf = c["wf"][:4]
    run = lambda u_dev, h_dev, c1, aK, nc, live: _fold(u_dev, h_dev, c1, aK, c["w2"], wf, H, W, nc, live)
    full = run(c["u_dev"], c["h_dev"], c["c1"], c["aK"], 48, 0)
    for live in (1, 2):
        assert torch.equal(run(c["u_dev"], c["h_dev"], c["c1"], c["aK"], 48, live), full[:, :, _sel(H, W, live).cuda()])
    # slot 35 of nc = 48 -> slot 3 of nc = 16 (the other columns: different data)
    gen = torch.Generator().manual_seed(7)
    u16, h16 = torch.randn(3, C, H, W, 16, generator=gen), torch.randn(3, C, H, W, 16, generator=gen)
    u16[..., 3], h16[..., 3] = c["u"][..., 35], c["h"][..., 35]
    u16 = torch.where((c["c1"] > 0).unsqueeze(-1), u16, torch.full_like(u16, float("nan")))
    for live in (0, 1):
        small = run(_to_dev(u16, 16), _to_dev(h16, 16), c["c1"], c["aK"], 16, live)
        big = full if not live else full[:, :, _sel(H, W, live).cuda()]
        assert torch.equal(small[..., 3], big[..., 35])
    # sample 1 of B = 3 on its own
    one = lambda t: t[1:2].contiguous()
    alone = run(one(c["u_dev"]), one(c["h_dev"]), one(c["c1"]), one(c["aK"]), 48, 0)
    assert torch.equal(alone[0], full[1])


@pytest.mark.parametrize("what", ["hidden width 32", "cout 9", "no bit mask"])
def test_unsupported_heads_are_rejected(what):
    from cmf_amd import engine as E
    H, W, nc, B = 4, 14, 16, 1
    hid = 32 if what == "hidden width 32" else C
    cout = 9 if what == "cout 9" else 2
    u, h = torch.zeros(B, H * W, 1, hid, 16, device="cuda"), torch.zeros(B, H * W, 1, hid, 16, device="cuda")
    c1, aK = torch.ones(B, hid, H, W, device="cuda"), torch.ones(B, hid, H, W, device="cuda")
    bits = E.relu_bits(c1)
    fk = dict(fmode=E.F_RELU, f=c1, f_np=hid * H * W, f_ci=H * W, f_px=1) if what == "no bit mask" else \
        dict(fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes)
    yt = torch.zeros(B, cout, H * W, nc, device="cuda")
    st = (hid * H * W * nc, 16, hid * nc)
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.conv_tangent(u, 0, *st, torch.nn.Parameter(torch.zeros(hid, hid, 3, 3, device="cuda")), 9, yt, cout * H * W * nc, H * W * nc, nc,
                       B, hid, hid, H, W, nc, res_t=h, res_np=st[0], x_sl=hid * 16, precision="bf16x3",
                       head=dict(weight=torch.nn.Parameter(torch.zeros(cout, hid, 1, 1, device="cuda")), act=aK), **fk)


@functools.lru_cache(maxsize=None)
def _oracle64(name):
    """The float64 oracle's J, J^T J, log-det and g_ij of a full-size fixture (its own two samples)."""
    from conftest import golden_model
    from oracle import cmf_oracle as O
    from test_gpu_parity import build
    g, meta, cfg, dens = build(name)
    _, _, _, ops, sd = golden_model(meta)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        p = O.elbo(sd64, ops, g["x"].double(), noise=g["noise"].double() if "noise" in g else None, add_offdiagonal_metric_reg=True,
                   return_parts=True)["parts"]
    return g, dens, {k: p[k] for k in ("J", "jtj", "logdet", "l1", "z_low")}


@pytest.mark.parametrize("name,B", [("c3_mnist_full", 32), ("c5_cifar_full", 16)])
def test_whole_path_with_the_folded_head(name, B, monkeypatch):
    """Fixture samples repeated to B: with FOLD_HEAD on, J, J^T J, log-det and g_ij stay within test_gpu_parity's tolerance
    (conftest.kink_tolerance(g, 1e-4), as that file takes it) of the float64 oracle; x_hat is bit-identical on and off (the primal
    pass is untouched); exactly the checkerboard couplers with a 64-wide network and cout <= 8 take the folded launch (7 per
    Jacobian sweep on C3) -- and none does under tangent="f32", at B = 2 or with ``save`` (training)."""
    from cmf_amd import engine as E
    from conftest import kink_tolerance
    from test_gpu_parity import find_head, inner, rel
    g, dens, p64 = _oracle64(name)
    head = find_head(dens)
    dequant = "noise" in g
    x0 = (g["x"] + g["noise"]) if dequant else g["x"]
    n = x0.shape[0]
    assert B % n == 0
    x = x0.repeat(B // n, *([1] * (x0.dim() - 1))).cuda()
    z64 = p64["z_low"].float().repeat(B // n, 1).cuda()
    calls, captured, eligible = [], [], []
    conv_tangent, net_tangent = E.conv_tangent, E.net_tangent

    def counting(*a, **k):
        calls.append(k.get("head") is not None)
        return conv_tangent(*a, **k)

    def capturing(net, T, view, acts, **k):
        before = sum(calls)
        if net.kind == "resnet":
            conv0, _, convf = E._resnet_parts(net)
            eligible.append(view.live is not None and conv0.out_channels == 64 and convf.out_channels <= 8)
        out = net_tangent(net, T, view, acts, **k)
        if sum(calls) > before and not captured:              # the first network whose head was folded (C5 has wider heads too)
            captured.append((net, T, view, acts))
        return out

    monkeypatch.setattr(E, "conv_tangent", counting)
    monkeypatch.setattr(E, "net_tangent", capturing)
    out = {}
    with torch.no_grad():
        for fold in (True, False):
            monkeypatch.setattr(E, "FOLD_HEAD", fold)
            del calls[:]
            inner(dens, dequant).elbo(x, add_offdiagonal_metric_reg=True)
            gr = head.last_gram
            z_low = head.program.encode(_head_input(dens, head, x, dequant))[0]
            # J at the ORACLE's latent (no encode rounding in between, as test_gpu_parity takes it); log-det and g_ij end to end
            del calls[:], eligible[:]
            x_hat, J = head.jacobian(z64)                                  # one Jacobian sweep: the launches counted below
            out[fold] = dict(x_hat=x_hat.clone(), J=J[:n].cpu(), jtj=gr.jtj[:n].cpu(), logdet=gr.logdet[:n].view(-1, 1).cpu(),
                             l1=gr.l1_off[:n].view(-1, 1).cpu(), folded=sum(calls), eligible=sum(eligible))
        errs = {k: (rel(out[True][k], p64[k]), rel(out[False][k], p64[k])) for k in ("J", "jtj", "logdet", "l1")}
        print(f"fold_head whole path {name} B={B}: relative error vs float64, folded / two launches: "
              + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items()) + f"; folded launches {out[True]['folded']}")
        assert out[True]["J"].shape == p64["J"].shape
        tol = kink_tolerance(g, 1e-4)
        for k in ("J", "jtj", "logdet", "l1"):
            assert errs[k][0] < tol, (k, errs[k], tol)
        assert torch.equal(out[True]["x_hat"], out[False]["x_hat"])
        assert out[True]["folded"] == out[True]["eligible"] > 0 and out[False]["folded"] == 0
        assert name != "c3_mnist_full" or out[True]["folded"] == 7
        # not engaged: exact-fp32 tangents, a batch that is no multiple of 16 (float activations), training (save)
        monkeypatch.setattr(E, "FOLD_HEAD", True)
        del calls[:]
        kernels, head.kernels = head.kernels, E.KernelConfig(tangent="f32")
        try:
            head.jacobian(z_low)
        finally:
            head.kernels = kernels
        assert len(calls) > 0 and sum(calls) == 0
        del calls[:]
        head.jacobian(z_low[:2])
        assert len(calls) > 0 and sum(calls) == 0
        del calls[:]
        net, T, view, acts = captured[0]
        net_tangent(net, T, view, acts)
        assert sum(calls) == 1
        del calls[:]
        net_tangent(net, T, view, acts, save=[])
        assert len(calls) > 0 and sum(calls) == 0


def _head_input(dens, head, x, dequant):
    """The tensor the non-square head sees for the batch ``x`` (the wrappers in front of it applied)."""
    from test_gpu_parity import inner
    m = inner(dens, dequant)
    while m is not head:
        x = m.bijection.x_to_z(x)["z"]
        m = m.prior
    return x
