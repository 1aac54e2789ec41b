"""The seeded residual of block 0's conv2 (``engine.SEED_RESIDUAL``, MODE 8 of csrc/conv_tangent_bf16x3.hip): the launch forms its
residual h0 = conv0(mask . v) from a one-channel seed panel in one extra K-step instead of reading the tensor the thin first conv used
to write.  Against float64, against today's two launches on the same inputs, and through the whole decode path."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_residual_plain_launch.npy")


def _mask(H, W, reverse):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = ((ii + jj) % 2 == 1).astype(np.float32)
    return torch.from_numpy((1 - m if reverse else m)[None].copy())


def _bitmask(E, live):
    """BitMask from a bool tensor (B, HW, 64): bit j of byte (b, px, o) = live[b, px, 8 o + j]."""
    B, HW, _ = live.shape
    m = E.BitMask(B, HW, C, "cuda")
    w = (live.reshape(B, HW, C // 8, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1)
    m.data.copy_(w.to(torch.uint8).cuda())
    return m


def _unslice(t):
    B, HW, nsl = t.shape[:3]
    return t.permute(0, 1, 3, 2, 4).reshape(B, HW, C, nsl * 16)


def _slice(t):
    """(B, HW, 64, nc) -> slice-major (B, HW, nc / 16, 64, 16)."""
    B, HW, _, nc = t.shape
    return t.reshape(B, HW, C, nc // 16, 16).permute(0, 1, 3, 2, 4).contiguous()


def plain_launch_inputs():
    """Seeded inputs of the plain residual launch whose bits tests/golden/seed_residual_plain_launch.npy records (written by
    tests/dev/seed_residual_gate.py --dump from the library BEFORE the seeded mode was added)."""
    gen = torch.Generator().manual_seed(20240)
    H, W, B, nc = 4, 14, 1, 16
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(H=H, W=W, B=B, nc=nc, u=rn(B, H * W, C, nc), r=rn(B, H * W, C, nc), live=rn(B, H * W, C) > 0, w2=rn(C, C, 3, 3) / 24)


def plain_launch(E, c):
    """conv2(relu'(c1) . u) + r on the split kernel, residual read from memory -> (B, HW, 64, nc)."""
    H, W, B, nc = c["H"], c["W"], c["B"], c["nc"]
    HW = H * W
    conv2 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
    with torch.no_grad():
        conv2.weight.copy_(c["w2"])
    hd, hsl = (C * HW * nc, 16, C * nc), C * 16
    bm = _bitmask(E, c["live"])
    y = torch.zeros(B, HW, nc // 16, C, 16, device="cuda")
    with E.scope(E.KernelConfig(tangent="bf16x3")):
        E.conv_tangent(_slice(c["u"]).cuda(), 0, *hd, conv2.weight, 9, y, *hd, B, C, C, H, W, nc, res_t=_slice(c["r"]).cuda(), x_sl=hsl,
                       y_sl=hsl, fmode=E.F_RELU_BITS, f=bm.data, f_np=bm.np_bytes)
    return _unslice(y).cpu()


@functools.lru_cache(maxsize=None)
def _case(H, W, B, nc, reverse, border=False):
    """Seeded inputs of one case and the float64 reference conv2(relu'(c1) . u) + conv0(mask . v), (B, HW, 64, nc)."""
    import torch.nn.functional as F
    HW = H * W
    gen = torch.Generator().manual_seed(100000 * H + 1000 * B + 10 * nc + reverse + 5 * border)
    rn = lambda *s: torch.randn(*s, generator=gen)
    v = rn(B, 1, HW, nc)
    if border:                                            # the large values on the image's border pixels
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        edge = torch.from_numpy(((ii == 0) | (ii == H - 1) | (jj == 0) | (jj == W - 1)).reshape(-1))
        v = torch.where(edge[None, None, :, None], 1000.0 * v, 0.001 * v)
    u = rn(B, HW, C, nc)
    live = rn(B, HW, C) > 0
    w0, w2 = rn(C, 1, 3, 3) / 3, rn(C, C, 3, 3) / 24
    mask = _mask(H, W, reverse)
    vm = (v.reshape(B, 1, H, W, nc) * mask[None, :, :, :, None]).permute(0, 4, 1, 2, 3).reshape(B * nc, 1, H, W).double()
    h0 = F.conv2d(vm, w0.double(), padding=1).reshape(B, nc, C, HW).permute(0, 3, 2, 1)
    ul = (u.double() * live.double().unsqueeze(-1)).permute(0, 3, 2, 1).reshape(B * nc, C, H, W)
    want = F.conv2d(ul, w2.double(), padding=1).reshape(B, nc, C, HW).permute(0, 3, 2, 1) + h0
    return dict(v=v, u=u, live=live, w0=w0, w2=w2, mask=mask, want=want)


def _nets(c):
    conv0 = torch.nn.Conv2d(1, C, 3, padding=1, bias=False).cuda()
    conv2 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
    with torch.no_grad():
        conv0.weight.copy_(c["w0"])
        conv2.weight.copy_(c["w2"])
    return conv0, conv2


def _run(E, c, H, W, B, nc, seeded, v=None, u=None, nets=None, h_fill=None):
    """h2 = conv2(relu'(c1) . u) + h0 through the engine's own calls: the seed panel + the seeded launch, or today's thin conv0 and
    the residual launch.  -> (B, HW, 64, nc)"""
    HW = H * W
    conv0, conv2 = nets or _nets(c)
    Tt = E.Tangent(B, HW, nc, "panel", "cuda", data=(c["v"] if v is None else v).contiguous().cuda().reshape(-1))
    view = E.NetView(E.Geometry((1, H, W)), 1, mask=c["mask"].cuda())
    bm = _bitmask(E, c["live"])
    factor = dict(fmode=E.F_RELU_BITS, f=bm.data, f_np=bm.np_bytes)
    ud = _slice(c["u"] if u is None else u).cuda()
    y = torch.full((B, HW, nc // 16, C, 16), float("nan"), device="cuda")
    hd, hsl = (C * HW * nc, 16, C * nc), C * 16
    with E.scope(E.KernelConfig(tangent="bf16x3")):
        if seeded:
            sd = E.seed_panel(Tt, view, H, W)
            E.conv_tangent(ud, 0, *hd, conv2.weight, 9, y, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl,
                           seed=dict(sd, pack=E._seed_pack(conv0, "cuda")), **factor)
        else:
            h = torch.empty(B * HW * C * nc, device="cuda")
            E.conv_tangent(Tt.data, 0, Tt.t_b, HW * nc, nc, conv0.weight, 9, h, *hd, B, 1, C, H, W, nc, fmode=E.F_RAW, f=view.mask, f_np=0,
                           f_ci=HW, f_px=1, y_sl=hsl)
            E.conv_tangent(ud, 0, *hd, conv2.weight, 9, y, *hd, B, C, C, H, W, nc, res_t=h, x_sl=hsl, y_sl=hsl, **factor)
    return _unslice(y).cpu()


SHAPES = [(2, 14), (4, 14), (14, 14)]
CASES = [(reverse, nc) for reverse in (False, True) for nc in (16, 48)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_seeded_launch_against_float64(H, W, B):
    """conv2(relu'(c1) . u) + conv0(mask . v) in float64 against the seeded launch and against today's two launches on the same
    inputs: the seeded launch's maximum error is at most twice today's (h0 in fp32 products both ways, one K-step more)."""
    from cmf_amd import engine as E
    for reverse, nc in CASES:
        c = _case(H, W, B, nc, reverse)
        new, old = (_run(E, c, H, W, B, nc, s).double() for s in (True, False))
        e_new, e_old = float((new - c["want"]).abs().max()), float((old - c["want"]).abs().max())
        print(f"seed_residual {H}x{W} B={B} nc={nc} reverse={reverse}: max err {e_new:.3e}, today's launches {e_old:.3e}, "
              f"max |h2| {float(c['want'].abs().max()):.2f}")
        assert bool(torch.isfinite(new).all())
        assert e_new <= 2 * e_old, (reverse, nc, e_new, e_old)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H,W", [(2, 14), (4, 14)])
def test_padding_and_mask_exactness(H, W, reverse):
    """What the masked pixels of v hold (1e30, NaN) does not change a bit of the output (no h0 buffer is passed at all), and an input
    whose large values sit on the border pixels meets the float64 reference under the bound of the test above."""
    from cmf_amd import engine as E
    B, nc = 3, 48
    c = _case(H, W, B, nc, reverse)
    nets = _nets(c)
    base = _run(E, c, H, W, B, nc, True, nets=nets)
    assert bool(torch.isfinite(base).all())
    dead = (c["mask"].reshape(1, 1, H * W, 1) == 0).expand_as(c["v"])
    for poison in (1e30, float("nan")):
        v = torch.where(dead, torch.full_like(c["v"], poison), c["v"])
        assert torch.equal(_run(E, c, H, W, B, nc, True, v=v, nets=nets), base), poison
    cb = _case(H, W, B, nc, reverse, True)
    new, old = (_run(E, cb, H, W, B, nc, s).double() for s in (True, False))
    e_new, e_old = float((new - cb["want"]).abs().max()), float((old - cb["want"]).abs().max())
    print(f"seed_residual border {H}x{W} reverse={reverse}: max err {e_new:.3e}, today's launches {e_old:.3e}, "
          f"max |h2| {float(cb['want'].abs().max()):.2f}")
    assert e_new <= 2 * e_old, (e_new, e_old)


@pytest.mark.parametrize("reverse", [False, True])
def test_slot_batch_and_nc_independence(reverse):
    """Bit identity of a column's output: slot 35 of nc = 48, slot 3 of nc = 16 and slot 60 of nc = 64 (other columns: different
    data); sample 1 of B = 3 on its own."""
    from cmf_amd import engine as E
    H, W, B = 14, 14, 3
    c = _case(H, W, B, 48, reverse)
    nets = _nets(c)
    full = _run(E, c, H, W, B, 48, True, nets=nets)
    gen = torch.Generator().manual_seed(7)
    for nc, slot in ((16, 3), (64, 60)):
        v, u = torch.randn(B, 1, H * W, nc, generator=gen), torch.randn(B, H * W, C, nc, generator=gen)
        v[..., slot], u[..., slot] = c["v"][..., 35], c["u"][..., 35]
        other = _run(E, c, H, W, B, nc, True, v=v, u=u, nets=nets)
        assert torch.equal(other[..., slot], full[..., 35]), (nc, slot)
    one = dict(c, v=c["v"][1:2], u=c["u"][1:2], live=c["live"][1:2])
    assert torch.equal(_run(E, one, H, W, 1, 48, True, nets=nets)[0], full[1])


def test_bad_arguments_are_rejected():
    """A residual next to the seed, a float factor, a short column plane."""
    from cmf_amd import engine as E
    H, W, B, nc = 2, 14, 1, 16
    c = _case(H, W, B, nc, False)
    conv0, conv2 = _nets(c)
    HW = H * W
    Tt = E.Tangent(B, HW, nc, "panel", "cuda", data=c["v"].contiguous().cuda().reshape(-1))
    view = E.NetView(E.Geometry((1, H, W)), 1, mask=c["mask"].cuda())
    bm = _bitmask(E, c["live"])
    hd, hsl = (C * HW * nc, 16, C * nc), C * 16
    ud, y = _slice(c["u"]).cuda(), torch.zeros(B * HW * C * nc, device="cuda")
    with E.scope(E.KernelConfig(tangent="bf16x3")):
        sd = dict(E.seed_panel(Tt, view, H, W), pack=E._seed_pack(conv0, "cuda"))
        short = dict(sd, col=(H + 2) * (W + 2))
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.conv_tangent(ud, 0, *hd, conv2.weight, 9, y, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, seed=short, fmode=E.F_RELU_BITS,
                           f=bm.data, f_np=bm.np_bytes)
        with pytest.raises(AssertionError):
            E.conv_tangent(ud, 0, *hd, conv2.weight, 9, y, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, seed=sd, res_t=y, fmode=E.F_RELU_BITS,
                           f=bm.data, f_np=bm.np_bytes)


def test_plain_residual_launch_keeps_its_bits():
    """A residual launch of the split kernel that does not take the seeded mode gives the bits the library gave before that mode was
    added (recorded once from that build on the same seeded inputs)."""
    from cmf_amd import engine as E
    got = plain_launch(E, plain_launch_inputs()).numpy()
    want = np.load(GOLDEN)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_whole_path_with_the_seeded_residual(monkeypatch):
    """C3 fixture samples repeated to B = 32: with SEED_RESIDUAL on, J, J^T J, log-det and g_ij stay within test_gpu_parity's tolerance
    of the float64 oracle; x_hat is bit-identical on and off.  Per Jacobian sweep the switch trades three thin first convs for three
    seed panels (= three seeded launches); a training step, a vjp and the exact-fp32 tangent kernels take none."""
    from cmf_amd import _lib, engine as E
    from conftest import kink_tolerance
    from test_gpu_fold_head import _oracle64
    from test_gpu_parity import find_head, inner, rel
    name, B = "c3_mnist_full", 32
    g, dens, p64 = _oracle64(name)
    head = find_head(dens)
    dequant = "noise" in g
    x0 = (g["x"] + g["noise"]) if dequant else g["x"]
    n = x0.shape[0]
    reps = -(-B // n)
    x = x0.repeat(reps, *([1] * (x0.dim() - 1)))[:B].cuda()
    z64 = p64["z_low"].float().repeat(reps, 1)[:B].cuda()

    def run():
        inner(dens, dequant).elbo(x, add_offdiagonal_metric_reg=True)
        gr = head.last_gram
        with _lib.trace() as rec:
            x_hat, J = head.jacobian(z64)
        names = [r[0] for r in rec]
        return dict(x_hat=x_hat.clone(), J=J.clone(), jtj=gr.jtj.clone(), logdet=gr.logdet.clone().view(-1, 1), l1=gr.l1_off.clone().view(-1, 1),
                    thin=names.count("cmf_conv_tangent"), panels=names.count("cmf_seed_panel"))

    with torch.no_grad():
        out = {}
        for on in (True, False):
            monkeypatch.setattr(E, "SEED_RESIDUAL", on)
            out[on] = run()
        errs = {k: (rel(out[True][k][:n], p64[k]), rel(out[False][k][:n], p64[k])) for k in ("J", "jtj", "logdet", "l1")}
        print(f"seed_residual whole path {name} B={B}: relative error vs float64, on / off: "
              + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items())
              + f"; fp32-kernel launches {out[True]['thin']} / {out[False]['thin']}, seed panels {out[True]['panels']} / {out[False]['panels']}")
        tol = kink_tolerance(g, 1e-4)
        for k in ("J", "jtj", "logdet", "l1"):
            assert errs[k][0] < tol, (k, errs[k], tol)
        assert torch.equal(out[True]["x_hat"], out[False]["x_hat"])
        assert out[True]["panels"] == 3 and out[False]["panels"] == 0
        assert out[False]["thin"] - out[True]["thin"] == 3
        monkeypatch.setattr(E, "SEED_RESIDUAL", True)
        # not engaged under the exact-fp32 tangent kernels, in a vjp or in a training step
        kernels, head.kernels = head.kernels, E.KernelConfig(tangent="f32")
        try:
            with _lib.trace() as rec:
                head.jacobian(z64)
        finally:
            head.kernels = kernels
        assert not any(r[0] == "cmf_seed_panel" for r in rec)
        with _lib.trace() as rec:
            head.vjp_forward(z64, torch.ones_like(out[True]["x_hat"]))
        assert len(rec) > 0 and not any(r[0] == "cmf_seed_panel" for r in rec)
    with torch.enable_grad(), _lib.trace() as rec:
        dens.zero_grad()
        (-inner(dens, dequant).elbo(x.clone())["elbo"].mean()).backward()
    assert len(rec) > 0 and not any(r[0] == "cmf_seed_panel" for r in rec)


def test_switch_off_changes_nothing_else(monkeypatch):
    """The switch acts through the couplers that take the seeded launch and through nothing else: with no coupler eligible (no wired
    probe-front shape) the small fixture's elbo dict is the same bits with the switch on and off."""
    from cmf_amd import engine as E
    monkeypatch.setattr(E, "PROBE_FRONT_SHAPES", set())
    from test_gpu_fold_head import _oracle64
    from test_gpu_parity import inner
    g, dens, _ = _oracle64("mini_mnist")
    dequant = "noise" in g
    x = ((g["x"] + g["noise"]) if dequant else g["x"]).cuda()
    with torch.no_grad():
        out = {}
        for on in (True, False):
            monkeypatch.setattr(E, "SEED_RESIDUAL", on)
            out[on] = {k: v.clone() for k, v in inner(dens, dequant).elbo(x, add_offdiagonal_metric_reg=True).items() if torch.is_tensor(v)}
    assert out[True].keys() == out[False].keys() and len(out[True]) > 0
    for k in out[True]:
        assert torch.equal(out[True][k], out[False][k]), k


@pytest.mark.parametrize("reverse", [False, True])
def test_pack_and_panel_match_their_host_restatements(reverse):
    """The device pack of conv0's weight and the seed panel are, bit for bit, what engine.seed_pack_host / engine.seed_panel_index
    state (tests/test_seed_residual_layout.py checks those against the MFMA operand layout on the CPU)."""
    from cmf_amd import engine as E
    H, W, B, nc = 4, 14, 3, 48
    c = _case(H, W, B, nc, reverse)
    conv0, _ = _nets(c)
    pack = E._seed_pack(conv0, "cuda").cpu().numpy().view(np.float32).reshape(4, 64, 4)
    assert np.array_equal(pack, E.seed_pack_host(c["w0"].numpy()))
    v = torch.where((c["mask"].reshape(1, 1, H * W, 1) == 0).expand_as(c["v"]), torch.full_like(c["v"], float("nan")), c["v"])
    Tt = E.Tangent(B, H * W, nc, "panel", "cuda", data=v.contiguous().cuda().reshape(-1))
    sd = E.seed_panel(Tt, E.NetView(E.Geometry((1, H, W)), 1, mask=c["mask"].cuda()), H, W)
    got = sd["panel"].cpu().reshape(B, nc, sd["col"])
    idx = torch.from_numpy(E.seed_panel_index(H, W))
    keep = (idx >= 0) & (c["mask"].reshape(-1)[idx.clamp_min(0)] != 0)
    want = torch.where(keep[None, None, :], c["v"][:, 0].permute(0, 2, 1)[:, :, idx.clamp_min(0)], torch.zeros(()))
    assert sd["col"] == E.seed_plane(H, W) and torch.equal(got, want)
