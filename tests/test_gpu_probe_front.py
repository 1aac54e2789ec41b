"""The probe front of a checkerboard coupler's tangent network (csrc/probe_front.hip, ``engine.PROBE_FRONT``): block 0's conv1 on one
probe column per input class plus the apply kernel, against float64, against today's launch on every column, and through the whole
decode path."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
SENTINEL = 12345.0
#: forward bound of an n <= 26-term fp32 fmaf sum, (n + 1) 2^-24 sum |R T|
BOUND = 27 * 2.0 ** -24


def _mask(cin, H, W, reverse):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = ((ii + jj) % 2 == 1).astype(np.float32)
    return np.broadcast_to(1 - m if reverse else m, (cin, H, W)).copy()


def _plan(E, cin, H, W, reverse):
    host = E.probe_plan(_mask(cin, H, W, reverse))
    assert host is not None
    return host, {"ns": host["ns"], "cls": torch.from_numpy(host["cls"]).cuda(), "probes": torch.from_numpy(host["probes"]).reshape(-1).cuda()}


def _bitmask(E, live):
    """BitMask from a bool tensor (B, HW, 64), built by hand: bit j of byte (b, px, o) = live[b, px, 8 o + j]."""
    B, HW, _ = live.shape
    m = E.BitMask(B, HW, C, "cuda")
    w = (live.reshape(B, HW, C // 8, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1)
    m.data.copy_(w.to(torch.uint8).cuda())
    return m


def _apply_ref(R, T, cls, cin, H, W):
    """float64: R (B, HW, ncls, 64), T (B, cin, HW, nc) -> (sum, sum of absolute values), each (B, HW, 64, nc)."""
    HW = H * W
    out, out_abs = (torch.zeros(R.shape[0], HW, C, T.shape[-1], dtype=torch.float64) for _ in range(2))
    p = torch.arange(HW)
    r, col = p // W, p % W
    cls = torch.from_numpy(np.asarray(cls)).long().reshape(cin, HW)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok = (r + dy >= 0) & (r + dy < H) & (col + dx >= 0) & (col + dx < W)
            for c in range(cin):
                q = (p + dy * W + dx).clamp(0, HW - 1)
                sel = ok & (cls[c, q] >= 0)
                ps, qs = p[sel], q[sel]
                term = R[:, ps, cls[c, qs], :, None] * T[:, c, qs, None, :]
                out[:, ps] += term
                out_abs[:, ps] += term.abs()
    return out, out_abs


def _unslice(t):
    B, HW, nsl = t.shape[:3]
    return t.permute(0, 1, 3, 2, 4).reshape(B, HW, C, nsl * 16)


@functools.lru_cache(maxsize=None)
def _case(H, W, B, nc, cin, reverse):
    """Seeded inputs of one case and both float64 references: the apply formula on a random R, and the whole front."""
    import torch.nn.functional as F
    from cmf_amd import engine as E
    host, plan = _plan(E, cin, H, W, reverse)
    HW, ncls = H * W, 16 * host["ns"]
    gen = torch.Generator().manual_seed(100000 * H + 1000 * B + 10 * nc + 2 * cin + reverse)
    rn = lambda *s: torch.randn(*s, generator=gen)
    R = rn(B, HW, ncls, C)
    T = rn(B, cin, HW, nc)
    live = rn(B, HW, C) > 0
    a0 = rn(B, C, H, W)
    w0, w1 = rn(C, cin, 3, 3) / 3, rn(C, C, 3, 3) / 24
    want, want_abs = _apply_ref(R.double(), T.double(), host["cls"], cin, H, W)
    # the whole front in float64: conv1(relu'(a0) . conv0(mask . v)) per column
    mask = torch.from_numpy(_mask(cin, H, W, reverse))
    v = (T.reshape(B, cin, H, W, nc) * mask[None, :, :, :, None]).permute(0, 4, 1, 2, 3).reshape(B * nc, cin, H, W).double()
    h0 = F.conv2d(v, w0.double(), padding=1).reshape(B, nc, C, H, W) * (a0 > 0).double()[:, None]
    u0 = F.conv2d(h0.reshape(B * nc, C, H, W), w1.double(), padding=1).reshape(B, nc, C, HW).permute(0, 3, 2, 1)
    return dict(host=host, plan=plan, R=R, T=T, live=live, a0=a0, w0=w0, w1=w1, mask=mask, want=want, want_abs=want_abs, u0=u0)


def _apply(E, c, H, W, B, nc, cin, R=None, ymask=True, T=None):
    """The apply kernel alone -> (B, HW, 64, nc), rows it does not write = SENTINEL."""
    plan, HW = c["plan"], H * W
    ns = plan["ns"]
    Rd = (c["R"] if R is None else R).reshape(B, HW, ns, 16, C).permute(0, 1, 2, 4, 3).contiguous().cuda()
    Td = (c["T"] if T is None else T).contiguous().cuda()
    y = torch.full((B, HW, nc // 16, C, 16), SENTINEL, device="cuda")
    E.probe_apply(Rd, HW * C * 16 * ns, C * 16 * ns, Td, 0, cin * HW * nc, HW * nc, nc, plan["cls"], y, C * HW * nc, C * nc, B, cin, H, W,
                  nc, ns, ymask=_bitmask(E, c["live"]) if ymask else None)
    return _unslice(y).cpu()


def _nets(c, cin):
    conv0 = torch.nn.Conv2d(cin, C, 3, padding=1, bias=False).cuda()
    conv1 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
    with torch.no_grad():
        conv0.weight.copy_(c["w0"])
        conv1.weight.copy_(c["w1"])
    return conv0, conv1


def _front(E, c, H, W, B, nc, cin, probe, ymask=True, T=None, nets=None):
    """u_0 through the engine's own calls: today's two launches (thin conv0, conv1 on every column) or the probe front."""
    HW = H * W
    conv0, conv1 = nets or _nets(c, cin)
    Tt = E.Tangent(B, cin * HW, nc, "panel", "cuda", data=(c["T"] if T is None else T).contiguous().cuda().reshape(-1))
    view = E.NetView(E.Geometry((cin, H, W)), cin, mask=c["mask"].cuda(), probe=c["plan"])
    a0 = c["a0"].cuda().contiguous()
    factor = dict(fmode=E.F_RELU, f=a0, f_np=C * HW, f_ci=HW, f_px=1, f_group=1)
    ym = _bitmask(E, c["live"]) if ymask else None
    u = torch.full((B, HW, nc // 16, C, 16), SENTINEL, device="cuda")
    hd, hsl = (C * HW * nc, 16, C * nc), C * 16
    with E.scope(E.KernelConfig(tangent="bf16x3")):
        if probe:
            scratch = torch.full((B * HW * C * 16 * c["plan"]["ns"],), float("nan"), device="cuda")
            E.probe_front(conv0, conv1, Tt, view, c["plan"], factor, ym, scratch, u, H, W)
        else:
            h = torch.empty(B * HW * C * nc, device="cuda")
            E.conv_tangent(Tt.data, 0, Tt.t_b, HW * nc, nc, conv0.weight, 9, h, *hd, B, cin, C, H, W, nc, fmode=E.F_RAW, f=view.mask, f_np=0,
                           f_ci=HW, f_px=1, y_sl=hsl)
            E.conv_tangent(h, 0, *hd, conv1.weight, 9, u, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, ymask=ym, **factor)
    return _unslice(u).cpu()


CASES = [(cin, reverse, nc) for cin in (1, 2) for reverse in (False, True) for nc in (16, 48)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 14), (14, 14)])
def test_apply_kernel_against_float64(H, W, B):
    """Given R, T and the masks: every live row within (n + 1) 2^-24 sum |R T| of float64, every dead row untouched."""
    from cmf_amd import engine as E
    for cin, reverse, nc in CASES:
        c = _case(H, W, B, nc, cin, reverse)
        got = _apply(E, c, H, W, B, nc, cin).double()
        live = c["live"].unsqueeze(-1).expand_as(got)
        err, bound = (got - c["want"]).abs()[live], BOUND * c["want_abs"][live]
        print(f"probe_apply {H}x{W} B={B} nc={nc} cin={cin} reverse={reverse}: max err {float(err.max()):.3e}, "
              f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool(torch.isfinite(got).all())
        assert bool((err <= bound).all()), (cin, reverse, nc)
        assert bool((got[~live] == SENTINEL).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 14), (14, 14)])
def test_whole_substitution_against_float64(H, W, B):
    """conv1(relu'(a0) . conv0(mask . v)) in float64 against the probe front and against today's launch on the same inputs: the
    probe front's maximum error is at most twice today's (the same split-precision products plus one fp32 summation stage)."""
    from cmf_amd import engine as E
    for cin, reverse, nc in CASES:
        c = _case(H, W, B, nc, cin, reverse)
        live = c["live"].unsqueeze(-1).expand(B, H * W, C, nc)
        new, old = (_front(E, c, H, W, B, nc, cin, probe).double() for probe in (True, False))
        e_new, e_old = float((new - c["u0"]).abs()[live].max()), float((old - c["u0"]).abs()[live].max())
        print(f"probe_front {H}x{W} B={B} nc={nc} cin={cin} reverse={reverse}: max err {e_new:.3e}, today's launch {e_old:.3e}, "
              f"max |u0| {float(c['u0'].abs().max()):.2f}")
        assert bool(torch.isfinite(new[live]).all())
        assert bool((new[~live] == SENTINEL).all()) and bool((old[~live] == SENTINEL).all())
        assert e_new <= 2 * e_old, (cin, reverse, nc, e_new, e_old)


@pytest.mark.parametrize("cin,reverse", [(1, False), (2, True)])
def test_slot_batch_and_nc_independence(cin, reverse):
    """Bit identity of a column's output: slot 35 of nc = 48 and slot 3 of nc = 16 (other columns: different data); sample 1 of B = 3
    on its own."""
    from cmf_amd import engine as E
    H, W, B = 14, 14, 3
    c = _case(H, W, B, 48, cin, reverse)
    nets = _nets(c, cin)
    full = _front(E, c, H, W, B, 48, cin, True, nets=nets)
    gen = torch.Generator().manual_seed(7)
    T16 = torch.randn(B, cin, H * W, 16, generator=gen)
    T16[..., 3] = c["T"][..., 35]
    small = _front(E, c, H, W, B, 16, cin, True, T=T16, nets=nets)
    assert torch.equal(small[..., 3], full[..., 35])
    one = dict(c, T=c["T"][1:2], a0=c["a0"][1:2], live=c["live"][1:2])
    alone = _front(E, one, H, W, 1, 48, cin, True, nets=nets)
    assert torch.equal(alone[0], full[1])
    # the apply kernel alone: the same two properties on a given R
    full = _apply(E, c, H, W, B, 48, cin)
    assert torch.equal(_apply(E, c, H, W, B, 16, cin, T=T16)[..., 3], full[..., 35])
    assert torch.equal(_apply(E, dict(c, live=c["live"][1:2]), H, W, 1, 48, cin, R=c["R"][1:2], T=c["T"][1:2])[0], full[1])


@pytest.mark.parametrize("cin,reverse", [(1, True), (2, False)])
def test_dead_rows(cin, reverse):
    """Rows with a clear bit keep the sentinel; what the dead rows of R hold (0, 1e30, NaN) does not change a bit of the output; the
    filtered and the unfiltered form agree on every live row."""
    from cmf_amd import engine as E
    H, W, B, nc = 4, 14, 3, 48
    c = _case(H, W, B, nc, cin, reverse)
    base = _apply(E, c, H, W, B, nc, cin)
    live = c["live"].unsqueeze(-1).expand_as(base)
    assert bool((base[~live] == SENTINEL).all()) and bool((base[live] != SENTINEL).any())
    dead = ~c["live"][:, :, None, :].expand_as(c["R"])
    for poison in (0.0, 1e30, float("nan")):
        R = torch.where(dead, torch.full_like(c["R"], poison), c["R"])
        assert torch.equal(_apply(E, c, H, W, B, nc, cin, R=R), base), poison
    every = _apply(E, c, H, W, B, nc, cin, ymask=False)
    assert bool((every != SENTINEL).all()) and torch.equal(every[live], base[live])
    new, new_all = _front(E, c, H, W, B, nc, cin, True), _front(E, c, H, W, B, nc, cin, True, ymask=False)
    assert bool((new[~live] == SENTINEL).all()) and torch.equal(new[live], new_all[live])


@pytest.mark.parametrize("what", ["cin 3", "nc 24", "three slices of R", "short mask", "misaligned rows"])
def test_bad_arguments_are_rejected(what):
    from cmf_amd import engine as E
    H, W, B, nc, cin, ns = 4, 14, 1, 16, 1, 1
    HW = H * W
    R, T = torch.zeros(B, HW, 3, C, 16, device="cuda"), torch.zeros(B, 3, HW, 32, device="cuda")
    cls = torch.full((3 * HW,), -1, dtype=torch.int8, device="cuda")
    y = torch.zeros(B, HW, 2, C, 16, device="cuda")
    ym = E.BitMask(B, HW, C, "cuda")
    t_off = 0
    if what == "cin 3":
        cin = 3
    elif what == "nc 24":
        nc = 24
    elif what == "three slices of R":
        ns = 3
    elif what == "short mask":
        ym.np_bytes = HW * 8 - 8
    else:
        t_off = 2
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.probe_apply(R, HW * C * 16 * 3, C * 16 * 3, T, t_off, 3 * HW * 32, HW * 32, 32, cls, y, C * HW * 32, C * 32, B, cin, H, W, nc, ns, ymask=ym)


@pytest.mark.parametrize("name,B,shapes", [("mini_mnist", 16, None), ("c3_mnist_full", 32, None), ("c3_mnist_full", 32, "every checkerboard")])
def test_whole_path_with_the_probe_front(name, B, shapes, monkeypatch):
    """Fixture samples repeated to B: with PROBE_FRONT on, J, J^T J, log-det and g_ij stay within test_gpu_parity's tolerance
    (conftest.kink_tolerance(g, 1e-4)) of the float64 oracle; x_hat is bit-identical on and off; with it on, toggling SKIP_DEAD_ROWS,
    CHECKERBOARD_TAIL or FlowProgram.SEED_COLUMNS changes no bit.  The apply kernel runs for exactly the couplers of the wired shapes
    (or, second C3 row, of every checkerboard shape with a plan), and never under tangent="f32"."""
    from cmf_amd import engine as E
    from cmf_amd.densities import FlowProgram
    from conftest import kink_tolerance
    from test_gpu_fold_head import _oracle64
    from test_gpu_parity import find_head, inner, rel
    g, dens, p64 = _oracle64(name)
    head = find_head(dens)
    dequant = "noise" in g
    x0 = (g["x"] + g["noise"]) if dequant else g["x"]
    n = x0.shape[0]
    reps = -(-B // n)
    x = x0.repeat(reps, *([1] * (x0.dim() - 1)))[:B].cuda()
    z64 = p64["z_low"].float().repeat(reps, 1)[:B].cuda()
    if shapes is not None:
        monkeypatch.setattr(E, "PROBE_FRONT_SHAPES", {(28, 28, 1), (14, 14, 2), (14, 14, 1), (28, 28, 2)})
    calls, eligible = [], []
    probe_apply, net_tangent = E.probe_apply, E.net_tangent

    def counting(*a, **k):
        calls.append(1)
        return probe_apply(*a, **k)

    def watching(net, T, view, acts, **k):
        if net.kind == "resnet" and view.probe is not None:
            conv0 = E._resnet_parts(net)[0]
            eligible.append(conv0.out_channels == 64 and (view.geom.H, view.geom.W, view.cin) in E.PROBE_FRONT_SHAPES
                            and T.nc > 16 * view.probe["ns"])
        return net_tangent(net, T, view, acts, **k)

    monkeypatch.setattr(E, "probe_apply", counting)
    monkeypatch.setattr(E, "net_tangent", watching)

    def run():
        inner(dens, dequant).elbo(x, add_offdiagonal_metric_reg=True)
        gr = head.last_gram
        del calls[:], eligible[:]
        x_hat, J = head.jacobian(z64)
        return dict(x_hat=x_hat.clone(), J=J.clone(), jtj=gr.jtj.clone(), logdet=gr.logdet.clone().view(-1, 1), l1=gr.l1_off.clone().view(-1, 1),
                    applied=len(calls), eligible=sum(eligible))

    with torch.no_grad():
        out = {}
        for on in (True, False):
            monkeypatch.setattr(E, "PROBE_FRONT", on)
            out[on] = run()
        errs = {k: (rel(out[True][k][:n], p64[k]), rel(out[False][k][:n], p64[k])) for k in ("J", "jtj", "logdet", "l1")}
        print(f"probe_front whole path {name} B={B} shapes={shapes}: relative error vs float64, on / off: "
              + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items()) + f"; apply launches {out[True]['applied']}")
        tol = kink_tolerance(g, 1e-4)
        for k in ("J", "jtj", "logdet", "l1"):
            assert errs[k][0] < tol, (k, errs[k], tol)
        assert torch.equal(out[True]["x_hat"], out[False]["x_hat"])
        assert out[True]["applied"] == out[True]["eligible"] and out[False]["applied"] == 0
        if name == "c3_mnist_full":
            assert out[True]["applied"] == (3 if shapes is None else 7), out[True]["applied"]
        monkeypatch.setattr(E, "PROBE_FRONT", True)
        for owner, switch in ((E, "SKIP_DEAD_ROWS"), (E, "CHECKERBOARD_TAIL"), (FlowProgram, "SEED_COLUMNS")):
            monkeypatch.setattr(owner, switch, False)
            other = run()
            monkeypatch.setattr(owner, switch, True)
            for k in ("x_hat", "J", "jtj", "logdet", "l1"):
                assert torch.equal(other[k], out[True][k]), (switch, k)
        # not engaged under the exact-fp32 tangent kernels
        kernels, head.kernels = head.kernels, E.KernelConfig(tangent="f32")
        try:
            del calls[:]
            head.jacobian(z64)
        finally:
            head.kernels = kernels
        assert len(calls) == 0
