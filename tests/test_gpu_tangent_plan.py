"""Every ``engine.TangentPlan`` of one small checkerboard coupler on the device: 1 -> 64 -> 2 at 4 x 14 (the smallest image all the
kernels involved take), B = 16 (the primal pass writes bit masks), nc = 32 (two slices: more than the probe plan's one).  Each plan is
reached by the switches; the planner's answer, the launches made, the output's form and its error against a float64 composition of
the same network on the same relu masks are checked."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_fold_block_host import direct, live_sel

pytestmark = pytest.mark.gpu

C, H, W, B, NC, COUT = 64, 4, 14, 16, 32, 2
SWITCHES = ("CHECKERBOARD_TAIL", "SKIP_DEAD_ROWS", "FOLD_HEAD", "FOLD_BLOCK", "PROBE_FRONT", "SEED_RESIDUAL")
#: name -> (switches that are on, the plan two blocks get)
PLANS = {
    "all-plain": ((), (False, "plain", "plain", False)),
    "live": (("CHECKERBOARD_TAIL", "SKIP_DEAD_ROWS"), (True, "plain", "live", True)),
    "head": (("CHECKERBOARD_TAIL", "SKIP_DEAD_ROWS", "FOLD_HEAD"), (True, "plain", "head", True)),
    "head-full": (("FOLD_HEAD",), (False, "plain", "head", False)),
    "block": (("CHECKERBOARD_TAIL", "SKIP_DEAD_ROWS", "FOLD_HEAD", "FOLD_BLOCK"), (True, "plain", "block", True)),
    "probe": (("SKIP_DEAD_ROWS", "PROBE_FRONT"), (True, "probe", "plain", False)),
    "seeded": (("SKIP_DEAD_ROWS", "PROBE_FRONT", "SEED_RESIDUAL"), (True, "seeded", "plain", False)),
    "all-on": (SWITCHES, (True, "seeded", "block", True)),
}


def _bits(m):
    """BitMask -> bool (B, C, H, W): bit j of byte (b, px, o) = channel 8 o + j (the inverse of test_gpu_seed_residual._bitmask)."""
    d = m.data.cpu().to(torch.int32)
    return ((d.unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(B, H, W, C).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _case(nb):
    """The coupler with ``nb`` blocks, its primal activations, a random tangent stack and the float64 reference on every pixel."""
    from cmf_amd import engine as E, networks
    from test_gpu_seed_residual import _mask
    with torch.random.fork_rng():
        torch.manual_seed(4100 + nb)
        net = networks.get_resnet(1, [C] * nb, COUT).cuda()
    mask = _mask(H, W, False)
    HW = H * W
    host = E.probe_plan(mask.numpy())
    assert host is not None and host["ns"] == 1
    livepix = np.flatnonzero(mask.numpy().reshape(-1) == 0)
    live = {"parity": 1, "act_idx": torch.from_numpy((np.arange(C)[:, None] * HW + livepix[None, :]).reshape(-1).astype(np.int32)).cuda()}
    plan = {"ns": host["ns"], "cls": torch.from_numpy(host["cls"]).cuda(), "probes": torch.from_numpy(host["probes"]).reshape(-1).cuda()}
    view = E.NetView(E.Geometry((1, H, W)), 1, mask=mask.cuda(), live=live, probe=plan)
    gen = torch.Generator().manual_seed(4200 + nb)
    z, v = torch.randn(B, 1, H, W, generator=gen), torch.randn(B, HW, NC, generator=gen)
    with E.scope(E.KernelConfig(tangent="bf16x3")), torch.no_grad():
        acts = E.net_primal(net, z.cuda(), view, need_acts="bits")[2]
    assert all(isinstance(a, E.BitMask) for a in acts[1:-1]) and len(acts) == 2 * nb + 1
    # float64: h_0 = conv0(mask . v), each block through ``direct`` (the last one with the 1 x 1 conv, the others with the identity)
    conv0, blocks, convf = E._resnet_parts(net)
    w64 = lambda m: m.weight.detach().cpu().double()
    m_of = lambda a: _bits(a) if isinstance(a, E.BitMask) else (a.cpu() > 0)
    vm = (v.reshape(B, 1, H, W, NC) * mask[None, :, :, :, None]).permute(0, 4, 1, 2, 3).reshape(B * NC, 1, H, W).double()
    h = F.conv2d(vm, w64(conv0), padding=1).reshape(B, NC, C, H, W).permute(0, 2, 3, 4, 1)
    for k, blk in enumerate(blocks):
        out = k + 1 == nb
        h = direct(h, m_of(acts[2 * k]), m_of(acts[2 * k + 1]), m_of(acts[2 * k + 2]) if out else torch.ones(B, C, H, W, dtype=torch.bool),
                   w64(blk.conv1), w64(blk.conv2), w64(convf).reshape(COUT, C) if out else torch.eye(C, dtype=torch.float64))
        h = h if out else h.reshape(B, C, H, W, NC)
    return dict(net=net, view=view, acts=acts, v=v, want=h)                              # want (B, cout, HW, nc)


def _run(monkeypatch, nb, on):
    """The coupler's tangent under the switches ``on`` -> (plan, launch counts, returned stack, its values (B, cout, pixels, nc), the pixels)."""
    from cmf_amd import engine as E
    c = _case(nb)
    for sw in SWITCHES:
        monkeypatch.setattr(E, sw, sw in on)
    monkeypatch.setattr(E, "PROBE_FRONT_SHAPES", {(H, W, 1)})
    monkeypatch.setattr(E, "FOLD_BLOCK_SHAPES", ((H, W, COUT),))
    n = dict(thin=0, hidden=0, out=0, head=0, block=0, apply=0, panel=0, gather=0)
    conv_tangent, probe_apply, seed_panel, gather_primal = E.conv_tangent, E.probe_apply, E.seed_panel, E.gather_primal

    def counting(*a, **k):
        hd = k.get("head")
        n["thin"] += a[6] == 9 and a[12] == 1 and a[11] == B                   # (not the one-sample launch behind the probe columns)
        n["hidden"] += a[6] == 9 and a[12] == C and a[13] == C
        n["out"] += a[6] == 1
        n["head"] += hd is not None
        n["block"] += hd is not None and "conv1" in hd
        return conv_tangent(*a, **k)

    def count(name, f):
        def g(*a, **k):
            n[name] += 1
            return f(*a, **k)
        return g

    monkeypatch.setattr(E, "conv_tangent", counting)
    monkeypatch.setattr(E, "probe_apply", count("apply", probe_apply))
    monkeypatch.setattr(E, "seed_panel", count("panel", seed_panel))
    monkeypatch.setattr(E, "gather_primal", count("gather", gather_primal))
    T = E.Tangent(B, H * W, NC, "panel", "cuda", data=c["v"].contiguous().cuda().reshape(-1))
    with E.scope(E.KernelConfig(tangent="bf16x3")), torch.no_grad():
        plan = E.resnet_tangent_plan(c["net"], c["view"], NC, T.layout, c["acts"], False)
        yt = E.net_tangent(c["net"], T, c["view"], c["acts"])
        got = yt.to_dense(NC).reshape(B, COUT, -1, NC).cpu().double()
    sel = live_sel(H, W, 1 if yt.compact else 0)
    assert got.shape[2] == int(sel.sum()) and bool(torch.isfinite(got).all())
    return plan, n, yt, got, sel


def _check(monkeypatch, nb, name, on, want):
    c = _case(nb)
    if "plain" not in c:
        c["plain"] = _run(monkeypatch, nb, ())[3]
    plan, n, yt, got, sel = _run(monkeypatch, nb, on)
    filt, front, tail, compact = want
    # both errors on the pixels this plan returns
    err, err_plain = (float((t - c["want"][:, :, sel]).abs().max()) for t in (got, c["plain"][:, :, sel]))
    print(f"tangent_plan nb={nb} {name}: plan {tuple(plan)}, launches {n}, max err {err:.3e}, all-plain {err_plain:.3e} "
          f"(max |want| {float(c['want'].abs().max()):.3e})")
    assert tuple(plan) == want
    assert n["thin"] == (front != "seeded") and n["hidden"] == 2 * nb - (tail == "block") and n["out"] == (tail in ("plain", "live"))
    assert n["head"] == (tail in ("head", "block")) and n["block"] == (tail == "block")
    assert n["apply"] == (front != "plain") and n["panel"] == (front == "seeded") and n["gather"] == (tail == "live")
    assert yt.compact == compact and yt.N == COUT * (H * W // 2 if compact else H * W)
    assert err <= 2.0 * err_plain, (err, err_plain)
    return yt


@pytest.mark.parametrize("name", list(PLANS))
def test_two_blocks(name, monkeypatch):
    """Each plan of the two-block coupler: the planner's answer, the launches, the output's form, and a maximum error against float64
    of at most twice that of the all-switches-off run against the same reference (the project's factor for a re-ordered sum)."""
    from cmf_amd import engine as E
    yt = _check(monkeypatch, 2, name, *PLANS[name])
    if name == "all-on":                                  # the compact flag travels through expand_columns with the columns
        colmap = torch.cat([torch.arange(NC, dtype=torch.int32), torch.full((16,), -1, dtype=torch.int32)]).cuda()
        wide = E.expand_columns(yt, NC + 16, colmap)
        assert wide.compact is True and torch.equal(wide.to_dense(NC), yt.to_dense(NC)) and not bool(wide.to_dense(NC + 16)[:, :, NC:].any())


def test_one_block(monkeypatch):
    """One block: the probe front hands h_0 to the folded head as a tensor -- no seeding, no folded block."""
    _check(monkeypatch, 1, "all-on", SWITCHES, (True, "probe", "head", True))
