"""The folded block's formula (csrc/conv_block_head.hip, ``engine.FOLD_BLOCK``) in float64 on the CPU: the last residual block's
conv1, conv2 (with the residual) and the 1x1 output conv as per-pixel coefficients over a 5 x 5 window of the block's input h, against
the direct composition conv1 -> mask -> conv2 -> + h -> mask -> 1x1.  Also the argument checks of the C entry that fail before any
launch.  ``formula`` / ``direct`` / ``dead_rows`` are what tests/test_gpu_fold_block.py measures the kernel against."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

HID = 64


@pytest.fixture(scope="module")
def built_lib():
    from cmf_amd.build import build
    return build(verbose=False)


def live_sel(H, W, live):
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.ones(H * W, dtype=torch.bool) if not live else ((ii + jj) % 2 == live - 1).reshape(-1)


def direct(h, ma, m1, mK, w1, w2, wf):
    """h (B, C, H, W, nc); ma, m1, mK (B, C, H, W) bool; -> yt (B, cout, H*W, nc) float64, every pixel."""
    B, Cc, H, W, nc = h.shape
    img = lambda t: t.permute(0, 4, 1, 2, 3).reshape(B * nc, Cc, H, W)
    hd = img(h.double())
    rep = lambda m: m.double().unsqueeze(1).expand(B, nc, Cc, H, W).reshape(B * nc, Cc, H, W)
    u = F.conv2d(hd * rep(ma), w1.double(), padding=1)
    hK = F.conv2d(u * rep(m1), w2.double(), padding=1) + hd
    yt = torch.einsum("oc,nchw->nohw", wf.double(), hK * rep(mK))
    return yt.reshape(B, nc, -1, H * W).permute(0, 2, 3, 1)


def formula(h, ma, m1, mK, w1, w2, wf, absolute=False):
    """The issue's formula, term by term; ``absolute``: the same sums over absolute values (the scale of the rounding error)."""
    B, Cc, H, W, nc = h.shape
    cout = wf.shape[0]
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    w1, w2, wf, hd = ab(w1.double()), ab(w2.double()), ab(wf.double()), ab(h.double())
    G = wf.view(1, cout, Cc, 1, 1) * mK.double().unsqueeze(1)                                  # (B, o, c, H, W)
    E = torch.einsum("bochw,cit->botihw", G, w2.reshape(Cc, Cc, 9))                             # (B, o, t2, ci, H, W)
    m1p = F.pad(m1.double(), (1, 1, 1, 1))
    mhp = F.pad(hd * ma.double().unsqueeze(-1), (0, 0, 2, 2, 2, 2))                             # (B, c, H+4, W+4, nc)
    yt = torch.einsum("bochw,bchwn->bohwn", G, hd)
    Kd = torch.zeros(B, cout, 25, Cc, H, W, dtype=torch.float64)
    for t2 in range(9):
        e = E[:, :, t2] * m1p[:, None, :, t2 // 3:t2 // 3 + H, t2 % 3:t2 % 3 + W]              # (B, o, ci, H, W)
        for t1 in range(9):
            d = (t2 // 3 + t1 // 3) * 5 + t2 % 3 + t1 % 3
            Kd[:, :, d] += torch.einsum("boihw,ic->bochw", e, w1.reshape(Cc, Cc, 9)[:, :, t1])
    for d in range(25):
        yt = yt + torch.einsum("bochw,bchwn->bohwn", Kd[:, :, d], mhp[:, :, d // 5:d // 5 + H, d % 5:d % 5 + W])
    return yt.reshape(B, cout, H * W, nc)


def dead_rows(ma, mK, sel):
    """(B, C, H*W) bool: the rows of h the formula multiplies by an exact zero for the output pixels ``sel`` -- ma clear, and not
    the centre of an output pixel with mK set."""
    B, Cc, H, W = ma.shape
    centre = mK.reshape(B, Cc, -1) & sel.view(1, 1, -1)
    return ~(ma.reshape(B, Cc, -1) | centre)


def _inputs(H, W, cout, nc=3, B=2, seed=0):
    gen = torch.Generator().manual_seed(seed + 100 * H + W + 7 * cout)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    h = rn(B, HID, H, W, nc)
    ma, m1, mK = (rn(B, HID, H, W) > 0 for _ in range(3))
    return h, ma, m1, mK, rn(HID, HID, 3, 3) / 24, rn(HID, HID, 3, 3) / 24, rn(cout, HID) / 8


@pytest.mark.parametrize("cout", [2, 4])
@pytest.mark.parametrize("H,W", [(2, 14), (4, 14), (6, 6)])
def test_formula_matches_the_direct_composition(H, W, cout):
    args = _inputs(H, W, cout)
    want, got = direct(*args), formula(*args)
    scale = float(want.abs().max())
    for live in (0, 1, 2):
        sel = live_sel(H, W, live)
        assert float((got[:, :, sel] - want[:, :, sel]).abs().max()) <= 1e-12 * scale


def test_dead_rows_do_not_reach_the_output():
    """Whatever the rows ``dead_rows`` names hold, the direct composition (with the masks applied by ``where``) gives the same."""
    H, W, cout = 4, 14, 2
    h, ma, m1, mK, w1, w2, wf = _inputs(H, W, cout)
    for live in (1, 2):
        sel = live_sel(H, W, live)
        dead = dead_rows(ma, mK, sel).reshape(2, HID, H, W, 1)
        want = formula(h, ma, m1, mK, w1, w2, wf)[:, :, sel]
        got = formula(torch.where(dead, torch.zeros_like(h), h), ma, m1, mK, w1, w2, wf)[:, :, sel]
        assert torch.equal(got, want)
        assert bool(dead.any())


def _args(**over):
    """A cmf_conv_tangent_args the folded block accepts (pointers: aligned fakes, never dereferenced when a check fails first)."""
    from cmf_amd import _lib
    H, W, nc, cout = 4, 14, 16, 2
    a = _lib.ConvTangentArgs()
    a.x, a.x_np, a.x_ci, a.x_px, a.x_sl = 0x1000, HID * H * W * nc, 16, HID * nc, HID * 16
    a.f, a.f_np, a.fmode = 0x2000, H * W * 8, _lib.F_RELU_BITS
    a.w, a.head_w, a.head_cout = 0x3000, 0x4000, cout
    a.head_a, a.head_a_np, a.head_a_c, a.head_a_px = 0x5000, HID * H * W, H * W, 1
    a.head_y, a.head_y_np, a.head_y_co, a.head_y_px = 0x6000, cout * H * W * nc, H * W * nc, nc
    a.block_w1, a.block_m1, a.block_m1_np = 0x7000, 0x8000, H * W * 8
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps = 1, HID, HID, H, W, nc, 9
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over", [dict(block_m1=None), dict(r=0x9000), dict(block_w1=0x7004), dict(block_m1=0x8004), dict(block_m1_np=8),
                                  dict(fmode=1), dict(head_cout=9), dict(nc=24), dict(x_ci=1), dict(seed=0xa000), dict(cin=32)])
def test_c_entry_rejects_what_it_does_not_cover(built_lib, over):
    from cmf_amd import _lib
    lib = _lib.load()
    assert lib.cmf_conv_tangent_bf16x3(C.byref(_args(**over)), None) == -1


def test_pack_size_and_arguments(built_lib):
    from cmf_amd import _lib
    lib = _lib.load()
    n = C.c_longlong(0)
    assert lib.cmf_pack_block_weight(None, None, C.byref(n), None) == 0 and n.value == 9 * 4 * 2 * 2 * 64 * 16
    assert lib.cmf_pack_block_weight(None, None, None, None) == -1
    assert lib.cmf_pack_block_weight(0x1000, 0x2008, None, None) == -1
