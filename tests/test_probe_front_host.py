"""Host side of the probe front (engine.probe_plan, csrc/probe_front.hip): the class table's separation property, and a float64
emulation of "probe responses + apply" against the direct conv1(relu'(a0) . conv0(mask . v)).  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmf_amd import engine as E                                     # noqa: E402

SHAPES = [(4, 14), (14, 14), (28, 28)]


def checkerboard(cin, H, W, reverse):
    """The mask of Checkerboard2dAffineCouplingBijection: 1 = pass-through where (row + col) is odd, flipped by reverse_mask."""
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = ((ii + jj) % 2 == 1).astype(np.float32)
    if reverse:
        m = 1 - m
    return np.broadcast_to(m, (cin, H, W)).copy()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cin", [1, 2])
def test_separation_by_brute_force(H, W, reverse, cin):
    """Independently of probe_plan's own check: every 5 x 5 window, clipped at the border, holds each class at most once, and no more
    than 13 classes per channel; the table marks exactly the mask's rows; the probe columns are the classes' indicator vectors."""
    mask = checkerboard(cin, H, W, reverse)
    plan = E.probe_plan(mask)
    assert plan is not None and plan["ns"] == (13 * cin + 15) // 16
    cls = plan["cls"].reshape(cin, H, W)
    assert cls.dtype == np.int8 and ((cls >= 0) == (mask != 0)).all() and cls.max() < 13 * cin
    for c in range(cin):
        live = cls[c][cls[c] >= 0]
        assert live.min() >= 13 * c and live.max() < 13 * (c + 1)
    for r in range(H):
        for col in range(W):
            seen = set()
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    rr, cc = r + dy, col + dx
                    if 0 <= rr < H and 0 <= cc < W:
                        for c in range(cin):
                            k = int(cls[c, rr, cc])
                            if k >= 0:
                                assert k not in seen, (r, col, k)
                                seen.add(k)
            assert len(seen) <= 13 * cin
    P = plan["probes"]
    assert P.shape == (cin * H * W, 16 * plan["ns"]) and P.dtype == np.float32
    flat = cls.reshape(-1)
    for k in range(16 * plan["ns"]):
        assert (P[:, k] == (flat == k)).all()


def test_no_plan_without_a_checkerboard():
    assert E.probe_plan(np.ones((1, 14, 14), np.float32)) is None                 # every pixel an input: classes repeat in a window
    stripes = np.zeros((1, 14, 14), np.float32)
    stripes[:, :, ::2] = 1
    assert E.probe_plan(stripes) is None
    assert E.probe_plan(checkerboard(3, 14, 14, False)) is None                    # more channels than the apply kernel lists
    assert E.probe_plan(np.ones((14, 14), np.float32)) is None


def emulate_apply(R, v, cls, cin, H, W):
    """The apply kernel's formula in float64: R (B, HW, ncls, 64), v (B, cin, HW, nc) -> (B, 64, HW, nc); terms in raster order of
    the window, c ascending."""
    B, nc = v.shape[0], v.shape[-1]
    out = torch.zeros(B, R.shape[-1], H * W, nc, dtype=torch.float64)
    for p in range(H * W):
        r, col = divmod(p, W)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                rr, cc = r + dy, col + dx
                if not (0 <= rr < H and 0 <= cc < W):
                    continue
                for c in range(cin):
                    k = int(cls[c * H * W + rr * W + cc])
                    if k >= 0:
                        out[:, :, p, :] += R[:, p, k, :, None] * v[:, c, rr * W + cc, None, :]
    return out


@pytest.mark.parametrize("H,W", [(4, 14), (14, 14)])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cin", [1, 2])
def test_probe_responses_and_apply_in_float64(H, W, reverse, cin):
    """conv1(relu'(a0) . conv0(mask . v)) == apply(conv1(relu'(a0) . conv0(mask . probes)), v) to 1e-12 relative, on random weights,
    a random relu' pattern, a mask with random non-zero values on the checkerboard and random v; every pixel, borders included."""
    g = torch.Generator().manual_seed(1000 * H + 10 * cin + reverse)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, nc, hid = 2, 5, 8
    pattern = checkerboard(cin, H, W, reverse)
    plan = E.probe_plan(pattern)
    mask = torch.from_numpy(pattern).double() * (0.5 + torch.rand(cin, H, W, generator=g, dtype=torch.float64))
    w0, w1 = rn(hid, cin, 3, 3), rn(hid, hid, 3, 3)
    relu = (rn(B, hid, H, W) > 0).double()
    v = rn(B, cin, H, W, nc)

    def front(x):                                                # x (B', cin, H, W, n) -> (B, hid, H, W, n)
        n = x.shape[-1]
        xi = (x * mask[None, :, :, :, None]).permute(0, 4, 1, 2, 3).reshape(-1, cin, H, W)
        h0 = F.conv2d(xi, w0, padding=1).reshape(x.shape[0], n, hid, H, W)
        h0 = (h0 * relu[:, None]).reshape(-1, hid, H, W)
        return F.conv2d(h0, w1, padding=1).reshape(B, n, hid, H, W).permute(0, 2, 3, 4, 1)

    direct = front(v)
    ncls = 16 * plan["ns"]
    probes = torch.from_numpy(plan["probes"]).double().reshape(1, cin, H, W, ncls)
    R = front(probes.expand(B, -1, -1, -1, -1)).reshape(B, hid, H * W, ncls).permute(0, 2, 3, 1)
    got = emulate_apply(R, v.reshape(B, cin, H * W, nc), plan["cls"], cin, H, W).reshape(B, hid, H, W, nc)
    err = float((got - direct).abs().max() / direct.abs().max())
    assert err < 1e-12, err
