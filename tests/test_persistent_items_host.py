"""Host-side checks of the helpers behind tests/test_gpu_persistent_items.py (no GPU needed): the item counts the launch-geometry
mirror gives for the shapes of the existing kernel tests, the way items are dealt to workgroups, the batch-size choice, and the
per-element error bound ``c`` -- a CPU emulation of the three-product split has to stay inside it, and the same emulation with
one of two injected defects has to leave it."""
import math

import pytest
import torch
import torch.nn.functional as F

import _persistent_items as P


def test_item_counts_of_the_existing_kernel_tests():
    """The table of the existing tests' launches on a 256-CU device: all of them one item per workgroup."""
    assert P.forward_items(32, 32, 32, 64, 3) == 192                 # test_conv_tangent 64 -> 64, 32 x 32, nc 32 (4 x 8 tiles)
    assert P.forward_items(28, 28, 32, 64, 3) == 168
    assert P.forward_items(14, 14, 64, 64, 3) == 84
    assert P.forward_items(28, 28, 16, 64, 2, group=32) == 112       # test_f16x3_*: 32 samples = 2 groups, 32-channel items
    assert P.forward_items(28, 28, 16, 64, 2, group=64) == 56
    assert P.wgrad_rows_split(28, 64, 3) == 168                      # test_conv_tangent_weight_gradient 64 -> 128, 28 x 28, nc 64
    assert P.wgrad_rows_f32(28, 64, 3) == 336
    assert P.tile_shape(14, 14) == (2, 14) and P.tile_shape(28, 28) == (2, 14) and P.tile_shape(16, 16) == (4, 8)
    assert P.tile_shape(8, 32) == (4, 8) and P.n_tiles(8, 32) == 8 and P.n_tiles(12, 24) == 9 and P.n_tiles(14, 28) == 14
    assert P.forward_items(14, 14, 48, 128, 1) == 7 * 3 * 2 and P.forward_items(14, 14, 16, 32, 1) == 7
    assert P.f16_item_group(16, 16, 64) == 32 and P.f16_item_group(14, 14, 64) == 64 and P.f16_item_group(28, 28, 32) == 32
    for total in (192, 168, 84, 112):
        assert max(P.xcd_counts(total, min(total, 256))) == 1


@pytest.mark.parametrize("total,G", [(525, 256), (513, 256), (640, 256), (5, 5), (7, 7), (100, 100), (300, 256), (1000, 304), (0, 0)])
def test_items_are_dealt_like_the_kernels_deal_them(total, G):
    """The helper's dealing covers every item exactly once and its counts add up.  (A regression check of the helper against a
    second transcription of the kernels' formula -- conv_tangent_bf16x3.hip's item list, conv_wgrad_bf16x3.hip's with min(G, 8)
    ranges -- not independent evidence that it matches them: that is by reading the kernels.)"""
    if G == 0:
        assert P.xcd_counts(0, 0) == []
        return
    q, r = divmod(total, 8)
    seen = []
    for bid in range(G):
        xcd, jx = bid & 7, bid >> 3
        xstart = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        xlen = q + (1 if xcd < r else 0)
        nbx = (G - xcd + 7) >> 3
        mine = list(range(xstart + jx, xstart + xlen, nbx)) if jx < xlen else []
        assert len(mine) == P.xcd_counts(total, G)[bid]
        seen += mine
    assert sorted(seen) == list(range(total))
    assert sum(P.block_counts(total, G)) == total


def test_batch_size_choice_reaches_the_multi_item_regime():
    for cus in (256, 304, 240):
        for per in (7, 14, 21, 28, 42, 56, 8, 16, 64, 128, 9, 18, 14 * 3 * 2):
            np_ = P.choose_np(per, cus)
            total, G = per * np_, min(per * np_, cus)
            assert P.multi_item_problems(total, G, per) == []
            assert total >= 2 * G + 1 and total % G != 0 and (total % 8 != 0 or per % 8 == 0)
            counts = P.xcd_counts(total, G)
            assert min(counts) >= 2 and max(counts) >= 3 and len(set(counts)) > 1
            if per % 8:
                # unequal XCD ranges: some range is one item longer than another
                assert total % 8 != 0
    assert P.multi_item_problems(512, 256) and P.multi_item_problems(520, 256) and P.multi_item_problems(768 + 1, 769)
    assert P.choose_np(28, 256, multiple_of=1) % 2 == 1                # 28 np % 8 != 0 needs an odd batch
    for rows_per, cap in ((14, 256), (28, 256), (16, 256), (14, 120)):
        np_ = P.choose_np(rows_per, cap)
        counts = P.block_counts(rows_per * np_, cap)                   # contiguous blocks: the last workgroups may be idle
        assert max(counts) >= 3 and sum(counts) == rows_per * np_


def test_repeat_period_and_copy_plan():
    for per in (7, 14, 21, 42, 8, 9, 64, 128, 15):
        p = P.repeat_period(per)
        assert math.gcd(p, 8) == 1 and math.gcd(p, per) == 1
    base, expo = P.copy_plan(23, 3)
    assert base.tolist()[:7] == [0, 1, 2, 0, 1, 2, 0] and expo.tolist()[:7] == [0, 0, 0, 1, 1, 1, 2] and int(expo.max()) == 3
    # neighbouring samples never hold identical data: equal (base, exponent) pairs are 4 periods apart
    pairs = list(zip(base.tolist(), expo.tolist()))
    assert all(pairs[i] != pairs[j] for i in range(23) for j in range(i + 1, min(23, i + 12)))


def _emulation_case(cin, seed=0, n=8, H=14, W=14, cout=64):
    gen = torch.Generator().manual_seed(1000 * cin + seed)
    x = torch.randn(n, cin, H, W, generator=gen)
    prim = torch.randn(n, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (9 * cin) ** 0.5
    xin = x * (prim > 0).float()
    want, A = P.reference(xin, w)
    return xin, w, want, A


@pytest.mark.parametrize("cin", [32, 64, 128])
def test_split_emulation_stays_inside_the_bound_and_injected_defects_leave_it(cin):
    """The three-product split emulated on the CPU (hi / lo parts, fp32 ``F.conv2d``) against float64, per element and relative to
    A = conv2d(|x|, |w|): inside c with a factor of about four to spare; (a) without the hi * lo product and (b) with one tap of one
    output row read from the neighbouring sample it is outside c."""
    xin, w, want, A = _emulation_case(cin)
    for dt, c in ((torch.bfloat16, P.C_BF16X3), (torch.float16, P.C_F16X3)):
        ok = P.err_over_A(P.emulate_split_conv(xin, w, dt), want, A)
        print(f"cin {cin} {dt}: max |err| / A = 2^{math.log2(ok):.2f}  (c = 2^{math.log2(c):.0f})")
        assert ok <= c / 2, (dt, ok, c)                                   # the margin the bound was chosen with (measured: ~4x)
        # (a) the x_hi * w_lo product left out
        a = P.err_over_A(P.emulate_split_conv(xin, w, dt, drop_hi_lo=True), want, A)
        assert a > c, (dt, a, c)
        # (b) output row 5 of sample 2: tap (ky = 0, kx = 2) reads sample 3's input instead of its own
        y = P.emulate_split_conv(xin, w, dt)
        wt = torch.zeros_like(w)
        wt[:, :, 0, 2] = w[:, :, 0, 2]
        tap_own, tap_other = F.conv2d(xin[2:3], wt, padding=1), F.conv2d(xin[3:4], wt, padding=1)
        y[2, :, 5] += (tap_other - tap_own)[0, :, 5]
        b = P.err_over_A(y, want, A)
        assert b > c, (dt, b, c)
        # the defect is confined: every other output row is still inside the bound
        y[2, :, 5] = want[2, :, 5].float()
        assert P.err_over_A(y, want, A) <= c
    # exact fp32 products sit below both
    assert P.err_over_A(P.emulate_split_conv(xin, w, torch.float32), want, A) < P.C_F16X3


def test_max_norm_error_of_the_emulated_bf16_split():
    """The max-norm figure the kernel tests' 2e-5 bound is compared with: ~3e-6 for the emulated bf16 split."""
    xin, w, want, A = _emulation_case(64)
    y = P.emulate_split_conv(xin, w, torch.bfloat16)
    rel = float((y.double() - want).abs().max() / want.abs().max())
    assert rel < 1e-5, rel


@pytest.mark.parametrize("cin", [32, 128])
def test_sign_band_of_the_float64_reference_is_thin(cin):
    """Sign bits are compared where |want| > c A only; for normal data the float64 reference has far fewer than 0.1 % of its
    elements inside that band (it is 2^-16 of A wide, A ~ sqrt(K) |want|: 3e-4 of the elements at cin = 128, bf16)."""
    xin, w, want, A = _emulation_case(cin, seed=1)
    for c in (P.C_BF16X3, P.C_F16X3):
        share = float((want.abs() <= c * A).double().mean())
        assert share < 5e-4, (c, share)


def test_err_over_A_counts_zero_over_zero_as_zero():
    want, A = torch.tensor([0.0, 1.0], dtype=torch.float64), torch.tensor([0.0, 2.0], dtype=torch.float64)
    assert P.err_over_A(torch.tensor([0.0, 1.0]), want, A) == 0.0
    assert P.err_over_A(torch.tensor([1e-9, 1.0]), want, A) == math.inf
    assert P.err_over_A(torch.tensor([0.0, 1.5]), want, A) == 0.25
