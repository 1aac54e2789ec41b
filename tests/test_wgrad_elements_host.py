"""CPU checks of tests/_wgrad_elements.py: the emulations of the weight-gradient kernels' arithmetic meet the per-element bound on
every GPU case's own inputs and launch geometry (and say what C_WGRAD_F32 was derived from), channel scales pass through them bit
for bit, injected defects break the bound -- cross-talk between channels while the older tensor-wide check still passes, which is
the gap the per-element tests close -- and the launch-geometry mirrors say which kernel family every case reaches."""
import math

import pytest
import torch

import _wgrad_elements as WE

ALL = WE.CASES + WE.BATCHED
_ids = lambda cases: [c.id for c in cases]
_case = lambda fam, **kw: next(c for c in WE.CASES if c.family == fam and all(getattr(c, k) == v for k, v in kw.items()))


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_emulation_meets_the_bound(case):
    d = WE.case_data(case)
    got = d.prev + WE.emulate_case(case, d)
    ratio = WE.check_elements(f"emulation {case.id}", got, d.want, d.A, d.prev, case.arithmetic, case.R, tag="WGRAD_ELEMENTS_HOST")
    if case.arithmetic == "f32":                                           # the margin C_WGRAD_F32 was given over the emulation
        assert 4 * ratio <= WE.C_WGRAD_F32, (case.id, math.log2(ratio))


def test_c_wgrad_f32_is_four_times_the_emulation_rounded_up():
    """C_WGRAD_F32 = 4 x the largest emulated max |err| / A over the fp32 cases, rounded up to a power of two: not larger."""
    worst = 0.0
    for case in WE.CASES:
        if case.arithmetic == "f32":
            d = WE.case_data(case)
            worst = max(worst, WE.ratio_over_A(d.prev + WE.emulate_case(case, d), d.want, d.A, d.prev))
    print(f"\nWGRAD_ELEMENTS_HOST largest fp32 emulation error 2^{math.log2(worst):.2f} of A; C_WGRAD_F32 = 2^{math.log2(WE.C_WGRAD_F32):.0f}")
    assert WE.C_WGRAD_F32 == 2.0 ** math.ceil(math.log2(4 * worst)), math.log2(worst)
    assert WE.C_WGRAD_BF16X3 == WE.P.C_BF16X3 == 2.0 ** -16


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_channel_scales_pass_through_bit_for_bit(case):
    """emulate(graded) == emulate(all scales 1) s_co s_ci: powers of two commute with every rounding away from subnormals."""
    g, u = WE.make_data(case), WE.make_data(case, graded=False)
    sc = (g.s_co.view(-1, 1, 1, 1) * g.s_ci.view(1, -1, 1, 1))
    assert torch.equal(WE.emulate_case(case, g), WE.emulate_case(case, u) * sc), case.id


# ---------------------------------------------------------------------------------------------------------------------------
# injected defects
def _verdict(case, d, got):
    """(breaks the per-element bound, passes the older max-norm check, max err / A, max-norm error)"""
    err = (got.double() - d.want).abs()
    broken = bool((err > WE.bound(d.want, d.A, d.prev, WE.c_of(case))).any())
    rel = WE.max_norm_error(got, d.want, d.prev)
    return broken, rel < WE.MAX_NORM[case.arithmetic], WE.ratio_over_A(got, d.want, d.A, d.prev), rel


_DEFECT_CASES = [_case("rows3x3", cin=17, fmode="none"), _case("rows3x3", cin=64, H=14, fmode="none", f_group=1),
                 _case("split", cin=64, H=14, fmode="none"), _case("split", cin=128, fmode="none")]


@pytest.mark.parametrize("case", _DEFECT_CASES, ids=_ids(_DEFECT_CASES))
def test_defect_cross_talk_passes_the_max_norm_check_and_breaks_the_element_bound(case):
    """(a) 2^-16 of the scale-1 channel 0 of x leaks into every other channel: 2^-16 of the largest entries at most, so the
    tensor-wide check cannot see it; in a channel of scale 2^-12 it is 2^-4 of the entry's own products."""
    d = WE.case_data(case)
    leak = 2.0 ** -16 * d.xe[:, :1].clone()
    leak = leak.expand_as(d.xe).clone()
    leak[:, 0] = 0
    order, n_wg, waves = case.geometry()
    got = d.prev + WE.emulate(d.xe + leak, d.gy, d.fac32, case.arithmetic, n_wg, order, waves, case.taps)
    broken, old_ok, ratio, rel = _verdict(case, d, got)
    print(f"\nWGRAD_ELEMENTS_HOST defect (a) {case.id}: max |err| / A = 2^{math.log2(ratio):.2f}, max-norm error {rel:.2e}")
    assert old_ok, (case.id, rel)
    assert broken, (case.id, ratio)


def _leak(case, d, max_scale):
    return WE.emulate_case(case, d, leak_channels=(d.s_ci <= max_scale).nonzero().reshape(-1))


@pytest.mark.parametrize("case", _DEFECT_CASES, ids=_ids(_DEFECT_CASES))
def test_defect_border_tap_reads_the_neighbouring_row(case):
    """(b) At column 0 the dx = -1 taps read the pixel before it in memory (the previous row's last pixel) instead of zero, on the
    input channels of scale <= 2^-8 only.  The per-element bound breaks (max err / A = 2^-3.8 ... 2^-5.7).
    NOT asserted, because it is not so: that the older max-norm check passes.  A wrong tap adds a whole image column of products to
    an entry, 1 / sqrt(W) of the entry's own sum, and an input channel of scale 2^-8 meets output channels of scale 1: measured
    max-norm errors 8.5e-4 ... 1.2e-3 with the channels of scale <= 2^-8, 2.1e-4 ... 4.4e-4 with <= 2^-10, 6.4e-5 ... 8.7e-5 with
    2^-12 alone, against bounds of 2e-5 / 5e-5.  The tensor-wide check sees this defect at every scale the input recipe has; what it
    cannot do is say WHERE (the per-element failure names the dx = -1 entries of the small channels).  Defect (a) is the one that
    hides below it."""
    d = WE.case_data(case)
    broken, old_ok, ratio, rel = _verdict(case, d, d.prev + _leak(case, d, 2.0 ** -8))
    print(f"\nWGRAD_ELEMENTS_HOST defect (b) {case.id}: max |err| / A = 2^{math.log2(ratio):.2f}, max-norm error {rel:.2e}"
          f" (the max-norm check {'passes' if old_ok else 'fails'})")
    assert broken, (case.id, ratio)
    err = ((d.prev + _leak(case, d, 2.0 ** -8)).double() - d.want).abs() > WE.bound(d.want, d.A, d.prev, WE.c_of(case))
    assert not bool(err[:, :, :, 1:].any()) and not bool(err[:, d.s_ci > 2.0 ** -8].any()), "only the dx = -1 taps of the leaking channels"


@pytest.mark.parametrize("case", [c for c in WE.CASES if c.family == "split" and c.fmode in ("none", "relu")],
                         ids=_ids([c for c in WE.CASES if c.family == "split" and c.fmode in ("none", "relu")]))
def test_defect_dropped_hi_lo_product(case):
    """(c) the split kernel without its gy_hi x_lo product: 2^-9 of a product, 2^7 times the bound."""
    d = WE.case_data(case)
    broken, _, ratio, _ = _verdict(case, d, d.prev + WE.emulate_case(case, d, drop_hi_lo=True))
    assert broken, (case.id, ratio)


_RELU_CASES = [c for c in ALL if c.fmode in ("relu", "bits")]


@pytest.mark.parametrize("case", _RELU_CASES, ids=_ids(_RELU_CASES))
def test_defect_relu_of_plus_zero_taken_as_one(case):
    """(d) relu'(+0.0) = 1 (a ``>=`` for the ``>``, which also lets -0.0 through or not depending on how it is written: here +0.0
    only)."""
    d = WE.case_data(case)
    plus_zero = (d.src == 0) & ~torch.signbit(d.src)
    assert bool(plus_zero.any()) and bool(((d.src == 0) & torch.signbit(d.src)).any()) and bool((d.src == WE.TINY).any())
    order, n_wg, waves = case.geometry()
    fac = torch.where(plus_zero, torch.ones_like(d.fac32), d.fac32)
    got = d.prev + WE.emulate(d.xe, d.gy, fac, case.arithmetic, n_wg, order, waves, case.taps)
    broken, _, ratio, _ = _verdict(case, d, got)
    assert broken, (case.id, ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry
def test_dispatch_rules_are_the_ones_mirrored():
    """``family`` and ``Case.geometry`` restate the shape rules of cmf_conv_tangent_wgrad, wgrad_split_launch and
    engine.conv_tangent_wgrad; the lines they restate must still be in the sources."""
    assert WE.missing_dispatch_lines() == []


@pytest.mark.parametrize("cin,cout,taps,nc,fmode,f_group,precision,want", [
    (1, 64, 9, 16, "none", 1, "f32", "thin3x3_nt1"), (2, 64, 9, 16, "relu", 1, "f32", "thin3x3_nt2"), (3, 24, 9, 16, "raw", 1, "f32", "thin3x3_nt2"),
    (4, 64, 9, 16, "none", 1, "f32", "thin3x3_nt3"), (5, 24, 9, 16, "tanh", 1, "bf16x3", "thin3x3_nt3"), (6, 64, 9, 16, "self", 1, "f32", "thin3x3_nt4"),
    (7, 64, 9, 16, "none", 1, "f32", "thin3x3_nt4"), (8, 8, 9, 32, "none", 1, "f32", "rows3x3"), (130, 70, 9, 16, "raw", 1, "f32", "rows3x3"),
    (10, 16, 1, 16, "none", 1, "f32", "thin1x1"), (10, 17, 1, 16, "none", 1, "f32", "general1x1"), (130, 12, 1, 16, "none", 1, "f32", "thin1x1"),
    (64, 64, 9, 32, "relu", 1, "bf16x3", "split"), (64, 64, 9, 32, "bits", 1, "bf16x3", "split"), (64, 64, 9, 32, "tanh", 1, "bf16x3", "rows3x3"),
    (64, 64, 9, 32, "relu", 16, "bf16x3", "rows3x3"), (64, 64, 9, 16, "relu", 1, "bf16x3", "rows3x3"), (64, 32, 9, 32, "none", 1, "bf16x3", "rows3x3"),
    (64, 64, 9, 32, "none", 1, "f32", "rows3x3"), (64, 64, 1, 32, "none", 1, "bf16x3", "general1x1")])
def test_family_of_a_shape(cin, cout, taps, nc, fmode, f_group, precision, want):
    assert WE.family(cin, cout, taps, nc, fmode, f_group, precision) == want


def test_every_family_has_cases_and_the_listed_shapes_reach_them():
    fams = {c.family for c in ALL}
    assert fams == {"rows3x3", "general1x1", "thin1x1", "split", "thin3x3_nt1", "thin3x3_nt2", "thin3x3_nt3", "thin3x3_nt4"}
    assert {c.cin for c in WE.CASES if c.family == "thin3x3_nt3"} == {4, 5}
    for c in WE.CASES:
        if c.taps == 9 and c.precision == "f32":
            assert c.family == ("rows3x3" if c.cin >= 8 else f"thin3x3_nt{(1, 2, 2, 3, 3, 4, 4)[c.cin - 1]}"), c.id
        if c.precision == "bf16x3":
            assert c.family == "split", c.id                               # none of the small split shapes falls to the fp32 kernel
    assert {(c.cin, c.cout): c.family for c in WE.CASES if c.taps == 1} == {
        (130, 12): "thin1x1", (64, 2): "thin1x1", (10, 16): "thin1x1", (10, 17): "general1x1", (130, 70): "general1x1"}
    for fam, modes in (("rows3x3", WE.FMODES), ("split", WE.SPLIT_FMODES)):
        for shape in {(c.cin, c.cout, c.H, c.W) for c in WE.CASES if c.family == fam}:
            assert {c.fmode for c in WE.CASES if (c.cin, c.cout, c.H, c.W) == shape} >= set(modes), shape
    for cin in range(1, 8):
        assert {c.fmode for c in WE.CASES if c.cin == cin and c.taps == 9} == set(WE.FMODES), cin
    assert any(c.f_group == 16 for c in WE.CASES)
    assert sorted(c.nprob for c in WE.BATCHED) == [1, 1, 3, 3, 16, 16]


def test_geometry_covers_every_k_block_once():
    """Workgroup counts of the mirrored launches; ``emulate`` itself asserts that the dealing covers every K block exactly once."""
    geo = {c.id: c.geometry() for c in ALL}
    assert geo[_case("rows3x3", cin=17, fmode="none").id] == ("rows", 30, 1)
    assert geo[_case("rows3x3", cin=130, fmode="none").id] == ("rows", 6, 1)
    assert geo[_case("thin1x1", cin=130).id] == ("blocks", 11, 8)
    assert geo[_case("general1x1", cin=130).id] == ("blocks", 111, 1)
    assert geo[_case("split", cin=64, H=14, fmode="none").id] == ("xcd_rows", 42, 1)
    assert [c.geometry()[1] for c in WE.BATCHED] == [12, 80, 16, 6, 80, 16]
