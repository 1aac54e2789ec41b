"""The persistent kernels beyond one work item per workgroup, against float64 (``-m gpu``).

cmf_conv_tangent_bf16x3 / cmf_conv_tangent_f16x3, cmf_conv_tangent_wgrad_bf16x3(_batched) and the row-walking fp32 weight gradient
launch min(work, CUs or 256) workgroups and let each walk a list of items; the other kernel tests stop at one item per workgroup.
Here the batch size of every case is COMPUTED from the device's CU count so that every workgroup takes at least two items and
some take three, the eight XCD ranges have unequal lengths and workgroups of one XCD end on different item counts
(tests/_persistent_items.py; asserted before the launch, never skipped), plus one launch per family with fewer than 8 items and one
with 8 <= items < workgroup limit.

Every forward case asserts, for EVERY element,  |got - want| <= c A  with want = conv2d(F x, w) [+ res] in float64 on the CPU and
A = conv2d(|F x|, |w|) [+ |res|]  (c from the arithmetic: tests/_persistent_items.py, checked by tests/test_persistent_items_host.py),
and the max-norm bound of the corresponding one-item test unchanged; outputs are NaN-filled views into allocations with sentinel
guard bands that must come back untouched; the batch is a few base samples repeated with exact power-of-two scales (period coprime
to 8 and to the per-sample item count), and every copy must equal its base result times the scale BIT FOR BIT, whichever item
position it was computed at.  The fp16 form's input scale is one per launch (it enters amax_in), so its copies differ from their
base by a rotation of the 16 samples in the column slots instead -- columns never mix, so the results are the rotated ones, bit for
bit.  Every case prints its item count, workgroup count, items-per-workgroup range and the error it reached
(profiles/persistent_items_errors.txt).

A covering set, not the full product.  Left out: bias on the bf16x3 SELF_RELU launches (a per-launch constant does not scale with
the copies; the fp16 cases carry the bias); the tangent launch that reads relu' from a sample-grouped primal tensor (f_group = 16:
a factor-address variant of the relu mode); general float factors (tanh / raw) in slice-major layout and on cout = 32 apart from
one case each; nc = 48 with a residual in slice-major layout; checkerboard output from bit masks without residual on 2 x 14 tiles
and from floats without residual on 4 x 8 tiles (the other two pairings run); cin = 128 in the transposed and checkerboard forms.
items % 8 != 0 cannot hold when one sample has a multiple of 8 items (16 x 16, 32 x 32, 8 x 32: 8 or 64 tiles of 4 x 8); those
shapes run with equal XCD ranges and 12 x 24 images (9 tiles) carry the unequal ranges for the 4 x 8 tile form.
Workgroups WITHOUT an item: the forward kernels launch min(items, CUs) workgroups, so below 8 items and below the CU count every
workgroup has exactly one item and none is idle; their ``n_items > 0`` guards (amax_out atomic, residual descriptor) are NOT
reached by any case here.  Only a batched weight gradient, with its fixed workgroup count per problem, runs idle workgroups
(44 of 48 in the 4-row case); the fp32 row-walking kernel leaves its last workgroups without rows in the multi-row cases.
amax_out: the forward form's contract is the maximum over the stored values floored at 0 (the next conv's relu-on-load ignores
negative values, include/cmf_amd.h), the backward form's is max |stored|; each is asserted as EQUAL to that over the whole tensor."""
import math

import pytest
import torch
import torch.nn.functional as F

import _persistent_items as P
import _wgrad_elements as WE

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count      # the attribute cmf_device_cus() reads


def _launch(symbol, name, fn):
    """Run ``fn`` (one engine call) and assert WHICH kernel family it reached: the C ABI symbol (so that a shape rule change cannot
    turn a split-kernel test into a test of the fp32 fallback) and the launch's name in the engine's timer."""
    from cmf_amd import engine as E, _lib
    _lib.load()                                                           # trace() wraps a LOADED library: load it before, not inside
    with _lib.trace() as calls, E.timing(lambda n: True) as timer:
        fn()
    names = list(timer.by_name())
    torch.cuda.synchronize()
    syms = [c[0].split(":")[0] for c in calls if c[0].startswith(("cmf_conv_tangent", "cmf_conv_primal")) and "_ws" not in c[0]]
    assert syms == [symbol], (syms, symbol)
    assert names == [name], (names, name)


def _geometry(label, total, n_wg, per_sample, regime, counts_of=P.xcd_counts, fixed=False):
    """Assert the launch-geometry precondition of ``regime`` and print the item statistics.  Returns (G, counts).  ``fixed``: the
    launch has ``n_wg`` workgroups however few items there are (a problem of a batched weight gradient)."""
    G = n_wg if fixed else min(total, n_wg)
    counts = counts_of(total, G)
    print(f"\nPERSISTENT_ITEMS {label}: {P.describe(total, counts)}  regime {regime}")
    if regime == "multi":
        bad = P.multi_item_problems(total, G, per_sample)
        assert not bad, (label, bad)
        assert max(counts) >= 3 and len(set(c for c in counts if c)) > 1, (label, min(counts), max(counts))
        if counts_of is P.xcd_counts:
            assert min(counts) >= 2, (label, min(counts))
    elif regime == "lt8":
        assert 0 < total < 8, (label, total)
    else:
        assert 8 <= total < n_wg, (label, total, n_wg)
    return G, counts


def _np_for(per_sample, n_wg, regime, multiple_of=1):
    if regime == "multi":
        return P.choose_np(per_sample, n_wg, multiple_of)
    if regime == "lt8":
        assert per_sample * multiple_of < 8, per_sample
        return multiple_of
    np_ = -(-8 // per_sample)
    np_ = max(np_, 5 if per_sample * 5 < n_wg else np_)
    return -(-np_ // multiple_of) * multiple_of


class _Layout:
    """Logical tensors (np, C, H, W, nc) <-> 'panel' [sample][channel][pixel][nc] or the slice-major hidden layout 'slice'
    [sample][pixel][16-column slice][channel][16] (x_sl / y_sl: include/cmf_amd.h)."""

    def __init__(self, kind, H, W, nc):
        self.kind, self.HW, self.nc, self.S, self.H, self.W = kind, H * W, nc, nc // 16, H, W

    def to_dev(self, t):
        n, C = t.shape[0], t.shape[1]
        if self.kind == "panel":
            return t.contiguous().reshape(-1)
        return t.reshape(n, C, self.HW, self.S, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)

    def from_dev(self, flat, n, C, HW=None):
        HW = self.HW if HW is None else HW
        if self.kind == "panel":
            return flat.reshape(n, C, HW, self.nc)
        return flat.reshape(n, HW, self.S, C, 16).permute(0, 3, 1, 2, 4).reshape(n, C, HW, self.nc)

    def st(self, C, HW=None):
        HW = self.HW if HW is None else HW
        return (C * HW * self.nc, HW * self.nc, self.nc) if self.kind == "panel" else (C * HW * self.nc, 16, C * self.nc)

    def sl(self, C):
        return 16 if self.kind == "panel" else C * 16


def _columns_to_batch(t):
    """(n, C, H, W, nc) -> (n * nc, C, H, W): every Jacobian column an image."""
    n, C, H, W, nc = t.shape
    return t.permute(0, 4, 1, 2, 3).reshape(n * nc, C, H, W)


def _batch_to_columns(t, n, nc):
    N, C, H, W = t.shape
    return t.reshape(n, nc, C, H, W).permute(0, 2, 3, 4, 1)


def _first_bad(mask, n=5):
    idx = mask.nonzero()[:n].tolist()
    samples = sorted(set(mask.reshape(mask.shape[0], -1).any(1).nonzero().reshape(-1).tolist()))
    return f"{int(mask.sum())} elements, first (sample, channel, pixel, column) {idx}, samples {samples[:24]}"


def _check_values(label, got, want, A, c, max_norm):
    """Every element within c A of float64, and the one-item test's max-norm bound.  All on the device, in float64."""
    assert bool(torch.isfinite(got).all()), f"{label}: unwritten (NaN) output: {_first_bad(~torch.isfinite(got))}"
    err = (got.double() - want).abs()
    ratio = float((err / A.clamp_min(1e-300)).max())
    rel = float(err.max() / want.abs().max().clamp_min(1e-30))
    print(f"PERSISTENT_ITEMS {label}: max |err| / A = 2^{math.log2(max(ratio, 1e-300)):.2f} (c = 2^{math.log2(c):.0f})"
          f"  max-norm error {rel:.2e} (bound {max_norm:.0e})")
    bad = err > c * A
    assert not bool(bad.any()), f"{label}: |got - want| > c A at {_first_bad(bad)}; max ratio {ratio / c:.2f} c"
    assert rel < max_norm, (label, rel)


def _check_copies(label, got, base_idx, scale, per_sample, total, G, period):
    """Position independence: every copy == its base result (the first ``period`` samples) times its power of two, bit for bit."""
    expect = got[:period][base_idx] * scale.view(-1, *([1] * (got.dim() - 1)))
    same = (got == expect) | (torch.isnan(got) & torch.isnan(expect))
    if bool(same.all()):
        return
    pos = P.item_positions(total, G)
    bad_samples = (~same).reshape(same.shape[0], -1).any(1).nonzero().reshape(-1).tolist()
    where = {s: sorted(set(pos[w][1] for w in range(s * per_sample, (s + 1) * per_sample))) for s in bad_samples[:8]}
    raise AssertionError(f"{label}: copies differ from their base sample x 2^k: {_first_bad(~same)}; "
                         f"item positions (in their workgroups' lists) of the first differing samples {where}")


def _plan(np_, per_sample, device="cuda"):
    period = min(P.repeat_period(per_sample), np_)
    base_idx, expo = P.copy_plan(np_, period)
    return period, base_idx.to(device), (2.0 ** expo.float()).to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# cmf_conv_tangent_bf16x3, forward form
_FWD = [
    # H, W, cin, cout, nc, fmode, residual, layout               items per sample
    (14, 14, 64, 64, 16, "relu", True, "panel"),                 # 7
    (14, 14, 32, 128, 32, "none", False, "panel"),               # 28: two channel groups, one centre-tap chunk group
    (14, 14, 128, 64, 64, "bits", True, "slice"),                # 28
    (28, 28, 64, 64, 32, "tanh", True, "slice"),                 # 56
    (14, 14, 64, 32, 48, "raw", False, "panel"),                 # 21: three slices (seed columns), 32 output channels
    (28, 28, 32, 64, 16, "relu", False, "panel"),                # 28
    (14, 14, 64, 128, 48, "relu", True, "panel"),                # 42: three slices x two channel groups
    (14, 14, 64, 64, 16, "self", True, "panel"),                 # 7: SELF_RELU, primal data in the column slots
    (16, 16, 64, 64, 16, "relu", True, "panel"),                 # 8
    (32, 32, 64, 64, 32, "bits", False, "slice"),                # 128
    (8, 32, 32, 128, 16, "none", True, "panel"),                 # 16
    (16, 16, 128, 32, 48, "tanh", False, "panel"),               # 24
    (12, 24, 64, 64, 16, "raw", True, "slice"),                  # 9: unequal XCD ranges on 4 x 8 tiles
    (16, 16, 64, 128, 64, "relu", True, "slice"),                # 64
    (12, 24, 64, 64, 32, "none", False, "panel"),                # 18
    (16, 16, 64, 64, 16, "self", False, "panel"),                # 8: SELF_RELU on 4 x 8 tiles
]
_FWD_SMALL = [(14, 14, 64, 64, 16, "relu", True, "panel", "lt8"), (14, 14, 64, 64, 16, "bits", True, "panel", "ltG"),
              (16, 16, 64, 128, 16, "none", False, "slice", "ltG")]


def _factor(fmode, prim):
    """(factor multiplying x, the tensor the kernel reads it from) for a base primal tensor."""
    if fmode in ("none", "self"):
        return torch.ones_like(prim), None
    if fmode in ("relu", "bits"):
        return (prim > 0).float(), prim
    if fmode == "tanh":                                                    # the kernel reads t and forms 1 - t^2: float64 of THAT t
        return 1 - torch.tanh(prim).double() ** 2, torch.tanh(prim)
    return (prim > 0.3).float() * 1.5, (prim > 0.3).float() * 1.5


def _run_forward(H, W, cin, cout, nc, fmode, with_res, layout, regime):
    from cmf_amd import engine as E
    label = f"bf16x3 fwd {H}x{W} ci{cin} co{cout} nc{nc} {fmode}{' +res' if with_res else ''} {layout}"
    assert E._shape_ok_bf16x3(9, cin, W, False, H, cout), label
    per = P.forward_items(H, W, nc, cout, 1)
    np_ = _np_for(per, _cus(), regime)
    total = per * np_
    G, _ = _geometry(label, total, _cus(), per, regime)
    period, base_idx, scale = _plan(np_, per)
    gen = torch.Generator().manual_seed(H * 1000 + cin + cout + nc)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (9 * cin) ** 0.5
    xb = torch.randn(period, cin, H, W, nc, generator=gen)
    pb = torch.randn(period, cin, H, W, generator=gen)
    rb = torch.randn(period, cout, H, W, nc, generator=gen) if with_res else None
    fac, src = _factor(fmode, pb)
    xe = torch.relu(xb) if fmode == "self" else xb
    want, A = P.reference(_columns_to_batch(xe * fac.unsqueeze(-1)), w, None if rb is None else _columns_to_batch(rb))
    want, A = (_batch_to_columns(t, period, nc).reshape(period, cout, H * W, nc).cuda() for t in (want, A))
    s5 = scale.view(-1, 1, 1, 1, 1)
    L = _Layout(layout, H, W, nc)
    x = L.to_dev(xb.cuda()[base_idx] * s5)
    res = L.to_dev(rb.cuda()[base_idx] * s5) if with_res else None
    kw = {}
    if fmode == "bits":
        bits = E.relu_bits(pb.cuda()[base_idx].contiguous())
        kw = dict(fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes)
    elif fmode == "self":
        kw = dict(fmode=E.F_SELF_RELU)
    elif fmode != "none":
        kw = dict(fmode={"relu": E.F_RELU, "tanh": E.F_TANH, "raw": E.F_RAW}[fmode], f=src.cuda()[base_idx].contiguous(),
                  f_np=cin * H * W, f_ci=H * W, f_px=1)
    wd = torch.nn.Parameter(w.cuda())
    y = P.Guarded(np_ * cout * H * W * nc)
    _launch("cmf_conv_tangent_bf16x3", f"conv_tangent_t9_ci{cin}_co{cout}" + ("_primal" if fmode == "self" else ""),
            lambda: E.conv_tangent(x, 0, *L.st(cin), wd, 9, y.t, *L.st(cout), np_, cin, cout, H, W, nc, res_t=res, x_sl=L.sl(cin),
                                   y_sl=L.sl(cout), precision="bf16x3", **kw))
    y.check(label)
    got = L.from_dev(y.t, np_, cout)
    _check_values(label, got, want[base_idx] * s5.view(-1, 1, 1, 1).double(), A[base_idx] * s5.view(-1, 1, 1, 1).double(),
                  P.C_BF16X3, 2e-5)
    _check_copies(label, got, base_idx, scale, per, total, G, period)


@pytest.mark.parametrize("H,W,cin,cout,nc,fmode,with_res,layout", _FWD)
def test_bf16x3_forward_many_items_per_workgroup(H, W, cin, cout, nc, fmode, with_res, layout):
    _run_forward(H, W, cin, cout, nc, fmode, with_res, layout, "multi")


@pytest.mark.parametrize("H,W,cin,cout,nc,fmode,with_res,layout,regime", _FWD_SMALL)
def test_bf16x3_forward_fewer_items_than_workgroups(H, W, cin, cout, nc, fmode, with_res, layout, regime):
    """items < 8 and 8 <= items < CUs: as many workgroups as items, one item each (XCD ranges of length 0 and 1)."""
    _run_forward(H, W, cin, cout, nc, fmode, with_res, layout, regime)


# ---------------------------------------------------------------------------------------------------------------------------
# PLAIN transposed conv with the relu' OUTPUT bit mask, and the in-place skip form
@pytest.mark.parametrize("H,W,cl_out,cl_in,layout,regime", [(14, 14, 64, 64, "panel", "multi"), (8, 16, 64, 128, "slice", "multi"),
                                                            (28, 28, 64, 64, "slice", "multi"), (12, 24, 128, 64, "panel", "multi"),
                                                            (4, 14, 64, 64, "panel", "lt8"), (8, 8, 64, 64, "slice", "ltG")])
def test_bf16x3_transposed_conv_with_output_bit_mask_many_items(H, W, cl_out, cl_in, layout, regime):
    """y = [act > 0] . conv^T(x)  into a NaN-filled tensor (masked-off lanes store zeros), then  y <- y + [act > 0] . conv^T(x)  in
    place (masked-off lanes do not store: bit-identical to before)."""
    from cmf_amd import engine as E
    nc = 32
    label = f"bf16x3 transposed {H}x{W} ci{cl_out} co{cl_in} nc{nc} {layout}"
    per = P.forward_items(H, W, nc, cl_in, 1)
    np_ = _np_for(per, _cus(), regime)
    total = per * np_
    G, _ = _geometry(label, total, _cus(), per, regime)
    period, base_idx, scale = _plan(np_, per)
    gen = torch.Generator().manual_seed(H * W + cl_in)
    w = torch.randn(cl_out, cl_in, 3, 3, generator=gen) / (9 * cl_out) ** 0.5           # the LAYER's weight: cl_in -> cl_out
    xb = torch.randn(period, cl_out, H, W, nc, generator=gen)
    ab = torch.randn(period, cl_in, H, W, generator=gen)
    kb = torch.randn(period, cl_in, H, W, nc, generator=gen)
    on = (ab > 0).unsqueeze(-1)
    want, A = P.reference(_columns_to_batch(xb), w, transpose=True)
    want, A = (_batch_to_columns(t, period, nc) * on.double() for t in (want, A))
    flat = lambda t: t.reshape(period, cl_in, H * W, nc).cuda()
    s5 = scale.view(-1, 1, 1, 1, 1)
    s4 = scale.view(-1, 1, 1, 1).double()
    L = _Layout(layout, H, W, nc)
    x = L.to_dev(xb.cuda()[base_idx] * s5)
    bits = E.relu_bits(ab.cuda()[base_idx].contiguous())
    wd = torch.nn.Parameter(w.cuda())
    name = f"conv_tangent_t9_ci{cl_out}_co{cl_in}"
    y = P.Guarded(np_ * cl_in * H * W * nc)
    _launch("cmf_conv_tangent_bf16x3", name,
            lambda: E.conv_tangent(x, 0, *L.st(cl_out), wd, 9, y.t, *L.st(cl_in), np_, cl_out, cl_in, H, W, nc, fo=bits, transpose=True,
                                   x_sl=L.sl(cl_out), y_sl=L.sl(cl_in), precision="bf16x3"))
    y.check(label)
    got = L.from_dev(y.t, np_, cl_in)
    off = ~flat(on.expand(period, cl_in, H, W, nc))[base_idx]
    _check_values(label, got, flat(want)[base_idx] * s4, flat(A)[base_idx] * s4, P.C_BF16X3, 2e-5)
    assert bool((got[off] == 0).all()), f"{label}: masked-off lanes must store zeros"
    _check_copies(label, got, base_idx, scale, per, total, G, period)
    # in place: the skip connection is the output tensor
    label += " in place"
    y2 = P.Guarded(np_ * cl_in * H * W * nc)
    y2.t.copy_(L.to_dev(kb.cuda()[base_idx] * s5))
    before = y2.t.clone()
    _launch("cmf_conv_tangent_bf16x3", name,
            lambda: E.conv_tangent(x, 0, *L.st(cl_out), wd, 9, y2.t, *L.st(cl_in), np_, cl_out, cl_in, H, W, nc, fo=bits, transpose=True,
                                   x_sl=L.sl(cl_out), y_sl=L.sl(cl_in), res_t=y2.t, precision="bf16x3"))
    y2.check(label)
    got2 = L.from_dev(y2.t, np_, cl_in)
    _check_values(label, got2, (flat(want) + flat(kb).double())[base_idx] * s4, (flat(A) + flat(kb).double().abs())[base_idx] * s4,
                  P.C_BF16X3, 2e-5)
    assert torch.equal(got2[off], L.from_dev(before, np_, cl_in)[off]), f"{label}: masked-off lanes must keep what was in memory"
    _check_copies(label, got2, base_idx, scale, per, total, G, period)


# ---------------------------------------------------------------------------------------------------------------------------
# checkerboard output
@pytest.mark.parametrize("H,W,live,fmode,with_res,regime", [(14, 14, 1, "relu", True, "multi"), (14, 14, 2, "relu", False, "multi"),
                                                            (28, 28, 2, "bits", True, "multi"), (16, 16, 2, "bits", True, "multi"),
                                                            (16, 16, 1, "bits", False, "multi"), (12, 24, 1, "relu", True, "multi"),
                                                            (32, 32, 2, "relu", True, "multi"),
                                                            (4, 14, 2, "relu", True, "lt8"), (8, 8, 1, "bits", True, "ltG")])
def test_bf16x3_checkerboard_output_many_items(H, W, live, fmode, with_res, regime):
    """``live`` = 1 / 2: the pixels with (row + col) % 2 == live - 1, stored compactly into a NaN-filled tensor; the residual is read at
    those pixels of the FULL image (res_np = the full sample stride, twice the compact one)."""
    from cmf_amd import engine as E
    C, nc, HW = 64, 32, H * W
    label = f"bf16x3 checkerboard {H}x{W} live{live} {fmode}{' +res' if with_res else ''}"
    per = P.forward_items(H, W, nc, C, 1)
    np_ = _np_for(per, _cus(), regime)
    total = per * np_
    G, _ = _geometry(label, total, _cus(), per, regime)
    period, base_idx, scale = _plan(np_, per)
    gen = torch.Generator().manual_seed(H * 100 + W + live)
    w = torch.randn(C, C, 3, 3, generator=gen) / 24
    xb = torch.randn(period, C, H, W, nc, generator=gen)
    pb = torch.randn(period, C, H, W, generator=gen)
    rb = torch.randn(period, C, H, W, nc, generator=gen) if with_res else None
    want, A = P.reference(_columns_to_batch(xb * (pb > 0).float().unsqueeze(-1)), w, None if rb is None else _columns_to_batch(rb))
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sel = ((ii + jj) % 2 == live - 1).reshape(-1)                          # row-major order of the live pixels = the compact index
    assert int(sel.sum()) == HW // 2
    want, A = (_batch_to_columns(t, period, nc).reshape(period, C, HW, nc)[:, :, sel].cuda() for t in (want, A))
    s5, s4 = scale.view(-1, 1, 1, 1, 1), scale.view(-1, 1, 1, 1).double()
    L = _Layout("slice", H, W, nc)
    st, sl = L.st(C), L.sl(C)
    x = L.to_dev(xb.cuda()[base_idx] * s5)
    res = L.to_dev(rb.cuda()[base_idx] * s5) if with_res else None
    pd = pb.cuda()[base_idx].contiguous()
    bits = E.relu_bits(pd)
    fk = dict(fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes) if fmode == "bits" else dict(fmode=E.F_RELU, f=pd, f_np=C * HW, f_ci=HW, f_px=1)
    wd = torch.nn.Parameter(w.cuda())
    comp = P.Guarded(np_ * C * (HW // 2) * nc)
    _launch("cmf_conv_tangent_bf16x3", f"conv_tangent_t9_ci{C}_co{C}_live",
            lambda: E.conv_tangent(x, 0, *st, wd, 9, comp.t, st[0] // 2, st[1], st[2], np_, C, C, H, W, nc, res_t=res, x_sl=sl, y_sl=sl,
                                   precision="bf16x3", live=live, res_np=st[0], **fk))
    comp.check(label)
    got = L.from_dev(comp.t, np_, C, HW // 2)
    _check_values(label, got, want[base_idx] * s4, A[base_idx] * s4, P.C_BF16X3, 2e-5)
    _check_copies(label, got, base_idx, scale, per, total, G, period)


# ---------------------------------------------------------------------------------------------------------------------------
# cmf_conv_tangent_f16x3: the primal form, forward and backward
def _roll_plan(np_, per_sample):
    """fp16 form: copy i of base i % period holds the base group's 16 samples rotated by 5 (i // period) slots."""
    period = min(P.repeat_period(per_sample), np_)
    idx = torch.arange(np_)
    return period, (idx % period).cuda(), ((idx // period) * 5 % 16).tolist()


def _rolled(t, base_idx, rolls):
    """(period, ..., 16) -> (np, ..., 16): the copies, columns rotated."""
    out = t[base_idx].clone()
    for i, r in enumerate(rolls):
        if r:
            out[i] = torch.roll(out[i], r, dims=-1)
    return out


def _unpack_bits(mask, C):
    """(B, HW, C/8) uint8 -> bool (B, HW, C): bit j of byte o = channel 8 o + j."""
    return ((mask.to(torch.int32).unsqueeze(-1) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1).bool().flatten(2)


_F16 = [
    # H, W, item_channels, scale, residual, regime
    (14, 14, 64, 1.0, True, "multi"), (14, 14, 32, 3e4, False, "multi"), (28, 28, 64, 1e-4, True, "multi"),
    (28, 28, 32, 1.0, False, "multi"), (16, 16, 64, 3e4, True, "multi"), (8, 32, 32, 1e-4, True, "multi"),
    (12, 24, 32, 1.0, False, "multi"),
    (14, 14, 64, 1.0, True, "lt8"), (14, 14, 32, 1.0, True, "ltG"),
]


@pytest.mark.parametrize("H,W,item,scale,with_res,regime", _F16)
def test_f16x3_primal_forward_many_items(H, W, item, scale, with_res, regime):
    """Hidden primal conv, 16 samples in the column slots: relu on load, bias, residual against float64; the sign bits written for the
    next conv (a padded mask: the bytes between the samples' ranges stay untouched); amax_out == the largest stored value floored
    at 0, over every item of every workgroup."""
    from cmf_amd import engine as E
    C, HW = 64, H * W
    group = P.f16_item_group(H, W, item)
    label = f"f16x3 fwd {H}x{W} item{item}->{group} scale {scale:g}{' +res' if with_res else ''}"
    per = P.forward_items(H, W, 16, C, 1, group=group)
    np_ = _np_for(per, _cus(), regime)
    total = per * np_
    G, _ = _geometry(label, total, _cus(), per, regime)
    period, base_idx, rolls = _roll_plan(np_, per)
    gen = torch.Generator().manual_seed(H * W + item)
    w = torch.randn(C, C, 3, 3, generator=gen) / 24
    xb = scale * torch.randn(period, C, H, W, 16, generator=gen)
    bias = scale * torch.randn(C, generator=gen)
    rb = scale * torch.randn(period, C, H, W, 16, generator=gen) if with_res else None
    want, A = P.reference(_columns_to_batch(torch.relu(xb)), w, None if rb is None else _columns_to_batch(rb))
    want, A = want + bias.double().view(1, -1, 1, 1), A + bias.double().abs().view(1, -1, 1, 1)
    want, A = (_batch_to_columns(t, period, 16).reshape(period, C, HW, 16).cuda() for t in (want, A))
    x = _rolled(xb.cuda(), base_idx, rolls).reshape(-1)
    res = _rolled(rb.cuda(), base_idx, rolls).reshape(-1) if with_res else None
    wd = torch.nn.Parameter(w.cuda())
    pn = (C * HW * 16, HW * 16, 16)
    rng = torch.zeros(2, device="cuda")
    E.absmax(x, rng[0:1])
    assert float(rng[0]) == float(x.abs().max())
    y = P.Guarded(np_ * C * HW * 16)
    nbytes, pad = HW * C // 8, 64                                          # 64 untouched bytes after every sample's mask
    m = P.Guarded(np_ * 16 * (nbytes + pad), dtype=torch.uint8, fill=0xAA)
    _launch("cmf_conv_tangent_f16x3_item", f"conv_tangent_t9_ci{C}_co{C}_primal",
            lambda: E.conv_tangent(x, 0, *pn, wd, 9, y.t, *pn, np_, C, C, H, W, 16, fmode=E.F_SELF_RELU, bias=bias.cuda(), res_t=res,
                                   precision="f16x3", mask_out=m.t, mask_np=nbytes + pad, amax_in=rng[0:1], amax_out=rng[1:2],
                                   item_channels=item))
    y.check(label)
    m.check(label + " bit mask")
    got = y.t.reshape(np_, C, HW, 16)
    wantc, Ac = _rolled(want, base_idx, rolls), _rolled(A, base_idx, rolls)
    _check_values(label, got, wantc, Ac, P.C_F16X3, 1e-6)
    same = got == _rolled(got[:period], base_idx, rolls)
    assert bool(same.all()), f"{label}: copies differ from their rotated base group: {_first_bad(~same)}"
    assert float(rng[1]) == float(got.clamp_min(0).max()), (label, float(rng[1]), float(got.clamp_min(0).max()))
    mm = m.t.reshape(np_ * 16, nbytes + pad)
    assert bool((mm[:, nbytes:] == 0xAA).all()), f"{label}: bytes past a sample's mask were written"
    gbits = _unpack_bits(mm[:, :nbytes].reshape(np_ * 16, HW, C // 8), C)                 # (sample = group * 16 + column, HW, C)
    by_sample = lambda t: t.permute(0, 3, 2, 1).reshape(np_ * 16, HW, C)
    assert torch.equal(gbits, by_sample(got) > 0), f"{label}: the bit mask is not the sign of what was stored"
    sure = by_sample(wantc.abs() > P.C_F16X3 * Ac)
    assert float((~sure).double().mean()) <= 1e-3, (label, float((~sure).double().mean()))
    assert torch.equal(gbits[sure], (by_sample(wantc) > 0)[sure]), f"{label}: sign bits differ from the float64 result's"


@pytest.mark.parametrize("H,W,item,scale,with_res,regime", [
    (14, 14, 64, 1.0, True, "multi"), (28, 28, 32, 1e-4, False, "multi"), (16, 16, 64, 1.0, False, "multi"),
    (8, 32, 32, 3e4, True, "multi"), (28, 28, 64, 3e4, True, "multi"), (12, 24, 32, 1.0, True, "multi"),
    (14, 14, 64, 1.0, False, "lt8"), (16, 16, 32, 1.0, True, "ltG")])
def test_f16x3_primal_backward_many_items(H, W, item, scale, with_res, regime):
    """Data-gradient conv of the primal backward: plain cotangent in, the adjoint pack, per-sample relu' of the forward activation on
    the way out, optional residual; amax_out == max |stored| over every item of every workgroup."""
    from cmf_amd import engine as E
    C, HW = 64, H * W
    group = P.f16_item_group(H, W, item)
    label = f"f16x3 bwd {H}x{W} item{item}->{group} scale {scale:g}{' +res' if with_res else ''}"
    per = P.forward_items(H, W, 16, C, 1, group=group)
    np_ = _np_for(per, _cus(), regime)
    total = per * np_
    G, _ = _geometry(label, total, _cus(), per, regime)
    period, base_idx, rolls = _roll_plan(np_, per)
    gen = torch.Generator().manual_seed(H + W + item)
    w = torch.randn(C, C, 3, 3, generator=gen) / 24
    ab = torch.randn(period, C, H, W, 16, generator=gen)              # the forward activation whose relu the cotangent passes through
    gb = scale * torch.randn(period, C, H, W, 16, generator=gen)      # cotangent of y = conv2d(relu(act), w)
    rb = scale * torch.randn(period, C, H, W, 16, generator=gen) if with_res else None
    want, A = P.reference(_columns_to_batch(gb), w, transpose=True)
    on = (ab > 0).double()
    want, A = (_batch_to_columns(t, period, 16) * on for t in (want, A))
    if with_res:
        want, A = want + rb.double(), A + rb.double().abs()
    want, A = (t.reshape(period, C, HW, 16).cuda() for t in (want, A))
    gy = _rolled(gb.cuda(), base_idx, rolls).reshape(-1)
    act = _rolled(ab.cuda(), base_idx, rolls).reshape(-1)
    res = _rolled(rb.cuda(), base_idx, rolls).reshape(-1) if with_res else None
    wd = torch.nn.Parameter(w.cuda())
    pn = (C * HW * 16, HW * 16, 16)
    rng = torch.zeros(2, device="cuda")
    E.absmax(gy, rng[0:1])
    y = P.Guarded(np_ * C * HW * 16)
    _launch("cmf_conv_tangent_f16x3_item", f"conv_tangent_t9_ci{C}_co{C}_primal_bwd",
            lambda: E.conv_tangent(gy, 0, *pn, wd, 9, y.t, *pn, np_, C, C, H, W, 16, transpose=True, precision="f16x3", res_t=res,
                                   fo=act, fo_np=pn[0], fo_co=pn[1], fo_px=pn[2], fomode=E.F_SELF_RELU, amax_in=rng[0:1],
                                   amax_out=rng[1:2], item_channels=item))
    y.check(label)
    got = y.t.reshape(np_, C, HW, 16)
    _check_values(label, got, _rolled(want, base_idx, rolls), _rolled(A, base_idx, rolls), P.C_F16X3, 1e-6)
    same = got == _rolled(got[:period], base_idx, rolls)
    assert bool(same.all()), f"{label}: copies differ from their rotated base group: {_first_bad(~same)}"
    assert float(rng[1]) == float(got.abs().max()), (label, float(rng[1]), float(got.abs().max()))
    if not with_res:
        assert bool((got[act.reshape(np_, C, HW, 16) <= 0] == 0).all()), f"{label}: masked exactly, not approximately"


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradients
def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _check_wgrad_elements(label, dw, prev, xe, gb, fac, weights, arithmetic, R):
    """Every entry of the accumulated gradient within  c A + 2^-24 (|prev| + |want|)  of float64 (tests/_wgrad_elements.py): the
    copies are exact power-of-two multiples of their base samples, so want and A of the batch are those of the base samples with x
    times the copies' summed scales."""
    xw = xe.double() * weights.view(-1, 1, 1, 1, 1)
    want, A = WE.reference(xw, gb, None if fac is None else fac.double(), prev)
    WE.check_elements(label, dw.t.view(prev.shape).cpu(), want, A, prev, arithmetic, R, tag="PERSISTENT_ITEMS")


def _wgrad_reference(xb, gb, fac, weights, cout, cin):
    """float64 autograd of  sum_b weights_b <gy_b, conv(F x_b)>  with respect to w (at w = 0: the product is linear in w)."""
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(_columns_to_batch(xb * fac.unsqueeze(-1)).double(), w, padding=1)
    gy = _columns_to_batch(gb * weights.view(-1, 1, 1, 1, 1)).double()
    (y * gy).sum().backward()
    return w.grad


_WGRAD = [
    # precision, cin, cout, H, W, nc, fmode, layout, regime
    ("bf16x3", 64, 64, 14, 14, 32, "relu", "panel", "multi"), ("bf16x3", 128, 64, 14, 14, 32, "bits", "slice", "multi"),
    ("bf16x3", 64, 64, 16, 16, 32, "self", "panel", "multi"), ("bf16x3", 64, 128, 8, 16, 64, "none", "slice", "multi"),
    ("bf16x3", 64, 64, 4, 14, 32, "relu", "panel", "lt8"), ("bf16x3", 64, 64, 4, 14, 32, "self", "slice", "ltG"),
    ("f32", 64, 64, 14, 14, 16, "tanh", "panel", "multi"), ("f32", 32, 64, 16, 16, 32, "relu", "panel", "multi"),
    ("f32", 17, 40, 5, 7, 32, "self", "slice", "multi"), ("f32", 64, 32, 14, 14, 16, "none", "slice", "multi"),
    ("f32", 64, 64, 4, 14, 16, "tanh", "panel", "lt8"), ("f32", 32, 64, 4, 8, 16, "relu", "panel", "ltG"),
]


@pytest.mark.parametrize("precision,cin,cout,H,W,nc,fmode,layout,regime", _WGRAD)
def test_weight_gradient_many_rows_per_workgroup(precision, cin, cout, H, W, nc, fmode, layout, regime):
    """dW of <gy, conv(F x)> accumulated into a non-zero gradient, against float64 autograd: the split kernel (rows dealt XCD-aware)
    and the fp32 row-walking kernel (contiguous blocks of rows), every workgroup walking several image rows.  Max-norm, and every
    entry within c A + 2^-24 (|prev| + |want|), A = sum |gy| |F x| (tests/_wgrad_elements.py)."""
    from cmf_amd import engine as E
    split = precision == "bf16x3"
    label = f"wgrad {precision} {H}x{W} ci{cin} co{cout} nc{nc} {fmode} {layout}"
    per = P.wgrad_rows_split(H, nc, 1) if split else P.wgrad_rows_f32(H, nc, 1)
    np_ = _np_for(per, P.WG_MAX, regime)
    total = per * np_
    _geometry(label, total, P.WG_MAX, per, regime, P.xcd_counts if split else P.block_counts)
    period, base_idx, scale = _plan(np_, per)
    gen = torch.Generator().manual_seed(cin * 1000 + cout + H)
    xb = torch.randn(period, cin, H, W, nc, generator=gen)
    gb = torch.randn(period, cout, H, W, nc, generator=gen)
    pb = torch.randn(period, cin, H, W, generator=gen)
    fac, src = _factor("relu" if fmode == "bits" else fmode, pb)
    weights = torch.zeros(period, dtype=torch.float64).index_add_(0, base_idx.cpu(), scale.cpu().double())
    want = _wgrad_reference(torch.relu(xb) if fmode == "self" else xb, gb, fac, weights, cout, cin)
    L = _Layout(layout, H, W, nc)
    x = L.to_dev(xb.cuda()[base_idx] * scale.view(-1, 1, 1, 1, 1))               # the copies' inputs scaled, their cotangents not
    gy = L.to_dev(gb.cuda()[base_idx])
    f = None
    if fmode == "bits":
        f = E.relu_bits(pb.cuda()[base_idx].contiguous())
    elif src is not None:
        f = src.cuda()[base_idx].contiguous()
    prev = torch.randn(cout, cin, 3, 3, generator=gen)
    dw = P.Guarded(cout * cin * 9)
    dw.t.copy_(prev.reshape(-1))
    _launch("cmf_conv_tangent_wgrad_bf16x3" if split else "cmf_conv_tangent_wgrad", f"conv_wgrad_t9_ci{cin}_co{cout}" + ("_primal" if fmode == "self" else ""),
            lambda: E.conv_tangent_wgrad(x, 0, *L.st(cin), gy, 0, *L.st(cout), dw.t.view(cout, cin, 3, 3), 9, np_, cin, cout, H, W, nc,
                                         fmode={"none": E.F_NONE, "relu": E.F_RELU, "tanh": E.F_TANH, "self": E.F_SELF_RELU, "bits": E.F_NONE}[fmode],
                                         f=f, f_np=cin * H * W, f_ci=H * W, f_px=1, x_sl=L.sl(cin), y_sl=L.sl(cout), precision=precision))
    dw.check(label)
    got = dw.t.view(cout, cin, 3, 3).cpu() - prev
    err = _rel(got, want)
    print(f"PERSISTENT_ITEMS {label}: max-norm error {err:.2e} (bound {5e-5 if split else 2e-5:.0e})")
    assert err < (5e-5 if split else 2e-5), (label, err)
    _check_wgrad_elements(label, dw, prev, torch.relu(xb) if fmode == "self" else xb, gb, fac, weights, precision, np_ * H * W * nc)


@pytest.mark.parametrize("H,W,fmode,nprob,regime", [(14, 14, "self", 5, "multi"), (16, 16, "none", 3, "multi"), (4, 14, "self", 5, "lt8"),
                                                    (14, 14, "none", 16, "ltG")])
def test_batched_weight_gradient_many_rows_per_workgroup(H, W, fmode, nprob, regime):
    """cmf_conv_tangent_wgrad_bf16x3_batched: ``nprob`` problems of one shape on (256 / nprob) & ~7 workgroups each (sample groups
    paired as the two 16-column slices of a 32-column sample), accumulated into non-zero gradients, against float64 autograd."""
    from cmf_amd import engine as E
    C, HW, nc = 64, H * W, 32
    label = f"wgrad batched x{nprob} {H}x{W} {fmode}"
    wgp = (P.WG_MAX // nprob) & ~7
    per = P.wgrad_rows_split(H, nc, 1)
    np_ = _np_for(per, wgp, regime)
    total = per * np_
    _geometry(label, total, wgp, per, regime, fixed=True)
    period, base_idx, scale = _plan(np_, per)
    gs = C * HW * 16
    to_dev = lambda t: t.reshape(t.shape[0], C, HW, 2, 16).permute(0, 3, 1, 2, 4).contiguous().reshape(-1)   # [sample][slice][channel][pixel][16]
    weights = torch.zeros(period, dtype=torch.float64).index_add_(0, base_idx.cpu(), scale.cpu().double())
    xs, gys, dws, prevs, wants, xes, gbs = [], [], [], [], [], [], []
    for p in range(nprob):
        gen = torch.Generator().manual_seed(100 * H + p)
        xb = torch.randn(period, C, H, W, nc, generator=gen)
        gb = torch.randn(period, C, H, W, nc, generator=gen)
        wants.append(_wgrad_reference(torch.relu(xb) if fmode == "self" else xb, gb, torch.ones(period, C, H, W), weights, C, C))
        xes.append(torch.relu(xb) if fmode == "self" else xb)
        gbs.append(gb)
        xs.append(to_dev(xb.cuda()[base_idx] * scale.view(-1, 1, 1, 1, 1)))
        gys.append(to_dev(gb.cuda()[base_idx]))
        prevs.append(torch.randn(C, C, 3, 3, generator=gen))
        dws.append(P.Guarded(C * C * 9))
        dws[-1].t.copy_(prevs[-1].reshape(-1))
    _launch("cmf_conv_tangent_wgrad_bf16x3_batched", f"conv_wgrad_t9_ci{C}_co{C}" + ("_primal" if fmode == "self" else "") + "_batched",
            lambda: E.conv_tangent_wgrad_batched(xs, gys, [d.t.view(C, C, 3, 3) for d in dws], 2 * gs, HW * 16, 16, 2 * gs, HW * 16, 16,
                                                 np_, C, C, H, W, nc, fmode=E.F_SELF_RELU if fmode == "self" else E.F_NONE, x_sl=gs, y_sl=gs))
    worst = 0.0
    for p in range(nprob):
        dws[p].check(f"{label} problem {p}")
        err = _rel(dws[p].t.view(C, C, 3, 3).cpu() - prevs[p], wants[p])
        worst = max(worst, err)
        assert err < 5e-5, (label, p, err)
        _check_wgrad_elements(f"{label} problem {p}", dws[p], prevs[p], xes[p], gbs[p], None, weights, "bf16x3", np_ * H * W * nc)
    print(f"PERSISTENT_ITEMS {label}: max-norm error {worst:.2e} (bound 5e-05)")
