"""The weight-gradient kernels against float64, per element (``-m gpu``).

conv_wgrad.hip (row-walking 3x3, thin 3x3 with 1 .. 4 column tiles, thin and general 1x1, wgrad_reduce_kernel) and
conv_wgrad_bf16x3.hip (single and batched) at the smallest shapes at which each can go wrong -- partial 64-blocks, one-row and
one- to three-column images, cout on both sides of the thin / general 1x1 boundary, every factor mode each family implements --
with the inputs, the bound  |got - want| <= c A + 2^-24 (|prev| + |want|)  and the constants of tests/_wgrad_elements.py (their
derivation is there; tests/test_wgrad_elements_host.py checks it on the CPU).  Every case

* accumulates into a non-zero ``prev`` inside a guard-banded buffer and asserts the C ABI symbol and the launch name reached; the
  kernel family inside cmf_conv_tangent_wgrad follows from the shape rules that tests/test_wgrad_elements_host.py pins to the
  dispatch's source lines, and is printed;
* asserts the per-element bound, the rigorous (R + 9) 2^-24 A for the fp32 kernels and the older tensor-wide bound unchanged, and
  prints max err / A (profiles/wgrad_elements_errors.txt);
* asserts that entries without any non-zero product (A == 0: six of nine taps of a one-row image) keep ``prev`` bit for bit;
* launches again and asserts the same bits;
* channel isolation: with prev = 0, dw(graded channel scales) == dw(all scales 1) s_co s_ci bit for bit -- no product of one
  channel reaches another's sum;
* relu / bits / self: the float64 reference takes [f > 0] of a source with +0.0, -0.0 and 2^-149 sprinkled in.

A covering set: the row-walking, thin one-row and split shapes run every factor mode; cin = 1 .. 7 of the thin 3x3 form each run
every factor mode, spread over (cout 64 | 24) x (5 x 6 | 8 x 8) so that every cin meets all four shapes; 1x1 launches have no
factor mode in use.  np = 3 with sample 1 all zeros."""
import ctypes as C

import pytest
import torch

import _persistent_items as P
import _wgrad_elements as WE
from test_gpu_persistent_items import _Layout, _launch

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c.id for c in cases]


def _fmode(E, case):
    return {"none": E.F_NONE, "relu": E.F_RELU, "tanh": E.F_TANH, "raw": E.F_RAW, "self": E.F_SELF_RELU, "bits": E.F_NONE}[case.fmode]


def _factor_args(E, case, d):
    """(f tensor or BitMask, f_np, f_ci, f_px) as the kernels address the factor source."""
    HW = case.H * case.W
    if d.src is None:
        return None, 0, 0, 0
    src = d.src.cuda().contiguous()
    if case.fmode == "bits":
        return E.relu_bits(src), 0, 0, 0
    if case.f_group > 1:                              # [group][channel][pixel][slot]: sample n in slot n % 16; the other slots say "live"
        assert case.np <= case.f_group
        grouped = torch.ones(1, case.cin, HW, case.f_group, device="cuda")
        grouped[0, :, :, :case.np] = src.reshape(case.np, case.cin, HW).permute(1, 2, 0)
        return grouped.contiguous(), case.cin * HW * case.f_group, HW * case.f_group, case.f_group
    return src, case.cin * HW, HW, 1


def _operands(E, case, d):
    L = _Layout(case.layout, case.H, case.W, case.nc)
    return L, L.to_dev(d.x.cuda()), L.to_dev(d.gy.cuda()), _factor_args(E, case, d)


def _run(case, d, prev, assert_family=False):
    """One engine launch accumulating into a guard-banded copy of ``prev``; returns dw on the CPU."""
    from cmf_amd import engine as E
    c = case
    L, x, gy, (f, f_np, f_ci, f_px) = _operands(E, c, d)
    dw = P.Guarded(c.cout * c.cin * c.taps)
    dw.t.copy_(prev.reshape(-1))
    call = lambda: E.conv_tangent_wgrad(x, 0, *L.st(c.cin), gy, 0, *L.st(c.cout), dw.t.view(c.cout, c.cin, c.k, c.k), c.taps, c.np, c.cin,
                                        c.cout, c.H, c.W, c.nc, fmode=_fmode(E, c), f=f, f_np=f_np, f_ci=f_ci, f_px=f_px,
                                        f_group=c.f_group, x_sl=L.sl(c.cin), y_sl=L.sl(c.cout), precision=c.precision)
    if assert_family:
        _launch("cmf_conv_tangent_wgrad_bf16x3" if c.family == "split" else "cmf_conv_tangent_wgrad",
                f"conv_wgrad_t{c.taps}_ci{c.cin}_co{c.cout}" + ("_primal" if c.fmode == "self" else ""), call)
    else:
        call()
    torch.cuda.synchronize()
    dw.check(c.id)
    return dw.t.view(c.cout, c.cin, c.k, c.k).cpu()


def _check_case(case, run):
    """``run(data, prev, assert_family)`` -> dw (CPU): the assertions shared by the single and the batched launches."""
    d = WE.case_data(case)
    got = run(d, d.prev, True)
    WE.check_elements(f"{case.id} [{case.family}, {case.geometry()[1]} workgroups]", got, d.want, d.A, d.prev, case.arithmetic, case.R)
    assert torch.equal(run(d, d.prev, False), got), f"{case.id}: a second launch gives other bits"
    unit = WE.make_data(case, graded=False)
    zero = torch.zeros_like(d.prev)
    sc = d.s_co.view(-1, 1, 1, 1) * d.s_ci.view(1, -1, 1, 1)
    g0, u0 = run(d, zero, False), run(unit, zero, False)
    same = g0 == u0 * sc
    assert bool(same.all()), (f"{case.id}: dw(graded scales) != dw(unit scales) s_co s_ci at {int((~same).sum())} entries, first "
                              f"(co, ci, ky, kx) {(~same).nonzero()[:5].tolist()}")


@pytest.mark.parametrize("case", WE.CASES, ids=_ids(WE.CASES))
def test_weight_gradient_elements(case):
    _check_case(case, lambda d, prev, fam: _run(case, d, prev, fam))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WE.BATCHED, ids=_ids(WE.BATCHED))
def test_batched_weight_gradient_elements(case):
    """cmf_conv_tangent_wgrad_bf16x3_batched: ``nprob`` problems (the case's inputs drawn with seeds 0 .. nprob - 1) in one launch,
    every problem held to the assertions of the single launches."""
    from cmf_amd import engine as E
    c = case
    Cc, HW = 64, c.H * c.W
    gs = Cc * HW * 16
    to_dev = lambda t: t.cuda().reshape(t.shape[0], Cc, HW, 2, 16).permute(0, 3, 1, 2, 4).contiguous().reshape(-1)   # [sample][slice][channel][pixel][16]
    name = f"conv_wgrad_t9_ci{Cc}_co{Cc}" + ("_primal" if c.fmode == "self" else "") + "_batched"

    def launch(datas, prevs, assert_family):
        xs, gys = [to_dev(d.x) for d in datas], [to_dev(d.gy) for d in datas]
        dws = [P.Guarded(Cc * Cc * 9) for _ in datas]
        for dw, prev in zip(dws, prevs):
            dw.t.copy_(prev.reshape(-1))
        call = lambda: E.conv_tangent_wgrad_batched(xs, gys, [dw.t.view(Cc, Cc, 3, 3) for dw in dws], 2 * gs, HW * 16, 16, 2 * gs, HW * 16, 16,
                                                    c.np, Cc, Cc, c.H, c.W, c.nc, fmode=_fmode(E, c), x_sl=gs, y_sl=gs)
        if assert_family:
            _launch("cmf_conv_tangent_wgrad_bf16x3_batched", name, call)
        else:
            call()
        torch.cuda.synchronize()
        for p, dw in enumerate(dws):
            dw.check(f"{c.id} problem {p}")
        return [dw.t.view(Cc, Cc, 3, 3).cpu() for dw in dws]

    graded = [WE.case_data(c, seed=p) for p in range(c.nprob)]
    prevs = [d.prev for d in graded]
    got = launch(graded, prevs, True)
    for p, d in enumerate(graded):
        WE.check_elements(f"{c.id} problem {p} [{c.geometry()[1]} workgroups]", got[p], d.want, d.A, d.prev, "bf16x3", c.R)
    again = launch(graded, prevs, False)
    assert all(torch.equal(a, b) for a, b in zip(again, got)), f"{c.id}: a second launch gives other bits"
    zeros = [torch.zeros_like(p) for p in prevs]
    g0 = launch(graded, zeros, False)
    u0 = launch([WE.make_data(c, seed=p, graded=False) for p in range(c.nprob)], zeros, False)
    sc = graded[0].s_co.view(-1, 1, 1, 1) * graded[0].s_ci.view(1, -1, 1, 1)
    for p in range(c.nprob):
        assert torch.equal(g0[p], u0[p] * sc), f"{c.id} problem {p}: dw(graded scales) != dw(unit scales) s_co s_ci"


# ---------------------------------------------------------------------------------------------------------------------------
_FRESH = [next(c for c in WE.CASES if c.family == "rows3x3" and c.cin == 17 and c.fmode == "none"),
          next(c for c in WE.CASES if c.family == "thin1x1" and c.cin == 130)]


@pytest.mark.parametrize("case", _FRESH, ids=_ids(_FRESH))
def test_reduction_reads_only_blocks_this_launch_wrote(case):
    """wgrad_reduce_kernel sums the partial blocks of every workgroup of the launch from a workspace that is reused between launches,
    and waves whose tiles lie past cout / cin return without writing (cin 17, cout 40: five of eight waves; 130 x 12 1x1: a last
    64-block of two channels).  Through the C ABI with a workspace of the test's own that is all NaN before the launch, the result
    must be finite and equal the engine call's bit for bit."""
    from cmf_amd import engine as E, _lib
    c = case
    d = WE.case_data(c)
    want = _run(c, d, d.prev)
    lib = _lib.load()
    L, x, gy, (f, f_np, f_ci, f_px) = _operands(E, c, d)
    a = E.ConvTangentArgs()
    a.x = C.c_void_p(x.data_ptr()); a.x_np, a.x_ci, a.x_px = L.st(c.cin)
    a.f = E._p(f); a.f_np, a.f_ci, a.f_px, a.fmode, a.f_group = f_np, f_ci, f_px, _fmode(E, c), c.f_group
    a.y_np, a.y_co, a.y_px = L.st(c.cout)
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps = c.np, c.cin, c.cout, c.H, c.W, c.nc, c.taps
    a.x_sl, a.y_sl = L.sl(c.cin), L.sl(c.cout)
    need = int(lib.cmf_conv_tangent_wgrad_ws(C.byref(a)))
    assert need == P.WG_MAX * 64 * 64 * c.taps * 4
    ws = P.Guarded(need // 4)                                              # NaN-filled, guard-banded
    dw = P.Guarded(c.cout * c.cin * c.taps)
    dw.t.copy_(d.prev.reshape(-1))
    _lib.check(lib.cmf_conv_tangent_wgrad(C.byref(a), C.c_void_p(gy.data_ptr()), E._p(dw.t), E._p(ws.t), need, E._stream()), "cmf_conv_tangent_wgrad")
    torch.cuda.synchronize()
    ws.check(f"{c.id} workspace")
    dw.check(c.id)
    got = dw.t.view(c.cout, c.cin, c.k, c.k).cpu()
    assert bool(torch.isfinite(got).all()), f"{c.id}: the reduction read a block this launch did not write"
    assert torch.equal(got, want), f"{c.id}: the result depends on what the workspace held before"
