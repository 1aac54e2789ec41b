"""The fused MLP coupling layer (cmf_mlp_coupler, cmf_pack_mlp_layer) against float64, per element, on every launch path (``-m gpu``).

mlp_coupler_kernel<HT, TAN, NW> for HT = 1, 2, 8, both modes and both workgroup sizes, and mlp_coupler_split_kernel, each on one
tile, on a ragged tile and on more tiles than workgroups (the persistent loop carrying its weight double buffer and buffer parity
from one tile to the next, with odd and even layer counts, one and two workgroups per CU), with the inputs, the running bound and
the constants of tests/_mlp_coupler_elements.py (their derivation is there; tests/test_mlp_coupler_elements_host.py checks it on
the CPU and pins the dispatch mirror to the launcher's source lines).  The batch sizes follow from the device's CU count.

Layers are built with ``bijections._ChannelwiseACL`` directly, which reaches chan_off, chan_step and cin values the alternating
layer cannot.  Every case holds z, the fmajor tangent buffer and lj in guard-banded buffers, runs through ``layer.decode_`` /
``layer.encode_`` with the fused path on, asserts the launch's timer name, prints the variant, and asserts

1. the per-element bound on z, on every tangent element and on lj, next to the older tensor-wide 5e-6, printing max err / bound
   (profiles/mlp_coupler_errors.txt);
2. that guard bands, pass-through elements of z, pass-through rows of the tangent, tangent columns >= ncols (NaN-filled) and an
   lj buffer the launch was not given keep their bits;
3. the same bits from a second launch on restored inputs;
4. column isolation: the tangent output with column j scaled by 2^-(3 j) equals the unit-scale output times 2^-(3 j) bit for bit
   (another column's or sample's data leaking through a shared 16-column tile would break it);
5. position invariance: the batch in reverse order gives every sample the same bits (no arithmetic of a column depends on its
   tile, wave or slot);
6. for HT <= 2, that the primal the TANGENT mode writes equals the PRIMAL-mode decode bit for bit (the split kernel that wide
   networks reach in PRIMAL mode sums in another order: both are held to the bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mlp_coupler_elements as M
import _persistent_items as P

pytestmark = pytest.mark.gpu

EINVAL = -1                                                              # CMF_EINVAL (include/cmf_amd.h)

_ids = [c.id for c in M.CASES]
_bits = lambda t: t.contiguous().view(torch.int32)
_same = lambda a, b: torch.equal(_bits(a), _bits(b))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _layer(case, d):
    from torch import nn
    from cmf_amd.bijections import _ChannelwiseACL
    from cmf_amd.networks import ChunkedSharedCoupler, get_mlp
    layer = _ChannelwiseACL((case.D,), lambda npass: ChunkedSharedCoupler(get_mlp(npass, case.hidden, 2 * case.cmod)),
                            np.asarray(case.pass_idx), np.asarray(case.mod_idx)).cuda()
    lins = [m for m in layer.net if isinstance(m, nn.Linear)]
    assert [l.in_features for l in lins] + [lins[-1].out_features] == case.widths
    with torch.no_grad():
        for lin, (W, b) in zip(lins, d.net):
            lin.weight.copy_(W)
            lin.bias.copy_(b)
    v = layer.view("cuda")
    assert (v.chan_off, v.cin) == (case.pass_idx[0], len(case.pass_idx))
    assert [v.chan_off + i * v.chan_step for i in range(v.cin)] == case.pass_idx
    return layer


class _Out:
    pass


def _run(layer, case, d, mode, V=None, reverse=False):
    """One fused launch of ``mode`` on guard-banded copies of the case's inputs (``reverse``: the batch in reverse order, handed
    back in the original order).  CPU tensors: z (B, D), T (D, B, 16) raw, lj (B,) and the lj buffer the launch did not get."""
    from cmf_amd import engine as E
    B, D, nc = d.B, case.D, case.ncols
    flip = (lambda t, dim=0: t.flip(dim)) if reverse else (lambda t, dim=0: t)
    z, lj, other = P.Guarded(B * D), P.Guarded(B), P.Guarded(B)
    z.t.copy_(flip(d.z).reshape(-1))
    lj.t.copy_(flip(d.lj0))
    other.t.copy_(flip(d.lj0))
    zt, T, Tg = z.t.view(B, D), None, None
    if mode == "tangent":
        Tg = P.Guarded(D * B * 16)                                       # NaN: no column >= ncols is ever read
        Tg.t.view(D, B, 16)[:, :, :nc] = flip(V).permute(1, 0, 2)
        T = E.Tangent(B, D, 16, "fmajor", "cuda", data=Tg.t)
    assert E.FUSED_MLP
    with E.timing(lambda name: True) as timer, torch.no_grad():
        if mode == "tangent":
            layer.decode_(zt, T, ncols=nc)
        elif mode == "decode":
            layer.decode_(zt, None, lj.t)
        else:
            layer.encode_(zt, lj.t)
    names = set(timer.by_name())                                         # synchronises
    assert names == {"mlp_coupler_tangent" if mode == "tangent" else "mlp_coupler_primal"}, names
    for g, what in ((z, "z"), (lj, "lj"), (other, "the other lj"), (Tg, "tangent")):
        if g is not None:
            g.check(f"{case.id} {mode} {what}")
    o = _Out()
    o.z, o.lj, o.other = flip(zt.cpu()), flip(lj.t.cpu()), flip(other.t.cpu())
    o.T = flip(Tg.t.view(D, B, 16).cpu(), 1) if Tg is not None else None
    return o


def _equal(a, b):
    return _same(a.z, b.z) and _same(a.lj, b.lj) and (a.T is None or _same(a.T, b.T))


@pytest.mark.parametrize("case", M.CASES, ids=_ids)
def test_mlp_coupler_elements(case):
    cus = _cus()
    d, v = M.case_data(case, cus), case.variant(cus)
    print(f"\nMLP_COUPLER_ELEMENTS {case.id}: B = {d.B} on {cus} CUs, widths {case.widths}, {case.weights} weights -> {v}")
    assert v.path == case.want_path, (case.id, cus, v)
    layer = _layer(case, d)
    nc, mod = case.ncols, case.mod_idx
    keep = [i for i in range(case.D) if i not in mod]
    got = {}
    for mode in case.modes:
        ref = d.ref[mode]
        label = f"{case.id} {mode} [{M.kernel_of(case, cus, mode)}]"
        if mode != "tangent" and case.tangent:
            print(f"MLP_COUPLER_ELEMENTS {case.id}: PRIMAL-mode decode of the same inputs -> {case.variant(cus, None)}")
        o = got[mode] = _run(layer, case, d, mode, d.V)
        # 1. per element, and the older tensor-wide figure
        dense = o.T[:, :, :nc].permute(1, 0, 2) if mode == "tangent" else None
        M.check_elements(label, ref, o.z, dense, None if mode == "tangent" else o.lj)
        # 2. what the launch must not touch
        assert _same(o.z[:, keep], d.z[:, keep]), f"{label}: pass-through elements of z changed"
        assert _same(o.other, d.lj0), f"{label}: an lj buffer the launch was not given changed"
        if mode == "tangent":
            assert _same(o.lj, d.lj0), f"{label}: lj changed in TANGENT mode"
            assert _same(o.T[keep][:, :, :nc], d.V.permute(1, 0, 2)[keep]), f"{label}: pass-through rows of the tangent changed"
            assert bool(torch.isnan(o.T[:, :, nc:]).all()) and _same(o.T[:, :, nc:], torch.full_like(o.T[:, :, nc:], float("nan"))), \
                f"{label}: tangent columns >= ncols changed"
        # 3. again, on restored inputs
        assert _equal(_run(layer, case, d, mode, d.V), o), f"{label}: a second launch gives other bits"
        # 5. the batch in reverse order: another tile, wave and slot for every sample
        rev = _run(layer, case, d, mode, d.V, reverse=True)
        for name, a, b in (("z", rev.z, o.z), ("lj", rev.lj, o.lj), ("T", rev.T, o.T)):
            if a is not None:
                diff = _bits(a) != _bits(b)
                assert not bool(diff.any()), (f"{label}: {name} of {int(diff.sum())} elements depends on the sample's position in the batch, "
                                              f"first {diff.nonzero()[:5].tolist()}")
    if case.tangent:
        # 4. column isolation
        sc = M.column_scales(nc)
        unit = _run(layer, case, d, "tangent", d.Vu)
        diff = _bits(got["tangent"].T[:, :, :nc]) != _bits(unit.T[:, :, :nc] * sc)
        assert not bool(diff.any()), (f"{case.id}: T(graded columns) != T(unit columns) 2^-(3 j) at {int(diff.sum())} elements, first "
                                      f"(row, sample, column) {diff.nonzero()[:5].tolist()}")
        assert _same(unit.z, got["tangent"].z)
        # 6. the primal of the TANGENT mode against the PRIMAL mode
        if v.HT <= 2:
            assert case.variant(cus, None).kernel == "primal"
            assert _same(got["tangent"].z, got["decode"].z), f"{case.id}: the TANGENT mode's primal differs from the PRIMAL mode's"


# ---------------------------------------------------------------------------------------------------------------------------
# cmf_pack_mlp_layer through the C ABI
@pytest.mark.parametrize("out_f,in_f", [(10, 3), (33, 21), (128, 128), (64, 128)])
def test_pack_mlp_layer_is_pack_image(out_f, in_f):
    """The packed image, into a NaN-filled guard-banded buffer, equals ``pack_image`` bit for bit: first and later layers, the tile
    counts the sizes need and larger ones (hidden layers are padded to HT tiles), with and without a bias, and the size query."""
    from cmf_amd import _lib, engine as E
    lib = _lib.load()
    gen = torch.Generator().manual_seed(out_f * 1000 + in_f)
    W, b = torch.randn(out_f, in_f, generator=gen), torch.randn(out_f, generator=gen)
    Wd, bd = W.cuda(), b.cuda()
    mt0, kg0 = M.ceil_div(out_f, 16), M.ceil_div(in_f, 16)
    for first in (1, 0):
        for n_mt, n_kg in sorted({(mt0, kg0), (8, kg0), (mt0, 8), (8, 8), (mt0 + 1, kg0 + 1)}):
            n = C.c_longlong(-1)
            assert lib.cmf_pack_mlp_layer(None, None, out_f, in_f, first, n_mt, n_kg, None, C.byref(n), None) == 0
            assert n.value == M.image_floats(n_mt, n_kg)
            for bias in (bd, None):
                out = P.Guarded(n.value)
                n2 = C.c_longlong(-1)
                rc = lib.cmf_pack_mlp_layer(E._p(Wd), E._p(bias), out_f, in_f, first, n_mt, n_kg, E._p(out.t), C.byref(n2), E._stream())
                torch.cuda.synchronize()
                assert rc == 0 and n2.value == n.value
                out.check(f"pack {out_f}x{in_f} first={first} tiles {n_mt}x{n_kg}")
                want = torch.from_numpy(M.pack_image(W.numpy(), None if bias is None else b.numpy(), bool(first), n_mt, n_kg))
                assert _same(out.t.cpu(), want), (out_f, in_f, first, n_mt, n_kg, bias is not None)
    assert lib.cmf_pack_mlp_layer(None, None, out_f, in_f, 0, mt0, kg0, None, None, None) == EINVAL
    assert lib.cmf_pack_mlp_layer(E._p(Wd), None, out_f, in_f, 0, mt0 - 1, kg0, None, C.byref(C.c_longlong(0)), None) == EINVAL
    assert lib.cmf_pack_mlp_layer(E._p(Wd), None, out_f, in_f, 0, mt0, kg0 - 1, None, C.byref(C.c_longlong(0)), None) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# cmf_mlp_coupler's argument checks
def test_mlp_coupler_rejects_bad_arguments_without_launching():
    """Every argument the header rules out comes back CMF_EINVAL and leaves z, the tangent and lj as they were; the same
    arguments without the defect launch and change them."""
    from cmf_amd import _lib, engine as E
    lib = _lib.load()
    B, D, cin, hid, cm = 5, 5, 3, 10, 2
    gen = torch.Generator().manual_seed(5)
    W0, b0, W1, b1 = (torch.randn(*s, generator=gen) for s in ((hid, cin), (hid,), (2 * cm, hid), (2 * cm,)))
    img0, img1 = M.pack_image(W0.numpy(), b0.numpy(), True, 1, 1), M.pack_image(W1.numpy(), b1.numpy(), False, 1, 1)
    off1 = (img0.size + 3) // 4 * 4
    w = torch.zeros(1 << 18)                                             # room for the images of any width the checks let through
    w[:img0.size], w[off1:off1 + img1.size] = torch.from_numpy(img0), torch.from_numpy(img1)
    w = w.cuda()
    assert w.data_ptr() % 16 == 0
    zi, ti, si = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([3, 4], [0, 1], [2, 3]))
    z0, t0, l0 = torch.randn(B, D, generator=gen).cuda(), torch.randn(D * B * 16, generator=gen).cuda(), torch.randn(B, generator=gen).cuda()

    def call(tangent, **defect):
        z, t, lj = z0.clone(), t0.clone(), l0.clone()
        a = _lib.MlpCouplerArgs()
        a.z, a.z_b, a.w = E._p(z), D, E._p(w)
        a.zi, a.si, a.ti, a.n_mod = E._p(zi), E._p(si), E._p(ti), cm
        a.B, a.cin, a.chan_off, a.chan_step, a.n_layers = B, cin, 0, 1, 2
        a.width[0], a.width[1], a.width[2] = cin, hid, 2 * cm
        a.w_off[0], a.w_off[1] = 0, off1
        a.decode, a.ncols = 1, 3
        if tangent:
            a.t, a.t_f = E._p(t), B * 16
        else:
            a.lj = E._p(lj)
        for k, val in defect.items():
            if k == "width":
                for i, x in val.items():
                    a.width[i] = x
            elif k == "w_off1":
                a.w_off[1] = val
            elif k == "w_shift":
                a.w = C.c_void_p(w.data_ptr() + val)
            else:
                setattr(a, k, val)
        rc = lib.cmf_mlp_coupler(C.byref(a), E._stream())
        torch.cuda.synchronize()
        return rc, _same(z, z0) and _same(t, t0) and _same(lj, l0)

    for tangent in (False, True):
        rc, untouched = call(tangent)
        assert rc == 0 and not untouched, "the arguments the defects are applied to are valid and launch"
    bad = [(False, dict(n_layers=1)), (False, dict(width={0: cin + 1})), (False, dict(width={1: 129})), (False, dict(width={2: 65})),
           (False, dict(cin=129, width={0: 129})), (False, dict(w_off1=off1 + 2)), (False, dict(w_shift=4)), (True, dict(decode=0)),
           (True, dict(ncols=16)), (True, dict(ncols=0)), (False, dict(n_layers=9)), (False, dict(B=0))]
    for tangent, defect in bad:
        rc, untouched = call(tangent, **defect)
        assert rc == EINVAL, (defect, rc)
        assert untouched, f"{defect}: rejected, but something was written"
