"""The data-space operator kernel on the GPU (cmf_operator_apply_wrapped, csrc/operator_apply.hip) against float64
numpy on the same float32 inputs, its identity property -- with the triple (1, 0, 0) it is cmf_operator_apply bit for bit --, its
output contract, isolation, determinism and refusals.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds, per sample and element (tests/_wrapped_operator_emulation.py):
    |scale - s64| <= 2^-23 |s64|                                              one float32 rounding of a float64 evaluation
    |K - K64| <= C_WRAPPED (|a| |s| |J|)                                      from the emulation, K64 = a diag(s64) J
    |yhat - yhat64| <= 2^-24 |yhat64| + (D + 2 + WRAPPER_OPS) 2^-53 sum_i |a_mi| |u_i|
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN; x_hat is uniform in [-30, 30]."""
import math

import numpy as np
import pytest
import torch

import _wrapped_operator_emulation as WO
from test_gpu_projection import guarded, guards_intact, same_bits, stack

pytestmark = pytest.mark.gpu

LAYOUTS = ["panel", "fmajor"]


def run(a, J, xhat, triple, layout):
    """``engine.operator_apply_wrapped`` and ``engine.operator_image_wrapped`` on CPU inputs -> numpy (K (B, M, nc), yhat (B, M),
    scale (B, D), image (B, M))."""
    from cmf_amd import engine as E
    T = stack(J, layout)
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    K, yhat, scale = E.operator_apply_wrapped(T, ac, hc, triple)
    image = E.operator_image_wrapped(ac, hc, triple)
    torch.cuda.synchronize()
    assert isinstance(K, E.Tangent) and (K.B, K.N, K.nc, K.layout) == (T.B, a.shape[0], T.nc, layout)
    assert scale.shape == xhat.shape and scale.dtype == torch.float32
    return K.to_dense(K.nc).contiguous().cpu().numpy(), yhat.cpu().numpy(), scale.cpu().numpy(), image.cpu().numpy()


def run_plain(a, J, xhat, layout):
    from cmf_amd import engine as E
    K, yhat = E.operator_apply(stack(J, layout), torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda())
    return K.to_dense(K.nc).contiguous().cpu().numpy(), yhat.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(WO.TRIPLES))
@pytest.mark.parametrize("M,D,d", WO.SHAPES)
def test_kernel_matches_float64(M, D, d, name, layout):
    triple = WO.TRIPLES[name]
    a, J, xhat = WO.inputs(M, D, d)
    K, yhat, scale, image = run(a, J, xhat, triple, layout)
    u64, s64 = WO.wrapper64(xhat, triple)
    s_err = float((np.abs(scale.astype(np.float64) - s64) / WO.scale_bound(s64)).max())
    worst = 0.0
    for b in range(WO.BATCH):
        K64, S = WO.apply64(a, J[b], s64[b])
        worst = max(worst, WO.OA.ratio(K[b, :, :d], K64, S))
    y64, S = WO.image64(a, u64)
    y_err = float((np.abs(yhat.astype(np.float64) - y64) / WO.image_bound(y64, S, D)).max())
    print(f"M={M} D={D} d={d} {name} {layout}: worst |scale - s64| / bound = {s_err:.3f}; worst |K - K64| / (|a| |s| |J|) = "
          f"2^{math.log2(max(worst, 1e-300)):.2f} (bound 2^{math.log2(WO.C_WRAPPED):g}); worst |yhat - yhat64| / bound = {y_err:.3f}")
    assert s_err <= 1.0
    assert worst <= WO.C_WRAPPED
    assert np.isnan(K[:, :, d:]).all()                               # what the padding columns held stays in the padding columns
    assert y_err <= 1.0
    assert same_bits(image, yhat)                                    # the image-only mode: the same bits


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,D,d", WO.SHAPES)
def test_identity_triple_is_the_plain_kernel(M, D, d, layout):
    """(wa, wc, logit) = (1, 0, 0): s is 1.0f, u is x_hat, and K and yhat are cmf_operator_apply's bits."""
    a, J, xhat = WO.inputs(M, D, d, seed=4)
    K, yhat, scale, image = run(a, J, xhat, WO.IDENTITY, layout)
    K0, yhat0 = run_plain(a, J, xhat, layout)
    assert torch.equal(torch.as_tensor(scale), torch.ones(xhat.shape))
    assert torch.equal(torch.as_tensor(K[:, :, :d]), torch.as_tensor(K0[:, :, :d])) and np.isnan(K[:, :, d:]).all()
    assert torch.equal(torch.as_tensor(yhat), torch.as_tensor(yhat0)) and torch.equal(torch.as_tensor(image), torch.as_tensor(yhat0))


@pytest.mark.parametrize("B,M,D,d,layout", [(3, 17, 64, 17, "panel"), (2, 196, 784, 100, "fmajor"), (3, 1, 5, 3, "panel"),
                                            (2, 33, 1100, 33, "fmajor"), (2, 260, 64, 128, "panel")])
def test_outputs_stay_inside_their_buffers(B, M, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    triple = WO.TRIPLES["mini_mnist"]
    a, J, xhat = WO.inputs(M, D, d, B=B, seed=2)
    T = stack(J, layout)
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    bufs = {"k": guarded((B * M * T.nc,), torch.float32), "yhat": guarded((B, M), torch.float32),
            "scale": guarded((B, D), torch.float32), "image": guarded((B, M), torch.float32)}
    K = E.Tangent(B, M, T.nc, layout, "cuda", data=bufs["k"][1])
    p = lambda name: E._p(bufs[name][1])
    lib = _lib.load()
    w = (float(triple[0]), float(triple[1]), int(triple[2]))
    _lib.check(lib.cmf_operator_apply_wrapped(E._p(ac), M, D, E._p(T.data), T.t_b, T.t_r, T.nc, B, E._p(hc), *w, p("scale"), p("k"),
                                              K.t_b, K.t_r, p("yhat"), E._stream()), "cmf_operator_apply_wrapped")
    _lib.check(lib.cmf_operator_apply_wrapped(E._p(ac), M, D, None, 0, 0, 0, B, E._p(hc), *w, None, None, 0, 0, p("image"),
                                              E._stream()), "cmf_operator_apply_wrapped")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    want_k, want_y, want_s, want_i = run(a, J, xhat, triple, layout)
    assert same_bits(K.to_dense(K.nc).contiguous().cpu().numpy(), want_k)      # every element of k is written
    assert same_bits(bufs["yhat"][1].cpu().numpy(), want_y) and same_bits(bufs["image"][1].cpu().numpy(), want_i)
    assert same_bits(bufs["scale"][1].cpu().numpy(), want_s) and not np.isnan(want_s).any()
    # the engine writes into a buffer it is given, and returns it
    mine = torch.full((B, D), float("nan"), device="cuda")
    out = E.operator_apply_wrapped(T, ac, hc, triple, mine)
    assert out[2] is mine and same_bits(mine.cpu().numpy(), want_s)


@pytest.mark.parametrize("M,D,d,layout", [(17, 64, 17, "panel"), (196, 784, 100, "panel"), (17, 64, 17, "fmajor"),
                                          (300, 1100, 33, "fmajor")])
def test_position_independence_and_repeatability(M, D, d, layout):
    triple = WO.TRIPLES["mini_mnist"]
    a, J, xhat = WO.inputs(M, D, d, B=5, seed=3)
    batch, again = run(a, J, xhat, triple, layout), run(a, J, xhat, triple, layout)
    for x, y in zip(batch, again):
        assert same_bits(x, y)
    for b in range(5):
        alone = run(a, J[b:b + 1], xhat[b:b + 1], triple, layout)
        for x, y in zip(alone, batch):
            assert same_bits(x[0], y[b]), f"sample {b}"
    where = [4, 0, 2, 2, 1, 3, 0]
    for x, y in zip(run(a, J[where], xhat[where], triple, layout), batch):
        assert same_bits(x, y[where])


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, M, D, d = 2, 5, 8, 3
    a, J, xhat = WO.inputs(M, D, d, B=B)
    T = stack(J, "panel")
    ac, hc = torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    k, yhat = torch.zeros(B * M * T.nc + 4, device="cuda"), torch.zeros(B * M, device="cuda")
    scale = torch.zeros(B * D + 1, device="cuda")
    ok = [E._p(ac), M, D, E._p(T.data), T.t_b, T.t_r, T.nc, B, E._p(hc), 0.25, 0.5, 1, E._p(scale), E._p(k), M * T.nc, T.nc, E._p(yhat)]
    assert lib.cmf_operator_apply_wrapped(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(yhat.abs().sum()) > 0 and bool(torch.isnan(k).any()) and float(scale[:B * D].abs().min()) > 0 and float(scale[-1]) == 0
    k.zero_()
    yhat.zero_()
    scale.zero_()
    inf, nan = float("inf"), float("nan")
    bad = [(0, None), (1, 0), (2, 0), (4, T.t_b + 2), (5, T.t_r + 2), (5, 8), (4, 8), (6, 24), (6, 0), (7, 0), (8, None),
           (9, 0.0), (9, inf), (9, -inf), (9, nan), (10, inf), (10, nan), (11, 2), (11, -1), (12, None),
           (12, offset_pointer(scale, 1)), (13, None), (14, M * T.nc + 2), (15, T.nc + 2), (15, 8), (14, 8), (16, None),
           (3, E._p(T.data[1:])), (13, E._p(k[1:]))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_operator_apply_wrapped(*args, E._stream()) == -1, (i, value)
    # image-only mode: a, xhat, yhat and a sound triple are still required; scale, k and the stack are not looked at
    image = [E._p(ac), M, D, None, 0, 0, 0, B, E._p(hc), 0.25, 0.5, 1, None, None, 0, 0, E._p(yhat)]
    for i, value in ((0, None), (1, 0), (2, 0), (7, 0), (8, None), (9, 0.0), (9, nan), (10, inf), (11, 3), (16, None)):
        args = list(image)
        args[i] = value
        assert lib.cmf_operator_apply_wrapped(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert float(k.abs().sum()) == 0.0 and float(yhat.abs().sum()) == 0.0 and float(scale.abs().sum()) == 0.0
    assert lib.cmf_operator_apply_wrapped(*image, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(yhat.abs().sum()) > 0 and float(k.abs().sum()) == 0.0 and float(scale.abs().sum()) == 0.0


def offset_pointer(t, byte_offset):
    """A device pointer ``byte_offset`` bytes into ``t``: misaligned on purpose, for the refusals."""
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def test_engine_refusals():
    from cmf_amd import engine as E
    a, J, xhat = WO.inputs(5, 8, 3, B=2)
    T, ac, hc = stack(J, "panel"), torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    w = (0.25, 0.5, True)
    # the checks operator_apply / operator_image make, through the shared code
    with pytest.raises(ValueError, match="engine.Tangent"):
        E.operator_apply_wrapped(T.data, ac, hc, w)
    with pytest.raises(ValueError, match="float32"):
        E.operator_apply_wrapped(T, ac.double(), hc, w)
    with pytest.raises(ValueError, match="float32"):
        E.operator_image_wrapped(ac, hc.double(), w)
    with pytest.raises(ValueError, match="not contiguous"):
        E.operator_image_wrapped(ac, hc.t().contiguous().t(), w)
    with pytest.raises(ValueError, match="8 elements per sample"):
        E.operator_apply_wrapped(T, ac, hc[:, :7].contiguous(), w)
    with pytest.raises(ValueError, match="must hold"):
        E.operator_apply_wrapped(T, ac, hc[:1].contiguous(), w)
    with pytest.raises(ValueError, match="GPU"):
        E.operator_apply_wrapped(T, ac.cpu(), hc, w)
    with pytest.raises(ValueError, match="GPU"):
        E.operator_image_wrapped(ac, hc.cpu(), w)
    # the wrapper
    for bad in ((0.0, 0.5, True), (float("inf"), 0.5, False), (0.25, float("nan"), True), (0.25, 0.5, 2), (0.25, 0.5), "abc", None):
        with pytest.raises(ValueError, match="wrapper"):
            E.operator_apply_wrapped(T, ac, hc, bad)
        with pytest.raises(ValueError, match="wrapper"):
            E.operator_image_wrapped(ac, hc, bad)
    # the scale buffer
    for bad in (torch.zeros(2, 7, device="cuda"), torch.zeros(2, 8, device="cuda", dtype=torch.float64),
                torch.zeros(8, 2, device="cuda").t()):
        with pytest.raises(ValueError, match="scale"):
            E.operator_apply_wrapped(T, ac, hc, w, bad)
    with pytest.raises(ValueError, match="GPU"):
        E.operator_apply_wrapped(T, ac, hc, w, torch.zeros(2, 8))
    # B == 0: empties, no launch
    K, yhat, scale = E.operator_apply_wrapped(E.Tangent(0, 8, 16, "panel", "cuda"), ac, hc[:0], w)
    assert (K.B, K.N, K.nc, K.layout) == (0, 5, 16, "panel") and yhat.shape == (0, 5) and scale.shape == (0, 8)
    assert E.operator_image_wrapped(ac, hc[:0], w).shape == (0, 5)


def test_kernel_timer_entries():
    from cmf_amd import engine as E
    a, J, xhat = WO.inputs(5, 8, 3, B=2)
    T, ac, hc = stack(J, "panel"), torch.as_tensor(a).cuda(), torch.as_tensor(xhat).cuda()
    with E.timing(lambda name: True) as timer:
        E.operator_apply_wrapped(T, ac, hc, WO.TRIPLES["mini_mnist"])
        E.operator_image_wrapped(ac, hc, WO.TRIPLES["mini_mnist"])
        E.operator_apply(T, ac, hc)
    by = timer.by_name()
    assert set(by) == {"operator_apply_wrapped", "operator_image_wrapped", "operator_apply"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())
    assert by["operator_image_wrapped"][3] < by["operator_apply_wrapped"][3]
    # the scale array's write and its read by the one pass over J, and x_hat's second read
    assert by["operator_apply_wrapped"][3] - by["operator_apply"][3] == 4.0 * 2 * 8 * 3
