"""Parallel transport on the GPU: the per-curve kernel (csrc/transport_step.hip) against float64 numpy on the same
float32 inputs -- per segment, on the kernel's own w_i --, its known answers, its failure codes, isolation, determinism and
refusals; and ``cmf_amd.ManifoldGeodesic.transport_latents`` / ``transport`` / ``analogy`` end to end against the float64 reference
(tests/_transport_reference.py) and under the conditions tests/test_transport_host.py establishes.  Needs an MI355X: ``-m gpu``.

Kernel bounds, per segment and vector (u = 2^-53; the data: tests/_transport_emulation.py):
    forward:   ||G_{i+1} a - C_i^T w_i||_inf <= 32 d u (||G||_inf ||a||_inf + ||rhs||_inf)    the projector's bound, same elimination
    backward:  ||C_i b - G_i w_i||_inf       <= 64 d u (||C||_inf ||b||_inf + ||rhs||_inf)    the band solve's doubled constant
    out = (fwd + bwd) / 2 exactly;  norm2 to 2 (d + 2) u sum |terms|.
Every strict upper triangle of jtj and every cross block that straddles two curves is NaN.
Known answers: (i) a shared plane, reparametrised by unimodular integer matrices: both halves are R_i^-1 w_i to
2 * 64 d u cond_inf(M) ||x||_inf (the residual bound through the condition number of the half's matrix); (ii) prescribed principal
angles: norm2_{i+1} / norm2_i = ((cos + sec) / 2)^2 to 16 kappa sqrt(d) 2^-24 -- G and C reach the kernel rounded to float32, an
entrywise relative 2^-24, i.e. at most sqrt(d) 2^-24 of their norms, which each of the two solves and their right-hand sides carry
into w (4 kappa sqrt(d) 2^-24), twice that into the quadratic form, plus the forms' own matrices: (8 kappa + 2) sqrt(d) 2^-24,
rounded up; (iii) a cross block whose leading entry is an exact zero.

Product: ``vectors``, ``norm2`` and the end vector relative (max-norm) to the float64 reference on the same float32 latents within
the larger of 1e-4 -- the bound tests/test_gpu_parity.py holds dz_low to -- and 3 x the float32 oracle's own deviation."""
import ctypes as C

import numpy as np
import pytest
import torch

import _transport_emulation as M
import _transport_reference as T
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits
from test_gpu_shoot import product_ends

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
NAMES = ("out", "fwd", "bwd", "norm2", "info")


def run(jtj, cross, w0, P):
    """``engine.transport_chain`` on numpy inputs -> numpy (out, fwd, bwd, norm2, info)."""
    from cmf_amd import engine as E
    r = E.transport_chain(torch.as_tensor(jtj).cuda(), torch.as_tensor(cross).cuda(), torch.as_tensor(w0).cuda(), P)
    torch.cuda.synchronize()
    return tuple(getattr(r, k).cpu().numpy() for k in NAMES)


@pytest.mark.parametrize("d", M.WIDTHS)
def test_kernel_matches_float64(d):
    for P in M.POINTS:
        for curves in M.CURVES:
            for m in M.VECTORS:
                jtj, cross, w0 = M.case(curves, P, d, m)
                out, fwd, bwd, norm2, info = run(jtj, cross, w0, P)
                label = f"d={d} P={P} curves={curves} m={m}"
                assert out.shape == (curves, P, m, d) and fwd.shape == bwd.shape == (curves, P - 1, m, d), label
                assert norm2.shape == (curves, P, m) and info.shape == (curves,) and info.dtype == np.int32, label
                assert out.dtype == fwd.dtype == bwd.dtype == norm2.dtype == np.float64, label
                assert (info == 0).all(), label
                assert same_bits(out[:, 0], w0) and same_bits(out[:, 1:], 0.5 * (fwd + bwd)), label
                rf, rb, rn = M.residual_ratios(jtj, cross, out, fwd, bwd, norm2, P)
                print(f"{label}: forward {rf:.3f} (bound 32), backward {rb:.3f} (bound 64), norm2 {rn:.3f} u (bound {2 * (d + 2)})")
                assert rf <= M.FWD_CONSTANT and rb <= M.BWD_CONSTANT and rn <= 2 * (d + 2), label
                assert (norm2 > 0).all(), label


@pytest.mark.parametrize("d", [3, 16])
def test_a_shared_plane_only_changes_coordinates(d):
    P = 5
    J, inverse, conds = M.same_plane(d, P)
    jtj, cross = M.blocks(J)
    assert np.array_equal(np.tril(jtj.astype(np.float64)), np.tril(np.einsum("pra,prb->pab", J[0], J[0])))      # exact in float32
    w0 = np.random.default_rng(d).integers(-3, 4, (1, 3, d)).astype(np.float64)
    out, fwd, bwd, norm2, info = run(jtj, cross, w0, P)
    assert info[0] == 0
    for i in range(P - 1):
        want = out[0, i] @ inverse[i].T                              # R_i^-1 w_i, on the kernel's own w_i
        for half, cond in ((fwd, conds[i, 0]), (bwd, conds[i, 1])):
            tol = 2 * M.BWD_CONSTANT * d * U * cond * np.abs(want).max()
            print(f"d={d} segment {i}: error {np.abs(half[0, i] - want).max():.2e} (tolerance {tol:.2e})")
            assert np.abs(half[0, i] - want).max() <= tol
        # the ambient vector J_i w_i stays
        tol = np.abs(J[0, i + 1]).sum(1).max() * 2 * M.BWD_CONSTANT * d * U * conds[i].max() * np.abs(want).max()
        assert np.abs(out[0, i + 1] @ J[0, i + 1].T - out[0, i] @ J[0, i].T).max() <= tol + 4 * d * U * np.abs(out[0, i] @ J[0, i].T).max()


@pytest.mark.parametrize("d,P", [(2, 3), (6, 4), (33, 3)])
def test_prescribed_principal_angles(d, P):
    J, w0, ratio, kappa = M.turned_planes(d, P)
    w0, ratio = np.ascontiguousarray(w0[:, :16]), ratio[:16]         # one group of vectors
    jtj, cross = M.blocks(J)
    out, fwd, bwd, norm2, info = run(jtj, cross, w0, P)
    assert info[0] == 0
    got = norm2[0, 1:] / norm2[0, :-1]
    tol = 16 * kappa * np.sqrt(d) * 2.0 ** -24
    print(f"d={d}: ratios off by {np.abs(got / ratio[None] - 1.0).max():.2e} (tolerance {tol:.2e})")
    assert np.abs(got / ratio[None] - 1.0).max() <= tol


def test_a_zero_leading_entry_needs_the_pivot_search():
    J, Pi = M.pivoting_case()
    jtj, cross = M.blocks(J)
    assert cross[0, 0, 0] == 0.0                                     # an elimination without pivoting divides by this
    w0 = np.arange(15.0).reshape(1, 3, 5) - 7.0
    out, fwd, bwd, norm2, info = run(jtj, cross, w0, 2)
    assert info[0] == 0
    want = w0[0] @ Pi[0]                                             # Pi^-1 = Pi
    cond = np.linalg.cond(cross[0].astype(np.float64), np.inf)
    assert np.abs(bwd[0, 0] - want).max() <= 2 * M.BWD_CONSTANT * 5 * U * cond * np.abs(want).max()
    assert np.abs(out[0, 1] - want).max() <= 2 * M.BWD_CONSTANT * 5 * U * cond * np.abs(want).max()
    emu = M.chain(jtj, cross, w0, 2)
    assert np.allclose(out, emu[0], rtol=1e-12, atol=0) and np.allclose(norm2, emu[3], rtol=1e-12, atol=0)


def failure_inputs():
    """Five curves of five points, d = 4, m = 2: curve 1 has a zero Jacobian column at point 2, curve 2 a NaN vector, curve 3 a NaN
    in a cross block that is read and the zero column as well, curve 4 an infinity in a lower triangle."""
    Jf = M.jacobians(5, 5, 4, seed=3)
    clean = M.blocks(Jf) + (M.vectors(5, 2, 4, seed=3),)
    Jf[1, 2, :, 1] = 0.0
    Jf[3, 2, :, 1] = 0.0
    jtj, cross = M.blocks(Jf)
    w0 = clean[2].copy()
    w0[2, 1, 3] = NAN
    cross[3 * 5 + 3, 0, 2] = NAN
    jtj[4 * 5 + 4, 3, 0] = np.inf
    return clean, (jtj, cross, w0)


def test_failures_are_reported_and_confined():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    (jtj0, cross0, w00), (jtj, cross, w0) = failure_inputs()
    clean = run(jtj0, cross0, w00, 5)
    assert (clean[4] == 0).all()
    curves, P, m, d = 5, 5, 2, 4
    bufs = {"out": guarded((curves, P, m, d), torch.float64), "fwd": guarded((curves, P - 1, m, d), torch.float64),
            "bwd": guarded((curves, P - 1, m, d), torch.float64), "norm2": guarded((curves, P, m), torch.float64),
            "info": guarded((curves,), torch.int32)}
    for _, view, _ in bufs.values():
        view.fill_(7)                                                # every element must be written, the NaN ones too
    p = lambda name: E._p(bufs[name][1])
    dev = [torch.as_tensor(a).cuda() for a in (jtj, cross, w0)]
    _lib.check(_lib.load().cmf_transport_chain(E._p(dev[0]), E._p(dev[1]), E._p(dev[2]), d, m, P, curves, p("out"), p("fwd"), p("bwd"),
                                               p("norm2"), p("info"), E._stream()), "cmf_transport_chain")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    out, fwd, bwd, norm2, info = (bufs[k][1].cpu().numpy() for k in NAMES)
    assert info.tolist() == [0, 1, 2, 2, 2]
    for got, want in zip((out, fwd, bwd, norm2), clean):             # the healthy curve keeps its bits
        assert same_bits(got[0], want[0])
    # code 1 from segment 1 on (G_2 and C_1 are singular): points 0 and 1 and segment 0 keep their bits
    assert same_bits(out[1, :2], clean[0][1, :2]) and same_bits(norm2[1, :2], clean[3][1, :2])
    assert same_bits(fwd[1, 0], clean[1][1, 0]) and same_bits(bwd[1, 0], clean[2][1, 0])
    assert np.isnan(out[1, 2:]).all() and np.isnan(norm2[1, 2:]).all() and np.isnan(fwd[1, 1:]).all() and np.isnan(bwd[1, 1:]).all()
    for c in (2, 3, 4):                                              # code 2, also where code 1 would apply
        assert all(np.isnan(a[c]).all() for a in (out, fwd, bwd, norm2))
    again = run(jtj, cross, w0, 5)
    for got, want in zip((out, fwd, bwd, norm2, info), again):
        assert same_bits(got, want)


@pytest.mark.parametrize("d,m", [(3, 1), (17, 3), (100, 16)])
def test_position_independence_and_repeatability(d, m):
    P = 3
    jtj, cross, w0 = M.case(3, P, d, m, seed=5)
    base = run(jtj, cross, w0, P)
    where = [2, 0, 1, 1, 2, 0, 0]
    J = M.jacobians(3, P, d, seed=5)[where]
    jtj2, cross2 = M.blocks(J)                                       # the same curves, elsewhere in a larger batch
    for c, src in enumerate(where):
        assert same_bits(jtj2[c * P:(c + 1) * P], jtj[src * P:(src + 1) * P])
        assert same_bits(cross2[c * P:c * P + P - 1], cross[src * P:src * P + P - 1])
    batch = run(jtj2, cross2, w0[where], P)
    again = run(jtj2, cross2, w0[where], P)
    for a, b, c in zip(base, batch, again):
        assert same_bits(a[where], b) and same_bits(b, c)
    sym = np.stack([M.symmetric(g) for g in jtj]).astype(np.float32)  # the strict upper triangle is never read
    full = np.where(np.isnan(cross), np.float32(1.0), cross)          # nor are the straddling blocks
    for a, b in zip(base, run(sym, full, w0, P)):
        assert same_bits(a, b)
    alone = run(jtj[:P], cross[:P - 1], w0[:1, :1].copy(), P)         # one curve, one vector: the same bits as in the group
    assert same_bits(alone[0][0, :, 0], base[0][0, :, 0]) and same_bits(alone[3][0, :, 0], base[3][0, :, 0])


@pytest.mark.parametrize("curves,P,d,m", [(3, 2, 1, 1), (2, 3, 17, 3), (2, 2, 128, 16), (3, 5, 64, 16)])
def test_outputs_stay_inside_their_buffers(curves, P, d, m):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    jtj, cross, w0 = M.case(curves, P, d, m, seed=4)
    dev = [torch.as_tensor(a).cuda() for a in (jtj, cross, w0)]
    bufs = {"out": guarded((curves, P, m, d), torch.float64), "fwd": guarded((curves, P - 1, m, d), torch.float64),
            "bwd": guarded((curves, P - 1, m, d), torch.float64), "norm2": guarded((curves, P, m), torch.float64),
            "info": guarded((curves,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    _lib.check(_lib.load().cmf_transport_chain(E._p(dev[0]), E._p(dev[1]), E._p(dev[2]), d, m, P, curves, p("out"), p("fwd"), p("bwd"),
                                               p("norm2"), p("info"), E._stream()), "cmf_transport_chain")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    for name, want in zip(NAMES, run(jtj, cross, w0, P)):
        assert same_bits(bufs[name][1].cpu().numpy(), want)


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    curves, P, d, m = 2, 3, 3, 2
    jtj, cross, w0 = M.case(curves, P, d, m)
    dev = [torch.as_tensor(a).cuda() for a in (jtj, cross, w0)]
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
    out, fwd, bwd, norm2 = f64(curves, P, m, d), f64(curves, P - 1, m, d), f64(curves, P - 1, m, d), f64(curves, P, m)
    info = torch.empty(curves, dtype=torch.int32, device="cuda")
    ok = [E._p(dev[0]), E._p(dev[1]), E._p(dev[2]), d, m, P, curves, E._p(out), E._p(fwd), E._p(bwd), E._p(norm2), E._p(info)]
    assert lib.cmf_transport_chain(*ok, E._stream()) == 0
    for i, value in ((0, None), (1, None), (2, None), (3, 0), (3, 129), (3, -1), (4, 0), (4, 17), (5, 1), (5, 0), (6, 0), (6, -1),
                     (7, None), (8, None), (9, None), (10, None), (11, None)):
        args = list(ok)
        args[i] = value
        assert lib.cmf_transport_chain(*args, E._stream()) == -1, (i, value)
    for i in (2, 7, 8, 9, 10):                                       # float64 pointers: 8-byte aligned
        args = list(ok)
        args[i] = C.c_void_p(args[i].value + 4)
        assert lib.cmf_transport_chain(*args, E._stream()) == -1, i
    for i in (0, 1, 11):                                             # the others: 4-byte
        args = list(ok)
        args[i] = C.c_void_p(args[i].value + 2)
        assert lib.cmf_transport_chain(*args, E._stream()) == -1, i
    torch.cuda.synchronize()


def test_engine_refusals_and_timer_entry():
    from cmf_amd import engine as E
    assert E.TRANSPORT_MAX_WIDTH == 128 and E.TRANSPORT_MAX_VECTORS == 16
    jtj, cross, w0 = M.case(2, 3, 3, 2)
    G, Cr, w = (torch.as_tensor(np.nan_to_num(a)).cuda() for a in (jtj, cross, w0))
    for args in ((G.cpu(), Cr, w), (G, Cr.cpu(), w), (G, Cr, w.cpu())):
        with pytest.raises(ValueError, match="GPU"):
            E.transport_chain(*args, 3)
    with pytest.raises(ValueError, match="jtj must be float32"):
        E.transport_chain(G.double(), Cr, w, 3)
    with pytest.raises(ValueError, match="cross must be float32"):
        E.transport_chain(G, Cr.double(), w, 3)
    with pytest.raises(ValueError, match="w0 must be float64"):
        E.transport_chain(G, Cr, w.float(), 3)
    with pytest.raises(ValueError, match="contiguous"):
        E.transport_chain(G.transpose(1, 2), Cr, w, 3)
    with pytest.raises(ValueError, match="contiguous"):
        E.transport_chain(G, Cr.transpose(1, 2), w, 3)
    with pytest.raises(ValueError, match="contiguous"):
        E.transport_chain(G, Cr, w.transpose(1, 2).contiguous().transpose(1, 2), 3)
    with pytest.raises(ValueError, match="cross must be"):
        E.transport_chain(G, Cr[:4].contiguous(), w, 3)              # a block short
    with pytest.raises(ValueError, match="w0 must be"):
        E.transport_chain(G, Cr, w[:1].contiguous(), 3)
    with pytest.raises(ValueError, match="w0 must be"):
        E.transport_chain(G, Cr, w[:, :, :2].contiguous(), 3)
    with pytest.raises(ValueError, match="whole curves"):
        E.transport_chain(G, Cr, w, 4)
    with pytest.raises(ValueError, match="points >= 2"):
        E.transport_chain(G, Cr, torch.zeros(6, 2, 3, dtype=torch.float64, device="cuda"), 1)
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        E.transport_chain(G, Cr, torch.zeros(2, 17, 3, dtype=torch.float64, device="cuda"), 3)
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        E.transport_chain(G, Cr, torch.zeros(2, 0, 3, dtype=torch.float64, device="cuda"), 3)
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.transport_chain(torch.zeros(2, 129, 129, device="cuda"), torch.zeros(1, 129, 129, device="cuda"),
                          torch.zeros(1, 1, 129, dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.transport_chain(torch.zeros(2, 0, 0, device="cuda"), torch.zeros(1, 0, 0, device="cuda"),
                          torch.zeros(1, 1, 0, dtype=torch.float64, device="cuda"), 2)
    r = E.transport_chain(G[:0], Cr[:0], w[:0], 3)                   # no curve: empties, no launch
    assert r.out.shape == (0, 3, 2, 3) and r.fwd.shape == r.bwd.shape == (0, 2, 2, 3) and r.norm2.shape == (0, 3, 2)
    assert r.info.shape == (0,) and r.info.dtype == torch.int32 and r.out.dtype == r.norm2.dtype == torch.float64
    with E.timing(lambda name: True) as timer:
        E.transport_chain(G, Cr, w, 3)
    by = timer.by_name()
    assert set(by) == {"transport_chain"}
    n, ms, flops, nbytes = by["transport_chain"]
    assert n == 1 and ms >= 0 and flops > 0 and nbytes > 0


# --------------------------------------------------------------------------------------------------
# the product
# --------------------------------------------------------------------------------------------------


def geodesic(dens, **kw):
    import cmf_amd
    return cmf_amd.ManifoldGeodesic(dens, **kw)


def check_against_reference(name, geo, head, model, model32, latents32, w0):
    """``transport_latents`` on the float32 latents against the float64 reference on the same latents (``model32`` None: no
    float32 yardstick, the bound is 1e-4)."""
    want = T.transport(model, latents32.double(), w0)
    yard = None if model32 is None else T.transport(model32, latents32, w0.float())
    marker = object()
    head.last_gram = marker
    got = geo.transport_latents(latents32.cuda(), w0.cuda())
    assert head.last_gram is marker
    B, P, d = latents32.shape
    m = w0.shape[2]
    assert got["vectors"].shape == (B, P, d, m) and got["forward"].shape == got["backward"].shape == (B, P - 1, d, m)
    assert got["norm2"].shape == (B, P, m) and got["info"].shape == (B,) and got["info"].dtype == torch.int32
    assert all(got[k].dtype == torch.float64 and got[k].is_cuda for k in ("vectors", "forward", "backward", "norm2"))
    assert bool((got["info"] == 0).all())
    assert torch.equal(got["vectors"][:, 0], w0.cuda()) and torch.equal(got["vectors"][:, 1:], 0.5 * (got["forward"] + got["backward"]))
    for key, pick in (("vectors", lambda o: o["vectors"]), ("norm2", lambda o: o["norm2"]), ("end vector", lambda o: o["vectors"][:, -1])):
        g, r = pick(got).cpu(), pick(want)
        own = 0.0 if yard is None else T.rel(pick(yard).double(), r)
        bound = max(1e-4, 3.0 * own)
        print(f"{name}: {key}: rel {T.rel(g, r):.2e} (float32 oracle {own:.2e}, bound {bound:.2e})")
        assert T.rel(g, r) <= bound, key
    return got


@pytest.mark.parametrize("name", T.FIXTURES)
def test_transport_matches_the_float64_reference(name):
    g, meta, dens, head, x = build(name)
    model, z = T.relaxed(name, 9)
    latents32 = z.float()
    w0 = T.start_vectors(z)
    check_against_reference(name, geodesic(dens), head, model, T.SR.model_of(name, torch.float32), latents32, w0)


def test_the_full_size_model_transports_along_one_short_curve():
    """c3_mnist_full, one curve of three points: the only fixture that reaches the bf16x3 kernels and the 28 x 28 plans.  Held to
    1e-4 alone: the float32 oracle's pass over the full-size model would cost as much again as the float64 one."""
    name = "c3_mnist_full"
    g, meta, dens, head, x = build(name)
    model, model32 = T.SR.model_of(name), None
    with torch.no_grad():
        z = model.encode(model.y[:2]).float()
    latents32 = torch.stack([z[0], 0.5 * (z[0] + z[1]), z[1]])[None].contiguous()
    w0 = torch.randn(1, z.shape[1], 2, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    check_against_reference(name, geodesic(dens), head, model, model32, latents32, w0)


def metric_norm2(geo, z_end, vectors):
    """w^T G(z) w at the latents ``z_end`` (B, d) for ``vectors`` (B, d, m), by the product itself: norm2 at point 0 of the
    zero-length curve."""
    twice = z_end[:, None, :].expand(-1, 2, -1).contiguous()
    return geo.transport_latents(twice, vectors)["norm2"][:, 0]


@pytest.mark.parametrize("name", T.FIXTURES)
def test_transport_keeps_norms_returns_and_carries_the_velocity(name):
    """Conditions (b), (c) and (d) of tests/test_transport_host.py on the product's own ``connect`` curves."""
    g, meta, dens, head, x = build(name)
    x0, x1 = product_ends(name, x)
    geo = geodesic(dens, points=9, steps=10)
    lg = geo.log(x0, x1)
    w = T.start_vectors(lg["latents"].cpu()).cuda()
    tr = geo.transport(x0, x1, w)
    assert bool((tr["transport_info"] == 0).all()) and tr["transported"].shape == w.shape
    drift9 = T.drift(tr)
    back = geo.transport_latents(tr["latents"].flip(1).contiguous(), tr["transported"])
    fb = T.rel(back["vectors"][:, -1], w)
    print(f"{name}: drift at P = 9 {drift9:.2e} (bound 2e-3), forth and back {fb:.2e} (bound 3e-3)")
    assert drift9 <= 2e-3 and fb <= 3e-3
    geo17 = geodesic(dens, points=17, steps=10)
    lg17 = geo17.log(x0, x1)
    tr17 = geo17.transport(x0, x1, T.start_vectors(lg17["latents"].cpu()).cuda())
    got, want = tr17["transported"][:, :, 0], T.end_velocity(tr17["latents"])
    n2 = metric_norm2(geo17, tr17["latents"][:, -1], torch.stack([got - want, want], 2))
    err = float((n2[:, 0] / n2[:, 1]).sqrt().max())
    drift17 = T.drift(tr17)
    print(f"{name}: transported log velocity against the end difference at P = 17 {err:.2e} (bound 1e-2); drift at P = 17 "
          f"{drift17:.2e}")
    assert err <= 1e-2
    if name in T.MLP:
        assert drift17 <= drift9 / 4.0


def test_transport_is_connect_plus_the_new_keys():
    g, meta, dens, head, x = build("c2a_power")
    x0, x1 = product_ends("c2a_power", x)
    geo = geodesic(dens, points=6, steps=3)
    con = geo.connect(x0, x1)
    w = torch.randn(x0.shape[0], head.program.d, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).float().cuda()
    tr = geo.transport(x0, x1, w)
    new = {"vectors", "forward", "backward", "norm2", "transport_info", "transported"}
    assert set(tr) == set(con) | new and not (set(con) & new)
    assert all(torch.equal(tr[k], con[k]) for k in con)
    assert tr["vectors"].shape == (x0.shape[0], 6, head.program.d, 1)                # a (B, d) w is one vector
    assert torch.equal(tr["transported"], tr["vectors"][:, -1])
    same = geo.transport_latents(con["latents"], w[:, :, None].double())             # (B, d, 1), and any floating dtype
    assert torch.equal(same["vectors"], tr["vectors"]) and torch.equal(same["info"], tr["transport_info"])


def curves_and_vectors(name, n, m, P=5):
    g, meta, dens, head, x = build(name)
    model, z0, z1 = T.SR.ends(name)
    tt = torch.linspace(0, 1, P, dtype=torch.float64)[None, :, None]
    z = (z0[:n, None, :] + tt * (z1 - z0)[:n, None, :]).float().cuda().contiguous()
    w = torch.randn(n, z.shape[2], m, dtype=torch.float64, generator=torch.Generator().manual_seed(13)).cuda()
    return dens, head, z, w


def test_sub_batches_give_the_vectors_of_one_call(monkeypatch):
    from cmf_amd import engine as E
    dens, head, z, w = curves_and_vectors("c2a_power", 3, 2)
    geo = geodesic(dens)
    whole = geo.transport_latents(z, w)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 9 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert (prog.tangent_chunk(3 * 5 + 2) - 2) // 5 == 1            # three sub-batches of one curve and its two padding samples
    pieces = geo.transport_latents(z, w)
    assert set(pieces) == set(whole)
    for key in whole:
        assert pieces[key].shape == whole[key].shape and torch.equal(pieces[key], whole[key]), key
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 6 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    with pytest.raises(ValueError, match="points"):
        geo.transport_latents(z, w)


def test_seventeen_vectors_are_sixteen_and_one():
    dens, head, z, w = curves_and_vectors("c2b_hepmass", 2, 17)
    geo = geodesic(dens)
    all17 = geo.transport_latents(z, w)
    first, last = geo.transport_latents(z, w[:, :, :16].contiguous()), geo.transport_latents(z, w[:, :, 16])
    for key in ("vectors", "forward", "backward"):
        assert torch.equal(all17[key], torch.cat([first[key], last[key]], 3)), key
    assert torch.equal(all17["norm2"], torch.cat([first["norm2"], last["norm2"]], 2))
    assert torch.equal(all17["info"], first["info"]) and bool((all17["info"] == 0).all())


def test_an_analogy_along_no_distance_is_a_shot():
    g, meta, dens, head, x = build("c2a_power")
    xa, xb = product_ends("c2a_power", x)
    xa, xb = xa[:3].contiguous(), xb[:3].contiguous()
    geo = geodesic(dens, points=9, steps=10, shoot_steps=8)
    lg = geo.log(xa, xb)
    shot = geo.shoot(xa, lg["velocity"])
    out = geo.analogy(xa, xb, xa)
    assert set(out) == set(shot) | {"velocity", "transported", "transport_info"}
    assert torch.equal(out["velocity"], lg["velocity"]) and bool((out["transport_info"] == 0).all()) and bool((out["info"] == 0).all())
    miss = (out["path_head"][:, -1] - shot["path_head"][:, -1]).flatten(1).double().norm(dim=1) / lg["length"]
    print(f"analogy(xa, xb, xa) against shoot: {float(miss.max()):.2e} of the relaxed length (bound 1e-5); transported against the "
          f"velocity {T.rel(out['transported'], lg['velocity']):.2e}")
    assert bool((miss <= 1e-5).all())


def test_a_non_finite_curve_fails_alone():
    dens, head, z, w = curves_and_vectors("c2a_power", 3, 2)
    geo = geodesic(dens)
    bad = w.clone()
    bad[1, 0, 1] = NAN
    out = geo.transport_latents(z, bad)
    assert out["info"].tolist() == [0, 2, 0]
    assert all(bool(torch.isnan(out[k][1]).all()) for k in ("vectors", "forward", "backward", "norm2"))
    alone = geo.transport_latents(z[[0, 2]].contiguous(), w[[0, 2]].contiguous())
    for key in out:
        assert torch.equal(out[key][[0, 2]], alone[key]), key
    wide = torch.cat([w, w, w, w, w, w, w, w, w], 2)                 # 18 vectors: two groups; a NaN in the second marks the curve
    wide[2, 1, 17] = NAN
    out = geo.transport_latents(z, wide)
    assert out["info"].tolist() == [0, 0, 2] and bool(torch.isnan(out["vectors"][2]).all()) and bool(torch.isnan(out["norm2"][2]).all())
    assert torch.equal(out["vectors"][:2, :, :, :2], geo.transport_latents(z[:2].contiguous(), w[:2].contiguous())["vectors"])


def test_validation():
    dens, head, z, w = curves_and_vectors("c2a_power", 3, 2)
    geo = geodesic(dens)
    with pytest.raises(ValueError, match="latents"):
        geo.transport_latents(z[:, :1].contiguous(), w)
    with pytest.raises(RuntimeError, match="float32"):
        geo.transport_latents(z.double(), w)
    with pytest.raises(ValueError, match="latents"):
        geo.transport_latents(z[:, :, :1].contiguous(), w[:, :1].contiguous())
    with pytest.raises(ValueError, match="w "):
        geo.transport_latents(z, w[:2])
    with pytest.raises(ValueError, match="w "):
        geo.transport_latents(z, w.cpu())
    with pytest.raises(ValueError, match="w "):
        geo.transport_latents(z, w[:, :, :0])
    with pytest.raises(ValueError, match="w "):
        geo.transport_latents(z, w.long())
    with pytest.raises(ValueError, match="at least one"):
        geo.transport_latents(z[:0], w[:0])
    with pytest.raises(RuntimeError, match="CPU fallback"):
        geo.transport_latents(z.cpu(), w)
    two = geo.transport_latents(z[:, :2].contiguous(), w)           # two points: one segment
    assert two["vectors"].shape == (3, 2, z.shape[2], 2) and two["forward"].shape == (3, 1, z.shape[2], 2)
