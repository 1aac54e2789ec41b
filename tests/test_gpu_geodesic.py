"""The manifold geodesics on the GPU: the cross-Gram and curve step kernels (csrc/curve_step.hip) against float64 numpy
on the same float32 inputs, their output contract, isolation, determinism and refusals, and ``cmf_amd.ManifoldGeodesic`` end to end on
the reference-generated fixtures under the conditions tests/test_geodesic_host.py establishes on the float64 reference loop.  Needs
an MI355X: run with ``-m gpu``.

Kernel bounds (u = 2^-53), per element / per curve of M interior points:
    |cross - ref| <= 2 (D + 2) 2^-24 sum_r |J_a| |J_b|                       fp32 MFMA accumulation over D products
    |g - g_ref| <= 2 (D + 4) u sum_r |J| |s|                                  two float64 sums of D products, in different orders
    ||A delta - g||_inf <= 64 d u (||A||_inf ||delta||_inf + ||g||_inf)       with the kernel's own g on the dense (M d)^2 matrix: the
                                                                              projector's 32 d u with the band's doubled depth
    seg2: 2 (D + 2) u relative;  g^T delta, delta^T H delta: 2 (M d + 2) u sum |terms|, against recomputation from the outputs.
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN."""
import numpy as np
import pytest
import torch

import _curve_step_emulation as CE
import _geodesic_reference as R
from test_geodesic_host import check_curve, damping_family, known_answer
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits, stack

pytestmark = pytest.mark.gpu

NAN = float("nan")


def run(J, G, C, xhat, lam, P, layout="panel"):
    """``engine.cross_gram`` is NOT used here: ``engine.curve_step`` and ``engine.curve_energy`` on CPU inputs -> numpy
    (grad, delta, stats, seg2, info, e_seg2, e_sum, e_info)."""
    from cmf_amd import engine as E
    hc = torch.as_tensor(xhat).cuda()
    r = E.curve_step(stack(J, layout), torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), hc, P,
                     torch.as_tensor(lam, dtype=torch.float64).cuda())
    e_seg2, e_sum, e_info = E.curve_energy(hc, P)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r.grad, r.delta, r.stats, r.seg2, r.info, e_seg2, e_sum, e_info))


def run_cross(J, P, d, layout):
    from cmf_amd import engine as E
    out = E.cross_gram(stack(J, layout), d, P)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("d", CE.WIDTHS)
@pytest.mark.parametrize("D", CE.ROWS)
def test_cross_gram_matches_float64(D, d, layout):
    for P, curves in ((3, 1), (4, 3), (9, 3), (9, 1)):
        J, _, _, _ = CE.inputs(curves, P, D, d, seed=4)
        if d > 1 and P > 3:                                          # two bit-identical columns, in different tiles where d > 16
            J[1, :, d - 1] = J[1, :, 0]
            J[2, :, d - 1] = J[2, :, 0]
        got = run_cross(J, P, d, layout)
        assert got.shape == (curves, P - 3, d, d) and got.dtype == np.float32
        if P == 3:
            continue
        ref = CE.cross_of(J, P)
        mag = CE.cross_of(np.abs(J), P)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"D={D} d={d} P={P} curves={curves} {layout}: max err / bound = {float((err / np.maximum(mag, 1e-300)).max() / (2 * (D + 2) * 2.0 ** -24)):.3f}")
        assert (err <= 2 * (D + 2) * 2.0 ** -24 * mag).all()
        if d > 1:
            assert same_bits(got[0, 0, d - 1, :], got[0, 0, 0, :])      # rows, from the columns of the first operand
            assert same_bits(got[0, 0, :, d - 1], got[0, 0, :, 0])      # columns, from the columns of the second operand


def test_cross_gram_is_position_independent_and_confined():
    P, D, d = 5, 64, 17
    J, _, _, _ = CE.inputs(3, P, D, d, seed=5)
    base = run_cross(J, P, d, "panel")
    order = [2, 0, 1, 1, 2, 0, 0]
    rows = np.concatenate([np.arange(c * P, (c + 1) * P) for c in order])
    again = run_cross(J[rows], P, d, "panel")
    assert same_bits(again, base[order]) and same_bits(run_cross(J[rows], P, d, "panel"), again)
    assert same_bits(run_cross(J[rows], P, d, "fmajor"), again)
    # a non-finite input reaches the blocks of its own pairs only; the end points are not read
    Jn = J.copy()
    Jn[P + 2, 7, 3] = NAN                                            # curve 1, point 2: pairs (1, 2) and (2, 3)
    Jn[0] = NAN
    Jn[P - 1] = NAN
    got = run_cross(Jn, P, d, "panel")
    assert same_bits(got[[0, 2]], base[[0, 2]])
    assert np.isnan(got[1, 0, :, 3]).all() and np.isnan(got[1, 1, 3, :]).all()
    keep = np.ones((d, d), dtype=bool)
    keep[:, 3] = False
    assert same_bits(got[1, 0][keep], base[1, 0][keep]) and same_bits(got[1, 1][keep.T], base[1, 1][keep.T])


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("d", CE.WIDTHS)
@pytest.mark.parametrize("D", CE.ROWS)
def test_curve_step_matches_float64(D, d, layout):
    lams = damping_family(D, d)
    worst = 0.0
    for P in CE.POINTS:
        J, G, C, xhat = CE.inputs(len(lams), P, D, d)
        lam = np.array(lams)
        grad, delta, stats, seg2, info, e_seg2, e_sum, e_info = run(J, G, C, xhat, lam, P, layout)
        assert (info == 0).all() and (e_info == 0).all()
        for c in range(len(lams)):
            sl = slice(c * P, (c + 1) * P)
            worst = max(worst, check_curve(J[sl], G[sl], C[c], xhat[sl], lam[c], grad[c], delta[c], stats[c], seg2[c], CE.BOUND_C,
                                           f"P {P} curve {c}"))
        assert same_bits(e_seg2, seg2) and same_bits(e_sum, stats[:, 0])      # the energy-only mode: the same bits
        if P == 9:
            ref = np.linalg.solve(CE.dense(G[:P], C[0], lam[0])[0], grad[0].reshape(-1))
            print(f"D={D} d={d} {layout}: max |delta - solve| / max |solve| = "
                  f"{float(np.abs(delta[0].reshape(-1) - ref).max() / np.abs(ref).max()):.2e}")
    print(f"D={D} d={d} {layout}: worst residual / (d 2^-53 scale) = {worst:.3f} (bound {CE.BOUND_C:g})")


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("P,D,d", [(3, 5, 3), (4, 64, 17), (9, 64, 16), (9, 784, 64), (4, 784, 100), (4, 784, 128)])
def test_one_step_lands_on_the_straight_line(P, D, d, layout):
    """The known answer of tests/test_geodesic_host.py, with the cross blocks from the kernel (exact: small integers)."""
    J, G, C, xhat, z, line, tol = known_answer(P, D, d, seed=0)
    got = run_cross(J, P, d, layout)
    assert np.array_equal(got[0], C)
    grad, delta, stats, seg2, info, *_ = run(J, G, got[0][None], xhat, np.zeros(1), P, layout)
    assert info.tolist() == [0]
    err = np.abs(z[1:-1] + delta[0] - line[1:-1]).max()
    print(f"P={P} D={D} d={d} {layout}: max |z + delta - line| = {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
def test_failures_are_reported_and_confined(layout):
    P, D, d = 4, 64, 5
    J, G, C, xhat = CE.inputs(3, P, D, d, seed=1)
    lam = np.zeros(3)
    clean = run(J, G, C, xhat, lam, P, layout)
    assert clean[4].tolist() == [0, 0, 0]
    Jz = J.copy()
    Jz[P + 2, :, 3] = 0.0                                            # an all-zero column at an interior point of curve 1
    Gz = (Jz.astype(np.float64).transpose(0, 2, 1) @ Jz.astype(np.float64)).astype(np.float32)
    Cz = CE.cross_of(Jz, P).astype(np.float32)
    assert same_bits(run_cross(Jz, P, d, layout)[1, :, :, 3], np.zeros((P - 3, d), dtype=np.float32))
    for value in CE.DAMPINGS:
        base = run(J, G, C, xhat, np.full(3, value), P, layout)
        grad, delta, stats, seg2, info, e_seg2, e_sum, e_info = run(Jz, Gz, Cz, xhat, np.full(3, value), P, layout)
        assert info.tolist() == [0, 1, 0] and e_info.tolist() == [0, 0, 0]
        assert np.isnan(delta[1]).all() and np.isnan(stats[1, 1:3]).all()
        assert np.isfinite(grad[1]).all() and np.isfinite(stats[1, [0, 3]]).all() and same_bits(seg2, base[3])
        for got, want in zip((grad, delta, stats, seg2), base):
            assert same_bits(got[[0, 2]], want[[0, 2]])
        assert CE.batch(Jz, Gz, Cz, xhat, np.full(3, value), P)[4].tolist() == info.tolist()
    for where in ("xhat", "xhat_end", "J", "G", "C"):
        Jn, Gn, Cn, hn = J.copy(), G.copy(), C.copy(), xhat.copy()
        if where == "xhat":
            hn[P + 1, 0] = NAN
        elif where == "xhat_end":
            hn[2 * P - 1, 3] = np.inf
        elif where == "J":
            Jn[P + 2, 3, 4] = NAN
        elif where == "G":
            Gn[P + 1, 4, 2] = NAN
        else:
            Cn[1, 0, 2, 4] = NAN
        out = run(Jn, Gn, Cn, hn, lam, P, layout)
        assert out[4].tolist() == [0, 2, 0], where
        assert all(np.isnan(o[1]).all() for o in out[:4]), where
        assert all(same_bits(o[[0, 2]], w[[0, 2]]) for o, w in zip(out[:4], clean[:4])), where
        assert out[7].tolist() == ([0, 2, 0] if where.startswith("xhat") else [0, 0, 0])
        if where.startswith("xhat"):
            assert np.isnan(out[5][1]).all() and np.isnan(out[6][1]) and same_bits(out[5][[0, 2]], clean[5][[0, 2]])
    # the end points' jtj and Jacobians and the upper triangles of jtj are never read
    Jn, Gn = J.copy(), G.copy()
    Gn[P] = NAN
    Gn[2 * P - 1] = NAN
    Jn[P] = NAN
    Jn[2 * P - 1] = NAN
    Gn[P + 1, 2, 4] = NAN
    for got, want in zip(run(Jn, Gn, C, xhat, lam, P, layout), clean):
        assert same_bits(got, want)


@pytest.mark.parametrize("P,D,d,layout", [(4, 64, 17, "panel"), (9, 784, 64, "fmajor"), (4, 5, 100, "panel"), (3, 64, 128, "fmajor"),
                                          (5, 64, 65, "panel")])
def test_outputs_stay_inside_their_buffers(P, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    curves, N, M = 2, P - 1, P - 2
    J, G, C, xhat = CE.inputs(curves, P, D, d, seed=2)
    lam = np.full(curves, 1e-3)
    T = stack(J, layout)
    Gc, hc, lc = torch.as_tensor(G).cuda(), torch.as_tensor(xhat).cuda(), torch.as_tensor(lam).cuda()
    lib = _lib.load()
    need = lib.cmf_curve_step_ws(d, P, curves)
    assert need > 0
    bufs = {"cross": guarded((curves, max(P - 3, 0), d, d), torch.float32), "grad": guarded((curves, M, d), torch.float64),
            "delta": guarded((curves, M, d), torch.float64), "stats": guarded((curves, 4), torch.float64),
            "seg2": guarded((curves, N), torch.float64), "info": guarded((curves,), torch.int32), "ws": guarded((need,), torch.float64),
            "stats_e": guarded((curves, 4), torch.float64), "seg2_e": guarded((curves, N), torch.float64),
            "info_e": guarded((curves,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    _lib.check(lib.cmf_cross_gram(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, curves, p("cross") if P > 3 else None, E._stream()),
               "cmf_cross_gram")
    _lib.check(lib.cmf_curve_step(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, curves, E._p(Gc), p("cross") if P > 3 else None, E._p(hc),
                                  E._p(lc), p("grad"), p("delta"), p("stats"), p("seg2"), p("info"), p("ws"), need, E._stream()),
               "cmf_curve_step")
    _lib.check(lib.cmf_curve_step(None, 0, 0, D, 0, 0, P, curves, None, None, E._p(hc), None, None, None, p("stats_e"), p("seg2_e"),
                                  p("info_e"), None, 0, E._stream()), "cmf_curve_step")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    got = lambda name: bufs[name][1].cpu().numpy()
    Ck = got("cross")
    grad, delta, stats, seg2, info, e_seg2, e_sum, e_info = run(J, G, Ck, xhat, lam, P, layout)
    assert same_bits(Ck, run_cross(J, P, d, layout))
    assert same_bits(got("grad"), grad) and same_bits(got("delta"), delta) and same_bits(got("stats"), stats)
    assert same_bits(got("seg2"), seg2) and (got("info") == info).all() and (info == 0).all() and (got("info_e") == 0).all()
    se = got("stats_e")
    assert same_bits(se[:, 0], stats[:, 0]) and np.isnan(se[:, 1:]).all() and same_bits(got("seg2_e"), seg2)


@pytest.mark.parametrize("P,D,d,layout", [(4, 64, 17, "panel"), (9, 784, 100, "panel"), (5, 64, 64, "fmajor")])
def test_position_independence_and_repeatability(P, D, d, layout):
    J, G, C, xhat = CE.inputs(3, P, D, d, seed=3)
    lam = np.array([0.0, 1e-3, 10.0])
    order = [0, 1, 2, 2, 0, 1, 1]
    rows = np.concatenate([np.arange(c * P, (c + 1) * P) for c in order])
    base = run(J, G, C, xhat, lam, P, layout)
    batch = run(J[rows], G[rows], C[order], xhat[rows], lam[order], P, layout)
    again = run(J[rows], G[rows], C[order], xhat[rows], lam[order], P, layout)
    for a, b, c in zip(base, batch, again):
        assert same_bits(a[order], b) and same_bits(b, c)
    for c in range(3):                                               # a curve alone: curves = 1
        sl = slice(c * P, (c + 1) * P)
        for a, b in zip(base, run(J[sl], G[sl], C[c:c + 1], xhat[sl], lam[c:c + 1], P, layout)):
            assert same_bits(a[c:c + 1], b)


def test_entry_points_refuse_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    curves, P, D, d = 2, 4, 8, 3
    J, G, C, xhat = CE.inputs(curves, P, D, d)
    T = stack(J, "panel")
    Gc, Cc, hc = torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    lc = torch.zeros(curves, dtype=torch.float64, device="cuda")
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    grad, delta, stats, seg2 = z64(curves * (P - 2) * d + 1), z64(curves * (P - 2) * d), z64(curves * 4), z64(curves * (P - 1))
    info = torch.zeros(curves, dtype=torch.int32, device="cuda")
    need = lib.cmf_curve_step_ws(d, P, curves)
    ws = z64(need)
    odd = grad.view(torch.float32)[1:]                              # 4 bytes past an 8-byte boundary
    off16 = E._p(T.data.view(torch.float32)[1:])
    for args in ((0, P, curves), (129, P, curves), (d, 2, curves), (d, P, 0), (d, P, -1)):
        assert lib.cmf_curve_step_ws(*args) == -1, args
    assert lib.cmf_curve_step_ws(128, 3, 1) > lib.cmf_curve_step_ws(64, 3, 1) > 0
    # cmf_cross_gram
    cross = torch.zeros_like(Cc)
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, curves, E._p(cross)]
    assert lib.cmf_cross_gram(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(cross.abs().sum()) > 0
    cross.zero_()
    bad = [(0, None), (0, off16), (1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (3, 0), (4, 24), (4, 0), (4, 144), (5, 0), (5, 129), (5, 17),
           (6, 2), (7, 0), (8, None)]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_cross_gram(*args, E._stream()) == -1, (i, value)
    three = list(ok)
    three[6], three[8] = 3, None                                    # P == 3: nothing to write, cross may be NULL
    assert lib.cmf_cross_gram(*three, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(cross.abs().sum()) == 0.0
    # cmf_curve_step
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, curves, E._p(Gc), E._p(Cc), E._p(hc), E._p(lc), E._p(grad), E._p(delta),
          E._p(stats), E._p(seg2), E._p(info), E._p(ws), need]
    assert lib.cmf_curve_step(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(delta.abs().sum()) > 0
    for t in (grad, delta, stats, seg2):
        t.zero_()
    bad = [(0, off16), (1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (3, 0), (4, 24), (4, 0), (5, 0), (5, 129), (5, 17), (6, 2), (7, 0),
           (8, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None), (16, None), (17, None),
           (18, need - 1), (11, E._p(odd)), (12, E._p(odd)), (13, E._p(odd)), (14, E._p(odd)), (15, E._p(odd)), (17, E._p(odd))]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_curve_step(*args, E._stream()) == -1, (i, value)
    # energy-only mode: xhat, stats, seg2 and info are still required
    res = [None, 0, 0, D, 0, 0, P, curves, None, None, E._p(hc), None, None, None, E._p(stats), E._p(seg2), E._p(info), None, 0]
    for i, value in ((3, 0), (6, 2), (7, 0), (10, None), (14, None), (15, None), (16, None), (14, E._p(odd)), (15, E._p(odd))):
        args = list(res)
        args[i] = value
        assert lib.cmf_curve_step(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in (grad, delta, stats, seg2))


def test_engine_refusals():
    from cmf_amd import engine as E
    curves, P, D, d = 2, 4, 8, 3
    J, G, C, xhat = CE.inputs(curves, P, D, d)
    T, Gc, Cc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    lam = torch.zeros(curves, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.cross_gram(E.Tangent(8, 8, 144, "panel", "cuda"), 129, 4)
    with pytest.raises(ValueError, match="points >= 3"):
        E.cross_gram(T, d, 2)
    with pytest.raises(ValueError, match="whole curves"):
        E.cross_gram(T, d, 3)
    with pytest.raises(ValueError, match="points >= 3"):
        E.curve_energy(hc, 2)
    with pytest.raises(ValueError, match="whole curves"):
        E.curve_energy(hc, 3)
    with pytest.raises(ValueError, match="float32"):
        E.curve_energy(hc.double(), P)
    with pytest.raises(ValueError, match="contiguous"):
        E.curve_energy(hc.t().contiguous().t(), P)
    with pytest.raises(ValueError, match="contiguous"):
        E.curve_step(T, Gc.transpose(1, 2), Cc, hc, P, lam)
    with pytest.raises(ValueError, match="float32"):
        E.curve_step(T, Gc.double(), Cc, hc, P, lam)
    with pytest.raises(ValueError, match="float32"):
        E.curve_step(T, Gc, Cc.double(), hc, P, lam)
    with pytest.raises(ValueError, match="cross must be"):
        E.curve_step(T, Gc, Cc[:, :0], hc, P, lam)
    with pytest.raises(ValueError, match="float64"):
        E.curve_step(T, Gc, Cc, hc, P, lam.float())
    with pytest.raises(ValueError, match="must hold"):
        E.curve_step(T, Gc, Cc, hc[:, :7].contiguous(), P, lam)
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.curve_step(E.Tangent(4, 8, 144, "panel", "cuda"), torch.zeros(4, 129, 129, device="cuda"), torch.zeros(1, 1, 129, 129, device="cuda"),
                     hc[:4], 4, lam[:1])
    for cpu in ((T, Gc.cpu(), Cc, hc, P, lam), (T, Gc, Cc.cpu(), hc, P, lam), (T, Gc, Cc, hc.cpu(), P, lam)):
        with pytest.raises(ValueError, match="GPU"):
            E.curve_step(*cpu)
    # no curve: empties, no launch
    r = E.curve_step(E.Tangent(0, 8, 16, "panel", "cuda"), Gc[:0], Cc[:0], hc[:0], P, lam[:0])
    assert r.grad.shape == (0, 2, 3) and r.delta.shape == (0, 2, 3) and r.stats.shape == (0, 4) and r.seg2.shape == (0, 3)
    assert r.info.shape == (0,)
    seg2, total, info = E.curve_energy(hc[:0], P)
    assert seg2.shape == (0, 3) and total.shape == (0,) and total.dtype == torch.float64 and info.shape == (0,)
    assert E.cross_gram(E.Tangent(0, 8, 16, "panel", "cuda"), d, P).shape == (0, 1, 3, 3)


def test_kernel_timer_entries():
    from cmf_amd import engine as E
    curves, P, D, d = 2, 4, 8, 3
    J, G, C, xhat = CE.inputs(curves, P, D, d)
    T, Gc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(xhat).cuda()
    with E.timing(lambda name: True) as timer:
        cross = E.cross_gram(T, d, P)
        E.curve_step(T, Gc, cross, hc, P, torch.zeros(curves, dtype=torch.float64, device="cuda"))
        E.curve_energy(hc, P)
    by = timer.by_name()
    assert set(by) == {"cross_gram", "curve_step", "curve_energy"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------


def fixture_ends(name, x):
    h = x.shape[0] // 2
    n = 1 if name in R.ONE_CURVE else h
    return x[:n].contiguous(), x[h:h + n].contiguous()


def run_connect(dens, head, x0, x1, steps, points=R.POINTS):
    """One ``connect`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    geo = cmf_amd.ManifoldGeodesic(dens, points=points, steps=steps)
    keep0, keep1, marker = x0.clone(), x1.clone(), object()
    head.last_gram = marker
    out = geo.connect(x0, x1)
    assert head.last_gram is marker and torch.equal(x0, keep0) and torch.equal(x1, keep1)
    B, d, P = x0.shape[0], head.program.d, points
    assert out["latents"].shape == (B, P, d) and out["latents"].dtype == torch.float32
    assert out["path_head"].shape == (B, P, *head.x_shape) and out["path"].shape == (B, P, *x0.shape[1:])
    for key in ("energy", "initial_energy", "length", "initial_length", "gradient_max", "damping"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64
    assert out["segment_lengths"].shape == (B, P - 1) and out["gradient"].shape == (B, P - 2, d)
    for key in ("accepted", "info"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    assert bool((out["energy"] <= out["initial_energy"]).all()) and bool((0 <= out["accepted"]).all())
    assert bool((out["accepted"] <= steps).all())
    return geo, out


@pytest.mark.parametrize("name", R.FIXTURES)
def test_connect_relaxes_the_straight_line(name):
    g, meta, dens, head, x = build(name)
    x0, x1 = fixture_ends(name, x)
    model, ref0, ref = R.reference_run(name)
    N, B = R.POINTS - 1, x0.shape[0]
    outs = [run_connect(dens, head, x0, x1, steps)[1] for steps in (0, 4, R.STEPS)]
    start, end = outs[0], outs[-1]
    energies = torch.stack([o["energy"] for o in outs])
    assert bool((end["info"] == 0).all()) and bool((start["info"] == 0).all())
    assert bool((energies[1:] <= energies[:-1]).all())              # monotone in the number of steps: a prefix of the same loop
    assert torch.equal(start["energy"], start["initial_energy"]) and torch.equal(start["initial_energy"], end["initial_energy"])
    assert bool((start["accepted"] == 0).all())
    for out in (start, end):                                         # L^2 <= E to the float64 rounding of the two sums of N terms
        assert bool((out["length"] ** 2 <= out["energy"] * (1 + 4 * (N + 2) * 2.0 ** -53)).all())
        assert torch.equal(out["length"], out["segment_lengths"].sum(1))
    # the bounds come from the reference run alone
    xr = ref["path_head"]                                            # (B, P, D) float64
    colsum = ref["jacobian"].abs().sum(2).flatten(1).max(1).values
    g_floor = 4e-5 * xr.abs().flatten(1).max(1).values * colsum
    g_need = torch.maximum(10.0 * ref["gradient_max"], g_floor)
    e_tol = 2.0 * (2e-5 * xr.norm(dim=2).max(1).values) / ref["segment_lengths"].min(1).values
    gm, e_rel = end["gradient_max"].cpu(), (end["energy"].cpu() - ref["energy"]).abs() / ref["energy"]
    print(f"{name}: accepted {end['accepted'].tolist()} (reference {ref['accepted'].tolist()}); gradient_max / allowed in "
          f"[{float((gm / g_need).min()):.3e}, {float((gm / g_need).max()):.3e}] (fell by {float((start['gradient_max'].cpu() / gm).min()):.3g}"
          f" .. {float((start['gradient_max'].cpu() / gm).max()):.3g}); |E - E_ref| / E_ref / tolerance max {float((e_rel / e_tol).max()):.3e}; "
          f"energy gain {float((1 - end['energy'] / end['initial_energy']).max()):.3e}")
    assert bool((gm <= g_need).all())
    assert bool((e_rel <= e_tol).all())
    e0_rel = (start["energy"].cpu() - ref0["energy"]).abs() / ref0["energy"]
    assert bool((e0_rel <= 2.0 * (2e-5 * ref0["path_head"].norm(dim=2).max(1).values) / ref0["segment_lengths"].min(1).values).all())
    with torch.no_grad():
        assert torch.equal(end["path_head"].flatten(0, 1), head.flow_forward(end["latents"].flatten(0, 1)))


def test_a_point_connects_to_itself_at_zero_cost():
    g, meta, dens, head, x = build("c2a_power")
    x = x[:3].contiguous()
    for steps in (0, 3):
        _, out = run_connect(dens, head, x, x, steps, points=5)
        assert bool((out["info"] == 0).all()) and bool((out["accepted"] == 0).all())
        for key in ("energy", "initial_energy", "length", "initial_length", "gradient_max"):
            assert bool((out[key] == 0).all()), key
        assert bool((out["gradient"] == 0).all()) and bool((out["segment_lengths"] == 0).all())


def test_zero_steps_return_the_straight_latent_line():
    g, meta, dens, head, x = build("c2b_hepmass")
    x0, x1 = fixture_ends("c2b_hepmass", x)
    _, out = run_connect(dens, head, x0, x1, 0, points=6)
    with torch.no_grad():
        z0 = dens.extract_latent(x0.clone(), earliest_latent=False)
        z1 = dens.extract_latent(x1.clone(), earliest_latent=False)
    z = out["latents"]
    assert torch.equal(z[:, 0], z0) and torch.equal(z[:, -1], z1)
    tt = torch.arange(6, device="cuda", dtype=torch.float64) / 5
    line = z0.double()[:, None] + tt[None, :, None] * (z1.double() - z0.double())[:, None]
    assert float((z.double() - line).abs().max()) <= 8 * 2.0 ** -24 * float(line.abs().max())
    assert torch.equal(out["energy"], out["initial_energy"]) and torch.equal(out["length"], out["initial_length"])
    import cmf_amd
    same = cmf_amd.ManifoldGeodesic(dens, points=6).connect_latents(z0, z1, steps=0)
    assert all(torch.equal(same[k], out[k]) for k in out)


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_curves_of_one_call(name, monkeypatch):
    import cmf_amd
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    h, P = x.shape[0] // 2, 4
    x0, x1 = x[[0, 1, 0]].contiguous(), x[[h, h + 1, h + 1]].contiguous()      # three curves from a batch of four or more
    _, whole = run_connect(dens, head, x0, x1, 6, points=P)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * P * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3 * P) // P == 1                      # 3 curves run as three sub-batches of one curve
    _, pieces = run_connect(dens, head, x0, x1, 6, points=P)
    e0 = whole["initial_energy"]
    print(f"{name}: pieces against whole: bit-equal latents {torch.equal(pieces['latents'], whole['latents'])}, energy rel "
          f"{float(((pieces['energy'] - whole['energy']).abs() / e0).max()):.2e}")
    assert float(((pieces["initial_energy"] - e0).abs() / e0).max()) <= 1e-5
    assert float(((pieces["energy"] - whole["energy"]).abs() / e0).max()) <= 1e-5
    assert bool((pieces["info"] == 0).all()) and pieces["latents"].shape == whole["latents"].shape
    # a curve that does not fit one sub-batch
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    with pytest.raises(ValueError, match="points"):
        cmf_amd.ManifoldGeodesic(dens, points=P).connect(x0, x1)


def test_the_log_density_path_is_untouched():
    import cmf_amd
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    h = x.shape[0] // 2
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        marker = head.last_gram
        cmf_amd.ManifoldGeodesic(dens, points=4, steps=2).connect(x[:2].contiguous(), x[h:h + 2].contiguous())
        assert head.last_gram is marker
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
