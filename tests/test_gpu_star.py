"""The Frechet means on the GPU: the star step kernels (csrc/star_step.hip) against float64 numpy on the same float32
inputs, against ``engine.curve_step`` on a two-arm star joined into one curve and on a known answer, their output contract,
isolation, determinism and refusals, and ``cmf_amd.ManifoldGeodesic.mean`` end to end on the reference-generated fixtures under the
conditions tests/test_star_host.py establishes on the float64 reference loop.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds (u = 2^-53), per star of K arms with M interior points each:
    ||A delta - g||_inf <= 96 d u (||A||_inf ||delta||_inf + ||g||_inf)       with the kernels' own g on the dense ((K M + 1) d)^2
                                                                              matrix: the band's 64 d u with the centre as a third level
    |g - g_ref| <= 2 (D + 4) u w_k sum_r |J| |s|                              at the arm points
    |g_c - ref| <= 2 (D + K + 4) u sum_k w_k sum_r |J| |s|                    at the centre: the arm sum on top
    seg2: 2 (D + 2) u relative;  g^T delta, delta^T H delta: 2 (n + K + 2) u sum |terms|, against recomputation from the outputs.
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN; the fmajor runs hold the stack from sample 1 of a
Jacobian stack padded with a NaN sample at each end."""
import numpy as np
import pytest
import torch

import _curve_step_emulation as CE
import _frechet_reference as FR
import _star_step_emulation as SE
from test_gpu_geodesic import run as run_curve
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits, stack
from test_star_host import KNOWN, WEIGHTS, check_star, damping_family, known_answer, known_answer_error

pytestmark = pytest.mark.gpu

NAN = float("nan")
VALUES = ("grad", "grad_centre", "delta", "delta_centre", "seg2", "stats")


def padded_stack(J, layout, first):
    if first:
        J = np.concatenate([np.full_like(J[:1], NAN), J, np.full_like(J[:1], NAN)])
    return stack(J, layout)


def run(J, G, C, xhat, w, lam, P, layout="panel"):
    """``engine.star_step`` on CPU inputs -> a dict of numpy arrays (the StarStepResult's fields).  fmajor: behind a padded stack."""
    from cmf_amd import engine as E
    first = int(layout == "fmajor")
    K = w.shape[1]
    n = w.shape[0] * K * P
    r = E.star_step(padded_stack(J[:n], layout, first), torch.as_tensor(G[:n]).cuda(), torch.as_tensor(C[:n - 1]).cuda(),
                    torch.as_tensor(xhat[:n]).cuda(), P, K, torch.as_tensor(w, dtype=torch.float64).cuda(),
                    torch.as_tensor(lam, dtype=torch.float64).cuda(), first=first)
    torch.cuda.synchronize()
    return {key: getattr(r, key).cpu().numpy() for key in VALUES + ("info",)}


def star_of(out, s):
    return {key: v[s] for key, v in out.items()}


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("d", [16, 17, 64, 65, 100, 128])
def test_star_step_matches_float64(d, layout):
    worst = np.zeros(3)
    cases = [(stars, K, P, 64) for stars in (1, 3) for K in SE.ARMS for P in (3, 4)] + [(3, 3, 4, 784), (3, 2, 3, 5)]
    if d == 17:
        cases += [(1, 3, 9, 64), (3, 2, 9, 64)]
    for stars, K, P, D in cases:
        lams = damping_family(D, d)
        lam = np.array([lams[s % len(lams)] for s in range(stars)]) if stars > 1 else np.array([1e-3])
        J, G, C, xhat = SE.inputs(stars, K, P, D, d, seed=stars)
        w = np.tile(WEIGHTS[:K], (stars, 1))
        out = run(J, G, C, xhat, w, lam, P, layout)
        assert (out["info"] == 0).all(), (stars, K, P, D)
        n = K * P
        for s in range(stars):
            worst = np.maximum(worst, check_star(J[s * n:(s + 1) * n], G[s * n:(s + 1) * n], C[s * n:], xhat[s * n:(s + 1) * n], w[s],
                                                 lam[s], P, star_of(out, s), SE.BOUND_C, f"stars {stars} K {K} P {P} D {D} star {s}"))
    print(f"d={d} {layout}: reached fractions of the bounds: residual {worst[0]:.4f} (of {SE.BOUND_C:g} d u), gradient {worst[1]:.3f}, "
          f"centre gradient {worst[2]:.3f}")


@pytest.mark.parametrize("P,D,d", [(3, 5, 3), (4, 64, 17), (4, 64, 16), (3, 784, 64), (4, 784, 100), (3, 64, 128)])
def test_two_equal_arms_are_the_joined_curve(P, D, d):
    from cmf_amd import engine as E
    for lam in damping_family(D, d):
        J, G, C, xhat = SE.inputs(1, 2, P, D, d, seed=6)
        star = star_of(run(J, G, C, xhat, np.ones((1, 2)), np.array([lam]), P), 0)
        Jj, Gj, Cj, xj = SE.joined(J, G, C, xhat, P)
        grad, delta, stats, seg2, info, *_ = run_curve(Jj, Gj, Cj[None], xj, np.array([lam]), 2 * P - 1)
        assert star["info"] == 0 and info.tolist() == [0]
        A, _ = CE.dense(Gj, Cj, lam)
        as_curve = np.concatenate([star["delta"][0], star["delta_centre"][None], star["delta"][1][::-1]])
        ratio = CE.residual_ratio(A, d, grad[0], as_curve)
        print(f"P={P} D={D} d={d} lambda={lam:g}: residual of the star's step in the curve's system {ratio:.4f} (bound {SE.BOUND_C:g} d u); "
              f"max |delta_star - delta_curve| / max |delta| = {float(np.abs(as_curve - delta[0]).max() / np.abs(delta[0]).max()):.2e}")
        assert ratio <= SE.BOUND_C
        assert abs(star["stats"][0] - stats[0, 0]) <= 4 * SE.U * stats[0, 0]
        assert same_bits(np.concatenate([star["seg2"][0], star["seg2"][1][::-1]]), seg2[0])
        # the arms as curves: the energy-only mode of the curve kernel gives the bits of seg2
        e_seg2, e_sum, _ = E.curve_energy(torch.as_tensor(xhat).cuda(), P)
        assert same_bits(e_seg2.cpu().numpy(), star["seg2"])


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("K,P,D,d,fixed", KNOWN)
def test_one_step_lands_on_the_weighted_mean(K, P, D, d, fixed, layout):
    """The known answer of tests/test_star_host.py at 4 x its tolerance."""
    J, G, C, xhat, w, z, target, tol = known_answer(K, P, D, d, seed=0)
    tol = min(tol, fixed)
    out = star_of(run(J, G, C, xhat, w[None], np.zeros(1), P, layout), 0)
    assert out["info"] == 0
    err = known_answer_error(out, z, target)
    print(f"K={K} P={P} D={D} d={d} {layout}: max |z + delta - target| = {err:.3e} (tolerance {4 * tol:.3e})")
    assert err <= 4 * tol


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
def test_failures_are_reported_and_confined(layout):
    K, P, D, d = 3, 4, 64, 5
    n = K * P
    J, G, C, xhat = SE.inputs(3, K, P, D, d, seed=1)
    w, lam = np.tile(WEIGHTS[:K], (3, 1)), np.zeros(3)
    clean = run(J, G, C, xhat, w, lam, P, layout)
    assert clean["info"].tolist() == [0, 0, 0]

    def regram(Jz):
        J64 = Jz.astype(np.float64)
        return (J64.transpose(0, 2, 1) @ J64).astype(np.float32), SE.cross_of(Jz).astype(np.float32)

    # a zero Jacobian column in one arm of star 1, or at every copy of its centre: info 1
    for rows in ([n + P + 2], [n + k * P + P - 1 for k in range(K)]):
        Jz = J.copy()
        Jz[rows, :, 3] = 0.0
        Gz, Cz = regram(Jz)
        for value in SE.DAMPINGS:
            base = run(J, G, C, xhat, w, np.full(3, value), P, layout)
            out = run(Jz, Gz, Cz, xhat, w, np.full(3, value), P, layout)
            assert out["info"].tolist() == [0, 1, 0]
            assert np.isnan(out["delta"][1]).all() and np.isnan(out["delta_centre"][1]).all() and np.isnan(out["stats"][1, 1:3]).all()
            assert np.isfinite(out["grad"][1]).all() and np.isfinite(out["grad_centre"][1]).all()
            assert np.isfinite(out["stats"][1, [0, 3]]).all() and same_bits(out["seg2"], base["seg2"])
            assert all(same_bits(out[key][[0, 2]], base[key][[0, 2]]) for key in VALUES)
            assert SE.batch(Jz, Gz, Cz, xhat, w, np.full(3, value), P)["info"].tolist() == [0, 1, 0]
    # a non-finite value in one arm: info 2, alone or beside a failing pivot in another arm of the star
    Jz = J.copy()
    Jz[n + 2, :, 3] = 0.0
    Gz, Cz = regram(Jz)
    for where in ("xhat", "xhat_end", "J", "J_centre", "G", "G_centre", "C", "weight"):
        for Jb, Gb, Cb in ((J, G, C), (Jz, Gz, Cz)):
            Jn, Gn, Cn, hn, wn = Jb.copy(), Gb.copy(), Cb.copy(), xhat.copy(), w.copy()
            if where == "xhat":
                hn[n + P + 1, 0] = NAN
            elif where == "xhat_end":
                hn[n + 2 * P, 3] = np.inf
            elif where == "J":
                Jn[n + P + 2, 3, 4] = NAN
            elif where == "J_centre":
                Jn[n + 2 * P - 1, 3, 4] = NAN
            elif where == "G":
                Gn[n + P + 1, 4, 2] = NAN
            elif where == "G_centre":
                Gn[n + 3 * P - 1, 4, 2] = NAN
            elif where == "C":
                Cn[n + P + 2, 2, 4] = NAN
            else:
                wn[1, 2] = np.inf
            out = run(Jn, Gn, Cn, hn, wn, lam, P, layout)
            assert out["info"].tolist() == [0, 2, 0], where
            assert all(np.isnan(out[key][1]).all() for key in VALUES), where
            assert all(same_bits(out[key][[0, 2]], clean[key][[0, 2]]) for key in VALUES), where
    # never read: the fixed ends' Jacobians and jtj, the upper triangles, the cross blocks of the fixed ends and between two arms
    Jn, Gn, Cn = J.copy(), G.copy(), C.copy()
    for k in range(K):
        Jn[n + k * P] = NAN
        Gn[n + k * P] = NAN
        Cn[n + k * P] = NAN
        Cn[n + k * P + P - 1] = NAN
    Gn[n + 1, 2, 4] = NAN
    out = run(Jn, Gn, Cn, xhat, w, lam, P, layout)
    assert all(same_bits(out[key], clean[key]) for key in VALUES + ("info",))


@pytest.mark.parametrize("layout", ["panel", "fmajor"])
@pytest.mark.parametrize("n,D,d", [(3, 5, 3), (4, 64, 17), (13, 64, 16), (24, 784, 64), (7, 64, 128)])
def test_star_cross_gram_gives_the_blocks_of_the_unpadded_stack(n, D, d, layout):
    """Every block a star reads, to the bound of ``cross_gram`` (2 (D + 2) 2^-24 sum_r |J_a| |J_b|) and with the bits ``cross_gram``
    gives on the stack padded by one sample at each end; block 0 is zero."""
    from cmf_amd import engine as E
    J, _, _, _ = CE.inputs(1, n, D, d, seed=8)
    got = E.star_cross_gram(stack(J, layout), d)
    padded = E.cross_gram(padded_stack(J, layout, 1), d, n + 2)[0]
    torch.cuda.synchronize()
    got, padded = got.cpu().numpy(), padded.cpu().numpy()
    assert got.shape == (n - 1, d, d) and got.dtype == np.float32 and not got[0].any()
    assert same_bits(got[1:], padded[1:])
    ref, mag = SE.cross_of(J)[1:], SE.cross_of(np.abs(J))[1:]
    assert (np.abs(got[1:].astype(np.float64) - ref) <= 2 * (D + 2) * 2.0 ** -24 * mag).all()


def call_entry(lib, E, T, first, D, d, P, K, stars, Gc, Cc, hc, wc, lc, bufs, need):
    p = lambda name: E._p(bufs[name][1])
    return lib.cmf_star_step(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, K, stars, first, E._p(Gc), E._p(Cc), E._p(hc), E._p(wc), E._p(lc),
                             p("grad"), p("grad_centre"), p("delta"), p("delta_centre"), p("arm"), p("seg2"), p("info"), p("ws"), need,
                             E._stream())


@pytest.mark.parametrize("K,P,D,d,layout", [(3, 4, 64, 17, "panel"), (2, 5, 784, 64, "fmajor"), (5, 3, 5, 100, "panel"),
                                            (1, 3, 64, 128, "fmajor"), (2, 4, 64, 65, "panel")])
def test_outputs_stay_inside_their_buffers(K, P, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    stars, N, M = 2, P - 1, P - 2
    J, G, C, xhat = SE.inputs(stars, K, P, D, d, seed=2)
    w, lam = np.tile(WEIGHTS[:K], (stars, 1)), np.full(stars, 1e-3)
    first = int(layout == "fmajor")
    T = padded_stack(J, layout, first)
    Gc, Cc, hc = torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    wc, lc = torch.as_tensor(w).cuda(), torch.as_tensor(lam).cuda()
    lib = _lib.load()
    need = lib.cmf_star_step_ws(d, P, K, stars)
    assert need > 0
    f64 = torch.float64
    bufs = {"grad": guarded((stars, K, M, d), f64), "grad_centre": guarded((stars, d), f64), "delta": guarded((stars, K, M, d), f64),
            "delta_centre": guarded((stars, d), f64), "arm": guarded((stars, K, 4), f64), "seg2": guarded((stars, K, N), f64),
            "info": guarded((stars,), torch.int32), "ws": guarded((need,), f64)}
    _lib.check(call_entry(lib, E, T, first, D, d, P, K, stars, Gc, Cc, hc, wc, lc, bufs, need), "cmf_star_step")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    got = lambda name: bufs[name][1].cpu().numpy()
    out = run(J, G, C, xhat, w, lam, P, layout)
    for key in ("grad", "grad_centre", "delta", "delta_centre", "seg2"):
        assert same_bits(got(key), out[key]), key
    assert (got("info") == 0).all() and (out["info"] == 0).all()
    arm = got("arm")
    assert np.isfinite(arm).all()
    for j in range(3):                                               # the engine's sums over the arms, in arm order
        total = np.zeros(stars)
        for k in range(K):
            total = total + w[:, k] * arm[:, k, j]
        assert same_bits(total, out["stats"][:, j])


@pytest.mark.parametrize("K,P,D,d,layout", [(3, 4, 64, 17, "panel"), (2, 5, 784, 100, "panel"), (3, 3, 64, 64, "fmajor")])
def test_position_independence_and_repeatability(K, P, D, d, layout):
    J, G, C, xhat = SE.inputs(3, K, P, D, d, seed=3)
    n = K * P
    w = np.stack([WEIGHTS[:K], WEIGHTS[:K][::-1], np.ones(K)])
    lam = np.array([0.0, 1e-3, 10.0])
    order = [0, 1, 2, 2, 0, 1, 1]
    rows = np.concatenate([np.arange(s * n, (s + 1) * n) for s in order])
    Cp = np.full((len(rows) - 1, d, d), NAN, dtype=np.float32)      # the blocks between two stars are not read
    for i, s in enumerate(order):
        Cp[i * n:(i + 1) * n - 1] = C[s * n:(s + 1) * n - 1]
    base = run(J, G, C, xhat, w, lam, P, layout)
    batch = run(J[rows], G[rows], Cp, xhat[rows], w[order], lam[order], P, layout)
    again = run(J[rows], G[rows], Cp, xhat[rows], w[order], lam[order], P, layout)
    for key in VALUES + ("info",):
        assert same_bits(base[key][order], batch[key]) and same_bits(batch[key], again[key]), key
    for s in range(3):                                               # a star alone: stars = 1
        sl = slice(s * n, (s + 1) * n)
        alone = run(J[sl], G[sl], C[s * n:], xhat[sl], w[s:s + 1], lam[s:s + 1], P, layout)
        for key in VALUES + ("info",):
            assert same_bits(base[key][s:s + 1], alone[key]), key


def test_entry_points_refuse_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    stars, K, P, D, d = 2, 2, 4, 8, 3
    J, G, C, xhat = SE.inputs(stars, K, P, D, d)
    T = stack(J, "panel")
    Gc, Cc, hc = torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    wc = torch.ones(stars, K, dtype=torch.float64, device="cuda")
    lc = torch.zeros(stars, dtype=torch.float64, device="cuda")
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    Md = stars * K * (P - 2) * d
    grad, delta, gcen, dcen, arm, seg2 = z64(Md + 1), z64(Md), z64(stars * d), z64(stars * d), z64(stars * K * 4), z64(stars * K * (P - 1))
    info = torch.zeros(stars, dtype=torch.int32, device="cuda")
    need = lib.cmf_star_step_ws(d, P, K, stars)
    ws = z64(need)
    odd = grad.view(torch.float32)[1:]                              # 4 bytes past an 8-byte boundary
    off16 = E._p(T.data.view(torch.float32)[1:])
    for args in ((0, P, K, stars), (129, P, K, stars), (d, 2, K, stars), (d, P, 0, stars), (d, P, 65, stars), (d, P, K, 0), (d, P, K, -1)):
        assert lib.cmf_star_step_ws(*args) == -1, args
    assert lib.cmf_star_step_ws(128, 3, 1, 1) > lib.cmf_star_step_ws(64, 3, 1, 1) > 0
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, P, K, stars, 0, E._p(Gc), E._p(Cc), E._p(hc), E._p(wc), E._p(lc), E._p(grad), E._p(gcen),
          E._p(delta), E._p(dcen), E._p(arm), E._p(seg2), E._p(info), E._p(ws), need]
    assert lib.cmf_star_step(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert float(delta.abs().sum()) > 0 and float(dcen.abs().sum()) > 0
    outs = (grad, delta, gcen, dcen, arm, seg2)
    for t in outs:
        t.zero_()
    bad = [(0, None), (0, off16), (1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (3, 0), (4, 24), (4, 0), (5, 0), (5, 129), (5, 17), (6, 2),
           (7, 0), (7, 65), (8, 0), (9, -1), (23, need - 1)]
    bad += [(i, None) for i in range(10, 23)] + [(i, E._p(odd)) for i in (13, 14, 15, 16, 17, 18, 19, 20, 22)]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_star_step(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in outs)


def test_engine_refusals():
    from cmf_amd import engine as E
    stars, K, P, D, d = 2, 2, 4, 8, 3
    J, G, C, xhat = SE.inputs(stars, K, P, D, d)
    T, Gc, Cc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    w = torch.ones(stars, K, dtype=torch.float64, device="cuda")
    lam = torch.zeros(stars, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="1 <= arms <= 64"):
        E.star_step(T, Gc, Cc, hc, P, 0, w, lam)
    with pytest.raises(ValueError, match="points >= 3"):
        E.star_step(T, Gc, Cc, hc, 2, K, w, lam)
    with pytest.raises(ValueError, match="whole"):
        E.star_step(T, Gc, Cc, hc, 3, K, w, lam)
    with pytest.raises(ValueError, match="whole stars"):
        E.star_step(T, Gc, Cc, hc, P, 3, w, lam)
    with pytest.raises(ValueError, match="contiguous"):
        E.star_step(T, Gc.transpose(1, 2), Cc, hc, P, K, w, lam)
    with pytest.raises(ValueError, match="float32"):
        E.star_step(T, Gc.double(), Cc, hc, P, K, w, lam)
    with pytest.raises(ValueError, match="float32"):
        E.star_step(T, Gc, Cc.double(), hc, P, K, w, lam)
    with pytest.raises(ValueError, match="cross must be"):
        E.star_step(T, Gc, Cc[:-1], hc, P, K, w, lam)
    with pytest.raises(ValueError, match="float64"):
        E.star_step(T, Gc, Cc, hc, P, K, w.float(), lam)
    with pytest.raises(ValueError, match="weights must be"):
        E.star_step(T, Gc, Cc, hc, P, K, w[:, :1].contiguous(), lam)
    with pytest.raises(ValueError, match="float64"):
        E.star_step(T, Gc, Cc, hc, P, K, w, lam.float())
    with pytest.raises(ValueError, match="must hold"):
        E.star_step(T, Gc, Cc, hc[:, :7].contiguous(), P, K, w, lam)
    with pytest.raises(ValueError, match="must hold"):
        E.star_step(T, Gc, Cc, hc, P, K, w, lam, first=1)          # T holds no sample behind the stack
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.star_step(E.Tangent(8, 8, 144, "panel", "cuda"), torch.zeros(8, 129, 129, device="cuda"), torch.zeros(7, 129, 129, device="cuda"),
                    hc[:8], 4, 2, w[:1], lam[:1])
    for cpu in ((T, Gc.cpu(), Cc, hc, P, K, w, lam), (T, Gc, Cc.cpu(), hc, P, K, w, lam), (T, Gc, Cc, hc.cpu(), P, K, w, lam),
                (T, Gc, Cc, hc, P, K, w.cpu(), lam)):
        with pytest.raises(ValueError, match="GPU"):
            E.star_step(*cpu)
    # no star: empties, no launch
    r = E.star_step(E.Tangent(0, 8, 16, "panel", "cuda"), Gc[:0], Cc[:0], hc[:0], P, K, w[:0], lam[:0])
    assert r.grad.shape == (0, 2, 2, 3) and r.delta.shape == (0, 2, 2, 3) and r.grad_centre.shape == (0, 3)
    assert r.delta_centre.shape == (0, 3) and r.stats.shape == (0, 4) and r.seg2.shape == (0, 2, 3) and r.info.shape == (0,)


def test_kernel_timer_entry():
    from cmf_amd import engine as E
    stars, K, P, D, d = 2, 2, 4, 8, 3
    J, G, C, xhat = SE.inputs(stars, K, P, D, d)
    T, Gc, Cc, hc = stack(J, "panel"), torch.as_tensor(G).cuda(), torch.as_tensor(C).cuda(), torch.as_tensor(xhat).cuda()
    with E.timing(lambda name: True) as timer:
        E.star_step(T, Gc, Cc, hc, P, K, torch.ones(stars, K, dtype=torch.float64, device="cuda"),
                    torch.zeros(stars, dtype=torch.float64, device="cuda"))
    by = timer.by_name()
    assert set(by) == {"star_step"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in by.values())


# --------------------------------------------------------------------------------------------------
# end to end on the fixtures
# --------------------------------------------------------------------------------------------------


def run_mean(dens, head, xs, weights, steps, points=FR.POINTS):
    """One ``mean`` with the side-effect and shape checks every end-to-end case makes."""
    import cmf_amd
    geo = cmf_amd.ManifoldGeodesic(dens, points=points, steps=steps)
    keep, marker = xs.clone(), object()
    head.last_gram = marker
    out = geo.mean(xs, weights)
    assert head.last_gram is marker and torch.equal(xs, keep)
    B, K, d, P = xs.shape[0], xs.shape[1], head.program.d, points
    assert out["mean_latent"].shape == (B, d) and out["mean_latent"].dtype == torch.float32
    assert out["mean_head"].shape == (B, *head.x_shape) and out["mean"].shape == (B, *xs.shape[2:])
    assert out["latents"].shape == (B, K, P, d) and out["latents"].dtype == torch.float32
    assert out["path_head"].shape == (B, K, P, *head.x_shape) and out["path"].shape == (B, K, P, *xs.shape[2:])
    for key in ("energy", "initial_energy", "variance", "gradient_max", "damping"):
        assert out[key].shape == (B,) and out[key].dtype == torch.float64, key
    for key in ("distances", "initial_distances"):
        assert out[key].shape == (B, K) and out[key].dtype == torch.float64, key
    assert out["segment_lengths"].shape == (B, K, P - 1) and out["gradient"].shape == (B, K, P - 2, d)
    assert out["gradient_centre"].shape == (B, d)
    for key in ("accepted", "info"):
        assert out[key].shape == (B,) and out[key].dtype == torch.int32
    assert all(v.is_cuda for v in out.values())
    assert bool((out["energy"] <= out["initial_energy"]).all()) and bool((0 <= out["accepted"]).all())
    assert bool((out["accepted"] <= steps).all())
    assert torch.equal(out["mean_latent"], out["latents"][:, 0, -1]) and torch.equal(out["mean_head"], out["path_head"][:, 0, -1])
    assert bool((out["latents"][:, :, -1] == out["latents"][:, :1, -1]).all())                  # one centre
    return geo, out


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_mean_relaxes_the_star(name):
    g, meta, dens, head, x = build(name)
    xs = FR.star_inputs(x, name).contiguous()
    model, w_ref, ref0, ref = FR.reference_run(name)
    weights = torch.tensor(FR.WEIGHTS, dtype=torch.float64, device="cuda")
    N, B = FR.POINTS - 1, xs.shape[0]
    outs = [run_mean(dens, head, xs, weights, steps)[1] for steps in (0, 4, FR.STEPS)]
    start, end = outs[0], outs[-1]
    energies = torch.stack([o["energy"] for o in outs])
    assert bool((end["info"] == 0).all()) and bool((start["info"] == 0).all())
    assert bool((energies[1:] <= energies[:-1]).all())              # monotone in the number of steps: a prefix of the same loop
    assert torch.equal(start["energy"], start["initial_energy"]) and torch.equal(start["initial_energy"], end["initial_energy"])
    assert bool((start["accepted"] == 0).all())
    w_sum = sum(FR.WEIGHTS)
    for out in (start, end):                                         # L_k^2 <= N sum_i ||r_{k,i}||^2 to the rounding of the two sums
        seg2 = out["segment_lengths"] ** 2
        assert bool((out["distances"] ** 2 <= N * seg2.sum(2) * (1 + 4 * (N + 2) * 2.0 ** -53)).all())
        assert torch.equal(out["distances"], out["segment_lengths"].sum(2))
        assert torch.allclose(out["variance"] * w_sum, out["energy"], rtol=1e-14, atol=0)
    # the bounds come from the reference run alone
    xr = ref["path_head"].flatten(1, 2)                              # (B, K P, D) float64
    colsum = ref["jacobian"].abs().sum(3).flatten(1).max(1).values
    g_floor = 4e-5 * xr.abs().flatten(1).max(1).values * colsum * w_sum
    g_need = torch.maximum(10.0 * ref["gradient_max"], g_floor)
    e_tol = 2.0 * (2e-5 * xr.norm(dim=2).max(1).values) / ref["segment_lengths"].flatten(1).min(1).values
    gm, e_rel = end["gradient_max"].cpu(), (end["energy"].cpu() - ref["energy"]).abs() / ref["energy"]
    print(f"{name}: accepted {end['accepted'].tolist()} (reference {ref['accepted'].tolist()}); gradient_max / allowed in "
          f"[{float((gm / g_need).min()):.3e}, {float((gm / g_need).max()):.3e}] (fell by {float((start['gradient_max'].cpu() / gm).min()):.3g}"
          f" .. {float((start['gradient_max'].cpu() / gm).max()):.3g}); |E - E_ref| / E_ref / tolerance max {float((e_rel / e_tol).max()):.3e}; "
          f"energy gain {float((1 - end['energy'] / end['initial_energy']).max()):.3e}")
    assert bool((gm <= g_need).all())
    assert bool((e_rel <= e_tol).all())
    e0_rel = (start["energy"].cpu() - ref0["energy"]).abs() / ref0["energy"]
    x0 = ref0["path_head"].flatten(1, 2)
    assert bool((e0_rel <= 2.0 * (2e-5 * x0.norm(dim=2).max(1).values) / ref0["segment_lengths"].flatten(1).min(1).values).all())
    with torch.no_grad():
        assert torch.equal(end["path_head"].flatten(0, 2), head.flow_forward(end["latents"].flatten(0, 2)))


def test_zero_steps_return_the_weighted_latent_mean_and_straight_arms():
    import cmf_amd
    g, meta, dens, head, x = build("c2b_hepmass")
    xs = FR.star_inputs(x, "c2b_hepmass").contiguous()
    B, K, P = xs.shape[0], xs.shape[1], 6
    weights = torch.tensor(FR.WEIGHTS, dtype=torch.float64, device="cuda")
    _, out = run_mean(dens, head, xs, weights, 0, points=P)
    with torch.no_grad():
        zs = dens.extract_latent(xs.flatten(0, 1).clone(), earliest_latent=False).view(B, K, -1)
    z = out["latents"]
    assert torch.equal(z[:, :, 0], zs)
    centre = (weights[None, :, None] * zs.double()).sum(1) / weights.sum()
    assert float((out["mean_latent"].double() - centre).abs().max()) <= 4 * 2.0 ** -24 * float(zs.abs().max())
    tt = torch.arange(P, device="cuda", dtype=torch.float64) / (P - 1)
    zc = out["mean_latent"].double()
    line = zs.double()[:, :, None] + tt[None, None, :, None] * (zc[:, None] - zs.double())[:, :, None]
    assert float((z.double() - line).abs().max()) <= 8 * 2.0 ** -24 * float(line.abs().max())
    assert torch.equal(out["energy"], out["initial_energy"]) and torch.equal(out["distances"], out["initial_distances"])
    geo = cmf_amd.ManifoldGeodesic(dens, points=P)
    same = geo.mean_latents(zs, weights.float().expand(B, K), steps=0)          # (B, K) float32 weights: used as given
    assert all(torch.equal(same[k], out[k]) for k in out)
    ones = geo.mean_latents(zs, steps=0)                                        # the default: all ones
    assert float((ones["mean_latent"].double() - zs.double().mean(1)).abs().max()) <= 4 * 2.0 ** -24 * float(zs.abs().max())
    assert torch.allclose(ones["variance"] * K, ones["energy"], rtol=1e-14, atol=0)


def test_copies_of_one_input_cost_exactly_zero():
    g, meta, dens, head, x = build("c2a_power")
    xs = x[:3, None].expand(3, 3, *x.shape[1:]).contiguous()
    weights = torch.tensor(FR.WEIGHTS, dtype=torch.float64, device="cuda")
    for steps in (0, 3):
        _, out = run_mean(dens, head, xs, weights, steps, points=5)
        assert bool((out["info"] == 0).all()) and bool((out["accepted"] == 0).all())
        for key in ("energy", "initial_energy", "variance", "distances", "initial_distances", "gradient_max", "gradient",
                    "gradient_centre", "segment_lengths"):
            assert bool((out[key] == 0).all()), key
        assert torch.equal(out["mean_latent"], out["latents"][:, 0, 0])


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_sub_batches_give_the_stars_of_one_call(name, monkeypatch):
    import cmf_amd
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    K, P = 2, 4
    xs = torch.stack([x[[0, 1, 2]], x[[1, 2, 0]]], 1).contiguous()              # three stars of two inputs
    weights = torch.tensor([1.0, 2.0], dtype=torch.float64, device="cuda")
    _, whole = run_mean(dens, head, xs, weights, 6, points=P)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * K * P * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3 * K * P) // (K * P) == 1             # 3 stars run as three sub-batches of one star
    _, pieces = run_mean(dens, head, xs, weights, 6, points=P)
    e0 = whole["initial_energy"]
    print(f"{name}: pieces against whole: bit-equal latents {torch.equal(pieces['latents'], whole['latents'])}, energy rel "
          f"{float(((pieces['energy'] - whole['energy']).abs() / e0).max()):.2e}")
    assert float(((pieces["initial_energy"] - e0).abs() / e0).max()) <= 1e-5
    assert float(((pieces["energy"] - whole["energy"]).abs() / e0).max()) <= 1e-5
    assert bool((pieces["info"] == 0).all()) and pieces["latents"].shape == whole["latents"].shape
    # a star that does not fit one sub-batch
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    with pytest.raises(ValueError, match="points.*inputs"):
        cmf_amd.ManifoldGeodesic(dens, points=P).mean(xs, weights)


def test_the_log_density_path_is_untouched():
    import cmf_amd
    g, meta, dens, head, x = build("mini_mnist")
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        marker = head.last_gram
        cmf_amd.ManifoldGeodesic(dens, points=4, steps=2).mean(x[None, :3].contiguous())
        assert head.last_gram is marker
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
