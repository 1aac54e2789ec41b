"""Host-side checks of the Frechet means (no GPU): the numpy emulation of the star step kernels against float64 numpy on
the dense block-arrow system, against the curve step emulation on a two-arm star joined into one curve and on a known answer, its
info codes, the float64 reference loop on the fixtures -- the conditions tests/test_gpu_star.py asserts of the product are
established here on the reference alone -- and the refusals of the public API.

Bounds (u = 2^-53; the kernel's, the emulation is held to a quarter): ||A delta - g||_inf <= 96 d u (||A||_inf ||delta||_inf +
||g||_inf) on the dense ((K M + 1) d)^2 matrix -- the band's 64 with the centre as a third elimination level --; |g - g_ref| <=
2 (D + 4) u w_k sum |J| |s| at the arm points and 2 (D + K + 4) u sum_k w_k sum |J| |s| at the centre; seg2 to 2 (D + 2) u."""
import numpy as np
import pytest
import torch

import _curve_step_emulation as CE
import _frechet_reference as FR
import _star_step_emulation as SE
from test_geodesic_host import small_density

POINTS = [3, 4]
WEIGHTS = np.array([1.0, 2.0, 0.5, 3.0, 0.25])


def damping_family(D, d):
    """The dampings a shape is run at: D < d (a rank-deficient H) only with lambda > 0."""
    return [lam for lam in SE.DAMPINGS if D >= d or lam > 0.0]


def check_star(J, G, C, xhat, w, lam, P, out, bound_c, label):
    """One star's outputs (info 0; ``out``: a dict as _star_step_emulation.step returns) against float64 numpy on the same float32
    inputs; returns the reached fractions (residual, gradient, centre gradient) of their bounds."""
    K, (_, D, d) = len(w), J.shape
    M, N = P - 2, P - 1
    share = bound_c / SE.BOUND_C
    x = xhat.astype(np.float64).reshape(K, P, D)
    J64 = J.astype(np.float64).reshape(K, P, D, d)
    s = (x[:, :-2] + x[:, 2:]) - 2.0 * x[:, 1:-1]
    g_ref = w[:, None, None] * np.einsum("kir,kirc->kic", s, J64[:, 1:-1])
    g_abs = w[:, None, None] * np.einsum("kir,kirc->kic", np.abs(s), np.abs(J64[:, 1:-1]))
    g_err = np.abs(out["grad"] - g_ref)
    assert (g_err <= share * 2 * (D + 4) * SE.U * g_abs).all(), label
    sc = x[:, M] - x[:, N]
    c_ref = (w[:, None] * np.einsum("kr,krc->kc", sc, J64[:, N])).sum(0)
    c_abs = (w[:, None] * np.einsum("kr,krc->kc", np.abs(sc), np.abs(J64[:, N]))).sum(0)
    c_err = np.abs(out["grad_centre"] - c_ref)
    assert (c_err <= share * 2 * (D + K + 4) * SE.U * c_abs).all(), label
    r = x[:, 1:] - x[:, :-1]
    assert (np.abs(out["seg2"] - (r * r).sum(2)) <= 2 * (D + 2) * SE.U * (r * r).sum(2)).all(), label
    total = 0.0
    for k in range(K):
        arm = 0.0
        for v in out["seg2"][k]:
            arm += float(v)
        total += w[k] * arm
    stats = out["stats"]
    assert stats[0] == total and stats[3] == max(np.abs(out["grad"]).max(), np.abs(out["grad_centre"]).max()), label
    A, H = SE.dense(G, C, w, lam, P)
    gv, dv = SE.unknowns(out["grad"], out["grad_centre"]), SE.unknowns(out["delta"], out["delta_centre"])
    ratio = CE.residual_ratio(A, d, gv, dv)
    assert ratio <= bound_c, label
    n = len(gv)
    assert abs(stats[1] - gv @ dv) <= 2 * (n + K + 2) * SE.U * np.abs(gv * dv).sum(), label
    assert abs(stats[2] - dv @ H @ dv) <= 2 * (n + K + 2) * SE.U * np.abs(H * np.outer(dv, dv)).sum(), label
    tiny = 1e-300
    return ratio / bound_c, float((g_err / np.maximum(2 * (D + 4) * SE.U * g_abs, tiny)).max()), \
        float((c_err / np.maximum(2 * (D + K + 4) * SE.U * c_abs, tiny)).max())


@pytest.mark.parametrize("d", SE.WIDTHS)
@pytest.mark.parametrize("D", SE.ROWS)
def test_emulation_solves_the_block_arrow_system(D, d):
    lams = damping_family(D, d)
    worst = np.zeros(3)
    for P in POINTS:
        for K in SE.ARMS:
            J, G, C, xhat = SE.inputs(len(lams), K, P, D, d)
            w = np.tile(WEIGHTS[:K], (len(lams), 1))
            out = SE.batch(J, G, C, xhat, w, np.array(lams), P)
            assert (out["info"] == 0).all()
            n = K * P
            for s, lam in enumerate(lams):
                one = {key: v[s] for key, v in out.items()}
                worst = np.maximum(worst, check_star(J[s * n:(s + 1) * n], G[s * n:(s + 1) * n], C[s * n:], xhat[s * n:(s + 1) * n],
                                                     w[s], lam, P, one, SE.BOUND_C / 4, f"P {P} K {K} star {s}"))
                for k in range(K):                                   # seg2: the curve emulation's energy-only mode on the arm
                    rows = slice(s * n + k * P, s * n + (k + 1) * P)
                    assert np.array_equal(CE.energy(xhat[rows], P)[0], out["seg2"][s, k])
    print(f"D={D} d={d}: reached fractions of the bounds: residual {worst[0]:.4f} (of {SE.BOUND_C / 4:g} d u), gradient {worst[1]:.3f}, "
          f"centre gradient {worst[2]:.3f}")


@pytest.mark.parametrize("P,D,d", [(3, 5, 3), (4, 64, 17), (4, 64, 16), (3, 784, 64), (4, 784, 100), (3, 64, 128)])
def test_two_equal_arms_are_the_joined_curve(P, D, d):
    """K = 2 with equal weights is curve_step's problem on the joined curve of 2 P - 1 points (arm 1 reversed, the centre its middle
    interior point): the two eliminations differ only by rounding, so the star's step satisfies the curve's system to the residual
    bound, with the curve emulation's own gradient as right-hand side."""
    for lam in damping_family(D, d):
        J, G, C, xhat = SE.inputs(1, 2, P, D, d, seed=6)
        star = SE.step(J, G, C, xhat, np.ones(2), lam, P)
        grad, delta, stats, seg2, info = CE.step(*SE.joined(J, G, C, xhat, P), lam)
        assert star["info"] == 0 and info == 0
        Jj, Gj, Cj, _ = SE.joined(J, G, C, xhat, P)
        A, _ = CE.dense(Gj, Cj, lam)
        as_curve = np.concatenate([star["delta"][0], star["delta_centre"][None], star["delta"][1][::-1]])
        ratio = CE.residual_ratio(A, d, grad, as_curve)
        scale = np.abs(delta).max()
        print(f"P={P} D={D} d={d} lambda={lam:g}: residual of the star's step in the curve's system {ratio:.4f} (bound {SE.BOUND_C / 4:g} d u); "
              f"max |delta_star - delta_curve| / max |delta| = {float(np.abs(as_curve - delta).max() / scale):.2e}")
        assert ratio <= SE.BOUND_C / 4
        assert abs(star["stats"][0] - stats[0]) <= 4 * SE.U * stats[0]
        assert np.array_equal(np.concatenate([star["seg2"][0], star["seg2"][1][::-1]]), seg2)


def known_answer(K, P, D, d, seed):
    """Every point of the star has the same Jacobian J (small integers: J^T J is exact in float32) and xhat = float32(J z + c) for
    scattered z (the K centre copies share one z): one undamped step must put the centre at sum_k w_k z_k0 / sum_k w_k and every arm
    on the evenly spaced points of its straight line.  Returns (J, G, C, xhat, w, z (K, P, d), target (K, P, d), tol): tol bounds
    |z + delta - target| by the float32 rounding e of xhat carried through the weighted least-squares solve -- ||K^+|| ||sqrt(W) D
    e||_2 with K = sqrt(W) T (x) J, T the K N x (K M + 1) difference matrix of the star, ||D e||_2 <= 2 sqrt(sum ||e_i||^2), |e_i| <=
    2^-24 |xhat_i| -- plus the float64 solve's own residual bound carried through A^-1."""
    rng = np.random.default_rng(7919 * d + 13 * D + 101 * K + P + seed)
    M, N = P - 2, P - 1
    J1 = rng.integers(-2, 3, size=(D, d)).astype(np.float32)
    J1[np.arange(d) % D, np.arange(d)] += 3.0                        # keep every column away from zero
    w = WEIGHTS[:K].copy()
    z = rng.standard_normal((K, P, d))
    z[:, 1:] += 0.5 * rng.standard_normal((K, N, d))
    z[:, N] = z[0, N]
    x64 = z @ J1.astype(np.float64).T + rng.standard_normal(D)
    xhat = x64.astype(np.float32).reshape(K * P, D)
    G1 = J1.astype(np.float64).T @ J1.astype(np.float64)
    assert np.array_equal(G1.astype(np.float32).astype(np.float64), G1)
    J = np.broadcast_to(J1, (K * P, D, d)).copy()
    G = np.broadcast_to(G1.astype(np.float32), (K * P, d, d)).copy()
    C = np.broadcast_to(G1.astype(np.float32), (K * P - 1, d, d)).copy()
    centre = (w[:, None] * z[:, 0]).sum(0) / w.sum()
    target = z[:, :1] + np.linspace(0.0, 1.0, P)[None, :, None] * (centre - z[:, 0])[:, None, :]
    T = np.zeros((K * N, K * M + 1))
    for k in range(K):
        for i in range(N):                                           # segment i of arm k: point i + 1 minus point i
            for point, sign in ((i + 1, 1.0), (i, -1.0)):
                if point > 0:
                    T[k * N + i, K * M if point == N else k * M + point - 1] = sign * np.sqrt(w[k])
    sigma_t = np.linalg.svd(T, compute_uv=False)[-1]
    sigma_j = np.linalg.svd(J1.astype(np.float64), compute_uv=False)[-1]
    rounding = 2.0 * 2.0 ** -24 * np.sqrt(w.max() * (xhat.astype(np.float64) ** 2).sum()) / (sigma_t * sigma_j)
    A, _ = SE.dense(G, C, w, 0.0, P)
    move = np.abs(target - z).max()
    solve = 2.0 * SE.BOUND_C * d * SE.U * np.linalg.cond(A, np.inf) * move
    return J, G, C, xhat, w, z, target, rounding + solve


#: (K, P, D, d, 40 x the error the emulation reaches, rounded up to one digit): the asserted tolerance is the smaller of this and
#: of the computed bound of ``known_answer``
KNOWN = [(1, 3, 5, 3, 3e-6), (2, 4, 64, 17, 2e-6), (3, 3, 64, 16, 3e-6), (3, 4, 784, 64, 2e-6), (5, 3, 784, 100, 2e-6),
         (3, 3, 784, 128, 3e-6)]


def known_answer_error(out, z, target):
    M = z.shape[1] - 2
    arms = np.abs(z[:, 1:M + 1] + out["delta"] - target[:, 1:M + 1]).max()
    return max(float(arms), float(np.abs(z[0, -1] + out["delta_centre"] - target[0, -1]).max()))


@pytest.mark.parametrize("K,P,D,d,fixed", KNOWN)
def test_emulation_finds_the_known_answer(K, P, D, d, fixed):
    J, G, C, xhat, w, z, target, tol = known_answer(K, P, D, d, seed=0)
    tol = min(tol, fixed)
    out = SE.step(J, G, C, xhat, w, 0.0, P)
    assert out["info"] == 0
    err = known_answer_error(out, z, target)
    print(f"K={K} P={P} D={D} d={d}: max |z + delta - target| = {err:.3e} (tolerance {tol:.3e}; the step itself {np.abs(target - z).max():.3e})")
    assert err <= tol < 1e-3 * np.abs(target - z).max()


def test_emulation_info_codes():
    K, P, D, d = 3, 4, 64, 5
    n = K * P
    J, G, C, xhat = SE.inputs(3, K, P, D, d, seed=1)
    w, lam = np.tile(WEIGHTS[:K], (3, 1)), np.zeros(3)
    clean = SE.batch(J, G, C, xhat, w, lam, P)
    assert clean["info"].tolist() == [0, 0, 0]
    values = ("grad", "grad_centre", "delta", "delta_centre", "seg2", "stats")

    def regram(Jz):
        J64 = Jz.astype(np.float64)
        return (J64.transpose(0, 2, 1) @ J64).astype(np.float32), SE.cross_of(Jz).astype(np.float32)

    def confined(out):
        return all(np.array_equal(out[key][[0, 2]], clean[key][[0, 2]]) for key in values)

    # an all-zero Jacobian column at an interior point of arm 1 of star 1, or at every copy of its centre: a pivot is exactly 0
    for rows in ([n + P + 2], [n + k * P + P - 1 for k in range(K)]):
        Jz = J.copy()
        Jz[rows, :, 3] = 0.0
        Gz, Cz = regram(Jz)
        for value in SE.DAMPINGS:
            base = SE.batch(J, G, C, xhat, w, np.full(3, value), P)
            out = SE.batch(Jz, Gz, Cz, xhat, w, np.full(3, value), P)
            assert out["info"].tolist() == [0, 1, 0]
            assert np.isnan(out["delta"][1]).all() and np.isnan(out["delta_centre"][1]).all() and np.isnan(out["stats"][1, 1:3]).all()
            assert np.isfinite(out["grad"][1]).all() and np.isfinite(out["grad_centre"][1]).all()
            assert np.isfinite(out["stats"][1, [0, 3]]).all() and np.array_equal(out["seg2"], base["seg2"])
            assert all(np.array_equal(out[key][[0, 2]], base[key][[0, 2]]) for key in values)
    # every place a non-finite value may sit; with a failing pivot in another arm of the same star, code 2 takes precedence
    Jz = J.copy()
    Jz[n + 2, :, 3] = 0.0                                            # arm 0 of star 1
    Gz, Cz = regram(Jz)
    for where in ("xhat", "xhat_end", "J", "J_centre", "G", "G_centre", "C", "weight"):
        for Jb, Gb, Cb in ((J, G, C), (Jz, Gz, Cz)):
            Jn, Gn, Cn, hn, wn = Jb.copy(), Gb.copy(), Cb.copy(), xhat.copy(), w.copy()
            if where == "xhat":
                hn[n + P + 1, 0] = np.nan
            elif where == "xhat_end":
                hn[n + 2 * P, 3] = np.inf                            # the fixed end of arm 2
            elif where == "J":
                Jn[n + P + 2, 3, 4] = np.nan
            elif where == "J_centre":
                Jn[n + 2 * P - 1, 3, 4] = np.nan
            elif where == "G":
                Gn[n + P + 1, 4, 2] = np.nan
            elif where == "G_centre":
                Gn[n + 3 * P - 1, 4, 2] = np.nan
            elif where == "C":
                Cn[n + P + 2, 2, 4] = np.nan                         # the pair (M, N) of arm 1
            else:
                wn[1, 2] = np.inf
            out = SE.batch(Jn, Gn, Cn, hn, wn, lam, P)
            assert out["info"].tolist() == [0, 2, 0], where
            assert all(np.isnan(out[key][1]).all() for key in values), where
            assert confined(out), where
    # never read: the fixed ends' Jacobians and jtj, the upper triangles, the cross blocks of the fixed ends and between two arms
    Jn, Gn, Cn = J.copy(), G.copy(), C.copy()
    for k in range(K):
        Jn[n + k * P] = np.nan
        Gn[n + k * P] = np.nan
        Cn[n + k * P] = np.nan
        Cn[n + k * P + P - 1] = np.nan
    Gn[n + 1, 2, 4] = np.nan
    out = SE.batch(Jn, Gn, Cn, xhat, w, lam, P)
    assert all(np.array_equal(out[key], clean[key]) for key in values) and out["info"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_reference_loop_finds_the_mean(name):
    model, w, start, end = FR.reference_run(name)
    N = FR.POINTS - 1
    fall = start["gradient_max"] / end["gradient_max"]
    gain = 1.0 - end["energy"] / end["initial_energy"]
    print(f"{name}: accepted {end['accepted'].tolist()}; max |gradient| fell by {float(fall.min()):.3g} .. {float(fall.max()):.3g}; "
          f"energy gain {float(gain.min()):.3e} .. {float(gain.max()):.3e}; variance {end['variance'].tolist()}")
    assert bool((end["info"] == 0).all()) and bool((start["info"] == 0).all())
    assert bool((end["energies"][1:] <= end["energies"][:-1]).all()) and bool((end["energy"] <= end["initial_energy"]).all())
    assert torch.equal(end["energies"][0], end["initial_energy"]) and torch.equal(end["energies"][-1], end["energy"])
    assert torch.equal(start["energy"], start["initial_energy"]) and torch.equal(start["initial_energy"], end["initial_energy"])
    assert bool((start["accepted"] == 0).all()) and bool((end["accepted"] <= FR.STEPS).all())
    for out in (start, end):                                         # L_k^2 <= N sum_i ||r_{k,i}||^2 per arm
        assert bool((out["distances"] ** 2 <= N * (out["segment_lengths"] ** 2).sum(2) * (1 + 1e-12)).all())
        assert torch.allclose(out["energy"], N * FR.arm_sum(w, (out["segment_lengths"] ** 2).sum(2)), rtol=1e-13, atol=0)
        assert torch.allclose(out["variance"] * sum(FR.WEIGHTS), out["energy"], rtol=1e-14, atol=0)
    assert bool((end["gradient_max"] * 1e6 <= start["gradient_max"]).all())
    assert torch.equal(end["latents"][:, :, 0], start["latents"][:, :, 0])                       # the inputs stay
    assert bool((end["latents"][:, :, -1] == end["latents"][:, :1, -1]).all())                  # one centre


def test_api_refusals():
    import cmf_amd
    from cmf_amd import engine as E
    assert E.STAR_MAX_ARMS == 64
    dens = small_density()
    geo = cmf_amd.ManifoldGeodesic(dens, points=5)
    d = geo.head.program.d
    zs = torch.zeros(2, 3, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.mean(torch.zeros(2, 3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.mean_latents(zs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geo.mean_latents(zs, weights=torch.tensor([1.0, 2.0, 0.5]))
    for bad in (torch.zeros(2, 6), torch.zeros(0, 3, 6), torch.zeros(2, 0, 6)):
        with pytest.raises(ValueError, match="xs|at least one"):
            geo.mean(bad)
    for bad in (torch.zeros(2, d), torch.zeros(2, 3, d + 1), torch.zeros(2, 3, d, dtype=torch.float64), torch.zeros(2, 3, 1, d)):
        with pytest.raises(ValueError, match="zs must be"):
            geo.mean_latents(bad)
    for bad in (torch.zeros(0, 3, d), torch.zeros(2, 0, d), torch.zeros(2, 65, d)):
        with pytest.raises(ValueError, match="at least one group"):
            geo.mean_latents(bad)
    with pytest.raises(ValueError, match="steps >= 0"):
        geo.mean_latents(zs, steps=-1)
    for bad in (torch.ones(2), torch.ones(3, 2), torch.ones(2, 3, 1), torch.ones(3, dtype=torch.int64), [1.0, 2.0, 0.5]):
        with pytest.raises(ValueError, match="weights must be a floating point tensor"):
            geo.mean_latents(zs, weights=bad)
    for value in (0.0, -1.0, float("inf"), float("nan")):
        for shape in ((3,), (2, 3)):
            bad = torch.ones(shape)
            bad[..., 1] = value
            with pytest.raises(ValueError, match="finite and > 0"):
                geo.mean_latents(zs, weights=bad)
    # the engine
    w, lam = torch.ones(2, 2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    args = (E.Tangent(12, 6, 16, "panel", "cpu"), torch.zeros(12, 2, 2), torch.zeros(11, 2, 2), torch.zeros(12, 6), 3, 2, w, lam)
    with pytest.raises(ValueError, match="GPU"):
        E.star_step(*args)
    for arms in (0, 65):
        with pytest.raises(ValueError, match="1 <= arms <= 64"):
            E.star_step(*args[:5], arms, w, lam)
    # wider than the star kernels' window
    wide = small_density("mnist", latent_dimension=130)
    with pytest.raises(ValueError, match="1 <= latent_dimension <= 128"):
        cmf_amd.ManifoldGeodesic(wide)
