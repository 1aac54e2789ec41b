#!/usr/bin/env python3
"""Cost of the Frechet means: the three launches of ``cmf_star_step`` beside ``cmf_curve_step`` at the same total
point count and beside one ``cmf_metric_solve`` per star, one ``ManifoldGeodesic.mean(xs, steps=4)`` against as many ``elbo`` calls
as it makes tangent sweeps on the full-size C3 model, and the ratios the product reaches on the fixtures against the float64
reference loop.

    python tools/bench_star.py [--reps 20] [--evals 6] [--out profiles/star.txt]

Kernel: seeded random panel-layout Jacobian stacks at 8 stars x 4 arms x 16 points with d = 64, D = 784 (C3) and 4 x 4 x 16 with
d = 128, D = 3072 (C5), their Gram matrices through ``engine.gram_cholesky(T, d, 1)``, the cross-Gram blocks of neighbouring samples
through ``engine.star_cross_gram``, a noisy straight line per arm as x_hat, weights 1, 2, 0.5, 3, damping 1e-3; HIP events around the C
entry alone (outputs and workspace allocated once), median of --reps.  End to end: full-size C3 (recipe seed 0), 8 stars of 4
seeded inputs with 16 points per arm past the dequantisation wrapper, host clock around work that ends in a synchronise,
alternated, medians of --evals.  Fixtures: the stars and bounds of tests/test_gpu_star.py.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_geodesic import event_ms                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--evals", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import _lib
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_star needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    med = statistics.median
    lib = _lib.load()
    emit(f"# the three launches of cmf_star_step (per arm forward, per star the centre, per arm backward) beside cmf_curve_step on the "
         f"arms as curves (the same total point count) and cmf_metric_solve on one matrix per star, HIP events, median of {a.reps}")
    for label, stars, K, P, d, D in (("C3", 8, 4, 16, 64, 784), ("C5", 4, 4, 16, 128, 3072)):
        n, nc = stars * K * P, E.ceil16(d)
        T = E.Tangent(n, D, nc, "panel", "cuda", data=(torch.randn(n * D * nc, generator=gen) / D ** 0.5).cuda())
        tt = torch.linspace(0.0, 1.0, P)[None, :, None]
        xhat = (torch.randn(stars * K, 1, D, generator=gen) + tt * torch.randn(stars * K, 1, D, generator=gen)
                + 0.1 * torch.randn(stars * K, P, D, generator=gen)).reshape(n, D).cuda().contiguous()
        lam = torch.full((stars,), 1e-3, dtype=torch.float64, device="cuda")
        w = torch.tensor([1.0, 2.0, 0.5, 3.0], dtype=torch.float64, device="cuda").expand(stars, K).contiguous()
        jtj = E.gram_cholesky(T, d, 1).jtj
        cross = E.star_cross_gram(T, d)
        r = E.star_step(T, jtj, cross, xhat, P, K, w, lam)
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
        need = lib.cmf_star_step_ws(d, P, K, stars)
        ws, arm = f64(need), f64(stars, K, 4)

        def entry():
            _lib.check(lib.cmf_star_step(E._p(T.data), T.t_b, T.t_r, D, nc, d, P, K, stars, 0, E._p(jtj), E._p(cross), E._p(xhat), E._p(w),
                                         E._p(lam), E._p(r.grad), E._p(r.grad_centre), E._p(r.delta), E._p(r.delta_centre), E._p(arm),
                                         E._p(r.seg2), E._p(r.info), E._p(ws), need, E._stream()), "cmf_star_step")

        star = event_ms(entry, a.reps)
        cr = event_ms(lambda: E.star_cross_gram(T, d), a.reps)
        whole = event_ms(lambda: E.star_step(T, jtj, cross, xhat, P, K, w, lam), a.reps)
        lam_c = torch.full((stars * K,), 1e-3, dtype=torch.float64, device="cuda")
        cross_c = E.cross_gram(T, d, P)
        curve = event_ms(lambda: E.curve_step(T, jtj, cross_c, xhat, P, lam_c), a.reps)
        rhs = torch.randn(stars, d, generator=gen).double().cuda()
        solve = event_ms(lambda: E.metric_solve(jtj[:stars].contiguous(), rhs), a.reps)
        info = r.info.cpu()
        emit(f"{label:3s} {stars} stars x {K} arms x {P} points, d = {d:3d} D = {D:4d}: cmf_star_step {med(star) * 1e3:9.1f} us (min "
             f"{min(star) * 1e3:.1f}), info != 0: {int((info != 0).sum())}; engine.star_step with its sums over the arms "
             f"{med(whole) * 1e3:9.1f} us; cmf_curve_step on {stars * K} curves {med(curve) * 1e3:9.1f} us (min {min(curve) * 1e3:.1f}); "
             f"cmf_metric_solve on {stars} matrices {med(solve) * 1e3:7.1f} us; star_cross_gram {med(cr) * 1e3:7.1f} us; star_step / curve_step = {med(star) / med(curve):.3f}, "
             f"(star_step - curve_step) / metric_solve = {(med(star) - med(curve)) / med(solve):.2f}")
        del T

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    stars, K, P = 8, 4, 16
    B = stars * K * P
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both sides see the same input
    geo = cmf_amd.ManifoldGeodesic(model, points=P, steps=4)
    xc = x.cuda()
    xs = xc[:stars * K].view(stars, K, 1, 28, 28).contiguous()
    last = {}

    def mean():
        last["out"] = geo.mean(xs)

    def five_elbos():
        for _ in range(5):
            model.elbo(xc, add_reconstruction=True)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    runners = {"mean(steps=4)": mean, "5 x elbo": five_elbos}
    for fn in runners.values():
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    m = {which: med(t) for which, t in times.items()}
    emit(f"# C3 full size, {stars} stars x {K} inputs x {P} points = {B} samples: one mean(xs, steps=4) (5 tangent sweeps + 5 "
         f"primal decodes + 1 encode of {stars * K}) against five elbo calls on {B} samples (5 tangent sweeps + 5 encodes), "
         f"host clock, median of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:14s} {m[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"mean / (5 x elbo) = {m['mean(steps=4)'] / m['5 x elbo']:.3f}")
    out = last["out"]
    e1, e0 = out["energy"].cpu(), out["initial_energy"].cpu()
    l1, l0 = out["distances"].cpu(), out["initial_distances"].cpu()
    emit(f"# that call: energy / initial_energy in [{float((e1 / e0).min()):.4f}, {float((e1 / e0).max()):.4f}], distances / "
         f"initial_distances in [{float((l1 / l0).min()):.4f}, {float((l1 / l0).max()):.4f}], accepted {int(out['accepted'].min())} .. "
         f"{int(out['accepted'].max())}, info != 0: {int((out['info'] != 0).sum())}")

    import _frechet_reference as FR
    from test_gpu_metric_stats import build
    emit(f"# fixtures, {FR.ARMS} inputs per star with weights {FR.WEIGHTS}, {FR.POINTS} points per arm, {FR.STEPS} steps: the product "
         f"against the float64 reference loop (allowed: max(10 x the reference's final max |g|, g_floor); tolerance: 2 (2e-5 max ||x||) "
         f"/ min ||r_i||)")
    weights = torch.tensor(FR.WEIGHTS, dtype=torch.float64, device="cuda")
    for name in FR.FIXTURES:
        g, meta, fd, fh, fx = build(name)
        fxs = FR.star_inputs(fx, name).contiguous()
        _, _, ref0, ref = FR.reference_run(name)
        o = cmf_amd.ManifoldGeodesic(fd, points=FR.POINTS, steps=FR.STEPS).mean(fxs, weights)
        o0 = cmf_amd.ManifoldGeodesic(fd, points=FR.POINTS, steps=0).mean(fxs, weights)
        xr = ref["path_head"].flatten(1, 2)
        g_floor = 4e-5 * xr.abs().flatten(1).max(1).values * ref["jacobian"].abs().sum(3).flatten(1).max(1).values * sum(FR.WEIGHTS)
        g_need = torch.maximum(10.0 * ref["gradient_max"], g_floor)
        e_tol = 2.0 * (2e-5 * xr.norm(dim=2).max(1).values) / ref["segment_lengths"].flatten(1).min(1).values
        gm = o["gradient_max"].cpu()
        e_rel = (o["energy"].cpu() - ref["energy"]).abs() / ref["energy"]
        fall = o0["gradient_max"].cpu() / gm
        gain = 1 - o["energy"].cpu() / o["initial_energy"].cpu()
        emit(f"{name:12s} max |g| / allowed in [{float((gm / g_need).min()):.3e}, {float((gm / g_need).max()):.3e}]; max |g| fell by "
             f"{float(fall.min()):.3g} .. {float(fall.max()):.3g} (reference {float((ref0['gradient_max'] / ref['gradient_max']).min()):.3g} .. "
             f"{float((ref0['gradient_max'] / ref['gradient_max']).max()):.3g}); |E - E_ref| / E_ref / tolerance <= "
             f"{float((e_rel / e_tol).max()):.3e}; energy gain {float(gain.min()):.3e} .. {float(gain.max()):.3e}; accepted "
             f"{int(o['accepted'].min())} .. {int(o['accepted'].max())}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
