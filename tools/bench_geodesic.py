#!/usr/bin/env python3
"""Cost of the manifold geodesics: the cross-Gram, curve step and energy-only launches beside one Gram + Cholesky
launch at the head's shapes, one ``ManifoldGeodesic.connect(x0, x1, steps=4)`` against as many ``elbo`` calls as it makes tangent
sweeps on the full-size C3 model, and the ratios the product reaches on the fixtures against the float64 reference loop.

    python tools/bench_geodesic.py [--reps 20] [--evals 6] [--out profiles/geodesic.txt]

Kernel: seeded random panel-layout Jacobian stacks at 32 curves x 16 points with d = 64, D = 784 (C3) and 16 x 16 with d = 128,
D = 3072 (C5), their Gram matrices through ``engine.gram_cholesky(T, d, 1)``, a noisy straight line as x_hat, damping 1e-3; HIP
events around one launch (the output and workspace allocations are inside the bracket, served by the caching allocator after the
warm-up), median of --reps.  End to end: full-size C3 (recipe seed 0), 32 curves of 16 points between seeded inputs past the
dequantisation wrapper, host clock around work that ends in a synchronise, alternated, medians of --evals; the tangent sweep of
one iteration (``decode(z, tangents=True)`` on the 512 points) by HIP events in the same process.  Fixtures: the curves and bounds
of tests/test_gpu_geodesic.py.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--evals", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_geodesic needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    med = statistics.median
    emit(f"# cross-Gram launch (cmf_cross_gram: J_i^T J_i+1 by fp32 MFMA, one workgroup per pair), curve step launch (cmf_curve_step: "
         f"gradient and the float64 block tridiagonal solve, one workgroup per curve) and its energy-only mode beside the Gram + "
         f"Cholesky launch (cmf_gram_cholesky, one attempt), HIP events, median of {a.reps}")
    kernel_ms = {}
    for label, curves, P, d, D in (("C3", 32, 16, 64, 784), ("C5", 16, 16, 128, 3072)):
        B, nc = curves * P, E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        tt = torch.linspace(0.0, 1.0, P)[None, :, None]
        xhat = (torch.randn(curves, 1, D, generator=gen) + tt * torch.randn(curves, 1, D, generator=gen)
                + 0.1 * torch.randn(curves, P, D, generator=gen)).reshape(B, D).cuda().contiguous()
        lam = torch.full((curves,), 1e-3, dtype=torch.float64, device="cuda")
        jtj = E.gram_cholesky(T, d, 1).jtj
        cross = E.cross_gram(T, d, P)
        gram = event_ms(lambda: E.gram_cholesky(T, d, 1), a.reps)
        cr = event_ms(lambda: E.cross_gram(T, d, P), a.reps)
        step = event_ms(lambda: E.curve_step(T, jtj, cross, xhat, P, lam), a.reps)
        en = event_ms(lambda: E.curve_energy(xhat, P), a.reps)
        info = E.curve_step(T, jtj, cross, xhat, P, lam).info.cpu()
        kernel_ms[label] = med(cr) + med(step) + med(en)
        emit(f"{label:3s} {curves} curves x {P} points, d = {d:3d} D = {D:4d}: cross_gram {med(cr) * 1e3:8.1f} us (min {min(cr) * 1e3:.1f}); "
             f"curve_step {med(step) * 1e3:9.1f} us (min {min(step) * 1e3:.1f}), info != 0: {int((info != 0).sum())}; energy-only "
             f"{med(en) * 1e3:6.1f} us (min {min(en) * 1e3:.1f}); gram_cholesky {med(gram) * 1e3:7.1f} us; cross_gram / gram_cholesky = "
             f"{med(cr) / med(gram):.2f}; the three new launches together {kernel_ms[label] * 1e3:.1f} us")
        del T

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    curves, P = 32, 16
    B = curves * P
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both sides see the same input
    geo = cmf_amd.ManifoldGeodesic(model, points=P, steps=4)
    xc = x.cuda()
    x0, x1 = xc[:curves].contiguous(), xc[curves:2 * curves].contiguous()
    last = {}

    def connect():
        last["out"] = geo.connect(x0, x1)

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

    runners = {"connect(steps=4)": connect, "5 x elbo": five_elbos}
    for fn in runners.values():
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    m = {which: med(t) for which, t in times.items()}
    emit(f"# C3 full size, {curves} curves x {P} points = {B} samples: one connect(x0, x1, steps=4) (5 tangent sweeps + 5 primal "
         f"decodes + 2 encodes of {curves}) against five elbo calls on {B} samples (5 tangent sweeps + 5 encodes), host clock, median "
         f"of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:17s} {m[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"connect / (5 x elbo) = {m['connect(steps=4)'] / m['5 x elbo']:.3f}")
    head, z = geo.head, last["out"]["latents"].reshape(B, -1).contiguous()
    with torch.no_grad(), E.scope(head.kernels):
        sweep = event_ms(lambda: head.program.decode(z, tangents=True), a.reps)
    emit(f"tangent sweep of one iteration (decode with all d columns, {B} points) {med(sweep):8.2f} ms (min {min(sweep):.2f}); the three "
         f"new launches at the C3 shapes above are {kernel_ms['C3'] / med(sweep) * 100:.2f} % of it")
    out = last["out"]
    e1, e0, l1, l0 = (out[k].cpu() for k in ("energy", "initial_energy", "length", "initial_length"))
    emit(f"# that call: energy / initial_energy in [{float((e1 / e0).min()):.4f}, {float((e1 / e0).max()):.4f}], length / initial_length "
         f"in [{float((l1 / l0).min()):.4f}, {float((l1 / l0).max()):.4f}], accepted {int(out['accepted'].min())} .. "
         f"{int(out['accepted'].max())}, info != 0: {int((out['info'] != 0).sum())}")

    import _geodesic_reference as R
    from test_gpu_geodesic import fixture_ends
    from test_gpu_metric_stats import build
    emit(f"# fixtures, {R.POINTS} points, {R.STEPS} steps, first half of the batch connected to the second: the product against the float64 "
         f"reference loop (allowed: max(10 x the reference's final max |g|, g_floor); tolerance: 2 (2e-5 max ||x||) / min ||r_i||)")
    for name in R.FIXTURES:
        g, meta, fd, fh, fx = build(name)
        f0, f1 = fixture_ends(name, fx)
        _, ref0, ref = R.reference_run(name)
        o = cmf_amd.ManifoldGeodesic(fd, points=R.POINTS, steps=R.STEPS).connect(f0, f1)
        o0 = cmf_amd.ManifoldGeodesic(fd, points=R.POINTS, steps=0).connect(f0, f1)
        xr = ref["path_head"]
        g_floor = 4e-5 * xr.abs().flatten(1).max(1).values * ref["jacobian"].abs().sum(2).flatten(1).max(1).values
        g_need = torch.maximum(10.0 * ref["gradient_max"], g_floor)
        e_tol = 2.0 * (2e-5 * xr.norm(dim=2).max(1).values) / ref["segment_lengths"].min(1).values
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
