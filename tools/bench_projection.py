#!/usr/bin/env python3
"""Cost of the manifold projection: the Gauss-Newton step launch and its residual-only mode beside the Gram +
Cholesky launch at the head's shapes, one ``ManifoldProjector.project(x, steps=4)`` against four ``elbo`` calls on the full-size
C3 model, and the excess over the known answer the projection reaches on the fixtures.

    python tools/bench_projection.py [--reps 20] [--evals 6] [--out profiles/projection.txt]

Kernel: seeded random panel-layout Jacobian stacks at C3 (B = 512, d = 64, D = 784) and C5 (B = 256, d = 128, D = 3072), their Gram
matrices through ``engine.gram_cholesky(T, d, 1)``, random x and x_hat, damping 1e-3; HIP events around one launch (the output
allocations are inside the bracket, served by the caching allocator after the warm-up), median of --reps.  End to end: full-size
C3 (recipe seed 0), B = 512 seeded inputs past the dequantisation wrapper, host clock around work that ends in a synchronise,
alternated, medians of --evals.  Known answer: the construction of tests/test_gpu_projection.py on the small fixtures.  Fails
without a GPU."""
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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_projection needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# step launch (cmf_gauss_newton_step: J^T r and the float64 normal-equation solve, one workgroup per sample) and its "
         f"residual-only mode beside the Gram + Cholesky launch (cmf_gram_cholesky, one attempt), HIP events, median of {a.reps}")
    for label, B, d, D in (("C3", 512, 64, 784), ("C5", 256, 128, 3072)):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        x, xhat = torch.randn(B, D, generator=gen).cuda(), torch.randn(B, D, generator=gen).cuda()
        lam = torch.full((B,), 1e-3, dtype=torch.float64, device="cuda")
        jtj = E.gram_cholesky(T, d, 1).jtj
        m_gram = statistics.median(event_ms(lambda: E.gram_cholesky(T, d, 1), a.reps))
        step = event_ms(lambda: E.gauss_newton_step(T, jtj, x, xhat, lam), a.reps)
        res = event_ms(lambda: E.residual_sqnorm(x, xhat), a.reps)
        info = E.gauss_newton_step(T, jtj, x, xhat, lam).info.cpu()
        m_step, m_res = statistics.median(step), statistics.median(res)
        gb = 4.0 * B * D * nc / 1e9
        emit(f"{label:3s} B = {B:3d} d = {d:3d} D = {D:4d}: step {m_step * 1e3:8.1f} us (min {min(step) * 1e3:.1f}; {gb / m_step * 1e3:.0f} GB/s of "
             f"the {gb * 1e3:.0f} MB of J), info != 0: {int((info != 0).sum())}; residual-only {m_res * 1e3:6.1f} us (min "
             f"{min(res) * 1e3:.1f}); gram_cholesky {m_gram * 1e3:7.1f} us; step / gram_cholesky = {m_step / m_gram:.2f}")
        del T

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    B = a.batch
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both sides see the same input
    proj = cmf_amd.ManifoldProjector(model, steps=4)
    xc = x.cuda()
    last = {}

    def project():
        last["out"] = proj.project(xc)

    def four_elbos():
        for _ in range(4):
            model.elbo(xc, add_reconstruction=True)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    runners = {"project(steps=4)": project, "4 x elbo": four_elbos}
    for fn in runners.values():
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    med = {which: statistics.median(t) for which, t in times.items()}
    emit(f"# C3 full size, B = {B}: one project(x, steps=4) (5 tangent sweeps + 5 primal decodes + 1 encode) against four elbo calls "
         f"(4 tangent sweeps + 4 encodes), host clock, median of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:17s} {med[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"project / (4 x elbo) = {med['project(steps=4)'] / med['4 x elbo']:.3f}")
    out = last["out"]
    d2, d0, tang = out["distance2"].cpu(), out["initial_distance2"].cpu(), out["tangential2"].cpu()
    emit(f"# that projection: distance2 / initial_distance2 in [{float((d2 / d0).min()):.4f}, {float((d2 / d0).max()):.4f}], accepted "
         f"{int(out['accepted'].min())} .. {int(out['accepted'].max())}, max tangential2 / distance2 {float((tang / d2).max()):.3e}, "
         f"info != 0: {int((out['info'] != 0).sum())}")

    import _projection_reference as R
    from test_gpu_metric_stats import build
    emit("# known answer (y = g(z_0) + 0.1 ||g(z_0)|| n, n normal to range(J(z_0)), rho^2 = ||float32(y) - g(z_0)||^2), ten steps")
    for name in ("c2b_hepmass", "c2a_power", "mini_mnist"):
        g, meta, fd, head, fx = build(name)
        with torch.no_grad():
            z0 = fd.extract_latent(fx.clone(), earliest_latent=False)
            x_on, J = head.jacobian(z0)
        y = R.normal_offset(x_on.cpu(), J.cpu(), seed=0)[0].float()
        rho2 = ((y.double() - x_on.cpu().double()).flatten(1) ** 2).sum(1)
        o = cmf_amd.ManifoldProjector(head, steps=10).project(y.cuda().contiguous())
        e0, e1 = o["initial_distance2"].cpu() / rho2 - 1, o["distance2"].cpu() / rho2 - 1
        emit(f"{name:12s} initial_distance2 / rho^2 - 1 in [{float(e0.min()):.3e}, {float(e0.max()):.3e}]; reached distance2 / rho^2 - 1 in "
             f"[{float(e1.min()):.3e}, {float(e1.max()):.3e}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
