#!/usr/bin/env python3
"""Cost of the error bars of a Gauss-Newton fit: the ``engine.tangent_leverage`` launch and its covariance-only mode
at the head's shapes, beside ``engine.gauss_newton_step`` on the same inputs, and one ``ManifoldProjector.uncertainty`` against the
``project(steps=4)`` it qualifies on the full-size C3 model.

    python tools/bench_uncertainty.py [--reps 20] [--evals 6] [--out profiles/uncertainty.txt] [--launches-only]

Kernel: seeded random panel-layout Jacobian stacks at C3 (B = 512, D = 784, d = nc = 64) and C5 (B = 256, D = 3072, d = nc = 128),
their Gram matrices from ``engine.gram_cholesky(T, d, 1)``, random x and x_hat, damping 1e-3.  HIP events around one launch (the
output allocations are inside the bracket, served by the caching allocator after the warm-up), median of --reps after three warm-up
launches.  The flop and byte figures are the ones the engine's timer entry counts: per sample the elimination, the inverse of the
unit factor and cov, and per row d^2 / 2 float64 multiply-adds; J once, the triangle in, cov and lev out.  What to read off: how far
the row pass is from the float64 FMA rate, and the launch from ``gauss_newton_step``, which streams the same J and eliminates the
same matrix.  End to end: full-size C3 (recipe seed 0), B = 512 seeded inputs past the dequantisation wrapper, host clock around work
that ends in a synchronise, alternated, medians of --evals; the expectation to hold the figure against is one tangent sweep, a fifth
of ``project(steps=4)``'s five.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty.txt"))
    ap.add_argument("--launches-only", action="store_true", help="the launch table alone, nothing written: what a kernel trace runs")
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_uncertainty needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# leverage launch (cmf_tangent_leverage: cov = gram^-1 and lev_i = j_i^T cov j_i in float64, one workgroup per sample) and its "
         f"covariance-only mode, beside gauss_newton_step on the same J and Gram matrix; HIP events, median of {a.reps}")
    for label, B, d, D in (("C3", 512, 64, 784), ("C5", 256, 128, 3072)):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        x, xhat = torch.randn(B, D, generator=gen).cuda(), torch.randn(B, D, generator=gen).cuda()
        lam = torch.full((B,), 1e-3, dtype=torch.float64, device="cuda")
        jtj = E.gram_cholesky(T, d, 1).jtj
        with E.timing(lambda name: name == "tangent_leverage") as timer:
            r = E.tangent_leverage(T, jtj)
        _, _, flops, counted = timer.by_name()["tangent_leverage"]
        info = r.info.cpu()
        trace = float((r.stats[:, 0] - d).abs().max())
        full = event_ms(lambda: E.tangent_leverage(T, jtj), a.reps)
        only = event_ms(lambda: E.tangent_leverage(T, jtj, rows=False), a.reps)
        step = event_ms(lambda: E.gauss_newton_step(T, jtj, x, xhat, lam), a.reps)
        m_full, m_only, m_step = (statistics.median(v) for v in (full, only, step))
        rows_gf = B * D * (d * d + 3.0 * d) / max(m_full - m_only, 1e-6) / 1e6
        emit(f"{label:3s} B = {B:3d} D = {D:4d} d = {d:3d}: tangent_leverage {m_full * 1e3:8.1f} us (min {min(full) * 1e3:.1f}; "
             f"{flops / 1e9:.2f} GFLOP counted = {flops / m_full / 1e9:.2f} TFLOP/s float64, {counted / 1e6:.0f} MB = "
             f"{counted / m_full / 1e6:.0f} GB/s); covariance-only {m_only * 1e3:7.1f} us; the row pass alone (the difference) "
             f"{rows_gf / 1e3:.2f} TFLOP/s; gauss_newton_step {m_step * 1e3:7.1f} us (x {m_full / m_step:.2f}); info != 0: "
             f"{int((info != 0).sum())}, max |sum lev - d| {trace:.2e}")
        del T
    if a.launches_only:
        return

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
        last["project"] = proj.project(xc)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run(project)
    w = (torch.rand(xc.shape, generator=gen) > 0.5).float().cuda()

    def uncertainty():
        last["uncertainty"] = proj.uncertainty(last["project"])

    def uncertainty_weighted():
        last["weighted"] = proj.uncertainty(last["project"], weights=w)

    def uncertainty_data():
        last["data"] = proj.uncertainty(last["project"], space="data")

    runners = {"uncertainty": uncertainty, "uncertainty(weights)": uncertainty_weighted, "uncertainty(space='data')": uncertainty_data,
               "project(steps=4)": project}
    for fn in runners.values():
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    med = {which: statistics.median(t) for which, t in times.items()}
    with E.timing(lambda name: True) as timer:
        uncertainty()
    emit(f"# C3 full size, B = {B}: one uncertainty(project(x)) -- 1 tangent sweep, 1 Gram launch, 1 leverage launch -- against one "
         f"project(x, steps=4) -- 5 tangent sweeps + 5 primal decodes + 1 encode --, host clock, median of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:26s} {med[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"uncertainty / project = {med['uncertainty'] / med['project(steps=4)']:.3f}  (one sweep of five: 0.2)")
    by = timer.by_name()
    total = sum(v[1] for v in by.values())
    emit(f"# kernel families of one uncertainty call, ms by the engine's timer (sum {total:.2f}): tangent_leverage "
         f"{by['tangent_leverage'][1]:.3f}, gram_cholesky {by.get('gram_cholesky', (0, 0.0))[1]:.3f}, the sweep {total - by['tangent_leverage'][1] - by.get('gram_cholesky', (0, 0.0))[1]:.2f}")
    out = last["uncertainty"]
    lev = out["leverage"].flatten(1)
    emit(f"# that call: info != 0: {int((out['info'] != 0).sum())}, dof {int(out['dof'].min())}, max |sum lev - d| "
         f"{float((lev.sum(1) - 64).abs().max()):.2e}, reconstruction_std_head in [{float(out['reconstruction_std_head'].min()):.3e}, "
         f"{float(out['reconstruction_std_head'].max()):.3e}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
