#!/usr/bin/env python3
"""Cost of the metric spectrum: the Jacobi launch at the head's shapes, with and without eigenvectors, and one
``MetricSpectrum.update`` against one ``MetricStatistics.update`` on the full-size C3 model.

    python tools/bench_metric_spectrum.py [--reps 20] [--evals 6] [--out profiles/metric_spectrum.txt]

Kernel: Gram matrices of seeded random panel-layout Jacobian stacks at C3 (B = 512, d = 64, D = 784) and C5 (B = 256, d = 128,
D = 3072) through ``engine.gram_cholesky(T, d, 1)``; HIP events around ``engine.gram_spectrum`` (one launch; the output
allocations are inside the bracket, served by the caching allocator after the warm-up), median of --reps.  End to end: full-size
C3 (recipe seed 0), B = 512 seeded inputs, ``MetricSpectrum.update(x)`` and ``MetricStatistics.update(x)`` (latent coordinates)
in one process, host clock around each call ending in a synchronise, alternated, medians of --evals each.  Fails without a GPU."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_spectrum.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_metric_spectrum needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# spectrum launch (cmf_gram_spectrum: float64 Jacobi, one workgroup per sample) beside the Gram + Cholesky launch "
         f"(cmf_gram_cholesky, one attempt), HIP events, median of {a.reps}")
    for label, B, d, D in (("C3", 512, 64, 784), ("C5", 256, 128, 3072)):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        jtj = E.gram_cholesky(T, d, 1).jtj
        gram = event_ms(lambda: E.gram_cholesky(T, d, 1), a.reps)
        m_gram = statistics.median(gram)
        for vectors in (False, True):
            ms = event_ms(lambda: E.gram_spectrum(jtj, vectors=vectors), a.reps)
            r = E.gram_spectrum(jtj, vectors=vectors)
            sweeps, info = r.sweeps.cpu(), r.info.cpu()
            m = statistics.median(ms)
            emit(f"{label:3s} B = {B:3d} d = {d:3d} vectors = {str(vectors):5s}: spectrum {m * 1e3:9.1f} us (min {min(ms) * 1e3:.1f}), "
                 f"sweeps {int(sweeps.min())} .. {int(sweeps.max())}, info != 0: {int((info != 0).sum())}; gram_cholesky "
                 f"{m_gram * 1e3:8.1f} us; spectrum / gram_cholesky = {m / m_gram:.2f}")
        del T

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    B = a.batch
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both calls see the same input
    runners = {"statistics": cmf_amd.MetricStatistics(model), "spectrum": cmf_amd.MetricSpectrum(model),
               "spectrum+vectors": cmf_amd.MetricSpectrum(model, vectors=True)}
    xc = x.cuda()

    def run(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runners[which].update(xc)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for which in runners:
        run(which)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which in runners:
            times[which].append(run(which))
    med = {which: statistics.median(t) for which, t in times.items()}
    emit(f"# C3 full size, B = {B}: one MetricSpectrum.update against one MetricStatistics.update (latent coordinates), host clock, "
         f"median of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:17s} {med[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"spectrum / statistics = {med['spectrum'] / med['statistics']:.3f}, with vectors {med['spectrum+vectors'] / med['statistics']:.3f}")
    r = runners["spectrum"].result()
    emit(f"# spectrum of the {r['count']} accumulated samples ({r['skipped']} skipped): mean log-volume {r['mean_log_volume']:.4f}, mean "
         f"participation ratio {r['mean_participation_ratio']:.3f}, geometric-mean eigenvalues {float(r['mean_log_eigenvalues'][0].exp()):.3e} "
         f".. {float(r['mean_log_eigenvalues'][-1].exp()):.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
